#!/usr/bin/env python
"""Record what every public workspace-size query of libdccn.so answers -> tests/golden/workspace_sizes.json.

The fixture pins the sizes of the build it was generated from (tests/test_workspace_sizes.py holds every later build to
them), so generate it from the commit whose layouts are the reference -- point DCCN_LIB_PATH at that build's library:

    DCCN_LIB_PATH=/path/to/libdccn.so python tests/golden/make_workspace_sizes.py

Only the library is called; no device is needed (the planning assumes 256 compute units when none is visible, which is
also what an MI355X reports).  Each entry is {"query": name without the _workspace_size suffix, "args": [...], "bytes": n};
the receiver step's three queries take a shape (batch, S, kin, F, D, nbits), dccn_rx_workspace_size also `train`.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (batch, S, kin, F, D, nbits): what bench.py and the suite run ...
RX_SHAPES = ([(36, 7, 80, 64, 320, nb) for nb in (1, 2, 3, 4)] + [(73, 7, 68, 64, 320, 2), (300, 7, 64, 64, 320, 2)] +
             [(1170, 7, 80, 64, 320, nb) for nb in (1, 2, 3, 4)] +
             [(2000, 7, 80, 64, 320, 1), (48, 7, 552, 512, 2000, 2), (585, 7, 1096, 1024, 4000, 2)])
# ... and awkward ones: rows that are no multiple of 64, F = 33, few rows (<= 96), one frame, one symbol, a C-Conv output
# of one tile under more than 16 384 rows (its split plan is clamped to the slab capacity), invalid shapes (size 0)
RX_AWKWARD = [(1, 7, 80, 64, 320, 2), (37, 7, 80, 64, 320, 3), (65, 7, 80, 33, 320, 2), (96, 7, 64, 64, 320, 4),
              (97, 7, 68, 64, 320, 1), (511, 7, 80, 64, 320, 2), (769, 7, 80, 64, 320, 2), (127, 3, 20, 33, 50, 2),
              (2400, 7, 32, 32, 160, 2), (20000, 1, 16, 16, 64, 1), (130, 14, 144, 128, 600, 4), (12, 7, 64, 16, 320, 2),
              (0, 7, 80, 64, 320, 2), (36, 7, 80, 64, 320, 5), (36, 0, 80, 64, 320, 2), (36, 7, 80, 64, 320, 0),
              (-4, 7, 80, 64, 320, 2)]


def cases():
    """(query, args) pairs; the operator queries are asked at every receiver shape's own sub-problem and a few more"""
    out = []
    for sh in RX_SHAPES + RX_AWKWARD:
        b, S, kin, F, D, nb = sh
        out += [("dccn_rx", list(sh) + [0]), ("dccn_rx", list(sh) + [1]), ("dccn_rx_receive", list(sh))]
        out += [("dccn_rx_backward", [b, S, kin, F, D]),
                ("dccn_batch_moment_norm", [b, S * kin * 2]),
                ("dccn_clip_power", [b * S * kin]),
                ("dccn_dense_bwd_w", [b, S * 2 * F, 2 * D]),
                ("dccn_cconv_gemm_bwd_w", [b * S, kin, F]),
                ("dccn_cconv_patch_bwd_w", [b, S, 1, 1, 1, kin, F]),
                ("dccn_demod_tail", [b * D, nb]),
                ("dccn_dense_tail", [b, 2 * D, nb]),
                ("dccn_ingraph_awgn", [b, S * kin]),
                ("dccn_channel_awgn", [b, S * kin, 9]),
                ("dccn_channel_doppler_awgn", [b, S * kin, 9, S]),
                ("dccn_channel_groups_awgn", [b, S * kin, S]),
                ("dccn_eq_monitor", [b, S, F])]
    out += [("dccn_dense_bwd_w", a) for a in ([73, 896, 896], [73, 896, 16], [73, 16, 896], [300, 896, 640], [1170, 640, 896],
                                              [96, 640, 640], [97, 640, 640], [1, 1, 1], [5, 3, 7], [100000, 64, 64],
                                              [0, 896, 640], [73, -1, 640], [73, 896, 0])]
    out += [("dccn_cconv_gemm_bwd_w", a) for a in ([511, 80, 64], [16385, 32, 32], [40000, 32, 32], [70000, 16, 16],
                                                   [511, 80, 33], [8190, 256, 256], [8190, 257, 256], [4095, 1096, 1024],
                                                   [1, 1, 1], [0, 80, 64], [511, 0, 64], [511, 80, -2])]
    out += [("dccn_cconv_patch_bwd_w", a) for a in ([4, 28, 28, 2, 3, 3, 16], [73, 7, 64, 2, 3, 5, 32], [2, 200, 100, 1, 1, 1, 8],
                                                    [0, 28, 28, 2, 3, 3, 16], [4, 28, 28, 2, 3, 3, 0])]
    out += [("dccn_cconv_patch_bwd_x", a) for a in ([2, 3, 3, 16], [1, 1, 1, 1], [3, 5, 7, 33], [64, 3, 3, 64], [0, 3, 3, 16],
                                                    [2, 3, 3, -1])]
    out += [("dccn_cconv1d_bwd", [F]) for F in (32, 64, 33, 1, 0, -8)]
    out += [("dccn_demod_tail", a) for a in ([1, 1], [36 * 320, 2], [36 * 320, 4], [10 ** 9, 3], [0, 2], [100, 5], [100, 0])]
    out += [("dccn_dense_tail", a) for a in ([36, 640, 2], [73, 640, 2], [96, 640, 1], [97, 640, 1], [96, 648, 2], [16, 16, 4],
                                             [585, 8000, 2], [0, 640, 2], [36, 0, 2], [36, 640, 5])]
    out += [("dccn_ingraph_awgn", a) for a in ([4, 560], [4, 257], [1, 1], [129, 560], [0, 560], [4, 0])]
    out += [("dccn_classical", [])]
    out += [("dccn_channel_awgn", a) for a in ([73, 560, 9], [6, 560, 9], [1, 1, 1], [6, 257, 64], [0, 560, 9], [6, 0, 9],
                                               [6, 560, 0])]
    out += [("dccn_channel_doppler_awgn", a) for a in ([6, 560, 9, 7], [1, 1, 1, 1], [6, 560, 9, 0])]
    out += [("dccn_channel_groups_awgn", a) for a in ([6, 560, 7], [1, 1, 1], [6, 560, 0])]
    out += [("dccn_eq_monitor", a) for a in ([73, 7, 64], [1, 1, 1], [1170, 7, 64], [0, 7, 64], [73, 0, 64], [73, 7, 0])]
    out += [("dccn_batch_moment_norm", a) for a in ([4, 1120], [257, 1118], [1, 1], [1025, 1120], [0, 1120], [4, 0])]
    out += [("dccn_clip_power", a) for a in ([1], [2240], [10 ** 10])]
    seen, uniq = set(), []
    for q, a in out:
        if (q, tuple(a)) not in seen:
            seen.add((q, tuple(a)))
            uniq.append((q, a))
    return uniq


def ask(lib, query, args):
    """the library's answer to one case (used by the generator and by the test)"""
    from dl_ofdm_amd import _lib
    if query in ("dccn_rx", "dccn_rx_receive"):
        sh = _lib.RxShape(*args[:6])
        if query == "dccn_rx":
            return int(lib.dccn_rx_workspace_size(C.byref(sh), args[6]))
        return int(lib.dccn_rx_receive_workspace_size(C.byref(sh)))
    return int(getattr(lib, query + "_workspace_size")(*args))


def main():
    from dl_ofdm_amd import _lib
    lib = _lib.load()
    rows = [{"query": q, "args": a, "bytes": ask(lib, q, a)} for q, a in cases()]
    path = os.path.join(HERE, "workspace_sizes.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d cases from build %s -> %s" % (len(rows), lib.dccn_build_id().decode(), path))


if __name__ == "__main__":
    main()
