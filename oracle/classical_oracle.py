"""CPU oracle of the four device stages of the classical pilot-aided receivers.

TEST INFRASTRUCTURE ONLY -- same import rule as oracle/dccn_oracle.py: nothing under dl_ofdm_amd/ may import this
file; it is the checker of tests/, never the product.

A float64 NumPy restatement of dccn_classical_pilot_ls / _gain / _estimate / _detect, written from their contract in
include/dccn.h ("classical pilot-aided receivers"), at any geometry: nothing here knows the product's S = 7, K = 64.
What pins it: tests/test_classical_oracle.py holds it to dl_ofdm_amd.benchmark.ClassicalReceiver, the whole-receiver
restatement of the same estimators, at the product geometry.

Conventions: frames Y and responses H are complex arrays [n, S*K] (flat cell index = symbol*K + carrier); "planes" are
real arrays with a leading axis of 2 (0 = real parts, 1 = imaginary parts), the layout the interpolation GEMM consumes
and produces.
"""
from __future__ import annotations

import numpy as np

LS, LMMSE, ALMMSE, PERFECT, FRAME_MEAN = 0, 1, 2, 3, 4


def _c128(a):
    return np.asarray(a, dtype=np.complex128)


def from_planes(planes):
    """[2, ...] real planes -> complex [...]"""
    p = np.asarray(planes, dtype=np.float64)
    return p[0] + 1j * p[1]


def to_planes(z):
    """complex [...] -> [2, ...] real planes"""
    z = _c128(z)
    return np.stack([z.real, z.imag], 0)


def pilot_ls(Y, pil, pv):
    """LS at the pilots: planes [2, n, P] of Y[:, pil] / pv.  Y [n, SK] complex, pil [P] flat cell indices (any order)."""
    return to_planes(_c128(Y)[:, np.asarray(pil, dtype=np.int64)] / complex(pv))


def gain_sums(Y, H, Gls, pil, pv):
    """(sums [4], scales [4]) of dccn_classical_gain: sums = {Re, Im of sum Y_p conj(H_p pv), sum |H_p pv|^2 over every
    frame's pilots, sum |G_ls|^2 over every cell}; scales[k] = the L1 norm, sum |term|, of the terms sums[k] adds (what a
    rounding bound on the sum is relative to).  Gls: planes [2, n, SK].  H None: the first three sums are 0."""
    g = np.asarray(Gls, dtype=np.float64)
    t3 = g[0] ** 2 + g[1] ** 2
    sums, scales = np.zeros(4), np.zeros(4)
    sums[3] = scales[3] = t3.sum()
    if H is not None:
        pil = np.asarray(pil, dtype=np.int64)
        hp = _c128(H)[:, pil] * complex(pv)
        t = _c128(Y)[:, pil] * np.conj(hp)
        t2 = np.abs(hp) ** 2
        sums[:3] = t.real.sum(), t.imag.sum(), t2.sum()
        scales[:3] = np.abs(t.real).sum(), np.abs(t.imag).sum(), t2.sum()
    return sums, scales


def gain_scalar(sums):
    """the complex a that maps the unit-gain response onto the frames: (sums[0] + i sums[1]) / sums[2]"""
    return complex(sums[0], sums[1]) / sums[2]


def estimate(Gls_planes, H, mode, c, a=1.0):
    """dccn_classical_estimate.  Gls_planes [2, n, S, K], H [n, S, K] complex or None, c = LS error variance at a pilot,
    a = gain_scalar of the batch (modes 1 and 3).  Returns G [n, S*K] complex; mode 4: the frame mean V [n, K].
      0 LS            G = G_ls
      1 ideal LMMSE   per symbol, rank-one Rhh = h h^H with h = H a:  G = h <h, g_ls> / (|h|^2 + c)
      2 ALMMSE        v = mean over the symbols of g_ls, e = sum_k |v|^2 / S:  every symbol's row = v e / (e + c)
      3 Perfect       G = H a
      4 frame mean    V = v"""
    g = from_planes(Gls_planes)
    if g.ndim != 3:
        raise ValueError("Gls_planes must be [2, n, S, K]")
    n, S, K = g.shape
    if mode == LS:
        return g.reshape(n, S * K)
    if mode in (LMMSE, PERFECT):
        if H is None:
            raise ValueError("modes 1 and 3 need the true response H")
        h = _c128(H).reshape(n, S, K) * complex(a)
        if mode == PERFECT:
            return h.reshape(n, S * K)
        proj = (np.conj(h) * g).sum(-1, keepdims=True) / ((np.abs(h) ** 2).sum(-1, keepdims=True) + c)
        return (h * proj).reshape(n, S * K)
    if mode in (ALMMSE, FRAME_MEAN):
        v = g.mean(axis=1)
        if mode == FRAME_MEAN:
            return v
        e = (np.abs(v) ** 2).sum(-1, keepdims=True) / S
        return np.repeat((v * (e / (e + c)))[:, None, :], S, axis=1).reshape(n, S * K)
    raise ValueError("mode must be 0 ... 4")


def lmmse_weights(H, c, a):
    """[n, S] |h|^2 / (|h|^2 + c) of mode 1 (what the noise term c does to the projection); H [n, S, K]"""
    e = (np.abs(_c128(H) * complex(a)) ** 2).sum(-1)
    return e / (e + c)


def almmse_weights(Gls_planes, c):
    """[n] e / (e + c) of mode 2"""
    g = from_planes(Gls_planes)                             # [n, S, K]
    e = (np.abs(g.mean(axis=1)) ** 2).sum(-1) / g.shape[1]
    return e / (e + c)


def nearest(Y, G, dat, table, g_row, g_mod):
    """(idx [n, D], margin [n, D]): x = Y / G at the data cells; idx = the FIRST minimum over table [m] of the squared
    distance |x - table[q]|^2 (np.argmin); margin = distance to the second nearest point minus distance to the nearest
    (how far the cell is from a tie; 0 for a table of one point).  A few frames at a time: [n, D, m] need not fit."""
    Y, table = _c128(Y), _c128(table)
    n, m = Y.shape[0], table.shape[0]
    dat = np.asarray(dat, dtype=np.int64)
    Gr = _c128(G).reshape(n, int(g_row))
    x = Y[:, dat] / Gr[:, dat % int(g_mod) if g_mod > 0 else dat]
    idx = np.empty(x.shape, dtype=np.int64)
    margin = np.zeros(x.shape)
    step = max(1, (1 << 21) // (x.shape[1] * m))
    for f in range(0, n, step):
        d = x[f:f + step, :, None] - table[None, None, :]
        d2 = d.real ** 2 + d.imag ** 2
        idx[f:f + step] = np.argmin(d2, axis=-1)
        if m > 1:
            two = np.sqrt(np.partition(d2, 1, axis=-1)[..., :2])
            margin[f:f + step] = two[..., 1] - two[..., 0]
    return idx, margin


def detect(Y, G, dat, table, labels, bits, g_row, g_mod):
    """dccn_classical_detect: x = Y / G at the data cells dat [D] (any order), nearest point of table [m] (the first
    minimum, like np.argmin), det [n, D, nbits] = labels [m, nbits] of that point, errors = how many of them differ from
    bits [n, D, nbits].  G: g_row cells per frame; the cell index is taken modulo g_mod when g_mod > 0 (one estimate row
    [K] per frame).  Returns (det, errors)."""
    det = np.asarray(labels, dtype=np.int32)[nearest(Y, G, dat, table, g_row, g_mod)[0]]
    return det, int(np.count_nonzero(det != np.asarray(bits).reshape(det.shape)))


def decision_margin(Y, G, dat, table, g_row, g_mod):
    return nearest(Y, G, dat, table, g_row, g_mod)[1]
