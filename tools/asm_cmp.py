"""Per-kernel comparison of two device-only assembly dumps of the same unit (a refactor's parent against the change).

    hipcc <the Makefile's FLAGS> --cuda-device-only -S dl_ofdm_amd/csrc/dccn_abi.hip -o /tmp/a.s      (once per tree and unit)
    python tools/asm_cmp.py /tmp/a.s /tmp/b.s [--show <symbol substring>]

Per kernel symbol: the instruction stream (comments, labels and directives stripped, branch targets replaced by the ordinal of
the label inside the kernel), its opcode histogram, and the resource numbers of the kernel's info block and metadata (VGPR,
AGPR, SGPR, LDS, scratch, spills, occupancy).  Prints one line per kernel that is not identical and the totals; exit status 1
when a kernel's histogram or resources differ (a reordered stream alone is status 0).  --show prints the unified diff of the
streams of the kernels whose name contains the substring.
"""
import collections
import difflib
import re
import sys

INFO = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")
META = (".sgpr_spill_count", ".vgpr_spill_count")


def kernels(path):
    src = open(path).read().split("\n")
    names = [l.split()[1] for l in src if l.strip().startswith(".amdhsa_kernel ")]
    start = {l.split(":")[0]: i for i, l in enumerate(src) if l[:1] not in ("", "\t", " ", ".", ";") and ":" in l}
    out = {}
    for name in names:
        i = start[name] + 1
        body, labels = [], {}
        while not src[i].startswith(".Lfunc_end"):
            s = src[i].split(";")[0].strip()
            i += 1
            if s.endswith(":"):
                labels[s[:-1]] = "L%d" % len(labels)
            elif s and not s.startswith("."):
                body.append(" ".join(s.split()))
        body = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.get(m.group(0), m.group(0)), l) for l in body]
        res = {}
        while i < len(src) and not src[i].startswith("; Kernel info:"):
            i += 1
        for l in src[i:i + 30]:
            m = re.match(r"; (\w+): (\d+)", l)
            if m and m.group(1) in INFO:
                res[m.group(1)] = int(m.group(2))
        out[name] = [body, res]
    cur = None
    for l in src:                               # metadata: spill counts, keyed by .name
        t = l.strip()
        if t.startswith(".name:") and t.split()[-1] in out:
            cur = t.split()[-1]
        elif cur and t.split(":")[0] in META:
            out[cur][1][t.split(":")[0]] = int(t.split()[-1])
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    show = sys.argv[sys.argv.index("--show") + 1] if "--show" in sys.argv else None
    same = reordered = differ = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("ONLY IN %s: %s" % ("A" if name in a else "B", name))
            differ += 1
            continue
        (ba, ra), (bb, rb) = a[name], b[name]
        if ba == bb and ra == rb:
            same += 1
            continue
        ha, hb = collections.Counter(l.split()[0] for l in ba), collections.Counter(l.split()[0] for l in bb)
        dh = {k: hb[k] - ha[k] for k in sorted(set(ha) | set(hb)) if ha[k] != hb[k]}
        dr = {k: (ra.get(k), rb.get(k)) for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)}
        nd = sum(1 for l in difflib.unified_diff(ba, bb, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
        kind = "REORDERED" if not dh and not dr else "DIFFERENT"
        reordered += kind == "REORDERED"
        differ += kind == "DIFFERENT"
        print("%s %s: %d -> %d instructions, %d diff lines%s%s" % (
            kind, name, len(ba), len(bb), nd, ", opcodes %s" % dh if dh else "", ", resources %s" % dr if dr else ""))
        if kind == "REORDERED":
            print("    resources %s" % ra)
        if show and show in name:
            print("\n".join(difflib.unified_diff(ba, bb, lineterm="", n=2)))
    print("%d kernels: %d identical, %d reordered (same opcode histogram and resources), %d different" % (
        same + reordered + differ, same, reordered, differ))
    sys.exit(1 if differ else 0)


main()
