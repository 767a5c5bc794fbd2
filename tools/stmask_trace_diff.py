#!/usr/bin/env python3
"""Where the spacetime search loop spends more time than the temporal one: two rocprofv3 kernel traces, one per loop
(each taken in a run of its own), compared iteration by iteration.

    rocprofv3 --kernel-trace -d A -o t --output-format csv -- python3 tools/stmask_bench.py --loop temporal
    rocprofv3 --kernel-trace -d B -o t --output-format csv -- python3 tools/stmask_bench.py --loop spacetime
    python tools/stmask_trace_diff.py A/**/t_kernel_trace.csv B/**/t_kernel_trace.csv [--out FILE]

An iteration runs from one launch of the loop's regulariser kernel (mask_reg_kernel / stmask_reg_kernel) to the next.
The iterations of the last calls are taken, those that span a call boundary dropped (longer than 1.5 x the median), and
per iteration: its wall time, the time some kernel is running (union of the intervals: the I3D plan runs one branch of
every Inception module on a side stream), the rest (gaps), and the kernel time by kernel family.  The difference of
the two loops is then attributed to families and to gaps.  Times under the profiler; the end-to-end figure is taken
without it (tools/stmask_bench.py).
"""
import argparse
import collections
import csv
import re
import statistics


NETWORK = ("convolutions", "max-pool", "head")


def family(name):
    k = re.sub(r"\(.*$", "", re.sub(r"^void ", "", name)).replace("ivf::", "")
    k = re.sub(r"<.*$", "", k)
    if k.startswith("conv3d") or "conv" in k and "lstm" not in k:
        return "convolutions"
    if "pool" in k:
        return "max-pool"
    if "head" in k:
        return "head"
    return k


def iterations(path, marker, keep):
    rows = list(csv.DictReader(open(path)))
    ks = sorted(((r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in rows), key=lambda t: t[1])
    starts = [i for i, k in enumerate(ks) if marker in k[0]]
    its = []
    for a, b in zip(starts[:-1], starts[1:]):
        seg = ks[a:b]
        wall = ks[b][1] - seg[0][1]
        busy, end = 0, seg[0][1]
        for _, s, e in seg:                      # union of intervals (sorted by start)
            if e > end:
                busy += e - max(s, end)
                end = e
        fam = collections.Counter()
        cnt = collections.Counter()
        for n, s, e in seg:
            fam[family(n)] += e - s
            cnt[family(n)] += 1
        net = [(re.sub(r"^void ", "", n).replace("ivf::", ""), e - s) for n, s, e in seg if family(n) in NETWORK]
        first = next((i for i, (n, _, _) in enumerate(seg) if family(n) in NETWORK), None)
        quiet = [(n, e - s) for n, s, e in seg[:first]] if first else []
        its.append((wall, busy, fam, cnt, net, quiet))
    its = its[-keep:]
    med = statistics.median(it[0] for it in its)
    return [it for it in its if it[0] < 1.5 * med]


def mean(vals):
    vals = list(vals)
    return sum(vals) / len(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("temporal")
    ap.add_argument("spacetime")
    ap.add_argument("--keep", type=int, default=30, help="iterations taken from the end of each trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s)
        lines.append(s)

    a = iterations(args.temporal, "ivf::mask_reg_kernel", args.keep)
    b = iterations(args.spacetime, "stmask_reg_kernel", args.keep)
    out(f"# tools/stmask_trace_diff.py: {len(a)} temporal and {len(b)} spacetime iterations (rocprofv3 --kernel-trace, one run per loop)")
    wa, wb = mean(i[0] for i in a), mean(i[0] for i in b)
    ba, bb = mean(i[1] for i in a), mean(i[1] for i in b)
    out(f"iteration wall:      temporal {wa / 1e6:8.3f} ms   spacetime {wb / 1e6:8.3f} ms   diff {(wb - wa) / 1e3:+8.1f} us")
    out(f"some kernel running: temporal {ba / 1e6:8.3f} ms   spacetime {bb / 1e6:8.3f} ms   diff {(bb - ba) / 1e3:+8.1f} us")
    out(f"no kernel running:   temporal {(wa - ba) / 1e3:8.1f} us   spacetime {(wb - bb) / 1e3:8.1f} us   diff {((wb - bb) - (wa - ba)) / 1e3:+8.1f} us")
    fams = sorted(set().union(*[i[2] for i in a + b]))
    rows = []
    for f in fams:
        ta, tb = mean(i[2][f] for i in a), mean(i[2][f] for i in b)
        na, nb = mean(i[3][f] for i in a), mean(i[3][f] for i in b)
        rows.append((tb - ta, f, ta, tb, na, nb))
    out("kernel time per iteration by family (sum of durations; overlapping kernels count in full), largest difference first:")
    for d, f, ta, tb, na, nb in sorted(rows, key=lambda r: -abs(r[0])):
        out(f"  {d / 1e3:+9.1f} us   {ta / 1e3:10.1f} -> {tb / 1e3:10.1f} us   launches {na:6.1f} -> {nb:6.1f}   {f[:70]}")
    out(f"  sum of the differences {sum(r[0] for r in rows) / 1e3:+.1f} us")
    # the network's launches are the same in both loops: compare them one by one, in launch order
    na, nb = [i[4] for i in a], [i[4] for i in b]
    n = len(na[0])
    if all(len(v) == n for v in na + nb) and [k for k, _ in na[0]] == [k for k, _ in nb[0]]:
        pos = []
        for k in range(n):
            ta, tb = [v[k][1] for v in na], [v[k][1] for v in nb]
            pos.append((mean(tb) - mean(ta), k, ta, tb, na[0][k][0]))
        out(f"the network's {n} launches one by one (same kernels in the same order in both loops), largest difference first:")
        for d, k, ta, tb, name in sorted(pos, key=lambda r: -abs(r[0]))[:6]:
            out(f"  {d / 1e3:+9.1f} us   launch {k:3d}   temporal {mean(ta) / 1e3:8.1f} us ({min(ta) / 1e3:.0f}..{max(ta) / 1e3:.0f})   "
                f"spacetime {mean(tb) / 1e3:8.1f} us ({min(tb) / 1e3:.0f}..{max(tb) / 1e3:.0f})   {name[:60]}")
        rest = sum(r[0] for r in pos) - sum(r[0] for r in sorted(pos, key=lambda r: -abs(r[0]))[:6])
        out(f"  the other {n - 6} launches together {rest / 1e3:+.1f} us")
        out("launch 0 (the first convolution, which reads the staged clip) iteration by iteration, us:")
        out("  temporal  " + " ".join(f"{v[0][1] / 1e3:.0f}" for v in na))
        out("  spacetime " + " ".join(f"{v[0][1] / 1e3:.0f}" for v in nb))
    for label, its_ in (("temporal", a), ("spacetime", b)):
        q = collections.Counter()
        for it in its_:
            for name, d in it[5]:
                q[re.sub(r"\(.*$", "", re.sub(r"^void ", "", name)).replace("ivf::", "")] += d / len(its_)
        out(f"{label}: kernels between the last network kernel's successor (the regulariser) and launch 0: "
            + ", ".join(f"{k[:34]} {v / 1e3:.0f} us" for k, v in q.items()))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
