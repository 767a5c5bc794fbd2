#!/usr/bin/env python3
"""HBM bytes per launch from two rocprofv3 --pmc passes (dev tool).

    rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d A -- python3 bench.py --full ...
    rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d B -- python3 bench.py --full ...
    python tools/pmc_traffic.py A B <batch> out.json

    python tools/pmc_traffic.py A B <batch> out.json [bench_line.json] [math] [frames]

bytes = (2*FETCH_SIZE + WRITE_SIZE) * 1024: FETCH_SIZE is doubled per MI355X_MICROARCH.md (HBM
section: gfx950 counts 128-byte requests as 64).  Only the launches of the search iterations
(first mask_reg_kernel .. last search_step_kernel) are counted -- the launch mix bench.py's
roofline samples.  With the JSON line bench.py printed in one of the passes, the dominant
kernel's entry also records its algorithmic GFLOP per launch: bench.py only quotes `traffic` for
a run whose dominant kernel has the same figure (same template on the same layers).
"""
import csv, glob, json, os, re, sys
from collections import defaultdict


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*$", "", name)
    name = name.replace("ivf::", "").replace("(anonymous namespace)::", "")
    return re.sub(r"\s+", "", name)


def per_kernel(folder, counter):
    f = glob.glob(os.path.join(folder, "**", "*counter_collection.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(f)) if r["Counter_Name"] == counter]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    start = next(i for i, r in enumerate(rows) if "mask_reg_kernel" in r["Kernel_Name"])
    stop = max(i for i, r in enumerate(rows) if "search_step_kernel" in r["Kernel_Name"])
    acc = defaultdict(lambda: [0.0, 0])
    for r in rows[start:stop + 1]:      # the search iterations only: the launch mix bench.py samples
        k = short(r["Kernel_Name"])
        acc[k][0] += float(r["Counter_Value"])
        acc[k][1] += 1
    return acc


def stem_backward(folder, counter):
    """The stem's backward-data launches: in every search iteration the LAST conv3d_* dispatch before the
    freeze backward (the plan's backward runs the ops in reverse; Conv3d_1a_7x7 is the first op)."""
    f = glob.glob(os.path.join(folder, "**", "*counter_collection.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(f)) if r["Counter_Name"] == counter]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    tot, n, kern, last = 0.0, 0, None, None
    for r in rows:
        k = short(r["Kernel_Name"])
        if k.startswith("conv3d_"):
            last = r
        elif k.startswith("freeze_bwd") and last is not None:
            tot += float(last["Counter_Value"])
            n += 1
            kern = short(last["Kernel_Name"])
            last = None
    return tot / max(n, 1), n, kern


def stem_forward(folder, counter):
    """The stem's forward launches of the search iterations: the FIRST conv3d_* dispatch after each freeze_fwd* /
    reverse_fwd* dispatch (Conv3d_1a_7x7 is the first op of the plan)."""
    f = glob.glob(os.path.join(folder, "**", "*counter_collection.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(f)) if r["Counter_Name"] == counter]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    tot, n, kern, armed = 0.0, 0, None, False
    for r in rows:
        k = short(r["Kernel_Name"])
        if k.startswith("freeze_fwd") or k.startswith("reverse_fwd"):
            armed = True
        elif k.startswith("conv3d_") and armed:
            tot += float(r["Counter_Value"])
            n += 1
            kern = k
            armed = False
    return tot / max(n, 1), n, kern


def main():
    fa, fb, batch, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    bench_line = sys.argv[5] if len(sys.argv) > 5 else None
    math = sys.argv[6] if len(sys.argv) > 6 else "bf16x6"
    frames = int(sys.argv[7]) if len(sys.argv) > 7 else 16
    fetch, write = per_kernel(fa, "FETCH_SIZE"), per_kernel(fb, "WRITE_SIZE")
    kernels = {}
    for k in fetch:
        if k not in write:
            continue
        # the tuner may give a small layer to a different variant in the two passes: per-pass averages,
        # flagged when the launch counts (hence the layer mix) differ
        nf, nw = fetch[k][1], write[k][1]
        fkb, wkb = fetch[k][0] / nf, write[k][0] / nw
        kernels[k] = {"launches": nf, "hbm_bytes_per_launch": int((2 * fkb + wkb) * 1024),
                      "fetch_kb_raw_per_launch": int(fkb), "write_kb_per_launch": int(wkb)}
        if nf != nw:
            kernels[k]["launches_write_pass"] = nw
    if bench_line:
        txt = [ln for ln in open(bench_line) if ln.startswith("{")][-1]
        roof = json.loads(txt)["roofline"]
        kn = re.sub(r"\s+", "", roof["kernel"])
        if kn in kernels:
            kernels[kn]["algorithmic_gflop_per_launch"] = roof["algorithmic_gflop_per_launch"]
    total = sum(v["hbm_bytes_per_launch"] * v["launches"] for v in kernels.values())
    sites = {}
    fkb, nf, kf = stem_backward(fa, "FETCH_SIZE")
    wkb, nw, kw = stem_backward(fb, "WRITE_SIZE")
    if nf and nw and kf == kw:
        sites["Conv3d_1a_7x7 backward-data"] = {
            "kernel": kf, "launches": nf, "hbm_bytes_per_launch": int((2 * fkb + wkb) * 1024),
            "fetch_kb_raw_per_launch": int(fkb), "write_kb_per_launch": int(wkb),
            "found_as": "last conv3d_* dispatch before each freeze_bwd* dispatch"}
    fkb, nf, kf = stem_forward(fa, "FETCH_SIZE")
    wkb, nw, kw = stem_forward(fb, "WRITE_SIZE")
    if nf and nw and kf == kw:
        sites["Conv3d_1a_7x7 forward"] = {
            "kernel": kf, "launches": nf, "hbm_bytes_per_launch": int((2 * fkb + wkb) * 1024),
            "fetch_kb_raw_per_launch": int(fkb), "write_kb_per_launch": int(wkb),
            "found_as": "first conv3d_* dispatch after each freeze_fwd* / reverse_fwd* dispatch"}
    doc = {"sites": sites, "math": math, "frames": frames,
           "how": "rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in two separate passes of the same short bench.py "
                  "command; launches from the first search iteration on (after autotune); "
                  "bytes = (2*FETCH_SIZE + WRITE_SIZE)*1024, FETCH_SIZE doubled per MI355X_MICROARCH.md section HBM "
                  "(gfx950 counts 128-B requests at 64 B)",
           "batch": batch, "total_hbm_bytes_counted": total,
           "kernels": dict(sorted(kernels.items(), key=lambda kv: -kv[1]["hbm_bytes_per_launch"] * kv[1]["launches"]))}
    json.dump(doc, open(out, "w"), indent=1)
    for k, v in list(doc["kernels"].items())[:12]:
        print(f"{v['hbm_bytes_per_launch']/1e6:10.1f} MB/launch x{v['launches']:5d}  {k}")


if __name__ == "__main__":
    main()
