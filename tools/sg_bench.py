"""SmoothGrad / SmoothGrad^2 / VarGrad against Integrated Gradients on one MI355X.

    python tools/sg_bench.py [--clips 4] [--samples 32] [--reps 7] [--out profiles/smoothgrad_bench.txt]

1. ms per (clip, sample) row of ivf_i3d_smoothgrad against ms per (clip, node) row of ivf_i3d_ig (--clips clips x
   --samples samples / nodes each, chunks of the plan's 32 rows) on the same plan at S16, B = 32, the default arithmetic
   (bf16x6): the two alternated in the same run between device events, median of --reps calls each after warm-up, with
   min and max.  Both run one network forward and backward per row; the difference is the staging (noise against a
   path point) and the reduction (two moments against one weighted sum) around them.
2. Every new kernel alone at the same shape: median device-event time and the achieved TB/s against its compulsory
   bytes, beside the IG kernels they stand in for.

Kernel choice: the committed headline choice (profiles/r03_bench_tuning.json) where it fits the plan, else the built-in
one; never autotuned, so both sides run the same network kernels.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "interpreting-video-features_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import ivf_lib as L  # noqa: E402
import ivf_recipe as R  # noqa: E402
from blob_bench import engine, event_ms, median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--level", type=float, default=0.15)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    B, b, n = args.batch, args.clips, args.samples
    eng, choice = engine("s16", B)
    C, T, H, W = eng.clip_shape
    HW = H * W
    x = torch.stack([torch.from_numpy(R.clip(21 + i)) for i in range(b)]).cuda()
    tgt = torch.cat([eng.argmax(eng.forward(x[i:i + B])) for i in range(0, b, B)])
    dev = torch.cuda.get_device_properties(0)
    out(f"# tools/sg_bench.py on {dev.name}, S16 B={B}, math {eng.math}, kernel choice: {choice}; {b} clips x {n} samples "
        f"(SmoothGrad, level {args.level}) or nodes (IG) = {b * n} rows per call, median of {args.reps} calls (device "
        f"events), the two alternated")
    lib, st = L.lib(), L.stream

    # ---- 1. SmoothGrad rows against IG rows
    _, alpha, w = eng._ig_rule(n, None, None)
    ws_ig = torch.empty(lib.ivf_ig_workspace_bytes(b, C, T, HW, n), dtype=torch.uint8, device="cuda")
    ws_sg = torch.empty(lib.ivf_sg_workspace_bytes(b, C, T, HW, n), dtype=torch.uint8, device="cuda")
    maps = [torch.empty(b, T, HW, device="cuda") for _ in range(3)]
    frames = [torch.empty(b, T, device="cuda") for _ in range(3)]
    total, scores, sigma = torch.empty(b, device="cuda"), torch.empty(b, n, device="cuda"), torch.empty(b, device="cuda")

    def sg():
        L.check(lib.ivf_i3d_smoothgrad(eng._h, L.ptr(x), b, L.ptr(tgt), n, args.level, 0, *[L.ptr(t) for t in maps + frames],
                                       L.ptr(scores), L.ptr(sigma), L.ptr(ws_sg), st()))

    def ig():
        L.check(lib.ivf_i3d_ig(eng._h, L.ptr(x), b, L.ptr(tgt), 0, None, 0.0, L.ptr(alpha), L.ptr(w), n, L.ptr(maps[0]),
                               L.ptr(frames[0]), L.ptr(frames[1]), L.ptr(total), L.ptr(scores), L.ptr(ws_ig), st()))

    for _ in range(2):
        sg()
        ig()
    torch.cuda.synchronize()
    ts_, ti_ = [], []
    for _ in range(args.reps):
        ts_.append(event_ms(sg) / (b * n))
        ti_.append(event_ms(ig) / (b * n))
    ms, mi = statistics.median(ts_), statistics.median(ti_)
    out(f"smoothgrad (ivf_i3d_smoothgrad):    {ms:8.4f} ms / row  (min {min(ts_):.4f}, max {max(ts_):.4f})")
    out(f"integrated gradients (ivf_i3d_ig):  {mi:8.4f} ms / row  (min {min(ti_):.4f}, max {max(ti_):.4f})")
    out(f"a smoothgrad row against an IG row: {ms - mi:+.4f} ms = {100 * (ms - mi) / mi:+.2f} %")
    sg()
    out(f"one clip at n = {n}: {ms * n:.2f} ms; sigma {sigma.tolist()}; sum var (n - 1) / sum G2 of clip 0 = "
        f"{float(frames[2][0].double().sum() * (n - 1) / (frames[1][0].double().sum() * n)):.4f}")

    # ---- 2. the kernels alone, one 32-row chunk (the rows of one clip when n = 32)
    rows = min(B, b * n)
    P = torch.empty(rows, T, HW, 4, device="cuda")
    g = torch.randn(rows, T, HW, 4, device="cuda")
    G1, G2 = torch.zeros(b, C, T, HW, device="cuda"), torch.zeros(b, C, T, HW, device="cuda")
    clip_b = C * T * HW * 4
    nclips = (rows + n - 1) // n
    L.check(lib.ivf_sg_range(L.ptr(x), b, C, T, HW, args.level, L.ptr(sigma), st()))
    kernels = [
        (f"ivf_sg_stage ({rows} rows, 16-byte pixels)", nclips * clip_b + P.numel() * 4,
         lambda: lib.ivf_sg_stage(L.ptr(x), L.ptr(sigma), b, C, T, HW, n, 0, 0, rows, L.ptr(P), 4, st())),
        (f"ivf_sg_accumulate ({rows} rows)", g.numel() * 4 + 4 * nclips * clip_b,
         lambda: lib.ivf_sg_accumulate(L.ptr(g), 4, n, 0, rows, L.ptr(G1), L.ptr(G2), b, C, T, HW, st())),
        (f"ivf_sg_finish ({b} clips, once per call)", b * (2 * clip_b + 3 * T * HW * 4),
         lambda: lib.ivf_sg_finish(L.ptr(G1), L.ptr(G2), n, b, C, T, HW, *[L.ptr(t) for t in maps + frames], st())),
        (f"ivf_sg_range ({b} clips, once per call)", b * clip_b,
         lambda: lib.ivf_sg_range(L.ptr(x), b, C, T, HW, args.level, L.ptr(sigma), st())),
        (f"ivf_ig_stage ({rows} rows, for comparison)", nclips * clip_b + P.numel() * 4,
         lambda: lib.ivf_ig_stage(L.ptr(x), 0, None, 0.0, L.ptr(alpha), b, C, T, HW, n, 0, rows, L.ptr(P), 4, st())),
        (f"ivf_ig_accumulate ({rows} rows, for comparison)", g.numel() * 4 + 2 * nclips * clip_b,
         lambda: lib.ivf_ig_accumulate(L.ptr(g), 4, L.ptr(w), n, 0, rows, L.ptr(G1), b, C, T, HW, st())),
    ]
    out("kernels alone, launched back to back on the same buffers (compulsory bytes: what each must read and write once):")
    t_new = t_old = 0.0
    for name, nbytes, fn in kernels:
        L.check(fn())
        t = median_ms(fn, 4 * args.reps)
        if "comparison" in name:
            t_old += t
        elif "once per call" not in name:
            t_new += t
        out(f"{name:48s} {t * 1e3:9.1f} us  {nbytes / 2**20:8.1f} MiB compulsory  {nbytes / t / 1e9:8.3f} TB/s")
    out(f"stage + accumulate of a {rows}-row chunk: smoothgrad {t_new:.3f} ms, IG {t_old:.3f} ms; difference "
        f"{1e3 * (t_new - t_old) / rows:+.2f} us per row = {100 * (t_new - t_old) / rows / mi:+.2f} % of an IG row")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
