"""Integrated Gradients against the temporal mask search on one MI355X.

    python tools/ig_bench.py [--clips 4] [--steps 32] [--iters 4] [--reps 7] [--out profiles/ig_bench.txt]

1. ms per (clip, node) row of ivf_i3d_ig (--clips clips x --steps nodes, chunks of the plan's 32 rows: stage -> forward
   -> backward -> accumulate, then finish) against ms per clip-iteration of ivf_i3d_search (32 clips, --iters
   iterations) on the same plan at S16, B = 32, the default arithmetic (bf16x6): the two alternated in the same run
   between device events, median of --reps calls each after warm-up.  Both run one network forward and backward per
   row; the difference is the staging and reduction around them.
2. Every new kernel alone at the same shape: median device-event time and the achieved GB/s against its compulsory
   bytes, beside the temporal freeze pair they stand in for.

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
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    B, N, b, K = args.batch, args.iters, args.clips, args.steps
    eng, choice = engine("s16", B)
    C, T, H, W = eng.clip_shape
    HW = H * W
    x = torch.stack([torch.from_numpy(R.clip(21 + i)) for i in range(B)]).cuda()
    tgt = eng.argmax(eng.forward(x))
    dev = torch.cuda.get_device_properties(0)
    out(f"# tools/ig_bench.py on {dev.name}, S16 B={B}, math {eng.math}, kernel choice: {choice}; IG {b} clips x {K} "
        f"nodes = {b * K} rows per call, search {N} iterations of {B} clips per call, median of {args.reps} calls "
        f"(device events), the two alternated")
    lib, st = L.lib(), L.stream

    # ---- 1. IG rows against search iterations
    _, alpha, w = eng._ig_rule(K, None, None)
    xi, ti = x[:b].contiguous(), tgt[:b].contiguous()
    ws = torch.empty(lib.ivf_ig_workspace_bytes(b, C, T, HW, K), dtype=torch.uint8, device="cuda")
    ig_map, frames, absf = torch.empty(b, T, HW, device="cuda"), torch.empty(b, T, device="cuda"), torch.empty(b, T, device="cuda")
    total, path = torch.empty(b, device="cuda"), torch.empty(b, K, device="cuda")
    raw = torch.zeros(B, T, device="cuda")

    def ig():
        L.check(lib.ivf_i3d_ig(eng._h, L.ptr(xi), b, L.ptr(ti), 0, None, 0.0, L.ptr(alpha), L.ptr(w), K, L.ptr(ig_map),
                               L.ptr(frames), L.ptr(absf), L.ptr(total), L.ptr(path), L.ptr(ws), st()))

    def search():
        raw.fill_(0.5)
        eng.search(x, tgt, raw, 0.01, 0.02, N, want_traj=False)

    for _ in range(2):
        ig()
        search()
    torch.cuda.synchronize()
    ti_, ts_ = [], []
    for _ in range(args.reps):
        ti_.append(event_ms(ig) / (b * K))
        ts_.append(event_ms(search) / (N * B))
    mi, ms = statistics.median(ti_), statistics.median(ts_)
    out(f"integrated gradients (ivf_i3d_ig):  {mi:8.4f} ms / row             (min {min(ti_):.4f}, max {max(ti_):.4f})")
    out(f"temporal search (ivf_i3d_search):   {ms:8.4f} ms / clip-iteration  (min {min(ts_):.4f}, max {max(ts_):.4f})")
    out(f"an IG row against a search clip-iteration: {mi - ms:+.4f} ms = {100 * (mi - ms) / ms:+.2f} %")
    out(f"one clip at K = {K}: {mi * K:.2f} ms; ig_total {total.tolist()}, "
        f"path scores of clip 0 from {float(path[0, 0]):.4f} to {float(path[0, -1]):.4f}")

    # ---- 2. the kernels alone, one 32-row chunk (the rows of one clip when K = 32)
    rows = min(B, b * K)
    P = torch.empty(rows, T, HW, 4, device="cuda")
    g = torch.randn(rows, T, HW, 4, device="cuda")
    Gsum = torch.zeros(b, C, T, HW, device="cuda")
    mrows = torch.rand(B, T, device="cuda")
    fws = torch.empty(lib.ivf_freeze_bwd_workspace_bytes(B, T), dtype=torch.uint8, device="cuda")
    dmask = torch.empty(B, T, device="cuda")
    Pb, gb = torch.empty(B, T, HW, 4, device="cuda"), torch.randn(B, T, HW, 4, device="cuda")
    clip_b = C * T * HW * 4
    nclips = (rows + K - 1) // K
    kernels = [
        (f"ivf_ig_stage ({rows} rows, 16-byte pixels)", nclips * clip_b + P.numel() * 4,
         lambda: lib.ivf_ig_stage(L.ptr(xi), 0, None, 0.0, L.ptr(alpha), b, C, T, HW, K, 0, rows, L.ptr(P), 4, st())),
        (f"ivf_ig_accumulate ({rows} rows)", g.numel() * 4 + 2 * nclips * clip_b,
         lambda: lib.ivf_ig_accumulate(L.ptr(g), 4, L.ptr(w), K, 0, rows, L.ptr(Gsum), b, C, T, HW, st())),
        (f"ivf_ig_finish ({b} clips, once per call)", b * (2 * clip_b + T * HW * 4),
         lambda: lib.ivf_ig_finish(L.ptr(xi), 0, None, 0.0, L.ptr(Gsum), b, C, T, HW, L.ptr(ig_map), L.ptr(frames), L.ptr(absf),
                                   L.ptr(total), st())),
        (f"ivf_freeze_fwd ({B} clips, for comparison)", x.numel() * 4 + Pb.numel() * 4,
         lambda: lib.ivf_freeze_fwd(L.ptr(x), L.ptr(mrows), L.ptr(Pb), B, C, T, HW, 1, 4, st())),
        (f"ivf_freeze_bwd ({B} clips, for comparison)", x.numel() * 4 + gb.numel() * 4,
         lambda: lib.ivf_freeze_bwd(L.ptr(x), L.ptr(mrows), L.ptr(gb), L.ptr(dmask), None, B, C, T, HW, 1, 4, L.ptr(fws), st())),
    ]
    out("kernels alone, launched back to back on the same buffers (compulsory bytes: what each must read and write once):")
    t_new = t_old = 0.0
    for name, nbytes, fn in kernels:
        L.check(fn())
        t = median_ms(fn, 4 * args.reps)
        if "comparison" in name:
            t_old += t
        elif "finish" not in name:
            t_new += t
        out(f"{name:48s} {t * 1e3:9.1f} us  {nbytes / 2**20:8.1f} MiB compulsory  {nbytes / t / 1e6:8.1f} GB/s")
    out(f"stage + accumulate of a {rows}-row chunk {t_new:.3f} ms; the temporal freeze pair of {B} clips {t_old:.3f} ms; "
        f"difference {1e3 * (t_new - t_old) / rows:+.2f} us per row = {100 * (t_new - t_old) / rows / ms:+.2f} % of a search "
        f"clip-iteration")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
