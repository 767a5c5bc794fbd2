"""Exhaustive one-box search (maskType 'stcombi') throughput on one MI355X.

    python tools/box_bench.py [--reps 7] [--out profiles/box_search_bench.txt]

S16, B = 32, the default arithmetic (bf16x6), grid 7x7 with the default blur (sigma 16).

1. Candidates per second of ivf_i3d_box_scores against ivf_i3d_blob_scores (maskType 'combi', untouched by the one-box
   search: the figure of the code before it) on the same plan, the two alternated, each call between two device events,
   median and spread of --reps calls after warm-up.  Two candidate spaces: small boxes (max_len 1, max_box (1, 2):
   1,456 rows, against the full 'combi' grids of 11 clips, 1,496 rows) and every box size on one frame (max_len 1,
   max_box (7, 7): 12,544 rows, --reps // 2 calls).
2. ivf_box_stage alone against ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the same 32 rows (the explicit S of each
   candidate), alternated: the first 32 rows (unit boxes) and the last 32 rows (the largest boxes on all 16 frames) of
   the full space, max_len 16, max_box (7, 7).  Achieved GB/s against the compulsory bytes: the staged rows written once
   and the clip read once (the pair also writes and reads M and reads 32 copies of the clip).
3. ivf_box_select and ivf_box_drop on the full space of one clip (106,624 candidates).

Kernel choice: as tools/blob_bench.py (the committed headline choice where it fits the plan, never autotuned).
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
import ivf_search  # noqa: E402
from blob_bench import engine, event_ms  # noqa: E402


def spread(t):
    return f"median {statistics.median(t):9.3f} ms  (min {min(t):.3f}, max {max(t):.3f}, {len(t)} calls)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    B = args.batch
    eng, choice = engine("s16", B)
    C, T, H, W = eng.clip_shape
    HW, grid, sigma = H * W, (7, 7), None
    gh, gw = grid
    xs = torch.stack([torch.from_numpy(R.clip(21 + i)) for i in range(11)]).cuda()
    x1 = xs[:1].contiguous()
    tgt = eng.argmax(eng.forward(xs))
    dev = torch.cuda.get_device_properties(0)
    out(f"# tools/box_bench.py on {dev.name}, S16 B={B}, math {eng.math}, kernel choice: {choice}, grid {gh}x{gw}, "
        f"sigma {0.5 * H / gh:g}, device events")

    # ---- 1. candidates per second, box against blob, alternated
    n_blob = L.lib().ivf_blob_count(T, T)
    for ml, mb, reps in ((1, (1, 2), args.reps), (1, (7, 7), max(args.reps // 2, 1))):
        n_box = L.lib().ivf_box_count(T, ml, gh, gw, mb[0], mb[1])

        def box():
            return eng.box_scores(x1, tgt[:1], grid, sigma, ml, mb)

        def blob():
            return eng.blob_scores(xs, tgt, None, "freeze")

        box(), blob()
        torch.cuda.synchronize()
        tb, tc = [], []
        for _ in range(reps):
            tb.append(event_ms(box))
            tc.append(event_ms(blob))
        rb, rc = 1e3 * n_box / statistics.median(tb), 1e3 * xs.shape[0] * n_blob / statistics.median(tc)
        out(f"max_len {ml}, max_box {mb}: {n_box} candidates of one clip")
        out(f"  ivf_i3d_box_scores   {spread(tb)}  {rb:8.1f} candidates/s")
        out(f"  ivf_i3d_blob_scores  {spread(tc)}  {rc:8.1f} candidates/s  ({xs.shape[0]} clips x {n_blob})")
        out(f"  box / blob per candidate: {rc / rb:.4f} of the time of a 'combi' candidate ({100 * (rc / rb - 1):+.2f} %)")

    # ---- 2. the staging kernel alone against the pair it replaces, on the same rows
    lib = L.lib()
    _, _, _, AH, AW = eng._st_axes(grid, sigma)
    n = lib.ivf_box_count(T, T, gh, gw, gh, gw)
    tab = ivf_search.box_candidates(T, grid)
    P = torch.empty(B, T, HW, 4, device='cuda')
    P2 = torch.empty_like(P)
    M = torch.empty(B, T, H, W, device='cuda')
    xr = x1.expand(B, C, T, H, W).contiguous()
    st = L.stream
    staged = P.numel() * 4 + x1.numel() * 4
    out(f"staging alone, {B} rows of the full space ({n} candidates), compulsory bytes {staged / 2**20:.1f} MiB "
        f"(staged rows written once, the clip read once):")
    for name, first in (("first 32 rows (unit boxes, one frame)", 0), ("last 32 rows (largest boxes, 16 frames)", n - B)):
        S = ivf_search.box_masks(tab[first:first + B].cuda(), T, grid)

        def stage():
            L.check(lib.ivf_box_stage(L.ptr(x1), 1, C, T, H, W, L.ptr(AH), L.ptr(AW), gh, gw, T, gh, gw, first, B, L.ptr(P), 4, st()))

        def pair():
            L.check(lib.ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AH), L.ptr(AW), L.ptr(M), B, T, gh, gw, H, W, st()))
            L.check(lib.ivf_stfreeze_fwd(L.ptr(xr), L.ptr(M), L.ptr(P2), B, C, T, HW, 4, st()))

        for _ in range(3):
            stage(), pair()
        torch.cuda.synchronize()
        assert torch.equal(P, P2), "ivf_box_stage differs from expand_fwd + stfreeze_fwd"
        ts, tp = [], []
        for _ in range(4 * args.reps):
            ts.append(event_ms(stage))
            tp.append(event_ms(pair))
        ms, mp = statistics.median(ts), statistics.median(tp)
        out(f"  {name}")
        out(f"    ivf_box_stage                  {spread(ts)}  {staged / ms / 1e6:8.1f} GB/s of compulsory bytes")
        out(f"    expand_fwd + stfreeze_fwd      {spread(tp)}  ({mp / ms:.2f} x the time; outputs equal)")

    # ---- 3. selection and drop map on the full space of one clip
    scores = torch.rand(1, n, device='cuda')
    orig, full = torch.ones(1, device='cuda'), torch.zeros(1, device='cuda')
    for name, fn in (("ivf_box_select", lambda: ivf_search.box_select(scores, orig, full, T, grid, want_obj=True)),
                     ("ivf_box_drop", lambda: ivf_search.box_drop(scores, orig, T, grid))):
        fn()
        torch.cuda.synchronize()
        t = [event_ms(fn) for _ in range(args.reps)]
        out(f"{name:16s} on {n} candidates of one clip: {spread(t)}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
