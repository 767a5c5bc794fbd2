"""RISE random-mask saliency throughput on one MI355X.

    python tools/rise_bench.py [--reps 7] [--out profiles/rise_bench.txt]

S16, B = 32, the default arithmetic (bf16x6), grid (8, 7, 7) with the default blur (sigma 16), p = 0.5.

1. Rows per second of ivf_i3d_rise_scores beside ivf_i3d_box_scores (maskType 'stcombi', untouched by RISE: the
   yardstick) on the same plan, the two alternated, each call between two device events, median and spread of --reps
   calls after warm-up.  Both are one forward per row: 1,456 masks of one clip against the 1,456 small boxes (max_len 1,
   max_box (1, 2)) of tools/box_bench.py.  A third series runs the same RISE entry at p = 2^-18, where almost every row is
   the clip itself, as a small box on one frame nearly leaves it: the same kernels on the data of the yardstick.
2. ivf_rise_stage alone on 32 rows, beside ivf_box_stage on 32 rows of the same geometry (the largest boxes of the full
   one-box space, 16 frames) and ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit masks of the RISE rows, the
   three alternated.  Achieved GB/s against the compulsory bytes: the staged rows written once and the clip read once.
   The staging time against the forward time of a 32-row chunk (from 1.): the feature's cost is meant to be n forwards.
3. One rise() call at n = 2048 masks on one clip, everything included (the clip's own forward, scores, reduction,
   expansion to the map), and ivf_rise_reduce alone on its scores.

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

import ivf_engine  # noqa: E402
import ivf_lib as L  # noqa: E402
import ivf_recipe as R  # noqa: E402
from blob_bench import engine, event_ms  # noqa: E402
from box_bench import spread  # noqa: E402


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
    HW, grid, sigma, p, seed = H * W, (8, 7, 7), None, 0.5, 0
    gt, gh, gw = grid
    x1 = torch.from_numpy(R.clip(21))[None].cuda()
    tgt = eng.argmax(eng.forward(x1))
    dev = torch.cuda.get_device_properties(0)
    out(f"# tools/rise_bench.py on {dev.name}, S16 B={B}, math {eng.math}, kernel choice: {choice}, grid {gt}x{gh}x{gw}, "
        f"sigma {0.5 * H / gh:g}, p {p}, device events")

    # ---- 1. rows per second, RISE beside the one-box search, alternated
    lib = L.lib()
    ml, mb = 1, (1, 2)
    n = lib.ivf_box_count(T, ml, gh, gw, mb[0], mb[1])

    def rise():
        return eng.rise_scores(x1, tgt, n, p, grid, sigma, seed)

    def rise_thin():          # the same entry and kernels on nearly unperturbed rows (2 of 1000 masks freeze any cell at all)
        return eng.rise_scores(x1, tgt, n, 2.0 ** -18, grid, sigma, seed)

    def box():
        return eng.box_scores(x1, tgt, (gh, gw), sigma, ml, mb)

    rise(), rise_thin(), box()
    torch.cuda.synchronize()
    tr, tt, tb = [], [], []
    for _ in range(args.reps):
        tr.append(event_ms(rise))
        tt.append(event_ms(rise_thin))
        tb.append(event_ms(box))
    rr, rb = 1e3 * n / statistics.median(tr), 1e3 * n / statistics.median(tb)
    out(f"{n} rows of one clip, one forward per row:")
    out(f"  ivf_i3d_rise_scores  {spread(tr)}  {rr:8.1f} rows/s")
    out(f"  ivf_i3d_box_scores   {spread(tb)}  {rb:8.1f} rows/s  (max_len {ml}, max_box {mb})")
    out(f"  rise / box per row: {rb / rr:.4f} of the time of a 'stcombi' candidate ({100 * (rb / rr - 1):+.2f} %)")
    rt = 1e3 * n / statistics.median(tt)
    out(f"  ivf_i3d_rise_scores at p = 2^-18 (rows nearly the clip itself, as the small boxes leave it): {spread(tt)}  "
        f"{rt:8.1f} rows/s, {rb / rt:.4f} of the time of a 'stcombi' candidate ({100 * (rb / rt - 1):+.2f} %)")
    chunk_ms = statistics.median(tb) * B / n

    # ---- 2. the staging kernel alone, beside the box staging and the kernel pair
    _, _, _, AH, AW = eng._st_axes((gh, gw), sigma)
    thresh = ivf_engine.rise_thresh(p)
    nbox = lib.ivf_box_count(T, T, gh, gw, gh, gw)
    P = torch.empty(B, T, HW, 4, device='cuda')
    P2 = torch.empty_like(P)
    P3 = torch.empty_like(P)
    M = torch.empty(B, T, H, W, device='cuda')
    xr = x1.expand(B, C, T, H, W).contiguous()
    kt = (torch.arange(T, device='cuda') * gt) // T
    S = eng.rise_masks(B, p, grid, seed)[:, kt].contiguous()              # [B,T,gh,gw], the rows' explicit masks
    st = L.stream
    staged = P.numel() * 4 + x1.numel() * 4

    def stage():
        L.check(lib.ivf_rise_stage(L.ptr(x1), 1, C, T, H, W, L.ptr(AH), L.ptr(AW), gt, gh, gw, n, seed, thresh, 0, B, L.ptr(P), 4,
                                   st()))

    def box_stage():
        L.check(lib.ivf_box_stage(L.ptr(x1), 1, C, T, H, W, L.ptr(AH), L.ptr(AW), gh, gw, T, gh, gw, nbox - B, B, L.ptr(P3), 4, st()))

    def pair():
        L.check(lib.ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AH), L.ptr(AW), L.ptr(M), B, T, gh, gw, H, W, st()))
        L.check(lib.ivf_stfreeze_fwd(L.ptr(xr), L.ptr(M), L.ptr(P2), B, C, T, HW, 4, st()))

    for _ in range(3):
        stage(), box_stage(), pair()
    torch.cuda.synchronize()
    assert torch.equal(P, P2), "ivf_rise_stage differs from expand_fwd + stfreeze_fwd"
    ts, tx, tp = [], [], []
    for _ in range(4 * args.reps):
        ts.append(event_ms(stage))
        tx.append(event_ms(box_stage))
        tp.append(event_ms(pair))
    ms, mx, mp = statistics.median(ts), statistics.median(tx), statistics.median(tp)
    out(f"staging alone, {B} rows, compulsory bytes {staged / 2**20:.1f} MiB (staged rows written once, the clip read once):")
    out(f"  ivf_rise_stage                 {spread(ts)}  {staged / ms / 1e6:8.1f} GB/s of compulsory bytes")
    out(f"  ivf_box_stage (largest boxes)  {spread(tx)}  {staged / mx / 1e6:8.1f} GB/s  (rise / box: {ms / mx:.2f} x the time)")
    out(f"  expand_fwd + stfreeze_fwd      {spread(tp)}  ({mp / ms:.2f} x the time of ivf_rise_stage; outputs equal)")
    out(f"  forward of a {B}-row chunk (from the box rate above): {chunk_ms:.3f} ms; staging is {100 * ms / chunk_ms:.2f} % of it")

    # ---- 3. a whole rise() call at n = 2048 on one clip, and the reduction alone
    nm = 2048

    def whole():
        return eng.rise(x1, tgt, n_masks=nm, p=p, grid=grid, sigma=sigma, seed=seed)

    r = whole()
    torch.cuda.synchronize()
    tw = [event_ms(whole) for _ in range(max(args.reps // 2, 1))]
    out(f"rise() at n = {nm} masks on one clip (forward, scores, reduction, map): {spread(tw)}  "
        f"{1e3 * nm / statistics.median(tw):8.1f} masks/s")
    out(f"  counts per cell {int(r['rise_count'].min())}..{int(r['rise_count'].max())}, mean drop {float(r['rise_mean_drop'][0]):.5f}, "
        f"score {float(r['score_x'][0]):.5f}")

    def reduce():
        return eng.rise_reduce(r["rise_scores"], r["score_x"], p, grid, seed)

    reduce()
    torch.cuda.synchronize()
    tq = [event_ms(reduce) for _ in range(4 * args.reps)]
    out(f"ivf_rise_reduce on {nm} scores, {gt * gh * gw} cells: {spread(tq)}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
