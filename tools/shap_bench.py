"""Shapley value sampling throughput on one MI355X.

    python tools/shap_bench.py [--reps 7] [--out profiles/shapley_bench.txt]

S16, B = 32, the default arithmetic (bf16x6).

1. Rows per second of ivf_i3d_shap_scores beside ivf_i3d_rise_scores (RISE, untouched by this feature: the yardstick) on
   the same plan, alternated, each call between two device events, median and spread of --reps calls after warm-up.
   Both are one forward per row: 64 permutations of the 16 frames (the default grid (16, 1, 1), 1,088 rows of one clip)
   against 1,088 RISE masks on its default grid (8, 7, 7) at p = 0.5, and against 1,088 RISE masks on the Shapley grid
   (16, 1, 1) -- the same staging geometry, so what is left between those two is the data of the rows.
2. ivf_shap_stage alone on the first 32 rows (a whole chunk: prefixes 0 .. 16 of permutation 0, 0 .. 14 of permutation
   1), beside ivf_rise_stage on 32 rows of the same grid and ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit
   masks of the Shapley rows, the three alternated.  Achieved GB/s against the compulsory bytes (the staged rows
   written once, the clip read once), and the staging time against the forward time of a 32-row chunk (from 1.).
3. One shapley() call with its defaults (64 permutations, grid (T, 1, 1), antithetic) on one clip, everything included
   (the clip's own forward, ranks, scores, reduction, expansion to the map); ivf_shap_ranks alone at 64 permutations of
   16 and of 4,096 players; ivf_shap_reduce alone.

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
    HW, n, seed, p = H * W, 64, 0, 0.5
    grid, rgrid = (T, 1, 1), (8, 7, 7)
    P = T
    rows = n * (P + 1)
    x1 = torch.from_numpy(R.clip(21))[None].cuda()
    tgt = eng.argmax(eng.forward(x1))
    dev = torch.cuda.get_device_properties(0)
    out(f"# tools/shap_bench.py on {dev.name}, S16 B={B}, math {eng.math}, kernel choice: {choice}, grid {grid}, "
        f"{n} permutations, default blur, device events")

    # ---- 1. rows per second, Shapley beside RISE, alternated
    def shap():
        return eng.shap_scores(x1, tgt, n, grid, None, seed)

    def rise():
        return eng.rise_scores(x1, tgt, rows, p, rgrid, None, seed)

    def rise_same():
        return eng.rise_scores(x1, tgt, rows, p, grid, None, seed)

    shap(), rise(), rise_same()
    torch.cuda.synchronize()
    ts_, tr, tq = [], [], []
    for _ in range(args.reps):
        ts_.append(event_ms(shap))
        tr.append(event_ms(rise))
        tq.append(event_ms(rise_same))
    rs, rr, rq = (1e3 * rows / statistics.median(t) for t in (ts_, tr, tq))
    out(f"{rows} rows of one clip, one forward per row:")
    out(f"  ivf_i3d_shap_scores (ranks included)   {spread(ts_)}  {rs:8.1f} rows/s")
    out(f"  ivf_i3d_rise_scores grid {rgrid}     {spread(tr)}  {rr:8.1f} rows/s")
    out(f"  ivf_i3d_rise_scores grid {grid}    {spread(tq)}  {rq:8.1f} rows/s")
    out(f"  shapley / rise per row: {rr / rs:.4f} of the time of a RISE row on {rgrid} ({100 * (rr / rs - 1):+.2f} %), "
        f"{rq / rs:.4f} of one on {grid} ({100 * (rq / rs - 1):+.2f} %)")
    chunk_ms = statistics.median(tr) * B / rows

    # ---- 2. the staging kernel alone, beside the RISE staging and the kernel pair
    lib = L.lib()
    gt, gh, gw = grid
    _, _, _, AH, AW = eng._st_axes((gh, gw), None)
    thresh = ivf_engine.rise_thresh(p)
    ranks = eng.shap_ranks(n, grid, seed)
    Pb = torch.empty(B, T, HW, 4, device='cuda')
    P2 = torch.empty_like(Pb)
    P3 = torch.empty_like(Pb)
    M = torch.empty(B, T, H, W, device='cuda')
    xr = x1.expand(B, C, T, H, W).contiguous()
    r = torch.arange(B, device='cuda')
    k, j = r // (P + 1), r % (P + 1)
    S = (ranks[k].to(torch.int32) < j[:, None]).to(torch.float32).reshape(B, gt, gh, gw)
    S = S[:, (torch.arange(T, device='cuda') * gt) // T].contiguous()          # [B,T,gh,gw], the rows' explicit masks
    st = L.stream
    staged = Pb.numel() * 4 + x1.numel() * 4

    def stage():
        L.check(lib.ivf_shap_stage(L.ptr(x1), 1, C, T, H, W, L.ptr(AH), L.ptr(AW), gt, gh, gw, n, L.ptr(ranks), 0, B, L.ptr(Pb), 4,
                                   st()))

    def rise_stage():
        L.check(lib.ivf_rise_stage(L.ptr(x1), 1, C, T, H, W, L.ptr(AH), L.ptr(AW), gt, gh, gw, rows, seed, thresh, 0, B,
                                   L.ptr(P3), 4, st()))

    def pair():
        L.check(lib.ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AH), L.ptr(AW), L.ptr(M), B, T, gh, gw, H, W, st()))
        L.check(lib.ivf_stfreeze_fwd(L.ptr(xr), L.ptr(M), L.ptr(P2), B, C, T, HW, 4, st()))

    for _ in range(3):
        stage(), rise_stage(), pair()
    torch.cuda.synchronize()
    assert torch.equal(Pb, P2), "ivf_shap_stage differs from expand_fwd + stfreeze_fwd"
    tg, tx, tp = [], [], []
    for _ in range(4 * args.reps):
        tg.append(event_ms(stage))
        tx.append(event_ms(rise_stage))
        tp.append(event_ms(pair))
    ms, mx, mp = statistics.median(tg), statistics.median(tx), statistics.median(tp)
    out(f"staging alone, {B} rows, compulsory bytes {staged / 2**20:.1f} MiB (staged rows written once, the clip read once):")
    out(f"  ivf_shap_stage                 {spread(tg)}  {staged / ms / 1e6:8.1f} GB/s of compulsory bytes")
    out(f"  ivf_rise_stage (same grid)     {spread(tx)}  {staged / mx / 1e6:8.1f} GB/s  (shapley / rise: {ms / mx:.2f} x the time)")
    out(f"  expand_fwd + stfreeze_fwd      {spread(tp)}  ({mp / ms:.2f} x the time of ivf_shap_stage; outputs equal)")
    out(f"  forward of a {B}-row chunk (from the RISE rate above): {chunk_ms:.3f} ms; staging is {100 * ms / chunk_ms:.2f} % of it")

    # ---- 3. the default call on one clip; the rank table and the reduction alone
    def whole():
        return eng.shapley(x1, tgt)

    res = whole()
    torch.cuda.synchronize()
    tw = [event_ms(whole) for _ in range(max(args.reps // 2, 1))]
    out(f"shapley() with its defaults ({n} permutations of {T} frames, {rows} rows) on one clip (forward, ranks, scores, "
        f"reduction, map): {spread(tw)} = {statistics.median(tw) / 1e3:.3f} s")
    cells = res["shap_cells"][0].reshape(-1)
    out(f"  frame values {float(cells.min()):+.5f} .. {float(cells.max()):+.5f}, largest stderr {float(res['shap_stderr'].max()):.5f}, "
        f"sum {float(cells.sum()):+.5f}, shap_total {float(res['shap_total'][0]):+.5f}, score {float(res['score_x'][0]):.5f}")

    for g in (grid, (4, 32, 32)):                         # the default table and the largest one
        table = torch.empty(n, g[0] * g[1] * g[2], dtype=torch.int16, device='cuda')

        def rk():
            L.check(lib.ivf_shap_ranks(seed, 1, 0, n, g[0], g[1], g[2], L.ptr(table), st()))

        rk()
        torch.cuda.synchronize()
        tk = [event_ms(rk) for _ in range(4 * args.reps)]
        out(f"ivf_shap_ranks, {n} permutations of {g[0] * g[1] * g[2]} players: {spread(tk)}")

    def reduce():
        return eng.shap_reduce(res["shap_scores"], grid, seed)

    reduce()
    torch.cuda.synchronize()
    tq = [event_ms(reduce) for _ in range(4 * args.reps)]
    out(f"ivf_shap_reduce (ranks included) on {n} x {P + 1} scores, {P} cells: {spread(tq)}")
    out("not measured: the ConvLSTM plan, S32, grids with spatial cells")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
