"""Deletion / insertion curves throughput on one MI355X.

    python tools/curve_bench.py [--reps 7] [--out profiles/curve_bench.txt]

S16, B = 32, the default arithmetic (bf16x6).

1. Rows per second of ivf_i3d_curve_scores -- 32 clips, grid (16, 1, 1), step 1, both curves: 32 x 2 x 17 = 1,088 rows in
   34 chunks -- beside ivf_i3d_shap_scores (Shapley, untouched by this feature: the yardstick) on the same grid and the
   same number of rows (64 permutations of one clip), alternated, each call between two device events, median and
   spread of --reps calls after warm-up.
2. The same 32 clips through the emulation the feature replaces: one ivf_i3d_shap_scores call per clip with the caller's
   table (the clip's ranks and their reverse: 34 rows, a chunk of 32 and one of 2), 64 chunks in all.
3. ivf_curve_stage alone on the first 32 rows (a whole chunk) beside ivf_shap_stage on 32 rows of the same grid, against
   the forward time of a 32-row chunk (from 1.).
4. ivf_curve_ranks at 4,096 players for 32 clips, and at the default 16; ivf_curve_reduce on the scores of 1.

Kernel choice: as tools/blob_bench.py (the committed headline choice where it fits the plan, never autotuned).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "interpreting-video-features_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivf_lib as L  # noqa: E402
import ivf_recipe as R  # noqa: E402
from blob_bench import engine, event_ms  # noqa: E402
from box_bench import spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    B, nb = args.batch, args.clips
    eng, choice = engine("s16", B)
    C, T, H, W = eng.clip_shape
    grid, P = (T, 1, 1), T
    rows = nb * 2 * (P + 1)
    x = torch.from_numpy(np.stack([R.clip(i) for i in range(nb)])).cuda()
    tgt = torch.cat([eng.argmax(eng.forward(x[i:i + B])) for i in range(0, nb, B)])
    attr = torch.rand(nb, T, generator=torch.Generator().manual_seed(0)).cuda()
    ranks = eng.curve_ranks(attr, grid)
    n = rows // (P + 1)
    dev = torch.cuda.get_device_properties(0)
    out(f"# tools/curve_bench.py on {dev.name}, S16 B={B}, math {eng.math}, kernel choice: {choice}, grid {grid}, step 1, "
        f"both curves, {nb} clips, default blur, device events")

    # ---- 1. rows per second, curves beside Shapley, alternated
    def curves():
        return eng.curve_scores(x, tgt, ranks, grid, None, 1, 3)

    def shap():
        return eng.shap_scores(x[:1], tgt[:1], n, grid, None, 0)

    # ---- 2. the emulation: one Shapley call per clip with the clip's table and its reverse
    lib = L.lib()
    _, _, _, AH, AW = eng._st_axes((1, 1), None)
    pair = torch.stack([ranks, (P - 1) - ranks], dim=1).contiguous()              # [nb, 2, P]
    emu_scores = torch.empty(nb, 2, P + 1, device='cuda')
    fn = eng._fn("shap_scores")

    def emulation():
        for i in range(nb):
            L.check(fn(eng._h, L.ptr(x[i:i + 1]), 1, L.ptr(tgt[i:i + 1]), L.ptr(AH), L.ptr(AW), T, 1, 1, 2, L.ptr(pair[i]),
                       L.ptr(emu_scores[i]), L.stream()))

    sc = curves()
    shap(), emulation()
    torch.cuda.synchronize()
    err = float((emu_scores[:, 0] - sc[:, 0]).abs().max()), float((emu_scores[:, 1].flip(-1) - sc[:, 1]).abs().max())
    tc, ts_, te = [], [], []
    for _ in range(args.reps):
        tc.append(event_ms(curves))
        ts_.append(event_ms(shap))
        te.append(event_ms(emulation))
    rc, rs, re_ = (1e3 * rows / statistics.median(t) for t in (tc, ts_, te))
    chunks, emu_chunks = -(-rows // B), nb * -(-2 * (P + 1) // B)
    out(f"{rows} rows, one forward per row:")
    out(f"  ivf_i3d_curve_scores, {nb} clips ({chunks} chunks)         {spread(tc)}  {rc:8.1f} rows/s")
    out(f"  ivf_i3d_shap_scores, 1 clip x {n} permutations          {spread(ts_)}  {rs:8.1f} rows/s")
    out(f"  curves / shapley per row: {rs / rc:.4f} of the time of a Shapley row ({100 * (rs / rc - 1):+.2f} %)")
    out(f"  emulation: {nb} ivf_i3d_shap_scores calls of 2 permutations ({emu_chunks} chunks)  {spread(te)}  {re_:8.1f} rows/s")
    out(f"  curves / emulation: {statistics.median(te) / statistics.median(tc):.3f} x faster ({emu_chunks} chunks against "
        f"{chunks}); largest score difference deletion {err[0]:.2e}, insertion {err[1]:.2e}")
    chunk_ms = statistics.median(tc) / chunks

    # ---- 3. the staging kernel alone
    Pb = torch.empty(B, T, H * W, 4, device='cuda')
    P2 = torch.empty_like(Pb)
    staged = Pb.numel() * 4 + x[:1].numel() * 4                    # the first 32 rows are clip 0's
    sranks = eng.shap_ranks(2, grid, 0)

    def stage():
        L.check(lib.ivf_curve_stage(L.ptr(x), nb, C, T, H, W, L.ptr(AH), L.ptr(AW), T, 1, 1, L.ptr(ranks), 3, 1, 0, B,
                                    L.ptr(Pb), 4, L.stream()))

    def shap_stage():
        L.check(lib.ivf_shap_stage(L.ptr(x), 1, C, T, H, W, L.ptr(AH), L.ptr(AW), T, 1, 1, 2, L.ptr(sranks), 0, B, L.ptr(P2), 4,
                                   L.stream()))

    for _ in range(3):
        stage(), shap_stage()
    torch.cuda.synchronize()
    tg, tx = [], []
    for _ in range(4 * args.reps):
        tg.append(event_ms(stage))
        tx.append(event_ms(shap_stage))
    ms, mx = statistics.median(tg), statistics.median(tx)
    out(f"staging alone, {B} rows, compulsory bytes {staged / 2**20:.1f} MiB (staged rows written once, the clip read once):")
    out(f"  ivf_curve_stage                {spread(tg)}  {staged / ms / 1e6:8.1f} GB/s of compulsory bytes")
    out(f"  ivf_shap_stage (same grid)     {spread(tx)}  (curves / shapley: {ms / mx:.2f} x the time)")
    out(f"  a {B}-row chunk of 1. (staging, forward, pick): {chunk_ms:.3f} ms; staging is {100 * ms / chunk_ms:.2f} % of it")

    # ---- 4. the rank table and the reduction alone
    for g in ((4, 32, 32), grid):
        a = torch.rand(32, g[0], g[1], g[2], device='cuda')
        table = torch.empty(32, g[0] * g[1] * g[2], dtype=torch.int16, device='cuda')

        def rk():
            L.check(lib.ivf_curve_ranks(L.ptr(a), 32, g[0], T, g[0], g[1], g[2], 0, L.ptr(table), L.stream()))

        rk()
        torch.cuda.synchronize()
        tk = [event_ms(rk) for _ in range(4 * args.reps)]
        out(f"ivf_curve_ranks, 32 clips of {g[0] * g[1] * g[2]} players: {spread(tk)}")

    def reduce():
        return eng.curve_reduce(sc, grid, 1, 3)

    reduce()
    torch.cuda.synchronize()
    tq = [event_ms(reduce) for _ in range(4 * args.reps)]
    out(f"ivf_curve_reduce on {nb} x 2 x {P + 1} scores: {spread(tq)}")
    out("not measured: the ConvLSTM plan, S32, grids with spatial cells, steps above 1")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
