"""KernelSHAP and LIME on one MI355X: throughput of the rows, cost of the fit, agreement with Shapley sampling.

    python tools/linsur_bench.py [--reps 7] [--out profiles/linear_surrogate_bench.txt]

S16, B = 32, the default arithmetic (bf16x6).

1. Rows per second of ivf_i3d_lin_scores beside ivf_i3d_shap_scores (Shapley sampling, untouched by this feature: the
   yardstick) on the same plan and the same grid (16, 1, 1), alternated in the same run, each call between two device
   events, median and spread of --reps calls after warm-up.  Both are one forward per row, 1,088 rows of one clip: 64
   permutations of the 16 frames against 1,087 KernelSHAP rows and the fully frozen row.
2. ivf_lin_stage alone on the first 32 rows (a whole chunk) beside ivf_shap_stage on 32 rows of the same grid, alternated,
   and the staging time against the time of a 32-row chunk (from 1.).
3. ivf_lin_moments, ivf_lin_solve and ivf_lin_fit alone, at P = 16, 392 and 1,024 players with n = 4 P KernelSHAP rows and
   one clip (random scores: the cost does not depend on them), and the same for LIME's weighted system at P = 1,024.
4. The solve against the accurate fp64 solution of tests/linsur_refs.py at 33 and 1,023 unknowns, both kinds: measured
   error over the gate 2^-24 |phi*| + 8 e_ref (what tests/test_gpu_linsur.py asserts).
5. For one clip, max |kshap_cells - shap_cells| in units of shap_stderr at equal forward passes (64 permutations of the 16
   frames = 1,088 rows against 1,086 paired KernelSHAP rows + 1), and the same for LIME's cells (another estimand: no
   efficiency constraint, a ridge), for orientation.

Kernel choice: as tools/blob_bench.py (the committed headline choice where it fits the plan, never autotuned).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "interpreting-video-features_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivf_lib as L  # noqa: E402
import ivf_recipe as R  # noqa: E402
import linsur_refs as LR  # noqa: E402
import rise_refs as RR  # noqa: E402
from blob_bench import engine, event_ms  # noqa: E402
from box_bench import spread  # noqa: E402


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).reshape(-1))).cuda()


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
    HW, nperm, seed = H * W, 64, 0
    grid = (T, 1, 1)
    P = T
    rows = nperm * (P + 1)
    nlin = rows - 1
    x1 = torch.from_numpy(R.clip(21))[None].cuda()
    tgt = eng.argmax(eng.forward(x1))
    dev = torch.cuda.get_device_properties(0)
    lib, st = L.lib(), L.stream
    out(f"# tools/linsur_bench.py on {dev.name}, S16 B={B}, math {eng.math}, kernel choice: {choice}, grid {grid}, "
        f"default blur, device events")

    # ---- 1. rows per second, the linear-surrogate rows beside Shapley's, alternated
    bits, _ = eng.kshap_rows(nlin, grid, seed, paired=False)

    def lin():
        return eng.lin_scores(x1, tgt, bits, grid, None)

    def shap():
        return eng.shap_scores(x1, tgt, nperm, grid, None, seed)

    lin(), shap()
    torch.cuda.synchronize()
    tl, ts_ = [], []
    for _ in range(args.reps):
        tl.append(event_ms(lin))
        ts_.append(event_ms(shap))
    rl, rs = (1e3 * rows / statistics.median(t) for t in (tl, ts_))
    out(f"{rows} rows of one clip, one forward per row:")
    out(f"  ivf_i3d_lin_scores                     {spread(tl)}  {rl:8.1f} rows/s")
    out(f"  ivf_i3d_shap_scores (ranks included)   {spread(ts_)}  {rs:8.1f} rows/s")
    out(f"  lin / shapley per row: {rs / rl:.4f} of the time of a Shapley row ({100 * (rs / rl - 1):+.2f} %)")
    chunk_ms = statistics.median(tl) * B / rows

    # ---- 2. the staging kernel alone, beside Shapley's
    gt, gh, gw = grid
    _, _, _, AH, AW = eng._st_axes((gh, gw), None)
    ranks = eng.shap_ranks(nperm, grid, seed)
    Pb, P2 = torch.empty(B, T, HW, 4, device='cuda'), torch.empty(B, T, HW, 4, device='cuda')

    def stage():
        L.check(lib.ivf_lin_stage(L.ptr(x1), 1, C, T, H, W, L.ptr(AH), L.ptr(AW), gt, gh, gw, nlin, L.ptr(bits), 0, B, L.ptr(Pb),
                                  4, st()))

    def shap_stage():
        L.check(lib.ivf_shap_stage(L.ptr(x1), 1, C, T, H, W, L.ptr(AH), L.ptr(AW), gt, gh, gw, nperm, L.ptr(ranks), 0, B,
                                   L.ptr(P2), 4, st()))

    for _ in range(3):
        stage(), shap_stage()
    torch.cuda.synchronize()
    tg, tx = [], []
    for _ in range(4 * args.reps):
        tg.append(event_ms(stage))
        tx.append(event_ms(shap_stage))
    ms, mx = statistics.median(tg), statistics.median(tx)
    staged = Pb.numel() * 4 + x1.numel() * 4
    out(f"staging alone, {B} rows, compulsory bytes {staged / 2**20:.1f} MiB (staged rows written once, the clip read once):")
    out(f"  ivf_lin_stage                  {spread(tg)}  {staged / ms / 1e6:8.1f} GB/s of compulsory bytes")
    out(f"  ivf_shap_stage (same grid)     {spread(tx)}  {staged / mx / 1e6:8.1f} GB/s  (lin / shapley: {ms / mx:.2f} x the time)")
    out(f"  a {B}-row chunk (stage + forward + pick, from 1.): {chunk_ms:.3f} ms; staging is {100 * ms / chunk_ms:.2f} % of it")

    # ---- 3. the fit alone
    g = np.random.default_rng(0)
    out("the fit alone, one clip, n = 4 P rows (moments | Cholesky solve | fit quality):")
    for kind, Pn in ((0, 16), (0, 392), (0, 1024), (1, 1024)):
        n = 4 * Pn
        Z = LR.kshap_rows(1234, n, Pn)[0] if kind == 0 else LR.lime_rows(1234, RR.thresh(0.5), n, Pn)
        bd = torch.from_numpy(LR.pack(Z).view(np.int32)).cuda()
        s, sx = _dev(g.random((1, n + 1)), np.float32), _dev(g.random(1), np.float32)
        wt = None if kind == 0 else _dev(LR.lime_wtab(Pn), np.float64)
        f64 = dict(dtype=torch.float64, device='cuda')
        N, v, Ws, r, t, wrow = (torch.empty(Pn, Pn, **f64), torch.empty(Pn, **f64), torch.empty(1, **f64),
                                torch.empty(1, Pn, **f64), torch.empty(1, **f64), torch.empty(n, **f64))
        ok = torch.empty(1, dtype=torch.int32, device='cuda')
        cells, icpt, tot, r2 = (torch.empty(1, Pn, device='cuda'), torch.empty(1, device='cuda'), torch.empty(1, device='cuda'),
                                torch.empty(1, device='cuda'))
        work = torch.empty(lib.ivf_lin_workspace_bytes(Pn), dtype=torch.uint8, device='cuda')

        def moments():
            L.check(lib.ivf_lin_moments(L.ptr(s), L.ptr(sx), L.ptr(bd), L.ptr(wt), 1, n, Pn, L.ptr(N), L.ptr(v), L.ptr(Ws), L.ptr(r),
                                        L.ptr(t), L.ptr(wrow), L.ptr(ok), st()))

        def solve():
            L.check(lib.ivf_lin_solve(kind, L.ptr(N), L.ptr(v), L.ptr(Ws), L.ptr(r), L.ptr(t), L.ptr(s), L.ptr(sx), 1, n, Pn, 1.0,
                                      L.ptr(work), L.ptr(cells), L.ptr(icpt), L.ptr(tot), L.ptr(ok), st()))

        def fit():
            L.check(lib.ivf_lin_fit(L.ptr(s), L.ptr(sx), L.ptr(bd), L.ptr(wrow), L.ptr(cells), L.ptr(icpt), L.ptr(t), L.ptr(Ws),
                                    L.ptr(ok), 1, n, Pn, L.ptr(r2), st()))

        moments(), solve(), fit()
        torch.cuda.synchronize()
        tm, tv, tf = [], [], []
        for _ in range(args.reps):
            tm.append(event_ms(moments))
            tv.append(event_ms(solve))
            tf.append(event_ms(fit))
        total = sum(statistics.median(q) for q in (tm, tv, tf))
        out(f"  {'kernelshap' if kind == 0 else 'lime      '} P {Pn:5d} n {n:5d}: {spread(tm)} | {spread(tv)} | {spread(tf)}  "
            f"= {total:.3f} ms, ok {int(ok[0])}, r2 {float(r2[0]):+.4f}")

    # ---- 4. the solve against the accurate fp64 solution
    out("solve against phi* (numpy solve + 2 refinement steps in longdouble), 3 right-hand sides, err / gate:")
    for kind in (0, 1):
        for m in (33, 1023):
            Pn = m + 1 if kind == 0 else m
            n = 4 * Pn if kind == 0 else 256
            Z = LR.kshap_rows(1234, n, Pn)[0] if kind == 0 else LR.lime_rows(1234, RR.thresh(0.5), n, Pn)
            s, sx = g.random((3, n + 1)).astype(np.float32), g.random(3).astype(np.float32)
            ref = LR.kshap_fit(Z, s, sx) if kind == 0 else LR.lime_fit(Z, s, sx, LR.lime_wtab(Pn), 1.0)
            bd = torch.from_numpy(LR.pack(Z).view(np.int32)).cuda()
            got = eng.lin_solve("kernelshap" if kind == 0 else "lime", torch.from_numpy(s).cuda(), torch.from_numpy(sx).cuda(), bd,
                                Pn, None if kind == 0 else LR.lime_wtab(Pn), 1.0)
            err = np.abs(got["cells"].cpu().numpy().astype(np.float64) - ref["cells"])
            out(f"  kind {kind} unknowns {m:5d}: e_ref {ref['e_ref']:.2e}, worst err / gate {float((err / LR.gate(ref['cells'], ref['e_ref'])).max()):.3f}, "
                f"worst err / |phi*|_max {float(err.max() / np.abs(ref['cells']).max()):.2e}")

    # ---- 5. KernelSHAP beside Shapley sampling at equal forward passes
    sh = eng.shapley(x1, tgt, n_perms=nperm, grid=grid, seed=seed)
    ks = eng.kernelshap(x1, tgt, n_samples=rows - 2, grid=grid, seed=seed)
    lm = eng.lime(x1, tgt, n_samples=rows - 1, grid=grid, seed=seed)
    se = sh["shap_stderr"][0].reshape(-1)
    dk = ((ks["kshap_cells"][0].reshape(-1) - sh["shap_cells"][0].reshape(-1)).abs() / se)
    dl = ((lm["lime_cells"][0].reshape(-1) - sh["shap_cells"][0].reshape(-1)).abs() / se)
    ok_ = se > 0
    out(f"one clip, grid {grid}, {rows} forward passes each: max |kshap_cells - shap_cells| = {float(dk[ok_].max()):.2f} shap_stderr "
        f"(median {float(dk[ok_].median()):.2f}); kshap_ok {int(ks['kshap_ok'][0])}, r2 {float(ks['kshap_r2'][0]):.4f}, "
        f"sum {float(ks['kshap_cells'].sum()):+.5f} = kshap_total {float(ks['kshap_total'][0]):+.5f}, shap_total {float(sh['shap_total'][0]):+.5f}")
    out(f"  LIME (p 0.5, width 0.25, ridge 1): max |lime_cells - shap_cells| = {float(dl[ok_].max()):.2f} shap_stderr; lime_ok "
        f"{int(lm['lime_ok'][0])}, r2 {float(lm['lime_r2'][0]):.4f}, intercept {float(lm['lime_intercept'][0]):+.5f}")
    out("not measured: the ConvLSTM plan, S32, grids with spatial cells on the plan")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
