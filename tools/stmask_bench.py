"""Spatio-temporal mask search (maskType 'spacetime') against the temporal search on one MI355X.

    python tools/stmask_bench.py [--iters 10] [--reps 7] [--out profiles/stmask_bench.txt] [--loop temporal|spacetime]

1. ms per iteration of ivf_i3d_stsearch (grid 7x7, sigma 16) against ivf_i3d_search on the same plan at S16, B=32, the
   default arithmetic (bf16x6): `--iters` iterations per call between two device events, the two loops alternated,
   median of --reps calls each after warm-up.
2. Every new kernel alone at the same shape: median device-event time and the achieved GB/s against its compulsory
   bytes (what it must read and write once: the clip, M or dM, the staged input or its gradient).
3. The network's forward behind the temporal and the per-pixel staging kernel, on the same staged values.

Kernel choice: the committed headline choice (profiles/r03_bench_tuning.json) where it fits the plan, else the built-in
one; never autotuned, so both loops run the same network kernels.
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", choices=["temporal", "spacetime"], default=None,
                    help="run this loop alone (one warm-up call, then --reps calls) and exit: for tools/stmask_trace_diff.py")
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    B, N = args.batch, args.iters
    eng, choice = engine("s16", B)
    C, T, H, W = eng.clip_shape
    HW, gh, gw, sigma = H * W, 7, 7, 16.0
    x = torch.stack([torch.from_numpy(R.clip(21 + i)) for i in range(B)]).cuda()
    tgt = eng.argmax(eng.forward(x))
    dev = torch.cuda.get_device_properties(0)
    out(f"# tools/stmask_bench.py on {dev.name}, S16 B={B}, math {eng.math}, kernel choice: {choice}, grid {gh}x{gw}, "
        f"sigma {sigma:g}, {N} iterations per call, median of {args.reps} calls (device events)")

    # ---- 1. the two loops, alternated
    raw_t = torch.zeros(B, T, device='cuda')
    raw_s = torch.zeros(B, T, gh, gw, device='cuda')

    def temporal():
        raw_t.fill_(0.5)
        eng.search(x, tgt, raw_t, 0.01, 0.02, N, want_traj=False)

    def spacetime():
        raw_s.fill_(0.5)
        eng.st_search(x, tgt, raw_s, 0.01, 0.02, N, (gh, gw), sigma, want_traj=False)

    if args.loop:
        fn = temporal if args.loop == "temporal" else spacetime
        fn()
        torch.cuda.synchronize()
        t = [event_ms(fn) / N for _ in range(args.reps)]
        print(f"{args.loop} loop alone: {statistics.median(t):.3f} ms / iteration over {args.reps} calls of {N}")
        return
    for _ in range(2):
        temporal()
        spacetime()
    torch.cuda.synchronize()
    tt, ts = [], []
    for _ in range(args.reps):
        tt.append(event_ms(temporal) / N)
        ts.append(event_ms(spacetime) / N)
    mt, ms = statistics.median(tt), statistics.median(ts)
    out(f"temporal search  (ivf_i3d_search):   {mt:8.3f} ms / iteration  (min {min(tt):.3f}, max {max(tt):.3f})")
    out(f"spacetime search (ivf_i3d_stsearch): {ms:8.3f} ms / iteration  (min {min(ts):.3f}, max {max(ts):.3f})")
    out(f"overhead of the spacetime loop: {ms - mt:+.3f} ms / iteration = {100 * (ms - mt) / mt:+.2f} % of the temporal one")

    # ---- 2. the kernels alone
    lib = L.lib()
    _, _, _, AH, AW = eng._st_axes((gh, gw), sigma)
    S = torch.sigmoid(torch.randn(B, T, gh, gw, device='cuda'))
    M = eng.st_expand(S, (gh, gw), sigma)
    P = torch.empty(B, T, HW, 4, device='cuda')
    g = torch.randn(B, T, HW, 4, device='cuda')
    dM, dS = torch.empty(B, T, HW, device='cuda'), torch.empty(B, T, gh, gw, device='cuda')
    sig, dreg, terms = torch.empty_like(S), torch.empty_like(S), torch.empty(B, 3, device='cuda')
    score, am, av, row = torch.zeros(B, device='cuda'), torch.zeros_like(S), torch.zeros_like(S), torch.empty(B, 5, device='cuda')
    rows = torch.rand(B, T, device='cuda')
    ws = torch.empty(lib.ivf_freeze_bwd_workspace_bytes(B, T), dtype=torch.uint8, device='cuda')
    dmask = torch.empty(B, T, device='cuda')
    sig_t, dreg_t, terms_t = torch.empty(B, T, device='cuda'), torch.empty(B, T, device='cuda'), torch.empty(B, 2, device='cuda')
    am_t, av_t, row_t = torch.zeros(B, T, device='cuda'), torch.zeros(B, T, device='cuda'), torch.empty(B, 4, device='cuda')
    st = L.stream
    xb, mb, pb = x.numel() * 4, M.numel() * 4, P.numel() * 4
    small = S.numel() * 4
    kernels = [
        ("ivf_stmask_reg", small * 3, lambda: lib.ivf_stmask_reg(L.ptr(raw_s), B, T, gh, gw, 0.01, 0.02, 0.02, L.ptr(sig), L.ptr(terms), L.ptr(dreg), st())),
        ("ivf_stmask_expand_fwd", mb, lambda: lib.ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AH), L.ptr(AW), L.ptr(M), B, T, gh, gw, H, W, st())),
        ("ivf_stfreeze_fwd (16-byte pixels)", xb + mb + pb, lambda: lib.ivf_stfreeze_fwd(L.ptr(x), L.ptr(M), L.ptr(P), B, C, T, HW, 4, st())),
        ("ivf_stfreeze_bwd (16-byte pixels)", xb + mb + pb + mb, lambda: lib.ivf_stfreeze_bwd(L.ptr(x), L.ptr(M), L.ptr(g), L.ptr(dM), B, C, T, HW, 4, st())),
        ("ivf_stmask_expand_bwd", mb, lambda: lib.ivf_stmask_expand_bwd(L.ptr(dM), L.ptr(AH), L.ptr(AW), L.ptr(dS), B, T, gh, gw, H, W, st())),
        ("ivf_stmask_step", small * 9, lambda: lib.ivf_stmask_step(L.ptr(raw_s), L.ptr(sig), L.ptr(dS), L.ptr(dreg), L.ptr(terms), L.ptr(score), L.ptr(am), L.ptr(av), L.ptr(row), B, T, gh, gw, 1, 0.2, 0.9, 0.999, 1e-8, st())),
        ("ivf_freeze_fwd (temporal, for comparison)", xb + pb, lambda: lib.ivf_freeze_fwd(L.ptr(x), L.ptr(rows), L.ptr(P), B, C, T, HW, 1, 4, st())),
        ("ivf_freeze_bwd (temporal, for comparison)", xb + pb, lambda: lib.ivf_freeze_bwd(L.ptr(x), L.ptr(rows), L.ptr(g), L.ptr(dmask), None, B, C, T, HW, 1, 4, L.ptr(ws), st())),
        ("ivf_mask_reg (temporal, for comparison)", B * T * 12, lambda: lib.ivf_mask_reg(L.ptr(raw_t), B, T, 0.01, 0.02, L.ptr(sig_t), L.ptr(terms_t), L.ptr(dreg_t), st())),
        ("ivf_search_step (temporal, for comparison)", B * T * 36, lambda: lib.ivf_search_step(L.ptr(raw_t), L.ptr(sig_t), L.ptr(dmask), L.ptr(dreg_t), L.ptr(terms_t), L.ptr(score), L.ptr(am_t), L.ptr(av_t), L.ptr(row_t), B, T, 1, 0.2, 0.9, 0.999, 1e-8, st())),
    ]
    out("kernels alone, launched back to back on the same buffers (M and dM, 98 MiB each, then stay in the 256 MB "
        "last-level cache: in the loop they are read after the network's traffic; see the trace attribution):")
    total_new = total_old = 0.0
    for name, nbytes, fn in kernels:
        L.check(fn())
        t = median_ms(fn, 4 * args.reps)
        if "temporal" in name:
            total_old += t
        else:
            total_new += t
        out(f"{name:44s} {t * 1e3:9.1f} us  {nbytes / 2**20:8.1f} MiB compulsory  {nbytes / t / 1e6:8.1f} GB/s")
    out(f"sum of the six new kernels {total_new:.3f} ms; the four temporal kernels they replace {total_old:.3f} ms; "
        f"difference {total_new - total_old:+.3f} ms = {100 * (total_new - total_old) / mt:+.2f} % of a temporal iteration")
    # ---- 3. the network's forward behind each staging kernel (the trace shows the first convolution slower in the
    # spacetime loop): the same clip values staged three ways, alternated
    Mc = rows.view(B, T, 1, 1).expand(B, T, H, W).contiguous()
    variants = [
        ("ivf_freeze_fwd + forward", lambda: eng.perturbed_forward(x, rows, "freeze")),
        ("ivf_stfreeze_fwd + forward", lambda: eng.st_perturbed_forward(x, Mc)),
        ("ivf_stmask_expand_fwd + ivf_stfreeze_fwd + forward", lambda: (kernels[1][2](), eng.st_perturbed_forward(x, Mc))),
    ]
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(2 * args.reps + 1):
        for k, (_, fn) in enumerate(variants):
            times[k].append(event_ms(fn))
    base = statistics.median(times[0])
    for (name, _), t in zip(variants, times):
        m = statistics.median(t)
        out(f"{name:52s} {m:8.3f} ms  (min {min(t):.3f}, max {max(t):.3f})  {1e3 * (m - base):+7.1f} us against the first")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
