"""Exhaustive one-blob search (maskType 'combi') throughput on one MI355X.

    python tools/blob_bench.py [--reps 25] [--out FILE] [--grid-only]

1. Per-chunk overhead at S16, B=32: device-event time of one 32-row ivf_i3d_blob_scores call (stage -> forward ->
   pick) against ivf_i3d_forward_staged(32) on the same plan, alternated, median of --reps each after warm-up; the
   stage and the selection alone as well.
2. Candidates/s and exhaustive-search clips/s (grid + selection) at S16 and K32, full grid and max_len=8.
3. The naive alternative: the clip replicated into a [32,C,T,H,W] batch and ivf_i3d_perturbed_forward per chunk.

Kernel choice: the committed headline choice (profiles/r03_bench_tuning.json) where it fits the plan, else the
built-in one; never autotuned, so both sides of every comparison run the same kernels.
--grid-only runs one S16 full grid of one clip (for a kernel trace) and exits.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "interpreting-video-features_amd"))

import torch  # noqa: E402

import ivf_engine  # noqa: E402
import ivf_lib as L  # noqa: E402
import ivf_recipe as R  # noqa: E402
import ivf_search  # noqa: E402

TUNING_FILE = os.path.join(ROOT, "profiles", "r03_bench_tuning.json")


def engine(kind, B):
    if kind == "s16":
        eng = ivf_engine.I3DEngine(174, (3, 16, 224, 224), max_batch=B, softmax=True)
        eng.load_state_dict(R.i3d_state_dict(num_classes=174), autotune=False)
    else:
        eng = ivf_engine.I3DEngine(6, (3, 32, 120, 160), max_batch=B, head_hw=(4, 5), head_time_base=4, softmax=True)
        eng.load_state_dict(R.i3d_state_dict(num_classes=6, tag='i3d_kth'), autotune=False)
    choice = "built-in"
    try:
        doc = json.load(open(TUNING_FILE))
        if (doc.get("batch"), doc.get("math"), doc.get("frames"), doc.get("lib_version")) == \
                (B, eng.math, eng.clip_shape[1], L.lib().ivf_version()) and kind == "s16":
            eng.set_tuning(doc["variants"])
            choice = os.path.relpath(TUNING_FILE, ROOT)
    except (OSError, ValueError, KeyError, L.IvfError):
        pass
    return eng, choice


def clip(kind, i):
    if kind == "s16":
        return torch.from_numpy(R.clip(i)).cuda()
    return torch.from_numpy(R.clip(i, 3, 32, 120, 160)).cuda()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(event_ms(fn) for _ in range(reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--grid-only", action="store_true")
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    B = 32
    eng, choice = engine("s16", B)
    x1 = clip("s16", 21)[None]
    t1 = [int(torch.argmax(eng.forward(x1)[0]))]
    if args.grid_only:
        for _ in range(3):
            grid = eng.blob_scores(x1, t1)
            ivf_search.blob_select(grid, torch.ones(1, device='cuda'), torch.zeros(1, device='cuda'), 16)
        torch.cuda.synchronize()
        print("grid-only: three S16 full grids (136 candidates each) + selection done")
        return
    dev = torch.cuda.get_device_properties(0)
    out(f"# tools/blob_bench.py on {dev.name} ({torch.cuda.get_device_name(0)}), math {eng.math}, "
        f"kernel choice: {choice}, reps {args.reps} (median of device-event times)")

    # ---- 1. one 32-row chunk vs the forward alone, alternated
    x2 = torch.cat([x1, clip("s16", 7)[None]])
    t2 = torch.tensor(t1 + [3], dtype=torch.int32, device='cuda')
    scores = torch.empty(2, 16, device='cuda')
    h = eng._h

    def chunk():   # b=2 clips x max_len 1 (16 candidates each) = exactly one 32-row chunk
        L.check(L.lib().ivf_i3d_blob_scores(h, L.ptr(x2), 2, L.ptr(t2), 1, 0, L.ptr(scores), L.stream()))

    def fwd():
        L.check(L.lib().ivf_i3d_forward_staged(h, B, None, None, L.stream()))

    def stage():
        L.check(L.lib().ivf_blob_stage(L.ptr(x2), 2, 3, 16, 224 * 224, 1, 0, 0, B, L.lib().ivf_i3d_input_buffer(h), 4,
                                       L.stream()))

    for _ in range(3):
        chunk()
        fwd()
    torch.cuda.synchronize()
    tc, tf = [], []
    for _ in range(args.reps):
        tc.append(event_ms(chunk))
        tf.append(event_ms(fwd))
    mc, mf = statistics.median(tc), statistics.median(tf)
    ms = median_ms(stage, args.reps)
    grid = eng.blob_scores(x1, t1)
    probs = eng.forward(x1)
    orig = probs[:, t1[0]]
    full = eng.perturbed_forward(x1, torch.ones(1, 16, device='cuda'), "freeze")[:, t1[0]]
    orig, full = orig.contiguous(), full.contiguous()
    best, minimal = torch.empty(1, 2, dtype=torch.int32, device='cuda'), torch.empty(1, 2, dtype=torch.int32, device='cuda')
    bobj = torch.empty(1, device='cuda')

    def select():
        L.check(L.lib().ivf_blob_select(L.ptr(grid), L.ptr(orig), L.ptr(full), 1, 16, 16, 0.01, 0.02, 0.9, L.ptr(best),
                                        L.ptr(bobj), None, L.ptr(minimal), L.stream()))

    msel = median_ms(select, args.reps)
    msel_py = median_ms(lambda: ivf_search.blob_select(grid, orig, full, 16, None, 0.01, 0.02), args.reps)
    per_chunk = msel * B / grid.shape[1]            # one selection per grid of 136 rows = 4.25 chunks
    out(f"S16 B=32 chunk (stage + forward + pick): {mc:.3f} ms; ivf_i3d_forward_staged(32): {mf:.3f} ms; "
        f"overhead {100 * (mc - mf) / mf:+.2f} % of the forward")
    out(f"S16 B=32 ivf_blob_stage alone (32 rows, 16-byte stores): {ms * 1e3:.1f} us ({100 * ms / mf:.2f} %)")
    out(f"S16 ivf_blob_select of one 136-entry grid: {msel * 1e3:.1f} us, {per_chunk * 1e3:.1f} us per 32-row chunk "
        f"({100 * per_chunk / mf:.2f} %); through ivf_search.blob_select (torch glue included) {msel_py * 1e3:.1f} us")
    out(f"S16 B=32 staging + pick + selection per chunk: {100 * (mc - mf + per_chunk) / mf:.2f} % of the chunk's forward")

    # ---- 2. candidates/s and clips/s
    for kind in ("s16", "k32"):
        if kind == "k32":
            del eng
            torch.cuda.empty_cache()
            eng, choice = engine("k32", B)
        T = eng.clip_shape[1]
        for nclips in (1, 4):
            x = torch.stack([clip(kind, 21 + i) for i in range(nclips)])
            tg = eng.argmax(eng.forward(x))
            o, f = torch.ones(nclips, device='cuda'), torch.zeros(nclips, device='cuda')   # selection cost only
            for ml in (T, 8):
                n = L.lib().ivf_blob_count(T, ml)

                def search():
                    g = eng.blob_scores(x, tg, ml)
                    ivf_search.blob_select(g, o, f, T, ml, 0.01, 0.02)

                t = median_ms(search, max(5, args.reps // 3), warmup=2)
                out(f"{kind.upper()} B=32 ({choice}) {nclips} clip(s) max_len {ml:2d}: {nclips * n:5d} candidates in "
                    f"{t:8.2f} ms -> {nclips * n / t * 1e3:8.1f} candidates/s, {nclips / t * 1e3:6.2f} clips/s "
                    "(grid + selection)")
        if kind == "s16":
            # ---- 3. the naive alternative: replicate the clip, perturbed_forward per chunk
            cands = ivf_search.blob_candidates(T)
            masks = ivf_search.blob_masks(cands.cuda(), T)
            xr = x1.expand(B, -1, -1, -1, -1).contiguous()
            n = cands.shape[0]

            def naive():
                for s in range(0, n, B):
                    c = min(B, n - s)
                    eng.perturbed_forward(xr[:c], masks[s:s + c], "freeze")

            def staged():
                eng.blob_scores(x1, t1)

            tn = median_ms(naive, max(5, args.reps // 3), warmup=2)
            ts = median_ms(staged, max(5, args.reps // 3), warmup=2)
            out(f"S16 one clip, full grid ({n}): replicated clip + perturbed_forward per chunk {tn:.2f} ms "
                f"(+{xr.numel() * 4 / 2**20:.0f} MiB replica); ivf_i3d_blob_scores {ts:.2f} ms "
                f"({100 * (tn - ts) / ts:+.1f} %)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
