"""Score-CAM throughput on one MI355X.

    python tools/scorecam_bench.py [--reps 5] [--out profiles/scorecam_bench.txt]

S16, B = 32, the default arithmetic (bf16x6), the default blur of the spacetime search, 'freeze', 'increase', for two
target layers in one run: Mixed_5c (1024 channels, a 2 x 7 x 7 map) and Mixed_3c (480 channels, 8 x 28 x 28).  Per layer:

1. The share of channels that are not valid (dead after the ReLU: a constant plane).  Each still costs a forward; a
   later change that compacts them out of the row list can judge its gain from this line.
2. ivf_scorecam_stage alone on 32 rows beside ivf_rise_stage on 32 rows of the same grid dimensions (p = 0.5), the two
   alternated, each call between two device events; and the plan's forward of a 32-row chunk on the staged rows.  The
   staging share of a chunk's forward is the ratio of the two medians.
3. ivf_i3d_scorecam_scores over all channels of one clip: rows per second; and one whole scorecam() call (planes,
   scores, reduction, resize): seconds per clip.

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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--layers", default="Mixed_5c,Mixed_3c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    B = args.batch
    eng, choice = engine("s16", B)
    C, T, H, W = eng.clip_shape
    HW = H * W
    lib, st = L.lib(), L.stream
    x1 = torch.from_numpy(R.clip(21))[None].cuda()
    tgt = eng.argmax(eng.forward(x1))
    dev = torch.cuda.get_device_properties(0)
    out(f"# tools/scorecam_bench.py on {dev.name}, S16 B={B}, math {eng.math}, kernel choice: {choice}, default sigma, "
        f"'freeze', 'increase', device events")
    P = torch.empty(B, T, HW, 4, device='cuda')
    P2 = torch.empty_like(P)
    thresh = ivf_engine.rise_thresh(0.5)
    for layer in args.layers.split(","):
        planes = eng.scorecam_planes(x1, layer)
        F, valid = planes["F"], planes["valid"]
        nc, gt, gh, gw = F.shape[1:]
        dead = nc - int(valid.sum())
        _, _, sigma, AH, AW = eng._st_axes((gh, gw), None)
        out(f"{layer}: {nc} channels, map {gt}x{gh}x{gw} ({gt * gh * gw} cells), sigma {sigma:g}; "
            f"{dead} channels not valid ({100.0 * dead / nc:.1f} % of the rows are forwards of the baseline row)")

        def stage():
            L.check(lib.ivf_scorecam_stage(L.ptr(x1), 1, C, T, H, W, L.ptr(AH), L.ptr(AW), gt, gh, gw, L.ptr(F), nc, 0, 0, B,
                                           L.ptr(P), 4, st()))

        def rise_stage():
            L.check(lib.ivf_rise_stage(L.ptr(x1), 1, C, T, H, W, L.ptr(AH), L.ptr(AW), gt, gh, gw, B, 0, thresh, 0, B, L.ptr(P2),
                                       4, st()))

        for _ in range(3):
            stage(), rise_stage()
        rows = P.view(B, T, H, W, 4)[..., :C].permute(0, 4, 1, 2, 3).contiguous()     # the staged rows as NCTHW clips

        def fwd():
            return eng.forward(rows)

        fwd()
        torch.cuda.synchronize()
        ts, tr, tf = [], [], []
        for _ in range(4 * args.reps):
            ts.append(event_ms(stage))
            tr.append(event_ms(rise_stage))
        for _ in range(args.reps):
            tf.append(event_ms(fwd))
        ms, mr, mf = statistics.median(ts), statistics.median(tr), statistics.median(tf)
        staged = P.numel() * 4 + x1.numel() * 4
        out(f"  ivf_scorecam_stage, {B} rows   {spread(ts)}  {staged / ms / 1e6:8.1f} GB/s of compulsory bytes, "
            f"{2.0 * B * HW * gt * gh * gw / ms / 1e6:8.1f} GFLOP/s of the dense sums")
        out(f"  ivf_rise_stage, same grid      {spread(tr)}  (scorecam / rise: {ms / mr:.2f} x the time)")
        out(f"  forward of a {B}-row chunk      {spread(tf)}  staging is {100 * ms / mf:.2f} % of it")

        def scores():
            return eng.scorecam_scores(x1, tgt, F, None, "freeze")

        def whole():
            return eng.scorecam(x1, tgt, layer=layer)

        scores(), whole()
        torch.cuda.synchronize()
        tq = [event_ms(scores) for _ in range(args.reps)]
        tw = [event_ms(whole) for _ in range(max(args.reps // 2, 1))]
        out(f"  ivf_i3d_scorecam_scores, {nc + 1} rows  {spread(tq)}  {1e3 * (nc + 1) / statistics.median(tq):8.1f} rows/s")
        out(f"  scorecam() on one clip          {spread(tw)}  {statistics.median(tw) / 1e3:.3f} s per clip")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
