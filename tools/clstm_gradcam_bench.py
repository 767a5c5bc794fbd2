"""Grad-CAM of the ConvLSTM backbone against forward + full backward of the same plan, on one MI355X.

    python tools/clstm_gradcam_bench.py [--reps 25] [--batch 32] [--out FILE]

KTH geometry (3 x 32 x 120 x 160, 2 layers, hidden 4, stride 2, effective steps 7/15/23/31), recipe weights.
Device-event time of one call, alternated round-robin over the five candidates so that clock drift hits all of
them alike, median of --reps each after a warm-up:
  forward                  ivf_clstm_forward
  forward + backward       ivf_clstm_forward + ivf_clstm_backward (full BPTT down to the clip): the yardstick
  gradcam 'clstm'          target (A): head backward only, 4 maps
  gradcam 'cell1'          target (B), top layer: head backward only, 32 maps
  gradcam 'cell0'          target (B), layer 0: the top layer's BPTT as well
Every gradcam call includes its own forward, the reduction and the resize to 120 x 160.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "interpreting-video-features_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivf_engine  # noqa: E402
import ivf_recipe as R  # noqa: E402

EFF = [7, 15, 23, 31]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B = args.batch
    eng = ivf_engine.CLSTMEngine(6, (3, 32, 120, 160), max_batch=B, hidden=4, layers=2, kernel=5, stride=2,
                                 softmax=True, out_step=31, effective_steps=EFF)
    eng.load_state_dict(R.clstm_state_dict(channels=3, tag='clstm3'))
    x = torch.from_numpy(np.stack([R.clip(i, 3, 32, 120, 160) / 255.0 for i in range(B)])).float().cuda()
    tgt = eng.argmax(eng.forward(x))

    def fwd_bwd():
        eng.forward(x)
        eng.backward(B, target=tgt)
    cands = [
        ("forward", lambda: eng.forward(x)),
        ("forward + backward", fwd_bwd),
        ("gradcam 'clstm' (A)", lambda: eng.gradcam(x, tgt, out_hw=(120, 160))),
        ("gradcam 'cell1' (B, top)", lambda: eng.gradcam(x, tgt, out_hw=(120, 160), layer=1)),
        ("gradcam 'cell0' (B, layer 0)", lambda: eng.gradcam(x, tgt, out_hw=(120, 160), layer=0)),
    ]
    for _ in range(3):
        for _, fn in cands:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cands}
    for _ in range(args.reps):
        for name, fn in cands:
            times[name].append(event_ms(fn))
    base = statistics.median(times["forward + backward"])
    lines = [f"ConvLSTM Grad-CAM, KTH geometry, B = {B}, {torch.cuda.get_device_name(0)}, median of {args.reps} "
             f"(min .. max), ms per call of {B} clips"]
    for name, _ in cands:
        t = times[name]
        m = statistics.median(t)
        lines.append(f"  {name:30s} {m:8.3f}  ({min(t):.3f} .. {max(t):.3f})   {m / base:5.2f} x forward + backward")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
