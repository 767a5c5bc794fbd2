"""The Grad-CAM family against the Grad-CAM reduction on one MI355X.

    python tools/cam_bench.py [--batch 32] [--reps 15] [--call-reps 3] [--out profiles/cam_family_bench.txt]

Setting: the 16 x 224 x 224 I3D clip at the bench's batch, targets Conv3d_1a_7x7, Mixed_3c, Mixed_5c, on the
activations and gradients a Grad-CAM call of the plan leaves (fp32 copies, and the same values rounded to bf16 for
the bf16 entry points).  All in one run, device events, medians after warm-up:

1. ivf_gradcam_reduce (untouched) beside ivf_cam_reduce for every single kind and for the four new kinds together,
   with the compulsory bytes of each -- sizeof(feat) and sizeof(grad) times the passes the kinds need -- and the
   bandwidth that gives.
2. the whole `cam` call (five kinds) beside the whole `gradcam` call.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "interpreting-video-features_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import ivf_lib as L  # noqa: E402
import ivf_recipe as R  # noqa: E402
from blob_bench import engine, median_ms  # noqa: E402

KINDS = ("gradcam", "gradcam++", "xgradcam", "hirescam", "layercam")
# passes over (feat, grad) of a set of kinds: the s_k pass reads feat (and grad for XGrad-CAM's numerator), the
# Grad-CAM++ pass reads grad, the map pass reads feat (and grad for HiResCAM / LayerCAM); Grad-CAM reads each once
PASSES = {"gradcam": (1, 1), "gradcam++": (2, 1), "xgradcam": (2, 1), "hirescam": (1, 1), "layercam": (1, 1),
          "the four new": (2, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--call-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    B = args.batch
    eng, choice = engine("s16", B)
    x = torch.stack([torch.from_numpy(R.clip(21 + i)) for i in range(B)]).cuda()
    tgt = eng.argmax(eng.forward(x))
    lib, st = L.lib(), L.stream
    out(f"# tools/cam_bench.py on {torch.cuda.get_device_properties(0).name}, S16 B={B}, math {eng.math}, kernel choice: "
        f"{choice}; medians of {args.reps} launches / {args.call_reps} calls (device events), one run")
    for layer in ("Conv3d_1a_7x7", "Mixed_3c", "Mixed_5c"):
        raw = eng.cam_raw(x, tgt, kinds=("gradcam",), layer=layer)
        feat, grad = raw["feat"], raw["grad"]
        b, Tf, Hf, Wf, C = feat.shape
        npos = Tf * Hf * Wf
        del raw
        out(f"## {layer}: feat, grad [{b}, {npos}, {C}]")
        for storage in ("fp32", "bf16"):
            f = feat if storage == "fp32" else feat.to(torch.bfloat16)
            g = grad if storage == "fp32" else grad.to(torch.bfloat16)
            esz = f.element_size()
            nbytes = f.numel() * esz
            ws = torch.empty(lib.ivf_cam_ws_bytes(b, npos, C), dtype=torch.uint8, device="cuda")
            w = torch.empty(5, b, C, device="cuda")
            cam = torch.empty(5, b, npos, device="cuda")
            old_fn = lib.ivf_gradcam_reduce if storage == "fp32" else lib.ivf_gradcam_reduce_bf16
            new_fn = lib.ivf_cam_reduce if storage == "fp32" else lib.ivf_cam_reduce_bf16

            def old():
                L.check(old_fn(L.ptr(f), L.ptr(g), L.ptr(w), L.ptr(cam), b, npos, C, st()))

            def new(ids, n):
                return lambda: L.check(new_fn(L.ptr(f), L.ptr(g), n, ids, L.ptr(w), L.ptr(cam), L.ptr(ws), b, npos, C, st()))
            rows = [("ivf_gradcam_reduce (as before)", "gradcam", old)]
            for k in KINDS:
                rows.append((f"ivf_cam_reduce {k}", k, new(L.cam_kind_ids((k,))[1], 1)))
            rows.append(("ivf_cam_reduce the four new kinds", "the four new", new(L.cam_kind_ids(KINDS[1:])[1], 4)))
            t_old = None
            for name, key, fn in rows:
                t = median_ms(fn, args.reps)
                t_old = t if t_old is None else t_old
                pf, pg = PASSES[key]
                comp = (pf + pg) * nbytes
                out(f"{storage} {name:36s} {t * 1e3:10.1f} us  {comp / 2**20:9.1f} MiB compulsory ({pf} x feat + {pg} x grad)"
                    f"  {comp / t / 1e6:8.1f} GB/s  {t / t_old:6.2f} x the old reduction")
            del f, g, ws, w, cam
        del feat, grad
        t_g = median_ms(lambda: eng.gradcam(x, tgt, layer=layer), args.call_reps, warmup=1)
        t_c = median_ms(lambda: eng.cam(x, tgt, kinds=KINDS, layer=layer), args.call_reps, warmup=1)
        out(f"whole call: gradcam {t_g:9.2f} ms, cam (five kinds) {t_c:9.2f} ms, {t_c - t_g:+.2f} ms = "
            f"{100 * (t_c - t_g) / t_g:+.2f} %")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
