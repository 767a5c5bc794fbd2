#!/usr/bin/env python3
"""Generate tests/golden/ig.npz: Integrated Gradients by torch autograd on the REFERENCE's own
I3D_doubled.Model with the recipe weights.  Run where make_golden.py runs:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ig.py

IG has no counterpart in the reference; what is pinned is the gradient of the reference's model along the path, the
semantics (tests/ig_refs.py restates them) and the quadrature.  Clips 21 and 7, K = 8 midpoint nodes, baselines
'frozen' (every frame = frame 0) and 'black' (constant 0.0), target = the model's argmax on the clip.  The map is
stored at make_golden.sample_idx positions; frames, abs_frames, totals and endpoint scores whole.  Three legs, as
make_golden.gen_search_spread: fp32 / 8 threads (the fixture proper), fp64, and fp32 / 4 threads (another summation
order inside torch's convolutions) -- the distance between them is the noise floor the GPU gates are set against.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG          # noqa: E402  (binds the reference's modules and the recipe)

R = MG.R
CLIPS = (21, 7)
K = 8
BASELINES = ('frozen', 'black')
LEGS = (('', torch.float32, 8), ('f64_', torch.float64, 8), ('f32t4_', torch.float32, 4))


def ig_run(model, x, target, baseline, dtype):
    """x [1,C,T,H,W] in `dtype`.  The semantics of DESIGN 13 with the arithmetic of `dtype` throughout."""
    x0 = x[:, :, :1].expand_as(x).clone() if baseline == 'frozen' else torch.zeros_like(x)
    alpha = ((2.0 * np.arange(K, dtype=np.float32) + np.float32(1.0)) / np.float32(2 * K)).astype(np.float32)
    w = np.full(K, np.float32(1.0) / np.float32(K), dtype=np.float32)
    gsum = torch.zeros_like(x)
    path = []
    for k in range(K):
        p = (x0 + float(alpha[k]) * (x - x0)).detach().requires_grad_()
        s = model(p)[0, target]
        s.backward()
        gsum += float(w[k]) * p.grad
        path.append(float(s))
    A = ((x - x0) * gsum)[0].double().numpy()                   # [C,T,H,W]
    with torch.no_grad():
        score_x = float(model(x)[0, target])
        score_base = float(model(x0)[0, target])
    ig_map = A.sum(0)                                           # [T,H,W]
    frames = ig_map.sum((1, 2))
    return dict(map=ig_map, frames=frames, abs_frames=np.abs(A).sum((0, 2, 3)), total=frames.sum(),
                score_x=score_x, score_base=score_base, path_scores=np.array(path))


def gen_ig():
    out = {'K': np.array(K), 'clips': np.array(CLIPS)}
    for leg, dtype, threads in LEGS:
        torch.set_num_threads(threads)
        torch.set_default_dtype(dtype)
        try:
            m = MG._i3d(False).to(dtype)
            for p in m.parameters():
                p.requires_grad_(False)
            for cid in CLIPS:
                x = torch.from_numpy(R.clip(cid))[None].to(dtype)
                if leg == '':
                    with torch.no_grad():
                        out[f'c{cid}_target'] = np.array(int(torch.argmax(m(x)[0])))
                target = int(out[f'c{cid}_target'])
                for bl in BASELINES:
                    r = ig_run(m, x, target, bl, dtype)
                    tag = f'{leg}c{cid}_{bl}'
                    idx = MG.sample_idx(f'g/ig/{cid}/{bl}', r['map'].size, 4096)
                    if leg == '':
                        out[f'{tag}_map_idx'] = idx
                    out[f'{tag}_map_val'] = r['map'].ravel()[idx]
                    for key in ('frames', 'abs_frames', 'total', 'score_x', 'score_base', 'path_scores'):
                        out[f'{tag}_{key}'] = np.asarray(r[key], dtype=np.float64)
                    print(tag, 'total', r['total'], 'f(x)-f(x0)', r['score_x'] - r['score_base'], 'sum|A|',
                          r['abs_frames'].sum(), flush=True)
                    MG.save('ig', **out)
        finally:
            torch.set_default_dtype(torch.float32)
            torch.set_num_threads(8)


if __name__ == '__main__':
    gen_ig()
