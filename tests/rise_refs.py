"""References for RISE random-mask saliency (csrc/rise_ops.hip): test_gpu_rise.py on the GPU,
test_rise_refs_host.py on the CPU.  Nothing here needs a GPU.

Mask family.  uint32 arithmetic restated in numpy uint64 masked to 32 bits:
    fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
    u(seed, k, c) = fmix32( fmix32(seed + 0x9E3779B9 (k + 1)) ^ (0x85EBCA77 (c + 1)) )
    S_k[c] = 1  iff  u(seed, k, c) < thresh,  thresh = floor(p 2^32), 0 < p < 1
Frame u of T belongs to temporal cell kt = (u gt) // T; c = (kt gh + i) gw + j.

Staging.  The contract is equality with ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit per-frame S, so the
GPU test needs no bound.

Reduction.  cells = (sum over the counted masks of d_k) / cnt in fp32, k ascending, against the same in fp64 from the
same fp32 inputs: the subtraction d_k = orig - s_k, cnt - 1 effective adds and one divide, each rounded once,
    b = (cnt + 2) 2^-24 sum |d_k| / cnt                                 (`reduce_ref`).
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h = h ^ (h >> np.uint64(16))
    return h


def hash_u(seed, k, c):
    """u(seed, k, c) as uint64 holding a uint32; k and c broadcast"""
    k = np.asarray(k, dtype=np.uint64)
    c = np.asarray(c, dtype=np.uint64)
    key = fmix32((np.uint64(seed) + np.uint64(0x9E3779B9) * (k + np.uint64(1))) & M32)
    return fmix32(key ^ ((np.uint64(0x85EBCA77) * (c + np.uint64(1))) & M32))


def thresh(p):
    """floor(p 2^32) for 0 < p < 1; ValueError at and beyond the edges (and where it would round to 0)"""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"p must be in (0, 1), got {p}")
    t = int(np.floor(p * 4294967296.0))
    if t < 1:
        raise ValueError(f"p = {p} is below 2^-32")
    return t


def bits(seed, p, n, cells, first_k=0):
    """bool [n, cells]: mask first_k + r freezes cell c"""
    k = np.arange(first_k, first_k + n, dtype=np.uint64)[:, None]
    c = np.arange(cells, dtype=np.uint64)[None, :]
    return hash_u(seed, k, c) < np.uint64(thresh(p))


def masks(seed, p, n, grid, first_k=0):
    """float32 [n, gt, gh, gw] of 0.0 / 1.0"""
    gt, gh, gw = grid
    return bits(seed, p, n, gt * gh * gw, first_k).reshape(n, gt, gh, gw).astype(np.float32)


def frame_cell(T, gt):
    """int64 [T]: temporal cell of every frame"""
    return (np.arange(T, dtype=np.int64) * gt) // T


def frame_masks(S, T):
    """per-frame grid masks [n, T, gh, gw] of S [n, gt, gh, gw]"""
    return S[:, frame_cell(T, S.shape[1])]


def reduce_ref(scores, orig, seed, p, grid):
    """fp64 estimator of scores [b,n], orig [b]: (cells [b,gt,gh,gw] (NaN where uncounted), count int64, mean_drop [b],
    bound [b,gt,gh,gw] on the fp32 cells)"""
    gt, gh, gw = grid
    s = np.asarray(scores, dtype=np.float64)
    b, n = s.shape
    Sb = bits(seed, p, n, gt * gh * gw)                              # [n, cells]
    d = np.asarray(orig, np.float64).reshape(b, 1) - s
    ok = ~np.isnan(s)
    d = np.where(ok, d, 0.0)
    use = ok[:, :, None] & Sb[None]                                  # [b, n, cells]
    cnt = use.sum(axis=1)
    sm = (d[:, :, None] * use).sum(axis=1)
    sab = (np.abs(d)[:, :, None] * use).sum(axis=1)
    nall = ok.sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        cells = np.where(cnt > 0, sm / cnt, np.nan)
        mean_drop = np.where(nall > 0, d.sum(axis=1) / nall, np.nan)
        bound = (cnt + 2) * 2.0 ** -24 * sab / np.maximum(cnt, 1)
    shape = (b, gt, gh, gw)
    return cells.reshape(shape), cnt.reshape(shape).astype(np.int64), mean_drop, bound.reshape(shape)


def planted_scores(seed, p, n, grid, weights, orig=0.9):
    """synthetic scores s_k = orig - sum_c w_c S_k[c] of one clip, [1, n] float64"""
    gt, gh, gw = grid
    Sb = bits(seed, p, n, gt * gh * gw).astype(np.float64)
    return (orig - Sb @ np.asarray(weights, np.float64))[None]
