"""References for Score-CAM (csrc/scorecam_ops.hip): test_gpu_scorecam.py on the GPU,
test_scorecam_refs_host.py on the CPU.  Nothing here needs a GPU.

Normalise.  Per (clip, channel) lo = min A, hi = max A (order-free, so exact; a zero is written as +0.0, a plane with a
NaN gives NaN for both), valid = lo, hi finite and hi > lo, F = (hi - A) / (hi - lo): two fp32 subtractions and one
correctly rounded fp32 division per element, which numpy float32 restates operation for operation (`normalise`); F = 1
where the channel is not valid.  The contract is bit-equality.

Staging.  The contract is equality with ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit per-frame S of a row
(`frame_planes`: S[u] = F[kt(u)], kt = (u gt) // T), so the GPU test needs no bound; 'blank' rows are the torch
expression (1 - M) x, two fp32 operations, on the same M.

Reduce.  d_k = s_k - s_nc is ONE fp32 subtraction: 'increase' weights are bit-equal to numpy float32 (`weights_increase`).
The cam is compared with fp64 computed from the DEVICE's own fp32 weights: per position nc products, each rounded once,
and nc - 1 adds, each rounded once (a fixed order, no contraction), so by the standard recursive-summation bound
    |cam32 - cam64| <= (nc + 2) 2^-24 sum_k |w_k A_k|                    (`cam_ref`; relu is 1-Lipschitz).
'softmax' weights are compared with the fp64 softmax of the same fp32 d_k (`weights_softmax`).  The device computes
e_k = expf(fl(d_k - d_max)), S = sum_k e_k (k ascending, fp32) and e_k / S.  Relative errors, first order, u = 2^-24:
    the argument: one fp32 subtraction, absolute error <= u |d_k - d_max|, which exp turns into the same relative error;
    expf itself: EXPF_ULP ulp = EXPF_ULP 2^-23.  ROCm's device-library documentation is not installed beside the
        compiler here; the figure is the one the device library is built to, the OpenCL C specification's table of
        minimum accuracy (exp: <= 3 ulp), which also covers the HIP math API reference's own figure for expf (1 ulp);
    so every e_k is within eps_e = EXPF_ULP 2^-23 + u max_k |d_k - d_max| of exp(d_k - d_max);
    the sum of nc positive terms: eps_e from its terms plus (nc - 1) u from its adds; the division: u.
    w_k relative <= 2 eps_e + (nc + 1) u, times 1.01 for the second-order terms (nc <= 1024: (nc u)^2 << 1e-2 nc u).
Nothing in these bounds comes from a run of the kernels.
"""
import numpy as np

EXPF_ULP = 3.0
U = 2.0 ** -24
NAN32 = np.float32(np.nan)


def frame_cell(T, gt):
    """int64 [T]: temporal cell of every frame"""
    return (np.arange(T, dtype=np.int64) * gt) // T


def frame_planes(F, T):
    """per-frame grid masks [..., T, gh, gw] of planes F [..., gt, gh, gw]"""
    F = np.asarray(F)
    return np.take(F, frame_cell(T, F.shape[-3]), axis=-3)


def normalise(A):
    """A [b,nc,...] float32 -> (lo, hi [b,nc] float32, valid [b,nc] bool, F like A float32), operation for operation"""
    A = np.asarray(A, dtype=np.float32)
    b, nc = A.shape[:2]
    flat = A.reshape(b, nc, -1)
    with np.errstate(invalid='ignore'):
        nan = np.isnan(flat).any(axis=2)
        lo = np.where(nan, NAN32, np.nanmin(np.where(np.isnan(flat), np.float32(np.inf), flat), axis=2) + np.float32(0))
        hi = np.where(nan, NAN32, np.nanmax(np.where(np.isnan(flat), np.float32(-np.inf), flat), axis=2) + np.float32(0))
        lo, hi = lo.astype(np.float32), hi.astype(np.float32)
        valid = np.isfinite(lo) & np.isfinite(hi) & (hi > lo)
        rng = (hi - lo).astype(np.float32)
        F = ((hi[:, :, None] - flat).astype(np.float32) / np.where(valid, rng, np.float32(1))[:, :, None]).astype(np.float32)
    F = np.where(valid[:, :, None], F, np.float32(1)).astype(np.float32)
    return lo, hi, valid, F.reshape(A.shape)


def counting(scores, valid):
    """(d [b,nc] float32 = s_k - s_nc in one fp32 subtraction, ok [b,nc] bool: valid and d not NaN)"""
    s = np.asarray(scores, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        d = (s[:, :-1] - s[:, -1:]).astype(np.float32)
    return d, np.asarray(valid).astype(bool) & ~np.isnan(d)


def weights_increase(scores, valid):
    """float32 [b,nc]: d_k where the channel counts, else +0.0 -- the device's bits"""
    d, ok = counting(scores, valid)
    return np.where(ok, d, np.float32(0)).astype(np.float32)


def weights_softmax(scores, valid):
    """(w [b,nc] float64: the softmax over the counting channels of the fp32 d_k, 0 elsewhere; rel [b]: the relative
    bound on the device's fp32 weights)"""
    d, ok = counting(scores, valid)
    d64 = np.where(ok, d.astype(np.float64), -np.inf)
    dmax = d64.max(axis=1, keepdims=True)
    with np.errstate(invalid='ignore'):
        e = np.where(ok, np.exp(d64 - np.where(np.isfinite(dmax), dmax, 0.0)), 0.0)
    tot = e.sum(axis=1, keepdims=True)
    w = np.where(ok, e / np.where(tot > 0, tot, 1.0), 0.0)
    nc = d.shape[1]
    with np.errstate(invalid='ignore'):
        spread = np.where(ok, np.abs(d64 - dmax), 0.0).max(axis=1)
    eps_e = EXPF_ULP * 2.0 ** -23 + U * spread
    return w, 1.01 * (2.0 * eps_e + (nc + 1) * U)


def cam_ref(w, A):
    """w [b,nc] (the DEVICE's fp32 weights), A [b,nc,...] float32 -> (cam float64 [b,...], bound [b,...]); channels of
    weight 0 are left out (a plane that is not finite belongs to a channel that is not valid, whose weight is 0)"""
    w64 = np.asarray(w, dtype=np.float64)
    A64 = np.asarray(A, dtype=np.float64)
    b, nc = w64.shape
    shape = (b, nc) + (1,) * (A64.ndim - 2)
    with np.errstate(invalid='ignore'):
        terms = np.where(w64.reshape(shape) != 0.0, w64.reshape(shape) * A64, 0.0)
    return np.maximum(terms.sum(axis=1), 0.0), (nc + 2) * U * np.abs(terms).sum(axis=1)


def torch_normalise(A):
    """the same normalise written with torch float32 ops (test_scorecam_refs_host.py holds the two against each other)"""
    import torch
    A = torch.as_tensor(np.asarray(A, np.float32))
    flat = A.reshape(A.shape[0], A.shape[1], -1)
    lo, hi = flat.amin(dim=2) + 0.0, flat.amax(dim=2) + 0.0          # amin / amax propagate NaN
    valid = torch.isfinite(lo) & torch.isfinite(hi) & (hi > lo)
    F = (hi[:, :, None] - flat) / torch.where(valid, hi - lo, torch.ones_like(lo))[:, :, None]
    F = torch.where(valid[:, :, None], F, torch.ones_like(F))
    return lo.numpy(), hi.numpy(), valid.numpy(), F.reshape(A.shape).numpy()
