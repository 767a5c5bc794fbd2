"""References for the deletion / insertion curves (csrc/curve_ops.hip): test_gpu_curves.py on the GPU,
test_curve_refs_host.py on the CPU.  Nothing here needs a GPU.

Players: the P = gt gh gw cells of a grid; frame u belongs to temporal cell (u gt) // T.

Rank.  order 0 (most relevant first): rank[c] = #{c' : a[c'] > a[c], or a[c'] == a[c] and c' < c}; order 1 flips > to <.
A NaN cell ranks after every number in either order, NaN cells among themselves by index; -0.0 == +0.0 is a tie.

Curves.  J = ceil(P / step), k_j = min(j step, P), j = 0 .. J.  Deletion row j freezes the cells with rank < k_j,
insertion row j those with rank >= k_j.  Rows of a call are flattened as [clip][curve][j]; `curves` is a bitmask (1
deletion, 2 insertion, 3 both, deletion first).  Staging is pinned by equality with ivf_stmask_expand_fwd +
ivf_stfreeze_fwd on the explicit per-frame S, so the GPU test needs no bound there.

Reduction.  auc = (1 / (2P)) sum_{j<J} (k_{j+1} - k_j) (s_j + s_{j+1}); auc_norm = (auc - s_lo) / (s_hi - s_lo), s_hi the
score of the clip and s_lo that of the fully frozen clip (deletion: rows 0 and J; insertion: rows J and 0).  The device
works in fp32 (u = 2^-24 per rounding): one add and one multiply by the exact integer width per interval, J - 1 adds of
the running sum and one division, at most J + 2 roundings on any term, so
    |auc^ - auc| <= B_a := 1.01 (J + 3) u (1 / (2P)) sum_j w_j (|s_j| + |s_{j+1}|)
(1.01 and the spare u cover the second order).  The normalisation subtracts and divides: with d = s_hi - s_lo exact in
fp64 from the same fp32 scores, and each of the device's subtract, subtract, divide rounding once,
    |norm^ - norm| <= B_n := (B_a + u |auc - s_lo| ) / |d| + 3 u |norm|            (first order, times 1.01)
The fp64 reference works from the same fp32 scores; its own error is ignored.

Pooling.  cell[u,i,j] = sum_yx A_H[y,i] A_W[x,j] a[u,y,x] / (sum_y A_H[y,i] sum_x A_W[x,j]); the numerator is the
device's ivf_stmask_expand_bwd (H W products and sums), the denominator fp64 rounded once to fp32, then one division:
    |cell^ - cell| <= (H W + T + 3) u sum|terms| / den
with `terms` the H W products of the numerator (the T covers the mean over at most T frames taken afterwards).
"""
import numpy as np

import shap_refs as SH

U = 2.0 ** -24


def ranks(a, order=0):
    """int64 [b, P] of a [b, P] (any float dtype): the definition by a stable sort -- numbers by value (descending for
    order 0), ties by index, NaN last."""
    a = np.asarray(a)
    if a.ndim == 1:
        return ranks(a[None], order)[0]
    b, P = a.shape
    v = a.astype(np.float64) + 0.0                      # -0.0 + 0.0 = +0.0: one zero
    nan = np.isnan(v)
    key = np.where(nan, 0.0, v if order else -v)
    # three levels, the last the most significant: (is NaN, key, index) -- +-inf are numbers and stay before every NaN
    idx = np.broadcast_to(np.arange(P), (b, P))
    order_idx = np.lexsort((idx, key, nan), axis=1)
    r = np.empty((b, P), np.int64)
    np.put_along_axis(r, order_idx, np.broadcast_to(np.arange(P, dtype=np.int64), (b, P)), axis=1)
    return r


def ranks_brute(a, order=0):
    """the definition, cell by cell (small P only); a [P]"""
    a = [float(v) for v in a]
    P = len(a)

    def before(o, c):
        if a[c] != a[c]:
            return a[o] == a[o] or o < c
        if a[o] != a[o]:
            return False
        first = a[o] < a[c] if order else a[o] > a[c]
        return first or (a[o] == a[c] and o < c)
    return [sum(1 for o in range(P) if o != c and before(o, c)) for c in range(P)]


def grid_cells(a, T, gt):
    """float32 [b, gt, gh, gw] of per-frame cells a [b, T, gh, gw]: the fp32 sum over the frames of the temporal cell in
    ascending u from 0, one division by the frame count (what curve_ranks_kernel does)."""
    a = np.asarray(a, np.float32)
    b, t_in, gh, gw = a.shape
    assert t_in == T
    kt = (np.arange(T) * gt) // T
    out = np.zeros((b, gt, gh, gw), np.float32)
    cnt = np.zeros(gt, np.float32)
    with np.errstate(invalid='ignore'):
        for u in range(T):
            out[:, kt[u]] = out[:, kt[u]] + a[:, u]
            cnt[kt[u]] += 1
        return out / cnt[None, :, None, None]


def thresholds(P, step):
    """k_j, j = 0 .. J"""
    J = -(-P // step)
    return np.minimum(np.arange(J + 1) * step, P)


def row_list(b, P, step, curves):
    """[(clip, ins, k)] of the flattened rows of a call"""
    ks = thresholds(P, step)
    kinds = {1: (0,), 2: (1,), 3: (0, 1)}[curves]
    return [(c, ins, int(k)) for c in range(b) for ins in kinds for k in ks]


def row_masks(rk, grid, rows):
    """float32 [len(rows), gt, gh, gw]: the binary S of rows [(clip, ins, k)] under the per-clip table rk [b,P]"""
    gt, gh, gw = grid
    rk = np.asarray(rk, np.int64)
    out = np.empty((len(rows), gt * gh * gw), np.float32)
    for n, (c, ins, k) in enumerate(rows):
        out[n] = (rk[c] >= k) if ins else (rk[c] < k)
    return out.reshape(len(rows), gt, gh, gw)


def frame_masks(S, T):
    return SH.frame_masks(S, T)


def auc_ref(scores, P, step, curves):
    """fp64 reduction of scores [b, ncurves, J+1].  Returns dict auc, auc_norm, bound_auc, bound_norm, all [b, ncurves]."""
    s = np.asarray(scores, np.float64)
    b, nc, J1 = s.shape
    ks = thresholds(P, step)
    assert J1 == len(ks) and nc == (2 if curves == 3 else 1)
    w = np.diff(ks).astype(np.float64)
    J = J1 - 1
    with np.errstate(invalid='ignore', divide='ignore'):
        auc = (w * (s[..., :-1] + s[..., 1:])).sum(axis=-1) / (2.0 * P)
        mag = (w * (np.abs(s[..., :-1]) + np.abs(s[..., 1:]))).sum(axis=-1) / (2.0 * P)
        ba = 1.01 * (J + 3) * U * mag
        ins = np.array({1: [0], 2: [1], 3: [0, 1]}[curves], bool)[None, :]
        hi = np.where(ins, s[..., J], s[..., 0])
        lo = np.where(ins, s[..., 0], s[..., J])
        d = hi - lo
        norm = np.where(d == 0, np.nan, (auc - lo) / d)
        bn = 1.01 * ((ba + U * np.abs(auc - lo)) / np.abs(d) + 3 * U * np.abs(norm))
    bad = np.isnan(s).any(axis=-1)
    auc = np.where(bad, np.nan, auc)
    norm = np.where(bad, np.nan, norm)
    return dict(auc=auc, auc_norm=norm, bound_auc=ba, bound_norm=bn)


def pool_ref(a, AH, AW):
    """fp64 footprint-weighted mean of a [b,T,H,W] on the fp32 matrices AH [H,gh], AW [W,gw]: (cells [b,T,gh,gw], sum of
    |terms| / den, den [gh,gw] in fp64)."""
    a = np.asarray(a, np.float64)
    AH, AW = np.asarray(AH, np.float64), np.asarray(AW, np.float64)
    den = AH.sum(axis=0)[:, None] * AW.sum(axis=0)[None, :]
    num = np.einsum('yi,btyx,xj->btij', AH, a, AW)
    mag = np.einsum('yi,btyx,xj->btij', np.abs(AH), np.abs(a), np.abs(AW))
    return num / den, mag / den, den


def random_baseline(shap_scores):
    """expected random curves from Shapley rows [b,n,P+1]: float64 [b,2,P+1] = (mean_k s[k][j], mean_k s[k][P-j])"""
    s = np.asarray(shap_scores, np.float64)
    m = s.mean(axis=1)
    return np.stack([m, m[:, ::-1]], axis=1)
