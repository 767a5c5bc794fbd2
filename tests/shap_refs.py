"""References for Shapley value sampling (csrc/shapley_ops.hip): test_gpu_shapley.py on the GPU,
test_shap_refs_host.py on the CPU.  Nothing here needs a GPU.

Permutation family.  With u(seed, k, c) the uint32 hash of tests/rise_refs.py and P = gt gh gw players,
    rank_k[c] = #{c' : (u(seed,k,c'), c') < (u(seed,k,c), c)}              (lexicographic: a tie falls to the lower index)
and, antithetic, an odd k is permutation k - 1 (hashed as itself) reversed: rank_k[c] = P - 1 - rank_{k-1}[c].
Row j = 0 .. P of permutation k freezes the cells with rank_k[c] < j.

Staging.  The contract is equality with ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit per-frame S, so the
GPU test needs no bound.

Reduction, u = 2^-24 (fp32 unit roundoff; the device's subtract, add, multiply, divide and sqrtf each round once,
correctly).  The fp64 reference works from the same fp32 scores; its own error (2^-53 relative) is ignored.

cells.  d_k = s[k][r] - s[k][r+1] rounded once, cnt - 1 adds, one divide, as rise_refs:
    B_c = (cnt + 2) u sum|d_k| / cnt.
total is the same expression over the permutations with finite end scores: B_t = (nall + 2) u sum|s[k][0] - s[k][P]| / nall.

stderr = sqrt(SS / (cnt - 1) / cnt), SS = sum_k e_k^2, e_k = d_k - phi (fp64), second pass in the same order.
 1. The device forms e^_k = fl(d^_k - phi^) with |d^_k - d_k| <= u |d_k| and |phi^ - phi| <= B_c, so
        |e^_k - e_k| <= eta_k := u (|d_k| + |e_k|) + B_c            (first order; the u^2 terms are covered in step 3)
    and, as vectors over the cnt terms, ||e^|| <= E + H with E = ||e||_2 = sqrt(SS), H = ||eta||_2.
 2. SS^ = sum_k e^_k^2 (1 + theta_k): one rounding of the square and at most cnt - 1 of the adds, |theta_k| <= cnt u.
    Hence sqrt(SS^) lies within (E + H) (1 + cnt u / 2) above and (E - H) (1 - cnt u / 2) below:
        |sqrt(SS^) - E| <= H + (E + H) cnt u / 2.
 3. Two divides under the root and the root itself: three more roundings, the two under the root halved by it: a
    relative 2 u.  One further u covers every second-order term above (cnt u << 1 for cnt <= 2^20).  With
    D = sqrt(cnt (cnt - 1)):
        B_s = ( H + (E + H) (cnt / 2 + 3) u ) / D.
    B_s does not vanish with E: where all d_k are equal the fp64 stderr is 0, but phi^ may be a rounding off d_k and
    the device's deviations are then of the order of B_c -- the H term.
"""
import numpy as np

import rise_refs as RR

U = 2.0 ** -24


def ranks(seed, n, P, antithetic=True, first_k=0):
    """int64 [n, P]: rank of cell c in permutation first_k + r"""
    k = np.arange(first_k, first_k + n, dtype=np.int64)
    base = np.where((k & 1).astype(bool) & bool(antithetic), k - 1, k)
    h = RR.hash_u(seed, base.astype(np.uint64)[:, None], np.arange(P, dtype=np.uint64)[None, :])      # [n, P]
    order = np.lexsort((np.broadcast_to(np.arange(P), h.shape), h), axis=1)      # hash first, then the index
    r = np.empty((n, P), np.int64)
    np.put_along_axis(r, order, np.broadcast_to(np.arange(P, dtype=np.int64), (n, P)), axis=1)
    rev = (k & 1).astype(bool) & bool(antithetic)
    r[rev] = P - 1 - r[rev]
    return r


def ranks_brute(seed, k, P, antithetic=True):
    """the definition, cell by cell (small P only)"""
    base = k - 1 if (antithetic and k % 2) else k
    h = [int(RR.hash_u(seed, base, c)) for c in range(P)]
    r = [sum(1 for o in range(P) if (h[o], o) < (h[c], c)) for c in range(P)]
    return [P - 1 - v for v in r] if base != k else r


def row_masks(rk_table, grid, rows):
    """float32 [len(rows), gt, gh, gw]: the masks of rows (numbers inside ONE clip's n (P+1) list) of rk_table [n,P]"""
    gt, gh, gw = grid
    P = gt * gh * gw
    rows = np.asarray(rows, np.int64)
    k, j = rows // (P + 1), rows % (P + 1)
    return (rk_table[k] < j[:, None]).reshape(len(rows), gt, gh, gw).astype(np.float32)


def frame_masks(S, T):
    """per-frame grid masks [n, T, gh, gw] of S [n, gt, gh, gw]"""
    return RR.frame_masks(S, T)


def reduce_ref(scores, rk):
    """fp64 estimator of scores [b,n,P+1] with the rank table rk [n,P].  Returns a dict of [b,P] arrays cells, stderr,
    count (int64), bound_cells, bound_stderr and [b] arrays total, bound_total, nall."""
    s = np.asarray(scores, dtype=np.float64)
    b, n, P1 = s.shape
    P = P1 - 1
    rk = np.asarray(rk, np.int64)
    assert rk.shape == (n, P)
    kk = np.arange(n)[:, None]
    a, z = s[:, kk, rk], s[:, kk, rk + 1]                             # [b, n, P]
    ok = ~(np.isnan(a) | np.isnan(z))
    d = np.where(ok, a - z, 0.0)
    cnt = ok.sum(axis=1)
    sab = np.abs(d).sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        phi = np.where(cnt > 0, d.sum(axis=1) / cnt, np.nan)
        e = np.where(ok, d - phi[:, None, :], 0.0)
        SS = (e * e).sum(axis=1)
        D = np.sqrt(cnt * (cnt - 1.0))
        se = np.where(cnt >= 2, np.sqrt(SS) / D, np.nan)
        bc = (cnt + 2) * U * sab / np.maximum(cnt, 1)
        eta = np.where(ok, U * (np.abs(d) + np.abs(e)) + bc[:, None, :], 0.0)
        H, E = np.sqrt((eta * eta).sum(axis=1)), np.sqrt(SS)
        bs = np.where(cnt >= 2, (H + (E + H) * (cnt / 2.0 + 3.0) * U) / D, np.nan)
        fin = np.isfinite(s[:, :, 0]) & np.isfinite(s[:, :, P])
        dt = np.where(fin, s[:, :, 0] - s[:, :, P], 0.0)
        nall = fin.sum(axis=1)
        total = np.where(nall > 0, dt.sum(axis=1) / nall, np.nan)
        bt = (nall + 2) * U * np.abs(dt).sum(axis=1) / np.maximum(nall, 1)
    return dict(cells=phi, stderr=se, count=cnt.astype(np.int64), bound_cells=bc, bound_stderr=bs, total=total,
                bound_total=bt, nall=nall)


def additive_scores(rk, w, orig):
    """scores [1, n, P+1] of the additive game s(S) = orig - sum_{c in S} w_c along the permutations rk [n,P]: prefix j
    has the cells of rank < j frozen.  float64; exact where orig and w are multiples of one power of two."""
    rk = np.asarray(rk, np.int64)
    n, P = rk.shape
    w = np.asarray(w, np.float64)
    by_rank = np.empty((n, P))
    np.put_along_axis(by_rank, rk, np.broadcast_to(w, (n, P)), axis=1)             # by_rank[k][rank] = w of that cell
    out = np.empty((1, n, P + 1))
    out[0, :, 0] = orig
    out[0, :, 1:] = orig - np.cumsum(by_rank, axis=1)
    return out


def gated_cells_slack(scores, rk, gate, floor):
    """What an error of `gate` on every score, each against its own magnitude (|s^ - s| <= gate max(|s|, floor), the
    form of conftest.rel_err_elem), can move the fp64 cells by: each of the cnt terms d_k = s[k][r] - s[k][r+1] carries
    two gated scores, so |d^_k - d_k| <= gate (m[k][r] + m[k][r+1]) with m = max(|s|, floor), and
    |phi^ - phi| <= gate sum_k (m[k][r] + m[k][r+1]) / cnt.  [b,P]; for scores without NaN (cnt = n)."""
    m = np.maximum(np.abs(np.asarray(scores, dtype=np.float64)), floor)
    b, n, P1 = m.shape
    rk = np.asarray(rk, np.int64)
    kk = np.arange(n)[:, None]
    return gate * (m[:, kk, rk] + m[:, kk, rk + 1]).sum(axis=1) / n


def frames_sum_bound(cells, grid):
    """|sum_u shap_frames[u] - sum_c cells[c]| of fp32 shap_frames against the fp64 sum of the same fp32 cells, [b].  A
    frame's value is the spatial sum of its temporal cell by the expand with unit weights (the products are exact; gw - 1
    adds per grid row and gh - 1 over the rows, at most gh gw - 1 roundings on any term), times the fp32 reciprocal of
    the cell's frame count (one rounding), the product rounded once: at most gh gw + 1 roundings, each relative to the
    magnitudes summed; the frames of a cell then share its sum as counted."""
    gt, gh, gw = grid
    a = np.abs(np.asarray(cells, np.float64)).reshape(len(cells), -1).sum(axis=1)
    return (gh * gw + 1) * U * a
