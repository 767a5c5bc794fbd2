"""References for the linear surrogates, KernelSHAP and LIME (csrc/linsur_ops.hip): test_gpu_linsur.py on
the GPU, test_linsur_refs_host.py on the CPU.  Nothing here needs a GPU.

Rows.  P = gt gh gw players, z_kc = 1: sample row k freezes cell c; u the uint32 hash of tests/rise_refs.py, rank_k the
table of tests/shap_refs.py.
  KernelSHAP  h_k = u(seed, base_k, P) (the cell index the rank hashes never use), s_k = 1 + #{i : h_k >= size_table[i]},
              size_table[i-1] = floor(2^32 CDF(i)), i = 1 .. P-2, CDF that of q(s) ~ 1 / (s (P-s)) on 1 .. P-1 by an fp64
              cumsum; row k freezes the cells with rank_k[c] < s_k.  paired: an odd k has base_k = k-1, the rank reversed
              and s_k = P - s_{k-1}: the complement of row k-1.
  LIME        z_kc = u(seed, k, c) < thresh: the bits of ivf_rise_masks.
Packed: bits [n, ceil(P/32)] uint32, bit c % 32 of word c / 32, unused high bits zero.

Moments (fp64, every element one chain in ascending k, a product rounded before it is added; numpy neither fuses nor
reorders an elementwise a += b): with y_bk = (double)score_x[b] - (double)scores[b,k] and w_k = wtab[popcount(row k)]
(no table: 1),
  N[c,c'] = sum_k w_k [z_kc & z_kc'], v[c] = sum_k w_k z_kc, Wsum = sum_k w_k, r[b,c] = sum_k fl(w_k y_bk) z_kc,
  t[b] = sum_k fl(w_k y_bk);
a row that does not set a bit adds nothing (so a NaN score stays inside its own clip).  The device's moments are these
to the bit.  With w = 1 every partial sum of N is an integer below 2^53, exact in any order: `moments(..., exact_N=True)`
then takes N from one matrix product, which the loop would give bit for bit (test_linsur_refs_host.py compares them).

Systems.  KernelSHAP, l = P-1, total_b = score_x[b] - scores[b,n] in fp64:
  A[c,c'] = ((N[c,c'] - N[c,l]) - N[l,c']) + N[l,l],  rhs[b,c] = (r[b,c] - r[b,l]) - total_b (N[c,l] - N[l,l]),
  phi_l = total_b - sum_{c<l} phi_c, intercept 0.
LIME, mu = v / Wsum:
  G[c,c'] = (N[c,c'] - Wsum (mu_c mu_c')) + ridge [c == c'],  rhs[b,c] = r[b,c] - mu_c t_b,
  intercept = t_b / Wsum - sum_c mu_c phi_c.
Both are assembled here in the device's order of operations, so the device solves the very same fp64 system.

Accurate solution phi*: numpy's solve plus two steps of iterative refinement with the residual in np.longdouble;
e_ref = max |phi_numpy - phi*| is the fp64 error of the reference solve itself.  The gate of the device's fp32 cells is
  |phi_dev - phi*| <= 2^-24 |phi*| + 8 e_ref
(the one fp32 rounding of the output, and a factor for a summation order that is not LAPACK's).

Singularity: a Cholesky pivot d_j <= 2^-20 A_jj (A_jj the entry before the factorisation) or a pivot that is not
finite.  `chol_pivots` factors unblocked; the regular and the singular sampled systems lie decades away from 2^-20 on
either side, so the blocking of the device's factorisation does not move a system across.
"""
import numpy as np

import rise_refs as RR
import shap_refs as SH

PIVOT_TOL = 2.0 ** -20
LIN_MAX_PLAYERS = 1024


# ---------------------------------------------------------------------------------------------------- rows
def size_table(P):
    """uint32 [P-2]: floor(2^32 CDF(i)), i = 1 .. P-2"""
    s = np.arange(1, P, dtype=np.float64)
    c = np.cumsum(1.0 / (s * (P - s)))
    return np.floor(4294967296.0 * (c[:P - 2] / c[-1])).astype(np.uint32)


def _base(k, paired):
    odd = (k & 1).astype(bool) & bool(paired)
    return np.where(odd, k - 1, k), odd


def kshap_sizes(seed, n, P, paired=True, first_k=0):
    """int64 [n]: the coalition size of rows first_k .. first_k + n - 1"""
    k = np.arange(first_k, first_k + n, dtype=np.int64)
    base, odd = _base(k, paired)
    h = RR.hash_u(seed, base.astype(np.uint64), np.uint64(P))
    s = 1 + (h[:, None] >= size_table(P).astype(np.uint64)[None, :]).sum(axis=1)
    return np.where(odd, P - s, s).astype(np.int64)


def kshap_rows(seed, n, P, paired=True, first_k=0):
    """(Z bool [n,P], sizes int64 [n])"""
    s = kshap_sizes(seed, n, P, paired, first_k)
    return SH.ranks(seed, n, P, paired, first_k) < s[:, None], s


def kshap_row_brute(seed, k, P, paired=True):
    """the definition, cell by cell (small P only): (row as a list of 0 / 1, size)"""
    base = k - 1 if (paired and k % 2) else k
    h = int(RR.hash_u(seed, base, P))
    s = 1 + sum(1 for v in size_table(P).tolist() if h >= v)
    if base != k:
        s = P - s
    rk = SH.ranks_brute(seed, k, P, paired)
    return [1 if r < s else 0 for r in rk], s


def lime_rows(seed, thresh, n, P, first_k=0):
    """bool [n,P]: u(seed, k, c) < thresh"""
    k = np.arange(first_k, first_k + n, dtype=np.uint64)[:, None]
    return RR.hash_u(seed, k, np.arange(P, dtype=np.uint64)[None, :]) < np.uint64(thresh)


def pack(Z):
    """uint32 [n, ceil(P/32)] of Z bool [n,P]"""
    Z = np.asarray(Z, bool)
    n, P = Z.shape
    nw = (P + 31) // 32
    pad = np.zeros((n, nw * 32), np.uint64)
    pad[:, :P] = Z
    return (pad.reshape(n, nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack(bits, P):
    bits = np.asarray(bits).astype(np.uint32)
    return (((bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(len(bits), -1)[:, :P]).astype(bool)


def row_masks(Z, grid, rows):
    """float32 [len(rows), gt, gh, gw]: the masks of rows (numbers inside ONE clip's n + 1 list; row n: all frozen)"""
    gt, gh, gw = grid
    Zall = np.concatenate([np.asarray(Z, bool), np.ones((1, Z.shape[1]), bool)])
    return Zall[np.asarray(rows, np.int64)].reshape(len(rows), gt, gh, gw).astype(np.float32)


def lime_wtab(P, width=0.25):
    """fp64 [P+1]: exp(-D^2 / (2 width^2)), D = 1 - sqrt((P - m) / P): lime_image's cosine distance of a binary row
    with m cells switched off to the all-ones row, under its exponential kernel"""
    m = np.arange(P + 1, dtype=np.float64)
    D = 1.0 - np.sqrt((P - m) / P)
    return np.exp(-(D * D) / (2.0 * width * width))


# ---------------------------------------------------------------------------------------------------- moments
def moments(Z, scores, score_x, wtab=None, exact_N=False):
    """dict N [P,P], v [P], Wsum, r [b,P], t [b], w [n], ok [b] of Z bool [n,P], scores [b,n+1], score_x [b] (fp32)"""
    Z = np.asarray(Z, bool)
    n, P = Z.shape
    s = np.asarray(scores, np.float32)
    sx = np.asarray(score_x, np.float32)
    b = s.shape[0]
    assert s.shape == (b, n + 1) and sx.shape == (b,)
    w = np.ones(n) if wtab is None else np.asarray(wtab, np.float64)[Z.sum(axis=1)]
    y = sx.astype(np.float64)[:, None] - s[:, :n].astype(np.float64)
    N, v, r, t = np.zeros((P, P)), np.zeros(P), np.zeros((b, P)), np.zeros(b)
    Wsum = 0.0
    if exact_N:
        assert wtab is None and n < 2 ** 52
        Zf = Z.astype(np.float64)
        N = Zf.T @ Zf
    with np.errstate(invalid='ignore'):
        for k in range(n):
            z = Z[k]
            if not exact_N:
                N[np.ix_(z, z)] += w[k]
            v[z] += w[k]
            Wsum += w[k]
            wy = w[k] * y[:, k]
            r[:, z] += wy[:, None]
            t += wy
    ok = (np.isfinite(s).all(axis=1) & np.isfinite(sx)).astype(np.int32)
    return dict(N=N, v=v, Wsum=Wsum, r=r, t=t, w=w, ok=ok)


def totals(scores, score_x):
    return np.asarray(score_x, np.float32).astype(np.float64) - np.asarray(scores, np.float32)[:, -1].astype(np.float64)


# ---------------------------------------------------------------------------------------------------- systems
def kshap_system(N, r, total):
    """(A [P-1,P-1], rhs [b,P-1]) in the device's order of operations"""
    l = len(N) - 1
    A = ((N[:l, :l] - N[:l, [l]]) - N[[l], :l]) + N[l, l]
    dn = N[:l, l] - N[l, l]
    with np.errstate(invalid='ignore'):
        rhs = (r[:, :l] - r[:, [l]]) - total[:, None] * dn[None, :]
    return A, rhs


def lime_system(N, v, Wsum, r, t, ridge):
    """(G [P,P], rhs [b,P], mu [P]) in the device's order of operations"""
    mu = v / Wsum
    G = N - Wsum * (mu[:, None] * mu[None, :])
    G[np.diag_indices_from(G)] += ridge
    with np.errstate(invalid='ignore'):
        rhs = r - mu[None, :] * t[:, None]
    return G, rhs, mu


def solve_ref(A, rhs):
    """(phi* [b,m], phi_numpy [b,m], e_ref): numpy's solve, and that plus two steps of iterative refinement with the
    residual in np.longdouble"""
    x0 = np.linalg.solve(A, rhs.T)
    Al, bl = A.astype(np.longdouble), rhs.T.astype(np.longdouble)
    x = x0.copy()
    for _ in range(2):
        res = bl - Al @ x.astype(np.longdouble)
        x = x + np.linalg.solve(A, res.astype(np.float64))
    return x.T, x0.T, float(np.abs(x0 - x).max())


def chol_pivots(A):
    """(singular, ratios): the unblocked right-looking Cholesky's pivots d_j / A_jj up to and including the first one
    that the rule d_j <= 2^-20 A_jj (or not finite) calls singular"""
    a = np.array(A, np.float64)
    d0 = np.diag(a).copy()
    ratios = []
    for j in range(len(a)):
        d = a[j, j]
        with np.errstate(divide='ignore', invalid='ignore'):
            ratios.append(float(d / d0[j]) if d0[j] != 0 else float('-inf'))
        if not (d > PIVOT_TOL * d0[j]) or not np.isfinite(d):
            return True, np.array(ratios)
        col = a[j + 1:, j] / np.sqrt(d)
        a[j + 1:, j] = col
        a[j + 1:, j + 1:] -= np.outer(col, col)
    return False, np.array(ratios)


def gate(phi_star, e_ref):
    """the solve gate, per element"""
    return 2.0 ** -24 * np.abs(phi_star) + 8.0 * e_ref


# ---------------------------------------------------------------------------------------------------- fits
def kshap_fit(Z, scores, score_x, exact_N=True):
    """fp64 KernelSHAP of scores [b,n+1]: dict cells [b,P] (phi*), cells_numpy, e_ref, total [b], ok [b], singular"""
    mo = moments(Z, scores, score_x, None, exact_N)
    total = totals(scores, score_x)
    A, rhs = kshap_system(mo["N"], mo["r"], total)
    sing, _ = chol_pivots(A)
    b, P = mo["r"].shape
    out = dict(mo, total=total, singular=sing, A=A, rhs=rhs, intercept=np.zeros(b))
    good = mo["ok"].astype(bool) & (not sing)
    cells, cells_np = np.full((b, P), np.nan), np.full((b, P), np.nan)
    e_ref = 0.0
    if good.any():
        xs, x0, e_ref = solve_ref(A, rhs[good])
        cells[good] = np.concatenate([xs, (total[good] - xs.sum(axis=1))[:, None]], axis=1)
        cells_np[good] = np.concatenate([x0, (total[good] - x0.sum(axis=1))[:, None]], axis=1)
    out["intercept"][~good] = np.nan
    out.update(cells=cells, cells_numpy=cells_np, e_ref=e_ref, ok=good.astype(np.int32))
    return out


def lime_fit(Z, scores, score_x, wtab, ridge=1.0):
    """fp64 LIME of scores [b,n+1]: dict cells [b,P] (phi*), cells_numpy, e_ref, intercept [b], ok [b], singular"""
    mo = moments(Z, scores, score_x, wtab)
    G, rhs, mu = lime_system(mo["N"], mo["v"], mo["Wsum"], mo["r"], mo["t"], ridge)
    sing, _ = chol_pivots(G)
    b, P = mo["r"].shape
    good = mo["ok"].astype(bool) & (not sing)
    cells, cells_np, icpt = np.full((b, P), np.nan), np.full((b, P), np.nan), np.full(b, np.nan)
    e_ref = 0.0
    if good.any():
        xs, x0, e_ref = solve_ref(G, rhs[good])
        cells[good], cells_np[good] = xs, x0
        icpt[good] = mo["t"][good] / mo["Wsum"] - xs @ mu
    return dict(mo, total=totals(scores, score_x), singular=sing, A=G, rhs=rhs, mu=mu, cells=cells, cells_numpy=cells_np,
                e_ref=e_ref, intercept=icpt, ok=good.astype(np.int32))


def lime_augmented(Z, scores, score_x, wtab, ridge=1.0):
    """the same ridge regression in its textbook form: minimise sum_k w_k (y_k - a - phi . z_k)^2 + ridge |phi|^2 over
    (a, phi) at once, the intercept unpenalised: (cells [b,P], intercept [b])"""
    Z = np.asarray(Z, bool)
    n, P = Z.shape
    w = np.asarray(wtab, np.float64)[Z.sum(axis=1)]
    X = np.concatenate([np.ones((n, 1)), Z.astype(np.float64)], axis=1)
    y = np.asarray(score_x, np.float32).astype(np.float64)[:, None] - np.asarray(scores, np.float32)[:, :n].astype(np.float64)
    R = ridge * np.eye(P + 1)
    R[0, 0] = 0.0
    sol = np.linalg.solve(X.T @ (w[:, None] * X) + R, X.T @ (w[:, None] * y.T))      # [P+1,b]
    return sol[1:].T, sol[0]


def r2_ref(Z, w, scores, score_x, cells32, intercept32, t, Wsum):
    """fit quality [b] from the fp32 outputs widened to fp64, every sum a chain in the device's order; NaN where the
    denominator is 0"""
    Z = np.asarray(Z, bool)
    n, P = Z.shape
    s = np.asarray(scores, np.float32)
    b = s.shape[0]
    y = np.asarray(score_x, np.float32).astype(np.float64)[:, None] - s[:, :n].astype(np.float64)
    phi = np.asarray(cells32, np.float32).astype(np.float64)
    yh = np.asarray(intercept32, np.float32).astype(np.float64)[:, None] * np.ones((1, n))
    for c in range(P):
        yh[:, Z[:, c]] += phi[:, [c]]
    ybar = np.asarray(t, np.float64) / Wsum
    e1, e2 = y - yh, y - ybar[:, None]
    n1, n2 = w[None, :] * (e1 * e1), w[None, :] * (e2 * e2)
    num, den = np.zeros(b), np.zeros(b)
    for k in range(n):
        num += n1[:, k]
        den += n2[:, k]
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den == 0.0, np.nan, 1.0 - num / den)


def additive_scores(Z, weights, orig):
    """scores [1, n+1] of the additive game s(S) = orig - sum_{c in S} w_c on the rows Z and the all-frozen row"""
    w = np.asarray(weights, np.float64)
    Zall = np.concatenate([np.asarray(Z, bool), np.ones((1, len(w)), bool)])
    return (orig - Zall.astype(np.float64) @ w)[None]
