"""CPU: the references of tests/linsur_refs.py for KernelSHAP and LIME (csrc/linsur_ops.hip): the rows
against their cell-by-cell definition, the pairing, the size law, the raw-moment assembly of both systems against their
textbook forms, the recovery of a planted additive game, the pivot rule on the sampled systems, and the argument
refusals of the C entries (error codes, nothing launched, no GPU needed)."""
import numpy as np
import pytest

import linsur_refs as LR
import rise_refs as RR
import shap_refs as SH


def _lib():
    import ivf_lib as L
    return L, L.lib()


# ------------------------------------------------------------------------------------------------ rows
def test_size_table_is_the_cdf_of_the_shapley_kernel():
    for P in (3, 4, 16, 392, 1024):
        t = LR.size_table(P).astype(np.float64)
        assert t.shape == (P - 2,) and bool((np.diff(t) > 0).all()) and 0 < t[0] and t[-1] < 2.0 ** 32
        s = np.arange(1, P)
        q = 1.0 / (s * (P - s))
        cdf = np.cumsum(q) / q.sum()
        assert np.abs(t / 2.0 ** 32 - cdf[:P - 2]).max() < 2.0 ** -31
    assert LR.size_table(2).shape == (0,)
    # a symmetric law: CDF(7) + CDF(8) = 1 at P = 16, within the flooring
    t = LR.size_table(16).astype(np.float64) / 2.0 ** 32
    assert abs(t[6] + t[7] - 1.0) < 1e-9


@pytest.mark.parametrize("paired", [True, False])
def test_rows_are_their_definition_cell_by_cell(paired):
    for P in (2, 3, 8, 33):
        Z, s = LR.kshap_rows(1234, 6, P, paired)
        for k in range(6):
            row, size = LR.kshap_row_brute(1234, k, P, paired)
            assert Z[k].astype(int).tolist() == row and int(s[k]) == size, (P, k)
    # first_k shifts the row index and nothing else (an odd first_k still complements the even row before it)
    Z, s = LR.kshap_rows(7, 8, 36, paired)
    Z3, s3 = LR.kshap_rows(7, 5, 36, paired, first_k=3)
    assert np.array_equal(Z3, Z[3:]) and np.array_equal(s3, s[3:])


@pytest.mark.parametrize("P", [2, 33, 36, 1024])
def test_a_paired_row_is_its_predecessors_complement_and_sizes_are_inside(P):
    n = 64
    Z, s = LR.kshap_rows(1234, n, P, True)
    assert np.array_equal(Z[1::2], ~Z[0::2]) and np.array_equal(s[1::2], P - s[0::2])
    for paired in (True, False):
        Z, s = LR.kshap_rows(1234, n, P, paired)
        assert s.min() >= 1 and s.max() <= P - 1 and np.array_equal(Z.sum(axis=1), s)
    Zp, Zu = LR.kshap_rows(1234, n, P, True)[0], LR.kshap_rows(1234, n, P, False)[0]
    assert np.array_equal(Zu[0::2], Zp[0::2])                                # an even row is hashed as itself either way
    if P > 2:
        assert not np.array_equal(Zu[1::2], Zp[1::2])


def test_sizes_follow_the_shapley_kernel():
    """P = 8, seed 7, 7000 unpaired rows: the sizes 1 .. 7 against q(s) ~ 1 / (s (8 - s)).  Gate: chi-square with 6
    degrees of freedom, its 0.1 % point 22.46 (the family is fixed, so the test is deterministic)."""
    n, P = 7000, 8
    s = LR.kshap_sizes(7, n, P, paired=False)
    sz = np.arange(1, P)
    q = 1.0 / (sz * (P - sz))
    q /= q.sum()
    cnt = np.bincount(s, minlength=P)[1:]
    chi = float(((cnt - n * q) ** 2 / (n * q)).sum())
    assert chi < 22.46, chi


def test_pack_and_lime_rows():
    Z = LR.lime_rows(1234, RR.thresh(0.5), 9, 36)
    assert np.array_equal(Z, RR.bits(1234, 0.5, 9, 36)) and 0 < Z.sum() < Z.size
    assert np.array_equal(LR.lime_rows(1234, RR.thresh(0.5), 4, 36, first_k=5), Z[5:])
    for P in (2, 31, 32, 33, 36, 1024):
        Zk, _ = LR.kshap_rows(5, 6, P)
        b = LR.pack(Zk)
        assert b.dtype == np.uint32 and b.shape == (6, (P + 31) // 32) and np.array_equal(LR.unpack(b, P), Zk)
        if P % 32:
            assert not (b[:, -1] >> np.uint32(P % 32)).any()                # unused high bits
    assert LR.pack(np.array([[1, 0, 1] + [0] * 30 + [1]], bool)).tolist() == [[5, 2]]


def test_lime_weights():
    w = LR.lime_wtab(36)
    assert w.shape == (37,) and w[0] == 1.0 and bool((np.diff(w) < 0).all())
    assert abs(w[36] - np.exp(-1.0 / (2 * 0.0625))) < 1e-18                 # every cell frozen: D = 1
    assert abs(w[27] - np.exp(-0.25 / (2 * 0.0625))) < 1e-15                # a quarter left: D = 1/2


# ------------------------------------------------------------------------------------------------ moments, systems
def _random_case(P, n, b, seed=3, kind="kshap"):
    g = np.random.default_rng(seed)
    Z = LR.kshap_rows(1234, n, P)[0] if kind == "kshap" else LR.lime_rows(1234, RR.thresh(0.5), n, P)
    return Z, g.random((b, n + 1)).astype(np.float32), g.random(b).astype(np.float32)


def test_unweighted_N_from_one_product_is_the_loop():
    Z, s, sx = _random_case(36, 144, 2)
    a, e = LR.moments(Z, s, sx), LR.moments(Z, s, sx, exact_N=True)
    for k in ("N", "v", "r", "t"):
        assert np.array_equal(a[k], e[k]), k
    assert a["Wsum"] == 144.0 and np.array_equal(a["v"], Z.sum(axis=0)) and np.array_equal(np.diag(a["N"]), a["v"])


def test_kshap_raw_moment_assembly_is_the_explicit_form():
    """A = u^T u and rhs = u^T (y - total z_l) with u_k = z_k[:l] - z_kl: the constraint eliminated row by row"""
    P, n, b = 16, 64, 3
    Z, s, sx = _random_case(P, n, b)
    mo = LR.moments(Z, s, sx)
    total = LR.totals(s, sx)
    A, rhs = LR.kshap_system(mo["N"], mo["r"], total)
    u = Z[:, :P - 1].astype(np.float64) - Z[:, [P - 1]].astype(np.float64)
    assert np.array_equal(A, u.T @ u)                                        # integers: exact either way
    y = sx.astype(np.float64)[:, None] - s[:, :n].astype(np.float64)
    want = (y - total[:, None] * Z[:, P - 1].astype(np.float64)[None, :]) @ u
    assert np.abs(rhs - want).max() < 1e-12
    # and the solution is the constrained least-squares minimiser: the full gradient is a multiple of the ones vector
    f = LR.kshap_fit(Z, s, sx)
    assert not f["singular"] and f["ok"].tolist() == [1, 1, 1]
    res = y - f["cells"] @ Z.T.astype(np.float64)
    grad = res @ Z.astype(np.float64)
    assert np.abs(grad - grad.mean(axis=1, keepdims=True)).max() < 1e-10
    assert np.abs(f["cells"].sum(axis=1) - total).max() < 1e-14


def test_lime_is_the_augmented_intercept_ridge():
    P, n, b = 36, 80, 2
    Z, s, sx = _random_case(P, n, b, kind="lime")
    wt = LR.lime_wtab(P)
    f = LR.lime_fit(Z, s, sx, wt, ridge=1.0)
    cells, icpt = LR.lime_augmented(Z, s, sx, wt, ridge=1.0)
    assert not f["singular"]
    assert np.abs(f["cells"] - cells).max() < 1e-12 and np.abs(f["intercept"] - icpt).max() < 1e-12
    # another ridge is another answer
    assert np.abs(LR.lime_fit(Z, s, sx, wt, ridge=0.01)["cells"] - cells).max() > 1e-6


def test_a_nan_score_stays_inside_its_clip():
    Z, s, sx = _random_case(16, 64, 3)
    s2 = s.copy()
    s2[1, 7] = np.nan
    a, e = LR.moments(Z, s, sx), LR.moments(Z, s2, sx)
    assert e["ok"].tolist() == [1, 0, 1] and np.array_equal(a["N"], e["N"])
    assert np.array_equal(a["r"][[0, 2]], e["r"][[0, 2]]) and np.array_equal(a["t"][[0, 2]], e["t"][[0, 2]])
    f = LR.kshap_fit(Z, s2, sx)
    assert f["ok"].tolist() == [1, 0, 1] and np.isnan(f["cells"][1]).all() and np.isfinite(f["cells"][[0, 2]]).all()


@pytest.mark.parametrize("P,n", [(16, 64), (1024, 4096)])
def test_kernelshap_recovers_a_planted_additive_game(P, n):
    """dyadic weights (multiples of 2^-12, exact in fp32): the scores are exact, the model is the game"""
    g = np.random.default_rng(4)
    w = g.integers(-40, 120, P) / 4096.0
    Z, _ = LR.kshap_rows(1234, n, P)
    s = LR.additive_scores(Z, w, 0.75)
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    f = LR.kshap_fit(Z, s.astype(np.float32), np.array([0.75], np.float32))
    assert not f["singular"] and f["total"][0] == w.sum()
    err = float(np.abs(f["cells"][0] - w).max())
    assert err <= 4e-13, err
    r2 = LR.r2_ref(Z, f["w"], s, [0.75], f["cells"].astype(np.float32), [0.0], f["t"], f["Wsum"])
    assert r2[0] > 1.0 - 1e-6


# ------------------------------------------------------------------------------------------------ the pivot rule
REGULAR = [(16, 64), (392, 1568), (1024, 4096)]
SINGULAR = [(8, 16), (1024, 2048)]


def _sampled_system(P, n, seed=1234):
    Z, _ = LR.kshap_rows(seed, n, P, True)
    Zf = Z.astype(np.float64)
    N = Zf.T @ Zf
    A, _ = LR.kshap_system(N, np.zeros((1, P)), np.zeros(1))
    return A


@pytest.mark.parametrize("P,n", REGULAR)
def test_regular_sampled_systems_pass_the_pivot_rule(P, n):
    sing, ratios = LR.chol_pivots(_sampled_system(P, n))
    assert not sing and len(ratios) == P - 1
    assert ratios.min() > 0.05, ratios.min()                                 # decades above 2^-20


@pytest.mark.parametrize("P,n", SINGULAR)
def test_singular_sampled_systems_fail_the_pivot_rule(P, n):
    A = _sampled_system(P, n)
    assert np.linalg.matrix_rank(A) < P - 1
    sing, ratios = LR.chol_pivots(A)
    assert sing and abs(ratios[-1]) < 1e-12                                  # rounding noise, decades below 2^-20
    assert bool((ratios[:-1] > LR.PIVOT_TOL).all())


# ------------------------------------------------------------------------------------------------ the C entries
def test_every_entry_refuses_null_pointers_by_name():
    """-1 and the entry's own name in ivf_last_error(); nothing is launched, no GPU is needed"""
    L, lib = _lib()
    calls = {
        "kshap_rows": lambda: lib.ivf_kshap_rows(1, 1, 0, 4, 2, 2, 2, None, None, None, None),
        "lime_rows": lambda: lib.ivf_lime_rows(1, 1 << 31, 0, 4, 2, 2, 2, None, None),
        "lin_stage": lambda: lib.ivf_lin_stage(None, 1, 3, 4, 8, 8, None, None, 2, 2, 2, 4, None, 0, 1, None, 0, None),
        "lin_moments": lambda: lib.ivf_lin_moments(None, None, None, None, 1, 4, 8, None, None, None, None, None, None, None,
                                                   None),
        "lin_solve": lambda: lib.ivf_lin_solve(0, None, None, None, None, None, None, None, 1, 4, 8, 1.0, None, None, None,
                                               None, None, None),
        "lin_fit": lambda: lib.ivf_lin_fit(None, None, None, None, None, None, None, None, None, 1, 4, 8, None, None),
        "i3d_lin_scores": lambda: lib.ivf_i3d_lin_scores(None, None, 1, None, None, None, 2, 2, 2, 4, None, None, None),
        "clstm_lin_scores": lambda: lib.ivf_clstm_lin_scores(None, None, 1, None, None, None, 2, 2, 2, 4, None, None, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() in lib.ivf_last_error(), (name, lib.ivf_last_error())
    assert lib.ivf_lin_workspace_bytes(1024) == (1024 * 1024 + 2 * 1024 + 1) * 8
    assert lib.ivf_lin_workspace_bytes(0) == 0 and b"lin_workspace_bytes" in lib.ivf_last_error()
    assert lib.ivf_lin_workspace_bytes(1025) == 0
