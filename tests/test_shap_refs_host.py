"""CPU: the references of tests/shap_refs.py for Shapley value sampling (csrc/shapley_ops.hip): the rank
known answers, that every row is a permutation, the antithetic reverses, a chi-square gate on the rank of a fixed cell,
the fp64 estimator on synthetic games (additive game, efficiency, dummy player, NaN rules), the derived fp32 bounds, and
the argument refusals of the C entries (error codes, nothing launched, no GPU needed)."""
import ctypes

import numpy as np
import pytest

import rise_refs as RR
import shap_refs as SH


def _lib():
    import ivf_lib as L
    return L, L.lib()


# ------------------------------------------------------------------------------------------------ ranks
def test_rank_known_answers():
    assert SH.ranks(1234, 2, 8).tolist() == [[1, 0, 7, 2, 4, 3, 6, 5], [6, 7, 0, 5, 3, 4, 1, 2]]
    # antithetic off: permutation 1 is hashed as itself
    assert SH.ranks(1234, 2, 8, antithetic=False)[1].tolist() == [7, 3, 0, 6, 4, 5, 1, 2]
    assert SH.ranks(1234, 1, 16)[0].tolist() == [4, 2, 15, 5, 8, 7, 14, 11, 1, 9, 3, 13, 10, 6, 12, 0]
    # the vectorised table is the definition, cell by cell
    for anti in (True, False):
        for k in range(5):
            assert SH.ranks(1234, 1, 8, anti, first_k=k)[0].tolist() == SH.ranks_brute(1234, k, 8, anti), (anti, k)
    # first_k shifts the permutation index and nothing else (an odd first_k still reverses the even one before it)
    assert np.array_equal(SH.ranks(7, 5, 36, first_k=3), SH.ranks(7, 8, 36)[3:])
    assert not np.array_equal(SH.ranks(8, 4, 36), SH.ranks(7, 4, 36))


@pytest.mark.parametrize("P", [1, 8, 36, 4096])
def test_every_row_is_a_permutation_and_odd_rows_are_reverses(P):
    n = 6
    for anti in (True, False):
        r = SH.ranks(99, n, P, anti)
        assert r.shape == (n, P) and r.min() == 0 and r.max() == P - 1
        assert np.array_equal(np.sort(r, axis=1), np.broadcast_to(np.arange(P), (n, P)))
    r, plain = SH.ranks(99, n, P, True), SH.ranks(99, n, P, False)
    assert np.array_equal(r[0::2], plain[0::2])
    assert np.array_equal(r[1::2], P - 1 - r[0::2])
    if P > 2:
        assert not np.array_equal(plain[1::2], r[1::2])


def test_a_hash_tie_falls_to_the_lower_index(monkeypatch):
    """with every hash equal the order is the index order: still a permutation"""
    monkeypatch.setattr(RR, "hash_u", lambda seed, k, c: np.zeros(np.broadcast(k, c).shape, np.uint64))
    assert SH.ranks(1, 2, 5).tolist() == [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]]
    assert SH.ranks_brute(1, 0, 5) == [0, 1, 2, 3, 4]


def test_rank_of_a_fixed_cell_is_uniform():
    """P = 8, seed 7, 4000 independent permutations (antithetic off): the rank of each cell against the uniform law.
    Gate: chi-square with 7 degrees of freedom, its 0.1 % point 24.32 (a uniform family fails one time in a thousand;
    the family is fixed, so the test is deterministic)."""
    n, P = 4000, 8
    r = SH.ranks(7, n, P, antithetic=False)
    for c in range(P):
        counts = np.bincount(r[:, c], minlength=P)
        chi2 = float(((counts - n / P) ** 2 / (n / P)).sum())
        print(f"[shap ranks] cell {c}: counts {counts.min()}..{counts.max()}, chi2 {chi2:.2f}")
        assert chi2 < 24.32, (c, counts.tolist())


# ------------------------------------------------------------------------------------------------ estimator
W8 = np.array([3, -1, 0, 8, 2, 0, -4, 5]) / 1024.0              # multiples of 2^-10: every sum below is exact


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64])
@pytest.mark.parametrize("anti", [True, False])
def test_additive_game_is_recovered_for_every_n(n, anti):
    rk = SH.ranks(1234, n, 8, anti)
    s = SH.additive_scores(rk, W8, 0.75)
    assert np.all(s[0, :, 0] == 0.75) and np.all(s[0, :, 8] == 0.75 - W8.sum())
    r = SH.reduce_ref(s, rk)
    assert np.array_equal(r["cells"][0], W8)                      # phi = w exactly, whatever n
    assert r["count"].tolist() == [[n] * 8]
    assert r["total"][0] == W8.sum()
    if n >= 2:
        assert np.array_equal(r["stderr"][0], np.zeros(8))
    else:
        assert np.isnan(r["stderr"]).all()
    # fp32 copies of the same (exactly representable) scores: nothing changes
    assert np.array_equal(SH.reduce_ref(s.astype(np.float32), rk)["cells"], r["cells"])


def test_efficiency_and_dummy_player():
    g = np.random.default_rng(3)
    n, P = 6, 12
    rk = SH.ranks(5, n, P)
    s = g.random((2, n, P + 1)).astype(np.float32)
    r = SH.reduce_ref(s, rk)
    assert np.allclose(r["cells"].sum(axis=1), r["total"], rtol=0, atol=1e-13)          # the telescoping sum
    assert np.allclose(r["total"], (s[:, :, 0].astype(np.float64) - s[:, :, P]).mean(axis=1), rtol=0, atol=1e-15)
    # dummy player: cell 4 never changes the score -- the row after its entry repeats the row before
    s2 = s.copy()
    for k in range(n):
        j = rk[k, 4]
        s2[:, k, j + 1:] = s2[:, k, j:P].copy()                  # shift: s[j+1] = s[j], later rows follow
    r2 = SH.reduce_ref(s2, rk)
    assert np.all(r2["cells"][:, 4] == 0.0) and np.all(r2["stderr"][:, 4] == 0.0)
    assert np.all(np.abs(r2["cells"][:, :4]).sum(axis=1) > 0)
    assert np.allclose(r2["cells"].sum(axis=1), r2["total"], rtol=0, atol=1e-13)


def test_nan_rules():
    n, P = 5, 6
    rk = SH.ranks(11, n, P)
    g = np.random.default_rng(8)
    s = g.random((1, n, P + 1)).astype(np.float32)
    base = SH.reduce_ref(s, rk)
    s1 = s.copy()
    s1[0, 2, 3] = np.nan                                         # prefix 3 of permutation 2
    r = SH.reduce_ref(s1, rk)
    hit = (rk[2] == 2) | (rk[2] == 3)                            # the cells entering at prefix 3 and leaving it
    assert hit.sum() == 2
    assert np.array_equal(base["count"][0] - r["count"][0], hit.astype(np.int64))
    assert np.array_equal(r["cells"][0][~hit], base["cells"][0][~hit])
    for c in np.nonzero(hit)[0]:
        d = [float(s[0, k, rk[k, c]]) - float(s[0, k, rk[k, c] + 1]) for k in range(n) if k != 2]
        assert abs(r["cells"][0, c] - np.mean(d)) < 1e-15
        assert abs(r["stderr"][0, c] - np.std(d, ddof=1) / np.sqrt(len(d))) < 1e-15
    assert r["total"][0] == base["total"][0] and r["nall"][0] == n       # the ends are untouched
    # a NaN end score drops the permutation from total (and its first or last marginal from one cell)
    s2 = s.copy()
    s2[0, 1, 0] = np.nan
    r2 = SH.reduce_ref(s2, rk)
    assert r2["nall"][0] == n - 1
    assert abs(r2["total"][0] - np.mean([float(s[0, k, 0]) - float(s[0, k, P]) for k in range(n) if k != 1])) < 1e-15
    assert (base["count"][0] - r2["count"][0]).tolist() == (rk[1] == 0).astype(int).tolist()
    # an infinite end score forms marginals (it is not NaN) but is not in total
    s3 = s.copy()
    s3[0, 1, P] = np.inf
    r3 = SH.reduce_ref(s3, rk)
    assert r3["nall"][0] == n - 1 and r3["count"].min() == n
    # cnt = 1: a value, no stderr; cnt = 0: NaN cells
    one = SH.reduce_ref(s[:, :1], rk[:1])
    assert np.isnan(one["stderr"]).all() and np.isnan(one["bound_stderr"]).all() and not np.isnan(one["cells"]).any()
    s4 = np.full((1, 2, P + 1), np.nan, np.float32)
    none = SH.reduce_ref(s4, rk[:2])
    assert np.isnan(none["cells"]).all() and np.isnan(none["stderr"]).all() and not none["count"].any()
    assert np.isnan(none["total"]).all()


def _fp32_device_order(s, rk):
    """the device's arithmetic restated in numpy float32, same order (k ascending, two passes)"""
    s = np.asarray(s, np.float32)
    b, n, P1 = s.shape
    P = P1 - 1
    cells, se = np.empty((b, P), np.float32), np.empty((b, P), np.float32)
    for bi in range(b):
        for c in range(P):
            d = [np.float32(s[bi, k, rk[k, c]] - s[bi, k, rk[k, c] + 1]) for k in range(n)]
            d = [v for v in d if not np.isnan(v)]
            sm = np.float32(0)
            for v in d:
                sm = np.float32(sm + v)
            cnt = len(d)
            mean = np.float32(sm / np.float32(cnt)) if cnt else np.float32(np.nan)
            ss = np.float32(0)
            for v in d:
                e = np.float32(v - mean)
                ss = np.float32(ss + np.float32(e * e))
            cells[bi, c] = mean
            se[bi, c] = np.sqrt(np.float32(np.float32(ss / np.float32(cnt - 1)) / np.float32(cnt))) if cnt >= 2 else np.nan
    return cells, se


def test_derived_fp32_bounds_hold_for_an_fp32_restatement():
    """the bounds of the module docstring against the same arithmetic in numpy float32: random scores, a game with
    equal marginals (fp64 stderr 0, fp32 not necessarily) and scores with a large common offset"""
    g = np.random.default_rng(17)
    n, P = 33, 10
    rk = SH.ranks(21, n, P)
    tenth = SH.additive_scores(rk, np.full(P, 0.1), 3.3).astype(np.float32)      # 0.1 is no fp32 number: d_k vary by rounding
    for what, s in (("random", g.random((2, n, P + 1)).astype(np.float32)),
                    ("equal marginals", tenth),
                    ("offset", (1000.0 + 1e-3 * g.random((1, n, P + 1))).astype(np.float32))):
        r = SH.reduce_ref(s, rk)
        cells, se = _fp32_device_order(s, rk)
        ec, es = np.abs(cells - r["cells"]), np.abs(se - r["stderr"])
        print(f"[shap bounds] {what}: cells err/bound {float((ec / r['bound_cells']).max()):.3f}, "
              f"stderr err/bound {float((es / r['bound_stderr']).max()):.3f}")
        assert bool((ec <= r["bound_cells"]).all()) and bool((es <= r["bound_stderr"]).all()), what
        # the bounds are rounding-sized: far below the values they guard wherever those are not themselves rounding
        assert float(r["bound_cells"].max()) <= (n + 2) * SH.U * float(np.abs(s).max()) * 2
    assert bool((r["bound_stderr"] > 0).all())


# ------------------------------------------------------------------------------------------------ C entries
FAKE = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below is refused before anything is launched


def test_shap_ranks_refusals():
    L, lib = _lib()
    assert lib.ivf_shap_ranks(1, 1, 0, 4, 2, 3, 3, None, None) == -1 and b"shap_ranks" in lib.ivf_last_error()
    for gt, gh, gw in ((0, 3, 3), (65, 3, 3), (2, 0, 3), (2, 33, 3), (2, 3, 0), (2, 3, 33), (5, 32, 32), (64, 32, 32)):
        assert lib.ivf_shap_ranks(1, 1, 0, 4, gt, gh, gw, FAKE, None) == -1, (gt, gh, gw)
        assert b"shap_ranks" in lib.ivf_last_error()
    assert lib.ivf_shap_ranks(1, 2, 0, 4, 2, 3, 3, FAKE, None) == -1 and b"antithetic" in lib.ivf_last_error()
    assert lib.ivf_shap_ranks(1, 1, -1, 4, 2, 3, 3, FAKE, None) == -1
    assert lib.ivf_shap_ranks(1, 1, 0, 0, 2, 3, 3, FAKE, None) == -1
    assert lib.ivf_shap_ranks(1, 1, 0x7fffffff, 1, 2, 3, 3, FAKE, None) == -1


def _stage_args(x=FAKE, b=2, C=3, T=5, H=12, W=20, AH=FAKE, AW=FAKE, gt=3, gh=3, gw=4, n=2, ranks=FAKE, first=0, count=4,
                p=FAKE, cpad=0):
    return (x, b, C, T, H, W, AH, AW, gt, gh, gw, n, ranks, first, count, p, cpad, None)


def test_shap_stage_refusals():
    L, lib = _lib()
    for kw in (dict(x=None), dict(AH=None), dict(AW=None), dict(ranks=None), dict(p=None)):
        assert lib.ivf_shap_stage(*_stage_args(**kw)) == -1, kw
        assert b"shap_stage" in lib.ivf_last_error()
    bad = (dict(b=0), dict(C=0), dict(H=0), dict(W=0), dict(T=0), dict(T=65, gt=8), dict(gt=0), dict(gt=6), dict(gh=0),
           dict(gh=33), dict(gw=0), dict(gw=33), dict(n=0), dict(first=-1), dict(count=0),
           dict(T=64, gt=5, gh=32, gw=32),             # 5120 players
           dict(first=146, count=3),                   # rows outside b * n * (P + 1) = 148
           dict(first=148, count=1),
           dict(n=2000, count=65536),                  # more than 65535 rows a call
           dict(cpad=8), dict(cpad=4, C=5),
           dict(cpad=4, p=ctypes.c_void_p((1 << 20) + 4)))      # channels-last buffer not 16-byte aligned
    for kw in bad:
        assert lib.ivf_shap_stage(*_stage_args(**kw)) == -1, kw
        assert b"shap_stage" in lib.ivf_last_error(), kw
    assert lib.ivf_shap_stage(*_stage_args(first=146, count=3)) == -1 and b"148" in lib.ivf_last_error()
    assert lib.ivf_shap_stage(*_stage_args(T=64, gt=5, gh=32, gw=32)) == -1 and b"4096" in lib.ivf_last_error()
    assert lib.ivf_shap_stage(*_stage_args(cpad=4, p=ctypes.c_void_p((1 << 20) + 4))) == -1 and b"aligned" in lib.ivf_last_error()


def test_shap_reduce_refusals():
    L, lib = _lib()
    ok = dict(scores=FAKE, ranks=FAKE, b=2, n=4, gt=2, gh=3, gw=3, cells=FAKE, se=FAKE, count=FAKE, total=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ivf_shap_reduce(a["scores"], a["ranks"], a["b"], a["n"], a["gt"], a["gh"], a["gw"], a["cells"], a["se"],
                                   a["count"], a["total"], None)
    for kw in (dict(scores=None), dict(ranks=None), dict(cells=None), dict(se=None), dict(count=None), dict(total=None),
               dict(b=0), dict(n=0), dict(gt=0), dict(gt=65), dict(gh=33), dict(gw=0), dict(gt=5, gh=32, gw=32)):
        assert call(**kw) == -1, kw
        assert b"shap_reduce" in lib.ivf_last_error()


def test_plan_entries_are_exported_and_the_tf_plan_has_none():
    L, lib = _lib()
    assert hasattr(lib, "ivf_i3d_shap_scores") and hasattr(lib, "ivf_clstm_shap_scores")
    assert not hasattr(lib, "ivf_tfclstm_shap_scores")
    # an unbound plan is refused before anything else is looked at
    cfg = L.CLSTMConfig()
    cfg.B, cfg.C, cfg.T, cfg.H, cfg.W = 2, 2, 6, 24, 32
    cfg.hidden, cfg.layers, cfg.kernel, cfg.stride, cfg.num_classes = 4, 2, 5, 2, 5
    cfg.softmax, cfg.batch_norm, cfg.out_step = 0, 1, 5
    h = ctypes.c_void_p()
    L.check(lib.ivf_clstm_create(ctypes.byref(cfg), ctypes.byref(h)))
    assert lib.ivf_clstm_shap_scores(h, FAKE, 2, FAKE, FAKE, FAKE, 2, 2, 2, 8, FAKE, FAKE, None) != 0
    lib.ivf_clstm_destroy(h)


def test_public_modules_import_without_a_gpu():
    import ivf_find_masks
    import ivf_search
    import shapley_videos
    import inspect
    assert "do_shapley" in inspect.signature(ivf_search.MaskSearch.__init__).parameters
    assert "do_shapley" in inspect.signature(ivf_find_masks.find_masks_impl).parameters
    assert inspect.signature(shapley_videos.ShapleyVideo.__init__).parameters["n_perms"].default == 64
    import FindMasksComparison_I3D_KTH as kth
    import FindMasksComparison_I3D_smth as smth
    for drv in (kth, smth):
        ps = inspect.signature(drv.find_masks).parameters
        assert ps["doShapley"].default is False and ps["shapPerms"].default == 64
        assert all(k in ps for k in ("shapGrid", "shapSigma", "shapSeed"))
