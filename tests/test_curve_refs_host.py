"""CPU: the references of tests/curve_refs.py for the deletion / insertion curves (csrc/curve_ops.hip): the
rank known answers (ties, NaN, +-0, both orders), the deletion / insertion complement identity, J and the short last
interval, the fp64 AUC on planted curves, the NaN rules, the pooling on a constant map, and the argument refusals of the
C entries (error codes, nothing launched, no GPU needed)."""
import ctypes

import numpy as np
import pytest

import curve_refs as CR
import shap_refs as SH

FAKE = ctypes.c_void_p(1 << 20)
NAN = float('nan')


def _lib():
    import ivf_lib as L
    return L, L.lib()


# ------------------------------------------------------------------------------------------------ ranks
def test_rank_known_answers():
    a = [0.5, 2.0, -1.0, 2.0, 0.5]
    assert CR.ranks(np.array(a), 0).tolist() == [2, 0, 4, 1, 3]          # ties fall to the lower index
    assert CR.ranks(np.array(a), 1).tolist() == [1, 3, 0, 4, 2]          # ... in either order
    # NaN after every number, -inf included, in both orders; NaN cells among themselves by index
    a = [NAN, 1.0, -np.inf, NAN, np.inf]
    assert CR.ranks(np.array(a), 0).tolist() == [3, 1, 2, 4, 0]
    assert CR.ranks(np.array(a), 1).tolist() == [3, 1, 0, 4, 2]
    # -0.0 == +0.0: a tie, by index
    a = [0.0, -0.0, 1.0, -0.0, -1.0]
    assert CR.ranks(np.array(a), 0).tolist() == [1, 2, 0, 3, 4]
    assert CR.ranks(np.array(a), 1).tolist() == [1, 2, 4, 3, 0]
    assert CR.ranks(np.full(4, NAN), 0).tolist() == [0, 1, 2, 3] == CR.ranks(np.full(4, NAN), 1).tolist()
    assert CR.ranks(np.array([3.0]), 0).tolist() == [0]


def test_vectorised_ranks_are_the_definition():
    g = np.random.default_rng(3)
    for P in (1, 2, 9, 37):
        a = g.integers(-3, 4, (6, P)).astype(np.float32) / 2          # many ties
        a[g.random((6, P)) < 0.15] = np.nan
        a[g.random((6, P)) < 0.1] = -0.0
        a[0, 0] = np.inf
        a[1, -1] = -np.inf
        for order in (0, 1):
            r = CR.ranks(a, order)
            assert np.array_equal(np.sort(r, axis=1), np.broadcast_to(np.arange(P), (6, P)))
            for i in range(6):
                assert r[i].tolist() == CR.ranks_brute(a[i], order), (P, order, i)


def test_without_ties_lerf_is_morf_reversed():
    a = np.random.default_rng(1).permutation(20).astype(np.float32)[None]
    assert np.array_equal(CR.ranks(a, 1), 19 - CR.ranks(a, 0))


def test_grid_cells_mean_over_uneven_temporal_cells():
    """T = 9, gt = 4: frames per cell 3, 2, 2, 2"""
    kt = (np.arange(9) * 4) // 9
    assert np.bincount(kt).tolist() == [3, 2, 2, 2]
    a = np.arange(9, dtype=np.float32).reshape(1, 9, 1, 1) * 0.25
    assert CR.grid_cells(a, 9, 4).reshape(-1).tolist() == [0.25, 0.875, 1.375, 1.875]
    b = a.copy()
    b[0, 4] = np.nan
    assert np.isnan(CR.grid_cells(b, 9, 4).reshape(-1)).tolist() == [False, True, False, False]
    # gt == T: the cells themselves
    assert np.array_equal(CR.grid_cells(a, 9, 9), a)


# ------------------------------------------------------------------------------------------------ rows
def test_row_count_and_the_short_last_interval():
    assert CR.thresholds(8, 3).tolist() == [0, 3, 6, 8]                 # J = 3, the last interval 2 cells
    assert CR.thresholds(8, 1).tolist() == list(range(9))
    assert CR.thresholds(8, 8).tolist() == [0, 8] == CR.thresholds(8, 8).tolist()
    assert CR.thresholds(7, 7).tolist() == [0, 7]
    rows = CR.row_list(2, 8, 3, 3)
    assert len(rows) == 2 * 2 * 4
    assert rows[:8] == [(0, 0, 0), (0, 0, 3), (0, 0, 6), (0, 0, 8), (0, 1, 0), (0, 1, 3), (0, 1, 6), (0, 1, 8)]
    assert rows[8] == (1, 0, 0)
    assert [r[1] for r in CR.row_list(1, 8, 3, 2)] == [1] * 4 and [r[1] for r in CR.row_list(1, 8, 3, 1)] == [0] * 4


def test_row_ends_and_the_complement_identity():
    g = np.random.default_rng(5)
    grid, P = (2, 2, 3), 12
    rk = np.stack([g.permutation(P), g.permutation(P)])
    for step in (1, 5):
        rows = CR.row_list(2, P, step, 3)
        S = CR.row_masks(rk, grid, rows)
        J = len(CR.thresholds(P, step)) - 1
        S = S.reshape(2, 2, J + 1, P)
        assert not S[:, 0, 0].any() and S[:, 0, J].all()                # deletion: the clip .. fully frozen
        assert S[:, 1, 0].all() and not S[:, 1, J].any()                # insertion: fully frozen .. the clip
        assert np.array_equal(S[:, 0] + S[:, 1], np.ones_like(S[:, 0]))  # the two rows of a threshold are complements
        assert S[:, 0].sum(axis=-1).tolist() == [CR.thresholds(P, step).tolist()] * 2
    # insertion at k under rank == deletion at P - k under P - 1 - rank
    for k in range(P + 1):
        ins = CR.row_masks(rk, grid, [(0, 1, k), (1, 1, k)])
        dele = CR.row_masks(P - 1 - rk, grid, [(0, 0, P - k), (1, 0, P - k)])
        assert np.array_equal(ins, dele), k
    # a deletion curve at step 1 is a Shapley permutation with that table
    assert np.array_equal(CR.row_masks(rk[:1], grid, CR.row_list(1, P, 1, 1)), SH.row_masks(rk[:1], grid, np.arange(P + 1)))


# ------------------------------------------------------------------------------------------------ reduction
def test_auc_of_a_linear_curve_is_one_half():
    for P, step in ((8, 1), (8, 3), (16, 5), (4096, 1), (7, 7)):
        k = CR.thresholds(P, step).astype(np.float64)
        s = np.stack([1 - k / P, k / P])[None]                          # deletion falls, insertion rises, linearly in k
        r = CR.auc_ref(s, P, step, 3)
        assert np.allclose(r["auc"], 0.5, rtol=0, atol=1e-15), (P, step)
        assert np.allclose(r["auc_norm"], 0.5, rtol=0, atol=1e-15)
    # exact where the scores are multiples of 2^-8 and P a power of two
    s = (np.array([[8, 7, 6, 5, 4, 3, 2, 1, 0]]) / 8.0)[None]
    r = CR.auc_ref(s, 8, 1, 1)
    assert r["auc"][0, 0] == 0.5 and r["auc_norm"][0, 0] == 0.5
    # a step curve: everything lost with the first cell
    s = np.array([[[1.0] + [0.25] * 8]])
    r = CR.auc_ref(s, 8, 1, 1)
    assert r["auc"][0, 0] == (1.25 + 7 * 0.5) / 16 and r["auc_norm"][0, 0] == (r["auc"][0, 0] - 0.25) / 0.75


def test_step_three_rows_are_a_subset_and_weigh_the_short_interval():
    s1 = np.random.default_rng(0).random((1, 1, 9))
    s3 = s1[:, :, [0, 3, 6, 8]]
    r = CR.auc_ref(s3, 8, 3, 1)
    want = (3 * (s3[0, 0, 0] + s3[0, 0, 1]) + 3 * (s3[0, 0, 1] + s3[0, 0, 2]) + 2 * (s3[0, 0, 2] + s3[0, 0, 3])) / 16
    assert abs(r["auc"][0, 0] - want) < 1e-15


def test_nan_rules_and_the_normalisation_ends():
    s = np.random.default_rng(2).random((2, 2, 5))
    s[1, 0, 2] = np.nan
    r = CR.auc_ref(s, 4, 1, 3)
    assert np.isnan(r["auc"]).tolist() == [[False, False], [True, False]]
    assert np.isnan(r["auc_norm"]).tolist() == [[False, False], [True, False]]
    # s_hi == s_lo: auc is a number, auc_norm is NaN
    s = np.array([[[0.5, 0.7, 0.5]]])
    r = CR.auc_ref(s, 2, 1, 1)
    assert r["auc"][0, 0] == 0.6 and np.isnan(r["auc_norm"][0, 0])
    # deletion: hi = row 0; insertion: hi = row J
    s = np.array([[[1.0, 0.5, 0.0], [0.0, 0.5, 1.0]]])
    r = CR.auc_ref(s, 2, 1, 3)
    assert r["auc_norm"].tolist() == [[0.5, 0.5]]
    assert CR.auc_ref(s[:, :1], 2, 1, 1)["auc_norm"].tolist() == [[0.5]]
    assert CR.auc_ref(s[:, 1:], 2, 1, 2)["auc_norm"].tolist() == [[0.5]]


def test_morf_lerf_sandwich_on_an_additive_game():
    """s(S) = orig - sum_{c in S} w_c: freezing the largest weights first lowers every prefix score the most, so the
    deletion AUC under 'morf' is the least and under 'lerf' the greatest over all orders -- by construction."""
    g = np.random.default_rng(8)
    P = 16
    w = g.integers(0, 200, P) / 4096.0
    aucs = {}
    for name, rk in (("morf", CR.ranks(w, 0)[None]), ("lerf", CR.ranks(w, 1)[None]), ("hash", SH.ranks(1234, 8, P))):
        s = SH.additive_scores(rk, w, 0.75)                              # [1, n, P+1]
        aucs[name] = CR.auc_ref(s[0][:, None, :], P, 1, 1)["auc"][:, 0]
    assert bool((aucs["morf"][0] <= aucs["hash"]).all()) and bool((aucs["hash"] <= aucs["lerf"][0]).all())
    assert aucs["morf"][0] < aucs["lerf"][0]


def test_random_baseline_is_the_mean_and_its_mirror():
    s = np.random.default_rng(4).random((2, 5, 9))
    r = CR.random_baseline(s)
    assert r.shape == (2, 2, 9)
    assert np.array_equal(r[:, 0], s.mean(axis=1)) and np.array_equal(r[:, 1], s.mean(axis=1)[:, ::-1])


def test_pooling_a_constant_map_gives_the_constant():
    import stmask_refs as SR
    AH, AW = SR.axis_weights(12, 3, 1.5).numpy(), SR.axis_weights(20, 4, 1.5).numpy()
    cells, mag, den = CR.pool_ref(np.full((1, 2, 12, 20), 0.375), AH, AW)
    assert np.allclose(cells, 0.375, rtol=1e-14, atol=0) and np.allclose(mag, 0.375, rtol=1e-14, atol=0)
    assert den.shape == (3, 4) and abs(den.sum() - 12 * 20) < 1e-3      # the rows of A sum to 1


# ------------------------------------------------------------------------------------------------ C-level refusals
def test_curve_ranks_refusals():
    L, lib = _lib()
    assert lib.ivf_curve_ranks(None, 2, 4, 9, 4, 2, 2, 0, FAKE, None) == -1 and b"curve_ranks" in lib.ivf_last_error()
    assert lib.ivf_curve_ranks(FAKE, 2, 4, 9, 4, 2, 2, 0, None, None) == -1
    assert lib.ivf_curve_ranks(FAKE, 0, 4, 9, 4, 2, 2, 0, FAKE, None) == -1
    for gt, gh, gw in ((0, 3, 3), (10, 3, 3), (2, 0, 3), (2, 33, 3), (2, 3, 0), (2, 3, 33), (5, 32, 32)):
        assert lib.ivf_curve_ranks(FAKE, 2, gt, 9, gt, gh, gw, 0, FAKE, None) == -1, (gt, gh, gw)
        assert b"curve_ranks" in lib.ivf_last_error()
    assert lib.ivf_curve_ranks(FAKE, 2, 4, 65, 4, 2, 2, 0, FAKE, None) == -1
    assert lib.ivf_curve_ranks(FAKE, 2, 5, 9, 4, 2, 2, 0, FAKE, None) == -1 and b"t_in" in lib.ivf_last_error()
    assert lib.ivf_curve_ranks(FAKE, 2, 4, 9, 4, 2, 2, 2, FAKE, None) == -1 and b"order" in lib.ivf_last_error()
    assert lib.ivf_curve_ranks(FAKE, 2, 4, 9, 4, 2, 2, -1, FAKE, None) == -1


def _stage_args(x=FAKE, b=2, C=3, T=5, H=12, W=20, AH=FAKE, AW=FAKE, gt=3, gh=3, gw=4, ranks=FAKE, curves=3, step=1, first=0,
                count=4, p=FAKE, cpad=0):
    return (x, b, C, T, H, W, AH, AW, gt, gh, gw, ranks, curves, step, first, count, p, cpad, None)


def test_curve_stage_refusals():
    L, lib = _lib()
    for kw in (dict(x=None), dict(AH=None), dict(AW=None), dict(ranks=None), dict(p=None)):
        assert lib.ivf_curve_stage(*_stage_args(**kw)) == -1, kw
        assert b"curve_stage" in lib.ivf_last_error()
    bad = (dict(b=0), dict(C=0), dict(H=0), dict(W=0), dict(T=0), dict(T=65, gt=8), dict(gt=0), dict(gt=6), dict(gh=0),
           dict(gh=33), dict(gw=0), dict(gw=33), dict(first=-1), dict(count=0),
           dict(T=64, gt=5, gh=32, gw=32),             # 5120 players
           dict(step=0), dict(step=37), dict(curves=0), dict(curves=4), dict(curves=-1),
           dict(first=146, count=3),                   # rows outside b * 2 * (P + 1) = 148
           dict(first=148, count=1),
           dict(curves=1, first=74, count=1),          # one curve: 74 rows
           dict(step=3, first=50, count=3),            # J = 12: 2 * 2 * 13 = 52 rows
           dict(b=2000, count=65536),                  # more than 65535 rows a call
           dict(cpad=8), dict(cpad=4, C=5),
           dict(cpad=4, p=ctypes.c_void_p((1 << 20) + 4)))      # channels-last buffer not 16-byte aligned
    for kw in bad:
        assert lib.ivf_curve_stage(*_stage_args(**kw)) == -1, kw
        assert b"curve_stage" in lib.ivf_last_error(), kw
    assert lib.ivf_curve_stage(*_stage_args(first=146, count=3)) == -1 and b"148" in lib.ivf_last_error()
    assert lib.ivf_curve_stage(*_stage_args(step=3, first=50, count=3)) == -1 and b"52" in lib.ivf_last_error()
    assert lib.ivf_curve_stage(*_stage_args(T=64, gt=5, gh=32, gw=32)) == -1 and b"4096" in lib.ivf_last_error()
    assert lib.ivf_curve_stage(*_stage_args(step=37)) == -1 and b"step" in lib.ivf_last_error()
    assert lib.ivf_curve_stage(*_stage_args(curves=4)) == -1 and b"curves" in lib.ivf_last_error()
    assert lib.ivf_curve_stage(*_stage_args(cpad=4, p=ctypes.c_void_p((1 << 20) + 4))) == -1 and b"aligned" in lib.ivf_last_error()


def test_curve_reduce_refusals():
    L, lib = _lib()
    ok = dict(scores=FAKE, b=2, nc=2, curves=3, P=8, step=3, auc=FAKE, norm=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ivf_curve_reduce(a["scores"], a["b"], a["nc"], a["curves"], a["P"], a["step"], a["auc"], a["norm"], None)
    for kw in (dict(scores=None), dict(auc=None), dict(norm=None), dict(b=0), dict(nc=1), dict(nc=3), dict(curves=0),
               dict(curves=4), dict(curves=1), dict(P=0), dict(P=4097), dict(step=0), dict(step=9)):
        assert call(**kw) == -1, kw
        assert b"curve_reduce" in lib.ivf_last_error()


def test_plan_entries_are_exported_and_the_tf_plan_has_none():
    L, lib = _lib()
    assert hasattr(lib, "ivf_i3d_curve_scores") and hasattr(lib, "ivf_clstm_curve_scores")
    assert not hasattr(lib, "ivf_tfclstm_curve_scores")
    # an unbound plan is refused before anything else is looked at
    cfg = L.CLSTMConfig()
    cfg.B, cfg.C, cfg.T, cfg.H, cfg.W = 2, 2, 6, 24, 32
    cfg.hidden, cfg.layers, cfg.kernel, cfg.stride, cfg.num_classes = 4, 2, 5, 2, 5
    cfg.softmax, cfg.batch_norm, cfg.out_step = 0, 1, 5
    h = ctypes.c_void_p()
    L.check(lib.ivf_clstm_create(ctypes.byref(cfg), ctypes.byref(h)))
    assert lib.ivf_clstm_curve_scores(h, FAKE, 2, FAKE, FAKE, FAKE, 2, 2, 2, FAKE, 3, 1, FAKE, None) != 0
    lib.ivf_clstm_destroy(h)


def test_public_modules_import_without_a_gpu():
    import inspect

    import faithfulness_videos
    import ivf_engine
    ps = inspect.signature(faithfulness_videos.FaithfulnessVideo.__init__).parameters
    assert ps["step"].default == 1 and ps["grid"].default is None and ps["sigma"].default is None
    for name in ("curve_cells", "curve_ranks", "curve_scores", "curve_reduce", "curve_random_baseline", "faithfulness"):
        assert callable(getattr(ivf_engine._Engine, name))
    ps = inspect.signature(ivf_engine._Engine.faithfulness).parameters
    assert ps["step"].default == 1 and ps["order"].default == "morf"
    import ivf_find_masks
    import ivf_search
    assert inspect.signature(ivf_search.MaskSearch.__init__).parameters["do_curves"].default is False
    assert inspect.signature(ivf_find_masks.find_masks_impl).parameters["do_curves"].default is False
    import FindMasksComparison_I3D_KTH as kth
    import FindMasksComparison_I3D_smth as smth
    for drv in (kth, smth):
        ps = inspect.signature(drv.find_masks).parameters
        assert ps["doCurves"].default is False and ps["curveStep"].default == 1
        assert ps["curveGrid"].default is None and ps["curveSigma"].default is None
