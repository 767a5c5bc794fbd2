"""CPU: the references of tests/rise_refs.py for RISE random-mask saliency (csrc/rise_ops.hip) against the
known answers of the mask hash, the refused edges of p, the frame-to-cell map, a planted-cell ranking through the fp64
reduction, and the argument refusals of the C entries (error codes, nothing launched, no GPU needed)."""
import ctypes

import numpy as np
import pytest

import rise_refs as RR


def _lib():
    import ivf_lib as L
    return L, L.lib()


KNOWN = {(0, 0): 0x4e9c01b3, (0, 1): 0x175ea60e, (0, 2): 0xf33c5152, (1, 0): 0xd8c0aef4, (1, 35): 0x8c750ce7,
         (63, 35): 0x97baaa4d}


def test_hash_known_answers():
    for (k, c), want in KNOWN.items():
        assert int(RR.hash_u(1234, k, c)) == want, (k, c)
    # broadcast form == scalar form
    k = np.array([0, 1, 63])[:, None]
    c = np.array([0, 1, 2, 35])[None]
    u = RR.hash_u(1234, k, c)
    assert int(u[0, 2]) == KNOWN[(0, 2)] and int(u[1, 3]) == KNOWN[(1, 35)] and int(u[2, 3]) == KNOWN[(63, 35)]
    row = RR.bits(1234, 0.5, 1, 12)[0]
    assert "".join("1" if v else "0" for v in row) == "110111001010"
    # first_k shifts the mask index and nothing else
    assert np.array_equal(RR.bits(1234, 0.5, 5, 12, first_k=3), RR.bits(1234, 0.5, 8, 12)[3:])
    # the seed matters, and wraps as uint32 arithmetic does
    assert not np.array_equal(RR.bits(1235, 0.5, 4, 12), RR.bits(1234, 0.5, 4, 12))
    assert int(RR.hash_u(0xFFFFFFFF, 0, 0)) == int(RR.fmix32(RR.fmix32((0xFFFFFFFF + 0x9E3779B9) & 0xFFFFFFFF) ^ np.uint64(0x85EBCA77)))


def test_thresh_and_its_refused_edges():
    assert RR.thresh(0.5) == 1 << 31 and RR.thresh(0.25) == 1 << 30
    assert RR.thresh(1.0 - 2.0 ** -32) == (1 << 32) - 1
    assert RR.thresh(2.0 ** -32) == 1
    for p in (0.0, 1.0, -0.1, 1.5, float('nan'), 2.0 ** -33):
        with pytest.raises(ValueError):
            RR.thresh(p)
    # the product's own computation of thresh agrees and refuses the same edges with IvfError
    import ivf_engine
    import ivf_lib as L
    for p in (0.5, 0.25, 0.1, 1.0 - 2.0 ** -32, 2.0 ** -32, 1e-3):
        assert ivf_engine.rise_thresh(p) == RR.thresh(p)
    for p in (0.0, 1.0, -0.1, 1.5, float('nan'), 2.0 ** -33, "half"):
        with pytest.raises(L.IvfError):
            ivf_engine.rise_thresh(p)


def test_frame_to_cell_map():
    assert RR.frame_cell(5, 3).tolist() == [0, 0, 1, 1, 2]
    assert RR.frame_cell(16, 8).tolist() == [u // 2 for u in range(16)]
    assert RR.frame_cell(17, 4).tolist() == [(u * 4) // 17 for u in range(17)]
    for T in (1, 5, 16, 17, 40, 64):
        for gt in {1, min(2, T), T // 2 or 1, T}:
            kt = RR.frame_cell(T, gt)
            assert kt[0] == 0 and kt[-1] == gt - 1 and np.all(np.diff(kt) >= 0) and np.all(np.diff(kt) <= 1)
            assert sorted(set(kt.tolist())) == list(range(gt))           # every temporal cell owns a frame
        assert RR.frame_cell(T, T).tolist() == list(range(T))
    S = RR.masks(1234, 0.5, 2, (3, 3, 4))
    F = RR.frame_masks(S, 5)
    assert F.shape == (2, 5, 3, 4) and np.array_equal(F[:, 1], S[:, 0]) and np.array_equal(F[:, 4], S[:, 2])


@pytest.mark.parametrize("n,grid,want_counts,want_min", [(16, (1, 3, 4), [9, 9, 11, 7, 8, 6, 6, 6, 8, 5, 10, 11], 5),
                                                         (64, (4, 3, 3), None, 22)])
def test_planted_cell_is_ranked_first(n, grid, want_counts, want_min):
    seed, p = 1234, 0.5
    cells = grid[0] * grid[1] * grid[2]
    planted = 7 % cells
    w = np.full(cells, 0.01)
    w[planted] = 0.5
    s = RR.planted_scores(seed, p, n, grid, w)
    got, cnt, mean_drop, bound = RR.reduce_ref(s, [0.9], seed, p, grid)
    assert int(cnt.min()) >= 1 and int(cnt.min()) == want_min           # every cell counted: the ranking is meaningful
    if want_counts is not None:
        assert cnt.reshape(-1).tolist() == want_counts
    assert int(np.argmax(got.reshape(-1))) == planted
    # cells is a conditional mean: the planted cell's own weight is in every term of its sum -- it holds the whole
    # weight, plus at most what the other cells can add (d_k is formed in fp32: 1e-6 of slack)
    assert 0.5 - 1e-6 <= got.reshape(-1)[planted] <= 0.5 + 0.01 * (cells - 1) + 1e-6
    d = 0.9 - s[0]
    assert abs(mean_drop[0] - d.mean()) < 1e-6


def test_reduce_reference_nan_rules_and_brute_force():
    seed, p, grid, n = 7, 0.25, (2, 2, 3), 12
    g = np.random.default_rng(5)
    s = g.random((2, n)).astype(np.float32)
    s[0, 3] = np.nan
    s[1, :] = np.nan                                                   # a clip with nothing left
    orig = np.array([0.8, 0.6], np.float32)
    got, cnt, mean_drop, bound = RR.reduce_ref(s, orig, seed, p, grid)
    Sb = RR.bits(seed, p, n, 12)
    for c in range(12):
        ks = [k for k in range(n) if Sb[k, c] and k != 3]
        assert cnt.reshape(2, -1)[0, c] == len(ks)
        if ks:
            want = np.mean([float(orig[0]) - float(s[0, k]) for k in ks])
            assert abs(got.reshape(2, -1)[0, c] - want) < 1e-12
        else:
            assert np.isnan(got.reshape(2, -1)[0, c])
    assert np.isnan(got[1]).all() and not cnt[1].any() and np.isnan(mean_drop[1])
    assert abs(mean_drop[0] - np.mean([float(orig[0]) - float(s[0, k]) for k in range(n) if k != 3])) < 1e-12
    # n = 2 with a small p leaves cells uncounted: NaN there
    got2, cnt2, _, _ = RR.reduce_ref(g.random((1, 2)), [0.5], 1234, 0.1, (2, 3, 3))
    assert (cnt2 == 0).any() and np.array_equal(np.isnan(got2), cnt2 == 0)


# ------------------------------------------------------------------------------------------------ C entries
FAKE = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below is refused before anything is launched
HALF = 1 << 31


def test_rise_masks_refusals():
    L, lib = _lib()
    assert lib.ivf_rise_masks(1, HALF, 0, 4, 2, 3, 3, None, None) == -1 and b"rise_masks" in lib.ivf_last_error()
    assert lib.ivf_rise_masks(1, 0, 0, 4, 2, 3, 3, FAKE, None) == -1 and b"thresh" in lib.ivf_last_error()
    for gt, gh, gw in ((0, 3, 3), (65, 3, 3), (2, 0, 3), (2, 33, 3), (2, 3, 0), (2, 3, 33)):
        assert lib.ivf_rise_masks(1, HALF, 0, 4, gt, gh, gw, FAKE, None) == -1, (gt, gh, gw)
    assert lib.ivf_rise_masks(1, HALF, -1, 4, 2, 3, 3, FAKE, None) == -1
    assert lib.ivf_rise_masks(1, HALF, 0, 0, 2, 3, 3, FAKE, None) == -1


def _stage_args(x=FAKE, b=2, C=3, T=5, H=12, W=20, AH=FAKE, AW=FAKE, gt=3, gh=3, gw=4, n=16, seed=1, thresh=HALF, first=0,
                count=4, p=FAKE, cpad=0):
    return (x, b, C, T, H, W, AH, AW, gt, gh, gw, n, seed, thresh, first, count, p, cpad, None)


def test_rise_stage_refusals():
    L, lib = _lib()
    for kw in (dict(x=None), dict(AH=None), dict(AW=None), dict(p=None)):
        assert lib.ivf_rise_stage(*_stage_args(**kw)) == -1, kw
        assert b"rise_stage" in lib.ivf_last_error()
    bad = (dict(b=0), dict(C=0), dict(H=0), dict(W=0), dict(T=0), dict(T=65, gt=8), dict(gt=0), dict(gt=6), dict(gh=0),
           dict(gh=33), dict(gw=0), dict(gw=33), dict(thresh=0), dict(n=0), dict(first=-1), dict(count=0),
           dict(first=30, count=3),                    # rows outside b * n = 32
           dict(n=70000, count=65536),                 # more than 65535 rows a call
           dict(cpad=8), dict(cpad=4, C=5),
           dict(cpad=4, p=ctypes.c_void_p((1 << 20) + 4)))      # channels-last buffer not 16-byte aligned
    for kw in bad:
        assert lib.ivf_rise_stage(*_stage_args(**kw)) == -1, kw
        assert lib.ivf_last_error()
    assert lib.ivf_rise_stage(*_stage_args(thresh=0)) == -1 and b"thresh" in lib.ivf_last_error()
    assert lib.ivf_rise_stage(*_stage_args(cpad=4, p=ctypes.c_void_p((1 << 20) + 4))) == -1 and b"aligned" in lib.ivf_last_error()


def test_rise_reduce_refusals():
    L, lib = _lib()
    ok = dict(scores=FAKE, orig=FAKE, b=2, n=16, seed=1, thresh=HALF, gt=2, gh=3, gw=3, cells=FAKE, count=FAKE, mean=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ivf_rise_reduce(a["scores"], a["orig"], a["b"], a["n"], a["seed"], a["thresh"], a["gt"], a["gh"], a["gw"],
                                   a["cells"], a["count"], a["mean"], None)
    for kw in (dict(scores=None), dict(orig=None), dict(cells=None), dict(count=None), dict(mean=None), dict(b=0), dict(n=0),
               dict(thresh=0), dict(gt=0), dict(gt=65), dict(gh=33), dict(gw=0)):
        assert call(**kw) == -1, kw
        assert b"rise_reduce" in lib.ivf_last_error()


def test_plan_entries_are_exported_and_the_tf_plan_has_none():
    L, lib = _lib()
    assert hasattr(lib, "ivf_i3d_rise_scores") and hasattr(lib, "ivf_clstm_rise_scores")
    assert not hasattr(lib, "ivf_tfclstm_rise_scores")
    # an unbound plan is refused before anything else is looked at
    cfg = L.CLSTMConfig()
    cfg.B, cfg.C, cfg.T, cfg.H, cfg.W = 2, 2, 6, 24, 32
    cfg.hidden, cfg.layers, cfg.kernel, cfg.stride, cfg.num_classes = 4, 2, 5, 2, 5
    cfg.softmax, cfg.batch_norm, cfg.out_step = 0, 1, 5
    h = ctypes.c_void_p()
    L.check(lib.ivf_clstm_create(ctypes.byref(cfg), ctypes.byref(h)))
    assert lib.ivf_clstm_rise_scores(h, FAKE, 2, FAKE, FAKE, FAKE, 2, 2, 2, 8, 1, HALF, FAKE, None) != 0
    lib.ivf_clstm_destroy(h)
