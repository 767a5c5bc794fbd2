"""CPU: the host side of the exhaustive one-blob search (maskType 'combi'): candidate count and table, argument
checks of the new entry points, and the selection rule restated in numpy against the reference fixture
(tests/golden/blob.npz, written by make_golden_blob.py from the reference's mask.py and models)."""
import ctypes

import numpy as np
import pytest
import torch

CASES = [("s16", "freeze"), ("s16", "reverse"), ("k32", "freeze"), ("c1", "freeze"), ("c1", "reverse")]


def np_candidates(T, max_len):
    return [(a, L) for L in range(1, max_len + 1) for a in range(T - L + 1)]


def np_tv33(m):
    """mask.calc_tv_norm(m, 3, 3) in the fp32 arithmetic of tv_norm_dev."""
    m = np.asarray(m, dtype=np.float32)
    val = np.float32(0)
    for u in range(1, m.size - 1):
        d0, d1 = np.abs(m[u - 1] - m[u]), np.abs(m[u + 1] - m[u])
        val = np.float32(val + d0 * d0 * d0)
        val = np.float32(val + d1 * d1 * d1)
    y = np.power(val, np.float32(1.0 / 3.0))
    return np.float32(y * y * y)


def np_select(scores, orig, full, T, max_len, lam1, lam2, threshold=0.9):
    """The selection rule of ivf_blob_select: argmin J (canonical order breaks ties, NaN skipped) and the smallest
    sufficient blob (smallest L with r >= threshold, largest r, smallest a)."""
    cands = np_candidates(T, max_len)
    f32 = np.float32
    J = np.empty(len(cands), dtype=np.float32)
    for k, (a, L) in enumerate(cands):
        m = np.zeros(T, dtype=np.float32)
        m[a:a + L] = 1
        J[k] = f32(f32(f32(lam1) * f32(L)) + f32(f32(lam2) * np_tv33(m))) + f32(scores[k])
    ok = ~np.isnan(J)
    best = cands[int(np.flatnonzero(ok)[np.argmin(J[ok])])] if ok.any() else (-1, -1)
    r = (f32(orig) - scores.astype(np.float32)) / (f32(orig) - f32(full))
    minimal = (-1, -1)
    for L in range(1, max_len + 1):
        ks = [k for k, c in enumerate(cands) if c[1] == L and r[k] >= threshold]
        if ks:
            minimal = cands[max(ks, key=lambda k: (r[k], -cands[k][0]))]
            break
    return J, best, minimal


@pytest.mark.parametrize("T", [1, 9, 16, 32, 40])
def test_blob_count_matches_candidate_table(T):
    import ivf_lib as L
    import ivf_search
    lib = L.lib()
    for ml in range(1, T + 1):
        n = lib.ivf_blob_count(T, ml)
        assert n == sum(T - ln + 1 for ln in range(1, ml + 1))
        tab = ivf_search.blob_candidates(T, ml)
        assert tuple(tab.shape) == (n, 2)
        assert tab.tolist() == [list(c) for c in np_candidates(T, ml)]
        # canonical index k(a, L) = sum_{l<L} (T-l+1) + a
        assert ivf_search.blob_index(tab, T).tolist() == list(range(n))
    assert tuple(ivf_search.blob_candidates(T).shape) == (lib.ivf_blob_count(T, T), 2)
    for bad in (0, -1, T + 1):
        assert lib.ivf_blob_count(T, bad) == -1 and b"blob_count" in lib.ivf_last_error()
        with pytest.raises(L.IvfError):
            ivf_search.blob_candidates(T, bad)


def test_blob_masks_and_index():
    import ivf_search
    best = torch.tensor([[0, 1], [3, 4], [15, 1], [-1, -1]])
    m = ivf_search.blob_masks(best, 16)
    want = np.zeros((4, 16), np.float32)
    want[0, 0] = 1
    want[1, 3:7] = 1
    want[2, 15] = 1
    assert np.array_equal(m.numpy(), want)
    assert ivf_search.blob_index(best, 16).tolist() == [0, 16 + 15 + 14 + 3, 15, -1]


def test_null_pointers_return_error_codes():
    import ivf_lib as L
    lib = L.lib()
    assert lib.ivf_blob_stage(None, 1, 3, 16, 10, 16, 0, 0, 1, None, 4, None) == -1
    assert b"blob_stage" in lib.ivf_last_error()
    assert lib.ivf_blob_select(None, None, None, 1, 16, 16, 0.01, 0.02, 0.9, None, None, None, None, None) == -1
    assert b"blob_select" in lib.ivf_last_error()
    assert lib.ivf_i3d_blob_scores(None, None, 1, None, 16, 0, None, None) == -1
    assert b"i3d" in lib.ivf_last_error()
    assert lib.ivf_clstm_blob_scores(None, None, 1, None, 32, 0, None, None) == -1
    assert b"clstm" in lib.ivf_last_error()
    # an unbound plan is refused before any device work
    cfg = L.I3DConfig()
    cfg.B, cfg.C, cfg.T, cfg.H, cfg.W = 2, 3, 16, 224, 224
    cfg.num_classes, cfg.stem_stride_t, cfg.pool4a_stride_t, cfg.pool5a_stride_t = 174, 2, 2, 2
    cfg.head_kt, cfg.head_kh, cfg.head_kw, cfg.softmax = 2, 7, 7, 1
    h = ctypes.c_void_p()
    L.check(lib.ivf_i3d_create(ctypes.byref(cfg), ctypes.byref(h)))
    try:
        assert lib.ivf_i3d_blob_scores(h, None, 1, None, 16, 0, None, None) == -1
        assert b"bind" in lib.ivf_last_error()
    finally:
        lib.ivf_i3d_destroy(h)


@pytest.mark.parametrize("tag,mode", CASES)
def test_numpy_selection_reproduces_fixture(tag, mode, golden):
    g = golden("blob")
    scores = g[f"{tag}_{mode}_scores"]
    T = {"s16": 16, "k32": 32, "c1": 32}[tag]
    ml = int(g[f"{tag}_max_len"])
    lam1, lam2 = (float(v) for v in g[f"{tag}_lam"])
    assert scores.shape == (len(np_candidates(T, ml)),)
    J, best, minimal = np_select(scores, float(g[f"{tag}_orig"]), float(g[f"{tag}_full"]), T, ml, lam1, lam2)
    # the reference's fp32 calc_tv_norm and this restatement agree to rounding
    assert np.max(np.abs(J - g[f"{tag}_{mode}_J"])) < 1e-6
    assert tuple(best) == tuple(g[f"{tag}_{mode}_best"])
    assert tuple(minimal) == tuple(g[f"{tag}_{mode}_minimal"])
