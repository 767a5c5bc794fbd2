"""CPU: the references of tests/scorecam_refs.py for Score-CAM (csrc/scorecam_ops.hip) against a torch
restatement and brute force, the planted-channel ranking through the fp64 reduction, and the argument refusals of the C
entries (error codes, nothing launched, no GPU needed)."""
import ctypes

import numpy as np
import pytest

import scorecam_refs as SC


def _planes(b=2, nc=6, shape=(2, 3, 4), seed=0):
    g = np.random.default_rng(seed)
    A = g.standard_normal((b, nc) + shape).astype(np.float32)
    A[0, 1] = 0.25                        # constant: not valid
    A[0, 2, 0, 1, 1] = np.nan             # NaN: not valid
    A[1, 0, 1, 0, 0] = np.inf             # +Inf: not valid
    A[1, 3, 0, 0, 0] = -np.inf            # -Inf: not valid
    A[1, 4] = np.maximum(A[1, 4], 0)      # a ReLU plane: lo = +0.0
    return A


def test_normalise_against_torch_and_by_hand():
    A = _planes()
    lo, hi, valid, F = SC.normalise(A)
    tlo, thi, tvalid, tF = SC.torch_normalise(A)
    assert np.array_equal(valid, tvalid)
    assert np.array_equal(np.isnan(lo), np.isnan(tlo)) and np.array_equal(lo[~np.isnan(lo)], tlo[~np.isnan(lo)])
    assert np.array_equal(np.isnan(hi), np.isnan(thi)) and np.array_equal(hi[~np.isnan(hi)], thi[~np.isnan(hi)])
    assert np.array_equal(F.view(np.uint32), tF.view(np.uint32))
    want_valid = np.ones((2, 6), bool)
    want_valid[0, 1] = want_valid[0, 2] = want_valid[1, 0] = want_valid[1, 3] = False
    assert np.array_equal(valid, want_valid)
    assert np.isnan(lo[0, 2]) and np.isnan(hi[0, 2]) and lo[0, 2:3].view(np.uint32)[0] == 0x7FC00000
    assert hi[1, 0] == np.inf and lo[1, 3] == -np.inf and lo[0, 1] == hi[0, 1] == np.float32(0.25)
    assert lo[1, 4] == 0 and not np.signbit(lo[1, 4])
    assert np.all(F[~valid] == 1)
    fv = F[valid]
    assert fv.min() == 0 and fv.max() == 1                     # hi maps to 0, lo to 1, exactly
    k = (1, 5)
    a = A[k].astype(np.float64)
    assert np.abs(F[k] - (a.max() - a) / (a.max() - a.min())).max() < 4 * 2.0 ** -24
    assert F[k].reshape(-1)[np.argmax(A[k])] == 0 and F[k].reshape(-1)[np.argmin(A[k])] == 1


def test_frame_planes_follow_the_grid_rule():
    F = np.arange(2 * 3 * 2 * 2, dtype=np.float32).reshape(2, 3, 2, 2)
    P = SC.frame_planes(F, 5)
    assert P.shape == (2, 5, 2, 2) and SC.frame_cell(5, 3).tolist() == [0, 0, 1, 1, 2]
    assert np.array_equal(P[:, 1], F[:, 0]) and np.array_equal(P[:, 3], F[:, 1]) and np.array_equal(P[:, 4], F[:, 2])
    assert np.array_equal(SC.frame_planes(F, 6), np.repeat(F, 2, axis=1))       # T % gt == 0: frame repetition
    import rise_refs as RR
    for T, gt in ((16, 2), (17, 4), (32, 8), (5, 5)):
        assert np.array_equal(SC.frame_cell(T, gt), RR.frame_cell(T, gt))


def test_weights_and_cam_references():
    g = np.random.default_rng(3)
    nc = 7
    s = g.random((2, nc + 1)).astype(np.float32)
    valid = np.ones((2, nc), bool)
    valid[0, 2] = False
    s[1, 4] = np.nan
    w = SC.weights_increase(s, valid)
    assert w.dtype == np.float32 and w[0, 2] == 0 and w[1, 4] == 0
    assert w[0, 0] == np.float32(s[0, 0] - s[0, nc])
    ws, rel = SC.weights_softmax(s, valid)
    assert ws[0, 2] == 0 and ws[1, 4] == 0 and np.allclose(ws.sum(axis=1), 1.0, atol=1e-12)
    import torch
    for r, drop in ((0, 2), (1, 4)):
        keep = [k for k in range(nc) if k != drop]
        d = torch.tensor((s[r, :nc] - s[r, nc]).astype(np.float64))[keep]
        assert np.allclose(ws[r, keep], torch.softmax(d, 0).numpy(), rtol=1e-13)
    assert np.all(rel < 2e-4) and np.all(rel > (nc + 1) * 2.0 ** -24)
    # a baseline row that is NaN leaves nothing counting
    s2 = s.copy()
    s2[0, nc] = np.nan
    assert not SC.weights_increase(s2, valid)[0].any() and not SC.weights_softmax(s2, valid)[0][0].any()
    A = g.standard_normal((2, nc, 2, 3, 3)).astype(np.float32)
    A[0, 2] = np.nan                                           # not valid: weight 0, left out of the map
    cam, bound = SC.cam_ref(w, A)
    assert cam.shape == (2, 2, 3, 3) and np.isfinite(cam).all() and (cam >= 0).all() and (bound > 0).all()
    brute = sum(float(w[1, k]) * A[1, k].astype(np.float64) for k in range(nc))
    assert np.abs(cam[1] - np.maximum(brute, 0)).max() < 1e-15


def test_planted_channel_is_the_argmax_of_the_reference_cam():
    g = np.random.default_rng(8)
    nc, shape = 7, (2, 7, 7)
    A = (0.1 * g.random((1, nc) + shape)).astype(np.float32)
    A[0, 3] = 0
    A[0, 3, 1, 4, 2] = 5.0                                     # a single hot cell
    s = np.full((1, nc + 1), 0.2, np.float32)
    s[0, 3] = 0.9                                              # one d_k large
    for w in (SC.weights_increase(s, np.ones((1, nc), bool)), SC.weights_softmax(s, np.ones((1, nc), bool))[0]):
        cam, _ = SC.cam_ref(w, A)
        assert int(np.argmax(cam.reshape(-1))) == (1 * 7 + 4) * 7 + 2


# ------------------------------------------------------------------------------------------------ C entries
FAKE = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below is refused before anything is launched


def _lib():
    import ivf_lib as L
    return L, L.lib()


def _stage_args(x=FAKE, b=2, C=3, T=5, H=12, W=20, AH=FAKE, AW=FAKE, gt=3, gh=3, gw=4, F=FAKE, nc=5, perturb=0, first=0,
                count=4, p=FAKE, cpad=0):
    return (x, b, C, T, H, W, AH, AW, gt, gh, gw, F, nc, perturb, first, count, p, cpad, None)


def test_scorecam_stage_refusals():
    L, lib = _lib()
    for kw in (dict(x=None), dict(AH=None), dict(AW=None), dict(F=None), dict(p=None)):
        assert lib.ivf_scorecam_stage(*_stage_args(**kw)) == -1, kw
        assert b"scorecam_stage: null pointer" in lib.ivf_last_error()
    bad = (dict(b=0), dict(C=0), dict(H=0), dict(W=0), dict(T=0), dict(T=65, gt=8), dict(gt=0), dict(gt=6), dict(gh=0),
           dict(gh=33), dict(gw=33), dict(T=16, gt=9, gh=32, gw=32),         # 9216 cells
           dict(T=64, gt=64, gh=32, gw=5),                                    # 10240 cells
           dict(nc=0), dict(perturb=2), dict(perturb=-1),
           dict(first=-1), dict(count=0), dict(first=9, count=4),             # a window past b (nc + 1) = 12
           dict(first=12, count=1), dict(b=20000, nc=5, count=65536),
           dict(cpad=3), dict(cpad=4, C=5), dict(cpad=4, p=ctypes.c_void_p((1 << 20) + 4)))
    for kw in bad:
        assert lib.ivf_scorecam_stage(*_stage_args(**kw)) == -1, kw
        assert b"scorecam_stage" in lib.ivf_last_error(), kw
    # 8193 cells cannot be factored within the sides; the closest products on either side of the limit
    assert lib.ivf_scorecam_stage(*_stage_args(T=8, gt=8, gh=32, gw=32, first=11, count=2)) == -1     # 8192 cells: the window
    assert b"rows [11, 13)" in lib.ivf_last_error()
    assert lib.ivf_scorecam_stage(*_stage_args(T=33, gt=33, gh=32, gw=8)) == -1                       # 8448 cells
    assert b"8192" in lib.ivf_last_error()
    assert lib.ivf_scorecam_stage(*_stage_args(perturb=2)) == -1 and b"perturb" in lib.ivf_last_error()


def test_scorecam_normalise_and_reduce_refusals():
    L, lib = _lib()
    nrm = lib.ivf_scorecam_normalise
    for i in (0, 4, 5, 6, 7):
        a = [FAKE, 2, 5, 98, FAKE, FAKE, FAKE, FAKE, None]
        a[i] = None
        assert nrm(*a) == -1 and b"scorecam_normalise: null pointer" in lib.ivf_last_error(), i
    for b, nc, cells in ((0, 5, 98), (2, 0, 98), (2, 5, 0), (2, 5, 8193), (1 << 20, 1 << 20, 4)):
        assert nrm(FAKE, b, nc, cells, FAKE, FAKE, FAKE, FAKE, None) == -1, (b, nc, cells)
        assert b"scorecam_normalise" in lib.ivf_last_error()
    red = lib.ivf_scorecam_reduce
    for i in (0, 1, 2, 7, 8):
        a = [FAKE, FAKE, FAKE, 2, 5, 98, 0, FAKE, FAKE, None]
        a[i] = None
        assert red(*a) == -1 and b"scorecam_reduce: null pointer" in lib.ivf_last_error(), i
    for b, nc, cells, kind in ((0, 5, 98, 0), (2, 0, 98, 0), (2, 5, 0, 0), (2, 5, 8193, 1), (2, 5, 98, 2), (2, 5, 98, -1)):
        assert red(FAKE, FAKE, FAKE, b, nc, cells, kind, FAKE, FAKE, None) == -1, (b, nc, cells, kind)
        assert b"scorecam_reduce" in lib.ivf_last_error()


def test_plan_entries_refuse_a_null_plan():
    L, lib = _lib()
    for fn in (lib.ivf_i3d_scorecam_scores, lib.ivf_clstm_scorecam_scores):
        assert fn(None, FAKE, 1, FAKE, FAKE, FAKE, 2, 3, 4, FAKE, 5, 0, FAKE, None) == -1


def test_scorecam_is_still_not_a_cam_kind():
    import ivf_lib as L
    with pytest.raises(L.IvfError, match="gradcam, gradcam\\+\\+, xgradcam, hirescam, layercam"):
        L.cam_kind_ids(["scorecam"])
    assert "scorecam" not in L.CAM_KINDS
