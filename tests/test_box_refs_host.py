"""CPU: the candidate space of the one-box search (ivf_box_count, ivf_search.box_candidates) and the soundness of
tests/box_refs.py, the references test_gpu_box.py holds the kernels to: the closed-form regulariser against
stmask_refs.reg_terms64 on the explicit S, the drop map against a brute-force loop, the direct staging sums against the
two kernels' own sums and the fp64 reference, and mutants that must land outside the gates."""
import numpy as np
import pytest
import torch

import box_refs as B
import mask_refs
import stmask_refs as SR

GRIDS = [(1, 1), (3, 4), (7, 7)]


def _lib():
    import ivf_lib as L
    return L, L.lib()


# ------------------------------------------------------------------------------------------------ counts and table
@pytest.mark.parametrize("T", [1, 5, 16, 40])
def test_box_count_is_the_product_formula(T):
    L, lib = _lib()
    for gh, gw in GRIDS:
        for ml in range(1, T + 1):
            for mh in range(1, gh + 1):
                for mw in range(1, gw + 1):
                    want = sum(T - l + 1 for l in range(1, ml + 1)) * sum(gh - l + 1 for l in range(1, mh + 1)) \
                        * sum(gw - l + 1 for l in range(1, mw + 1))
                    assert lib.ivf_box_count(T, ml, gh, gw, mh, mw) == want == B.box_count(T, ml, gh, gw, mh, mw)


@pytest.mark.parametrize("T", [1, 5, 16, 40])
def test_table_length_and_order(T):
    """len(box_candidates) == ivf_box_count for every max_*; the table is box_refs' (three nested one-blob tables)"""
    import ivf_search
    L, lib = _lib()
    for grid in GRIDS:
        gh, gw = grid
        for ml in range(1, T + 1):
            for mh in range(1, gh + 1):
                for mw in range(1, gw + 1):
                    tab = ivf_search.box_candidates(T, grid, ml, (mh, mw))
                    assert tab.shape == (lib.ivf_box_count(T, ml, gh, gw, mh, mw), 6)
        ml, mb = min(T, 3), (min(gh, 2), min(gw, 3))
        tab = ivf_search.box_candidates(T, grid, ml, mb).numpy()
        assert np.array_equal(tab, B.box_table(T, grid, ml, mb))
        full = ivf_search.box_candidates(T, grid)
        assert full.shape[0] == lib.ivf_box_count(T, T, gh, gw, gh, gw)
        assert tuple(full[-1].tolist()) == (0, T, 0, gh, 0, gw)


@pytest.mark.parametrize("case", [(1, (1, 1), 1, (1, 1)), (5, (3, 4), 3, (2, 3)), (16, (7, 7), 4, (7, 2)), (40, (3, 4), 2, (3, 4))])
def test_index_round_trip(case):
    T, grid, ml, mb = case
    tab = B.box_table(T, grid, ml, mb)
    assert len({tuple(r) for r in tab.tolist()}) == len(tab)
    for k, c in enumerate(tab):
        a, L_, i0, bh, j0, bw = c
        assert 1 <= L_ <= ml and 0 <= a <= T - L_ and 1 <= bh <= mb[0] and 0 <= i0 <= grid[0] - bh
        assert 1 <= bw <= mb[1] and 0 <= j0 <= grid[1] - bw
        assert B.box_index(c, T, grid, mb) == k


def test_bad_arguments_return_minus_one_with_a_message():
    L, lib = _lib()
    for args in ((0, 1, 3, 4, 1, 1), (65, 1, 3, 4, 1, 1), (16, 0, 3, 4, 1, 1), (16, 17, 3, 4, 1, 1), (16, 4, 0, 4, 1, 1),
                 (16, 4, 33, 4, 1, 1), (16, 4, 3, 33, 1, 1), (16, 4, 3, 4, 0, 1), (16, 4, 3, 4, 4, 1), (16, 4, 3, 4, 1, 5),
                 (16, 4, 3, 4, 1, 0)):
        assert lib.ivf_box_count(*args) == -1 and b"box_count" in lib.ivf_last_error(), args
    assert lib.ivf_box_count(64, 64, 32, 32, 32, 32) == 2080 * 528 * 528
    import ivf_search
    with pytest.raises(L.IvfError):
        ivf_search.box_candidates(16, (3, 4), 4, (4, 1))
    # host-side refusals of the device entries come back as error codes, nothing is launched
    assert lib.ivf_box_stage(None, 1, 3, 5, 12, 20, None, None, 3, 4, 3, 2, 3, 0, 1, None, 0, None) == -1
    assert b"box_stage" in lib.ivf_last_error()
    assert lib.ivf_box_select(None, None, None, 1, 5, 3, 4, 3, 2, 3, 0.0, 0.0, 0.0, 0.9, None, None, None, None, None) == -1
    assert lib.ivf_box_drop(None, None, 1, 5, 3, 4, 3, 2, 3, None, None) == -1


# ------------------------------------------------------------------------------------------------ objective
@pytest.mark.parametrize("case", [(1, (1, 1), 1, (1, 1)), (2, (2, 2), 2, (2, 2)), (3, (1, 3), 3, (1, 3)), (5, (3, 4), 5, (3, 4)),
                                  (6, (2, 1), 4, (2, 1))])
def test_closed_form_regulariser_is_reg_terms64_on_the_explicit_S(case):
    T, grid, ml, mb = case
    tab = B.box_table(T, grid, ml, mb)
    lams = (0.01, 0.02, 0.03)
    S = torch.stack([B.box_S(c, T, grid) for c in tab]).double()
    l1, tvt, tvs = SR.reg_terms64(S, [float(np.float32(v)) for v in lams])
    want = (l1 + tvt + tvs).numpy()
    s = np.linspace(0.1, 0.9, len(tab))[None]
    J, bound = B.objective64(tab, s, T, grid, lams)
    assert np.max(np.abs(J[0] - s[0] - want)) <= 1e-15
    # ... and the integers themselves
    vol, nt, ns = B.box_reg(tab, T, grid)
    cells = grid[0] * grid[1]
    one = SR.reg_terms64(S, (1.0, 1.0, 1.0))
    assert np.array_equal(vol, np.rint(one[0].numpy() * cells)) and np.array_equal(nt, np.rint(one[1].numpy() * cells))
    assert np.array_equal(ns, np.rint(one[2].numpy() * cells))
    # the float32 restatement of the device's expression sits within the derived gate
    J32 = B.objective32(tab, s.astype(np.float32), T, grid, lams).astype(np.float64)
    J64, bound = B.objective64(tab, s.astype(np.float32), T, grid, lams)
    assert bool((np.abs(J32 - J64) <= bound).all())
    assert float(bound.max()) < 1e-6        # a few ulp of J, J < 2
    # every pair once (the mutant of stmask_refs) moves J by far more than the gate wherever an interior pair is cut
    if T >= 4:
        m1 = SR.reg_terms64(S, [float(np.float32(v)) for v in lams], doubled=False)[1].numpy()
        moved = np.abs(m1 - tvt.numpy())
        assert float(moved.max()) > 1e3 * float(bound.max())


def test_select_rule_on_constructed_rows():
    T, grid, ml, mb = 4, (2, 2), 2, (2, 2)
    tab = B.box_table(T, grid, ml, mb)
    n = len(tab)
    s = np.ones((3, n), np.float32)
    ka, kb = B.box_index((1, 1, 0, 1, 1, 1), T, grid, mb), B.box_index((2, 1, 1, 1, 0, 1), T, grid, mb)
    s[0, [ka, kb]] = 0.25
    s[1] = np.nan
    s[2] = 0.5
    s[2, 3] = np.nan
    J = B.objective32(tab, s, T, grid, (0.0, 0.0, 0.0))
    best, minimal = B.select_rule(J, s, np.ones(3), np.zeros(3), tab, 0.7)
    assert best.tolist() == [min(ka, kb), -1, 0] and minimal.tolist() == [min(ka, kb), -1, -1]


# ------------------------------------------------------------------------------------------------ drop map
def test_drop_reference_is_the_brute_force_loop():
    T, grid, ml, mb = 4, (2, 3), 3, (2, 2)
    tab = B.box_table(T, grid, ml, mb)
    g = SR._gen('drophost')
    s = torch.rand(2, len(tab), generator=g).numpy().astype(np.float32)
    s[1, 5] = np.nan
    orig = np.asarray([0.9, 0.8], np.float32)
    ref, bound, cnt = B.drop_ref(s, orig, tab, T, grid)
    sm, c2, sab = B.drop_brute(s, orig, tab, T, grid)
    assert np.array_equal(cnt, c2) and int(cnt.min()) >= 1
    assert np.max(np.abs(ref - sm / c2)) <= 1e-15
    # every cell is covered by its own unit box; the NaN candidate is missing from exactly the cells it covers
    full = B.drop_ref(np.nan_to_num(s, nan=0.5), orig, tab, T, grid)[2]
    a, L_, i0, bh, j0, bw = tab[5]
    lost = full - cnt
    want = np.zeros_like(lost)
    want[1, a:a + L_, i0:i0 + bh, j0:j0 + bw] = 1
    assert np.array_equal(lost, want)


# ------------------------------------------------------------------------------------------------ staging
STAGE = dict(C=2, T=5, H=12, W=20, grid=(3, 4), ml=3, mb=(2, 3))


@pytest.mark.parametrize("sigma", [0.0, 1.5])
def test_direct_sums_equal_the_kernels_sums_and_mutants_do_not(sigma):
    c_ = STAGE
    C, T, H, W, grid = c_['C'], c_['T'], c_['H'], c_['W'], c_['grid']
    gh, gw = grid
    AH, AW = SR.axis_weights(H, gh, sigma), SR.axis_weights(W, gw, sigma)
    assert float(AH.min()) >= 0 and float(AW.min()) >= 0
    x = B.stage_inputs(1, C, T, H, W)[0]
    tab = B.box_table(T, grid, c_['ml'], c_['mb'])
    AHc, AWc = SR.axis_weights_ref(H, gh, sigma, align_corners=True).float(), SR.axis_weights_ref(W, gw, sigma, align_corners=True).float()
    picks = [0, 7, len(tab) // 2, len(tab) - 1] + [B.box_index(c, T, grid, c_['mb']) for c in ((1, 2, 1, 2, 0, 3), (0, 3, 0, 1, 2, 2))]
    for k in picks:
        c = tab[k]
        S = B.box_S(c, T, grid)
        got = B.stage32(x, c, AH, AW)
        via = B.stage32_via_S(x, S, AH, AW)
        assert torch.equal(got, via), f"candidate {tuple(c)}: the zero terms of the expand do not drop out exactly"
        ref = B.stage64(x, S, AH, AW)
        bound = mask_refs.freeze_fwd_bound(x[None].reshape(1, C, T, H * W)).reshape(C, T, H, W) \
            + T * SR.gamma(gh + gw + 2) * 2.0 * float(x.abs().max())
        err = (got.double() - ref).abs()
        assert bool((err <= bound).all())
        gate = float(bound.max())
        a, L_, i0, bh, j0, bw = (int(v) for v in c)
        moved = lambda other: float((other.double() - ref).abs().max())
        if a + L_ <= 1:                      # a blob on frame 0 alone perturbs nothing, whatever its mask
            assert torch.equal(got, x)
            continue
        if (i0, bh) != (j0, bw) and j0 + bw <= gh and i0 + bh <= gw:
            assert moved(B.stage32(x, c, AH, AW, swap=True)) > 1e3 * gate                     # rows <-> columns
        assert moved(B.stage32(x, c, AHc, AWc)) > 1e3 * gate                                   # align_corners=True
        if (a, L_) != (0, T) and (a, L_) != (1, T - 1):
            assert moved(B.stage32(x, c, AH, AW, all_frames=True)) > 1e3 * gate                # recurrence outside the blob
        if bh > 1:
            assert moved(B.stage32_via_S(x, B.box_S(c, T, grid, drop_last_row=True), AH, AW)) > 1e3 * gate
    # frames outside the blob are copies, frame 0 always
    c = tab[B.box_index((2, 2, 0, 2, 1, 2), T, grid, c_['mb'])]
    got = B.stage32(x, c, AH, AW)
    assert torch.equal(got[:, :2], x[:, :2]) and torch.equal(got[:, 4], x[:, 4]) and not torch.equal(got[:, 2], x[:, 2])


def test_1x1_grid_without_blur_is_the_frame_gather():
    """grid 1 x 1, sigma 0: A is all ones, M = 1 on the blob, the freeze returns P[u-1] exactly"""
    C, T, H, W = 2, 6, 5, 7
    AH, AW = SR.axis_weights(H, 1, 0.0), SR.axis_weights(W, 1, 0.0)
    assert torch.equal(AH, torch.ones(H, 1)) and torch.equal(AW, torch.ones(W, 1))
    x = B.stage_inputs(1, C, T, H, W)[0]
    for c in B.box_table(T, (1, 1), T, (1, 1)):
        a, L_ = int(c[0]), int(c[1])
        want = x.clone()
        want[:, a:a + L_] = x[:, max(a - 1, 0)][:, None]
        assert torch.equal(B.stage32(x, c, AH, AW), want)
