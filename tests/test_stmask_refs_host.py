"""CPU test of tests/stmask_refs.py and of the host side of csrc/stmask_ops.hip: the axis-weight matrices of the
library against torch, the fp64 references against torch autograd, what wrong kernels would do to the gates, and the
argument checks of the new entries -- on the very inputs test_gpu_stmask.py later runs the kernels on.
"""
import ctypes

import numpy as np
import pytest
import torch

import mask_refs
import stmask_refs as R
from conftest import note

F32 = np.float32


# ---------------------------------------------------------------------------------------------------- (a) axis weights
@pytest.mark.parametrize("case", R.AXIS_CASES, ids=[f"{o}from{i}s{s}" for o, i, s in R.AXIS_CASES])
def test_axis_weights_match_torch(case):
    """ivf_stmask_axis_weights against F.interpolate(bilinear, align_corners=False) followed by a replicate-padded
    Gaussian conv1d, in fp64: every entry within 2 fp32 ulp, entries >= 0, row sums within gamma(n_in) of 1"""
    n_out, n_in, sigma = case
    A = R.lib_axis_weights(n_out, n_in, sigma)
    ref = R.axis_weights_ref(n_out, n_in, sigma)
    assert A.shape == ref.shape and not bool(torch.isnan(A).any())
    err = (A.double() - ref).abs()
    worst = float((err / R.ulp32(ref)).max())
    assert bool((err <= 2 * R.ulp32(ref)).all()), f"{case}: {worst:.2f} ulp"
    assert bool((A >= 0).all())
    # n_in roundings of the entries themselves (each at most U relative, entries sum to 1)
    assert bool(((A.double().sum(dim=1) - 1).abs() <= R.gamma(n_in)).all())
    note(f"stmask axis weights {case}: worst {worst:.3f} fp32 ulp from torch fp64")


def test_axis_weights_identity_is_exact():
    for n in (1, 4, 32):
        assert torch.equal(R.lib_axis_weights(n, n, 0.0), torch.eye(n))


# ---------------------------------------------------------------------------------------------------- (b) adjointness
@pytest.mark.parametrize("name", list(R.EXPAND_CASES))
def test_expand_adjoint(name):
    """<A_H S A_W^T, D> == <S, A_H^T D A_W> in fp64 to 1e-12 relative"""
    c = R.expand_case(name)
    lhs = float((R.expand64(c['S'], c['AH'], c['AW']) * c['dM'].double()).sum())
    rhs = float((c['S'].double() * c['dS']).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    B, T, gh, gw, H, W, sigma = R.EXPAND_CASES[name]
    if (gh, gw, sigma) == (H, W, 0.0):
        assert torch.equal(c['M'].float(), c['S'])              # the identity case is one


# ---------------------------------------------------------------------------------------------------- (c) the chain
@pytest.mark.parametrize("shape", [(2, 3, 5, 3, 4, 9, 11, 1.0), (1, 1, 4, 1, 1, 5, 6, 0.0), (2, 2, 1, 2, 2, 6, 4, 2.0)])
def test_chain_gradient_equals_autograd(shape):
    """hand-written fp64 gradient of sigmoid -> expand -> per-pixel scan -> linear functional == torch fp64 autograd"""
    B, C, T, gh, gw, H, W, sigma = shape
    g = R._gen('chain', shape)
    Rw = (torch.rand(B, T, gh, gw, generator=g) * 6 - 3).float()
    x = torch.rand(B, C, T, H * W, generator=g) * 255
    up = torch.rand(B, C, T, H * W, generator=g) - 0.3
    AH, AW = R.axis_weights(H, gh, sigma), R.axis_weights(W, gw, sigma)
    hand, auto = R.chain_grad64(Rw, AH, AW, x, up), R.chain_autograd64(Rw, AH, AW, x, up)
    assert float((hand - auto).abs().max()) <= 1e-10 * float(auto.abs().max())
    if T > 1:
        assert float(auto[:, 0].abs().max()) == 0.0             # M[:, 0] never enters the recurrence


# ---------------------------------------------------------------------------------------------------- (d) reduction
@pytest.mark.parametrize("name", list(R.STFREEZE_CASES))
def test_scan_reference_reduces_to_the_temporal_one(name):
    """at a spatially constant M the per-pixel references equal mask_refs' exactly, and the dM gate summed over the
    pixels stays within the temporal gate's construction (same pieces, C + 2 for C HW terms)"""
    c = R.stfreeze_case(name)
    B, C, T, HW = R.STFREEZE_CASES[name]
    rows = c['rows']
    M = rows.view(B, T, 1).expand(B, T, HW).contiguous()
    assert torch.equal(R.stfreeze_fwd64(c['x'], M), mask_refs.freeze_fwd_ref(c['x'], rows))
    assert torch.equal(R.stfreeze_scan64(c['g'], M), mask_refs.freeze_scan64(c['g'], rows))
    ref = mask_refs.freeze_bwd_ref(c['x'], c['g'], rows)
    mine = R.stfreeze_bwd_ref(c['x'], c['g'], M)
    assert float((mine['dM'].sum(dim=2) - ref['formula']).abs().max()) <= 1e-12 * float(ref['sabs'].max() + 1)
    assert bool((mine['dM'][:, 0] == 0).all()) and bool((mine['b_dM'][:, 0] == 0).all())


# ---------------------------------------------------------------------------------------------------- fp32 restatements
def _expand32(S, AH, AW):
    """the kernel's sums in numpy float32, unfused: tmp over j ascending, then M over i ascending"""
    S, AH, AW = S.numpy().astype(F32), AH.numpy().astype(F32), AW.numpy().astype(F32)
    gh, gw = S.shape[-2:]
    tmp = np.zeros(S.shape[:-1] + (AW.shape[0],), F32)
    for j in range(gw):
        tmp = tmp + (S[..., :, j:j + 1] * AW[None, :, j]).astype(F32)
    out = np.zeros(S.shape[:-2] + (AH.shape[0], AW.shape[0]), F32)
    for i in range(gh):
        out = out + (AH[:, i:i + 1] * tmp[..., i:i + 1, :]).astype(F32)
    return torch.from_numpy(out)


def _expand_bwd32(dM, AH, AW):
    """y ascending into tmp, then x ascending (one of the orders the any-order bound covers)"""
    dM, AH, AW = dM.numpy().astype(F32), AH.numpy().astype(F32), AW.numpy().astype(F32)
    H, gh = AH.shape
    W, gw = AW.shape
    tmp = np.zeros(dM.shape[:-2] + (gh, W), F32)
    for y in range(H):
        tmp = tmp + (AH[y][:, None] * dM[..., y:y + 1, :]).astype(F32)
    out = np.zeros(dM.shape[:-2] + (gh, gw), F32)
    for x in range(W):
        out = out + (tmp[..., :, x:x + 1] * AW[x][None, :]).astype(F32)
    return torch.from_numpy(out)


@pytest.mark.parametrize("name", list(R.EXPAND_CASES))
def test_expand_fp32_restatement_is_inside_and_mutants_are_outside(name):
    B, T, gh, gw, H, W, sigma = R.EXPAND_CASES[name]
    c = R.expand_case(name)
    err = (_expand32(c['S'], c['AH'], c['AW']).double() - c['M']).abs()
    assert bool((err <= c['bM']).all())
    errb = (_expand_bwd32(c['dM'], c['AH'], c['AW']).double() - c['dS']).abs()
    assert bool((errb <= c['bdS']).all())
    note(f"stmask expand {name}: fp32 restatement worst err/gate fwd {float((err / c['bM']).max()):.3f} "
         f"bwd {float((errb / c['bdS']).max()):.4f}")
    # (e) mutants of the matrices, wherever the path is exercised
    muts = []
    if (H, W) != (gh, gw) and min(gh, gw) > 1:
        muts.append(('align_corners=True', dict(align_corners=True)))
    if sigma > 0 and min(gh, gw) > 1:
        muts.append(('zero-padded blur', dict(pad='constant')))
    for what, kw in muts:
        AHm, AWm = R.axis_weights_ref(H, gh, sigma, **kw), R.axis_weights_ref(W, gw, sigma, **kw)
        Mm = AHm @ c['S'].double() @ AWm.t()
        dSm = AHm.t() @ c['dM'].double() @ AWm
        f = float(((Mm - c['M']).abs() / c['bM']).max())
        fb = float(((dSm - c['dS']).abs() / c['bdS']).max())
        assert f > 1 and fb > 1, f"{name} {what}: {f:.2f} / {fb:.2f} times the gate"
        note(f"stmask expand {name} mutant {what}: {f:.3g} x the forward gate, {fb:.3g} x the backward gate")


@pytest.mark.parametrize("name", list(R.STFREEZE_CASES))
def test_stfreeze_fp32_restatement_is_inside_and_a_dropped_channel_is_outside(name):
    B, C, T, HW = R.STFREEZE_CASES[name]
    c = R.stfreeze_case(name)
    x, g, M = (c[k].numpy().astype(F32) for k in ('x', 'g', 'M'))
    P = np.empty_like(x)
    P[:, :, 0] = x[:, :, 0]
    for u in range(1, T):
        mu = M[:, u][:, None]
        P[:, :, u] = ((F32(1) - mu) * x[:, :, u]).astype(F32) + (mu * P[:, :, u - 1]).astype(F32)
    assert bool(((torch.from_numpy(P).double() - c['P']).abs() <= c['bP']).all())
    G = np.empty_like(g)
    G[:, :, T - 1] = g[:, :, T - 1]
    for u in range(T - 2, -1, -1):
        G[:, :, u] = g[:, :, u] + (M[:, u + 1][:, None] * G[:, :, u + 1]).astype(F32)
    dM = np.zeros((B, T, HW), F32)
    for ch in range(C):
        dM[:, 1:] = dM[:, 1:] + ((P[:, ch, :-1] - x[:, ch, 1:]).astype(F32) * G[:, ch, 1:]).astype(F32)
    err = (torch.from_numpy(dM).double() - c['dM']).abs()
    assert bool((err <= c['b_dM']).all()) and bool((dM[:, 0] == 0).all())
    if T > 1:
        mut = R.stfreeze_bwd_ref(c['x'], c['g'], c['M'], drop_channel=C - 1)['dM']
        nz = c['b_dM'] > 0
        f = float(((mut - c['dM']).abs()[nz] / c['b_dM'][nz]).max())
        assert f > 1
        note(f"stmask stfreeze {name}: dM restatement worst err/gate {float((err[nz] / c['b_dM'][nz]).max()):.3f}; "
             f"a dropped channel {f:.3g} x the gate")


@pytest.mark.parametrize("name", list(R.REG_CASES))
def test_reg_reference(name):
    """the gathered fp32 gradient formula of the kernel, restated in float32 torch, is inside the gates; the mutant
    without the doubled interior pairs is outside wherever interior pairs exist (T >= 4)"""
    B, T, gh, gw = R.REG_CASES[name]
    c = R.reg_case(name)
    s = torch.sigmoid(c['raw'])                                     # float32
    assert bool(((s.double() - c['sig']).abs() <= c['b_sig']).all())
    S = s.clone().requires_grad_()
    l1, tvt, tvs = R.reg_terms64(S, R.REG_LAMS)                       # the same graph in float32
    (l1.sum() + tvt.sum() + tvs.sum()).backward()
    got = torch.stack([l1, tvt, tvs], dim=1).detach().double()
    assert bool(((got - c['terms']).abs() <= c['b_terms']).all())
    assert bool(((S.grad.double() - c['dreg']).abs() <= c['b_dreg']).all())
    assert bool(torch.isfinite(c['dreg']).all())
    if T >= 4:
        mut = R.reg_ref(c['raw'], doubled=False)
        moving = c['terms'][:, 1] > 0                                    # a temporally constant clip has no TVt at all
        assert bool(moving.any()) and bool(((mut['terms'][:, 1] - c['terms'][:, 1]).abs() > c['b_terms'][:, 1])[moving].all())
        assert float(((mut['dreg'] - c['dreg']).abs() / c['b_dreg']).max()) > 1


def test_reg_reduces_to_the_temporal_loss_on_a_1x1_grid():
    """at a 1x1 grid J_reg is lam1 sum S + lam2 val, the temporal loop's regulariser ((val^(1/3))^3 == val in value)"""
    from oracle import mask_ref
    raw = R.reg_raw('R1')
    c = R.reg_case('R1')
    for b in range(raw.shape[0]):
        m = torch.sigmoid(raw[b, :, 0, 0].double())
        assert abs(float(R.REG_LAMS[0] * m.sum()) - float(c['terms'][b, 0])) < 1e-12
        assert abs(float(R.REG_LAMS[1] * mask_ref.calc_tv_norm(m)) - float(c['terms'][b, 1])) < 1e-12
        assert float(c['terms'][b, 2]) == 0.0


# ---------------------------------------------------------------------------------------------------- (f) arguments
def test_bad_arguments_are_refused_by_name():
    import ivf_lib as L
    lib = L.lib()
    buf = np.full(64, -7.0, dtype=F32)
    p = buf.ctypes.data_as(ctypes.c_void_p)     # host memory: a refused call must not touch it (and never launches)

    def refused(rc, name):
        assert rc == -1 and name.encode() in lib.ivf_last_error(), (rc, lib.ivf_last_error())
        assert bool((buf == -7.0).all())

    refused(lib.ivf_stmask_axis_weights(4, 2, 1.0, None), "stmask_axis_weights")
    refused(lib.ivf_stmask_axis_weights(0, 2, 1.0, p), "stmask_axis_weights")
    refused(lib.ivf_stmask_axis_weights(4, 2, -1.0, p), "stmask_axis_weights")
    refused(lib.ivf_stmask_expand_fwd(None, p, p, p, 1, 1, 2, 2, 4, 4, None), "stmask_expand_fwd")
    refused(lib.ivf_stmask_expand_fwd(p, p, p, p, 1, 1, 33, 2, 64, 4, None), "stmask_expand_fwd")
    refused(lib.ivf_stmask_expand_bwd(p, p, p, None, 1, 1, 2, 2, 4, 4, None), "stmask_expand_bwd")
    refused(lib.ivf_stmask_expand_bwd(p, p, p, p, 1, 1, 2, 33, 4, 64, None), "stmask_expand_bwd")
    refused(lib.ivf_stfreeze_fwd(p, None, p, 1, 3, 4, 4, 0, None), "stfreeze_fwd")
    refused(lib.ivf_stfreeze_fwd(p, p, p, 1, 5, 4, 4, 4, None), "stfreeze_fwd")
    refused(lib.ivf_stfreeze_bwd(p, p, p, None, 1, 3, 4, 4, 0, None), "stfreeze_bwd")
    refused(lib.ivf_stfreeze_bwd(p, p, p, p, 1, 5, 4, 4, 4, None), "stfreeze_bwd")
    refused(lib.ivf_stfreeze_bwd(p, p, p, p, 1, 3, 65, 4, 0, None), "stfreeze_bwd")
    refused(lib.ivf_stmask_reg(p, 1, 4, 33, 1, 0.0, 0.0, 0.0, p, p, p, None), "stmask_reg")
    refused(lib.ivf_stmask_reg(None, 1, 4, 2, 2, 0.0, 0.0, 0.0, p, p, p, None), "stmask_reg")
    refused(lib.ivf_stmask_step(p, p, p, p, p, p, p, p, None, 1, 4, 2, 2, 0, 0.2, 0.9, 0.999, 1e-8, None), "stmask_step")
    assert lib.ivf_stsearch_workspace_bytes(1, 16, 224, 224, 33, 7) == 0 and b"stsearch_workspace_bytes" in lib.ivf_last_error()
    # M and dM dominate: 2 * B*T*H*W*4 bytes, plus the five small pieces rounded up to 256 bytes each
    n = lib.ivf_stsearch_workspace_bytes(32, 16, 224, 224, 7, 7)
    assert 2 * 32 * 16 * 224 * 224 * 4 < n < 2 * 32 * 16 * 224 * 224 * 4 + 3 * 32 * 16 * 49 * 4 + 7 * 256 + 32 * 16
    # the plans refuse before they touch anything, and their workspace sizes are not the new loop's business
    assert lib.ivf_i3d_stsearch(None, p, 1, p, p, p, p, p, p, 7, 7, 0.0, 0.0, 0.0, 0.2, 0.9, 0.999, 1e-8, 1, 1, None, p, None) != 0
    assert lib.ivf_clstm_stsearch(None, p, 1, p, p, p, p, p, p, 7, 7, 0.0, 0.0, 0.0, 0.2, 0.9, 0.999, 1e-8, 1, 1, None, p, None) != 0
    assert lib.ivf_i3d_stperturbed_forward(None, p, 1, p, p, None) != 0
    assert lib.ivf_clstm_stperturbed_forward(None, p, 1, p, p, None) != 0


# ---------------------------------------------------------------------------------------------------- chain case
def test_chain_case_leaves_no_clip_out():
    """the clips of the backbone chain case have no ambiguous pool window (clstm_refs' criterion), so the GPU test
    compares every clip; its float32 floor is a float32-sized number and dS is not degenerate"""
    c = R.chain_case()
    assert int(c['ambiguous'].sum()) == 0
    assert c['floor'] < 1e-3 and float(np.abs(c['dS'][:, 1:]).min(axis=(1, 2, 3)).max()) > 0
    assert bool((c['dS'][:, 0] == 0).all())
    note(f"stmask chain {R.CHAIN_CASE}: float32 floor of dS {c['floor']:.3e}, gate {c['gate']:.3e}")


# ---------------------------------------------------------------------------------------------------- fixture
def test_fixture_is_consistent_with_the_references(golden):
    """tests/golden/stmask.npz: shapes as documented, and its first trajectory row's regulariser columns are those of
    stmask_refs on the stored start (a spatially constant mask: tvs is an exact 0, l1 and tvt the temporal loss's)"""
    g = golden('stmask')
    b, T = g['init'].shape
    gh, gw = (int(v) for v in g['grid'])
    assert g['traj'].shape == (6, b, 5) and g['st_mask'].shape == (b, T, gh, gw) and g['time_mask'].shape == (b, T)
    raw = torch.from_numpy(g['init']).view(b, T, 1, 1).expand(b, T, gh, gw).contiguous()
    ref = R.reg_ref(raw, tuple(float(v) for v in g['lams']))
    assert bool(((torch.from_numpy(g['traj'][0, :, 1:4]).double() - ref['terms']).abs() <= ref['b_terms'] + R.gamma(2) * ref['terms']).all())
    assert bool((g['traj'][0, :, 3] == 0).all())
    # every column was rounded to float32 once: the four terms and J each carry one rounding
    tot = g['traj'][:, :, 1:].astype(np.float64).sum(axis=2)
    assert np.max(np.abs(g['traj'][:, :, 0] - tot) / tot) <= 4 * R.U
    # time_mask is the float32 mean of gh gw values in (0, 1): the any-order sum bound, relative to a mean <= 1
    assert np.max(np.abs(g['st_mask'].astype(np.float64).mean(axis=(2, 3)) - g['time_mask'])) <= 2 * gh * gw * R.U
