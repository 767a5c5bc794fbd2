"""The spatio-temporal mask kernels of csrc/stmask_ops.hip, called directly through the C-ABI, and the spacetime search
loop on both backbones (tests/stmask_refs.py: case tables, float64 references and the derivation of every gate;
tests/test_stmask_refs_host.py proves them on the CPU on the same inputs).

The feature has no counterpart in the reference: it is pinned by torch autograd on the reference's models,
not by reference output.  Kernel gates are bit equality, an exact 0.0, or a bound derived in stmask_refs' docstring and
applied per element; every output has a sentinel row in front and one behind and starts out as a NaN pattern.
"""
import numpy as np
import pytest
import torch

import mask_refs
import stmask_refs as R
from conftest import note, ranking_consistent
from leaf_refs import sum_bound
from test_gpu_leaf_kernels import bits, guarded, untouched
from test_gpu_mask_kernels import NAN_BITS, bounded, grad_layout, same

pytestmark = pytest.mark.gpu


def nan_guarded(shape):
    buf, body = guarded(shape)
    bits(body).fill_(NAN_BITS)
    return buf, body


# ---------------------------------------------------------------------------------------------------- expand
def run_expand(Sd, AHd, AWd, case, bwd=False):
    import ivf_lib as L
    B, T, gh, gw, H, W, sigma = case
    B = Sd.shape[0]
    buf, out = nan_guarded((B, T, gh, gw) if bwd else (B, T, H, W))
    fn = L.lib().ivf_stmask_expand_bwd if bwd else L.lib().ivf_stmask_expand_fwd
    L.check(fn(L.ptr(Sd), L.ptr(AHd), L.ptr(AWd), L.ptr(out), B, T, gh, gw, H, W, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), "expand: a sentinel row was written"
    assert not bool(torch.isnan(out).any()), "expand: an element was never written"
    return out


@pytest.mark.parametrize("name", list(R.EXPAND_CASES))
def test_expand_fwd_and_bwd(name):
    case = B, T, gh, gw, H, W, sigma = R.EXPAND_CASES[name]
    c = R.expand_case(name)
    Sd, AHd, AWd, dMd = (c[k].cuda() for k in ('S', 'AH', 'AW', 'dM'))
    M = run_expand(Sd, AHd, AWd, case)
    dS = run_expand(dMd, AHd, AWd, case, bwd=True)
    wf = bounded(M, c['M'], c['bM'], f"expand_fwd {name}")
    wb = bounded(dS, c['dS'], c['bdS'], f"expand_bwd {name}")
    assert float(M.min()) >= 0.0 and float(M.max()) <= 1.0 + R.gamma(gh + gw + 2)
    if (gh, gw, sigma) == (H, W, 0.0):
        assert torch.equal(bits(M), bits(Sd)), "the identity expand is not bit-exact"
    if B > 1:        # a clip's rows do not depend on the batch it ran in
        for r in range(B):
            assert torch.equal(bits(run_expand(Sd[r:r + 1].contiguous(), AHd, AWd, case)), bits(M[r:r + 1]))
            assert torch.equal(bits(run_expand(dMd[r:r + 1].contiguous(), AHd, AWd, case, bwd=True)), bits(dS[r:r + 1]))
    assert torch.equal(bits(run_expand(dMd, AHd, AWd, case, bwd=True)), bits(dS)), "expand_bwd differs between two calls"
    note(f"stmask expand {name} {case}: worst err/gate fwd {wf:.3f} bwd {wb:.4f}")


# ---------------------------------------------------------------------------------------------------- per-pixel freeze
def run_stfwd(xd, Md, shape, cpad):
    import ivf_lib as L
    B, C, T, HW = shape
    buf, p = nan_guarded((B, C, T, HW) if cpad == 0 else (B, T, HW, cpad))
    L.check(L.lib().ivf_stfreeze_fwd(L.ptr(xd), L.ptr(Md), L.ptr(p), B, C, T, HW, cpad, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), f"stfreeze_fwd out_cpad={cpad}: a sentinel row was written"
    assert not bool(torch.isnan(p).any()), f"stfreeze_fwd out_cpad={cpad}: an element was never written"
    return p


def run_stbwd(xd, Md, gd, shape, cpad):
    import ivf_lib as L
    B, C, T, HW = shape
    buf, dM = nan_guarded((B, T, HW))
    L.check(L.lib().ivf_stfreeze_bwd(L.ptr(xd), L.ptr(Md), L.ptr(gd), L.ptr(dM), B, C, T, HW, cpad, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), f"stfreeze_bwd g_cpad={cpad}: a sentinel row was written"
    return dM


@pytest.mark.parametrize("name", list(R.STFREEZE_CASES))
def test_stfreeze_fwd(name):
    import ivf_lib as L
    shape = B, C, T, HW = R.STFREEZE_CASES[name]
    c = R.stfreeze_case(name)
    xd, Md = c['x'].cuda(), c['M'].cuda()
    p = run_stfwd(xd, Md, shape, 0)
    worst = bounded(p, c['P'], c['bP'], f"stfreeze_fwd {name}")
    assert torch.equal(bits(p[:, :, 0]), bits(xd[:, :, 0]))
    if T == 1:
        assert torch.equal(bits(p), bits(xd))
    # spatially constant M == the temporal kernel, bit for bit, in every layout
    rows = c['rows'].cuda()
    Mc = rows.view(B, T, 1).expand(B, T, HW).contiguous()
    for cpad in R.out_layouts(C):
        pcl = run_stfwd(xd, Md, shape, cpad)
        if cpad:
            assert torch.equal(bits(pcl[..., :C].permute(0, 3, 1, 2)), bits(p)), f"out_cpad={cpad} differs from NCTHW"
            if cpad > C:
                assert torch.equal(bits(pcl[..., C:]), torch.zeros_like(bits(pcl[..., C:]))), f"out_cpad={cpad}: pad lane not +0.0"
        tb, tp = nan_guarded(tuple(pcl.shape))
        L.check(L.lib().ivf_freeze_fwd(L.ptr(xd), L.ptr(rows), L.ptr(tp), B, C, T, HW, 1, cpad, L.stream()))
        assert torch.equal(bits(run_stfwd(xd, Mc, shape, cpad)), bits(tp)), f"constant M, out_cpad={cpad}: not ivf_freeze_fwd's bits"
    if C > 4:
        buf, q = guarded((B, T, HW, 4))
        assert L.lib().ivf_stfreeze_fwd(L.ptr(xd), L.ptr(Md), L.ptr(q), B, C, T, HW, 4, L.stream()) == -1
        torch.cuda.synchronize()
        assert untouched(buf) and bool((q == -12345.0).all())
    note(f"stmask stfreeze_fwd {name} {shape}: worst err/gate {worst:.3f}; layouts {R.out_layouts(C)} bit-equal")


@pytest.mark.parametrize("name", list(R.STFREEZE_CASES))
def test_stfreeze_bwd(name):
    import ivf_lib as L
    shape = B, C, T, HW = R.STFREEZE_CASES[name]
    c = R.stfreeze_case(name)
    xd, Md = c['x'].cuda(), c['M'].cuda()
    dM = run_stbwd(xd, Md, grad_layout(c['g'], 0), shape, 0)
    worst = bounded(dM, c['dM'], c['b_dM'], f"stfreeze_bwd {name}")
    assert torch.equal(bits(dM[:, 0]), torch.zeros_like(bits(dM[:, 0]))), "dM[:, 0] is not +0.0"
    for cpad in R.out_layouts(C)[1:]:          # NaN pad lanes
        assert torch.equal(bits(run_stbwd(xd, Md, grad_layout(c['g'], cpad), shape, cpad)), bits(dM)), f"g_cpad={cpad} differs"
    if C > 4:
        buf, q = guarded((B, T, HW))
        assert L.lib().ivf_stfreeze_bwd(L.ptr(xd), L.ptr(Md), L.ptr(grad_layout(c['g'], 8)), L.ptr(q), B, C, T, HW, 4, L.stream()) == -1
        torch.cuda.synchronize()
        assert untouched(buf) and bool((q == -12345.0).all())
    # constant M: the pixel sum is the temporal kernel's dmask
    rows = c['rows']
    Mc = rows.view(B, T, 1).expand(B, T, HW).contiguous().cuda()
    dMc = run_stbwd(xd, Mc, grad_layout(c['g'], 0), shape, 0)
    tref = mask_refs.freeze_bwd_ref(c['x'], c['g'], rows)
    ws = torch.empty(L.lib().ivf_freeze_bwd_workspace_bytes(B, T), dtype=torch.uint8, device='cuda')
    dmask = torch.empty(B, T, device='cuda')
    L.check(L.lib().ivf_freeze_bwd(L.ptr(xd), L.ptr(rows.cuda()), L.ptr(grad_layout(c['g'], 0)), L.ptr(dmask), None, B, C, T, HW, 1, 0,
                                   L.ptr(ws), L.stream()))
    summed = dMc.sum(dim=2)                      # float32
    gate = tref['b_dmask'] + sum_bound(dMc.double().abs().sum(dim=2).cpu(), HW)
    err = (summed.double().cpu() - dmask.double().cpu()).abs()
    assert bool((err <= gate).all()), f"sum_px dM vs ivf_freeze_bwd: worst {float((err - gate).max()):.3e} over"
    assert bool((err[:, 0] == 0).all())
    note(f"stmask stfreeze_bwd {name} {shape}: worst err/gate {worst:.3f}; sum over pixels vs ivf_freeze_bwd "
         f"{float((err[:, 1:] / gate[:, 1:]).max()) if T > 1 else 0.0:.4f} of its gate")


# ---------------------------------------------------------------------------------------------------- regulariser, step
@pytest.mark.parametrize("name", list(R.REG_CASES))
def test_reg_and_step(name):
    import ivf_lib as L
    B, T, gh, gw = R.REG_CASES[name]
    c = R.reg_case(name)
    lam = R.REG_LAMS
    raw = c['raw'].cuda()
    sb, sig = nan_guarded((B, T, gh, gw))
    tb, terms = nan_guarded((B, 3))
    db, dreg = nan_guarded((B, T, gh, gw))
    L.check(L.lib().ivf_stmask_reg(L.ptr(raw), B, T, gh, gw, lam[0], lam[1], lam[2], L.ptr(sig), L.ptr(terms), L.ptr(dreg), L.stream()))
    torch.cuda.synchronize()
    assert untouched(sb) and untouched(tb) and untouched(db)
    ws = bounded(sig, c['sig'], c['b_sig'], f"stmask_reg {name} sig")
    wt = bounded(terms, c['terms'], c['b_terms'], f"stmask_reg {name} terms")
    wd = bounded(dreg, c['dreg'], c['b_dreg'], f"stmask_reg {name} dreg")
    # clip 0's cell (0,0) is constant over time: its time pieces are exact zeros, the gradient finite
    assert bool(torch.isfinite(dreg).all())
    if gh * gw == 1:
        assert torch.equal(dreg[0].flatten().cpu(), torch.full((T,), lam[0], dtype=torch.float32))
        assert float(terms[0, 1]) == 0.0 and bool((terms[:, 2] == 0).all())
    # loop tail: trajectory row, chain through the sigmoid, Adam == ivf_adam_step on the same gradient
    g = R._gen('step', name)
    dsc = ((torch.rand(B, T, gh, gw, generator=g) - 0.5) * 0.01).cuda()
    score = torch.rand(B, generator=g).cuda()
    m0 = ((torch.rand(B, T, gh, gw, generator=g) - 0.5) * 0.01).cuda()
    v0 = (torch.rand(B, T, gh, gw, generator=g) * 1e-4).cuda()
    step, lr, b1, b2, eps = 3, 0.2, 0.9, 0.999, 1e-8
    raw1, m1, v1 = raw.clone(), m0.clone(), v0.clone()
    rb, row = nan_guarded((B, 5))
    L.check(L.lib().ivf_stmask_step(L.ptr(raw1), L.ptr(sig), L.ptr(dsc), L.ptr(dreg), L.ptr(terms), L.ptr(score), L.ptr(m1), L.ptr(v1),
                                    L.ptr(row), B, T, gh, gw, step, lr, b1, b2, eps, L.stream()))
    torch.cuda.synchronize()
    assert untouched(rb)
    sc, dc, dd = sig.cpu(), dsc.cpu(), dreg.cpu()          # IEEE float32 on the host, the kernel's expression
    gi = ((dd + dc) * (sc * (1.0 - sc))).cuda().contiguous()
    raw2, m2, v2 = raw.clone(), m0.clone(), v0.clone()
    L.check(L.lib().ivf_adam_step(L.ptr(raw2), L.ptr(gi), L.ptr(m2), L.ptr(v2), raw2.numel(), step, lr, b1, b2, eps, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(raw1), bits(raw2)) and torch.equal(bits(m1), bits(m2)) and torch.equal(bits(v1), bits(v2))
    t = terms.cpu()
    want = torch.stack([t[:, 0] + t[:, 1] + t[:, 2] + score.cpu(), t[:, 0], t[:, 1], t[:, 2], score.cpu()], dim=1)
    assert torch.equal(bits(row.cpu()), bits(want))
    note(f"stmask reg {name} {(B, T, gh, gw)}: worst err/gate sig {ws:.3f} terms {wt:.3f} dreg {wd:.3f}; step == ivf_adam_step")


# ---------------------------------------------------------------------------------------------------- chain, ConvLSTM
@pytest.fixture(scope="module")
def chain():
    import ivf_engine
    c = R.chain_case()
    case = c['case']
    eng = ivf_engine.CLSTMEngine(5, (case.C, case.T, case.H, case.W), max_batch=case.B, hidden=case.hid, layers=case.layers,
                                 kernel=case.k, stride=case.s, softmax=case.softmax, batch_norm=case.batch_norm)
    eng.load_state_dict(c['sd'])
    return eng, c


def _pieces(eng, c, raw, lam):
    """one iteration by its pieces: (sig, terms, dreg, dS, score)"""
    import ivf_lib as L
    case = c['case']
    b, T, gh, gw = raw.shape
    C, H, W = case.C, case.H, case.W
    x = c['x'].cuda()
    sig, terms, dreg = torch.empty_like(raw), torch.empty(b, 3, device='cuda'), torch.empty_like(raw)
    L.check(L.lib().ivf_stmask_reg(L.ptr(raw), b, T, gh, gw, lam[0], lam[1], lam[2], L.ptr(sig), L.ptr(terms), L.ptr(dreg), L.stream()))
    M = eng.st_expand(sig, (gh, gw), R.CHAIN_SIGMA)
    P = torch.empty_like(x)
    L.check(L.lib().ivf_stfreeze_fwd(L.ptr(x), L.ptr(M), L.ptr(P), b, C, T, H * W, 0, L.stream()))
    probs = eng.forward(P)
    score, dx = eng.backward(b, target=c['targets'])
    dM = torch.empty(b, T, H, W, device='cuda')
    L.check(L.lib().ivf_stfreeze_bwd(L.ptr(x), L.ptr(M), L.ptr(dx), L.ptr(dM), b, C, T, H * W, 0, L.stream()))
    dS = torch.empty_like(raw)
    _, _, _, AH, AW = eng._st_axes((gh, gw), R.CHAIN_SIGMA)
    L.check(L.lib().ivf_stmask_expand_bwd(L.ptr(dM), L.ptr(AH), L.ptr(AW), L.ptr(dS), b, T, gh, gw, H, W, L.stream()))
    torch.cuda.synchronize()
    return sig, terms, dreg, dS, score, probs, M


def test_chain_dS_matches_autograd_through_the_convlstm(chain):
    """sigmoid -> expand -> per-pixel freeze -> ConvLSTM -> score, and back: dS against torch fp64 autograd through
    clstm_refs' functional model, every clip, at clstm_refs' gate (GATE_MARGIN x the float32 floor of dS itself)"""
    import clstm_refs as CR
    eng, c = chain
    assert int(c['ambiguous'].sum()) == 0
    raw = c['raw'].cuda()
    sig, terms, dreg, dS, score, probs, M = _pieces(eng, c, raw, (0.01, 0.02, 0.02))
    # the engine builds its matrices with the library's host function: the same floats as the reference's
    _, _, _, AH, AW = eng._st_axes(R.CHAIN_GRID, R.CHAIN_SIGMA)
    assert torch.equal(AH.cpu(), c['AH']) and torch.equal(AW.cpu(), c['AW'])
    e = CR.elem_err(dS.cpu().numpy(), c['dS'])
    note(f"stmask chain {R.CHAIN_CASE}: dS floor {c['floor']:.3e} gpu {float(e.max()):.3e} ratio {float(e.max()) / c['floor']:.2f} "
         f"(gate {CR.GATE_MARGIN:g}x, clips compared {len(e)}/{len(e)})")
    assert bool((e <= c['gate']).all()), f"dS: {e} > gate {c['gate']:.3e}"
    assert torch.equal(bits(dS[:, 0]), torch.zeros_like(bits(dS[:, 0])))


def test_driver_iteration_equals_its_pieces(chain):
    """ivf_clstm_stsearch for one iteration == the same kernels called one by one: raw, Adam state and trajectory row
    bit for bit; st_perturbed_forward == forward of the staged clip"""
    import ivf_lib as L
    eng, c = chain
    lam = (0.01, 0.02, 0.03)
    raw = c['raw'].cuda()
    b, T, gh, gw = raw.shape
    sig, terms, dreg, dS, score, probs, M = _pieces(eng, c, raw, lam)
    raw1, m1, v1 = raw.clone(), torch.zeros_like(raw), torch.zeros_like(raw)
    row = torch.empty(b, 5, device='cuda')
    L.check(L.lib().ivf_stmask_step(L.ptr(raw1), L.ptr(sig), L.ptr(dS), L.ptr(dreg), L.ptr(terms), L.ptr(score), L.ptr(m1), L.ptr(v1),
                                    L.ptr(row), b, T, gh, gw, 1, 0.2, 0.9, 0.999, 1e-8, L.stream()))
    raw2 = raw.clone()
    traj, (m2, v2, done) = eng.st_search(c['x'].cuda(), c['targets'], raw2, lam[0], lam[1], 1, R.CHAIN_GRID, R.CHAIN_SIGMA, lam3=lam[2])
    torch.cuda.synchronize()
    assert done == 1 and tuple(traj.shape) == (1, b, 5)
    assert torch.equal(bits(traj[0]), bits(row)) and torch.equal(bits(raw2), bits(raw1))
    assert torch.equal(bits(m2), bits(m1)) and torch.equal(bits(v2), bits(v1))
    assert torch.equal(bits(eng.st_perturbed_forward(c['x'].cuda(), M)), bits(probs))


def test_clstm_1x1_grid_reduces_to_the_temporal_search(chain):
    """grid 1x1, sigma 0, lam3 = 0: M is the temporal mask on every pixel, so the staged clip is the temporal loop's bit
    for bit, dS is ivf_freeze_bwd's dmask within the kernels' bounds, and six iterations track eng.search within 1e-2"""
    import ivf_lib as L
    eng, c = chain
    case = c['case']
    x = c['x'].cuda()
    b, C, T, HW = x.shape[0], case.C, case.T, case.H * case.W
    raw_t = (torch.rand(b, T, generator=R._gen('reduce')) * 4 - 2).cuda().contiguous()
    S = torch.sigmoid(raw_t)
    M = eng.st_expand(S.view(b, T, 1, 1), (1, 1), 0.0)
    assert torch.equal(bits(M), bits(S.view(b, T, 1, 1).expand(b, T, case.H, case.W).contiguous()))
    P1, P2 = torch.empty_like(x), torch.empty_like(x)
    L.check(L.lib().ivf_stfreeze_fwd(L.ptr(x), L.ptr(M), L.ptr(P1), b, C, T, HW, 0, L.stream()))
    L.check(L.lib().ivf_freeze_fwd(L.ptr(x), L.ptr(S), L.ptr(P2), b, C, T, HW, 1, 0, L.stream()))
    assert torch.equal(bits(P1), bits(P2)) and torch.equal(bits(eng.st_freeze(x, M)), bits(P1))
    # dS against dmask on a common upstream gradient
    eng.forward(P1)
    _, dx = eng.backward(b, target=c['targets'])
    dM, dS, dmask = torch.empty(b, T, HW, device='cuda'), torch.empty(b, T, device='cuda'), torch.empty(b, T, device='cuda')
    L.check(L.lib().ivf_stfreeze_bwd(L.ptr(x), L.ptr(M), L.ptr(dx), L.ptr(dM), b, C, T, HW, 0, L.stream()))
    _, _, _, AH, AW = eng._st_axes((1, 1), 0.0)
    L.check(L.lib().ivf_stmask_expand_bwd(L.ptr(dM), L.ptr(AH), L.ptr(AW), L.ptr(dS), b, T, 1, 1, case.H, case.W, L.stream()))
    ws = torch.empty(L.lib().ivf_freeze_bwd_workspace_bytes(b, T), dtype=torch.uint8, device='cuda')
    L.check(L.lib().ivf_freeze_bwd(L.ptr(x), L.ptr(S), L.ptr(dx), L.ptr(dmask), None, b, C, T, HW, 1, 0, L.ptr(ws), L.stream()))
    torch.cuda.synchronize()
    tref = mask_refs.freeze_bwd_ref(c['x'].view(b, C, T, HW), dx.cpu().view(b, C, T, HW), S.cpu())
    gate = 2 * tref['b_dmask'] + sum_bound(tref['sabs'], max(HW, 2) + 1)     # both kernels' sums, and the expand's
    err = (dS.double().cpu() - dmask.double().cpu()).abs()
    assert bool((err <= gate).all())
    # six iterations of both loops from the same start
    ra, rb = raw_t.clone(), raw_t.clone().view(b, T, 1, 1).contiguous()
    ta, _ = eng.search(x, c['targets'], ra, 0.01, 0.02, 6)
    tb, _ = eng.st_search(x, c['targets'], rb, 0.01, 0.02, 6, (1, 1), 0.0, lam3=0.0)
    ta, tb = ta.cpu().numpy(), tb.cpu().numpy()
    assert bool((tb[:, :, 3] == 0).all())
    rel = np.abs(tb[:, :, [0, 1, 2, 4]] - ta) / np.abs(ta)
    note(f"stmask 1x1 reduction on the ConvLSTM: six-iteration trajectory within {float(rel.max()):.2e} of eng.search")
    assert float(rel.max()) < 1e-2
    assert float((torch.sigmoid(rb.view(b, T)) - torch.sigmoid(ra)).abs().max()) < 1e-2


def test_resumed_st_search_continues_bit_for_bit(chain):
    """4 iterations of the spacetime loop in one call == 2 + 2 through the returned state (first_step = steps done +
    1): raw, Adam moments and trajectory rows bit for bit"""
    from search_resume import check_resumed_search
    eng, c = chain
    x = c['x'].cuda()

    def search(raw, n, state):
        return eng.st_search(x, c['targets'], raw, 0.01, 0.02, n, R.CHAIN_GRID, R.CHAIN_SIGMA, lam3=0.03, state=state)
    check_resumed_search(search, c['raw'].cuda().contiguous(), 4, 2)


# ---------------------------------------------------------------------------------------------------- I3D
@pytest.fixture(scope="module", params=["fp32", "bf16x3", "bf16x6"])
def s16(request):
    import ivf_engine
    import ivf_recipe as RC
    eng = ivf_engine.I3DEngine(174, (3, 16, 224, 224), max_batch=2, softmax=True, math=request.param)
    eng.load_state_dict(RC.i3d_state_dict(num_classes=174))
    return eng


def test_i3d_1x1_grid_reduces_to_the_temporal_search(s16, golden):
    """the same reduction through the I3D plan (16-byte channels-last staging): staged input bit for bit, six iterations
    within the 1e-2 trajectory gate of test_gpu_i3d.py"""
    import ivf_lib as L
    import ivf_recipe as RC
    g = golden('search')
    x = torch.from_numpy(np.stack([RC.clip(21), RC.clip(7)])).cuda()
    b, C, T, H, W = x.shape
    target = s16.argmax(s16.forward(x)).tolist()
    raw_t = torch.from_numpy(np.stack([g['s16_init'], g['s16_init']])).cuda().contiguous()
    S = torch.sigmoid(raw_t)
    M = s16.st_expand(S.view(b, T, 1, 1), (1, 1), 0.0)
    P1, P2 = torch.empty(b, T, H * W, 4, device='cuda'), torch.empty(b, T, H * W, 4, device='cuda')
    L.check(L.lib().ivf_stfreeze_fwd(L.ptr(x), L.ptr(M), L.ptr(P1), b, C, T, H * W, 4, L.stream()))
    L.check(L.lib().ivf_freeze_fwd(L.ptr(x), L.ptr(S), L.ptr(P2), b, C, T, H * W, 1, 4, L.stream()))
    assert torch.equal(bits(P1), bits(P2))
    assert torch.equal(bits(s16.st_perturbed_forward(x, M)), bits(s16.perturbed_forward(x, S, 'freeze')))
    ra, rb = raw_t.clone(), raw_t.clone().view(b, T, 1, 1).contiguous()
    ta, _ = s16.search(x, target, ra, 0.01, 0.02, 6)
    tb, _ = s16.st_search(x, target, rb, 0.01, 0.02, 6, (1, 1), 0.0, lam3=0.0)
    ta, tb = ta.cpu().numpy(), tb.cpu().numpy()
    rel = np.abs(tb[:, :, [0, 1, 2, 4]] - ta) / np.abs(ta)
    note(f"stmask 1x1 reduction on I3D {s16.math}: six-iteration trajectory within {float(rel.max()):.2e} of eng.search")
    assert float(rel.max()) < 1e-2
    fa, fb = torch.sigmoid(ra).cpu().numpy(), torch.sigmoid(rb.view(b, T)).cpu().numpy()
    assert float(np.abs(fa - fb).max()) < 1e-2
    for r in range(b):
        assert ranking_consistent(np.argsort(-fb[r], kind='stable'), fa[r], 1e-2)


# ---------------------------------------------------------------------------------------------------- drivers
RECORD_KEYS = {'true_class', 'pred_class', 'video_id', 'time_mask', 'original_score_guess', 'original_score_true',
               'freeze_score', 'reverse_score'}


def test_smth_driver_spacetime_records(tmp_path, monkeypatch):
    """find_masks(maskType='spacetime') on two synthetic clips for two iterations: the records carry st_mask [T,gh,gw]
    beside every existing key, time_mask is its spatial mean, the strips are written from the expanded mask; and
    maskType='central' does not see the new keyword arguments: its records are byte-identical with and without them"""
    import pickle
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    import ivf_recipe as RC
    from models import I3D_doubled
    m = I3D_doubled.Model(174, last_stride=1, stride_mod_layers="", softMax=1)
    m.load_state_dict({"module." + k: v for k, v in RC.to_torch(RC.i3d_state_dict(num_classes=174)).items()})
    m = m.cuda().eval()
    monkeypatch.chdir(tmp_path)
    hp = {"batch_size": 2, "gradCamType": "guessed"}

    def run(mask_type, **kw):
        loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)
        drv.find_masks(loader, m, hp, 0.01, 0.02, 2, mask_type, "freeze", classOI=None, doGradCam=False, runTempMask=True,
                       verbose=False, **kw)
        return ivf_find_masks.find_masks_impl.last_results[0]

    st = run("spacetime")
    assert len(st) == 2
    for r in st:
        assert set(r) == RECORD_KEYS | {'st_mask'}
        assert r['st_mask'].shape == (16, 7, 7) and r['st_mask'].dtype == np.float32 and r['time_mask'].shape == (16,)
        assert float(r['st_mask'].min()) > 0 and float(r['st_mask'].max()) < 1
        mean = r['st_mask'].astype(np.float64).mean(axis=(1, 2))
        assert np.max(np.abs(mean - r['time_mask'])) <= R.gamma(16) * np.max(mean)      # 7 + 7 + 2 roundings
        assert np.isfinite(r['freeze_score']) and np.isfinite(r['reverse_score'])
    # the mask moved off its spatially constant start within two Adam steps of 0.2
    assert max(float(np.ptp(r['st_mask'], axis=(1, 2)).max()) for r in st) > 0
    assert len(list((tmp_path / "cam_saved_images").rglob("mygif.gif"))) == 2             # strips from the expanded mask
    st34 = run("spacetime", maskGrid=(3, 4), maskSigma=8.0, lam3=0.0)
    assert st34[0]['st_mask'].shape == (16, 3, 4)
    plain = pickle.dumps(run("central"))
    assert set(pickle.loads(plain)[0]) == RECORD_KEYS
    assert pickle.dumps(run("central", maskGrid=(3, 4), maskSigma=8.0, lam3=0.5)) == plain


def test_kth_driver_spacetime_on_the_convlstm(tmp_path, monkeypatch):
    """the KTH driver with the ConvLSTM backbone: default grid 4 x 5 at 120 x 160, T = 32"""
    import FindMasksComparison_I3D_KTH as drv
    import ivf_find_masks
    import ivf_recipe as RC
    from models import CLSTM_4
    m = CLSTM_4.Model(num_classes=6, nb_lstm_units=4, channels=3, conv_kernel_size=(5, 5), lstm_layers=2,
                      step=32, image_size=(160, 120), conv_stride=2, effective_step=[7, 15, 23, 31])
    m.load_state_dict(RC.to_torch(RC.clstm_state_dict(channels=3, tag='clstm3')))
    m = m.cuda().eval()
    monkeypatch.chdir(tmp_path)
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 32, 120, 160), 6, first_id=7)
    masks = drv.find_masks(loader, m, {"batch_size": 2, "gradCamType": "guessed"}, 0.02, 0.04, 2, 1, "spacetime", "freeze",
                           classOI=None, doGradCam=False, runTempMask=True, verbose=False)
    recs = ivf_find_masks.find_masks_impl.last_results[0]
    assert len(masks) == 2 and len(recs) == 2
    for r, mk in zip(recs, masks):
        assert set(r) == RECORD_KEYS | {'st_mask'} and r['st_mask'].shape == (32, 4, 5)
        assert np.array_equal(mk.cpu().numpy(), r['time_mask'])
    # the perturbed-frame PNGs are written from the per-pixel freeze; the mark in their corner is time_mask (KTH:360-367)
    from PIL import Image
    px = np.asarray(Image.open(next(p for p in (tmp_path / "cam_saved_images").rglob("case7pert3.png"))))
    assert px.shape == (120, 160, 3) and (px[:10, :10, 0] == np.uint8(np.float32(recs[0]['time_mask'][3]) * 255)).all()
    with pytest.raises(Exception):
        drv.find_masks(loader, m, {"batch_size": 2, "gradCamType": "guessed"}, 0.02, 0.04, 2, 1, "spacetime", "reverse",
                       classOI=None, doGradCam=False, runTempMask=True, verbose=False)


# ---------------------------------------------------------------------------------------------------- I3D, fixture
def test_i3d_spacetime_search_vs_fixture(s16, golden):
    """six iterations of ivf_i3d_stsearch against tests/golden/stmask.npz (make_golden_stmask.py: the reference's
    I3D_doubled.Model under the torch restatement of the perturbation and loss, torch autograd, torch.optim.Adam), at
    the gates test_gpu_i3d.py applies to search.npz.  The tvs column starts at an exact 0 (a spatially constant start)
    and stays below 1e-6 over these iterations: it has no relative error of its own and is held to the loss's gate,
    1e-2 of J, as the term of J that it is.  Measured on the MI355X (fp32 / bf16x3 / bf16x6): J within 9e-6 / 4e-5 /
    2e-5, score 2e-5 / 4e-5 / 3e-5, max |S - fixture| 3.4e-3 / 8.1e-3 / 7.8e-3 (cells whose gradient passes near zero in
    an early iteration take an Adam step of 0.2 in the other direction; the same spread test_gpu_i3d.py records)."""
    import ivf_recipe as RC
    g = golden('stmask')
    gh, gw = (int(v) for v in g['grid'])
    lam = [float(v) for v in g['lams']]
    x = torch.from_numpy(np.stack([RC.clip(int(c)) for c in g['clips']])).cuda()
    b, C, T, H, W = x.shape
    probs = s16.forward(x)
    target = s16.argmax(probs)
    assert target.tolist() == g['target'].tolist()                                   # integer output: bit-exact
    raw = torch.from_numpy(g['init']).cuda().view(b, T, 1, 1).expand(b, T, gh, gw).contiguous()
    traj, _ = s16.st_search(x, target, raw, lam[0], lam[1], 6, (gh, gw), float(g['sigma']), lam3=lam[2])
    traj, ref = traj.cpu().numpy().astype(np.float64), g['traj'].astype(np.float64)
    assert traj.shape == ref.shape == (6, b, 5)
    rel = np.abs(traj - ref) / np.maximum(np.abs(ref), 1e-300)
    S = torch.sigmoid(raw).cpu().numpy()
    tmask = S.astype(np.float64).mean(axis=(2, 3))
    dS = float(np.max(np.abs(S - g['st_mask'])))
    note(f"stmask 6-iteration search vs fixture, {s16.math}: J {rel[:, :, 0].max():.2e} l1 {rel[:, :, 1].max():.2e} "
         f"tvt {rel[:, :, 2].max():.2e} score {rel[:, :, 4].max():.2e} (relative); tvs abs {np.abs(traj - ref)[:, :, 3].max():.2e}; "
         f"max|S - fixture| {dS:.2e}")
    assert rel[:, :, [0, 1, 2]].max() < 1e-2                      # north_star: loss trajectory within 1e-2
    assert rel[:, :, 4].max() < 2e-3
    assert bool((np.abs(traj - ref)[:, :, 3] < 1e-2 * np.abs(ref[:, :, 0])).all())
    assert dS < 1e-2
    for r in range(b):
        assert ranking_consistent(np.argsort(-tmask[r], kind='stable'), g['time_mask'][r], 1e-2)
        assert np.array_equal(tmask[r] > 0.5, g['time_mask'][r] > 0.5) or np.min(np.abs(g['time_mask'][r] - 0.5)) < 1e-2
