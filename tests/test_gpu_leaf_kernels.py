"""The small kernels at both ends of the network, called directly through the C-ABI and compared with fp64 references
(tests/leaf_refs.py; the references and bounds are proven on the CPU by test_leaf_refs_host.py on the same inputs):
head forward / backward, arg-max, the Grad-CAM reductions and resize, the batched reverse perturbation, the batched
regulariser, the search step, sigmoid and the weight-pack helpers.

fp32 sums are gated by leaf_refs.sum_bound (no hand-picked constants); every output buffer has one sentinel row in
front and one behind, and both must come back untouched.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import leaf_refs as R
from conftest import note, rel_err

pytestmark = pytest.mark.gpu

SENT = -12345.0


def guarded(shape, dtype=torch.float32, sent=SENT):
    """(buffer, body): `body` has `shape`; the buffer holds one more leading row on each side, filled with `sent`."""
    shape = tuple(shape)
    buf = torch.full((shape[0] + 2,) + shape[1:], sent, dtype=dtype, device='cuda')
    return buf, buf[1:-1]


def untouched(buf, sent=SENT):
    s = torch.full_like(buf[0], sent)
    return bool(torch.equal(buf[0], s) and torch.equal(buf[-1], s))


def bits(t):
    """bit pattern (NaN-safe equality)"""
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def inside(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the bound, worst {float((err - bound).max()):.3e} over"
    return err


def dev_feat(feat, bf16):
    return (feat.bfloat16() if bf16 else feat).cuda().contiguous()


# ---------------------------------------------------------------------------------------------------- 1. head forward
def run_head_fwd(featd, wd, biasd, case, softmax, want_pooled, want_probs, bf16):
    import ivf_lib as L
    B, npos, C, K = case
    fn = L.lib().ivf_head_fwd_bf16 if bf16 else L.lib().ivf_head_fwd
    pb, pooled = guarded((B, C)) if want_pooled else (None, None)
    lb, logits = guarded((B, K))
    qb, probs = guarded((B, K)) if want_probs else (None, None)
    L.check(fn(L.ptr(featd), L.ptr(wd), L.ptr(biasd), L.ptr(pooled), L.ptr(logits), L.ptr(probs), B, npos, C, K,
               softmax, L.stream()))
    torch.cuda.synchronize()
    for b in (pb, lb, qb):
        assert b is None or untouched(b)
    return pooled, logits, probs


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", R.HEAD_CASES)
def test_head_fwd(case, bf16):
    """ivf_head_fwd / ivf_head_fwd_bf16: pooled and logits inside the running-sum bound, probs at the suite's fp32
    gate; softmax 0 copies the logits bit for bit; bias / pooled / probs NULL and given."""
    feat, w, bias = R.head_inputs(case, True, bf16)
    featd, wd, biasd = dev_feat(feat, bf16), w.cuda(), bias.cuda()
    for softmax, use_bias, want_pooled in itertools.product((0, 1), (False, True), (False, True)):
        ref = R.head_fwd_ref(feat, w, bias if use_bias else None, softmax)
        pooled, logits, probs = run_head_fwd(featd, wd, biasd if use_bias else None, case, softmax, want_pooled, True, bf16)
        if want_pooled:
            inside(pooled, ref['pooled'], ref['b_pooled'], f"pooled {case}")
        inside(logits, ref['logits'], ref['b_logits'], f"logits {case}")
        if softmax:
            err = (probs.double().cpu() - ref['probs']).abs()
            assert bool((err <= 1e-6 + 1e-5 * ref['probs']).all()), f"probs {case}: worst {float(err.max()):.3e}"
        else:
            assert torch.equal(bits(probs), bits(logits))
    _, logits2, none = run_head_fwd(featd, wd, biasd, case, 1, False, False, bf16)      # probs NULL
    assert none is None and torch.equal(bits(logits2), bits(logits))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_head_fwd_softmax_subtracts_the_maximum(bf16):
    """Logits spread over +-80: exp() of them overflows / underflows fp32 unless the maximum is subtracted first.
    probs are finite, sum to 1 within K * 2^-23, and match the fp64 reference computed from the inputs at the suite's
    gate 1e-6 + 1e-5 * ref; the softmax step alone (fp64 softmax of the kernel's own fp32 logits) is held to the same
    gate, and the logits to their sum bound."""
    case = R.HEAD_SPREAD_CASE
    B, npos, C, K = case
    feat, w, bias = R.head_inputs(case, True, bf16, spread=True)
    ref = R.head_fwd_ref(feat, w, None, 1)
    assert float(ref['logits'].max()) > 79 or float(ref['logits'].min()) < -79
    _, logits, probs = run_head_fwd(dev_feat(feat, bf16), w.cuda(), None, case, 1, False, True, bf16)
    inside(logits, ref['logits'], ref['b_logits'], "spread logits")
    p = probs.double().cpu()
    assert bool(torch.isfinite(p).all())
    assert float((p.sum(1) - 1).abs().max()) <= K * 2.0 ** -23
    want = torch.softmax(logits.double().cpu(), dim=1)
    err = (p - want).abs()
    note(f"leaf head_fwd spread{'_bf16' if bf16 else ''}: probs vs fp64 softmax of own logits {float(err.max()):.3e}, "
         f"vs fp64 from inputs {float((p - ref['probs']).abs().max()):.3e}")
    assert bool((err <= 1e-6 + 1e-5 * want).all())
    err_ref = (p - ref['probs']).abs()
    assert bool((err_ref <= 1e-6 + 1e-5 * ref['probs']).all()), f"spread probs vs fp64 from inputs: worst {float(err_ref.max()):.3e}"
    assert torch.equal(p.argmax(1), ref['probs'].argmax(1))


def test_head_fwd_refuses_what_does_not_fit_lds():
    import ivf_lib as L
    t = torch.zeros(64, device='cuda')
    for fn in (L.lib().ivf_head_fwd, L.lib().ivf_head_fwd_bf16):
        assert fn(L.ptr(t), L.ptr(t), None, None, L.ptr(t), L.ptr(t), 1, 1, 16000, 377, 1, L.stream()) == -1
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- 2. head backward
def run_head_bwd(featd, wd, probsd, targetd, doutd, case, softmax, gate, want, bf16):
    import ivf_lib as L
    B, npos, C, K = case
    fn = L.lib().ivf_head_bwd_bf16 if bf16 else L.lib().ivf_head_bwd
    w_score, w_dp, w_df = want
    sb, score = guarded((B,)) if w_score else (None, None)
    pb, dp = guarded((B, C)) if w_dp else (None, None)
    fb, df = guarded((B, npos, C), torch.bfloat16 if bf16 else torch.float32) if w_df else (None, None)
    L.check(fn(L.ptr(featd), L.ptr(wd), L.ptr(probsd), L.ptr(targetd), L.ptr(doutd), L.ptr(score), L.ptr(dp), L.ptr(df),
               B, npos, C, K, softmax, gate, L.stream()))
    torch.cuda.synchronize()
    for b in (sb, pb, fb):
        assert b is None or untouched(b)
    return score, dp, df


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", R.HEAD_CASES)
def test_head_bwd(case, bf16):
    """ivf_head_bwd / ivf_head_bwd_bf16 against the fp64 head backward (== fp64 autograd, test_leaf_refs_host.py):
    dpooled is the gradient w.r.t. the pooled vector (not divided by npos), dfeat = dpooled / npos gated by feat > 0
    with exact zeros where gated off, score[b] = probs[b, target[b]] bit for bit.  The bf16 entry point only changes
    storage: its dfeat equals the fp32 entry point's rounded once to bf16, its dpooled equals it bit for bit."""
    B, npos, C, K = case
    target = R.head_targets(case)
    dout = R.head_dout(case)
    targetd, doutd = target.cuda(), dout.cuda()
    for softmax, gate, use_dout in itertools.product((0, 1), (0, 1), (False, True)):
        feat, w, _ = R.head_inputs(case, bool(gate), bf16)
        probs = R.head_probs_input(case, softmax, bool(gate), bf16)
        ref = R.head_bwd_ref(feat, w, probs, None if use_dout else target, dout if use_dout else None, softmax, gate)
        wd, probsd = w.cuda(), probs.cuda()
        td, dd = (None, doutd) if use_dout else (targetd, None)
        f32d = feat.cuda()
        for want in ((1, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0)):
            if use_dout and want == (1, 0, 0):
                want = (0, 0, 0)            # nothing asked for: must be accepted and write nothing
            score, dp, df = run_head_bwd(f32d, wd, probsd, td, dd, case, softmax, gate, want, False)
            what = f"{case} softmax={softmax} gate={gate} dout={use_dout} want={want}"
            if dp is not None:
                inside(dp, ref['dpooled'], ref['b_dpooled'], "dpooled " + what)
                if C == 1000:       # the last, partial channel slice 896..999
                    assert bool((dp[:, 896:] != SENT).all())
            if df is not None:
                inside(df, ref['dfeat'], ref['b_dfeat'], "dfeat " + what)
                if gate:
                    assert bool(ref['off'].any()) and bool((df.cpu()[ref['off']] == 0).all())
                    live = ~ref['off'] & (ref['dfeat'].abs() > ref['b_dfeat'])
                    assert bool((df.cpu()[live] != 0).all())
            if score is not None and not use_dout:
                assert torch.equal(bits(score.cpu()), bits(ref['score']))
            elif score is not None:
                assert bool((score == SENT).all())          # no target: score is not written
            if bf16:
                s16, dp16, df16 = run_head_bwd(dev_feat(feat, True), wd, probsd, td, dd, case, softmax, gate, want, True)
                if dp is not None:
                    assert torch.equal(bits(dp16), bits(dp))
                if df is not None:
                    assert torch.equal(bits(df16), bits(df.bfloat16()))
                if score is not None:
                    assert torch.equal(bits(s16), bits(score))


# ---------------------------------------------------------------------------------------------------- 3. arg-max
@pytest.mark.parametrize("case", R.ARGMAX_CASES)
def test_argmax_first_maximum_wins(case):
    import ivf_lib as L
    b, K = case
    x = R.argmax_input(case)
    xd = x.cuda()
    buf, out = guarded((b,), torch.int32, -7)
    L.check(L.lib().ivf_argmax(L.ptr(xd), b, K, L.ptr(out), L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf, -7)
    want = np.argmax(x.numpy(), axis=1)
    assert out.cpu().numpy().tolist() == want.tolist()
    if b > 1:
        assert want[0] == 0 and want[b - 1] == K - 1
    else:       # the single row is quantised: its last entry holds the maximum, tied with any earlier one
        assert float(x[0, K - 1]) == float(x[0].max())


# ---------------------------------------------------------------------------------------------------- 4. Grad-CAM reduce
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", R.GRADCAM_CASES)
def test_gradcam_reduce(case, bf16):
    """ivf_gradcam_reduce / _bf16: weights = grad.mean(1) and cam = relu(feat @ weights) inside the propagated sum
    bound; where the reference is negative by more than the bound the kernel gives exactly 0.0."""
    import ivf_lib as L
    B, npos, C = case
    feat, grad = R.gradcam_inputs(case, bf16)
    ref = R.gradcam_ref(feat, grad)
    fd, gd = dev_feat(feat, bf16), dev_feat(grad, bf16)
    wb, wts = guarded((B, C))
    cb, cam = guarded((B, npos))
    fn = L.lib().ivf_gradcam_reduce_bf16 if bf16 else L.lib().ivf_gradcam_reduce
    L.check(fn(L.ptr(fd), L.ptr(gd), L.ptr(wts), L.ptr(cam), B, npos, C, L.stream()))
    torch.cuda.synchronize()
    assert untouched(wb) and untouched(cb)
    inside(wts, ref['weights'], ref['b_weights'], f"weights {case}")
    inside(cam, ref['cam'], ref['b_cam'], f"cam {case}")
    neg = ref['pre'] < -ref['b_cam']
    assert bool((cam.cpu()[neg] == 0).all()) and bool((cam >= 0).all())
    if B > 1:
        assert bool(neg.any())


# ---------------------------------------------------------------------------------------------------- 5. resize + normalise
@pytest.mark.parametrize("per_frame", [0, 1])
@pytest.mark.parametrize("case", R.RESIZE_CASES)
def test_cam_resize_normalise(case, per_frame):
    """ivf_cam_resize_normalise against F.interpolate(bilinear, align_corners=False) on float64, then x - min, / max.
    The gate on the resized map is measured: 4x the distance of the same fp32 formula (gradcam_ref.resize_bilinear)
    from the fp64 reference on this input, floor 2^-22 * max|cam|; it is applied to minmax_ws directly and, propagated
    through (x - mn) / den, to the output.  A constant slice gives NaN exactly as numpy's 0/0."""
    import ivf_lib as L
    B, ns, sh, sw, H, W, step = case
    cam = R.resize_input(case)
    gate, fig = R.resize_gate(cam, H, W)
    rs = R.resize_ref64(cam, H, W)
    want, den = R.normalise_ref(rs, step, per_frame)
    camd = cam.cuda()
    ob, out = guarded((B * ns * step, H, W))
    mb, mm = guarded((B * ns, 2))
    L.check(L.lib().ivf_cam_resize_normalise(L.ptr(camd), L.ptr(out), L.ptr(mm), B, ns, sh, sw, H, W, step, per_frame,
                                             L.stream()))
    torch.cuda.synchronize()
    assert untouched(ob) and untouched(mb)
    got = out.view(B, ns, step, H, W)
    for r in range(1, step):
        assert torch.equal(bits(got[:, :, r]), bits(got[:, :, 0]))
    mmc = mm.double().cpu().view(B, ns, 2)
    mm_err = max(float((mmc[..., 0] - rs.amin(dim=(2, 3))).abs().max()), float((mmc[..., 1] - rs.amax(dim=(2, 3))).abs().max()))
    g = out.double().cpu().view(B, ns * step, H, W)
    nan_ref = torch.isnan(want)
    assert torch.equal(torch.isnan(g), nan_ref)
    if (sh, sw) == (1, 1):
        assert bool(nan_ref.all())
    elif ns > 1 and per_frame:
        assert bool(nan_ref[0, step:2 * step].all()) and int(nan_ref.sum()) == step * H * W
    else:
        assert not bool(nan_ref.any())          # per_frame = 0: a constant slice among varying ones stays finite
    ok = ~nan_ref
    err = (g - want).abs()
    tol = R.normalise_tol(want, den, gate, step)
    note(f"leaf resize {case} per_frame={per_frame}: oracle-vs-fp64 {fig:.3e} gate {gate:.3e} | kernel min/max vs fp64 "
         f"{mm_err:.3e}, normalised out vs fp64 {float(err[ok].max()) if bool(ok.any()) else 0.0:.3e}")
    assert mm_err <= gate
    assert bool((err[ok] <= tol[ok]).all())


# ---------------------------------------------------------------------------------------------------- 6. batched reverse
def golden_rows(golden):
    g = golden('mask_ops')
    return [g[f'rev_{c}_mask'] for c in R.REV_GOLDEN]


def run_pairs_batched(maskd, B, T):
    import ivf_lib as L
    pb, partner = guarded((B, T), torch.int32, -7)
    wb, weight = guarded((B, T))
    L.check(L.lib().ivf_submask_pairs_batched(L.ptr(maskd), B, T, 0.1, L.ptr(partner), L.ptr(weight), L.stream()))
    torch.cuda.synchronize()
    assert untouched(pb, -7) and untouched(wb)
    return partner, weight


@pytest.mark.parametrize("case", R.REV_PAIR_CASES, ids=lambda c: f"B{c[0]}-T{c[1]}")
def test_submask_pairs_batched_rows_equal_single_row_call(case, golden):
    """row b of ivf_submask_pairs_batched == ivf_submask_pairs on that row (pinned by the golden), partner and weight
    bit for bit; and both equal the CPU restatement of mask.py:40-85."""
    import ivf_lib as L
    B, T = case
    masks = R.rev_masks(B, T, golden_rows(golden))
    maskd = masks.cuda()
    partner, weight = run_pairs_batched(maskd, B, T)
    rb1, run1 = guarded((B, T), torch.int32, -7)
    pb1, p1 = guarded((B, T), torch.int32, -7)
    wb1, w1 = guarded((B, T))
    for b in range(B):
        L.check(L.lib().ivf_submask_pairs(L.ptr(maskd[b]), T, 0.1, L.ptr(run1[b]), L.ptr(p1[b]), L.ptr(w1[b]), L.stream()))
    torch.cuda.synchronize()
    assert untouched(rb1, -7) and untouched(pb1, -7) and untouched(wb1)
    assert torch.equal(partner, p1) and torch.equal(bits(weight), bits(w1))
    ref = [R.pairs_ref(masks[b].numpy()) for b in range(B)]
    assert np.array_equal(partner.cpu().numpy(), np.stack([r[0] for r in ref]))
    assert np.array_equal(weight.cpu().numpy(), np.stack([r[1] for r in ref]))


@pytest.mark.parametrize("shape", R.REV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reverse_fwd_batched(shape, golden):
    """NCTHW and 4-channel channels-last against mask_ref.reverse per clip at the gate of the existing reverse test;
    the pad channels are exactly 0 and the two layouts bit-identical."""
    import ivf_lib as L
    B, C, T, HW = shape
    masks = R.rev_masks(B, T, golden_rows(golden))
    x, _ = R.rev_inputs(shape)
    xd, maskd = x.cuda(), masks.cuda()
    partner, weight = run_pairs_batched(maskd, B, T)
    nb, p_nc = guarded((B, C, T, HW))
    cb, p_cl = guarded((B, T, HW, 4))
    L.check(L.lib().ivf_reverse_fwd_batched(L.ptr(xd), L.ptr(partner), L.ptr(weight), L.ptr(p_nc), B, C, T, HW, 0, L.stream()))
    L.check(L.lib().ivf_reverse_fwd_batched(L.ptr(xd), L.ptr(partner), L.ptr(weight), L.ptr(p_cl), B, C, T, HW, 4, L.stream()))
    torch.cuda.synchronize()
    assert untouched(nb) and untouched(cb)
    want = R.reverse_ref(x, masks)
    for b in range(B):
        assert rel_err(p_nc[b].cpu().numpy(), want[b].numpy()) < 1e-6
    assert torch.equal(bits(p_cl[..., :C].permute(0, 3, 1, 2)), bits(p_nc))
    if C < 4:
        assert float(p_cl[..., C:].abs().max()) == 0.0
    assert not torch.equal(p_nc, xd)            # some clip is perturbed


@pytest.mark.parametrize("shape", R.REV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reverse_bwd(shape, golden):
    """ivf_reverse_bwd against fp64 autograd of mask_ref.reverse with loss (p * g).sum(), inside the sum bound with
    n = C * HW; g in NCTHW and channels-last rows of 4 and 8 (pad channels NaN: reading one poisons the sum).  Entries
    that are not the first-half member of a pair are exactly 0.0; a second call gives the same bits."""
    import ivf_lib as L
    B, C, T, HW = shape
    masks = R.rev_masks(B, T, golden_rows(golden))
    x, g = R.rev_inputs(shape)
    ref = R.reverse_bwd_ref(x, g, masks)
    _, sa, first = R.reverse_bwd_terms(x, g, masks)
    bound = R.sum_bound(sa, C * HW)
    xd, maskd = x.cuda(), masks.cuda()
    partner, _ = run_pairs_batched(maskd, B, T)
    nws = L.lib().ivf_freeze_bwd_workspace_bytes(B, T)
    wsbuf = torch.full((nws + 512,), 0xA5, dtype=torch.uint8, device='cuda')        # 256 guard bytes on each side
    ws = wsbuf[256:256 + nws]
    assert bool(first.any()) and (B == 1 or not bool(first.any(1).all()))
    for cpad in (0, 4, 8):
        if cpad == 0:
            gd = g.cuda()
        else:
            gd = torch.full((B, T, HW, cpad), float('nan'), device='cuda')
            gd[..., :C] = g.cuda().permute(0, 2, 3, 1)
        outs = []
        for _ in range(2):
            db, dm = guarded((B, T))
            L.check(L.lib().ivf_reverse_bwd(L.ptr(xd), L.ptr(partner), L.ptr(gd), L.ptr(dm), B, C, T, HW, cpad, L.ptr(ws),
                                            L.stream()))
            torch.cuda.synchronize()
            assert untouched(db)
            assert bool((wsbuf[:256] == 0xA5).all()) and bool((wsbuf[256 + nws:] == 0xA5).all())
            outs.append(dm)
        assert torch.equal(bits(outs[0]), bits(outs[1]))
        dm = outs[0]
        inside(dm, ref, bound, f"dmask {shape} g_cpad={cpad}")
        assert bool((dm.cpu()[~first] == 0).all())
        off = ~first.any(1)                    # all-off rows (and rows without a pair): all-zero dmask
        assert bool((dm.cpu()[off] == 0).all())


# ---------------------------------------------------------------------------------------------------- 7. regulariser, step
@pytest.mark.parametrize("case", R.REG_CASES, ids=lambda c: f"B{c[0]}-T{c[1]}")
def test_tv_norm_and_mask_reg_batched(case):
    """Every row of the batched ivf_tv_norm / ivf_mask_reg equals the B = 1 call on that row bit for bit (that call
    is pinned by the golden) and matches calc_tv_norm (+ L1) under fp64 autograd at the existing gates; the constant
    row (val == 0) has NaN gradients and its neighbours stay finite."""
    import ivf_lib as L
    lib = L.lib()
    B, T = case
    mask, raw = R.reg_inputs(case)
    md, rd = mask.cuda(), raw.cuda()
    vb, val = guarded((B,))
    gb, grad = guarded((B, T))
    L.check(lib.ivf_tv_norm(L.ptr(md), B, T, 3.0, 3.0, L.ptr(val), L.ptr(grad), L.stream()))
    vb2, val2 = guarded((B,))
    L.check(lib.ivf_tv_norm(L.ptr(md), B, T, 3.0, 3.0, L.ptr(val2), None, L.stream()))       # grad NULL
    sb, sig = guarded((B, T))
    tb, terms = guarded((B, 2))
    db, dreg = guarded((B, T))
    L.check(lib.ivf_mask_reg(L.ptr(rd), B, T, R.LAM1, R.LAM2, L.ptr(sig), L.ptr(terms), L.ptr(dreg), L.stream()))
    singles = [guarded(sh) for sh in ((B,), (B, T), (B, T), (B, 2), (B, T))]
    v1, g1, s1, t1, d1 = (body for _, body in singles)
    for b in range(B):
        L.check(lib.ivf_tv_norm(L.ptr(md[b]), 1, T, 3.0, 3.0, L.ptr(v1[b:]), L.ptr(g1[b]), L.stream()))
        L.check(lib.ivf_mask_reg(L.ptr(rd[b]), 1, T, R.LAM1, R.LAM2, L.ptr(s1[b]), L.ptr(t1[b]), L.ptr(d1[b]), L.stream()))
    torch.cuda.synchronize()
    for b_ in [vb, gb, vb2, sb, tb, db] + [buf for buf, _ in singles]:
        assert untouched(b_)
    assert torch.equal(bits(val), bits(v1)) and torch.equal(bits(grad), bits(g1)) and torch.equal(bits(val2), bits(val))
    assert torch.equal(bits(sig), bits(s1)) and torch.equal(bits(terms), bits(t1)) and torch.equal(bits(dreg), bits(d1))
    r = R.reg_const_row(B)
    val_c, grad_c, sig_c, terms_c, dreg_c = (t.double().cpu() for t in (val, grad, sig, terms, dreg))
    for b in range(B):
        rv, rg = R.tv_ref(mask[b])
        rs, l1, tv, rd_ = R.reg_ref(raw[b])
        assert float((sig_c[b] - rs).abs().max()) <= 2.0 ** -22
        assert abs(float(terms_c[b, 0]) - l1) <= 2e-5 * abs(l1)
        if b == r:
            assert float(val_c[b]) == 0.0 and bool(torch.isnan(grad_c[b]).all()) and bool(torch.isnan(rg).all())
            assert float(terms_c[b, 1]) == 0.0 and bool(torch.isnan(dreg_c[b]).all()) and bool(torch.isnan(rd_).all())
            continue
        assert abs(float(val_c[b]) - rv) <= 2e-5 * abs(rv)
        assert bool(torch.isfinite(grad_c[b]).all()) and rel_err(grad_c[b].numpy(), rg.numpy()) < 2e-4
        assert abs(float(terms_c[b, 1]) - tv) <= 2e-5 * abs(tv)
        assert bool(torch.isfinite(dreg_c[b]).all()) and rel_err(dreg_c[b].numpy(), rd_.numpy()) < 2e-4


def ulp_distance(a, b):
    ia, ib = (t.contiguous().view(torch.int32).long() for t in (a, b))
    ia = torch.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = torch.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int((ia - ib).abs().max())


@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: f"B{c[0]}-T{c[1]}")
def test_search_step_trajectory(case):
    """12 steps of ivf_search_step against torch fp64 Adam on g = (dreg + dscore) * sig * (1 - sig) and against
    ivf_adam_step fed that g formed in fp32 on the device, at the Adam gate of test_regulariser_and_adam; traj_row =
    [l1 + tv + score, l1, tv, score] with the last three copied bit for bit; traj_row NULL is accepted."""
    import ivf_lib as L
    lib = L.lib()
    B, T = case
    raw, sig, dscore, dreg, terms, score = R.step_inputs(case)
    a = R.ADAM
    g64 = R.step_grads64(sig, dscore, dreg)
    bufs = [guarded((B, T)) for _ in range(3)]
    (rb, rawd), (mb, am), (vb, av) = bufs
    rawd.copy_(raw.cuda()); am.zero_(); av.zero_()
    others = [guarded((B, T)) for _ in range(6)]
    raw_n, m_n, v_n, raw_a, m_a, v_a = (body for _, body in others)      # traj NULL run; ivf_adam_step run
    for t_ in (m_n, v_n, m_a, v_a):
        t_.zero_()
    raw_n.copy_(raw.cuda()); raw_a.copy_(raw.cuda())
    sigd, dsd, drd, td, scd = (t.cuda() for t in (sig, dscore, dreg, terms, score))
    worst_ulp = 0
    for i, (p64, m64, v64) in enumerate(R.adam_ref(raw, g64, **a)):
        tb, traj = guarded((B, 4))
        args = (L.ptr(sigd[i]), L.ptr(dsd[i]), L.ptr(drd[i]), L.ptr(td[i]), L.ptr(scd[i]))
        tail = (B, T, i + 1, a['lr'], a['b1'], a['b2'], a['eps'], L.stream())
        L.check(lib.ivf_search_step(L.ptr(rawd), *args, L.ptr(am), L.ptr(av), L.ptr(traj), *tail))
        L.check(lib.ivf_search_step(L.ptr(raw_n), *args, L.ptr(m_n), L.ptr(v_n), None, *tail))
        g32 = ((drd[i] + dsd[i]) * (sigd[i] * (1 - sigd[i]))).contiguous()
        L.check(lib.ivf_adam_step(L.ptr(raw_a), L.ptr(g32), L.ptr(m_a), L.ptr(v_a), B * T, i + 1, a['lr'], a['b1'], a['b2'],
                                  a['eps'], L.stream()))
        torch.cuda.synchronize()
        assert untouched(tb) and all(untouched(b[0]) for b in bufs + others)
        for got, want, name in ((rawd, p64, 'raw_mask'), (am, m64, 'exp_avg'), (av, v64, 'exp_avg_sq')):
            assert np.allclose(got.cpu().numpy(), want.numpy(), rtol=2e-6, atol=2e-6), f"{name} step {i + 1}"
        for got, other in ((rawd, raw_a), (am, m_a), (av, v_a)):
            assert np.allclose(got.cpu().numpy(), other.cpu().numpy(), rtol=2e-6, atol=2e-6)
        worst_ulp = max(worst_ulp, ulp_distance(rawd, raw_a))
        assert torch.equal(bits(rawd), bits(raw_n)) and torch.equal(bits(am), bits(m_n)) and torch.equal(bits(av), bits(v_n))
        tc = traj.cpu()
        assert torch.equal(bits(tc[:, 1:3]), bits(terms[i])) and torch.equal(bits(tc[:, 3]), bits(score[i]))
        assert torch.equal(bits(tc[:, 0]), bits((terms[i][:, 0] + terms[i][:, 1]) + score[i]))
    note(f"leaf search_step {case}: largest ulp distance of raw_mask from ivf_adam_step over {R.STEP_N} steps: {worst_ulp}")


@pytest.mark.parametrize("n", R.SIGMOID_N)
def test_sigmoid(n):
    import ivf_lib as L
    x = R.sigmoid_input(n)
    xd = x.cuda()
    yb, y = guarded((n,))
    L.check(L.lib().ivf_sigmoid(L.ptr(xd), L.ptr(y), n, L.stream()))
    torch.cuda.synchronize()
    assert untouched(yb)
    yc = y.double().cpu()
    assert float((yc - torch.sigmoid(x.double())).abs().max()) <= 2.0 ** -22
    assert bool(((yc >= 0) & (yc <= 1)).all())


# ---------------------------------------------------------------------------------------------------- 8. weight packs
MODES = ["fp32", "bf16x3", "bf16x6", "bf16act"]
NAN_BITS = 0x7fc07fc0           # a NaN as fp32 and as either bf16 half
NAN_BITS_REF = 0x7fa17fa1       # another one, for the buffer compared against: a gap shared by both would differ


def nan_buffer(n, pattern=NAN_BITS):
    """(buffer, body of n floats) prefilled with NaN patterns, 8 guard floats on each side"""
    buf = torch.full((n + 16,), pattern, dtype=torch.int32, device='cuda').view(torch.float32)
    return buf, buf[8:8 + n]


def no_nan_left(buf, body, math, pattern=NAN_BITS):
    """guards intact and no prefill left in the body: no fp32 word of it (fp32 pack), no 16-bit half (bf16 planes)"""
    i = buf.view(torch.int32)
    if not bool((i[:8] == pattern).all() and (i[-8:] == pattern).all()):
        return False
    if math == "fp32":
        return not bool((body.view(torch.int32) == pattern).any())
    half = pattern & 0xffff
    return not bool(((body.view(torch.int16).int() & 0xffff) == half).any())


@pytest.mark.parametrize("math", MODES)
@pytest.mark.parametrize("case", R.PACK_ROWS_CASES, ids=lambda c: "|".join(map(str, c[0])) + f"-k{c[3]}")
def test_pack_fwd_rows_equals_pack_of_concatenated_weight(case, math):
    import ivf_lib as L
    lib = L.lib()
    couts, cin, cinp, k = case
    mm = L.MATH_MODES[math]
    ws = [w.cuda() for w in R.pack_weights(couts, cin, k, 'rows')]
    total = sum(couts)
    wcat = torch.cat(ws, 0).contiguous()
    n = lib.ivf_conv3d_pack_fwd_elems(total, cinp, k, k, k, mm)
    rbuf, ref = nan_buffer(n, NAN_BITS_REF)
    L.check(lib.ivf_conv3d_pack_fwd(L.ptr(wcat), L.ptr(ref), total, cin, cinp, k, k, k, mm, L.stream()))
    offs = np.concatenate([[0], np.cumsum(couts)[:-1]]).tolist()
    for order in (list(range(len(ws))), list(reversed(range(len(ws))))):
        buf, body = nan_buffer(n)
        for u in order:
            L.check(lib.ivf_conv3d_pack_fwd_rows(L.ptr(ws[u]), L.ptr(body), couts[u], cin, cinp, k, k, k, offs[u], total, mm,
                                                 L.stream()))
        torch.cuda.synchronize()
        assert no_nan_left(buf, body, math) and no_nan_left(rbuf, ref, math, NAN_BITS_REF)
        assert torch.equal(bits(body), bits(ref))


@pytest.mark.parametrize("math", MODES)
@pytest.mark.parametrize("cin,cinp", R.FUSED_CINS)
def test_pack_bwd_fused1x1_and_its_gemm(cin, cinp, math):
    """Units packed side by side in every order give the same bytes with no prefill left (the unit ending at Ktotal
    zeroes the row padding); the backward GEMM over [dY_0 | dY_1 dY_2] read from two buffers then equals
    sum_u (dY_u * scale_u) @ W_u at the mode's gate, pad output channels exactly 0."""
    import ivf_lib as L
    lib = L.lib()
    mm = L.MATH_MODES[math]
    act16 = math == "bf16act"
    ws, sc, dy = R.fused_inputs(cin, act16)
    wsd, scd = [w.cuda() for w in ws], [s.cuda() for s in sc]
    couts = R.FUSED_COUTS
    ktot = sum(couts)
    offs = [0, couts[0], couts[0] + couts[1]]
    n = lib.ivf_conv3d_pack_bwd_fused1x1_elems(ktot, cinp, mm)
    packs = []
    for order in itertools.permutations(range(3)):
        buf, body = nan_buffer(n)
        for u in order:
            L.check(lib.ivf_conv3d_pack_bwd_fused1x1(L.ptr(wsd[u]), L.ptr(scd[u]), L.ptr(body), couts[u], cin, cinp, offs[u],
                                                     ktot, mm, L.stream()))
        torch.cuda.synchronize()
        assert no_nan_left(buf, body, math), f"order {order}"
        packs.append((buf, body))
        assert torch.equal(bits(body), bits(packs[0][1])), f"order {order}"
    wb = packs[0][1]
    Bc, Tt, Hh, Ww = 2, 3, 4, 5
    M = Bc * Tt * Hh * Ww
    adt = torch.bfloat16 if act16 else torch.float32
    in1 = torch.zeros(M + 1, couts[0], dtype=adt, device='cuda')            # (one spare row behind each source)
    in2 = torch.zeros(M + 1, couts[1] + couts[2], dtype=adt, device='cuda')
    in1[:M] = dy[0].cuda().to(adt)
    in2[:M] = torch.cat([dy[1], dy[2]], 1).cuda().to(adt)
    ob, out = guarded((M, cinp), adt)
    e = L.ConvDesc()
    e.B, e.Ti, e.Hi, e.Wi = Bc, Tt, Hh, Ww
    e.To, e.Ho, e.Wo = Tt, Hh, Ww
    e.Cin, e.in_ld, e.in_coff = ktot, couts[0], 0
    e.K0, e.in2_ld, e.in2_coff = couts[0], couts[1] + couts[2], 0
    e.in2 = ctypes.c_void_p(in2.data_ptr())
    e.Cout, e.out_ld, e.out_coff = cinp, cinp, 0
    e.kT = e.kH = e.kW = 1
    e.sT = e.sH = e.sW = 1
    e.math = mm
    L.check(lib.ivf_conv3d(ctypes.byref(e), L.ptr(in1), L.ptr(wb), None, None, None, L.ptr(out), L.stream()))
    torch.cuda.synchronize()
    assert untouched(ob)
    want = R.fused_ref(ws, sc, dy)
    got = out.double().cpu()
    if cinp > cin:
        assert float(got[:, cin:].abs().max()) == 0.0
    if act16:
        tol = 2.0 ** -8 * want.abs() + 1e-5 * want.abs().max()      # as test_every_conv_variant_bf16_activations
        assert bool(((got[:, :cin] - want).abs() <= tol).all())
    else:
        assert rel_err(got[:, :cin].numpy(), want.numpy()) < (1e-4 if math == "bf16x3" else 1e-5)
