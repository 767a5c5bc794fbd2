"""CPU test of tests/leaf_refs.py: the fp64 references and the bounds the GPU leaf-kernel tests use are sound on the
very inputs those tests run, before any kernel is compared with them.

* a plain fp32 restatement of each kernel's arithmetic (sequential sum over positions, dot over channels, the pair
  formula of reverse_bwd) stays inside `sum_bound` against the fp64 reference;
* leaving out one element, or reading a neighbour in its place, breaks the bound.  How far follows from the bound
  itself: one of n like-sized terms is 1/n of the sum and the bound is 2 (n-1) 2^-24 of it, so the ratio is about
  2^23 / n^2 -- above 100 only up to n ~ 290.  The test asserts >= 100x for a single element where n <= 128; for the
  longer sums (C up to 1024, K 1500, npos 784) it asserts that a single mean-sized element or neighbour difference
  still leaves the bound (>= 2x) and that a dropped trailing eighth (the partial last channel slice) is >= 10x; for
  the 12544-pixel reverse_bwd sums a single pixel is below any sound worst-case bound, there a slipped gradient
  index is what must be (and is) caught at >= 100x;
* the resize, cam, head-backward and Adam references agree with the oracle / autograd / golden they restate.
"""
import numpy as np
import pytest
import torch

import leaf_refs as R
from conftest import GOLDEN


def _seq_sum32(x, axis):
    """sequential fp32 sum along `axis`, as a one-thread kernel loop does it"""
    x = np.moveaxis(np.asarray(x, dtype=np.float32), axis, 0)
    s = np.zeros(x.shape[1:], dtype=np.float32)
    for i in range(x.shape[0]):
        s = (s + x[i]).astype(np.float32)
    return s


def _dot32(a, b):
    """sum_c a[..., c] * b[..., c] with fp32 products, sequential fp32 sum"""
    return _seq_sum32((np.asarray(a, np.float32) * np.asarray(b, np.float32)).astype(np.float32), -1)


def _inside(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref.numpy())
    assert bool((err <= bound.numpy()).all()), f"{what}: fp32 restatement leaves the bound by {float((err - bound.numpy()).max()):.3e}"


def _detect_ratio(terms, bound):
    """terms [n] (fp64) of one sum and its bound: how far leaving out the median-sized non-zero term, or reading its
    neighbour instead, moves the sum, in units of the bound."""
    t = terms.numpy()
    nz = np.flatnonzero(t)
    i = nz[np.argsort(np.abs(t[nz]))[len(nz) // 2]]
    drop = abs(t[i]) / bound
    d = np.abs(np.diff(t))
    dn = np.flatnonzero(d)
    shift = (np.sort(d[dn])[len(dn) // 2] / bound) if len(dn) else np.inf
    return drop, shift


def _assert_detect(terms, bound, n, what):
    if n < 2 or bound == 0:
        return
    drop, shift = _detect_ratio(terms, bound)
    if n <= 128:
        assert drop >= 100, f"{what}: dropping one of {n} terms moves the sum by only {drop:.1f}x the bound"
        assert shift >= 100, f"{what}: a shifted index moves the sum by only {shift:.1f}x the bound"
        return
    # longer sums: a mean-sized term is 2^23 / (n (n-1)) times the bare sum bound (see the module docstring): 8x at
    # n = 1024, 3.7x at n = 1500.  So a single dropped element, or a neighbour read in its place, must still leave the
    # bound: asserted at 2x for the mean-sized term / mean neighbour difference (against the bound of the sum's own
    # stage), and a dropped trailing slice (the last eighth: 128 of 1024 channels, 104 of 1000) at 10x
    t = np.abs(terms.numpy())
    mean_drop = float(t[t > 0].mean()) / bound
    mean_shift = float(np.abs(np.diff(terms.numpy())).mean()) / bound
    assert mean_drop >= 2, f"{what}: dropping a mean-sized one of {n} terms moves the sum by only {mean_drop:.2f}x the bound"
    assert mean_shift >= 2, f"{what}: a shifted index moves the sum by only {mean_shift:.2f}x the bound"
    k = -(-n // 8)
    tail = abs(float(terms[-k:].sum())) / bound
    assert tail >= 10, f"{what}: dropping the last eighth of {n} terms moves the sum by only {tail:.1f}x the bound"


def test_sum_bound_formula():
    assert R.sum_bound(3.0, 1) == 0.0
    assert R.sum_bound(3.0, 5) == 2 * 4 * 2.0 ** -24 * 3.0
    assert torch.equal(R.sum_bound(torch.tensor([1.0, 2.0], dtype=torch.float64), 3),
                       torch.tensor([1.0, 2.0], dtype=torch.float64) * 4 * 2.0 ** -24)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("case", R.HEAD_CASES + ['spread'])
def test_head_forward_restatement_inside_bound(case, gated, bf16):
    spread = case == 'spread'
    case = R.HEAD_SPREAD_CASE if spread else case
    B, npos, C, K = case
    feat, w, bias = R.head_inputs(case, gated, bf16, spread)
    ref = R.head_fwd_ref(feat, w, bias, 1)
    pooled = (_seq_sum32(feat.numpy(), 1) * np.float32(1.0 / npos)).astype(np.float32)
    _inside(pooled, ref['pooled'], ref['b_pooled'], "pooled")
    logits = (_dot32(pooled[:, None, :], w.numpy()[None]) + bias.numpy()).astype(np.float32)
    _inside(logits, ref['logits'], ref['b_logits'], "logits")
    if spread:
        # a softmax without max-subtraction would overflow fp32 on these logits (sum of exp ~ e^80 < inf, but the
        # spread 160 > 88.7 + 87.3 underflows the small ones to 0 / overflows after any shift)
        assert float(ref['logits'].abs().max()) > 79 and np.isfinite(ref['probs'].numpy()).all()
    # one position / one channel left out, or a neighbour read in its place
    f = feat.double()
    _assert_detect(f[0, :, C - 1] / npos, float(ref['b_pooled'][0, C - 1]), npos, f"pooled {case}")
    k = K - 1
    _assert_detect(ref['pooled'][0] * w.double()[k], float(R.sum_bound((ref['pooled'][0] * w.double()[k]).abs().sum(), C + 2)),
                   C, f"logits {case}")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("softmax", [0, 1])
@pytest.mark.parametrize("case", R.HEAD_CASES)
def test_head_backward_reference_is_fp64_autograd(case, softmax, gated, bf16):
    """head_bwd_ref (explicit formula from probs) == autograd of feat.mean(1) @ w.T (+ softmax), by target and by
    dout, and dfeat = dpooled / npos gated by feat > 0; its fp32 restatement stays inside the bounds on every input
    the GPU test feeds (gated and un-gated feat, fp32 and bf16-valued)."""
    B, npos, C, K = case
    feat, w, _ = R.head_inputs(case, gated, bf16)
    for use_dout in (False, True):
        target = None if use_dout else R.head_targets(case)
        dout = R.head_dout(case) if use_dout else None
        f = feat.double().requires_grad_()
        pooled = f.mean(1)
        pooled.retain_grad()
        out = pooled @ w.double().T
        if softmax:
            out = torch.softmax(out, dim=1)
        loss = (out * dout.double()).sum() if use_dout else out[torch.arange(B), target.long()].sum()
        loss.backward()
        ref = R.head_bwd_ref(feat, w, out.detach(), target, dout, softmax, 0)     # probs in fp64: same numbers
        scale = float(pooled.grad.abs().max()) + 1e-300
        assert float((ref['dpooled'] - pooled.grad).abs().max()) <= 1e-12 * scale
        assert float((ref['dfeat'] - f.grad).abs().max()) <= 1e-12 * scale
        gref = R.head_bwd_ref(feat, w, out.detach(), target, dout, softmax, 1)
        assert bool((gref['dfeat'][~(feat > 0)] == 0).all()) and bool((~(feat > 0)).any()) and bool((feat > 0).any())
        assert torch.equal(gref['dfeat'][feat > 0], ref['dfeat'][feat > 0])
        # fp32 restatement with the fp32 probs the kernel is handed
        p32 = R.head_probs_input(case, softmax, gated, bf16)
        r32 = R.head_bwd_ref(feat, w, p32, target, dout, softmax, 0)
        d = dout.numpy() if use_dout else np.eye(K, dtype=np.float32)[target.long().numpy()]
        p = p32.numpy()
        if softmax:
            dot = _dot32(p, d) if use_dout else p[np.arange(B), target.long().numpy()]
            dl = (p * (d - dot[:, None]).astype(np.float32)).astype(np.float32)
        else:
            dl = d.astype(np.float32)
        dp = _dot32(dl[:, None, :], w.numpy().T[None])
        _inside(dp, r32['dpooled'], r32['b_dpooled'], f"dpooled {case}")
        df = (dp * np.float32(1.0 / npos)).astype(np.float32)
        _inside(df, r32['dfeat'][:, 0], r32['b_dfeat'][:, 0], f"dfeat {case}")
        if use_dout:        # (by target and without softmax the sum has a single non-zero term)
            t = torch.from_numpy(dl[0].astype(np.float64)) * w.double()[:, C - 1]      # (this stage's own bound)
            _assert_detect(t, float(R.sum_bound(t.abs().sum(), K + 1)), K, f"dpooled {case}")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("case", R.GRADCAM_CASES)
def test_gradcam_restatement_inside_bound(case, bf16):
    B, npos, C = case
    feat, grad = R.gradcam_inputs(case, bf16)
    ref = R.gradcam_ref(feat, grad)
    wts = (_seq_sum32(grad.numpy(), 1) / np.float32(npos)).astype(np.float32)
    _inside(wts, ref['weights'], ref['b_weights'], "weights")
    cam = np.maximum(_dot32(feat.numpy(), wts[:, None, :]), 0)
    _inside(cam, ref['cam'], ref['b_cam'], "cam")
    if B > 1:
        assert bool((ref['pre'] < -ref['b_cam']).any()), "no clearly negative cam in this input"
    assert bool((ref['pre'] > ref['b_cam']).any()) or case == (1, 1, 1)
    _assert_detect(grad.double()[0, :, C - 1] / npos, float(ref['b_weights'][0, C - 1]), npos, f"weights {case}")
    t = feat.double()[0, npos - 1] * ref['weights'][0]
    _assert_detect(t, float(R.sum_bound(t.abs().sum(), C + 1)), C, f"cam {case}")


def test_cam_reference_equals_oracle_cam_from_activations():
    """leaf_refs' weights / cam / resize / normalise chain == gradcam_ref.cam_from_activations on a [C,T',h,w] sample
    within fp32 rounding, per_frame 0 and 1."""
    from oracle import gradcam_ref
    g = torch.Generator().manual_seed(11)
    C, Tp, h, w, H, W, step = 24, 2, 4, 5, 20, 30, 4
    act = torch.randn(C, Tp, h, w, generator=g) + 0.5
    grad = torch.randn(C, Tp, h, w, generator=g) * 0.5 + 0.25
    feat = act.permute(1, 2, 3, 0).reshape(1, Tp * h * w, C)
    gr = grad.permute(1, 2, 3, 0).reshape(1, Tp * h * w, C)
    ref = R.gradcam_ref(feat, gr)
    for per_frame in (0, 1):
        vid, wts, cam = gradcam_ref.cam_from_activations(act.numpy(), grad.numpy(), Tp * step, W, H, bool(per_frame))
        assert np.allclose(wts, ref['weights'][0].numpy(), rtol=1e-5, atol=1e-7)
        assert np.allclose(cam.reshape(-1), ref['cam'][0].numpy(), rtol=1e-5, atol=1e-5)
        rs = R.resize_ref64(ref['cam'].view(1, Tp, h, w), H, W)
        out, _ = R.normalise_ref(rs, step, per_frame)
        assert out.shape == (1, Tp * step, H, W)
        assert np.allclose(vid, out[0].numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("case", R.RESIZE_CASES)
def test_resize_reference_agrees_with_oracle(case):
    """F.interpolate on float64 and the fp32 formula of gradcam_ref.resize_bilinear sample the same rule: they differ
    by fp32 rounding only (the measured figure the kernel's gate is built from), and the NaN cases are NaN in both."""
    B, ns, sh, sw, H, W, step = case
    cam = R.resize_input(case)
    gate, fig = R.resize_gate(cam, H, W)
    assert fig <= 2.0 ** -20 * float(cam.abs().max()), f"oracle and fp64 reference differ by {fig:.3e}: not the same rule"
    assert gate >= 2.0 ** -22 * float(cam.abs().max())
    if (sh, sw) == (H, W):
        assert torch.equal(R.resize_ref64(cam, H, W), cam.double())
    rs64 = R.resize_ref64(cam, H, W)
    rs32 = R.resize_oracle32(cam, H, W)
    for per_frame in (0, 1):
        o64, den = R.normalise_ref(rs64, step, per_frame)
        with np.errstate(invalid='ignore', divide='ignore'):
            o32, _ = R.normalise_ref(rs32, step, per_frame)
        nan64 = torch.isnan(o64)
        assert torch.equal(nan64, torch.isnan(o32))
        const = (sh, sw) == (1, 1)
        if const:
            assert bool(nan64.all())
        elif ns > 1 and per_frame:
            assert bool(nan64[0, step:2 * step].all()) and int(nan64.sum()) == step * H * W
        else:
            assert not bool(nan64.any())
        ok = ~nan64
        tol = R.normalise_tol(o64, den, gate, step)
        assert bool(((o32.double() - o64).abs()[ok] <= tol[ok]).all())
        k = step
        assert torch.equal(o64[:, 0::k], o64[:, k - 1::k]) or bool(nan64.any())


def test_pairs_ref_matches_oracle_and_golden():
    from oracle import mask_ref
    g = dict(np.load(GOLDEN + "/mask_ops.npz"))
    rows = [g[f'rev_{c}_mask'] for c in R.REV_GOLDEN]
    for (B, T) in R.REV_PAIR_CASES:
        masks = R.rev_masks(B, T, rows)
        assert masks.shape == (B, T) and masks.dtype == torch.float32
        for b in range(B):
            partner, weight = R.pairs_ref(masks[b].numpy())
            want = np.arange(T)
            for run in mask_ref.find_submasks_from_mask(masks[b]):
                for u in range(len(run) // 2):
                    want[run[u]], want[run[-(u + 1)]] = run[-(u + 1)], run[u]
            assert partner.tolist() == want.tolist()
            first = partner > np.arange(T)
            assert np.array_equal(weight[first], masks[b].numpy()[first])
    m16 = R.rev_masks(130, 16, rows)
    kinds = {tuple(r.tolist()) for r in m16}
    assert all(tuple(np.asarray(r, np.float32).tolist()) in kinds for r in rows)
    assert any((p := R.pairs_ref(r.numpy())[0])[0] != 0 for r in m16) and any(R.pairs_ref(r.numpy())[0][15] != 15 for r in m16)


@pytest.mark.parametrize("shape", R.REV_SHAPES)
def test_reverse_bwd_pair_formula_inside_bound(shape):
    """fp64 autograd of mask_ref.reverse == the pair formula; its fp32 restatement stays inside sum_bound(n = C*HW);
    a gradient read with a slipped channel stride leaves it by far."""
    B, C, T, HW = shape
    g = dict(np.load(GOLDEN + "/mask_ops.npz"))
    masks = R.rev_masks(B, T, [g[f'rev_{c}_mask'] for c in R.REV_GOLDEN])
    x, gy = R.rev_inputs(shape)
    dm, sa, first = R.reverse_bwd_terms(x, gy, masks)
    auto = R.reverse_bwd_ref(x, gy, masks)
    assert float((auto - dm).abs().max()) <= 1e-11 * (float(sa.max()) + 1e-300)
    assert bool((auto[~first] == 0).all()) and bool(first.any())
    bound = R.sum_bound(sa, C * HW)
    xn, gn = x.numpy(), gy.numpy()
    got = np.zeros((B, T), np.float32)
    bad = np.zeros((B, T), np.float64)
    for b, t in zip(*np.nonzero(first.numpy())):
        pt = int(R.pairs_ref(masks[b].numpy())[0][t])
        term = ((xn[b, :, pt] - xn[b, :, t]).astype(np.float32) * (gn[b, :, t] - gn[b, :, pt]).astype(np.float32)).astype(np.float32)
        got[b, t] = _seq_sum32(term.reshape(-1), 0)
        gs = np.roll(gn[b].reshape(C, T, HW), 1, axis=2)          # every pixel of g read one place off
        bad[b, t] = ((xn[b, :, pt] - xn[b, :, t]).astype(np.float64) * (gs[:, t] - gs[:, pt])).sum()
    _inside(got, dm, bound, f"reverse_bwd {shape}")
    f = first.numpy()
    ratio = np.abs(bad - dm.numpy())[f] / np.maximum(bound.numpy()[f], 1e-300)
    assert np.median(ratio) >= 100, f"a slipped gradient index moves dmask by only {np.median(ratio):.1f}x the bound"
    if C * HW <= 128:
        b, t = [int(v[0]) for v in np.nonzero(f)]
        pt = int(R.pairs_ref(masks[b].numpy())[0][t])
        term = ((x[b, :, pt] - x[b, :, t]).double() * (gy[b, :, t] - gy[b, :, pt]).double()).reshape(-1)
        drop, _ = _detect_ratio(term, float(bound[b, t]))
        assert drop >= 100


def test_adam_reference_reproduces_golden_trajectory():
    import ivf_recipe as RC
    g = dict(np.load(GOLDEN + "/mask_ops.npz"))
    p = torch.from_numpy(RC.uniform('g/adam/p', (16,), -5, 5))
    grads = torch.from_numpy(RC.uniform('g/adam/g', (12, 16), -1e-2, 1e-2))
    traj = [p.numpy().astype(np.float64)] + [q.numpy() for q, _, _ in R.adam_ref(p, grads, **R.ADAM)]
    assert np.allclose(np.array(traj), g['adam_traj'], rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("case", R.STEP_CASES)
def test_search_step_reference_inputs(case):
    """the fp32 chain gradient the kernel forms is within fp32 rounding of the fp64 one, and no element sits where
    dreg + dscore cancels (Adam's first steps divide by |g|)"""
    raw, sig, dscore, dreg, terms, score = R.step_inputs(case)
    g64 = R.step_grads64(sig, dscore, dreg)
    g32 = (dreg + dscore) * (sig * (1 - sig))
    assert float((g32.double() - g64).abs().max()) <= 8 * R.U * float(g64.abs().max())
    assert float(g64.abs().min()) > 1e-7
    last = list(R.adam_ref(raw.reshape(-1), g64.reshape(R.STEP_N, -1), **R.ADAM))[-1][0]
    assert bool(torch.isfinite(last).all())


@pytest.mark.parametrize("case", R.REG_CASES)
def test_regulariser_reference_constant_row(case):
    B, T = case
    mask, raw = R.reg_inputs(case)
    r = R.reg_const_row(B)
    for b in sorted({0, B - 1, max(r, 0)}):
        v, gr = R.tv_ref(mask[b])
        sg, l1, tv, dr = R.reg_ref(raw[b])
        if b == r:
            assert v == 0.0 and bool(torch.isnan(gr).all()) and tv == 0.0 and bool(torch.isnan(dr).all())
        else:
            assert v > 0 and bool(torch.isfinite(gr).all()) and bool(torch.isfinite(dr).all())


def test_fused_reference_shapes():
    for cin, cinp in R.FUSED_CINS:
        ws, sc, dy = R.fused_inputs(cin)
        assert R.fused_ref(ws, sc, dy).shape == (dy[0].shape[0], cin)
    assert sum(R.FUSED_COUTS) == 100
