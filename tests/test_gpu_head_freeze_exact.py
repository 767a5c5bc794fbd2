"""ivf_head_fwd and the channels-last ivf_freeze_fwd, bit for bit against numpy fp32 restatements of the order the
kernels sum in.

Head: pooled[c] = (sum over p ascending of feat[p][c]) * (1 / npos); a logit is 64 lane partials (lane l adds
pooled[c] * W[k][c] for c = l, l + 64, ... ascending, product and sum rounded separately), folded by the
__shfl_down tree at 32, 16, ..., 1, plus the bias (or + 0.0f); the softmax takes the maximum and adds the
exponentials left to right.  expf is the device library's, which the host's does not reproduce to the bit, so the
probabilities are compared with what the one-workgroup-per-clip kernel this form replaced returned for the same input
(tests/golden/head_exact.npz, written by that library from head_case() below).

Freeze: P[0] = X[0], P[u] = (1 - m[u]) * X[u] + m[u] * P[u-1], every operation rounded (no contraction)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEAD = (3, 2 * 7 * 7, 1024, 174)   # B, npos, C, K: the I3D head


def head_case(bf16):
    B, npos, C, K = HEAD
    rng = np.random.default_rng(2024)
    feat = np.maximum(rng.standard_normal((B, npos, C)), 0).astype(np.float32)
    w = (rng.standard_normal((K, C)) * 0.05).astype(np.float32)
    bias = (rng.standard_normal(K) * 0.1).astype(np.float32)
    if bf16:   # bf16-representable features (truncated), so both storages see the same values
        feat = (feat.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    return feat, w, bias


def head_ref(feat, w, bias):
    B, npos, C = feat.shape
    K = w.shape[0]
    s = np.zeros((B, C), np.float32)
    for p in range(npos):
        s = s + feat[:, p]
    pooled = s * (np.float32(1) / np.float32(npos))
    prod = pooled[:, None, :] * w[None]                     # [B, K, C], each product rounded to fp32
    part = np.zeros((B, K, 64), np.float32)
    for j in range((C + 63) // 64):
        n = min(64, C - 64 * j)
        part[:, :, :n] = part[:, :, :n] + prod[:, :, 64 * j:64 * j + n]
    for o in (32, 16, 8, 4, 2, 1):                          # __shfl_down: lane l takes lane l + o
        part[:, :, :64 - o] = part[:, :, :64 - o] + part[:, :, o:]
    logits = part[:, :, 0] + (bias[None] if bias is not None else np.float32(0))
    return pooled, logits.astype(np.float32)


def run_head(feat, w, bias, softmax, want_pooled, want_probs, bf16):
    import torch
    import ivf_lib as L
    B, npos, C = feat.shape
    K = w.shape[0]
    f = torch.from_numpy(feat)
    featd = (f.bfloat16() if bf16 else f).cuda().contiguous()
    wd = torch.from_numpy(w).cuda()
    biasd = torch.from_numpy(bias).cuda() if bias is not None else None
    pooled = torch.full((B, C), -3.0, device='cuda') if want_pooled else None
    logits = torch.full((B, K), -3.0, device='cuda')
    probs = torch.full((B, K), -3.0, device='cuda') if want_probs else None
    fn = L.lib().ivf_head_fwd_bf16 if bf16 else L.lib().ivf_head_fwd
    L.check(fn(L.ptr(featd), L.ptr(wd), L.ptr(biasd), L.ptr(pooled), L.ptr(logits), L.ptr(probs), B, npos, C, K,
               softmax, L.stream()))
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in (pooled, logits, probs)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_head_fwd_bit_exact(bf16, golden):
    feat, w, bias = head_case(bf16)
    pooled_ref, logits_ref = head_ref(feat, w, bias)
    fixture = golden('head_exact')['probs_bf16' if bf16 else 'probs_fp32']
    for softmax, want_pooled, want_probs in [(1, True, True), (1, False, True), (0, True, True), (0, False, False),
                                             (1, True, False)]:
        pooled, logits, probs = run_head(feat, w, bias, softmax, want_pooled, want_probs, bf16)
        what = f"softmax={softmax} pooled={want_pooled} probs={want_probs}"
        assert np.array_equal(bits(logits), bits(logits_ref)), what
        if want_pooled:
            assert np.array_equal(bits(pooled), bits(pooled_ref)), what
        if want_probs and not softmax:
            assert np.array_equal(bits(probs), bits(logits_ref)), what
        if want_probs and softmax:
            assert np.array_equal(bits(probs), bits(fixture)), what
    # no bias: + 0.0f
    _, logits_nb = head_ref(feat, w, None)
    _, logits, _ = run_head(feat, w, None, 1, False, True, bf16)
    assert np.array_equal(bits(logits), bits(logits_nb))


@pytest.mark.parametrize("per_clip", [1, 0], ids=["per_clip_mask", "shared_mask"])
@pytest.mark.parametrize("T", [16, 32, 9])
def test_freeze_fwd_channels_last_bit_exact(T, per_clip):
    """T = 16 and 32: the kernels with every frame requested up front; 9: the run-time loop."""
    import torch
    import ivf_lib as L
    B, C, HW = 2, 3, 5 * 7
    rng = np.random.default_rng(100 * T + per_clip)
    x = rng.standard_normal((B, C, T, HW)).astype(np.float32)
    m = rng.random((B, T) if per_clip else (T,)).astype(np.float32)
    m.reshape(-1, T)[:, 3] = 0.0      # a frame taken as it is
    m.reshape(-1, T)[:, 5] = 1.0      # a frame frozen entirely
    mb = m if per_clip else np.broadcast_to(m, (B, T))
    one = np.float32(1)
    P = np.empty_like(x)
    P[:, :, 0] = x[:, :, 0]
    for u in range(1, T):
        mu = mb[:, u][:, None, None]
        P[:, :, u] = (one - mu) * x[:, :, u] + mu * P[:, :, u - 1]
    want = np.zeros((B, T, HW, 4), np.float32)
    want[..., :C] = P.transpose(0, 2, 3, 1)
    xd, md = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
    out = torch.full((B + 1, T, HW, 4), -7.0, device='cuda')     # one clip of sentinel behind the output
    L.check(L.lib().ivf_freeze_fwd(L.ptr(xd), L.ptr(md), L.ptr(out), B, C, T, HW, per_clip, 4, L.stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(bits(got[:B]), bits(want))
    assert (got[B] == -7.0).all()
