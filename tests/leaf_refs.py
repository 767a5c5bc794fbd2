"""Case tables, seeded inputs, fp64 references and error bounds for the leaf-kernel tests
(test_gpu_leaf_kernels.py on the GPU, test_leaf_refs_host.py on the CPU).  Both iterate the tables below, so the
host test proves the references and bounds on exactly the inputs the kernels are later compared on.

Every reference is torch / numpy float64 on the CPU, computed from the same fp32 (or bf16-valued) numbers the kernel
reads.  Nothing here needs a GPU or the HIP library.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of fp32


def sum_bound(terms_abs_sum, n):
    """Bound on |fp32 sum - exact sum| for `n` terms summed in ANY order: 2 * (n-1) * 2^-24 * sum|term_i|.

    The textbook first-order bound is (n-1) * 2^-24 * sum|term| (each of the n-1 additions rounds once, and a term
    passes through at most n-1 of them).  The factor 2 covers the terms' own rounding when they are products and the
    final scale of a mean.  Callers count: a plain sum of n stored numbers -> n; a dot product of n products -> n + 1
    (so that a single product, n = 1, still gets its one rounding).  `terms_abs_sum` may be a float, array or tensor.
    """
    return 2.0 * max(int(n) - 1, 0) * U * terms_abs_sum


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def bf16_values(t):
    """fp32 tensor holding bf16-representable values (what a bf16 entry point and its fp32 twin both read)."""
    return t.bfloat16().float()


# ------------------------------------------------------------------------------------------------ head
HEAD_CASES = [          # (B, npos, C, K); all satisfy (C + K + 8) * 4 <= 64 KiB
    (3, 98, 1024, 174),     # the I3D head
    (2, 1, 300, 6),         # the ConvLSTM use: one position
    (5, 7, 1000, 3),        # C >= 256 and not a multiple of 128 or 64: last backward slice is channels 896..999
    (1, 13, 255, 1),        # just under the slicing threshold, one class
    (2, 4, 256, 1500),      # more classes than waves
]
HEAD_SPREAD_CASE = (3, 98, 1024, 174)   # logits spread over +-80


def head_inputs(case, gated=True, bf16=False, spread=False):
    """feat [B,npos,C], w [K,C], bias [K].  gated: feat = relu(randn - 0.3) with extra exact zeros (zeros and
    positives, mean ~0.25); else randn + 0.5 + 0.01 * pos (negatives present).  w carries a mean too."""
    B, npos, C, K = case
    g = _gen('head', case, gated)
    feat = torch.randn(B, npos, C, generator=g)
    if gated:
        feat = torch.relu(feat - 0.3)
        feat.view(-1)[::7] = 0.0
    else:
        feat = feat + 0.5 + 0.01 * torch.arange(npos, dtype=torch.float32).view(1, -1, 1)
    w = torch.randn(K, C, generator=g) * 0.05 + 0.02
    bias = torch.randn(K, generator=g) * 0.1
    if bf16:
        feat = bf16_values(feat)
    if spread:
        lg = feat.double().mean(1) @ w.double().T
        w = (w.double() * (80.0 / float(lg.abs().max()))).float()
    return feat.contiguous(), w.contiguous(), bias.contiguous()


def head_fwd_ref(feat, w, bias, softmax):
    """fp64 pooled / logits / probs and the per-element bounds of pooled and logits.  pooled: sum of npos numbers,
    then one scale.  logits: dot of C products plus the bias (C + 1 terms -> n = C + 2), with pooled's own bound
    propagated through |w|."""
    B, npos, C = feat.shape
    f, wd = feat.double(), w.double()
    pooled = f.mean(1)
    b_pool = sum_bound(f.abs().sum(1) / npos, npos)
    logits = pooled @ wd.T
    s_abs = pooled.abs() @ wd.abs().T
    if bias is not None:
        logits = logits + bias.double()
        s_abs = s_abs + bias.double().abs()
    b_logit = sum_bound(s_abs, C + 2) + b_pool @ wd.abs().T
    probs = torch.softmax(logits, dim=1) if softmax else logits
    return dict(pooled=pooled, b_pooled=b_pool, logits=logits, b_logits=b_logit, probs=probs)


def head_probs_input(case, softmax, gated=True, bf16=False):
    """The fp32 `probs` array handed to the backward kernels: the fp64 forward rounded once."""
    feat, w, bias = head_inputs(case, gated, bf16)
    return head_fwd_ref(feat, w, None, softmax)['probs'].float().contiguous()


def head_targets(case):
    B, _, _, K = case
    return torch.randint(0, K, (B,), generator=_gen('head/t', case), dtype=torch.int32)


def head_dout(case):
    B, _, _, K = case
    return (torch.randn(B, K, generator=_gen('head/dout', case)) + 0.5).contiguous()


def head_bwd_ref(feat, w, probs, target, dout, softmax, gate_relu):
    """fp64 restatement of the head backward from the numbers the kernel reads (feat, w, the fp32 probs, target or
    dout).  test_leaf_refs_host.py shows it equals fp64 autograd of feat.mean(1) @ w.T (+ softmax).

    dpooled[c] = sum_k dl[k] w[k,c] is the gradient w.r.t. the pooled vector (NOT divided by npos); dfeat = dpooled /
    npos, zero where gate_relu and feat <= 0.  Bounds: dl[k] = p_k (d_k - dot) carries the bound of dot = sum_j p_j d_j
    (K products) plus two roundings of its own; dpooled is a dot of K products; dfeat adds the rounding of 1/npos and
    of the product."""
    B, npos, C = feat.shape
    K = w.shape[0]
    wd, p = w.double(), probs.double()
    if dout is not None:
        d = dout.double()
    else:
        d = torch.zeros(B, K, dtype=torch.float64)
        d[torch.arange(B), target.long()] = 1.0
    if softmax:
        dot = (p * d).sum(1, keepdim=True)
        b_dot = sum_bound((p * d).abs().sum(1, keepdim=True), K + 1) if dout is not None else 0.0 * dot
        dl = p * (d - dot)
        e_dl = p.abs() * b_dot + 2 * U * p.abs() * (d.abs() + dot.abs())
    else:
        dl = d
        e_dl = torch.zeros_like(d)
    dpooled = dl @ wd
    b_dp = sum_bound(dl.abs() @ wd.abs(), K + 1) + e_dl @ wd.abs()
    dfeat = (dpooled / npos)[:, None, :].expand(B, npos, C).clone()
    b_df = (b_dp / npos + 2 * U * dpooled.abs() / npos)[:, None, :].expand(B, npos, C).clone()
    off = torch.zeros(B, npos, C, dtype=torch.bool)
    if gate_relu:
        off = ~(feat > 0)
        dfeat[off] = 0.0
        b_df[off] = 0.0
    score = probs[torch.arange(B), target.long()] if target is not None else None
    return dict(dpooled=dpooled, b_dpooled=b_dp, dfeat=dfeat, b_dfeat=b_df, off=off, score=score)


# ------------------------------------------------------------------------------------------------ argmax
ARGMAX_CASES = [(b, K) for b in (1, 64, 65, 130) for K in (1, 6, 174)]


def argmax_input(case):
    """rows: random; every third row quantised to 4 levels (ties: the first maximum wins); row 0 has its maximum at
    index 0 and the last row at K - 1.  A single row (b == 1) stays quantised and gets the top level at K - 1: the
    maximum sits at the end, tied with any earlier entry at that level."""
    b, K = case
    x = torch.rand(b, K, generator=_gen('argmax', case))
    x[::3] = (x[::3] * 3).round() / 3
    if b > 1:
        x[0, 0] = 2.0
        x[b - 1, K - 1] = 2.0
    else:
        x[0, K - 1] = 1.0
    return x.contiguous()


# ------------------------------------------------------------------------------------------------ Grad-CAM
GRADCAM_CASES = [(2, 98, 1024), (3, 5, 100), (1, 1, 1), (2, 784, 480), (4, 33, 63)]   # (B, npos, C)


def gradcam_inputs(case, bf16=False):
    """feat = randn + 0.5 + 0.01 * pos; grad = randn * 0.5 + 0.25 with the sign of the mean flipped on odd clips, so
    that clip's cam is mostly negative (exact 0.0 after the ReLU)."""
    B, npos, C = case
    g = _gen('gradcam', case)
    feat = torch.randn(B, npos, C, generator=g) + 0.5 + 0.01 * torch.arange(npos, dtype=torch.float32).view(1, -1, 1)
    sign = torch.tensor([1.0 if b % 2 == 0 else -1.0 for b in range(B)]).view(-1, 1, 1)
    grad = torch.randn(B, npos, C, generator=g) * 0.5 + 0.25 * sign
    if bf16:
        feat, grad = bf16_values(feat), bf16_values(grad)
    return feat.contiguous(), grad.contiguous()


def gradcam_ref(feat, grad):
    """w = grad.mean(1); cam = relu(feat @ w).  cam's bound: dot of C products (n = C + 1) plus the bound of the
    weights propagated through |feat|.  `pre` is the value before the ReLU (the ReLU is 1-Lipschitz, so the bound
    holds after it; pre < -bound means the kernel must give exactly 0)."""
    B, npos, C = feat.shape
    f, g = feat.double(), grad.double()
    wts = g.mean(1)
    b_w = sum_bound(g.abs().sum(1) / npos, npos)
    pre = torch.einsum('bpc,bc->bp', f, wts)
    b_cam = sum_bound(torch.einsum('bpc,bc->bp', f.abs(), wts.abs()), C + 1) + torch.einsum('bpc,bc->bp', f.abs(), b_w)
    return dict(weights=wts, b_weights=b_w, pre=pre, cam=torch.relu(pre), b_cam=b_cam)


# ------------------------------------------------------------------------------------------------ resize / normalise
RESIZE_CASES = [        # (B, nslice, sh, sw, H, W, step)
    (2, 2, 7, 7, 224, 224, 8),
    (1, 4, 4, 5, 120, 160, 8),
    (2, 3, 5, 3, 17, 23, 1),
    (1, 2, 14, 14, 9, 11, 2),      # downscale
    (1, 2, 6, 9, 6, 9, 3),         # identity size
    (1, 1, 1, 1, 8, 8, 4),         # one cell: constant map
]


def resize_input(case):
    """cam [B,nslice,sh,sw] >= 0 with a ramp.  When there is more than one slice, slice (0, 1) is all zero (a slice
    the ReLU emptied): constant, so NaN under per_frame = 1 and finite under per_frame = 0."""
    B, ns, sh, sw = case[:4]
    cam = torch.rand(B, ns, sh, sw, generator=_gen('resize', case)) + 0.25
    cam = cam + 0.01 * torch.arange(sh * sw, dtype=torch.float32).view(1, 1, sh, sw)
    if ns > 1:
        cam[0, 1] = 0.0
    return cam.contiguous()


def resize_ref64(cam, H, W):
    """[B,nslice,sh,sw] -> [B,nslice,H,W] float64: half-pixel centres, clamped index (OpenCV INTER_LINEAR's rule)."""
    return F.interpolate(cam.double(), size=(H, W), mode='bilinear', align_corners=False, antialias=False)


def resize_oracle32(cam, H, W):
    """The same map by oracle.gradcam_ref.resize_bilinear: the kernel's fp32 formula on the CPU."""
    from oracle import gradcam_ref
    B, ns = cam.shape[:2]
    out = np.empty((B, ns, H, W), dtype=np.float32)
    for b in range(B):
        for s in range(ns):
            out[b, s] = gradcam_ref.resize_bilinear(cam[b, s].numpy(), W, H)
    return torch.from_numpy(out)


def resize_gate(cam, H, W):
    """(gate, oracle figure) in units of the resized map: 4x the distance of the fp32 formula from the fp64 reference
    on this input (the margin covers FMA contraction and another association of the four products), floored at
    2^-22 * max|cam|."""
    fig = float((resize_oracle32(cam, H, W).double() - resize_ref64(cam, H, W)).abs().max())
    return max(4.0 * fig, 2.0 ** -22 * float(cam.abs().max())), fig


def normalise_ref(rs, step, per_frame):
    """x - min, then / max, per slice block (per_frame) or per clip, as gradcam_ref.cam_from_activations; every slice
    repeated `step` times: [B, nslice * step, H, W].  0/0 is NaN as in numpy.  Also returns the denominator used for
    every slice [B,nslice]."""
    B, ns, H, W = rs.shape
    if per_frame:
        mn = rs.amin(dim=(2, 3), keepdim=True)
        mx = rs.amax(dim=(2, 3), keepdim=True)
    else:
        mn = rs.amin(dim=(1, 2, 3), keepdim=True).expand(B, ns, 1, 1)
        mx = rs.amax(dim=(1, 2, 3), keepdim=True).expand(B, ns, 1, 1)
    out = (rs - mn) / (mx - mn)
    return out.repeat_interleave(step, dim=1), (mx - mn).reshape(B, ns)


def normalise_tol(out_ref, den, gate, step):
    """|out - ref| allowed when the resized map, its min and its max are each within `gate`: out = (x - mn) / den, so
    d(out) <= (dx + dmn) / den + |out| d(den) / den with d(den) <= 2 gate; plus 2^-22 for the two fp32 roundings."""
    d = den.repeat_interleave(step, dim=1)[:, :, None, None]
    return gate * (2.0 + 2.0 * out_ref.abs()) / d + 2.0 ** -22


# ------------------------------------------------------------------------------------------------ reverse
THRESH = float(np.float32(0.1))     # the kernels compare in fp32: mask > 0.1f
REV_PAIR_CASES = [(B, T) for T in (9, 16, 32, 40, 64) for B in (1, 7, 65, 130)]
REV_SHAPES = [          # (B, C, T, HW): B in 1,7,65,130; C in 1,3,4; T in 9,16,32,40,64; HW in 15,240,12544
    (1, 3, 16, 12544), (7, 3, 9, 240), (65, 1, 16, 15), (130, 4, 40, 15), (7, 4, 32, 240), (2, 1, 64, 240),
    (3, 3, 64, 15),
]
REV_GOLDEN = ['even_mid', 'odd_mid', 'ends', 'thresh', 'all_on', 'all_off', 'single']


def rev_masks(B, T, golden_rows=None):
    """[B,T] fp32 mask rows, cycling through: all-off, a run touching frame 0, a run touching T - 1, an odd-length
    run (its middle frame has no partner), all-on, rows quantised around the 0.1 threshold, plain random rows, and
    (T == 16) the seven rev_*_mask rows of tests/golden/mask_ops.npz."""
    g = _gen('revmask', B, T)
    levels = torch.tensor([0.0, 0.05, 0.1, float(np.nextafter(np.float32(0.1), np.float32(1))), 0.35, 0.8])
    rows = []
    extra = list(golden_rows) if (golden_rows is not None and T == 16) else []
    for b in range(B):
        kind = b % (7 + len(extra))
        val = torch.rand(T, generator=g) * 0.85 + 0.15
        m = torch.zeros(T)
        if kind == 0 and B > 1:
            pass
        elif kind == 1:
            m[:4] = val[:4]
        elif kind == 2:
            m[T - 5:] = val[T - 5:]
        elif kind == 3 or (kind == 0 and B == 1):
            m[2:7] = val[2:7]
            m[T - 2:] = val[T - 2:]
        elif kind == 4:
            m = val
        elif kind == 5:
            m = levels[torch.randint(0, len(levels), (T,), generator=g)]
        elif kind == 6:
            m = torch.rand(T, generator=g)
        else:
            m = torch.from_numpy(np.asarray(extra[kind - 7], dtype=np.float32))
        rows.append(m.float())
    return torch.stack(rows).contiguous()


def pairs_ref(mask_row):
    """partner / weight of one mask row, mask.py:40-85 restated: runs of mask > 0.1f; within a run frame a = run[u]
    and b = run[-(u+1)] are partners, both weighted with mask[a]; everything else is its own partner, weight 0."""
    m = np.asarray(mask_row, dtype=np.float32)
    T = m.size
    partner = np.arange(T, dtype=np.int32)
    weight = np.zeros(T, dtype=np.float32)
    start = -1
    for j in range(T + 1):
        on = j < T and m[j] > np.float32(0.1)
        if on and start < 0:
            start = j
        if not on and start >= 0:
            ln = j - start
            for u in range(ln // 2):
                a, b = start + u, start + ln - 1 - u
                partner[a], partner[b] = b, a
                weight[a] = weight[b] = m[a]
            start = -1
    return partner, weight


def rev_inputs(shape):
    """x [B,C,T,HW] in 0..255 and the upstream gradient g in about -1..1, anti-correlated with x: the terms
    (X[b'] - X[a]) (G[a] - G[b']) of dmask then share a sign, so their sum is of the size of sum|term| and a gradient
    read at the wrong place (which decorrelates them) moves it by far more than the bound."""
    B, C, T, HW = shape
    gen = _gen('rev', shape)
    x = torch.rand(B, C, T, HW, generator=gen) * 255
    g = (0.5 - x / 255) * 1.4 + (torch.rand(B, C, T, HW, generator=gen) - 0.5) * 0.6
    return x.contiguous(), g.contiguous()


def reverse_ref(x, masks):
    """oracle.mask_ref.reverse per clip on float64 (the threshold stays the fp32 one)."""
    from oracle import mask_ref
    B, C, T, HW = x.shape
    out = torch.empty(B, C, T, HW, dtype=torch.float64)
    for b in range(B):
        out[b] = mask_ref.reverse(x[b:b + 1].double().view(1, C, T, HW, 1), masks[b].double(), THRESH)[0, ..., 0]
    return out


def reverse_bwd_ref(x, g, masks):
    """fp64 autograd of mask_ref.reverse with loss (p * g).sum(): dmask [B,T]."""
    from oracle import mask_ref
    B, C, T, HW = x.shape
    dm = torch.zeros(B, T, dtype=torch.float64)
    for b in range(B):
        m = masks[b].double().requires_grad_()
        p = mask_ref.reverse(x[b:b + 1].double().view(1, C, T, HW, 1), m, THRESH)
        if p.requires_grad:
            (p[0, ..., 0] * g[b].double()).sum().backward()
            dm[b] = m.grad
    return dm


def reverse_bwd_terms(x, g, masks):
    """Pair formula of the kernel in fp64: for a pair (a, b'), a < b', dmask[a] = sum (X[b'] - X[a]) (G[a] - G[b']).
    Returns (dmask [B,T], sum of |term| [B,T], first-half flags [B,T])."""
    B, C, T, HW = x.shape
    xd, gd = x.double(), g.double()
    dm = torch.zeros(B, T, dtype=torch.float64)
    sa = torch.zeros(B, T, dtype=torch.float64)
    first = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        partner, _ = pairs_ref(masks[b].numpy())
        for t in range(T):
            pt = int(partner[t])
            if pt > t:
                term = (xd[b, :, pt] - xd[b, :, t]) * (gd[b, :, t] - gd[b, :, pt])
                dm[b, t] = term.sum()
                sa[b, t] = term.abs().sum()
                first[b, t] = True
    return dm, sa, first


# ------------------------------------------------------------------------------------------------ regulariser / Adam
REG_CASES = [(B, T) for B in (1, 5, 65, 130) for T in (9, 16, 32, 64)]
LAM1, LAM2 = 0.01, 0.02
ADAM = dict(lr=0.2, b1=0.9, b2=0.999, eps=1e-8)
STEP_CASES = [(1, 16), (5, 9), (65, 32), (130, 32)]
STEP_N = 12
SIGMOID_N = [1, 255, 257, 4160]


def reg_const_row(B):
    """index of the constant row (val == 0: NaN gradients for that row only), or -1 when B == 1"""
    return 3 if B >= 5 else -1


def reg_inputs(case):
    """masks in (0,1) for ivf_tv_norm and raw masks in (-5,5) for ivf_mask_reg, one constant row each."""
    B, T = case
    g = _gen('reg', case)
    mask = torch.rand(B, T, generator=g)
    raw = torch.rand(B, T, generator=g) * 10 - 5
    r = reg_const_row(B)
    if r >= 0:
        mask[r] = 0.375
        raw[r] = -1.25
    return mask.contiguous(), raw.contiguous()


def tv_ref(mask_row, p=3, q=3):
    """mask_ref.calc_tv_norm under fp64 autograd: (val, grad[T])."""
    from oracle import mask_ref
    m = mask_row.double().requires_grad_()
    v = mask_ref.calc_tv_norm(m, p, q)
    v.backward()
    return float(v.detach()), m.grad.clone()


def reg_ref(raw_row, lam1=LAM1, lam2=LAM2):
    """sig, (l1, tv), d(l1 + tv)/dsig of one raw row in fp64 (FindMasksComparison_I3D_smth.py:198-200)."""
    from oracle import mask_ref
    sig = torch.sigmoid(raw_row.double()).requires_grad_()
    l1 = lam1 * sig.abs().sum()
    tv = lam2 * mask_ref.calc_tv_norm(sig, 3, 3)
    (l1 + tv).backward()
    return sig.detach(), float(l1.detach()), float(tv.detach()), sig.grad.clone()


def adam_ref(p0, grads, lr=0.2, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's single-tensor update in float64: yields (param, exp_avg, exp_avg_sq) after every step."""
    p = p0.double().clone()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    for i, g in enumerate(grads):
        g = g.double()
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        step = i + 1
        denom = v.sqrt() / np.sqrt(1 - b2 ** step) + eps
        p = p - (lr / (1 - b1 ** step)) * m / denom
        yield p.clone(), m.clone(), v.clone()


def step_inputs(case):
    """raw [B,T], and per step: sig in (0.02, 0.98), dscore and dreg of the size the search loop sees, terms [B,2],
    score [B]."""
    B, T = case
    g = _gen('step', case)
    raw = torch.rand(B, T, generator=g) * 10 - 5
    sig = torch.rand(STEP_N, B, T, generator=g) * 0.96 + 0.02
    dscore = torch.rand(STEP_N, B, T, generator=g) * 0.2 - 0.1
    dreg = torch.rand(STEP_N, B, T, generator=g) * 0.04 - 0.01
    terms = torch.rand(STEP_N, B, 2, generator=g) * 0.1
    score = torch.rand(STEP_N, B, generator=g)
    return raw, sig, dscore, dreg, terms, score


def step_grads64(sig, dscore, dreg):
    s = sig.double()
    return (dreg.double() + dscore.double()) * s * (1 - s)


def sigmoid_input(n):
    x = torch.rand(n, generator=_gen('sigmoid', n)) * 40 - 20
    special = torch.tensor([0.0, 88.0, -88.0, 104.0, -104.0])
    k = min(n, special.numel())
    x[:k] = special[:k]
    if n > 5:
        x[-5:] = special
    return x.contiguous()


# ------------------------------------------------------------------------------------------------ weight packs
PACK_ROWS_CASES = [     # (row counts of the units, Cin, CinPad, k)
    ((64, 96, 16), 192, 192, 1),
    ((60, 24, 16), 40, 40, 1),
    ((16, 8), 8, 8, 3),
]
FUSED_COUTS = (60, 24, 16)      # Ktotal = 100: off the 8 grid
FUSED_CINS = [(40, 40), (38, 40)]   # (Cin, CinPad)


def pack_weights(couts, cin, k, tag):
    g = _gen('pack', couts, cin, k, tag)
    return [(torch.randn(co, cin, k, k, k, generator=g) * 0.1 + 0.01).contiguous() for co in couts]


def fused_inputs(cin, bf16=False):
    """per unit: weight [Cout,Cin], scale [Cout], dY [M,Cout] (M positions); dY carries a mean."""
    g = _gen('fused', cin)
    M = 2 * 3 * 4 * 5
    ws = [(torch.randn(co, cin, generator=g) * 0.1 + 0.01).contiguous() for co in FUSED_COUTS]
    sc = [(torch.rand(co, generator=g) + 0.5).contiguous() for co in FUSED_COUTS]
    dy = [(torch.randn(M, co, generator=g) + 0.25).contiguous() for co in FUSED_COUTS]
    if bf16:
        dy = [bf16_values(d) for d in dy]
    return ws, sc, dy


def fused_ref(ws, sc, dy):
    """sum_u (dY_u * scale_u) @ W_u in fp64: [M, Cin]"""
    return sum((d.double() * s.double()) @ w.double() for w, s, d in zip(ws, sc, dy))
