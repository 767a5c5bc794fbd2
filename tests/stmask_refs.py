"""Case tables, seeded inputs, fp64 references and error bounds for the spatio-temporal mask kernels of
csrc/stmask_ops.hip (test_gpu_stmask.py on the GPU, test_stmask_refs_host.py on the CPU).  Both files iterate the tables
below.  Nothing here needs a GPU; `lib_axis_weights` needs the HIP library for a host function only.

The feature is an extension without a counterpart in the reference: these references are torch fp64
restatements of the semantics of DESIGN section 11, pinned by torch autograd, not reference output.

Rounding model: that of mask_refs (U = 2^-24, gamma(k) = k U / (1 - k U), FMA contraction only removes roundings).

Axis weights.  A = G U [n_out, n_in] (`axis_weights_ref`): U = F.interpolate(mode='bilinear', align_corners=False) of the
identity, G = conv1d with a replicate-padded, normalised Gaussian of radius ceil(3 sigma).  Both sides are fp64 sums of
at most 2 (2 r + 1) non-negative products; they differ by a few fp64 roundings, far below the single final rounding to
fp32.  The host test's gate is 2 fp32 ulp per entry.

Expand, M = A_H S A_W^T with every factor >= 0.  tmp[i][x] = sum_j S[i,j] A_W[x,j] is gw products and gw - 1 additions:
a term passes through at most gw roundings.  M[y,x] = sum_i A_H[y,i] tmp[i][x] adds one product and at most gh - 1
additions.  All terms share a sign, so the error is relative:
    b_M = gamma(gh + gw + 2) M_ref                  (`expand_bound`; the + 2 is slack, the count is gh + gw).

Expand backward, dS[i,j] = sum_{y,x} term, term = A_H[y,i] dM[y,x] A_W[x,j].  The kernel sums y first (tmp, H products
and H - 1 additions), then x (W products, W - 1 additions, any order): a term passes through at most H + W roundings,
which the any-order bound of a flat H W-term sum covers whenever H W >= H + W (every case; H = W = 1 has one term and
two roundings, and the bound's floor of 2 terms is applied there):
    b_dS = sum_bound(sum |term|, max(H W, 2) + 1)   (`expand_bwd_ref`; + 1 as leaf_refs counts dot products).

Per-pixel scan: mask_refs' derivation holds per pixel unchanged (it only uses m in [0,1]):
    b_P[u] = gamma(4 u) max_{v<=u} |X[v]|,   b_G[u] = gamma(2 (T-1-u)) sum_{v>=u} |g[v]|.

dM[b,u,px] = sum_c term_c, term_c = (P[u-1] - X[u]) G[u]: each term is rounded twice (difference, product) and passes
through at most C - 1 additions, C + 1 roundings, within sum_bound(sum|term|, C + 2) = 2 (C + 1) U sum|term|; plus
the forward and scan bounds carried through exactly as mask_refs.freeze_bwd_ref does:
    b_dM = sum_bound(sum_c |term|, C + 2) + sum_c (b_P[u-1] |G[u]| + b_G[u] |P[u-1] - X[u]| + b_P[u-1] b_G[u]).
dM[:, 0] is exactly 0.0.

Regulariser.  s = 1 / (1 + expf(-r)): expf within 1 ulp = 2 U relative (the documented accuracy of the device library;
4 U is allowed here), the addition and the division one rounding each, so |s_fp32 - s| <= E_S s with E_S = 8 U (the
error of e = exp(-r) enters s through e / (1 + e) <= 1).  A difference d = a - s then carries e_d = E_S (a + s) + U |d|,
and |d|^3 (two products) e_c = 3 d^2 e_d + 3 |d| e_d^2 + e_d^3 + gamma(2) |d|^3.  A value term lam * sum / cells: the
any-order sum of n terms, two more roundings for the scale:
    b_val = |lam| / cells * (sum_bound(sum t, n) + sum e_t) + gamma(2) |val|        (`reg_ref`).
The gradient's per-pair piece 3 d |d| (x |x| has the Lipschitz bound 2 |d| e_d + e_d^2, which also covers a sign that
flips at |d| <= e_d) is rounded four times (difference, square, 3 *, weight), an element gathers at most 2 pieces in
time and 4 in space, and (lam * g) / cells with the final three-term sum adds 4:
    b_dreg = sum_k |lam_k| / cells * (sum_pieces w 3 (2 |d| e_d + e_d^2) + gamma(10) sum_pieces |piece|) + gamma(4) lam1/cells.
"""
import ctypes
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import mask_refs
from leaf_refs import U, sum_bound
from mask_refs import gamma

MAX_GRID = 32


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7fffffff)


# ------------------------------------------------------------------------------------------------ axis weights
# (n_out, n_in, sigma): the axes of the expand cases below, plus an odd ratio with a wide blur and a downsampling pair
AXIS_CASES = [(224, 7, 16.0), (120, 4, 0.0), (160, 5, 0.0), (17, 1, 2.0), (23, 1, 2.0), (33, 14, 1.5), (47, 14, 1.5),
              (32, 32, 0.0), (224, 32, 3.0), (24, 3, 1.0), (32, 4, 1.0), (50, 9, 7.3), (5, 12, 0.7)]


def axis_weights_ref(n_out, n_in, sigma, align_corners=False, pad='replicate'):
    """A [n_out, n_in] float64 by torch: bilinear interpolation of the identity along one axis, then the blur.
    align_corners=True and pad='constant' (zeros) are the mutants of the host test."""
    sigma = float(np.float32(sigma))          # the C interface carries sigma as a float
    eye = torch.eye(n_in, dtype=torch.float64).view(1, n_in, n_in, 1)                 # channel j = unit vector e_j
    Ut = F.interpolate(eye, size=(n_out, 1), mode='bilinear', align_corners=align_corners)[0, :, :, 0]   # [n_in, n_out]
    rad = int(math.ceil(3.0 * sigma)) if sigma > 0 else 0
    if rad == 0:
        return Ut.t().contiguous()
    d = torch.arange(-rad, rad + 1, dtype=torch.float64)
    tap = torch.exp(-0.5 * d * d / (float(sigma) ** 2))
    tap = tap / tap.sum()
    if pad == 'replicate':          # F.pad's replicate mode limits the pad to the length; index instead
        idx = torch.clamp(torch.arange(-rad, n_out + rad), 0, n_out - 1)
        padded = Ut[:, idx]
    else:
        padded = F.pad(Ut, (rad, rad))
    At = F.conv1d(padded.view(n_in, 1, -1), tap.view(1, 1, -1))[:, 0]                   # symmetric taps
    return At.t().contiguous()


def lib_axis_weights(n_out, n_in, sigma):
    """ivf_stmask_axis_weights (host function of libivf_hip): [n_out, n_in] float32"""
    import ivf_lib as L
    buf = np.full((n_out, n_in), np.nan, dtype=np.float32)
    L.check(L.lib().ivf_stmask_axis_weights(n_out, n_in, float(sigma), buf.ctypes.data_as(ctypes.c_void_p)))
    return torch.from_numpy(buf)


@functools.lru_cache(maxsize=None)
def axis_weights(n_out, n_in, sigma):
    """the fp32 matrix the kernels are given: the reference rounded once (the host test holds the library's to it)"""
    return axis_weights_ref(n_out, n_in, sigma).float().contiguous()


def ulp32(v):
    """spacing of float32 at |v| (float64 tensor in, float64 out), at least the smallest normal's"""
    a = v.abs().float()
    return (torch.nextafter(a, torch.tensor(float('inf'))) - a).double().clamp_min(2.0 ** -149)


# ------------------------------------------------------------------------------------------------ expand
# (B, T, gh, gw, H, W, sigma)
EXPAND_CASES = {
    'E1': (2, 3, 7, 7, 224, 224, 16.0),     # the S16 geometry at 3 frames
    'E2': (1, 2, 4, 5, 120, 160, 0.0),      # KTH grid, no blur
    'E3': (3, 1, 1, 1, 17, 23, 2.0),        # a 1x1 grid
    'E4': (2, 2, 14, 14, 33, 47, 1.5),      # ragged rows, not a wave multiple
    'E5': (1, 2, 32, 32, 32, 32, 0.0),      # the identity: M == S bit for bit
    'E6': (1, 1, 32, 32, 224, 224, 3.0),    # the size limit
}


def expand64(S, AH, AW):
    return AH.double() @ S.double() @ AW.double().t()


def expand_bound(Mref, gh, gw):
    return gamma(gh + gw + 2) * Mref.abs()


def expand_bwd64(dM, AH, AW):
    return AH.double().t() @ dM.double() @ AW.double()


@functools.lru_cache(maxsize=None)
def expand_case(name):
    """inputs and references of one case (read-only): S = sigmoid of raw values in +-5 with saturated and exact 0.5
    entries; dM of mixed sign with a smooth positive part, so that a wrong row or column moves the sums"""
    B, T, gh, gw, H, W, sigma = EXPAND_CASES[name]
    g = _gen('expand', name)
    raw = (torch.rand(B, T, gh, gw, generator=g) * 10 - 5)
    raw.view(-1)[::7] = 5.0
    raw.view(-1)[3::11] = 0.0
    S = torch.sigmoid(raw).float().contiguous()
    AH, AW = axis_weights(H, gh, sigma), axis_weights(W, gw, sigma)
    yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
    dM = (0.5 + yy + 2 * xx * xx + (torch.rand(B, T, H, W, generator=g) - 0.5) * 2.0).float().contiguous()
    Mref = expand64(S, AH, AW)
    dS = expand_bwd64(dM, AH, AW)
    sabs = expand_bwd64(dM.abs(), AH, AW)           # A >= 0
    return dict(S=S, AH=AH, AW=AW, dM=dM, M=Mref, bM=expand_bound(Mref, gh, gw), dS=dS,
                bdS=sum_bound(sabs, max(H * W, 2) + 1))


# ------------------------------------------------------------------------------------------------ per-pixel freeze
# (B, C, T, HW)
STFREEZE_CASES = {
    'P1': (2, 3, 16, 12545),    # ordinary case
    'P2': (1, 3, 17, 240),      # ragged inside the 32-frame template
    'P3': (3, 4, 32, 240),      # the .w lane
    'P4': (2, 1, 40, 15),       # T > 32, the generic loop
    'P5': (3, 2, 1, 33),        # T = 1: p == x
    'P6': (5, 5, 16, 63),       # C > 4: layout 4 refused, layout 8 runs
}


def out_layouts(C):
    return (0, 4, 8) if C <= 4 else (0, 8)


def pixel_masks(B, T, HW):
    """M [B,T,HW] fp32: pixel px of clip b follows row (3 b + px) % 10 of mask_refs.freeze_masks(10, T) (random, random
    with exact 0/1 entries, all zero, all one, saturated); in clip 0 frame plane 1 is exact 0.0 and plane 2 exact 1.0."""
    rows = mask_refs.freeze_masks(10, T)                                        # [10,T]
    idx = (3 * torch.arange(B).view(B, 1) + torch.arange(HW).view(1, HW)) % 10  # [B,HW]
    M = rows[idx].permute(0, 2, 1).contiguous()                                 # [B,T,HW]
    if T > 1:
        M[0, 1] = 0.0
    if T > 2:
        M[0, 2] = 1.0
    return M


def stfreeze_inputs(name):
    """x and g built as mask_refs.freeze_inputs builds them (channels and frames far enough apart that a value read from
    the wrong place moves the result)"""
    B, C, T, HW = STFREEZE_CASES[name]
    gen = _gen('stfreeze', name)
    amp = 180.0 / (1.0 + 0.5 * torch.arange(C, dtype=torch.float32)).view(1, C, 1, 1)
    t = torch.arange(T, dtype=torch.float32).view(1, 1, T, 1) / max(T - 1, 1)
    step = amp / max(T - 1, 1)
    noise = (torch.rand(B, C, T, HW, generator=gen) * 2 - 1) * torch.clamp(step, max=30.0)
    x = 220.0 - amp * t + noise
    g = 0.3 + 0.15 * torch.arange(C, dtype=torch.float32).view(1, C, 1, 1) + (torch.rand(B, C, T, HW, generator=gen) - 0.5) * 0.4
    return x.contiguous(), g.contiguous()


def stfreeze_fwd64(x, M):
    """P [B,C,T,HW] float64; the expression of oracle.mask_ref.freeze with a mask value per pixel"""
    xd, m = x.double(), M.double()
    T = x.shape[2]
    frames = [xd[:, :, 0]]
    for u in range(1, T):
        mu = m[:, u].unsqueeze(1)
        frames.append((1 - mu) * xd[:, :, u] + mu * frames[-1])
    return torch.stack(frames, dim=2)


def stfreeze_scan64(g, M):
    gd, m = g.double(), M.double()
    T = g.shape[2]
    G = [None] * T
    G[T - 1] = gd[:, :, T - 1]
    for u in range(T - 2, -1, -1):
        G[u] = gd[:, :, u] + m[:, u + 1].unsqueeze(1) * G[u + 1]
    return torch.stack(G, dim=2)


def stfreeze_bwd_ref(x, g, M, drop_channel=None):
    """dM [B,T,HW] float64 by the explicit formula and its gate (module docstring); drop_channel: the mutant"""
    B, C, T, HW = x.shape
    P, G = stfreeze_fwd64(x, M), stfreeze_scan64(g, M)
    bP, bG = mask_refs.freeze_fwd_bound(x), mask_refs.freeze_scan_bound(g)
    diff = torch.zeros_like(P)
    diff[:, :, 1:] = P[:, :, :-1] - x.double()[:, :, 1:]
    term = diff * G
    term[:, :, 0] = 0.0
    if drop_channel is not None:
        term[:, drop_channel] = 0.0
    bPprev = torch.zeros_like(P)
    bPprev[:, :, 1:] = bP[:, :, :-1]
    prop = bPprev * G.abs() + bG * diff.abs() + bPprev * bG
    prop[:, :, 0] = 0.0
    b = sum_bound(term.abs().sum(dim=1), C + 2) + prop.sum(dim=1)
    b[:, 0] = 0.0
    return dict(dM=term.sum(dim=1), b_dM=b, P=P, G=G)


@functools.lru_cache(maxsize=None)
def stfreeze_case(name):
    B, C, T, HW = STFREEZE_CASES[name]
    x, g = stfreeze_inputs(name)
    M = pixel_masks(B, T, HW)
    return dict(x=x, g=g, M=M, rows=mask_refs.freeze_masks(B, T), bP=mask_refs.freeze_fwd_bound(x),
                **stfreeze_bwd_ref(x, g, M))


# ------------------------------------------------------------------------------------------------ regulariser
# (B, T, gh, gw)
REG_CASES = {'R1': (3, 16, 1, 1), 'R2': (2, 6, 4, 5), 'R3': (2, 16, 7, 7), 'R4': (1, 2, 3, 3), 'R5': (2, 3, 2, 1)}
REG_LAMS = (0.01, 0.02, 0.03)
E_S = 8 * U


def reg_raw(name):
    """raw [B,T,gh,gw] in +-5; clip 0's cell (0,0) is constant over time (its TVt gradient must be an exact zero of the
    time pieces), one frame of the last clip is spatially constant"""
    B, T, gh, gw = REG_CASES[name]
    raw = torch.rand(B, T, gh, gw, generator=_gen('reg', name)) * 10 - 5
    raw[0, :, 0, 0] = 1.25
    raw[B - 1, T - 1] = -0.5
    return raw.float().contiguous()


def tv_pairs(T, doubled=True):
    """weights w[k] of the frame pairs (k, k+1), k = 0..T-2, in calc_tv_norm's `val` (mask.py:93-96): interior pairs are
    visited twice.  doubled=False (every pair once) is the mutant."""
    w = torch.zeros(max(T - 1, 0), dtype=torch.float64)
    for u in range(1, T - 1):
        w[u - 1] += 1
        w[u] += 1
    return w if doubled else w.clamp(max=1)


def reg_terms64(S, lams, doubled=True):
    """(l1, tvt, tvs) [B] each, differentiable in S [B,T,gh,gw] float64"""
    B, T, gh, gw = S.shape
    cells = gh * gw
    w = tv_pairs(T, doubled).view(1, -1, 1, 1)
    l1 = lams[0] * S.abs().sum(dim=(1, 2, 3)) / cells
    tvt = lams[1] * (w * (S[:, 1:] - S[:, :-1]).abs() ** 3).sum(dim=(1, 2, 3)) / cells
    tvs = lams[2] * (((S[:, :, 1:] - S[:, :, :-1]).abs() ** 3).sum(dim=(1, 2, 3))
                     + ((S[:, :, :, 1:] - S[:, :, :, :-1]).abs() ** 3).sum(dim=(1, 2, 3))) / cells
    return l1, tvt, tvs


def _pair_bounds(a, s):
    """(e_c, e_piece, |piece|) of one pair with members a, s (module docstring)"""
    d = (a - s).abs()
    ed = E_S * (a + s) + U * d
    ec = 3 * d * d * ed + 3 * d * ed * ed + ed ** 3 + gamma(2) * d ** 3
    ep = 3 * (2 * d * ed + ed * ed)
    return ec, ep, 3 * d * d


def reg_ref(raw, lams=REG_LAMS, doubled=True):
    """fp64 value and gradient with the gates of the module docstring: terms [B,3], dreg [B,T,gh,gw], sig, and bounds"""
    B, T, gh, gw = raw.shape
    cells = gh * gw
    S = torch.sigmoid(raw.double()).requires_grad_()
    l1, tvt, tvs = reg_terms64(S, lams, doubled)
    (l1.sum() + tvt.sum() + tvs.sum()).backward()
    s = S.detach()
    w = tv_pairs(T, doubled).view(1, -1, 1, 1)
    lam1, lam2, lam3 = (abs(v) for v in lams)
    # values
    n = T * cells
    b_l1 = lam1 / cells * (sum_bound(s.sum(dim=(1, 2, 3)), n) + E_S * s.sum(dim=(1, 2, 3))) + gamma(2) * l1.detach().abs()
    ect, ept, pt = _pair_bounds(s[:, 1:], s[:, :-1])
    ech, eph, ph = _pair_bounds(s[:, :, 1:], s[:, :, :-1])
    ecw, epw, pw = _pair_bounds(s[:, :, :, 1:], s[:, :, :, :-1])
    t_sum = (w * (s[:, 1:] - s[:, :-1]).abs() ** 3).sum(dim=(1, 2, 3))
    s_sum = ((s[:, :, 1:] - s[:, :, :-1]).abs() ** 3).sum(dim=(1, 2, 3)) + ((s[:, :, :, 1:] - s[:, :, :, :-1]).abs() ** 3).sum(dim=(1, 2, 3))
    b_tvt = lam2 / cells * (sum_bound(t_sum, n + 2) + (w * ect).sum(dim=(1, 2, 3))) + gamma(2) * tvt.detach().abs()
    b_tvs = lam3 / cells * (sum_bound(s_sum, 2 * n + 2) + ech.sum(dim=(1, 2, 3)) + ecw.sum(dim=(1, 2, 3))) + gamma(2) * tvs.detach().abs()
    # gradient: scatter each pair's bound to both members
    et, at = torch.zeros_like(s), torch.zeros_like(s)
    for e, p, lo, hi in ((w * ept, w * pt, (slice(None), slice(0, -1)), (slice(None), slice(1, None))),):
        et[lo] += e; et[hi] += e; at[lo] += p; at[hi] += p
    es, as_ = torch.zeros_like(s), torch.zeros_like(s)
    es[:, :, :-1] += eph; es[:, :, 1:] += eph; as_[:, :, :-1] += ph; as_[:, :, 1:] += ph
    es[:, :, :, :-1] += epw; es[:, :, :, 1:] += epw; as_[:, :, :, :-1] += pw; as_[:, :, :, 1:] += pw
    b_dreg = (lam2 * (et + gamma(10) * at) + lam3 * (es + gamma(10) * as_)) / cells + gamma(4) * lam1 / cells
    return dict(sig=s, b_sig=E_S * s, terms=torch.stack([l1, tvt, tvs], dim=1).detach(),
                b_terms=torch.stack([b_l1, b_tvt, b_tvs], dim=1), dreg=S.grad.clone(), b_dreg=b_dreg)


@functools.lru_cache(maxsize=None)
def reg_case(name):
    raw = reg_raw(name)
    return dict(raw=raw, **reg_ref(raw))


# ------------------------------------------------------------------------------------------------ the whole chain
def chain_grad64(R, AH, AW, x, g):
    """Hand-written fp64 gradient of L = sum(P * g), P = per-pixel freeze of x by M = A_H sigmoid(R) A_W^T, with respect
    to R [B,T,gh,gw]: dM by the explicit formula, dS = A_H^T dM A_W, dR = dS S (1 - S).  x, g [B,C,T,H*W]."""
    B, T, gh, gw = R.shape
    H, W = AH.shape[0], AW.shape[0]
    S = torch.sigmoid(R.double())
    M = expand64(S, AH, AW).reshape(B, T, H * W)
    P, G = stfreeze_fwd64(x, M), stfreeze_scan64(g, M)
    diff = torch.zeros_like(P)
    diff[:, :, 1:] = P[:, :, :-1] - x.double()[:, :, 1:]
    dM = (diff * G).sum(dim=1)
    dM[:, 0] = 0.0
    dS = expand_bwd64(dM.view(B, T, H, W), AH, AW)
    return dS * S * (1 - S)


def chain_autograd64(R, AH, AW, x, g):
    B, T, gh, gw = R.shape
    H, W = AH.shape[0], AW.shape[0]
    Rd = R.double().clone().requires_grad_()
    M = (AH.double() @ torch.sigmoid(Rd) @ AW.double().t()).reshape(B, T, H * W)
    ((stfreeze_fwd64(x, M) * g.double()).sum() + 0.0 * Rd.sum()).backward()     # T = 1: P does not depend on R
    return Rd.grad


# ------------------------------------------------------------------------------------------------ chain on a backbone
# One iteration through a small ConvLSTM plan: clstm_refs' case S2 (C = 2, T = 6, 24 x 32, two layers), grid 3 x 4,
# sigma 1.  dS = d score / d S by torch fp64 autograd through clstm_refs' functional model; the gate is that module's:
# GATE_MARGIN x the float32 floor of the same quantity (the same chain run in float32 torch), measured per clip with
# clstm_refs.elem_err.  The clips are those for which clstm_refs' ambiguity criterion (no pool window of the float64
# run within tau of a tie, on the PERTURBED clip) leaves no clip out; the host test asserts it.
CHAIN_CASE, CHAIN_GRID, CHAIN_SIGMA = 'S2', (3, 4), 1.0


def _chain_run(case, x, sd, targets, raw, AH, AW, dtype):
    """(dS [b,T,gh,gw], probs, run dict) of the chain in `dtype`, the perturbed clip built by the per-pixel recurrence"""
    import clstm_refs as CR
    b, C, T, H, W = x.shape
    S = torch.sigmoid(raw.to(dtype)).requires_grad_()
    M = (AH.to(dtype) @ S @ AW.to(dtype).t())
    xd = x.to(dtype)
    frames = [xd[:, :, 0]]
    for u in range(1, T):
        mu = M[:, u].unsqueeze(1)
        frames.append((1 - mu) * xd[:, :, u] + mu * frames[-1])
    P = torch.stack(frames, dim=2)
    res = CR.run(case, P.detach(), sd, dtype, targets=targets)
    P.backward(torch.from_numpy(res["dx"]).to(dtype))
    return S.grad.detach().double().numpy(), res


@functools.lru_cache(maxsize=None)
def chain_case():
    import clstm_refs as CR
    case = CR.CASES[CHAIN_CASE]
    x, sd, targets, _ = CR.case_inputs(case)
    gh, gw = CHAIN_GRID
    raw = (torch.rand(case.b, case.T, gh, gw, generator=_gen('chainraw')) * 4 - 2).float().contiguous()
    AH, AW = axis_weights(case.H, gh, CHAIN_SIGMA), axis_weights(case.W, gw, CHAIN_SIGMA)
    dS64, ref = _chain_run(case, x, sd, targets, raw, AH, AW, torch.float64)
    dS32, r32 = _chain_run(case, x, sd, targets, raw, AH, AW, torch.float32)
    floor = max(CR.U, float(np.max(CR.elem_err(dS32, dS64))))
    fwd_floor = {n: max(CR.U, float(np.max(e))) for n, e in CR.errors(r32, ref, True).items()}
    amb, ties = CR.ambiguous_windows(ref["pre"], fwd_floor)
    return dict(case=case, x=x, sd=sd, targets=targets, raw=raw, AH=AH, AW=AW, dS=dS64, floor=floor,
                gate=CR.GATE_MARGIN * floor, ambiguous=amb, score=ref["score"], probs=ref["probs"])
