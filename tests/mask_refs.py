"""Case tables, seeded inputs, fp64 references and error bounds for the freeze and one-blob staging kernels of
csrc/mask_ops.hip (test_gpu_mask_kernels.py on the GPU, test_mask_refs_host.py on the CPU).  Both files iterate the
tables below, so the host test proves the references, the bounds and what a wrong kernel would do to them on exactly the
inputs the kernels are later compared on.  Nothing here needs a GPU; the blob tables need the HIP library for
ivf_blob_count only.

Rounding model.  U = 2^-24 is the unit roundoff of fp32; gamma(k) = k U / (1 - k U) bounds the relative error of a
quantity that went through k roundings (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1), to all
orders.  An FMA contraction only removes roundings, so every bound below holds with or without it.

Freeze forward, P[0] = X[0], P[u] = (1 - m[u]) X[u] + m[u] P[u-1] with m in [0, 1].  P[u] is a convex combination of
X[0..u], so |P[u]| <= M[u] = max_{v<=u} |X[v]| at that pixel.  One step rounds FOUR times: 1 - m, its product with
X[u], the product m P[u-1], and the sum.  With e[u] = |computed P[u] - P[u]|:
    e[u] <= m e[u-1] + (2 (1-m) |X[u]| + m |P[u-1]| + |P[u]|) U  <=  e[u-1] + 3 U M[u]      (first order),
and e[0] = 0 (frame 0 is copied).  The gate is the rounding COUNT, 4, which also covers the higher-order terms:
    b_P[u] = gamma(4 u) M[u]                    (`freeze_fwd_bound`).

Reverse scan of the backward, G[T-1] = g[T-1], G[u] = g[u] + m[u+1] G[u+1].  |G[u]| <= S[u] = sum_{v>=u} |g[v]|.  One
step rounds TWICE (product, sum): e[u] <= m e[u+1] + (m |G[u+1]| + |G[u]|) U <= e[u+1] + 2 U S[u], e[T-1] = 0:
    b_G[u] = gamma(2 (T-1-u)) S[u]              (`freeze_scan_bound`).

dmask[b,u] = sum over (c, px) of term = (P[u-1] - X[u]) G[u], u >= 1.  Its gate is per entry and has three parts
(`freeze_bwd_ref`): the fp32 summation of C*HW terms in any order, leaf_refs.sum_bound(sum|term|, C*HW) (its factor 2
covers the two roundings of the term itself, the difference and the product, since 2 (n-1) >= n + 1 from n = 3 on, and
no case has fewer than 15 terms); the forward bound carried through, sum b_P[u-1] |G[u]|; the scan bound carried
through, sum b_G[u] |P[u-1] - X[u]| (plus the product of the two bounds, which is second order and kept so that the
gate is a bound and not an estimate).  dmask[:, 0] is exactly 0.0: m[0] never enters the recurrence.

dX[0] = G[0], dX[u] = (1 - m[u]) G[u]: the G bound plus two roundings (1 - m and the product),
    b_dX[u] = b_G[u] + gamma(2) |dX[u]|         (b_G[u] alone at u = 0 and wherever T = 1).
"""
import functools
import zlib

import torch

from leaf_refs import REV_SHAPES, U, sum_bound  # noqa: F401  (re-exported for the two test files)


def gamma(k):
    return k * U / (1.0 - k * U)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7fffffff)


# ------------------------------------------------------------------------------------------------ freeze: case table
# (B, C, T, HW).  Kernels and template instantiations each case launches (fwd, the frame-mask kind of the freeze-scan
# family: NCTHW freeze_fwd_ncthw / out_cpad 4 freeze_fwd_cl4<TT> / out_cpad 8 freeze_fwd_cl, which writes its own pad
# lanes; bwd: g NCTHW / g_cpad 4 / g_cpad 8, each with and without dX; every bwd ends in freeze_bwd_reduce):
#   F1  freeze_fwd_ncthw, freeze_fwd_cl4<16>, freeze_fwd_cl; freeze_bwd<16> with C*HW = 37635: three trips of 16384, the last
#       ragged (4867) and not block-aligned; freeze_bwd_cl4<16> one trip
#   F2  freeze_bwd_cl4<16> second trip (HW = 20003 > 16384, ragged); freeze_bwd<16> with four trips (60009)
#   F3  C = 1, 65 clips (more clips than one wave of blocks), T = 9 ragged inside <16>, 63 of 64 blocks empty
#   F4  freeze_bwd<64> with 24 guarded frames; T > 32 sends g_cpad 4 through the generic kernel; 130 clips
#   F5  freeze_bwd_cl4<32> full, C = 4 (the .w lane); freeze_bwd<32> full
#   F6  freeze_bwd<32> and freeze_bwd_cl4<32> with 15 guarded frames
#   F7  freeze_bwd<64> full
#   F8  T = 1: p == x, dmask == 0.0, dx == g
#   F9  forward grid cap (2048 blocks of 256): freeze_fwd_ncthw 1 655 808 threads (four trips), freeze_fwd_cl4<0> and
#       freeze_fwd_cl 551 936 each (two trips); 13 MB of input.  Its out_cpad 8 output is 35 MB (out_cpad 8 runs on every
#       case).  Backward: ten trips of the generic kernel, four of the channels-last one (also an exact case).
#   F10 C > 4: freeze_fwd_cl with out_cpad 8 (out_cpad 4 is refused), backward with g_cpad 8
# The generic backward with dX and a channels-last gradient together runs in every case.
FREEZE_CASES = {
    'F1': (2, 3, 16, 12545),
    'F2': (1, 3, 16, 20003),
    'F3': (65, 1, 9, 15),
    'F4': (130, 4, 40, 15),
    'F5': (7, 4, 32, 240),
    'F6': (3, 3, 17, 240),
    'F7': (2, 1, 64, 240),
    'F8': (3, 2, 1, 33),
    'F9': (11, 3, 2, 50176),
    'F10': (5, 5, 16, 63),
}
EXACT_CASES = ['F1', 'F2', 'F4', 'F5', 'F9']     # F9 beyond the issue's four: ten trips of the generic backward, four of cl4
BWD_THREADS = 64 * 256          # FREEZE_BWD_BLOCKS_PER_CLIP blocks of 256 threads per clip


def freeze_runs():
    """(case name, mask_per_clip): every case with per-clip rows, and every case with B > 1 once more with row 0
    shared by all clips."""
    return [(n, pc) for n, s in FREEZE_CASES.items() for pc in ((1, 0) if s[0] > 1 else (1,))]


def exact_runs():
    return [r for r in freeze_runs() if r[0] in EXACT_CASES]


def out_layouts(C):
    """cpad values of the channels-last layouts a case runs, after 0 (NCTHW)"""
    return (0, 4, 8) if C <= 4 else (0, 8)


def bwd_kernel(C, T, g_cpad, dx):
    """which backward kernel ivf_freeze_bwd launches: ('cl4' = freeze_bwd_cl4_kernel | 'generic' = freeze_bwd_kernel,
    template T as with_frames_upto of csrc/ivf_common.h picks it)"""
    TT = 16 if T <= 16 else (32 if T <= 32 else 64)
    return ('cl4' if (g_cpad == 4 and C <= 4 and not dx and T <= 32) else 'generic'), TT


def freeze_masks(B, T):
    """[B,T] fp32 rows, cycling: random in (0,1); random with exact 0.0 and 1.0 entries; all zero (the identity, yet
    dmask != 0); all one; saturated sigmoid(+-5) values."""
    g = _gen('freezemask', B, T)
    sat = torch.sigmoid(torch.tensor([-5.0, 5.0]))
    rows = []
    for b in range(B):
        kind = b % 5
        m = torch.rand(T, generator=g) * 0.98 + 0.01
        pick = torch.randint(0, 2, (T,), generator=g)
        if kind == 1:
            m[1::3] = pick[1::3].float()
        elif kind == 2:
            m = torch.zeros(T)
        elif kind == 3:
            m = torch.ones(T)
        elif kind == 4:
            m = sat[pick]
        rows.append(m.float())
    return torch.stack(rows).contiguous()


def freeze_inputs(name):
    """x [B,C,T,HW] in 10..250 falling over time (by 180 / (1 + c/2) over the clip, channel c) plus noise of at most
    one frame step; g = 0.3 + 0.15 c + noise in +-0.2, all positive.  P[u-1] - X[u] and G[u] are then mostly positive,
    the terms of a dmask entry mostly share a sign, and both x and g differ from channel to channel by more than their
    noise: a gradient read from the wrong frame, pixel or lane moves the sum instead of hiding in cancellation."""
    B, C, T, HW = FREEZE_CASES[name]
    gen = _gen('freeze', name)
    amp = 180.0 / (1.0 + 0.5 * torch.arange(C, dtype=torch.float32)).view(1, C, 1, 1)
    t = torch.arange(T, dtype=torch.float32).view(1, 1, T, 1) / max(T - 1, 1)
    step = amp / max(T - 1, 1)
    noise = (torch.rand(B, C, T, HW, generator=gen) * 2 - 1) * torch.clamp(step, max=30.0)
    x = 220.0 - amp * t + noise
    g = 0.3 + 0.15 * torch.arange(C, dtype=torch.float32).view(1, C, 1, 1) + (torch.rand(B, C, T, HW, generator=gen) - 0.5) * 0.4
    return x.contiguous(), g.contiguous()


def rows_for(masks, B, per_clip):
    """[B,T] rows as the kernel reads them: its own row per clip, or row 0 for every clip"""
    return masks if per_clip else masks[:1].expand(B, masks.shape[1])


# ------------------------------------------------------------------------------------------------ freeze: references
def freeze_fwd_bound(x):
    """b_P [B,C,T,HW] float64 (module docstring): gamma(4 u) * max_{v<=u} |X[v]|"""
    T = x.shape[2]
    M = torch.cummax(x.double().abs(), dim=2).values
    k = torch.tensor([gamma(4 * u) for u in range(T)], dtype=torch.float64).view(1, 1, T, 1)
    return k * M


def freeze_scan_bound(g):
    """b_G [B,C,T,HW] float64 (module docstring): gamma(2 (T-1-u)) * sum_{v>=u} |g[v]|"""
    T = g.shape[2]
    S = torch.flip(torch.cumsum(torch.flip(g.double().abs(), (2,)), dim=2), (2,))
    k = torch.tensor([gamma(2 * (T - 1 - u)) for u in range(T)], dtype=torch.float64).view(1, 1, T, 1)
    return k * S


def freeze_fwd_ref(x, rows):
    """oracle.mask_ref.freeze in float64: [B,C,T,HW]"""
    from oracle import mask_ref
    B, C, T, HW = x.shape
    return mask_ref.freeze(x.double().view(B, C, T, HW, 1), rows.double())[..., 0]


def freeze_scan64(g, rows):
    """G [B,C,T,HW] float64: G[T-1] = g[T-1], G[u] = g[u] + m[u+1] G[u+1]"""
    B, C, T, HW = g.shape
    gd, m = g.double(), rows.double()
    G = [None] * T
    G[T - 1] = gd[:, :, T - 1]
    for u in range(T - 2, -1, -1):
        G[u] = gd[:, :, u] + m[:, u + 1].view(B, 1, 1) * G[u + 1]
    return torch.stack(G, dim=2)


def freeze_bwd_ref(x, g, rows):
    """fp64 autograd of mask_ref.freeze with loss (p * g).sum(), and the gates of the module docstring.

    dmask [B,T]: with a shared mask row the kernel still writes one row per clip (the caller sums them), so the loss
    is differentiated with respect to the expanded [B,T] rows in both modes.  Returns dmask, dx, b_dmask, b_dx, and
    the explicit formula's pieces: the terms' sum (`formula`), sum|term| (`sabs`), P, G."""
    from oracle import mask_ref
    B, C, T, HW = x.shape
    m = rows.double().clone().requires_grad_()
    xd = x.double().view(B, C, T, HW, 1).clone().requires_grad_()
    p = mask_ref.freeze(xd, m)
    (p[..., 0] * g.double()).sum().backward()
    dmask = m.grad.clone() if m.grad is not None else torch.zeros(B, T, dtype=torch.float64)
    dx = xd.grad[..., 0].clone()
    P = p.detach()[..., 0]
    G = freeze_scan64(g, rows)
    bP, bG = freeze_fwd_bound(x), freeze_scan_bound(g)
    xx = x.double()
    diff = torch.zeros_like(P)
    diff[:, :, 1:] = P[:, :, :-1] - xx[:, :, 1:]
    term = diff * G
    term[:, :, 0] = 0.0
    sabs = term.abs().sum(dim=(1, 3))
    bPprev = torch.zeros_like(P)
    bPprev[:, :, 1:] = bP[:, :, :-1]
    prop = (bPprev * G.abs() + bG * diff.abs() + bPprev * bG)
    prop[:, :, 0] = 0.0
    b_dmask = sum_bound(sabs, C * HW) + prop.sum(dim=(1, 3))
    b_dmask[:, 0] = 0.0
    b_dx = bG + gamma(2) * dx.abs()
    b_dx[:, :, 0] = bG[:, :, 0]
    return dict(dmask=dmask, dx=dx, b_dmask=b_dmask, b_dx=b_dx, formula=term.sum(dim=(1, 3)), sabs=sabs, P=P, G=G)


@functools.lru_cache(maxsize=None)
def freeze_case(name, per_clip):
    """inputs and references of one run of the table, computed once and shared by the tests that need them (read-only)"""
    B, C, T, HW = FREEZE_CASES[name]
    x, g = freeze_inputs(name)
    masks = freeze_masks(B, T)
    rows = rows_for(masks, B, per_clip)
    ref = freeze_bwd_ref(x, g, rows)
    return dict(x=x, g=g, masks=masks, rows=rows, bP=freeze_fwd_bound(x), **ref)


# ------------------------------------------------------------------------------------------------ freeze: exact cases
def probe_indices(C, HW, seed_key):
    """flat indices i = c * HW + px of the probe elements of one clip (at most 64): the boundaries of the index space
    of both backward kernels (the generic one strides i over C*HW, the channels-last one px over HW, both by 16384)"""
    n = C * HW
    want = [0, 255, 256, 16383, 16384, 16385, n - 1, HW - 1, HW]
    for k in range(1, n // BWD_THREADS + 1):
        want += [k * BWD_THREADS - 1, k * BWD_THREADS]
    for k in range(1, HW // BWD_THREADS + 1):                 # the same pixel boundaries in the last channel
        want += [(C - 1) * HW + k * BWD_THREADS - 1, (C - 1) * HW + k * BWD_THREADS]
    idx = sorted({i for i in want if 0 <= i < n})
    extra = torch.randint(0, n, (32,), generator=_gen('probe', seed_key)).tolist()
    idx = sorted(set(idx) | set(extra[:64 - len(idx)]))          # 32 seeded positions, fewer where the boundaries leave no room
    assert len(idx) <= 64
    return idx


def exact_inputs(name):
    """Inputs on which every fp32 operation of the freeze kernels is exact: x integer in 0..255; mask rows in
    {0, 0.5, 1} with at most two entries of 0.5 (P and G are then multiples of 1/4, a term of 1/16); g zero but at
    the probe elements, where it holds integers in -3..3 in a quarter of the frames (and a non-zero one in the last)."""
    B, C, T, HW = FREEZE_CASES[name]
    gen = _gen('exact', name)
    x = torch.randint(0, 256, (B, C, T, HW), generator=gen).float()
    masks = torch.randint(0, 2, (B, T), generator=gen).float()
    for b in range(B):
        if T > 2:
            masks[b, torch.randint(1, T, (2,), generator=gen)] = 0.5
        else:                       # one entry that matters: all three values over the clips
            masks[b, 1] = (0.0, 0.5, 1.0)[b % 3]
    g = torch.zeros(B, C, T, HW)
    probes = []
    for b in range(B):
        idx = probe_indices(C, HW, (name, b))
        probes.append(idx)
        ii = torch.tensor(idx)
        val = torch.randint(-3, 4, (len(idx), T), generator=gen).float()
        val = val * (torch.rand(len(idx), T, generator=gen) < 0.25).float()
        val[:, T - 1] = torch.randint(1, 4, (len(idx),), generator=gen).float()      # every probe carries something
        gb = torch.zeros(C * HW, T)
        gb[ii] = val
        g[b] = gb.view(C, HW, T).permute(0, 2, 1)
        if T == 2:                  # a probe's only term is (X[0] - X[1]) g[1]: keep it from vanishing
            cc, px = ii // HW, ii % HW
            same = x[b, cc, 0, px] == x[b, cc, 1, px]
            x[b, cc[same], 1, px[same]] = (x[b, cc[same], 0, px[same]] + 1) % 256
    return x.contiguous(), g.contiguous(), masks.contiguous(), probes


@functools.lru_cache(maxsize=None)
def exact_case(name, per_clip):
    B, C, T, HW = FREEZE_CASES[name]
    x, g, masks, probes = exact_inputs(name)
    rows = rows_for(masks, B, per_clip)
    ref = freeze_bwd_ref(x, g, rows)
    return dict(x=x, g=g, masks=masks, rows=rows, probes=probes, **ref)


# ------------------------------------------------------------------------------------------------ one-blob staging
# (b, C, T, HW, max_len).  out_cpad 4 -> blob_stage_cl4; NCTHW -> blob_stage_ncthw<4> when HW % 4 == 0 and both
# pointers are 16-byte aligned, else <1> (HW = 15, or the clips handed over one float off alignment).
BLOB_CASES = {
    'S1': (2, 3, 9, 240, 9),        # T 9, C 3
    'S2': (2, 1, 16, 15, 16),       # C 1, <1> by HW
    'S3': (2, 4, 64, 15, 3),        # T 64, max_len < T, C 4, <1> by HW
    'S4': (3, 4, 16, 240, 7),       # max_len < T, <4>
    # T 2, 150 rows of 4096 pixels: count*HW = 614 400 > 524 288 threads of the capped grid, so blob_stage_cl4 and
    # blob_stage_ncthw<4> (count*C*HW/4, C = 4) make a second trip and <1> five; each output is 19.7 MB
    'S5': (50, 4, 2, 4096, 2),
}


def blob_table(T, max_len):
    import ivf_search
    return ivf_search.blob_candidates(T, max_len)


def blob_chunks(b, n):
    """(first, count): everything; a chunk from the middle of clip 0's candidates into clip 1's; the last candidate"""
    return [(0, b * n), (n // 2, n), (b * n - 1, 1)]


def blob_input(name):
    b, C, T, HW, ml = BLOB_CASES[name]
    return (torch.rand(b, C, T, HW, generator=_gen('blob', name)) * 255).contiguous()


@functools.lru_cache(maxsize=None)
def blob_ref(name, mode):
    """[b*n, C, T, HW] fp32: mask_ref.perturb_sequence of every clip under the binary mask of every candidate (a binary
    mask makes both perturbations exact gathers: 0 * x + 1 * y == y for finite x)"""
    import ivf_search
    from oracle import mask_ref
    b, C, T, HW, ml = BLOB_CASES[name]
    x = blob_input(name)
    tab = blob_table(T, ml)
    masks = ivf_search.blob_masks(tab, T)
    kind = 'freeze' if mode == 0 else 'reverse'
    out = torch.empty(b, tab.shape[0], C, T, HW)
    for k in range(tab.shape[0]):
        out[:, k] = mask_ref.perturb_sequence(x.view(b, C, T, HW, 1), masks[k].clone(), kind)[..., 0]
    return out.reshape(b * tab.shape[0], C, T, HW)


def blob_src(u, a, L, mode):
    """source frame of frame u under blob (a, L): the rule of the kernels"""
    if u < a or u >= a + L:
        return u
    return (a - 1 if a > 0 else 0) if mode == 0 else 2 * a + L - 1 - u


# ------------------------------------------------------------------------------------------------ reverse, single mask
REV_CL_SHAPES = [REV_SHAPES[1], REV_SHAPES[2]]        # (7, 3, 9, 240), (65, 1, 16, 15)


def rev_single_mask(T):
    """one mask row with an odd run in the middle and a run touching T - 1"""
    from leaf_refs import rev_masks
    return rev_masks(7, T)[3].contiguous()
