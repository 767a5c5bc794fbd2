"""The freeze and one-blob staging kernels of csrc/mask_ops.hip, called directly through the C-ABI on every dispatch
path and compared with float64 references (tests/mask_refs.py: case tables, references and the derivation of every gate;
tests/test_mask_refs_host.py proves them on the CPU on the same inputs).

No gate here is a hand-picked tolerance: each is bit equality, an exact 0.0, or a bound derived in mask_refs' docstring
and applied per element (per dmask entry), never as a maximum over a tensor.  Every output has a sentinel row in front
and one behind, the reduction workspace has guard bytes on both sides, pad lanes of a channels-last gradient are NaN and
dx is pre-filled with a NaN pattern.
"""
import pytest
import torch

import mask_refs as M
from conftest import note
from test_gpu_leaf_kernels import bits, guarded, inside, untouched

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00ABC
RUNS = M.freeze_runs()
RUN_IDS = [f"{n}-{'perclip' if pc else 'shared'}" for n, pc in RUNS]


def bounded(got, ref, bound, what):
    """every element finite and inside its own bound; returns the worst error in units of the bound"""
    assert not bool(torch.isnan(got).any()), f"{what}: NaN in the output"
    err = inside(got, ref, bound, what)
    nz = bound > 0
    assert bool((err[~nz] == 0).all()), f"{what}: an element with a zero bound is not exact"
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def same(a, b):
    """bit equality, the sign of a zero aside (x + 0.0 turns -0.0 into +0.0 and nothing else)"""
    return torch.equal(bits(a + 0.0), bits(b + 0.0))


# ---------------------------------------------------------------------------------------------------- freeze forward
def run_fwd(xd, maskd, shape, per_clip, cpad):
    import ivf_lib as L
    B, C, T, HW = shape
    buf, p = guarded((B, C, T, HW) if cpad == 0 else (B, T, HW, cpad))
    L.check(L.lib().ivf_freeze_fwd(L.ptr(xd), L.ptr(maskd), L.ptr(p), B, C, T, HW, per_clip, cpad, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), f"freeze_fwd out_cpad={cpad}: a sentinel row was written"
    return p


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_freeze_fwd(run):
    """NCTHW inside gamma(4u) max|X[..u]| of mask_ref.freeze in float64, per element; frame 0 copied bit for bit; the
    channels-last layouts (16-byte rows for C <= 4, rows of 8 for every C) equal NCTHW bit for bit with pad lanes
    exactly 0.0 (the buffers start out filled with the sentinel, so the zeros are the kernels' own)."""
    import ivf_lib as L
    name, per_clip = run
    shape = B, C, T, HW = M.FREEZE_CASES[name]
    c = M.freeze_case(name, per_clip)
    xd, maskd = c['x'].cuda(), c['masks'].cuda()
    p = run_fwd(xd, maskd, shape, per_clip, 0)
    worst = bounded(p, c['P'], c['bP'], f"freeze_fwd {name}")
    assert torch.equal(bits(p[:, :, 0]), bits(xd[:, :, 0]))
    if T == 1:
        assert torch.equal(bits(p), bits(xd))
    for cpad in M.out_layouts(C)[1:]:
        pcl = run_fwd(xd, maskd, shape, per_clip, cpad)
        assert torch.equal(bits(pcl[..., :C].permute(0, 3, 1, 2)), bits(p)), f"out_cpad={cpad} differs from NCTHW"
        if cpad > C:
            assert torch.equal(bits(pcl[..., C:]), torch.zeros_like(bits(pcl[..., C:]))), f"out_cpad={cpad}: pad lane not +0.0"
    if C > 4:
        buf, q = guarded((B, T, HW, 4))
        assert L.lib().ivf_freeze_fwd(L.ptr(xd), L.ptr(maskd), L.ptr(q), B, C, T, HW, per_clip, 4, L.stream()) != 0
        torch.cuda.synchronize()
        assert untouched(buf) and bool((q == -12345.0).all())
    note(f"mask freeze_fwd {name} {shape} per_clip={per_clip}: worst err/gate {worst:.3f}; layouts {M.out_layouts(C)} bit-equal")


# ---------------------------------------------------------------------------------------------------- freeze backward
class Workspace:
    def __init__(self, B, T):
        import ivf_lib as L
        self.n = L.lib().ivf_freeze_bwd_workspace_bytes(B, T)
        self.buf = torch.full((self.n + 512,), 0xA5, dtype=torch.uint8, device='cuda')     # 256 guard bytes on each side
        self.ws = self.buf[256:256 + self.n]

    def intact(self):
        return bool((self.buf[:256] == 0xA5).all()) and bool((self.buf[256 + self.n:] == 0xA5).all())


def grad_layout(g, cpad):
    """the upstream gradient as the kernel reads it: NCTHW, or channels-last rows of `cpad` with NaN pad lanes"""
    if cpad == 0:
        return g.cuda()
    B, C, T, HW = g.shape
    gd = torch.full((B, T, HW, cpad), float('nan'), device='cuda')
    gd[..., :C] = g.cuda().permute(0, 2, 3, 1)
    return gd


def run_bwd(xd, maskd, gd, shape, per_clip, cpad, want_dx, wsp):
    """two calls, identical bits; sentinels, workspace guards and the NaN pre-fill of dx checked after each"""
    import ivf_lib as L
    B, C, T, HW = shape
    outs = []
    for _ in range(2):
        db, dm = guarded((B, T))
        xb, dx = guarded((B, C, T, HW)) if want_dx else (None, None)
        if want_dx:
            bits(dx).fill_(NAN_BITS)
        L.check(L.lib().ivf_freeze_bwd(L.ptr(xd), L.ptr(maskd), L.ptr(gd), L.ptr(dm), L.ptr(dx), B, C, T, HW, per_clip, cpad,
                                       L.ptr(wsp.ws), L.stream()))
        torch.cuda.synchronize()
        assert untouched(db) and wsp.intact() and (xb is None or untouched(xb)), f"freeze_bwd g_cpad={cpad}: wrote out of bounds"
        outs.append((dm, dx))
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])), "dmask differs between two calls"
    if want_dx:
        assert torch.equal(bits(outs[0][1]), bits(outs[1][1]))
        assert not bool(torch.isnan(outs[0][1]).any()), "an element of dx was never written"
    return outs[0]


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_freeze_bwd(run):
    """dmask and dx against fp64 autograd of mask_ref.freeze with loss (p * g).sum(), the gradient as NCTHW and as
    channels-last rows of 4 (C <= 4) and 8 with NaN pad lanes, with and without dx: every dmask entry inside its
    three-part gate, every dx element inside the scan bound plus two roundings, dmask[:, 0] exactly 0.0."""
    name, per_clip = run
    shape = B, C, T, HW = M.FREEZE_CASES[name]
    c = M.freeze_case(name, per_clip)
    xd, maskd = c['x'].cuda(), c['masks'].cuda()
    wsp = Workspace(B, T)
    figs = []
    for cpad in M.out_layouts(C):
        gd = grad_layout(c['g'], cpad)
        for want_dx in (False, True):
            dm, dx = run_bwd(xd, maskd, gd, shape, per_clip, cpad, want_dx, wsp)
            kern = "%s<%d>" % M.bwd_kernel(C, T, cpad, want_dx)
            what = f"freeze_bwd {name} g_cpad={cpad} dx={int(want_dx)} ({kern})"
            assert torch.equal(bits(dm[:, 0]), torch.zeros_like(bits(dm[:, 0]))), f"{what}: dmask[:, 0] is not +0.0"
            w_dm = bounded(dm, c['dmask'], c['b_dmask'], what + " dmask")
            fig = f"g_cpad={cpad} dx={int(want_dx)} {kern}: dmask {w_dm:.4f}"
            if want_dx:
                fig += f" dx {bounded(dx, c['dx'], c['b_dx'], what + ' dx'):.3f}"
                if T == 1:
                    assert torch.equal(bits(dx), bits(c['g'].cuda()))
            if T == 1:
                assert torch.equal(bits(dm), torch.zeros_like(bits(dm)))
            figs.append(fig)
    note(f"mask freeze_bwd {name} {shape} per_clip={per_clip}: worst err/gate | " + " | ".join(figs))


@pytest.mark.parametrize("run", M.exact_runs(), ids=lambda r: f"{r[0]}-{'perclip' if r[1] else 'shared'}")
def test_freeze_bwd_exact(run):
    """Inputs on which every fp32 operation is exact (test_exact_cases_are_exact): whatever the order of the sums,
    dmask and dx must equal the float64 result rounded once, bit for bit, in every layout and on both kernels.  The
    probes sit at the first and last index of every trip and block boundary, so an element dropped there shows; the
    F9 shape adds the ten trips of the generic kernel and the four of the channels-last one."""
    name, per_clip = run
    shape = B, C, T, HW = M.FREEZE_CASES[name]
    c = M.exact_case(name, per_clip)
    xd, maskd = c['x'].cuda(), c['masks'].cuda()
    want_dm, want_dx = c['dmask'].float().cuda(), c['dx'].float().cuda()
    assert torch.equal(want_dm.double().cpu(), c['dmask']) and torch.equal(want_dx.double().cpu(), c['dx'])
    wsp = Workspace(B, T)
    ran = []
    for cpad in M.out_layouts(C):
        gd = grad_layout(c['g'], cpad)
        for with_dx in (False, True):
            dm, dx = run_bwd(xd, maskd, gd, shape, per_clip, cpad, with_dx, wsp)
            what = f"exact {name} g_cpad={cpad} dx={int(with_dx)}"
            if not same(dm, want_dm):
                bad = torch.nonzero(dm != want_dm)
                b, u = bad[0].tolist()
                raise AssertionError(f"{what}: {bad.shape[0]} dmask entries differ, first [{b},{u}] = {float(dm[b, u])!r} "
                                     f"for {float(want_dm[b, u])!r}")
            if with_dx:
                assert same(dx, want_dx), f"{what}: {int((dx != want_dx).sum())} dx elements differ"
            ran.append("%s<%d>" % M.bwd_kernel(C, T, cpad, with_dx))
    note(f"mask freeze_bwd exact {name} {shape} per_clip={per_clip}: dmask and dx bit-equal to fp64 on {sorted(set(ran))}, "
         f"{len(ran)} layout/dx combinations")


# ---------------------------------------------------------------------------------------------------- one-blob staging
def run_stage(xd, case, mode, first, count, cpad):
    import ivf_lib as L
    b, C, T, HW, ml = case
    buf, p = guarded((count, C, T, HW) if cpad == 0 else (count, T, HW, 4))
    if cpad == 4 or (HW % 4 == 0 and xd.data_ptr() % 16 == 0):      # the 16-byte paths: cl4, ncthw<4>
        assert p.data_ptr() % 16 == 0
    L.check(L.lib().ivf_blob_stage(L.ptr(xd), b, C, T, HW, ml, mode, first, count, L.ptr(p), cpad, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), f"blob_stage out_cpad={cpad} rows [{first}, {first + count}): a sentinel row was written"
    return p


@pytest.mark.parametrize("mode", [0, 1], ids=["freeze", "reverse"])
@pytest.mark.parametrize("name", list(M.BLOB_CASES))
def test_blob_stage(name, mode):
    """ivf_blob_stage == mask_ref.perturb_sequence under each candidate's binary mask, bit for bit: the whole range, a
    chunk from the middle of clip 0's candidates into clip 1's, and the last candidate alone; 16-byte channels-last
    (pad lanes 0.0), NCTHW (<4> when HW % 4 == 0, else <1>) and NCTHW from clips one float off alignment (<1>)."""
    case = b, C, T, HW, ml = M.BLOB_CASES[name]
    x = M.blob_input(name)
    xd = x.cuda()
    assert xd.data_ptr() % 16 == 0
    off = torch.empty(x.numel() + 1, device='cuda')[1:].view(x.shape)
    off.copy_(xd)
    assert off.data_ptr() % 16 == 4
    ref = M.blob_ref(name, mode).cuda()
    n = ref.shape[0] // b
    assert not torch.equal(ref, xd[:, None].expand(b, n, C, T, HW).reshape(ref.shape))
    paths = []
    for first, count in M.blob_chunks(b, n):
        want = ref[first:first + count]
        pcl = run_stage(xd, case, mode, first, count, 4)
        assert torch.equal(bits(pcl[..., :C].permute(0, 3, 1, 2)), bits(want)), f"cl4 rows [{first}, {first + count})"
        if C < 4:
            assert torch.equal(bits(pcl[..., C:]), torch.zeros_like(bits(pcl[..., C:])))
        assert torch.equal(bits(run_stage(xd, case, mode, first, count, 0)), bits(want)), f"NCTHW rows [{first}, {first + count})"
        paths = ['cl4', 'ncthw<4>' if HW % 4 == 0 else 'ncthw<1>']
        if HW % 4 == 0:
            assert torch.equal(bits(run_stage(off, case, mode, first, count, 0)), bits(want)), f"NCTHW, unaligned clips, rows [{first}, {first + count})"
            paths.append('ncthw<1> (clips one float off)')
    note(f"mask blob_stage {name} {case} mode={mode}: {b * n} rows, chunks {M.blob_chunks(b, n)} bit-equal on {paths}")


# ---------------------------------------------------------------------------------------------------- reverse, one mask
@pytest.mark.parametrize("shape", M.REV_CL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reverse_fwd_channels_last(shape):
    """ivf_reverse_fwd (one mask for all clips, the form mask.py uses) with out_cpad 4 and 8: equal to its NCTHW
    output bit for bit, pad lanes exactly 0.0; NCTHW itself inside four roundings of the blend, per element."""
    import ivf_lib as L
    from leaf_refs import rev_inputs, reverse_ref
    B, C, T, HW = shape
    mask = M.rev_single_mask(T)
    x, _ = rev_inputs(shape)
    xd, maskd = x.cuda(), mask.cuda()
    run = torch.empty(T, dtype=torch.int32, device='cuda')
    partner = torch.empty(T, dtype=torch.int32, device='cuda')
    weight = torch.empty(T, device='cuda')
    L.check(L.lib().ivf_submask_pairs(L.ptr(maskd), T, 0.1, L.ptr(run), L.ptr(partner), L.ptr(weight), L.stream()))
    outs = {}
    for cpad in (0, 4, 8):
        buf, p = guarded((B, C, T, HW) if cpad == 0 else (B, T, HW, cpad))
        L.check(L.lib().ivf_reverse_fwd(L.ptr(xd), L.ptr(partner), L.ptr(weight), L.ptr(p), B, C, T, HW, cpad, L.stream()))
        torch.cuda.synchronize()
        assert untouched(buf)
        outs[cpad] = p
    want = reverse_ref(x, mask[None].expand(B, T))
    pt = partner.cpu().long()
    assert bool((pt != torch.arange(T)).any())
    pair_max = torch.maximum(x.double().abs(), x.double().abs()[:, :, pt])
    bound = M.gamma(4) * pair_max * (pt != torch.arange(T)).view(1, 1, T, 1)       # copied frames: exact
    worst = bounded(outs[0], want, bound, f"reverse_fwd {shape}")
    assert not torch.equal(outs[0], xd)
    for cpad in (4, 8):
        assert torch.equal(bits(outs[cpad][..., :C].permute(0, 3, 1, 2)), bits(outs[0]))
        if cpad > C:
            assert torch.equal(bits(outs[cpad][..., C:]), torch.zeros_like(bits(outs[cpad][..., C:])))
    note(f"mask reverse_fwd {shape}: NCTHW worst err/gate {worst:.3f}; out_cpad 4 and 8 bit-equal, pad lanes 0.0")
