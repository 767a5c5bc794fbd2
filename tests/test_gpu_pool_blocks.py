"""Max-pool backward kernels (the strided pools by stride-aligned blocks, the 3x3x3 stride-1 gather) through
ivf_maxpool3d_fwd / ivf_maxpool3d_bwd against a plain numpy fp32 statement of the documented rule, bit for bit:

  forward   the window is scanned in (kt, kh, kw) order over the ZERO-padded input; a tap takes over when it is the
            first, strictly greater, or NaN (so NaN takes the maximum); the recorded code is the flat tap of the
            winner, or 255 -- a dead window -- where gate_nonpos is set and the maximum is not > 0;
  backward  dX starts from the old dX when accumulating, else from 0; the windows are walked in ascending (to, ho, wo)
            order and each adds its dY to the cell its code points at (255 and pad cells: to none); the ReLU gate
            (relu_mask > 0, else 0) is applied last.

The inputs are small integers, so ties and dead windows are everywhere and every sum is exact."""
import ctypes
import itertools

import numpy as np
import pytest

GPU = pytest.mark.gpu

STRIDED = [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2))]
# odd sizes, partial last blocks and front padding 0 / even sizes / a pad cell in front of t, h and w (3-tap windows)
STRIDED_MAPS = [(3, 7, 9), (4, 8, 8), (3, 5, 5)]
S1_MAPS = [(1, 3, 3), (2, 7, 7), (4, 5, 14)]
B, C = 2, 8
IN_LD, IN_COFF = 12, 4      # the pooled tensor: a C = 8 slice at channel 4 of 12
OUT_LD, OUT_COFF = 16, 8    # the pool output / dY: a slice at channel 8 of 16


def geometry(thw, k, s):
    import ivf_arch as arch
    pads = [arch.same_pad(n, kk, ss)[0] for n, kk, ss in zip(thw, k, s)]
    outs = [arch.out_size(n, kk, ss) for n, kk, ss in zip(thw, k, s)]
    return pads, outs


def pool_fwd_ref(x, k, s, pads, outs, dead, dtype=np.float32):
    """x [B,T,H,W,C] fp32 -> (y [B,To,Ho,Wo,C] fp32, code [B,To,Ho,Wo,C] uint8); dtype: the arithmetic of the rule
    (float64: the same rule on an fp64 network, tests/i3d_refs.py)"""
    Bn, T, H, W, Cn = x.shape
    ext = [(o - 1) * ss + kk for o, ss, kk in zip(outs, s, k)]
    xp = np.zeros((Bn, max(ext[0], pads[0] + T), max(ext[1], pads[1] + H), max(ext[2], pads[2] + W), Cn), dtype)
    xp[:, pads[0]:pads[0] + T, pads[1]:pads[1] + H, pads[2]:pads[2] + W] = x
    y = np.zeros((Bn,) + tuple(outs) + (Cn,), dtype)
    code = np.zeros(y.shape, np.uint8)
    for to, ho, wo in itertools.product(*map(range, outs)):
        best = bi = None
        for tap, (kt, kh, kw) in enumerate(itertools.product(*map(range, k))):
            v = xp[:, to * s[0] + kt, ho * s[1] + kh, wo * s[2] + kw]
            if tap == 0:
                best, bi = v.copy(), np.zeros(v.shape, np.uint8)
                continue
            with np.errstate(invalid='ignore'):
                take = (v > best) | (v != v)
            best = np.where(take, v, best)
            bi = np.where(take, np.uint8(tap), bi)
        if dead:
            with np.errstate(invalid='ignore'):
                bi = np.where(best > 0, bi, np.uint8(255))
        y[:, to, ho, wo], code[:, to, ho, wo] = best, bi
    return y, code


def pool_bwd_ref(dy, code, x_shape, k, s, pads, old, gate, dtype=np.float32):
    """dy, code [B,To,Ho,Wo,C]; old: dX to accumulate into or None; gate: the relu_mask tensor or None"""
    Bn, T, H, W, Cn = x_shape
    dx = np.zeros(x_shape, dtype) if old is None else old.astype(dtype).copy()
    bb, cc = np.meshgrid(np.arange(Bn), np.arange(Cn), indexing='ij')
    _, To, Ho, Wo, _ = dy.shape
    for to, ho, wo in itertools.product(range(To), range(Ho), range(Wo)):
        cd = code[:, to, ho, wo].astype(np.int64)
        kt, kh, kw = cd // (k[1] * k[2]), (cd // k[2]) % k[1], cd % k[2]
        ti, hi, wi = to * s[0] - pads[0] + kt, ho * s[1] - pads[1] + kh, wo * s[2] - pads[2] + kw
        ok = (cd != 255) & (ti >= 0) & (ti < T) & (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
        # one target cell per (clip, channel) and window: no index repeats inside this update
        dx[bb[ok], ti[ok], hi[ok], wi[ok], cc[ok]] += dy[:, to, ho, wo][ok]
    if gate is not None:
        with np.errstate(invalid='ignore'):
            dx = np.where(gate > 0, dx, dtype(0))
    return dx


def small_ints(rng, shape):
    return rng.integers(-2, 3, size=shape).astype(np.float32)


# ------------------------------------------------------------------ the numpy rule against the reference's goldens (CPU)
POOL_CASES = {  # the pool table of tests/golden/make_golden.py: window, stride, map
    'p133': ((1, 3, 3), (1, 2, 2), (3, 8, 10)),
    'p133_odd': ((1, 3, 3), (1, 2, 2), (3, 7, 9)),
    'p333s2': ((3, 3, 3), (2, 2, 2), (4, 8, 8)),
    'p333s2_odd': ((3, 3, 3), (2, 2, 2), (5, 15, 7)),
    'p222': ((2, 2, 2), (2, 2, 2), (4, 6, 8)),
    'p222_odd': ((2, 2, 2), (2, 2, 2), (3, 7, 5)),
    'p333s1': ((3, 3, 3), (1, 1, 1), (3, 5, 6)),
    'p333s1t1': ((3, 3, 3), (1, 2, 2), (4, 8, 8)),
}


@pytest.mark.parametrize("name", list(POOL_CASES))
def test_numpy_rule_matches_reference_goldens(name, golden):
    """The rule above reproduces what the reference's MaxPool3dSamePadding gave for the cases of tests/golden/units.npz:
    the forward bit for bit, the backward up to torch's own order of its <= 27-term sums."""
    import ivf_recipe as R
    g = golden('units')
    k, s, thw = POOL_CASES[name]
    pads, outs = geometry(thw, k, s)
    x = np.maximum(R.uniform(f'g/pool/{name}/x', (2, 6) + thw, -1, 1), 0).astype(np.float32)
    gy = R.uniform(f'g/pool/{name}/gy', (2, 6) + tuple(outs), -1, 1).astype(np.float32)
    xcl, gycl = x.transpose(0, 2, 3, 4, 1), gy.transpose(0, 2, 3, 4, 1)
    y, code = pool_fwd_ref(xcl, k, s, pads, outs, 0)
    assert np.array_equal(y.transpose(0, 4, 1, 2, 3), g[f'pool_{name}_y'])
    dx = pool_bwd_ref(gycl, code, xcl.shape, k, s, pads, None, None).transpose(0, 4, 1, 2, 3)
    ref = g[f'pool_{name}_dx']
    assert np.array_equal(dx != 0, ref != 0)
    assert np.allclose(dx, ref, rtol=1e-6, atol=1e-7)


def test_front_padding_of_the_padded_case():
    """(3,5,5) puts a pad cell in front of every dimension a 3-tap stride-2 window walks: n = 5 or 3, n % 2 = 1, total
    padding k - 1 = 2, one cell in front; the 2-tap windows and the (3,7,9) / (4,8,8) maps' h and w start at 0 or 1 as
    the same arithmetic says."""
    assert geometry((3, 5, 5), (3, 3, 3), (2, 2, 2))[0] == [1, 1, 1]
    assert geometry((3, 5, 5), (1, 3, 3), (1, 2, 2))[0] == [0, 1, 1]
    assert geometry((3, 5, 5), (2, 2, 2), (2, 2, 2))[0] == [0, 0, 0]
    assert geometry((3, 7, 9), (3, 3, 3), (2, 2, 2))[0] == [1, 1, 1]
    assert geometry((4, 8, 8), (3, 3, 3), (2, 2, 2))[0] == [0, 0, 0]


# ------------------------------------------------------------------ the kernels
def run_case(k, s, thw, nan, combos):
    import torch
    import ivf_lib as L
    lib = L.lib()
    pads, outs = geometry(thw, k, s)
    rng = np.random.default_rng([*k, *s, *thw, int(nan)])
    x = small_ints(rng, (B,) + thw + (C,))
    if nan:
        x[0, thw[0] // 2, thw[1] // 2, thw[2] // 2, 1] = np.nan
        x[1, 0, 0, 0, 5] = np.nan
    dy = small_ints(rng, (B,) + tuple(outs) + (C,))
    old = small_ints(rng, x.shape)

    def slab(a, ld, coff, fill):
        t = np.full(a.shape[:-1] + (ld,), fill, np.float32)
        t[..., coff:coff + C] = a
        return torch.from_numpy(t).cuda()

    xd, dyd = slab(x, IN_LD, IN_COFF, 7.0), slab(dy, OUT_LD, OUT_COFF, 7.0)
    for dead in (0, 1):
        d = L.PoolDesc()
        d.B, d.Ti, d.Hi, d.Wi, d.C, d.in_ld, d.in_coff = B, *thw, C, IN_LD, IN_COFF
        d.To, d.Ho, d.Wo, d.out_ld, d.out_coff = *outs, OUT_LD, OUT_COFF
        d.kT, d.kH, d.kW = k
        d.sT, d.sH, d.sW = s
        d.pT, d.pH, d.pW = pads
        d.gate_nonpos = dead
        y_ref, code_ref = pool_fwd_ref(x, k, s, pads, outs, dead)
        yd = torch.full((B,) + tuple(outs) + (OUT_LD,), -5.0, device='cuda')
        coded = torch.zeros((B,) + tuple(outs) + (C,), dtype=torch.uint8, device='cuda')
        L.check(lib.ivf_maxpool3d_fwd(ctypes.byref(d), L.ptr(xd), L.ptr(yd), L.ptr(coded), L.stream()))
        yh = yd.cpu().numpy()
        assert np.array_equal(yh[..., OUT_COFF:OUT_COFF + C].view(np.uint32), y_ref.view(np.uint32))
        assert np.array_equal(coded.cpu().numpy(), code_ref)
        if dead:
            assert (code_ref == 255).any(), "no dead window in this case"
        for accumulate, relu in combos:
            dxd = slab(old if accumulate else np.full(x.shape, np.nan, np.float32), IN_LD, IN_COFF, -9.0)
            L.check(lib.ivf_maxpool3d_bwd(ctypes.byref(d), L.ptr(dyd), L.ptr(coded), L.ptr(dxd),
                                          L.ptr(xd) if relu else None, accumulate, L.stream()))
            want = pool_bwd_ref(dy, code_ref, x.shape, k, s, pads, old if accumulate else None, x if relu else None)
            got = dxd.cpu().numpy()
            what = f"k={k} s={s} map={thw} dead={dead} accumulate={accumulate} relu={relu}"
            assert np.array_equal(got[..., IN_COFF:IN_COFF + C].view(np.uint32), want.view(np.uint32)), what
            # nothing outside the channel slice is written
            assert np.array_equal(np.delete(got, np.s_[IN_COFF:IN_COFF + C], axis=-1),
                                  np.full(x.shape[:-1] + (IN_LD - C,), -9.0, np.float32)), what


ALL_COMBOS = list(itertools.product((0, 1), (0, 1)))


@GPU
@pytest.mark.parametrize("thw", STRIDED_MAPS, ids=lambda m: "x".join(map(str, m)))
@pytest.mark.parametrize("k,s", STRIDED, ids=lambda v: "".join(map(str, v)))
def test_strided_pool_bwd_blocks_bit_exact(k, s, thw):
    run_case(k, s, thw, False, ALL_COMBOS)


@GPU
@pytest.mark.parametrize("k,s", STRIDED, ids=lambda v: "".join(map(str, v)))
def test_strided_pool_bwd_blocks_with_nan(k, s):
    """A NaN in the pooled tensor takes every window that sees it; the gate (NaN > 0 is false) zeroes its own cell."""
    run_case(k, s, (3, 7, 9), True, ALL_COMBOS)


@GPU
@pytest.mark.parametrize("thw", S1_MAPS, ids=lambda m: "x".join(map(str, m)))
def test_stride1_pool_bwd_bit_exact(thw):
    run_case((3, 3, 3), (1, 1, 1), thw, False, ALL_COMBOS)
    run_case((3, 3, 3), (1, 1, 1), thw, True, [(0, 0), (1, 1)])
