"""Case table, seeded inputs, mode emulation, gates and mutants for the convolution-kernel tests
(test_gpu_conv_kernels.py on the GPU, test_conv_refs_host.py on the CPU).  Both iterate the tables below, so the host
test proves the references, the gates and the mutant distances on exactly the inputs the kernels are compared on.

A case is one convolution as ivf_conv3d sees it: forward ('fwd': ivf_conv3d_pack_fwd) or backward-data ('bwd':
ivf_conv3d_pack_bwd with scale NULL, so the packed values are the weights themselves), with the channel windows of its
input, output and ReLU-mask buffers.  Everything is torch float64 on the CPU, computed from the same fp32 (or
bf16-valued) numbers the kernel reads.  Nothing here needs a GPU or the HIP library.

Mode emulation.  `ideal` is the convolution the arithmetic mode is meant to compute, in fp64: the operands are cut into
the bf16 planes the kernels cut them into (round-to-nearest-even, as v_cvt_pk_bf16_f32 and torch.bfloat16 both do) and
the mode's plane products (TERMS, the order of mma_planes in csrc/conv_common.h) are summed.  A convolution is bilinear,
so each term is one fp64 convolution of an activation plane with a weight plane.

Exact cases (E1..E4).  Operands for which every product and every partial sum, in any order, is a multiple of one
power of two q and smaller than 2^24 q in magnitude: fp32 addition is then exact whatever the order, and a correct
kernel returns `ideal` bit for bit.
  E1  dense activations +-2^e (1 + 2^-10 + 2^-20), e in {0, 1} (planes h, m, l all non-zero); weights +-1 on NNZ entries
      of every packed row, 0 elsewhere
  E2  the mirror image: activations +-1, three-plane weights +-2^e (1 +- 2^-10 +- 2^-20) on NNZ entries per row
  E3  both operands +-(1 + 2^-10): the m*m, m*h and h*m terms
  E4  activations +-1, weights s (1 + 2^-10) and s' (1 - 2^-10) on TWO entries per row: where the hi parts cancel the
      result is the lo parts alone, which is what makes the lo pass visible through the bf16 store of bf16act
A term of a mode is CARRIED by a pattern when both of its planes are non-zero there; the host test shows that dropping
any carried term changes at least a quarter of the outputs, and that the patterns together carry every term of every
mode.  (HIDDEN: the one carried term the bf16 store hides.)

Random cases.  Seeded normal inputs; error measure max over elements of |got - ideal(mode)| / A with
A = sum |x||w| (times |scale|, plus |shift|, plus |base| when accumulating); floor = the same measure of a float32 CPU
evaluation of the same plane products against `ideal` (never below one fp32 rounding); gate = GATE_MARGIN * floor;
bf16 storage adds half a bf16 ulp of the stored value.

Mutants: CPU restatements of `ideal` with one defect each (MUTANTS, mutant_applies).
"""
import math
import zlib
from collections import OrderedDict, namedtuple

import torch
import torch.nn.functional as F

from clstm_refs import GATE_MARGIN
from leaf_refs import U, sum_bound  # noqa: F401  (re-exported: the host test bounds the floors with sum_bound)

MODES = ("fp32", "bf16x3", "bf16x6", "bf16act")
X3_TERMS = ((1, 0), (0, 1), (0, 0))
X6_TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
ACT_TERMS = ((0, 1), (0, 0))
SENTINEL = 7.0
MUTANT_DISTANCE = 10.0      # every mutant must sit at least this many gates away
DROP_SHARE = 0.25           # dropping a carried term must change at least this share of an exact case's outputs


# ------------------------------------------------------------------------------------------------ cases
_Case = namedtuple("Case", "id kind B cin cinp cout k s thw in_ld in_coff out_ld out_coff mask_ld mask_coff pattern")


def same_pad(n, k, s):
    p = max(k - s, 0) if n % s == 0 else max(k - (n % s), 0)
    return p // 2, p - p // 2


def _case(id, kind, B, cin, cout, k, thw, s=(1, 1, 1), in_ld=None, in_coff=0, out_ld=None, out_coff=0, mask_ld=None,
          mask_coff=0, pattern=None):
    k = (k,) * 3 if isinstance(k, int) else tuple(k)
    cinp = (cin + 3) // 4 * 4
    rows = cout if kind == "fwd" else cinp          # channels of the output window
    chan = cinp if kind == "fwd" else cout          # channels of the input window
    return _Case(id, kind, B, cin, cinp, cout, k, tuple(s), tuple(thw), in_ld or chan, in_coff, out_ld or rows, out_coff,
                 mask_ld or rows, mask_coff, pattern)


def _x4_cases():
    out = []
    for k in ((7, 7, 7), (3, 3, 3), (1, 5, 5), (5, 7, 3)):
        for s in ((2, 2, 2), (1, 2, 2)):
            for cout in (16, 6):
                out.append(_case(f"X4-k{k[0]}{k[1]}{k[2]}-s{s[0]}-n{cout}", "fwd", 2, 3, cout, k, (7, 15, 17), s=s))
    out.append(_case("X4-window", "fwd", 2, 3, 16, (3, 3, 3), (7, 15, 17), s=(2, 2, 2), out_ld=24, out_coff=4))
    return out


RANDOM_CASES = OrderedDict((c.id, c) for c in [
    # windows on a conv with taps
    _case("W3", "fwd", 2, 24, 40, 3, (5, 9, 15), in_ld=40, in_coff=8, out_ld=56, out_coff=12, mask_ld=48, mask_coff=4),
    # the scalar epilogue (Cout, out_ld, out_coff, mask_ld, mask_coff off the 4 grid)
    _case("S3-n6", "fwd", 2, 8, 6, 3, (3, 9, 10), out_ld=7, out_coff=1, mask_ld=9, mask_coff=2),
    _case("S3-n50", "fwd", 2, 16, 50, 3, (3, 9, 10), out_ld=51, out_coff=1, mask_ld=53, mask_coff=2),
    # batch 1 and an odd batch
    _case("B1", "fwd", 1, 8, 40, 3, (5, 9, 15)),
    _case("B3", "fwd", 3, 8, 40, 3, (5, 9, 15)),
    # maps smaller than any box
    _case("T1-123", "fwd", 2, 8, 32, 3, (1, 2, 3)),
    _case("T1-219", "fwd", 2, 8, 32, 3, (2, 1, 9)),
    # pointwise K tails (below one 32-deep chunk, or K % 8 == 4: padded rows, lo planes at Cout * ldw)
    _case("P4", "fwd", 2, 4, 72, 1, (3, 7, 9)),
    _case("P12", "fwd", 2, 12, 72, 1, (3, 7, 9)),
    _case("P20", "fwd", 2, 20, 72, 1, (3, 7, 9)),
    _case("P36", "fwd", 2, 36, 72, 1, (3, 7, 9)),
    # backward-data of even kernels (flipped taps, pads k-1-p != p)
    _case("R2", "bwd", 2, 8, 24, 2, (4, 9, 10)),
    _case("R4", "bwd", 2, 8, 16, 4, (4, 9, 10)),
    # non-cubic kernels
    _case("N1-133", "fwd", 2, 8, 40, (1, 3, 3), (5, 9, 15)),
    _case("N1-311", "fwd", 2, 8, 40, (3, 1, 1), (5, 9, 15)),
    _case("N1-234", "fwd", 2, 8, 40, (2, 3, 4), (5, 9, 15)),
    # stem backward with stride (1,2,2): depth-to-space with bsT = 1 and a non-cubic block kernel
    _case("D1", "bwd", 2, 3, 16, 7, (6, 12, 13), s=(1, 2, 2)),
] + _x4_cases())

PATTERNS = ("E1", "E2", "E3", "E4")
NNZ = {"E1": 4, "E2": 4, "E3": 4, "E4": 2}
# a carried term whose drop the bf16 store hides on most outputs: the lo part survives the rounding only where the hi
# parts cancel, which E2's four entries per row do too rarely; E4 is the pattern that shows this term
HIDDEN = {("E2", "bf16act"): ((0, 1),)}


def _exact_cases():
    out = []
    shapes = [("B3k3", 3, 8, 40, 3, (5, 9, 15), (1, 1, 1)), ("P12", 2, 12, 72, 1, (3, 7, 9), (1, 1, 1)),
              ("stem", 2, 3, 16, 7, (7, 15, 17), (2, 2, 2))]
    for pat in PATTERNS:
        for name, B, cin, cout, k, thw, s in shapes:
            for kind in ("fwd", "bwd"):
                out.append(_case(f"{pat}-{name}-{kind}", kind, B, cin, cout, k, thw, s=s, pattern=pat))
    return out


EXACT_CASES = OrderedDict((c.id, c) for c in _exact_cases())
CASES = OrderedDict(list(RANDOM_CASES.items()) + list(EXACT_CASES.items()))


def pads(case):
    return tuple(same_pad(n, k, s)[0] for n, k, s in zip(case.thw, case.k, case.s))


def fwd_outs(case):
    return tuple(-(-n // s) for n, s in zip(case.thw, case.s))


def is_d2s(case):
    return case.kind == "bwd" and case.s != (1, 1, 1)


def in_pos(case):
    """Positions of the buffer the kernel reads: the clip (fwd) or the forward output map (bwd)."""
    return case.thw if case.kind == "fwd" else fwd_outs(case)


def out_pos(case):
    return fwd_outs(case) if case.kind == "fwd" else case.thw


def in_chan(case):
    return case.cinp if case.kind == "fwd" else case.cout


def out_chan(case):
    return case.cout if case.kind == "fwd" else case.cinp


def is_stem(case):
    """The shape conv_pix4_supported admits (before its accumulate / mask conditions)."""
    return (case.kind == "fwd" and case.cinp == 4 and case.in_ld == 4 and case.in_coff == 0 and case.s[1] == 2 and
            case.s[2] == 2 and case.s[0] in (1, 2) and max(case.k) <= 7)


def in_bf16(case, mode):
    return mode == "bf16act" and not is_stem(case)      # (the 4-channel-pixel strided conv reads fp32 pixels)


def out_bf16(case, mode):
    return mode == "bf16act" and not is_d2s(case)       # (a depth-to-space backward writes fp32)


def forms(case, mode):
    """Epilogue forms a case runs in: 'ep' scale + shift + ReLU (depth-to-space: the plain store, which is all its
    epilogue has besides accumulate), 'acc' accumulate + ReLU mask (depth-to-space: accumulate alone; not with bf16act,
    whose depth-to-space output is a plain store)."""
    if is_d2s(case) and mode == "bf16act":
        return ("ep",)
    return ("ep", "acc")


def relu_on(case):
    """ReLU in the 'ep' form: the random cases.  An exact case keeps both signs, so that a dropped term shows on every
    output it reaches (scale a power of two, shift 0)."""
    return not case.pattern


def exact_applies(case, mode):
    """bf16 storage reads bf16-valued activations: the patterns whose activations are +-1."""
    return mode != "bf16act" or case.pattern in ("E2", "E4")


def operand_planes(case, mode):
    """(activation planes, weight planes, terms) of the kernels that serve the case in the mode."""
    if mode == "fp32":
        return 1, 1, ((0, 0),)
    if mode == "bf16x6":
        return 3, 3, X6_TERMS
    if mode == "bf16x3" or is_stem(case):
        return 2, 2, X3_TERMS
    return 1, 2, ACT_TERMS


# ------------------------------------------------------------------------------------------------ bf16 planes
def bf16_rne(t):
    return t.float().bfloat16().to(t.dtype)


def bf16_half_ulp(t):
    """Half the spacing of bf16 (8 significant bits) at each element: 2^(floor(log2 |t|) - 8); 0 at 0."""
    _, ex = torch.frexp(t)                       # |t| = m 2^ex, m in [0.5, 1)
    return torch.where(t == 0, torch.zeros_like(t), torch.ldexp(torch.ones_like(t), ex - 9))


def split_planes(t, n):
    """The kernels' split of fp32 values into n bf16 planes (split4 / split4x3 / store_packed): every plane is the RNE
    of what the planes before it left over; the residuals are exact in fp32."""
    if n == 1:
        return [t]
    out, rest = [], t
    for _ in range(n):
        p = bf16_rne(rest)
        out.append(p)
        rest = rest - p
    return out


# ------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def _signs(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def _tap_classes(case):
    """Flat tap indices by stride residue: one output of a backward-data conv meets the taps of one class only."""
    cls = OrderedDict()
    kT, kH, kW = case.k
    for t in range(kT):
        for h in range(kH):
            for w in range(kW):
                key = (t % case.s[0], h % case.s[1], w % case.s[2]) if case.kind == "bwd" else 0
                cls.setdefault(key, []).append((t * kH + h) * kW + w)
    return list(cls.values())


def _exact_weights(case, g):
    """w_ref [cout, cin, taps] with NNZ pattern entries on every packed row (fwd: per output channel; bwd: per input
    channel and tap class) and zeros elsewhere."""
    pat, nnz = case.pattern, NNZ[case.pattern]
    taps = case.k[0] * case.k[1] * case.k[2]
    w = torch.zeros(case.cout, case.cin, taps, dtype=torch.float64)
    rows = case.cout if case.kind == "fwd" else case.cin
    for r in range(rows):
        for cls in _tap_classes(case):
            other = case.cin if case.kind == "fwd" else case.cout
            pick = torch.randperm(other * len(cls), generator=g)[:nnz]
            if pat == "E4":       # both entries on ONE tap (two channels), the class's nearest to the kernel centre:
                kT, kH, kW = case.k     # inside the map together, at nearly every output
                dist = [abs(f // (kH * kW) - kT // 2) + abs(f // kW % kH - kH // 2) + abs(f % kW - kW // 2) for f in cls]
                tap = dist.index(min(dist))
                pick = torch.randperm(other, generator=g)[:nnz] * len(cls) + tap
            s = _signs((nnz,), g)
            e = torch.randint(0, 2, (nnz,), generator=g).double()
            t2, t3 = _signs((nnz,), g), _signs((nnz,), g)
            for j, p in enumerate(pick.tolist()):
                o, tap = p // len(cls), cls[p % len(cls)]
                if pat == "E1":
                    v = s[j]
                elif pat == "E2":
                    v = s[j] * 2.0 ** e[j] * (1 + t2[j] * 2.0 ** -10 + t3[j] * 2.0 ** -20)
                elif pat == "E3":
                    v = s[j] * (1 + 2.0 ** -10)
                else:
                    v = s[j] * (1 + (1 if j == 0 else -1) * 2.0 ** -10)
                if case.kind == "fwd":
                    w[r, o, tap] = v
                else:
                    w[o, r, tap] = v
    return w.view(case.cout, case.cin, *case.k)


def inputs(case, mode):
    """Seeded fp32-valued float64 tensors of a case in a mode (bf16 storage: bf16-valued), channels-last buffers as the
    kernel sees them, filled OUTSIDE the windows too: abuf [B, in positions, in_ld], w [cout, cin, k], scale / shift
    [rows], base [B, out positions, out_ld], mask [B, out positions, mask_ld]."""
    g = _gen("conv", case.id)
    B, rows = case.B, out_chan(case)
    ashape = (B,) + in_pos(case) + (case.in_ld,)
    oshape = (B,) + out_pos(case)
    if case.pattern:
        if case.pattern == "E1":
            a = _signs(ashape, g) * 2.0 ** torch.randint(0, 2, ashape, generator=g).double() * (1 + 2.0 ** -10 + 2.0 ** -20)
        elif case.pattern == "E3":
            a = _signs(ashape, g) * (1 + 2.0 ** -10)
        else:
            a = _signs(ashape, g)
        w = _exact_weights(case, g)
        scale = 2.0 ** torch.randint(-1, 2, (rows,), generator=g).double()
        shift = torch.zeros(rows, dtype=torch.float64)
        # (bf16-valued, and small enough that a cancelled hi sum leaves the lo sum visible through a bf16 store)
        base = torch.randint(-2, 3, oshape + (case.out_ld,), generator=g).double() * 2.0 ** -9
        mask = (torch.rand(oshape + (case.mask_ld,), generator=g) > 0.2).double()
    else:
        a = torch.randn(ashape, generator=g).float().double()
        w = (torch.randn((case.cout, case.cin) + case.k, generator=g) * 0.1).float().double()
        scale = (torch.rand(rows, generator=g) + 0.5).float().double() * _signs((rows,), g)
        shift = (torch.randn(rows, generator=g) * 0.1).float().double()
        base = torch.randn(oshape + (case.out_ld,), generator=g).float().double()
        mask = torch.relu(torch.randn(oshape + (case.mask_ld,), generator=g) + 0.5).float().double()
    if in_bf16(case, mode):
        a = bf16_rne(a)
    if out_bf16(case, mode):
        base, mask = bf16_rne(base), bf16_rne(mask)
    return {"abuf": a, "w": w, "scale": scale, "shift": shift, "base": base, "mask": mask}


# ------------------------------------------------------------------------------------------------ the convolution
def _ncthw(buf, coff, c):
    return buf[..., coff:coff + c].permute(0, 4, 1, 2, 3)


def conv_direct(a, w, s, pf, outs):
    """out[b, n, o] = sum_{c, k} a[b, c, o s - pf + k] w[n, c, k] on `outs` output positions, zeros outside the map."""
    pb = [max((o - 1) * st + k - n - p, 0) for o, st, k, n, p in zip(outs, s, w.shape[2:], a.shape[2:], pf)]
    ap = F.pad(a, (pf[2], pb[2], pf[1], pb[1], pf[0], pb[0]))
    return F.conv3d(ap, w, stride=s)[:, :, :outs[0], :outs[1], :outs[2]]


def bwd_direct_weights(w, flip=True):
    """Backward-data of a stride-1 conv as a conv over dY: Wb[ci][co][tap] = W[co][ci][flipped tap]."""
    return (w.flip(2, 3, 4) if flip else w).transpose(0, 1).contiguous()


def core(case, a, w, mutant=None):
    """The bilinear map of a case: a [B, in channels, in positions] (NCTHW), w [cout, cin, k] -> [B, rows, out
    positions].  Backward-data is the transposed convolution cropped by the forward front pads, i.e. what autograd
    gives; `flipped` / the mutants use the direct form the kernels are handed (flipped taps, pads k-1-p)."""
    p = pads(case)
    if mutant == "batch":
        a = torch.cat([a[:1], a[:-1]], 0)
    if mutant == "tapw":                                  # the centre tap reads one pixel further right
        c = tuple(k // 2 for k in case.k)
        w1 = torch.zeros_like(w)
        w1[..., c[0], c[1], c[2]] = w[..., c[0], c[1], c[2]]
        shifted = torch.cat([a[..., 1:], torch.zeros_like(a[..., :1])], -1)
        return core(case, a, w - w1) + core(case, shifted, w1)
    if case.kind == "fwd":
        wp = F.pad(w, (0, 0, 0, 0, 0, 0, 0, case.cinp - case.cin))
        return conv_direct(a, wp, case.s, p, fwd_outs(case))
    if mutant in ("flipped", "noflip", "bwdpad"):
        assert case.s == (1, 1, 1)
        pb = p if mutant == "bwdpad" else tuple(k - 1 - q for k, q in zip(case.k, p))
        out = conv_direct(a, bwd_direct_weights(w, flip=mutant != "noflip"), case.s, pb, case.thw)
    else:
        full = F.conv_transpose3d(a, w, stride=case.s)
        out = full[:, :, p[0]:p[0] + case.thw[0], p[1]:p[1] + case.thw[1], p[2]:p[2] + case.thw[2]]
    return F.pad(out, (0, 0, 0, 0, 0, 0, 0, case.cinp - case.cin))


def mode_sum(case, mode, a, w, dtype=torch.float64, mutant=None, drop=None):
    """Sum of the mode's plane products in the kernels' order (float64: `ideal`; float32: the floor's evaluation)."""
    na, nw, terms = operand_planes(case, mode)
    ap = [t.to(dtype) for t in split_planes(a, na)]
    wp = [t.to(dtype) for t in split_planes(w, nw)]
    if mutant == "wrow" and nw > 1:           # the plane at w_lo_off read one packed row off
        wp[1] = torch.roll(wp[1], 1, 0 if case.kind == "fwd" else 1)
    acc = None
    for pa, pw in terms:
        if (pa, pw) == drop:
            continue
        t = core(case, ap[pa], wp[pw], mutant)
        acc = t if acc is None else acc + t
    return core(case, ap[0] * 0, wp[0]) if acc is None else acc


def carried_terms(case, mode, inp):
    na, nw, terms = operand_planes(case, mode)
    a = _ncthw(inp["abuf"], case.in_coff, in_chan(case))
    ap, wp = split_planes(a, na), split_planes(inp["w"], nw)
    return [t for t in terms if bool(ap[t[0]].abs().max() > 0) and bool(wp[t[1]].abs().max() > 0)]


def expected(case, mode, form, inp, dtype=torch.float64, mutant=None, drop=None):
    """(want, A): the whole output buffer [B, out positions, out_ld] after the launch -- the mode's result inside the
    channel window, the pre-filled values (`base` when accumulating, else SENTINEL) outside it -- and the magnitude
    every element's error is measured against (1 outside the window: any change there counts in full).  For bf16 storage
    `want` is the value BEFORE the store's rounding (exact cases: the caller rounds)."""
    cin_w, rows = in_chan(case), out_chan(case)
    a = _ncthw(inp["abuf"], 0 if mutant == "incoff0" else case.in_coff, cin_w)
    w = inp["w"]
    v = mode_sum(case, mode, a, w, dtype, mutant, drop)
    absum = core(case, a.abs(), w.abs())
    view = (1, -1, 1, 1, 1)
    if form == "ep" and not is_d2s(case):
        sc, sh = inp["scale"].to(dtype).view(view), inp["shift"].to(dtype).view(view)
        v = v * sc + sh
        if relu_on(case):
            v = torch.relu(v)
        A = absum * inp["scale"].abs().view(view) + inp["shift"].abs().view(view)
    elif form == "ep":
        A = absum
    else:
        base = _ncthw(inp["base"], case.out_coff, rows)
        A = absum + base.abs()
        if is_d2s(case):
            v = base.to(dtype) + v
        else:
            gate = _ncthw(inp["mask"], 0 if mutant == "maskcoff0" else case.mask_coff, rows) > 0
            v = base.to(dtype) + v * gate if mutant == "maskfirst" else (base.to(dtype) + v) * gate
    want = inp["base"].clone() if form == "acc" else torch.full_like(inp["base"], SENTINEL)
    Afull = torch.ones_like(want)
    coff = 0 if mutant == "outcoff0" else case.out_coff
    want[..., coff:coff + rows] = v.permute(0, 2, 3, 4, 1).double()
    Afull[..., case.out_coff:case.out_coff + rows] = A.permute(0, 2, 3, 4, 1)
    return want, Afull


def measure(got, want, A, slack=None):
    """max over elements of |got - want| / A (0 / 0 = 0; NaN or a difference at A = 0 gives inf).  `slack`: a
    per-element allowance taken off the difference first (the bf16 half ulp of bf16 storage)."""
    d = (got.double() - want).abs()
    d = torch.where(torch.isnan(d), d, (d - slack).clamp(min=0)) if slack is not None else d
    e = torch.where(d == 0, torch.zeros_like(d), d / A)
    return float(torch.nan_to_num(e, nan=math.inf, posinf=math.inf).max())


def n_terms(case, mode):
    taps = case.k[0] * case.k[1] * case.k[2]
    return taps * in_chan(case) * len(operand_planes(case, mode)[2]) + 3      # + scale, shift, base


_REF = {}


def reference(case, mode, form):
    """want / A of a case in a mode and form, with floor and gate (random cases) -- computed once and shared."""
    key = (case.id, mode, form)
    if key not in _REF:
        inp = inputs(case, mode)
        want, A = expected(case, mode, form, inp)
        r = {"inp": inp, "want": want, "A": A}
        if not case.pattern:
            w32, _ = expected(case, mode, form, inp, torch.float32)
            r["floor"] = max(U, measure(w32, want, A))
            r["gate"] = GATE_MARGIN * r["floor"]
        _REF[key] = r
    return _REF[key]


def slack(case, mode, ref):
    """What bf16 storage adds to a random case's per-element bound: half a bf16 ulp of the value (zeros for fp32)."""
    if not out_bf16(case, mode):
        return torch.zeros_like(ref["want"])
    inside = torch.zeros_like(ref["want"], dtype=torch.bool)
    inside[..., case.out_coff:case.out_coff + out_chan(case)] = True
    return torch.where(inside, bf16_half_ulp(ref["want"]), torch.zeros_like(ref["want"]))


def tolerance(case, mode, ref):
    """Per-element bound of a random case: gate * A inside the channel window plus slack(); 0 outside it."""
    inside = torch.zeros_like(ref["want"], dtype=torch.bool)
    inside[..., case.out_coff:case.out_coff + out_chan(case)] = True
    return torch.where(inside, ref["gate"] * ref["A"], torch.zeros_like(ref["A"])) + slack(case, mode, ref)


def stored(case, mode, want):
    """What an exact case's buffer holds after the launch: `want` through the store's rounding."""
    return bf16_rne(want) if out_bf16(case, mode) else want


def lowest_bit(t):
    """The largest power of two that divides every element of t (t != 0 somewhere)."""
    q = 2.0 ** -60
    while bool(((t / (2 * q)) == (t / (2 * q)).round()).all()):
        q *= 2
    return q


# ------------------------------------------------------------------------------------------------ mutants
MUTANTS = ("tapw", "noflip", "bwdpad", "incoff0", "outcoff0", "maskcoff0", "batch", "maskfirst", "wrow")


def mutant_applies(case, mutant, mode, form):
    taps = case.k[0] * case.k[1] * case.k[2]
    s1bwd = case.kind == "bwd" and not is_d2s(case)
    if mutant == "tapw":
        return case.k[2] > 1
    if mutant == "noflip":
        return s1bwd and taps > 1
    if mutant == "bwdpad":
        return s1bwd and any(k % 2 == 0 for k in case.k)
    if mutant == "incoff0":
        return case.in_coff != 0
    if mutant == "outcoff0":
        return case.out_coff != 0
    if mutant == "maskcoff0":
        return case.mask_coff != 0 and form == "acc" and not is_d2s(case)
    if mutant == "batch":
        return case.B >= 2
    if mutant == "maskfirst":
        return form == "acc" and not is_d2s(case)
    if mutant == "wrow":
        return case.kind == "fwd" and (taps * case.cinp) % 8 == 4 and mode != "fp32"
    raise KeyError(mutant)


# ------------------------------------------------------------------------------------------------ dispatch tables
# kIgemmTiles (csrc/conv3d.hip): (BM, BN, split-bf16 only, fits the LDS with three operand planes)
IGEMM_TILES = [(128, 128, False, True), (128, 64, False, True), (128, 32, False, True), (128, 256, True, False),
               (128, 192, True, False), (128, 160, True, False), (64, 64, True, True), (64, 128, True, True)]
# kHaloTiles (csrc/conv3d_halo_impl.h): (TT, BN, WROWS, WCOLS, KS, BKH, TH, TW, TPS, DMA)
HALO_TILES = [
    (4, 192, 32, 96, 1, 32, 8, 8, 1, 0), (4, 128, 64, 64, 1, 32, 8, 8, 1, 0), (4, 128, 32, 64, 1, 32, 8, 8, 1, 0),
    (4, 96, 32, 96, 1, 32, 8, 8, 1, 0), (4, 64, 32, 64, 1, 32, 8, 8, 1, 0), (4, 64, 64, 64, 2, 32, 8, 8, 1, 0),
    (4, 32, 32, 32, 1, 32, 8, 8, 1, 0), (4, 32, 64, 32, 2, 32, 8, 8, 1, 0), (2, 192, 32, 96, 1, 32, 8, 8, 1, 0),
    (2, 128, 32, 64, 1, 32, 8, 8, 1, 0), (2, 96, 32, 96, 1, 32, 8, 8, 1, 0), (2, 64, 32, 64, 1, 32, 8, 8, 1, 0),
    (2, 32, 32, 32, 1, 32, 8, 8, 1, 0), (2, 64, 64, 64, 2, 32, 8, 8, 1, 0), (2, 128, 64, 64, 1, 32, 8, 8, 1, 0),
    (4, 64, 32, 64, 2, 32, 8, 8, 1, 0), (4, 96, 32, 96, 2, 32, 8, 8, 1, 0), (4, 32, 32, 32, 2, 32, 8, 8, 1, 0),
    (2, 192, 32, 96, 1, 16, 8, 8, 1, 0), (2, 128, 32, 64, 1, 16, 8, 8, 1, 0), (4, 96, 32, 96, 1, 16, 8, 8, 1, 0),
    (4, 64, 32, 64, 1, 16, 8, 8, 1, 0), (2, 96, 32, 96, 1, 16, 8, 8, 1, 0),
    (4, 192, 32, 96, 1, 32, 4, 14, 1, 0), (4, 128, 32, 64, 1, 32, 4, 14, 1, 0), (4, 96, 32, 96, 1, 32, 4, 14, 1, 0),
    (4, 64, 32, 64, 1, 32, 4, 14, 1, 0), (4, 32, 32, 32, 1, 32, 4, 14, 1, 0), (4, 64, 32, 32, 1, 32, 4, 14, 1, 0),
    (4, 32, 32, 32, 2, 32, 4, 14, 1, 0), (4, 128, 32, 128, 1, 32, 4, 14, 1, 0),
    (2, 32, 64, 32, 2, 16, 8, 8, 1, 0), (2, 32, 32, 32, 2, 16, 8, 8, 1, 0), (2, 32, 32, 32, 1, 16, 8, 8, 1, 0),
    (2, 64, 32, 64, 2, 16, 8, 8, 1, 0), (2, 64, 64, 64, 2, 16, 8, 8, 1, 0), (4, 32, 64, 32, 2, 16, 8, 8, 1, 0),
    (4, 32, 32, 32, 2, 16, 8, 8, 1, 0),
    (4, 32, 32, 32, 2, 16, 8, 8, 4, 0), (4, 32, 64, 32, 2, 16, 8, 8, 4, 0), (4, 32, 32, 32, 2, 16, 8, 8, 2, 0),
    (2, 32, 32, 32, 2, 32, 8, 8, 2, 0), (4, 64, 32, 64, 1, 16, 8, 8, 2, 0), (4, 64, 32, 64, 1, 32, 8, 8, 2, 0),
    (4, 32, 32, 32, 1, 16, 8, 8, 4, 0), (4, 96, 32, 96, 1, 16, 8, 8, 2, 0), (4, 32, 32, 32, 2, 32, 8, 8, 2, 0),
    (4, 64, 32, 64, 1, 32, 4, 14, 2, 0),
    (4, 192, 32, 96, 1, 32, 7, 8, 1, 0), (4, 128, 32, 64, 1, 32, 7, 8, 1, 0), (4, 96, 32, 96, 1, 16, 7, 8, 1, 0),
    (4, 64, 32, 64, 1, 16, 7, 8, 1, 0),
    (4, 192, 32, 96, 1, 32, 8, 8, 1, 1), (4, 192, 32, 96, 1, 32, 4, 14, 1, 1), (4, 128, 32, 64, 1, 32, 4, 14, 1, 1),
    (4, 128, 32, 64, 1, 32, 8, 8, 1, 1), (4, 32, 32, 32, 2, 32, 8, 8, 1, 1), (4, 128, 32, 64, 1, 32, 7, 8, 1, 1),
    (4, 96, 32, 96, 1, 32, 8, 8, 1, 1), (4, 64, 32, 64, 1, 32, 8, 8, 1, 1),
    (4, 192, 32, 96, 1, 16, 8, 8, 1, 0), (4, 128, 32, 64, 1, 16, 8, 8, 1, 0), (4, 192, 32, 96, 1, 16, 4, 14, 1, 0),
    (4, 128, 32, 64, 1, 16, 4, 14, 1, 0), (4, 96, 32, 96, 1, 16, 4, 14, 1, 0), (4, 64, 32, 64, 1, 16, 4, 14, 1, 0),
    (4, 192, 32, 96, 1, 16, 7, 8, 1, 0), (4, 128, 32, 64, 1, 16, 7, 8, 1, 0),
    (4, 192, 64, 96, 1, 16, 8, 8, 1, 0), (4, 128, 64, 64, 1, 16, 8, 8, 1, 0),
]
IGEMM_BASE, PIX4, HALO_BASE = 1, 15, 16       # IVF_CONV_* (include/ivf_hip.h)
LDS_MAX = 160 * 1024
MODE_PLANES = {"bf16x3": (2, 2), "bf16act": (1, 2), "bf16x6": (3, 3)}      # OpPlanes<AM>: (A, B)


def halo_lds_bytes(tile, npa, npb, k, d2s):
    """halo_lds_bytes of csrc/conv3d_halo_impl.h."""
    TT, BN, _, _, KS, BKH, TH, TW, TPS, DMA = tile
    rowb = (BKH + 8) * 2
    rowb_b = BKH * 2 if DMA else rowb
    ps = (TH + k[1] - 1) * (TW + k[2] - 1)
    if TT == 4 and TW == 8:
        ps += (4 - ps % 8 + 8) % 8
    hr = (TT + k[0] - 1) * ps
    shm = npa * hr * rowb + 2 * TPS * KS * npb * BN * rowb_b + hr * 4
    if KS == 2:
        shm = max(shm, TT * TH * TW * BN * 4)
    if d2s:
        shm = max(shm, 2 * TT * 256 * 4 * 4)
    return shm


def bwd_span(k, s, p):
    """Extent and front offset of the backward conv along one dim (bwd_span of csrc/conv3d.hip)."""
    if s == 1:
        return k, k - 1 - p
    lo = p - (k - 1)
    dlo = (lo + s - 1) // s if lo >= 0 else -((-lo) // s)
    dhi = (s - 1 + p) // s
    return dhi - dlo + 1, -dlo


def gemm_geometry(case):
    """Kernel extents, front pads and strides of the convolution ivf_conv3d is handed."""
    if case.kind == "fwd":
        return case.k, pads(case), case.s
    spans = [bwd_span(k, s, p) for k, s, p in zip(case.k, case.s, pads(case))]
    return tuple(sp[0] for sp in spans), tuple(sp[1] for sp in spans), (1, 1, 1)


def fill_desc(d, case, math_id):
    """The ivf_conv3d descriptor of a case (d: an ivf_lib.ConvDesc, or anything with those fields)."""
    k, p, s = gemm_geometry(case)
    d.B = case.B
    d.Ti, d.Hi, d.Wi = in_pos(case)
    d.Cin, d.in_ld, d.in_coff = in_chan(case), case.in_ld, case.in_coff
    d.kT, d.kH, d.kW = k
    d.sT, d.sH, d.sW = s
    d.pT, d.pH, d.pW = p
    d.out_ld, d.out_coff = case.out_ld, case.out_coff
    d.mask_ld, d.mask_coff = case.mask_ld, case.mask_coff
    d.math = math_id
    if is_d2s(case):
        d.d2s = 1
        d.bsT, d.bsH, d.bsW = case.s
        d.To, d.Ho, d.Wo = fwd_outs(case)
        d.Cout = 8 * case.cinp
        d.dT, d.dH, d.dW = case.thw
        d.dC = case.cinp
    else:
        d.To, d.Ho, d.Wo = out_pos(case)
        d.Cout = out_chan(case)
    return d


def listed_variants(case, mode):
    """What ivf_conv3d_variants lists for the case, from variant_rule and the tile tables of csrc."""
    k, _, s = gemm_geometry(case)
    taps = k[0] * k[1] * k[2]
    bf, d2s = mode != "fp32", is_d2s(case)
    if mode == "bf16act" and is_stem(case):
        return [PIX4]
    listed = []
    for i, (_, _, bf_only, fits_x6) in enumerate(IGEMM_TILES[:8 if taps == 1 else 3]):
        if (mode == "bf16act" and d2s) or (bf_only and not bf) or (mode == "bf16x6" and not fits_x6):
            continue
        listed.append(IGEMM_BASE + i)
    if bf and s == (1, 1, 1) and taps > 1 and max(k) <= 4 and in_chan(case) % 8 == 0:
        listed += [HALO_BASE + i for i in range(len(HALO_TILES))]
    if bf and is_stem(case):
        listed.append(PIX4)
    return listed


def admitted_variants(case, mode, form):
    """The listed ids that also accept the launch in this form: the LDS budgets (halo_lds_bytes for the 3x3x3 build
    rule and for the case's own kernel, launch_pix4's image) and what the pix4 kernel and a bf16act depth-to-space
    refuse -- from the tables and rules of csrc, not from return codes."""
    k, _, s = gemm_geometry(case)
    d2s, acc = is_d2s(case), form == "acc"
    out = []
    if mode == "bf16act" and d2s and acc:
        return out
    for v in listed_variants(case, mode):
        if v == PIX4:
            npa, npb = (3, 3) if mode == "bf16x6" else (2, 2)
            tt = 2 if mode == "bf16x6" else 4
            shm = npa * ((tt - 1) * s[0] + k[0]) * (14 + k[1]) * 24 * 8 + 3 * npb * 64 * 80
            if acc or shm > LDS_MAX:
                continue
        elif v >= HALO_BASE:
            npa, npb = MODE_PLANES[mode]
            tile = HALO_TILES[v - HALO_BASE]
            if halo_lds_bytes(tile, npa, npb, (3, 3, 3), False) > LDS_MAX or halo_lds_bytes(tile, npa, npb, k, d2s) > LDS_MAX:
                continue
        out.append(v)
    return out
