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

Fused forms (FUSED_RANDOM_CASES, FUSED_EXACT_CASES, FUSED_MUTANTS): what the I3D plan launches for every Inception module.
A case may have a second source (k0: channels [k0, cin) of the GEMM's K come from another buffer -- the ideal is the same
bilinear map on the concatenated channels), a second output window (n0: columns [n0, cout) go to another buffer) and
1-bit ReLU gates: form 'ep+rec' is 'ep' with the records gate_out / gate_out2 of (stored value > 0), 'acc+bits' is 'acc'
with the mask handed over as packed bits through gate_in.  expected_all() gives the whole of every buffer after the
launch, compare() is the one comparison of the GPU test and of the host's mutants.
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
_Case = namedtuple("Case", "id kind B cin cinp cout k s thw in_ld in_coff out_ld out_coff mask_ld mask_coff pattern "
                            "k0 in2_ld in2_coff n0 out2_ld out2_coff gate_ld gate_coff gate2_ld")


def same_pad(n, k, s):
    p = max(k - s, 0) if n % s == 0 else max(k - (n % s), 0)
    return p // 2, p - p // 2


def _case(id, kind, B, cin, cout, k, thw, s=(1, 1, 1), in_ld=None, in_coff=0, out_ld=None, out_coff=0, mask_ld=None,
          mask_coff=0, pattern=None, k0=0, in2_ld=None, in2_coff=0, n0=0, out2_ld=None, out2_coff=0, gate_ld=0, gate_coff=0,
          gate2_ld=0):
    """The fused forms (optional): k0 > 0 -- channels [k0, cin) of the GEMM's K come from a second source buffer (rows of
    in2_ld, window at in2_coff); n0 > 0 -- columns [n0, cout) go to a second output buffer (rows of out2_ld, window at
    out2_coff); gate_ld > 0 -- the case also runs with 1-bit ReLU gates: rows of gate_ld bytes, channel c of the window
    at bit (gate_coff + c) & 7 of byte (gate_coff + c) >> 3 (the record of `out`, or the gate an accumulating launch
    reads); the record of the second window has rows of gate2_ld bytes and sits at out2_coff, as out2 does."""
    k = (k,) * 3 if isinstance(k, int) else tuple(k)
    cinp = (cin + 3) // 4 * 4
    rows = cout if kind == "fwd" else cinp          # channels of the output window
    chan = cinp if kind == "fwd" else cout          # channels of the input window
    return _Case(id, kind, B, cin, cinp, cout, k, tuple(s), tuple(thw), in_ld or (k0 or chan), in_coff,
                 out_ld or (n0 or rows), out_coff, mask_ld or rows, mask_coff, pattern, k0, in2_ld or (chan - k0 if k0 else 0),
                 in2_coff, n0, out2_ld or (rows - n0 if n0 else 0), out2_coff, gate_ld, gate_coff, gate2_ld)


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


# The fused forms the I3D plan launches for every Inception module: two sources (the backward GEMM over
# [dY_b0 | dT_b1a dT_b2a]), two output windows (the forward b0 | b1a | b2a) and the 1-bit ReLU gates.
def _two_sources(id, k0, k1, cout=72, thw=(3, 7, 9), gate_coff=0, pattern=None):
    """Pointwise, every row buffer wider than its window."""
    return _case(id, "fwd", 2, k0 + k1, cout, 1, thw, in_ld=k0 + 8, in_coff=4, k0=k0, in2_ld=k1 + 12, in2_coff=8,
                 out_ld=cout + 4, out_coff=4, mask_ld=cout + 8, mask_coff=4, gate_ld=(gate_coff + cout + 7) // 8 + 1,
                 gate_coff=gate_coff, pattern=pattern)


def _two_windows(id, cin, n0, n1, k=1, thw=(3, 7, 9), pattern=None):
    """Both windows inside wider rows; where N0 + N1 allows records: window offsets 8, the record of `out` at 16."""
    if (n0 + n1) % 8:
        return _case(id, "fwd", 2, cin, n0 + n1, k, thw, n0=n0, out_ld=n0 + 7, out_coff=3, out2_ld=n1 + 5, out2_coff=2,
                     pattern=pattern)
    return _case(id, "fwd", 2, cin, n0 + n1, k, thw, n0=n0, out_ld=n0 + 16, out_coff=8, out2_ld=n1 + 16, out2_coff=8,
                 gate_ld=(16 + n0) // 8 + 1, gate_coff=16, gate2_ld=(n1 + 16) // 8, pattern=pattern)


FUSED_RANDOM_CASES = OrderedDict((c.id, c) for c in [
    _two_sources("F2-40+24", 40, 24, gate_coff=4),        # K0 off the 32-chunk grid
    _two_sources("F2-36+12", 36, 12, gate_coff=8),        # K0 % 8 == 4
    _two_sources("F2-32+20", 32, 20, gate_coff=4),        # K % 8 == 4: padded pack rows (mutant wrow)
    _two_sources("F2-4+32", 4, 32),                       # the smallest first source
    _two_sources("F2-96+16", 96, 16, cout=200, thw=(2, 5, 11), gate_coff=12),    # several column tiles of the wide tiles
    _two_windows("O2-24+48", 40, 24, 48),                 # N0 off the 32-column grid, % 8 == 0, both records
    _two_windows("O2-20+30", 40, 20, 30),                 # Cout % 4 != 0: the scalar epilogue's `second` branch
    _two_windows("O2-112+40", 64, 112, 40, thw=(2, 5, 11)),        # N0 past the 128-column edge of the narrow tiles
    _two_windows("O2-k3-48+24", 8, 48, 24, k=3, thw=(4, 9, 10)),   # tap-decoding tiles 0..2
    # gates on kernels with taps: every LDS-halo tile the mode admits records and reads them
    _case("G3", "fwd", 2, 24, 40, 3, (5, 9, 15), out_ld=56, out_coff=8, mask_ld=48, mask_coff=4, gate_ld=7, gate_coff=8),
])
FUSED_EXACT_CASES = OrderedDict((c.id, c) for pat in PATTERNS for c in [
    _two_sources(f"{pat}-F2-40+24", 40, 24, gate_coff=4, pattern=pat),
    _two_windows(f"{pat}-O2-24+48", 40, 24, 48, pattern=pat),
])
CASES = OrderedDict(list(RANDOM_CASES.items()) + list(EXACT_CASES.items()) + list(FUSED_RANDOM_CASES.items()) +
                    list(FUSED_EXACT_CASES.items()))


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
    whose depth-to-space output is a plain store).  The fused forms follow check_desc of csrc/conv3d.hip: a two-window
    case has no accumulate ('ep', and 'ep+rec' where its geometry admits gates), a two-source case runs 'ep', 'acc' and
    'acc+bits', a one-window case with gates all four."""
    if is_d2s(case) and mode == "bf16act":
        return ("ep",)
    if case.n0:         # (check_desc of csrc/conv3d.hip: a second window is a forward-epilogue feature)
        return ("ep", "ep+rec") if gates_ok(case) else ("ep",)
    if case.k0 or gates_ok(case):
        return ("ep", "acc") + ("ep+rec",) * (gates_ok(case) and not case.k0) + ("acc+bits",) * gates_ok(case)
    return ("ep", "acc")


def gates_ok(case):
    """A case that runs with 1-bit gates ('ep+rec': 'ep' with gate_out / gate_out2 records pre-filled with 0xAA;
    'acc+bits': 'acc' with the mask handed over as packed bits through gate_in, relu_mask NULL), and what check_desc
    asks of one: Cout % 8 == 0, 4-aligned output rows, 8-aligned record windows, a 4-aligned gate offset."""
    if not case.gate_ld:
        return False
    assert not is_d2s(case) and out_chan(case) % 8 == 0 and case.out_ld % 4 == 0 and case.out_coff % 4 == 0
    assert case.gate_coff % 4 == 0 and case.gate_coff + (case.n0 or out_chan(case)) <= 8 * case.gate_ld
    if case.n0:
        assert case.n0 % 8 == 0 and case.out2_ld % 4 == 0 and case.out2_coff % 8 == 0 and case.gate_coff % 8 == 0
        assert case.out2_coff + out_chan(case) - case.n0 <= 8 * case.gate2_ld
    return True


def base_form(form):
    return form.split("+")[0]


def windows(case):
    """name -> (first GEMM column, channel offset, channels) of every output buffer of a case."""
    rows = out_chan(case)
    w = OrderedDict(out=(0, case.out_coff, case.n0 or rows))
    if case.n0:
        w["out2"] = (case.n0, case.out2_coff, rows - case.n0)
    return w


def records(case):
    """name -> (output buffer, first bit, bytes per row) of the gate records an 'ep+rec' launch writes."""
    r = OrderedDict(rec=("out", case.gate_coff, case.gate_ld))
    if case.n0:
        r["rec2"] = ("out2", case.out2_coff, case.gate2_ld)
    return r


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
        if pat == "E4" and (case.k0 or case.n0) and r % 8 == 5:
            continue    # E4's two entries never sum to zero: the fused cases leave every eighth row empty, so that their
            #             windows hold exact zeros too (what tells a record of `> 0` from one of `>= 0`)
        for cls in _tap_classes(case):
            other = case.cin if case.kind == "fwd" else case.cout
            pick = torch.randperm(other * len(cls), generator=g)[:nnz]
            if pat == "E4":       # both entries on ONE tap (two channels), the class's nearest to the kernel centre:
                kT, kH, kW = case.k     # inside the map together, at nearly every output
                dist = [abs(f // (kH * kW) - kT // 2) + abs(f // kW % kH - kH // 2) + abs(f % kW - kW // 2) for f in cls]
                tap = dist.index(min(dist))
                pick = torch.randperm(other, generator=g)[:nnz] * len(cls) + tap
                if case.k0:         # one entry per source: the lo pass shows only if both buffers are read correctly
                    pick = torch.stack([torch.randint(0, case.k0, (), generator=g),
                                        torch.randint(case.k0, other, (), generator=g)]) * len(cls) + tap
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
    inp = {"abuf": a, "w": w, "scale": scale, "shift": shift, "base": base, "mask": mask}
    # the fused forms draw from a generator of their own (the values above are those of the unfused tables)
    g2 = _gen("conv-fused", case.id)
    if case.k0:             # 'abuf2': the second source, the same distribution as the first
        shape2 = ashape[:-1] + (case.in2_ld,)
        if not case.pattern:
            inp["abuf2"] = torch.randn(shape2, generator=g2).float().double()
        elif case.pattern == "E1":
            inp["abuf2"] = (_signs(shape2, g2) * 2.0 ** torch.randint(0, 2, shape2, generator=g2).double() *
                            (1 + 2.0 ** -10 + 2.0 ** -20))
        else:
            inp["abuf2"] = _signs(shape2, g2) * ((1 + 2.0 ** -10) if case.pattern == "E3" else 1.0)
    if case.n0:             # 'base2': what the second output buffer holds before the launch
        inp["base2"] = torch.randn(oshape + (case.out2_ld,), generator=g2).float().double()
    if case.gate_ld and not case.n0:    # 'bits' (of 'acc+bits'): the mask as packed bits, every bit outside the window random
        bits = torch.randint(0, 256, oshape + (case.gate_ld,), generator=g2).to(torch.uint8)
        inp["bits"] = pack_bits(bits, case.gate_coff, mask[..., case.mask_coff:case.mask_coff + rows] > 0)
    for name in ("abuf", "abuf2") * in_bf16(case, mode) + ("base", "base2", "mask") * out_bf16(case, mode):
        if name in inp:
            inp[name] = bf16_rne(inp[name])
    return inp


def pack_bits(rec, coff, bits):
    """`rec` [..., ld] uint8 with channel c of `bits` [..., n] at bit (coff + c) & 7 of byte (coff + c) >> 3, LSB first;
    every other bit as it was."""
    r = rec.to(torch.int32)
    for c in range(bits.shape[-1]):
        j = coff + c
        r[..., j >> 3] = (r[..., j >> 3] & ~(1 << (j & 7))) | (bits[..., c].to(torch.int32) << (j & 7))
    return r.to(torch.uint8)


def unpack_bits(rec, coff, n, mutant=None):
    """The n gate bits at channel offset coff of `rec` [..., ld] uint8, as booleans [..., n]."""
    j = torch.arange(n, device=rec.device) + (0 if mutant == "bitscoff0" else coff)
    bit = 7 - (j & 7) if mutant == "bitsmsb" else (j & 3 if mutant == "nibble" else j & 7)
    return ((rec.to(torch.int32)[..., j >> 3] >> bit) & 1).bool()


# ------------------------------------------------------------------------------------------------ the convolution
def _ncthw(buf, coff, c):
    return buf[..., coff:coff + c].permute(0, 4, 1, 2, 3)


def _rows_window(buf, ld, coff, c):
    """Channels [coff, coff + c) of every row of a channels-last buffer addressed with row length ld (its own: a plain
    slice; a mutant's: whatever lies there, zeros past the end)."""
    if ld == buf.shape[-1] and coff + c <= ld:
        return buf[..., coff:coff + c]
    m = buf.numel() // buf.shape[-1]
    idx = torch.arange(m)[:, None] * ld + coff + torch.arange(c)[None]
    flat = torch.cat([buf.reshape(-1), buf.new_zeros(max(int(idx.max()) + 1 - buf.numel(), 0))])
    return flat[idx].reshape(buf.shape[:-1] + (c,))


def act_window(case, inp, mutant=None):
    """The channels the GEMM reads, NCTHW: the input window, or the windows of both sources side by side."""
    coff = 0 if mutant == "incoff0" else case.in_coff
    if not case.k0:
        return _ncthw(inp["abuf"], coff, in_chan(case))
    K = in_chan(case)
    edge = min(-(-case.k0 // 32) * 32, K) if mutant == "k0late" else case.k0    # where the reads switch to in2
    first = _rows_window(inp["abuf"], case.in_ld, coff, edge)
    second = _rows_window(inp["abuf2"], case.in_ld if mutant == "in2ld" else case.in2_ld,
                          (0 if mutant == "in2coff0" else case.in2_coff) + edge - case.k0, K - edge)
    return torch.cat([first, second], -1).permute(0, 4, 1, 2, 3)


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
        plane = ap[pa]
        if drop is not None and (pa, pw) == tuple(drop[:2]):
            if len(drop) == 2:
                continue
            plane = plane.clone()       # (pa, pw, source): the pass is dropped on the chunks of one source only
            (plane[:, :case.k0] if drop[2] == 0 else plane[:, case.k0:]).zero_()
        t = core(case, plane, wp[pw], mutant)
        acc = t if acc is None else acc + t
    return core(case, ap[0] * 0, wp[0]) if acc is None else acc


def carried_terms(case, mode, inp):
    na, nw, terms = operand_planes(case, mode)
    a = act_window(case, inp)
    ap, wp = split_planes(a, na), split_planes(inp["w"], nw)
    return [t for t in terms if bool(ap[t[0]].abs().max() > 0) and bool(wp[t[1]].abs().max() > 0)]


def expected(case, mode, form, inp, dtype=torch.float64, mutant=None, drop=None):
    """(want, A): the whole output buffer [B, out positions, out_ld] after the launch -- the mode's result inside the
    channel window, the pre-filled values (`base` when accumulating, else SENTINEL) outside it -- and the magnitude
    every element's error is measured against (1 outside the window: any change there counts in full).  For bf16 storage
    `want` is the value BEFORE the store's rounding (exact cases: the caller rounds).  (The first buffer of
    expected_all.)"""
    return expected_all(case, mode, form, inp, dtype, mutant, drop)["out"]


def _put(buf, col0, vals):
    """vals [..., n] into channels [col0, col0 + n) of buf, as far as its rows reach."""
    n = max(min(vals.shape[-1], buf.shape[-1] - col0), 0)
    buf[..., col0:col0 + n] = vals[..., :n]


BIT_READ_MUTANTS = ("bitsmsb", "nibble", "bitscoff0")


def expected_all(case, mode, form, inp, dtype=torch.float64, mutant=None, drop=None):
    """The whole of every buffer the launch writes, by name: 'out' (and 'out2' of a two-window case) -> (want, A) as
    expected() describes them -- the second buffer is pre-filled with inp['base2'] --, 'rec' (and 'rec2') of an
    'ep+rec' launch -> the record bytes [B, out positions, gate_ld], (stored value > 0) of the window and 0xAA in every
    byte outside the window's bytes."""
    rows = out_chan(case)
    a = act_window(case, inp, mutant)
    w = inp["w"]
    v = raw = mode_sum(case, mode, a, w, dtype, mutant, drop)
    absum = core(case, a.abs(), w.abs())
    view = (1, -1, 1, 1, 1)
    bform = base_form(form)
    if bform == "ep" and not is_d2s(case):
        sc, sh = inp["scale"].to(dtype).view(view), inp["shift"].to(dtype).view(view)
        v = v * sc + sh
        if relu_on(case):
            v = torch.relu(v)
        A = absum * inp["scale"].abs().view(view) + inp["shift"].abs().view(view)
    elif bform == "ep":
        A = absum
    else:
        base = _ncthw(inp["base"], case.out_coff, rows)
        A = absum + base.abs()
        if is_d2s(case):
            v = base.to(dtype) + v
        else:
            if form == "acc+bits" and mutant in BIT_READ_MUTANTS:
                gate = unpack_bits(inp["bits"], case.gate_coff, rows, mutant).permute(0, 4, 1, 2, 3)
            else:           # (the bits of 'acc+bits' are the mask's: the same gate)
                gate = _ncthw(inp["mask"], 0 if mutant == "maskcoff0" else case.mask_coff, rows) > 0
            v = base.to(dtype) + v * gate if mutant == "maskfirst" else (base.to(dtype) + v) * gate
    vl, Al = v.permute(0, 2, 3, 4, 1).double(), A.permute(0, 2, 3, 4, 1)
    full = OrderedDict()
    for name, (col, coff, n) in windows(case).items():
        pre = inp["base" if name == "out" else "base2"]
        want = pre.clone() if bform == "acc" or name == "out2" else torch.full_like(pre, SENTINEL)
        Afull = torch.ones_like(want)
        Afull[..., coff:coff + n] = Al[..., col:col + n]
        full[name] = (want, Afull)
    # where the kernel (or the mutant) puts the columns
    n0 = case.n0 or rows
    split = min(-(-n0 // 32) * 32, rows) if mutant == "n0tile" else n0
    _put(full["out"][0], 0 if mutant == "outcoff0" else case.out_coff, vl[..., :split])
    if case.n0:
        _put(full["out2"][0], (0 if mutant == "out2coff0" else case.out2_coff) + (split if mutant == "n0col" else split - n0),
             vl[..., split:])
    if form == "ep+rec":
        val = raw if mutant == "recraw" else v
        bits = (val >= 0 if mutant == "recge" else val > 0).permute(0, 2, 3, 4, 1)
        for rname, (oname, bit0, ld) in records(case).items():
            col, _, n = windows(case)[oname]
            rec = torch.full(bits.shape[:-1] + (ld,), 0xAA, dtype=torch.uint8)
            full[rname] = pack_bits(rec, bit0, bits[..., col:col + n])
    return full


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
    """want / A of a case in a mode and form (the first output buffer; 'all': every buffer, as expected_all gives them),
    with floor and gate (random cases, over every output buffer) -- computed once and shared."""
    key = (case.id, mode, form)
    if key not in _REF:
        inp = inputs(case, mode)
        full = expected_all(case, mode, form, inp)
        r = {"inp": inp, "want": full["out"][0], "A": full["out"][1], "all": full}
        if not case.pattern:
            f32 = expected_all(case, mode, form, inp, torch.float32)
            r["floor"] = max([U] + [measure(f32[name][0], full[name][0], full[name][1]) for name in windows(case)])
            r["gate"] = GATE_MARGIN * r["floor"]
        _REF[key] = r
    return _REF[key]


def _inside(case, ref, name):
    _, coff, n = windows(case)[name]
    inside = torch.zeros_like(ref["all"][name][0], dtype=torch.bool)
    inside[..., coff:coff + n] = True
    return inside


def slack(case, mode, ref, name="out"):
    """What bf16 storage adds to a random case's per-element bound: half a bf16 ulp of the value (zeros for fp32)."""
    want = ref["all"][name][0]
    if not out_bf16(case, mode):
        return torch.zeros_like(want)
    return torch.where(_inside(case, ref, name), bf16_half_ulp(want), torch.zeros_like(want))


def tolerance(case, mode, ref, name="out"):
    """Per-element bound of a random case: gate * A inside the channel window plus slack(); 0 outside it."""
    A = ref["all"][name][1]
    return torch.where(_inside(case, ref, name), ref["gate"] * A, torch.zeros_like(A)) + slack(case, mode, ref, name)


# ------------------------------------------------------------------------------------------------ the comparison
def guarded(t, fill):
    """A buffer as the launch sees it: rows [positions, ld], with one guard row of `fill` behind the last."""
    rows = t.reshape(-1, t.shape[-1])
    return torch.cat([rows, torch.full_like(rows[:1], fill)])


def prefill(case, mode, form, inp):
    """What every buffer the launch writes holds before it (guarded): `base` when accumulating, else SENTINEL with NaN
    in the window; the second buffer inp['base2'] with NaN in its window; records 0xAA."""
    bufs = OrderedDict()
    for name, (_, coff, n) in windows(case).items():
        pre = inp["base" if name == "out" else "base2"].clone()
        if base_form(form) == "ep":
            if name == "out":
                pre.fill_(SENTINEL)
            pre[..., coff:coff + n] = float("nan")
        bufs[name] = guarded(pre, SENTINEL)
    if form == "ep+rec":
        for rname, (_, _, ld) in records(case).items():
            bufs[rname] = torch.full((bufs["out"].shape[0], ld), 0xAA, dtype=torch.uint8)
    return bufs


def targets(case, mode, form, device="cpu"):
    """What compare() holds a launch to, as guarded buffers on `device`: per output buffer 'want' (an exact case: through
    the store's rounding), and for a random case 'A', 'slack' and 'tol' (0 outside the window and on the guard row);
    per record the ideal's bytes."""
    ref = reference(case, mode, form)
    t = OrderedDict()
    for name in windows(case):
        want, A = ref["all"][name]
        e = {"want": guarded(stored(case, mode, want) if case.pattern else want, SENTINEL)}
        if not case.pattern:
            e["A"] = guarded(A, 1.0)
            e["slack"] = guarded(slack(case, mode, ref, name), 0.0)
            e["tol"] = guarded(tolerance(case, mode, ref, name), 0.0)
        t[name] = {k: x.to(device) for k, x in e.items()}
    for rname in records(case) if form == "ep+rec" else ():
        t[rname] = guarded(ref["all"][rname], 0xAA).to(device)
    return t


def as_buffers(case, full):
    """The result of expected_all (a mutant's, say) in the layout compare() takes."""
    return OrderedDict((name, guarded(x[0], SENTINEL) if name in windows(case) else guarded(x, 0xAA)) for name, x in full.items())


def worst(case, tgt, got):
    """The measured figure of a random case: max over the output buffers of measure()."""
    return max(measure(got[name], tgt[name]["want"], tgt[name]["A"], tgt[name]["slack"]) for name in windows(case))


def compare(case, mode, form, tgt, got, twin=None):
    """The one comparison of the GPU test and of the host's mutants: `got` name -> guarded buffer after the launch,
    `tgt` = targets(); `twin`: the buffers the same variant left in the 'acc' form (for 'acc+bits').  Returns the list
    of failures (empty: the launch passes).
      exact case    every buffer, records included, equals the ideal's (bf16 storage: through the store's rounding)
      random case   every element within its tolerance (0 outside the windows and on the guard rows);
                    every record byte equals (own stored value > 0) of the buffer the same launch wrote, 0xAA outside
                    the window's bytes and on the guard row; and the ideal's bit wherever |ideal| > tolerance
      'acc+bits'    bit-equal to `twin`"""
    fails = []
    for name, (_, coff, n) in windows(case).items():
        g, t = got[name].double(), tgt[name]
        if case.pattern:
            if not torch.equal(g, t["want"]):
                fails.append(f"{name}: {int((g != t['want']).sum())} of {g.numel()} values differ from the exact result")
        else:
            bad = ~((g - t["want"]).abs() <= t["tol"])
            if bool(bad.any()):
                fails.append(f"{name}: {int(bad.sum())} of {g.numel()} elements outside their tolerance, "
                             f"{int(bad[:, coff:coff + n].sum())} of them inside the window")
        if twin is not None and not torch.equal(got[name], twin[name]):
            fails.append(f"{name}: {int((got[name] != twin[name]).sum())} elements differ from the relu_mask launch")
    for rname, (oname, bit0, ld) in (records(case) if form == "ep+rec" else {}).items():
        _, coff, n = windows(case)[oname]
        r, ideal = got[rname], tgt[rname]
        own = pack_bits(torch.full_like(r, 0xAA)[:-1], bit0, got[oname][:-1, coff:coff + n] > 0)
        own = torch.cat([own, torch.full_like(r[:1], 0xAA)])
        if not torch.equal(r, own):
            fails.append(f"{rname}: {int((r != own).sum())} of {r.numel()} bytes differ from (stored value > 0) / 0xAA")
        if case.pattern:
            if not torch.equal(r, ideal):
                fails.append(f"{rname}: {int((r != ideal).sum())} of {r.numel()} bytes differ from the exact record")
        else:
            sure = tgt[oname]["want"][:-1, coff:coff + n].abs() > tgt[oname]["tol"][:-1, coff:coff + n]
            diff = (unpack_bits(r[:-1], bit0, n) != unpack_bits(ideal[:-1], bit0, n)) & sure
            if bool(diff.any()):
                fails.append(f"{rname}: {int(diff.sum())} bits differ from the ideal's where |ideal| > tolerance")
    return fails


def band_flips(case, form, tgt, got):
    """Record bits that differ from the ideal's where |ideal| <= tolerance (allowed; reported)."""
    k = 0
    for rname, (oname, bit0, _) in (records(case) if form == "ep+rec" and not case.pattern else {}).items():
        _, coff, n = windows(case)[oname]
        band = tgt[oname]["want"][:-1, coff:coff + n].abs() <= tgt[oname]["tol"][:-1, coff:coff + n]
        k += int(((unpack_bits(got[rname][:-1], bit0, n) != unpack_bits(tgt[rname][:-1], bit0, n)) & band).sum())
    return k


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
    # the fused forms
    if mutant == "k0late":          # the switch to in2 happens at the next 32-channel chunk edge
        return case.k0 % 32 != 0
    if mutant == "in2coff0":        # the second source is read at channel 0
        return case.k0 > 0 and case.in2_coff != 0
    if mutant == "in2ld":           # the second source is addressed with in_ld
        return case.k0 > 0 and case.in2_ld != case.in_ld
    if mutant == "n0col":           # the second window is written at column n, not n - N0
        return case.n0 > 0
    if mutant == "n0tile":          # the 32-column tile that contains N0 goes wholly to `out`
        return case.n0 % 32 != 0
    if mutant == "out2coff0":       # the second window is written at channel offset 0
        return case.n0 > 0 and case.out2_coff != 0
    if mutant in ("recraw", "recge"):       # the record is acc > 0 before scale and shift / is >= 0
        return form == "ep+rec"
    if mutant in ("bitsmsb", "nibble"):     # bits MSB-first in the byte / gate_in not shifted when (coff + n) & 4
        return form == "acc+bits"
    if mutant == "bitscoff0":       # the gate is read at channel offset 0
        return form == "acc+bits" and case.gate_coff != 0
    raise KeyError(mutant)


FUSED_MUTANTS = ("k0late", "in2coff0", "in2ld", "n0col", "n0tile", "out2coff0", "recraw", "recge", "bitsmsb", "nibble",
                 "bitscoff0")
BIT_MUTANTS = ("recraw", "recge")       # they change record bytes only: no distance, at least one failing byte


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


def fill_desc(d, case, math_id, in2=None, out2=None):
    """The ivf_conv3d descriptor of a case (d: an ivf_lib.ConvDesc, or anything with those fields).  in2 / out2: the
    addresses of the second source / second output buffer of a case that has one (a host-only call, which reads no
    data, takes any non-null value); the gate pointers, with their geometry, are set per form by set_form."""
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
    if case.k0:
        d.in2, d.K0, d.in2_ld, d.in2_coff = in2, case.k0, case.in2_ld, case.in2_coff
    if case.n0:
        d.out2, d.N0, d.out2_ld, d.out2_coff = out2, case.n0, case.out2_ld, case.out2_coff
    return d


def set_form(d, case, form, rec=None, rec2=None, bits=None):
    """The epilogue form of a launch: accumulate / relu, and the gate pointers (addresses) with their geometry."""
    d.accumulate = int(base_form(form) == "acc")
    d.relu = int(base_form(form) == "ep" and not is_d2s(case) and relu_on(case))
    d.gate_out = rec if form == "ep+rec" else None
    d.gate_out2 = rec2 if form == "ep+rec" and case.n0 else None
    d.gate_in = bits if form == "acc+bits" else None
    d.gate_out_ld, d.gate_out_coff, d.gate_out2_ld = case.gate_ld, case.gate_coff, case.gate2_ld
    d.gate_in_ld, d.gate_in_coff = case.gate_ld, case.gate_coff
    return d


def listed_variants(case, mode):
    """What ivf_conv3d_variants lists for the case, from variant_rule and the tile tables of csrc."""
    k, _, s = gemm_geometry(case)
    taps = k[0] * k[1] * k[2]
    bf, d2s = mode != "fp32", is_d2s(case)
    if mode == "bf16act" and is_stem(case):
        return [PIX4]
    assert not (case.n0 and is_stem(case))      # (resolve_variant refuses that pair; no case has it)
    listed = []
    for i, (_, _, bf_only, fits_x6) in enumerate(IGEMM_TILES[:8 if taps == 1 else 3]):
        if (mode == "bf16act" and d2s) or (bf_only and not bf) or (mode == "bf16x6" and not fits_x6):
            continue
        listed.append(IGEMM_BASE + i)
    if case.n0:
        return listed       # (variant_rule: a second output window is served by the implicit-GEMM tiles only)
    if bf and s == (1, 1, 1) and taps > 1 and max(k) <= 4 and in_chan(case) % 8 == 0:
        listed += [HALO_BASE + i for i in range(len(HALO_TILES))]
    if bf and is_stem(case):
        listed.append(PIX4)
    return listed


def admitted_variants(case, mode, form):
    """The listed ids that also accept the launch in this form: the LDS budgets (halo_lds_bytes for the 3x3x3 build
    rule and for the case's own kernel, launch_pix4's image) and what the pix4 kernel and a bf16act depth-to-space
    refuse -- from the tables and rules of csrc, not from return codes.  The fused forms: a second source needs the
    plain-GEMM form of the implicit GEMM in the split-bf16 modes (launch_variant); pix4 neither records nor reads 1-bit
    gates (conv_pix4_launch); the LDS-halo tiles take gate_out and gate_in as they take scale and relu_mask."""
    k, p, s = gemm_geometry(case)
    d2s, acc = is_d2s(case), base_form(form) == "acc"
    plain_gemm = k == (1, 1, 1) and s == (1, 1, 1) and p == (0, 0, 0) and not d2s and in_chan(case) >= 4
    out = []
    if mode == "bf16act" and d2s and acc:
        return out
    for v in listed_variants(case, mode):
        if v == PIX4:
            npa, npb = (3, 3) if mode == "bf16x6" else (2, 2)
            tt = 2 if mode == "bf16x6" else 4
            shm = npa * ((tt - 1) * s[0] + k[0]) * (14 + k[1]) * 24 * 8 + 3 * npb * 64 * 80
            if acc or shm > LDS_MAX or "+" in form:
                continue
        elif v >= HALO_BASE:
            npa, npb = MODE_PLANES[mode]
            tile = HALO_TILES[v - HALO_BASE]
            if halo_lds_bytes(tile, npa, npb, (3, 3, 3), False) > LDS_MAX or halo_lds_bytes(tile, npa, npb, k, d2s) > LDS_MAX:
                continue
        elif case.k0 and mode != "fp32" and not plain_gemm:
            continue
        out.append(v)
    return out
