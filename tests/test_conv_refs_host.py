"""CPU: what tests/conv_refs.py claims, proved on exactly the inputs test_gpu_conv_kernels.py runs -- the exact cases'
representability condition and how many outputs every dropped MFMA pass changes, the planes of the emulation, the
floors against the a-priori bound, the distance of every mutant from the gate, backward-data as a flipped-tap
convolution against fp64 autograd, and the restated dispatch tables against csrc and ivf_conv3d_variants."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_refs as R
from conftest import PKG, note

EXACT = list(R.EXACT_CASES)
RANDOM = list(R.RANDOM_CASES)


def _window(case, t):
    return t[..., case.out_coff:case.out_coff + R.out_chan(case)]


# ------------------------------------------------------------------------------------------------ emulation
@pytest.mark.parametrize("cid", list(R.CASES))
def test_planes_reconstruct_the_operands(cid):
    """The 3-way split carries all 24 bits: its planes sum back to the operand exactly; every plane is a bf16 value;
    the 2-way split leaves at most 2^-16 of the operand; bf16 storage reads bf16 values."""
    case = R.CASES[cid]
    inp = R.inputs(case, "bf16x6")
    for t in (inp["abuf"], inp["w"]):
        assert torch.equal(t, t.float().double())
        p3 = R.split_planes(t, 3)
        assert torch.equal(p3[0] + p3[1] + p3[2], t)
        assert all(torch.equal(p, R.bf16_rne(p)) for p in p3)
        p2 = R.split_planes(t, 2)
        assert bool(((t - p2[0] - p2[1]).abs() <= 2.0 ** -16 * t.abs()).all())
    act = R.inputs(case, "bf16act")
    for name in ("abuf",) * R.in_bf16(case, "bf16act") + ("base", "mask") * R.out_bf16(case, "bf16act"):
        assert torch.equal(act[name], R.bf16_rne(act[name])), name


@pytest.mark.parametrize("cid", EXACT)
def test_exact_cases_are_exact_and_show_every_pass(cid):
    """Per mode and form: every product is a multiple of q and sum |product| (+ |base|) < 2^24 q at every output, so
    any fp32 summation order is exact; `ideal` survives fp32 (and a float32 CPU evaluation returns it bit for bit);
    leaving out any one carried term changes at least DROP_SHARE of the outputs."""
    case = R.CASES[cid]
    for mode in R.MODES:
        if not R.exact_applies(case, mode):
            continue
        inp = R.inputs(case, mode)
        a = inp["abuf"][..., case.in_coff:case.in_coff + R.in_chan(case)]
        q = min(R.lowest_bit(a) * R.lowest_bit(inp["w"]), R.lowest_bit(inp["base"]))
        for form in R.forms(case, mode):
            ref = R.reference(case, mode, form)
            want = ref["want"]
            _, A = R.expected(case, mode, "acc", inp)        # sum |x||w| + |base|, before any scale
            assert float(_window(case, A).max()) < 2.0 ** 24 * q, (mode, form)
            assert float(inp["scale"].abs().max()) <= 2 and torch.equal(inp["scale"], 2.0 ** torch.log2(inp["scale"]).round())
            assert torch.equal(want.float().double(), want), (mode, form)
            w32, _ = R.expected(case, mode, form, inp, torch.float32)
            assert torch.equal(w32, want), (mode, form)
            got = _window(case, R.stored(case, mode, want))
            for term in R.carried_terms(case, mode, inp):
                dropped, _ = R.expected(case, mode, form, inp, drop=term)
                share = float((_window(case, R.stored(case, mode, dropped)) != got).double().mean())
                hidden = term in R.HIDDEN.get((case.pattern, mode), ())
                note(f"conv exact {cid} {mode} {form}: dropping term a{term[0]}*w{term[1]} changes {share:.1%} of the outputs"
                     + (" (hidden by the bf16 store; shown by E4)" if hidden else ""))
                if not hidden:
                    assert share >= R.DROP_SHARE, (mode, form, term)


@pytest.mark.parametrize("mode", R.MODES)
def test_patterns_carry_every_term_of_the_mode(mode):
    """Per shape and direction, the exact patterns together show every MFMA pass of the kernels that serve it."""
    shown, terms = {}, {}
    for case in R.EXACT_CASES.values():
        if not R.exact_applies(case, mode):
            continue
        shape = case.id.split("-", 1)[1]
        hidden = R.HIDDEN.get((case.pattern, mode), ())
        shown.setdefault(shape, set()).update(t for t in R.carried_terms(case, mode, R.inputs(case, mode)) if t not in hidden)
        terms[shape] = set(R.operand_planes(case, mode)[2])
    assert len(terms) == 6
    for shape, want in terms.items():
        if mode == "bf16act" and shape == "stem-fwd":
            want = {t for t in want if t[0] == 0}       # fp32 pixels that are +-1: their lo plane is empty (bf16x3 shows it)
        assert shown[shape] == want, (shape, shown[shape], want)


# ------------------------------------------------------------------------------------------------ gates and mutants
@pytest.mark.parametrize("cid", RANDOM)
def test_floors_are_bounded_and_mutants_leave_the_gate(cid):
    case = R.CASES[cid]
    for mode in R.MODES:
        for form in R.forms(case, mode):
            ref = R.reference(case, mode, form)
            assert ref["floor"] <= R.sum_bound(1.0, R.n_terms(case, mode)), (mode, form, ref["floor"])
            note(f"conv host {cid} {mode} {form}: floor {ref['floor']:.2e} gate {ref['gate']:.2e}")
            slack = R.slack(case, mode, ref)               # (the bf16 half ulp, where the storage is bf16)
            for mutant in R.MUTANTS:
                if not R.mutant_applies(case, mutant, mode, form):
                    continue
                got, _ = R.expected(case, mode, form, ref["inp"], mutant=mutant)
                dist = R.measure(got, ref["want"], ref["A"], slack) / ref["gate"]
                note(f"conv host {cid} {mode} {form}: mutant {mutant} at {dist:.3g} x gate")
                assert dist >= R.MUTANT_DISTANCE, (mode, form, mutant, dist)


def test_every_mutant_is_exercised():
    hit = {m: 0 for m in R.MUTANTS}
    for case in R.RANDOM_CASES.values():
        for m in R.MUTANTS:
            hit[m] += any(R.mutant_applies(case, m, mode, form) for mode in R.MODES for form in R.forms(case, mode))
    assert all(hit.values()), hit


# ------------------------------------------------------------------------------------------------ backward-data
@pytest.mark.parametrize("cid", [c.id for c in R.CASES.values() if c.kind == "bwd"])
def test_backward_data_forms_equal_autograd(cid):
    """core() of a backward case (a cropped transposed convolution) and, for stride 1, the flipped-tap convolution the
    kernels are handed (pads k-1-p) both equal fp64 autograd of the padded forward convolution."""
    case = R.CASES[cid]
    inp = R.inputs(case, "fp32")
    gy = inp["abuf"][..., case.in_coff:case.in_coff + case.cout].permute(0, 4, 1, 2, 3).contiguous()
    w = inp["w"]
    pf = [R.same_pad(n, k, s) for n, k, s in zip(case.thw, case.k, case.s)]
    xp = torch.zeros((case.B, case.cin) + tuple(n + p[0] + p[1] for n, p in zip(case.thw, pf)), dtype=torch.float64,
                     requires_grad=True)
    y = F.conv3d(xp, w, stride=case.s)
    assert tuple(y.shape[2:]) == R.fwd_outs(case)
    (y * gy).sum().backward()
    dx = xp.grad[:, :, pf[0][0]:pf[0][0] + case.thw[0], pf[1][0]:pf[1][0] + case.thw[1], pf[2][0]:pf[2][0] + case.thw[2]]
    scale = float(R.core(case, gy.abs(), w.abs()).max())
    forms = [None] + (["flipped"] if not R.is_d2s(case) else [])
    for f in forms:
        got = R.core(case, gy, w, f)
        assert float((got[:, :case.cin] - dx).abs().max()) <= 1e-13 * scale, f
        assert float(got[:, case.cin:].abs().max() if case.cinp > case.cin else 0.0) == 0.0


# ------------------------------------------------------------------------------------------------ dispatch tables
def _csrc(name):
    with open(os.path.join(PKG, "csrc", name)) as f:
        return f.read()


def test_tile_tables_are_those_of_csrc():
    src = _csrc("conv3d_halo_impl.h")
    body = src[src.index("constexpr HaloTile kHaloTiles[] = {"):src.index("constexpr int HALO_NUM_VARIANTS")]
    rows = re.findall(r"\{\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(true|false)\}", body)
    assert [tuple(int(v) for v in r[:9]) + (int(r[9] == "true"),) for r in rows] == R.HALO_TILES
    src = _csrc("conv3d.hip")
    body = src[src.index("constexpr IgemmTile kIgemmTiles[8] = {"):src.index("template <int V>\nstatic int launch_variant")]
    rows = re.findall(r"\{(\d+), (\d+), \d+, \d+, \d+, (true|false), (true|false)\}", body)
    assert [(int(a), int(b), c == "true", d == "true") for a, b, c, d in rows] == R.IGEMM_TILES
    assert "constexpr size_t HALO_LDS_MAX = 160 * 1024;" in _csrc("conv3d_halo_impl.h")


@pytest.mark.parametrize("mode", R.MODES)
def test_listed_variants_are_those_of_the_library(mode):
    """listed_variants restates variant_rule: ivf_conv3d_variants (a host-only call) must list the same ids for every
    case; the admitted ones are a subset, and every case but a bf16act depth-to-space with a 7-tap kernel has some."""
    import ivf_lib as L
    lib = L.lib()
    ids = (ctypes.c_int * 96)()
    for case in R.CASES.values():
        d = R.fill_desc(L.ConvDesc(), case, L.MATH_MODES[mode])
        n = lib.ivf_conv3d_variants(ctypes.byref(d), ids, 96)
        assert list(ids)[:n] == R.listed_variants(case, mode), case.id
        adm = R.admitted_variants(case, mode, "ep")
        assert set(adm) <= set(list(ids)[:n])
        assert adm or (mode == "bf16act" and case.id == "D1"), case.id
