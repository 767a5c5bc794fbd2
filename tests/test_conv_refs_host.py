"""CPU: what tests/conv_refs.py claims, proved on exactly the inputs test_gpu_conv_kernels.py runs -- the exact cases'
representability condition and how many outputs every dropped MFMA pass changes, the planes of the emulation, the
floors against the a-priori bound, the distance of every mutant from the gate, backward-data as a flipped-tap
convolution against fp64 autograd, and the restated dispatch tables against csrc and ivf_conv3d_variants.  For the fused
forms (second source, second output window, 1-bit gates) the same, per window and per source, with the mutants held to
conv_refs.compare itself, and the refusals of check_desc on the host."""
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
    for t in (inp["abuf"], inp["w"]) + ((inp["abuf2"],) if case.k0 else ()):
        assert torch.equal(t, t.float().double())
        p3 = R.split_planes(t, 3)
        assert torch.equal(p3[0] + p3[1] + p3[2], t)
        assert all(torch.equal(p, R.bf16_rne(p)) for p in p3)
        p2 = R.split_planes(t, 2)
        assert bool(((t - p2[0] - p2[1]).abs() <= 2.0 ** -16 * t.abs()).all())
    act = R.inputs(case, "bf16act")
    for name in ("abuf", "abuf2") * R.in_bf16(case, "bf16act") + ("base", "base2", "mask") * R.out_bf16(case, "bf16act"):
        if name in act:
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
    hit = {m: 0 for m in R.FUSED_MUTANTS}
    for case in R.FUSED_RANDOM_CASES.values():
        for m in R.FUSED_MUTANTS:
            hit[m] += any(R.mutant_applies(case, m, mode, form) for mode in R.MODES for form in R.forms(case, mode))
    assert all(hit.values()), hit
    assert hit["nibble"] >= 2 and hit["k0late"] >= 3 and hit["n0tile"] >= 3, hit


# ------------------------------------------------------------------------------------------------ the fused forms
@pytest.mark.parametrize("cid", list(R.FUSED_EXACT_CASES))
def test_fused_exact_cases_are_exact_and_show_every_pass(cid):
    """The exact patterns on the two-source and the two-window shape, per mode and form: the representability condition
    of test_exact_cases_are_exact_and_show_every_pass for every buffer; every window holds positive, negative and
    exactly zero ideal outputs on every clip (a record of `>= 0` differs from one of `> 0`); dropping any carried term
    changes at least DROP_SHARE of the outputs of EACH window, and so does dropping it on the chunks of EACH source
    alone; E4 has its two cancelling weights on channels of different sources."""
    case = R.CASES[cid]
    for mode in R.MODES:
        if not R.exact_applies(case, mode):
            continue
        inp = R.inputs(case, mode)
        a = R.act_window(case, inp)
        q = min(R.lowest_bit(a) * R.lowest_bit(inp["w"]), R.lowest_bit(inp["base"]))
        bound = float(R.core(case, a.abs(), inp["w"].abs()).max()) + float(inp["base"].abs().max())
        assert bound < 2.0 ** 24 * q, mode
        assert float(inp["scale"].abs().max()) <= 2 and torch.equal(inp["scale"], 2.0 ** torch.log2(inp["scale"]).round())
        if case.k0 and case.pattern == "E4":
            nz = inp["w"].reshape(case.cout, -1) != 0
            rows = nz.any(1)
            assert int(rows.sum()) >= case.cout * 3 // 4
            assert bool((nz[rows][:, :case.k0].sum(1) == 1).all()) and bool((nz[rows][:, case.k0:].sum(1) == 1).all())
        sources = (None, 0, 1) if case.k0 else (None,)
        for form in R.forms(case, mode):
            ref = R.reference(case, mode, form)
            f32 = R.expected_all(case, mode, form, inp, torch.float32)
            for name, (_, coff, n) in R.windows(case).items():
                want = ref["all"][name][0]
                assert torch.equal(want.float().double(), want), (mode, form, name)
                assert torch.equal(f32[name][0], want), (mode, form, name)
                win = want[..., coff:coff + n]
                for b in range(case.B):
                    assert bool((win[b] > 0).any()) and bool((win[b] < 0).any()) and bool((win[b] == 0).any()), (mode, form, name, b)
            for rname in R.records(case) if form == "ep+rec" else ():
                assert torch.equal(f32[rname], ref["all"][rname]), (mode, form, rname)
            for term in R.carried_terms(case, mode, inp):
                hidden = term in R.HIDDEN.get((case.pattern, mode), ())
                for src in sources:
                    dropped = R.expected_all(case, mode, form, inp, drop=term if src is None else term + (src,))
                    for name, (_, coff, n) in R.windows(case).items():
                        got = R.stored(case, mode, ref["all"][name][0])[..., coff:coff + n]
                        share = float((R.stored(case, mode, dropped[name][0])[..., coff:coff + n] != got).double().mean())
                        note(f"conv exact {cid} {mode} {form}: dropping term a{term[0]}*w{term[1]}"
                             + ("" if src is None else f" on source {src}") + f" changes {share:.1%} of {name}"
                             + (" (hidden by the bf16 store; shown by E4)" if hidden else ""))
                        if not hidden:
                            assert share >= R.DROP_SHARE, (mode, form, term, src, name)


@pytest.mark.parametrize("mode", R.MODES)
def test_fused_patterns_carry_every_term_of_the_mode(mode):
    """On the two-source and on the two-window shape, the exact patterns together show every MFMA pass of the mode."""
    shown, terms = {}, {}
    for case in R.FUSED_EXACT_CASES.values():
        if not R.exact_applies(case, mode):
            continue
        shape = case.id.split("-", 1)[1]
        hidden = R.HIDDEN.get((case.pattern, mode), ())
        shown.setdefault(shape, set()).update(t for t in R.carried_terms(case, mode, R.inputs(case, mode)) if t not in hidden)
        terms[shape] = set(R.operand_planes(case, mode)[2])
    assert len(terms) == 2
    for shape, want in terms.items():
        assert shown[shape] == want, (shape, shown[shape], want)


@pytest.mark.parametrize("cid", list(R.FUSED_RANDOM_CASES))
def test_fused_floors_are_bounded_and_mutants_are_rejected(cid):
    """Per mode and form of a fused case: the floor is inside the a-priori bound; the ideal itself passes R.compare, the
    comparison the GPU test applies; every mutant that applies -- the unfused ones included -- is rejected by it, a
    value mutant from at least MUTANT_DISTANCE gates away, a record mutant with at least one failing byte."""
    case = R.CASES[cid]
    for mode in R.MODES:
        for form in R.forms(case, mode):
            ref = R.reference(case, mode, form)
            assert ref["floor"] <= R.sum_bound(1.0, R.n_terms(case, mode)), (mode, form, ref["floor"])
            note(f"conv host {cid} {mode} {form}: floor {ref['floor']:.2e} gate {ref['gate']:.2e}")
            tgt = R.targets(case, mode, form)
            twin = R.as_buffers(case, R.reference(case, mode, "acc")["all"]) if form == "acc+bits" else None
            assert R.compare(case, mode, form, tgt, R.as_buffers(case, ref["all"]), twin) == []
            for mutant in R.MUTANTS + R.FUSED_MUTANTS:
                if not R.mutant_applies(case, mutant, mode, form):
                    continue
                got = R.as_buffers(case, R.expected_all(case, mode, form, ref["inp"], mutant=mutant))
                fails = R.compare(case, mode, form, tgt, got, twin)
                assert fails, (mode, form, mutant)
                if mutant in R.BIT_MUTANTS:
                    assert any(f.startswith("rec") for f in fails), (mode, form, mutant, fails)
                    note(f"conv host {cid} {mode} {form}: mutant {mutant}: {fails[0]}")
                    continue
                dist = R.worst(case, tgt, got) / ref["gate"]
                note(f"conv host {cid} {mode} {form}: mutant {mutant} at {dist:.3g} x gate")
                assert dist >= R.MUTANT_DISTANCE, (mode, form, mutant, dist)


_CODES = {"BAD_ARG": -1, "UNSUPPORTED": -3}       # IVF_ERR_* (include/ivf_hip.h)


def test_illegal_fused_descriptors_are_refused():
    """check_desc of csrc/conv3d.hip, on the host: every illegal combination of the fused forms comes back as
    IVF_ERR_BAD_ARG with its own message before any pointer is read (ivf_conv3d_default_variant; the two that need a
    relu_mask pointer through ivf_conv3d with NULL data pointers, which check_desc precedes), and the descriptors they
    were derived from are accepted; ivf_conv3d_variants offers a second window the implicit-GEMM tiles only."""
    import ivf_lib as L
    lib = L.lib()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.addressof(dummy)
    mm = L.MATH_MODES["bf16x3"]

    def desc(cid, form="ep"):
        case = R.CASES[cid]
        return R.set_form(R.fill_desc(L.ConvDesc(), case, mm, P, P), case, form, P, P, P)

    def refused(d, text, mask=None):
        rc = lib.ivf_conv3d(ctypes.byref(d), None, None, None, None, mask, None, None) if mask else \
            lib.ivf_conv3d_default_variant(ctypes.byref(d))
        assert rc == _CODES["BAD_ARG"], (text, rc)
        assert text in lib.ivf_last_error().decode(), (text, lib.ivf_last_error().decode())

    for cid, form in (("O2-24+48", "ep"), ("O2-24+48", "ep+rec"), ("F2-40+24", "acc"), ("F2-40+24", "acc+bits"), ("G3", "ep+rec"),
                      ("G3", "acc+bits")):
        assert lib.ivf_conv3d_default_variant(ctypes.byref(desc(cid, form))) > 0, (cid, form)
    d = desc("O2-24+48")
    d.accumulate = 1
    refused(d, "a second output window is a forward-epilogue feature")          # out2 with accumulate
    refused(desc("O2-24+48"), "a second output window is a forward-epilogue feature", mask=P)      # out2 with relu_mask
    d = desc("G3", "ep+rec")
    d.gate_in, d.gate_in_ld = P, 7
    refused(d, "gate_out / gate_out2 are forward-epilogue records")             # gate_out with gate_in
    refused(desc("G3", "acc+bits"), "gate_in replaces relu_mask", mask=P)       # gate_in with a mask
    d = desc("G3", "ep+rec")
    d.gate_out2, d.gate_out2_ld = P, 7
    refused(d, "gate_out2 needs out2")                                          # gate_out2 without out2
    d = desc("G3")
    d.in2, d.K0, d.in2_ld, d.in2_coff = P, 8, 16, 0
    refused(d, "a second input is only defined for 1x1x1 convs")                # in2 on a conv with taps
    d = desc("O2-24+48", "ep+rec")
    d.N0 = 22
    refused(d, "1-bit gates with out2 need 4-aligned windows")                  # a misaligned N0 with gates
    d = desc("O2-24+48", "ep+rec")
    d.N0, d.out_ld = 28, 48
    refused(d, "gate_out2 needs out2 with 8-aligned N0")
    d = desc("G3", "acc+bits")
    d.gate_in_coff = 6
    refused(d, "needs a 4-aligned channel offset")
    d = desc("G3", "ep+rec")
    d.gate_out_coff = 4
    refused(d, "gate_out window must be 8-aligned")
    d = desc("S3-n50")
    d.gate_out, d.gate_out_ld = P, 8
    refused(d, "1-bit gates need Cout")
    # the list of a two-window conv with taps: no LDS-halo tile, although the shape alone would admit them
    ids = (ctypes.c_int * 96)()
    d = desc("O2-k3-48+24")
    n = lib.ivf_conv3d_variants(ctypes.byref(d), ids, 96)
    assert list(ids)[:n] == [R.IGEMM_BASE, R.IGEMM_BASE + 1, R.IGEMM_BASE + 2]
    d.out2 = None
    assert lib.ivf_conv3d_variants(ctypes.byref(d), ids, 96) == 3 + len(R.HALO_TILES)


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
    dummy = ctypes.create_string_buffer(64)         # (a non-null in2 / out2: the call reads no data)
    for case in R.CASES.values():
        d = R.fill_desc(L.ConvDesc(), case, L.MATH_MODES[mode], ctypes.addressof(dummy), ctypes.addressof(dummy))
        n = lib.ivf_conv3d_variants(ctypes.byref(d), ids, 96)
        assert list(ids)[:n] == R.listed_variants(case, mode), case.id
        adm = R.admitted_variants(case, mode, "ep")
        assert set(adm) <= set(list(ids)[:n])
        assert adm or (mode == "bf16act" and case.id == "D1"), case.id
