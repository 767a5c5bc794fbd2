"""Every convolution kernel variant against tests/conv_refs.py: the exact cases bit for bit, the random cases per element
against the arithmetic mode's own fp64 ideal at 8 x the float32 floor, with the bytes around every channel window
checked.  Per case and mode every id of ivf_conv3d_variants is launched in both epilogue forms; the ids that ran must be
the ones conv_refs.admitted_variants derives from the tile tables and LDS budgets of csrc (test_conv_refs_host.py proves
the gates, the mutant distances and those tables on the CPU).  The fused forms of the Inception modules -- a second
source (in2 / K0), a second output window (out2 / N0), 1-bit ReLU gates written (gate_out / gate_out2: 'ep+rec') and read
(gate_in: 'acc+bits') -- go through the same comparison, conv_refs.compare, which also holds the guard row behind every
buffer, the record bytes and the relu_mask twin of a gate_in launch."""
import ctypes

import pytest
import torch

import conv_refs as R
from conftest import note

pytestmark = pytest.mark.gpu


def _dev(t, bf16):
    return t.to(torch.bfloat16 if bf16 else torch.float32).cuda().contiguous()


def _pack(lib, L, case, mm, w, in2, out2):
    """The packed weights of the case in the mode, and the descriptor of its convolution."""
    p = R.pads(case)
    if case.kind == "fwd":
        wp = torch.empty(lib.ivf_conv3d_pack_fwd_elems(case.cout, case.cinp, *case.k, mm), device="cuda")
        L.check(lib.ivf_conv3d_pack_fwd(L.ptr(w), L.ptr(wp), case.cout, case.cin, case.cinp, *case.k, mm, L.stream()))
        d = R.fill_desc(L.ConvDesc(), case, mm, in2, out2)
    else:
        wp = torch.empty(lib.ivf_conv3d_pack_bwd_elems(case.cout, case.cinp, *case.k, *case.s, *p, mm), device="cuda")
        geom = L.BwdGeom()
        L.check(lib.ivf_conv3d_pack_bwd(L.ptr(w), None, L.ptr(wp), case.cout, case.cin, case.cinp, *case.k, *case.s, *p, mm,
                                        ctypes.byref(geom), L.stream()))
        d = R.fill_desc(L.ConvDesc(), case, mm, in2, out2)
        k, pf, _ = R.gemm_geometry(case)        # the geometry the host test derived the admitted variants from
        assert (geom.kT, geom.kH, geom.kW) == k and (geom.pT, geom.pH, geom.pW) == pf
        assert geom.d2s == int(R.is_d2s(case)) and geom.rows == d.Cout
    return wp, d


def _run(cid):
    """Every listed variant of a case, in every mode and form, through R.compare: an exact case bit for bit in every
    buffer, a random case per element, with the guard rows, the bytes around every window, the gate records and the
    relu_mask twin of a gate_in launch (the docstring of R.compare)."""
    import ivf_lib as L
    lib = L.lib()
    case = R.CASES[cid]
    ids = (ctypes.c_int * 96)()
    for mode in R.MODES:
        if case.pattern and not R.exact_applies(case, mode):
            continue
        mm = L.MATH_MODES[mode]
        ib, ob = R.in_bf16(case, mode), R.out_bf16(case, mode)
        inp = R.inputs(case, mode)
        a = _dev(inp["abuf"], ib)
        a2 = _dev(inp["abuf2"], ib) if case.k0 else None
        w = _dev(inp["w"], False)
        scale, shift = _dev(inp["scale"], False), _dev(inp["shift"], False)
        mask = _dev(inp["mask"], ob)
        bits = inp["bits"].cuda().contiguous() if "bits" in inp else None
        # the buffers the launches write, at fixed addresses: refilled before every launch
        fills = {form: {n: (t.cuda() if t.dtype == torch.uint8 else _dev(t, ob)) for n, t in R.prefill(case, mode, form, inp).items()}
                 for form in R.forms(case, mode)}
        bufs = {n: torch.empty_like(t) for f in fills.values() for n, t in f.items()}
        wp, d = _pack(lib, L, case, mm, w, a2.data_ptr() if case.k0 else None, bufs["out2"].data_ptr() if case.n0 else None)
        n = lib.ivf_conv3d_variants(ctypes.byref(d), ids, 96)
        listed = list(ids)[:n]
        assert listed == R.listed_variants(case, mode), mode
        twins = {}
        for form in R.forms(case, mode):
            ref = R.reference(case, mode, form)
            tgt = R.targets(case, mode, form, "cuda")
            d2s, bform = R.is_d2s(case), R.base_form(form)
            R.set_form(d, case, form, bufs["rec"].data_ptr() if "rec" in bufs else None,
                       bufs["rec2"].data_ptr() if "rec2" in bufs else None, bits.data_ptr() if bits is not None else None)
            sc, sh = (scale, shift) if bform == "ep" and not d2s else (None, None)
            mk = mask if form == "acc" and not d2s else None
            ran, worst, flips = [], 0.0, 0
            for v in listed:
                d.variant = v
                got = {n: bufs[n] for n in fills[form]}
                for n, t in got.items():
                    t.copy_(fills[form][n])
                rc = lib.ivf_conv3d(ctypes.byref(d), L.ptr(a), L.ptr(wp), L.ptr(sc), L.ptr(sh), L.ptr(mk), L.ptr(got["out"]),
                                    L.stream())
                if rc != 0:
                    continue        # refused: the LDS budget of the tile, or a form the kernel does not have
                ran.append(v)
                if not case.pattern:
                    err = R.worst(case, tgt, got)
                    worst = max(worst, err)
                    flips += R.band_flips(case, form, tgt, got)
                    print(f"[conv] {cid} {mode} {form} variant {v}: {err:.3e} of A, gate {ref['gate']:.3e}")
                fails = R.compare(case, mode, form, tgt, got, twins.get(v) if form == "acc+bits" else None)
                assert form != "acc+bits" or v in twins, f"{cid} {mode} variant {v} ran 'acc+bits' but not 'acc'"
                assert not fails, f"{cid} {mode} {form} variant {v}: " + "; ".join(fails) + (
                    "" if case.pattern else f" (error {err:.3e} of A, gate {ref['gate']:.3e}, floor {ref['floor']:.3e})")
                if form == "acc":
                    twins[v] = {n: t.clone() for n, t in got.items()}
            assert ran == R.admitted_variants(case, mode, form), f"{cid} {mode} {form}"
            if not ran:
                note(f"conv {cid} {mode} {form}: no variant has this form")
            elif case.pattern:
                note(f"conv {cid} {mode} {form}: {len(ran)} variants bit-equal to the exact result")
            else:
                note(f"conv {cid} {mode} {form}: floor {ref['floor']:.2e} gate {ref['gate']:.2e} measured {worst:.2e} "
                     f"over {len(ran)} variants" + (f" ({worst / ref['gate']:.2f} x gate)" if cid in R.FUSED_RANDOM_CASES else "")
                     + (f", {flips} record bits off the ideal's inside the band" if form == "ep+rec" else ""))


@pytest.mark.parametrize("cid", list(R.EXACT_CASES))
def test_exact_cases_bit_for_bit(cid):
    """Operands whose products and partial sums are all representable in fp32: every variant of every mode must return
    the mode's ideal exactly (bf16 storage: its RNE), in the scaled-store and in the accumulate + mask epilogue.  A
    dropped, doubled or misread MFMA pass changes at least a quarter of the outputs (test_conv_refs_host.py)."""
    _run(cid)


@pytest.mark.parametrize("cid", list(R.RANDOM_CASES))
def test_random_cases_per_element(cid):
    """Geometry and addressing: windows on convs with taps, the scalar epilogue, batch 1 and 3, maps below a box,
    pointwise K tails, backward-data of even kernels, non-cubic kernels, the (1,2,2)-stride depth-to-space, pix4 off
    its 7x7x7 shape -- every element within 8 x the float32 floor of the mode's ideal, nothing outside the window
    touched."""
    _run(cid)


@pytest.mark.parametrize("cid", list(R.FUSED_EXACT_CASES))
def test_fused_exact_cases_bit_for_bit(cid):
    """The two-source backward GEMM and the two-window forward on the exact patterns: out, out2 and the gate records of
    every variant equal the ideal's bit for bit, and a gate_in launch equals its relu_mask twin.  A plane pass dropped
    on one source's chunks only, or in one window only, changes at least a quarter of that window's outputs
    (test_conv_refs_host.py)."""
    _run(cid)


@pytest.mark.parametrize("cid", list(R.FUSED_RANDOM_CASES))
def test_fused_random_cases_per_element(cid):
    """in2 / K0 (K0 off the 32-chunk and the 8 grid, K % 8 == 4, a 4-channel first source, several column tiles), out2 /
    N0 (N0 off the 32-column grid, the scalar epilogue, N0 past the 128-column tile edge, kernels with taps) and the
    1-bit gates (records of both windows; gate_in at both nibble parities; every LDS-halo tile): every element of out
    and out2 within 8 x the float32 floor, nothing outside the windows touched, every record byte (own stored value
    > 0), the ideal's bit outside the tolerance band, and gate_in bit-equal to relu_mask."""
    _run(cid)
