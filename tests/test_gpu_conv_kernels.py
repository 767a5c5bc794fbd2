"""Every convolution kernel variant against tests/conv_refs.py: the exact cases bit for bit, the random cases per element
against the arithmetic mode's own fp64 ideal at 8 x the float32 floor, with the bytes around every channel window
checked.  Per case and mode every id of ivf_conv3d_variants is launched in both epilogue forms; the ids that ran must be
the ones conv_refs.admitted_variants derives from the tile tables and LDS budgets of csrc (test_conv_refs_host.py proves
the gates, the mutant distances and those tables on the CPU)."""
import ctypes

import pytest
import torch

import conv_refs as R
from conftest import note

pytestmark = pytest.mark.gpu


def _dev(t, bf16):
    return t.to(torch.bfloat16 if bf16 else torch.float32).cuda().contiguous()


def _pack(lib, L, case, mm, w):
    """The packed weights of the case in the mode, and the descriptor of its convolution."""
    p = R.pads(case)
    if case.kind == "fwd":
        wp = torch.empty(lib.ivf_conv3d_pack_fwd_elems(case.cout, case.cinp, *case.k, mm), device="cuda")
        L.check(lib.ivf_conv3d_pack_fwd(L.ptr(w), L.ptr(wp), case.cout, case.cin, case.cinp, *case.k, mm, L.stream()))
        d = R.fill_desc(L.ConvDesc(), case, mm)
    else:
        wp = torch.empty(lib.ivf_conv3d_pack_bwd_elems(case.cout, case.cinp, *case.k, *case.s, *p, mm), device="cuda")
        geom = L.BwdGeom()
        L.check(lib.ivf_conv3d_pack_bwd(L.ptr(w), None, L.ptr(wp), case.cout, case.cin, case.cinp, *case.k, *case.s, *p, mm,
                                        ctypes.byref(geom), L.stream()))
        d = R.fill_desc(L.ConvDesc(), case, mm)
        k, pf, _ = R.gemm_geometry(case)        # the geometry the host test derived the admitted variants from
        assert (geom.kT, geom.kH, geom.kW) == k and (geom.pT, geom.pH, geom.pW) == pf
        assert geom.d2s == int(R.is_d2s(case)) and geom.rows == d.Cout
    return wp, d


def _run(cid):
    import ivf_lib as L
    lib = L.lib()
    case = R.CASES[cid]
    ids = (ctypes.c_int * 96)()
    rows = R.out_chan(case)
    for mode in R.MODES:
        if case.pattern and not R.exact_applies(case, mode):
            continue
        mm = L.MATH_MODES[mode]
        ib, ob = R.in_bf16(case, mode), R.out_bf16(case, mode)
        inp = R.inputs(case, mode)
        a = _dev(inp["abuf"], ib)
        w = _dev(inp["w"], False)
        scale, shift = _dev(inp["scale"], False), _dev(inp["shift"], False)
        base, mask = _dev(inp["base"], ob), _dev(inp["mask"], ob)
        wp, d = _pack(lib, L, case, mm, w)
        n = lib.ivf_conv3d_variants(ctypes.byref(d), ids, 96)
        listed = list(ids)[:n]
        assert listed == R.listed_variants(case, mode), mode
        for form in R.forms(case, mode):
            ref = R.reference(case, mode, form)
            if case.pattern:
                want = _dev(R.stored(case, mode, ref["want"]), ob)
            else:
                want, A, tol = ref["want"].cuda(), ref["A"].cuda(), R.tolerance(case, mode, ref).cuda()
                slack = R.slack(case, mode, ref).cuda()      # (the measured figure is what exceeds the bf16 half ulp)
            if form == "acc":
                fill = base
            else:
                fill = torch.full_like(base, R.SENTINEL)
                fill[..., case.out_coff:case.out_coff + rows] = float("nan")
            d2s = R.is_d2s(case)
            d.accumulate = int(form == "acc")
            d.relu = int(form == "ep" and not d2s and R.relu_on(case))
            sc, sh = (scale, shift) if form == "ep" and not d2s else (None, None)
            mk = mask if form == "acc" and not d2s else None
            ran, worst = [], 0.0
            for v in listed:
                d.variant = v
                out = fill.clone()
                rc = lib.ivf_conv3d(ctypes.byref(d), L.ptr(a), L.ptr(wp), L.ptr(sc), L.ptr(sh), L.ptr(mk), L.ptr(out),
                                    L.stream())
                if rc != 0:
                    continue        # refused: the LDS budget of the tile, or a form the kernel does not have
                ran.append(v)
                if case.pattern:
                    assert torch.equal(out, want), (f"{cid} {mode} {form} variant {v}: {int((out != want).sum())} of "
                                                    f"{want.numel()} values differ from the exact result")
                else:
                    err = R.measure(out, want, A, slack)
                    worst = max(worst, err)
                    assert bool(((out.double() - want).abs() <= tol).all()), \
                        f"{cid} {mode} {form} variant {v}: error {err:.3e} of A, gate {ref['gate']:.3e} (floor {ref['floor']:.3e})"
            assert ran == R.admitted_variants(case, mode, form), f"{cid} {mode} {form}"
            if not ran:
                note(f"conv {cid} {mode} {form}: no variant has this form")
            elif case.pattern:
                note(f"conv {cid} {mode} {form}: {len(ran)} variants bit-equal to the exact result")
            else:
                note(f"conv {cid} {mode} {form}: floor {ref['floor']:.2e} gate {ref['gate']:.2e} measured {worst:.2e} "
                     f"over {len(ran)} variants")


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
