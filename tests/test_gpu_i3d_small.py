"""The I3D plan op by op against fp64 at small, odd clip geometries (tests/i3d_refs.py: cases, restatement, gates).

Every op of the plan is compared on the GPU's OWN inputs: the forward of an op on the buffer the GPU read, the
backward on the gradient buffer and the activations (ReLU gates, arg-max inputs) the GPU read.  So there are no gate
flips and no tie ambiguity, every element of every buffer of all three clips is compared against its own gate, and
pools and the layout conversions at both ends are compared bit for bit.  The gates come from the CPU floors of
i3d_refs.reference (test_i3d_refs_host.py); nothing here is fitted to what the GPU gives."""
import contextlib
import time
from collections import OrderedDict

import numpy as np
import pytest
import torch

import arena_fill as AF
import i3d_refs as R
from conftest import note

pytestmark = pytest.mark.gpu

_T0 = []
_ENGINES = {}


def engine(cid, mode, tuned=False, fill=None):
    """One engine per (case, mode[, tuned]) for the whole module, built-in kernel choice unless tuned.  fill: a byte
    pattern (tests/arena_fill.py) both arenas hold when the plan is bound and its weights are loaded."""
    import ivf_engine
    key = (cid, mode, tuned, fill)
    _T0.append(time.time())
    if key not in _ENGINES:
        case = R.CASES[cid]
        with AF.filled(fill, outputs=False) if fill is not None else contextlib.nullcontext():
            eng = ivf_engine.I3DEngine(R.NUM_CLASSES, case.clip, max_batch=R.MAX_BATCH, softmax=True, math=mode,
                                       **case.engine)
            eng.load_state_dict(R.state_dict(case), autotune=False)
        if tuned:
            eng.autotune(reps=1)
        eng.case_id = cid
        _ENGINES[key] = eng
    return _ENGINES[key]


@pytest.fixture(scope="module", params=R.CASE_MODES, ids=[f"{c}-{m}" for c, m in R.CASE_MODES])
def plain(request):
    cid, mode = request.param
    return cid, mode, engine(cid, mode)


def read_all(eng, b, grad=False):
    """every buffer of the plan (or its gradient buffer), all b clips, NCTHW float64 on the host"""
    out = {}
    for name in R.buffer_names(R.CASES[eng.case_id]):
        out[name] = eng.endpoint(name + (":grad" if grad else ""), b).cpu().double()
    return out


def compare(results, bufs, extra, mode, gates, what):
    """Every result against its gate, in the order given (forward bottom-up, backward top-down: the first failing op
    is the one to look at).  Returns the worst measured / gate ratio and its key."""
    worst, at = 0.0, None
    for key, r in results.items():
        got = extra[key] if key in extra else bufs[r.buf.split(":")[0]][:, r.c0:r.c1]
        q = R.ratio(got, r, mode, gates.get(key, 1.0))
        assert q <= 1.0, f"{what}: first failing op {key} ({r.kind}): measured / gate = {q:.3g}"
        if r.kind == "A" and q > worst:
            worst, at = q, key
    return worst, at


def opwise(eng, cid, mode, variant, what, b=R.MAX_BATCH, fill=None):
    """forward at b clips, backward with a dense dout or the arg-max targets; every buffer of every clip.  fill: the
    byte pattern the whole workspace is set to before the forward."""
    case = R.CASES[cid]
    gates = R.reference(case, mode)["gate"]
    x = R.clips(case)[:b]
    xd = x.cuda()
    if fill is not None:
        AF.refill(eng, fill)
    probs, logits = eng.forward(xd, want_logits=True)
    acts = read_all(eng, b)
    assert bool((acts["input"][:, case.clip[0]:] == 0).all()), "pad channels of the cl4 input buffer"
    fres, _ = R.forward(case, mode, x, given=acts)
    extra = {"logits": logits.cpu().double(), "probs": probs.cpu().double()}
    wf, af = compare(fres, acts, extra, mode, gates, f"{what} forward")
    if variant == "dout":
        kw = dict(dout=R.dout(case)[:b])
        score, dx = eng.backward(b, dout=kw["dout"].cuda())
    else:
        kw = dict(target=eng.argmax(probs).cpu())
        score, dx = eng.backward(b, target=kw["target"].cuda())
        assert torch.equal(score.cpu(), probs.cpu()[torch.arange(b), kw["target"].long()])
    grads = read_all(eng, b, grad=True)
    bres, _ = R.backward(case, mode, acts, probs.cpu(), given=grads, **kw)
    wb, ab = compare(bres, grads, {}, mode, gates, f"{what} backward({variant})")
    assert torch.equal(dx.cpu().double(), grads["input"][:, :case.clip[0]]), "dx is not the first C channels of input:grad"
    assert len(fres) == 8 + 9 * 6 + 2 and len(bres) == 1 + 4 + 3 + 9 * 4
    return wf, af, wb, ab


# ------------------------------------------------------------------------------------------------ op-wise parity
@pytest.mark.parametrize("variant", ["dout", "target"])
def test_every_op_against_its_gate(plain, variant):
    """(smod in bf16act is the plan this test found broken: the forward ran, every backward stopped with 'bf16act
    depth-to-space needs the LDS-halo kernel (stride-1 form, k <= 4)' at the stem, whose backward at temporal stride 1
    is a 7-tap depth-to-space conv from bf16 gradients to an fp32 clip gradient -- see ivf_i3d::stem_bwd_wide.)"""
    cid, mode, eng = plain
    wf, af, wb, ab = opwise(eng, cid, mode, variant, f"{cid} {mode}")
    note(f"i3d small {cid} {mode} {variant}: worst measured/gate forward {wf:.3f} at {af}, backward {wb:.3f} at {ab}")
    if cid == "gray":
        # the same gates on a plan whose arenas held 0xFF (NaN in every float format of the plan) when it was bound and
        # loaded, and whose workspace holds it again before the forward: test_gpu_arena_contents.py has the matrix
        ff = engine(cid, mode, fill=0xFF)
        with AF.filled(0xFF):
            wf, af, wb, ab = opwise(ff, cid, mode, variant, f"{cid} {mode} 0xFF arenas", fill=0xFF)
        note(f"i3d small {cid} {mode} {variant} on 0xFF arenas: worst measured/gate forward {wf:.3f} at {af}, "
             f"backward {wb:.3f} at {ab}")


# ------------------------------------------------------------------------------------------------ partial batch, rows
def test_partial_batch_rows_are_bit_equal(plain):
    """b = 2 with clips (c2, c0) after a b = 3 run: probs and dx of each row equal the row of a fresh b = 3 run."""
    cid, mode, eng = plain
    case = R.CASES[cid]
    x = R.clips(case).cuda()
    p3 = eng.forward(x)
    tgt = eng.argmax(p3)
    _, dx3 = eng.backward(3, target=tgt)
    p3, dx3 = p3.clone(), dx3.clone()
    rows = [2, 0]
    p2 = eng.forward(x[rows].contiguous())
    _, dx2 = eng.backward(2, target=tgt[rows].contiguous())
    assert torch.equal(p2, p3[rows]) and torch.equal(dx2, dx3[rows])
    # and the full per-op check holds at b < max_batch with all clips read back
    opwise(eng, cid, mode, "target", f"{cid} {mode} b=2", b=2)


# ------------------------------------------------------------------------------------------------ history independence
def _record(eng, x, b=R.MAX_BATCH):
    probs = eng.forward(x)
    tgt = eng.argmax(probs)
    score, dx = eng.backward(b, target=tgt)
    grads = read_all(eng, b, grad=True)
    return OrderedDict([("probs", probs.clone()), ("score", score.clone()), ("dx", dx.clone())] +
                       [(k + ":grad", v) for k, v in grads.items()])


def test_result_is_independent_of_what_ran_before(plain):
    """forward + backward, bit for bit, before and after Grad-CAM passes (which switch off gates and dead-window
    marking at their target), a perturbed forward, searches in both modes and a b = 1 forward; with the side stream on
    and off, which must also agree with each other."""
    cid, mode, eng = plain
    case = R.CASES[cid]
    x = R.clips(case).cuda()
    T = case.clip[1]
    recs = {}
    try:
        for overlap in (True, False):
            eng.set_overlap(overlap)
            rec = _record(eng, x)
            tgt = eng.argmax(rec["probs"])
            eng.gradcam(x, target=tgt, layer="MaxPool3d_3a_3x3")
            eng.gradcam(x, target=tgt, layer="Mixed_4c")
            g = torch.Generator().manual_seed(5)
            eng.perturbed_forward(x, torch.rand(3, T, generator=g).cuda())
            for pmode in ("freeze", "reverse"):
                raw = (torch.rand(3, T, generator=g) - 0.5).cuda().contiguous()
                eng.search(x, tgt, raw, 0.01, 0.02, 2, mode=pmode)
            eng.forward(x[1:2].contiguous())
            again = _record(eng, x)
            for k in rec:
                assert torch.equal(rec[k], again[k]), f"{cid} {mode} overlap={overlap}: {k} depends on the history"
            recs[overlap] = rec
    finally:
        eng.set_overlap(True)
    for k in recs[True]:
        assert torch.equal(recs[True][k], recs[False][k]), f"{cid} {mode}: {k} differs with the side stream off"


# ------------------------------------------------------------------------------------------------ tuned plans
@pytest.mark.parametrize("mode", ["fp32", "bf16x6"])
@pytest.mark.parametrize("cid", list(R.CASES))
def test_tuned_plan_meets_the_same_gates(cid, mode):
    """A second engine per case after autotune(reps=1): the same per-element gates whichever variants the tuner
    picked.  The vector tested is noted (forward, backward id per convolution op; 0 = a site the fused GEMMs cover).  An
    untuned plan reports IVF_CONV_AUTO at every site, not the id it resolves to, so whether a tuned id is also the
    built-in choice is not recorded."""
    eng = engine(cid, mode, tuned=True)
    vec = eng.get_tuning()
    assert any(vec)
    wf, af, wb, ab = opwise(eng, cid, mode, "target", f"{cid} {mode} tuned")
    note(f"i3d small {cid} {mode} tuned: worst measured/gate forward {wf:.3f} at {af}, backward {wb:.3f} at {ab}; "
         f"tuning vector {vec}")


# ------------------------------------------------------------------------------------------------ Grad-CAM
@pytest.mark.parametrize("layer", ["MaxPool3d_4a_3x3", "Mixed_4f", "Mixed_5c"])
@pytest.mark.parametrize("cid", ["odd", "smod"])
def test_gradcam_on_a_small_plan(cid, layer):
    """gradcam(layer=L): every gradient buffer from the head down to L against its per-op reference with L ungated and
    the pool L feeds keeping true arg-max codes (Mixed_4f feeds MaxPool3d_5a, whose dead windows then route to their
    first cell); then the map from the GPU's own activation and gradient of L -- fp64 weights and sum
    (leaf_refs.gradcam_ref and its bound), fp64 resize (resize_gate), normalisation (normalise_tol) -- and
    oracle.gradcam_ref.cam_from_activations on the same buffers, NaN pattern included.  Mixed_5c's raw head gradient
    is not kept in a buffer: there the gradient is head_bwd_ref's, its bound carried into the map's."""
    import leaf_refs as LR
    from oracle import gradcam_ref
    mode = "fp32"
    case = R.CASES[cid]
    eng = engine(cid, mode)
    gates = R.reference(case, mode)["gate"]
    x = R.clips(case)
    C, T, H, W = case.clip
    tgt = eng.argmax(eng.forward(x.cuda()))
    cam, probs = eng.gradcam(x.cuda(), target=tgt, layer=layer)
    acts = read_all(eng, 3)
    feat = acts[layer]
    fcl = feat.permute(0, 2, 3, 4, 1).reshape(3, -1, feat.shape[1])
    extra = 0.0
    if layer == "Mixed_5c":
        h = LR.head_bwd_ref(fcl, R.weights(case)["logits"]["w"], probs.cpu(), tgt.cpu(), None, True, False)
        gcl = h["dfeat"]
        extra = torch.einsum("bpc,bc->bp", fcl.abs(), h["b_dfeat"].mean(1))
    else:
        grads = read_all(eng, 3, grad=True)
        bres, _ = R.backward(case, mode, acts, probs.cpu(), target=tgt.cpu(), given=grads, cam=layer)
        assert layer + ":grad" in bres and not any(k.startswith("Conv3d_1a") or k == "input:grad" for k in bres)
        compare(bres, grads, {}, mode, gates, f"{cid} gradcam {layer}")
        gcl = grads[layer].permute(0, 2, 3, 4, 1).reshape(3, -1, feat.shape[1])
    ref = LR.gradcam_ref(fcl, gcl)
    Tf, hf, wf = feat.shape[2:]
    step = T // Tf
    assert step == (1 if cid == "smod" else T // Tf) and cam.shape == (3, Tf * step, H, W)
    cam64 = ref["cam"].reshape(3, Tf, hf, wf)
    gate, _ = LR.resize_gate(cam64.float(), H, W)
    # (a resized pixel is a convex combination of its slice's cells: it carries at most the slice's largest bound)
    gate = gate + (ref["b_cam"] + extra).reshape(3, Tf, -1).amax(-1).repeat_interleave(step, dim=1)[:, :, None, None]
    want, den = LR.normalise_ref(LR.resize_ref64(cam64, H, W), step, True)
    tol = LR.normalise_tol(want, den, gate, step)
    got = cam.cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN pattern"
    blocks = cam.view(3, Tf, step, H, W).view(torch.int32)          # T // T' frames repeat each slice bit for bit
    assert torch.equal(blocks, blocks[:, :, :1].expand_as(blocks))
    ok = ~torch.isnan(want)
    err = (got - want).abs()
    assert bool((err[ok] <= tol[ok]).all()), f"worst {float((err[ok] / tol[ok]).max()):.3g} of the bound"
    for b in range(3):
        vid = gradcam_ref.cam_from_activations(feat[b].numpy().astype(np.float32), gcl[b].T.reshape(feat.shape[1:]).numpy()
                                               .astype(np.float32), T, W, H, True)[0]
        vid = torch.from_numpy(np.ascontiguousarray(vid)).double().reshape(-1, H, W)
        assert torch.equal(torch.isnan(vid), torch.isnan(got[b])), "NaN pattern against the oracle"
        assert bool(((vid - got[b]).abs()[ok[b]] <= 2 * tol[b][ok[b]]).all())
    note(f"i3d small gradcam {cid} {layer}: {Tf} slices x {step} frames, map error {float((err[ok] / tol[ok]).max()):.2e} "
         f"of its bound (worst {float(err[ok].max()):.2e}), NaN frames {int(torch.isnan(want).all(dim=(2, 3)).sum())}")


def test_wall_time_of_this_file():
    note(f"i3d small: wall time of tests/test_gpu_i3d_small.py {time.time() - _T0[0]:.0f} s")
