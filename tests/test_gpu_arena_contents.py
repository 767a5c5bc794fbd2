"""No result depends on what an arena, a scratch buffer or an output buffer held before the call.

include/ivf_hip.h: "the caller owns all memory", and ivf_*_bind only stores two pointers.  So every entry of a plan has
to write whatever it later reads.  Here every plan is built three times with the same weights, inside arenas that hold
0x00, 0xFF and 0x42 in every byte (tests/arena_fill.py: why these three), the workspace is put back to the pattern
before every entry -- except where the header defines an entry as reading what the previous one left: backward after
forward, the endpoint / layer_state reads -- and every returned tensor and every buffer readable through the plan is
compared BYTE FOR BYTE with the 0x00 engine's.  Parity with fp64 is gated elsewhere (test_gpu_i3d_small.py,
test_gpu_clstm_kernels.py, test_gpu_tfclstm_kernels.py); this makes those gates hold for any memory state.

Integer-typed regions of the workspaces, and why a pattern in them cannot become an address (read from the plan
builders, search_driver.h, mask_ops.hip, pool_head.hip, convlstm.hip, tf_clstm.hip):
  * arg-max records of every pool (uint8, all three plans): written by the forward for the b clips the backward reads;
    only ever COMPARED with a tap number, never used as an index;
  * 1-bit ReLU gate records (I3D): bits, written by the forward epilogues of the producers;
  * reverse partner table int [B,T] (I3D, CLSTM): ivf_submask_pairs_batched writes rows 0 .. b-1 in stage_perturbed
    before ivf_reverse_fwd_batched / ivf_reverse_bwd read the same rows; it is the one table that is used as an index;
  * off_target (I3D): carved, never used;  off_camtgt (CLSTM): written by ivf_argmax before the backward reads it;
  * per-row target tables of ig / smoothgrad (caller scratch): ig_row_targets writes all b K entries before the chunks;
  * the singular flag of ivf_lin_solve: lin_init_kernel writes it first.
No kernel waits on a value in memory, so no pattern can hang one either."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest
import torch

import arena_fill as AF
import clstm_refs as CR
import i3d_refs as R
import ivf_recipe
import tfclstm_refs as TR
from conftest import note

pytestmark = pytest.mark.gpu

_ENGINES = {}
ALL_KINDS = ("gradcam", "gradcam++", "xgradcam", "hirescam", "layercam")


def _rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


class Sequence:
    """One engine's walk through its entries: `call` refills the workspace and records what the entry returns; `read`
    records buffers the last entry left, without a refill."""

    def __init__(self, eng, pattern):
        self.eng, self.pattern, self.rec = eng, pattern, AF.Record()

    def call(self, label, fn, refill=True):
        if refill:
            AF.refill(self.eng, self.pattern)
        out = fn()
        self.rec.add(label, out)
        return out

    def read(self, label, value):
        self.rec.add(label, value, entry=False)


def _rows_beyond_b_hold(s, tail, what):
    """Rows b .. B-1 of a plan buffer after an entry at b < B still hold the pattern: the entry wrote no row it was not
    asked for -- and the fill is really what the kernels found there."""
    if tail.numel():
        assert bool((AF.as_bytes(tail) == s.pattern).all()), f"{what}: rows beyond b were written (0x{s.pattern:02X})"


def _compare(what, run):
    """run(pattern) -> Record, once per pattern; one note() line; asserts byte equality with the 0x00 record."""
    recs = OrderedDict((p, run(p)) for p in AF.PATTERNS)
    torch.cuda.synchronize()
    line, ok = AF.verdict(recs)
    note(f"arena contents {what}: {line}")
    assert ok, f"{what}: {line}"


# ================================================================================================== I3D plan
I3D_CASE_MODES = [("gray", m) for m in ("fp32", "bf16x3", "bf16act")] + \
                 [("odd", m) for m in ("fp32", "bf16x3", "bf16x6", "bf16act")]
MID_LAYERS = ("Mixed_5c", "Mixed_4d", "MaxPool3d_3a_3x3")


def i3d_engine(cid, mode, pattern):
    """One plan per (case, mode, pattern): built, and its weights loaded, inside arenas that hold the pattern."""
    import ivf_engine
    key = ("i3d", cid, mode, pattern)
    if key not in _ENGINES:
        case = R.CASES[cid]
        with AF.filled(pattern):
            eng = ivf_engine.I3DEngine(R.NUM_CLASSES, case.clip, max_batch=R.MAX_BATCH, softmax=True, math=mode,
                                       **case.engine)
            eng.load_state_dict(R.state_dict(case), autotune=False)
        eng.case_id = cid
        _ENGINES[key] = eng
    return _ENGINES[key]


def _i3d_bufs(eng, b, grad=False):
    return OrderedDict((n, eng.endpoint(n + (":grad" if grad else ""), b)) for n in R.buffer_names(R.CASES[eng.case_id]))


def _i3d_core(s, case, x, b, tgt):
    """forward / backward, the perturbed forwards and the gradient searches"""
    eng = s.eng
    T = case.clip[1]
    s.call("forward", lambda: eng.forward(x, want_logits=True))
    s.read("forward.acts", _i3d_bufs(eng, b))
    _rows_beyond_b_hold(s, eng.endpoint("input", R.MAX_BATCH)[b:], "the input buffer")
    s.call("backward(target)", lambda: eng.backward(b, target=tgt), refill=False)
    s.read("backward(target).grads", _i3d_bufs(eng, b, grad=True))
    s.call("forward'", lambda: eng.forward(x))
    s.call("backward(dout)", lambda: eng.backward(b, dout=R.dout(case)[:b].cuda()), refill=False)
    s.read("backward(dout).grads", _i3d_bufs(eng, b, grad=True))
    mask = _rand(5, R.MAX_BATCH, T)[:b].cuda()                       # runs above 0.1: the reverse pairing has pairs
    for pmode in ("freeze", "reverse"):
        s.call(f"perturbed_forward({pmode})", lambda: eng.perturbed_forward(x, mask, mode=pmode))
        s.read(f"perturbed_forward({pmode}).input", eng.endpoint("input", b))
    for pmode in ("freeze", "reverse"):
        raw = ((_rand(7, R.MAX_BATCH, T) - 0.3) * 4.0)[:b].cuda().contiguous()
        traj, (m, v, _) = s.call(f"search({pmode})", lambda: eng.search(x, tgt, raw, 0.01, 0.02, 3, mode=pmode))
        s.read(f"search({pmode}).state", (raw, m, v))
        s.read(f"search({pmode}).grads", _i3d_bufs(eng, b, grad=True))
    grid = (2, 3)
    raw = ((_rand(9, R.MAX_BATCH, T, *grid) - 0.5) * 2.0)[:b].cuda().contiguous()
    traj, (m, v, _) = s.call("st_search", lambda: eng.st_search(x, tgt, raw, 0.01, 0.02, 2, grid))
    s.read("st_search.state", (raw, m, v))
    M = eng.st_expand(_rand(11, R.MAX_BATCH, T, *grid)[:b].cuda(), grid)
    s.read("st_expand", M)
    s.call("st_perturbed_forward", lambda: eng.st_perturbed_forward(x, M))
    s.read("st_perturbed_forward.input", eng.endpoint("input", b))


def _i3d_cams(s, case, x, b, tgt):
    """The Grad-CAM family at the head, at a mid-module target and at a pool.  The truncated backward writes the
    gradient buffers from the head down to the target only, so of the plan's buffers the activations and the target's
    own gradient (cam_raw's 'grad') are compared, not the gradient buffers below it."""
    eng = s.eng
    for layer in MID_LAYERS:
        s.call(f"gradcam({layer})", lambda: eng.gradcam(x, target=tgt, layer=layer))
        s.call(f"gradcam({layer}, sequence)", lambda: eng.gradcam(x, target=tgt, layer=layer, per_frame=False,
                                                                 out_hw=(7, 9)))
        s.call(f"cam({layer})", lambda: eng.cam(x, target=tgt, kinds=ALL_KINDS, layer=layer))
        s.call(f"cam_raw({layer})", lambda: eng.cam_raw(x, target=tgt, kinds=ALL_KINDS, layer=layer))
        s.read(f"cam_raw({layer}).acts", _i3d_bufs(eng, b))


def _i3d_rows(s, case, x, b, tgt):
    """The forward-only row searches (each runs at least two chunks of max_batch rows), ig and smoothgrad"""
    eng = s.eng
    g3 = (2, 1, 2)

    def rows(label, fn):
        """a row search, then the rows its last chunk staged (pad lanes included) and the activations they gave"""
        scores = s.call(label, fn)
        assert scores.numel() > R.MAX_BATCH, f"{label}: one chunk only"
        last = scores.numel() % R.MAX_BATCH or R.MAX_BATCH
        s.read(f"{label}.input", eng.endpoint("input", last))
        s.read(f"{label}.Mixed_5c", eng.endpoint("Mixed_5c", last))
    for pmode in ("freeze", "reverse"):
        rows(f"blob_scores({pmode})", lambda: eng.blob_scores(x, tgt, max_len=2, mode=pmode))
    rows("box_scores", lambda: eng.box_scores(x, tgt, (2, 2), max_len=1, max_box=(1, 2)))
    rows("rise_scores", lambda: eng.rise_scores(x, tgt, n_masks=4, p=0.5, grid=(2, 2, 2), seed=3))
    rows("shap_scores", lambda: eng.shap_scores(x, tgt, n_perms=2, grid=(2, 1, 1), seed=3))
    bits, _ = eng.kshap_rows(4, g3, seed=3)
    rows("lin_scores", lambda: eng.lin_scores(x, tgt, bits, g3))
    ranks = eng.curve_ranks(_rand(13, R.MAX_BATCH, *g3)[:b].cuda(), g3)
    rows("curve_scores", lambda: eng.curve_scores(x, tgt, ranks, g3, step=2, curves=3))
    F = _rand(15, R.MAX_BATCH, 4, *g3)[:b].cuda()
    for perturb in ("freeze", "blank"):
        rows(f"scorecam_scores({perturb})", lambda: eng.scorecam_scores(x, tgt, F, perturb=perturb))
    s.call("ig", lambda: eng.ig(x, tgt, steps=3))
    s.call("ig(constant)", lambda: eng.ig(x, tgt, steps=3, baseline="constant", base=1.0))
    s.call("smoothgrad", lambda: eng.smoothgrad(x, tgt, n_samples=3, level=0.15, seed=3))
    last = (b * 3) % R.MAX_BATCH or R.MAX_BATCH            # rows of the last chunk: the backward wrote these
    s.read("smoothgrad.grads", _i3d_bufs(eng, min(last, b), grad=True))


I3D_PARTS = OrderedDict([("core", _i3d_core), ("cams", _i3d_cams), ("rows", _i3d_rows)])


def _i3d_run(cid, mode, b, part, overlap=True):
    case = R.CASES[cid]

    def run(pattern):
        eng = i3d_engine(cid, mode, pattern)
        eng.set_overlap(overlap)
        try:
            with AF.filled(pattern):
                x = R.clips(case)[:b].cuda()
                tgt = torch.tensor([(r + 1) % R.NUM_CLASSES for r in range(b)], dtype=torch.int32, device="cuda")
                s = Sequence(eng, pattern)
                I3D_PARTS[part](s, case, x, b, tgt)
        finally:
            eng.set_overlap(True)
        return s.rec
    _compare(f"i3d {cid} {mode} {part} b={b}/B={R.MAX_BATCH}" + ("" if overlap else " overlap off"), run)


@pytest.mark.parametrize("b", [R.MAX_BATCH, 2])
@pytest.mark.parametrize("part", list(I3D_PARTS))
@pytest.mark.parametrize("cid,mode", I3D_CASE_MODES, ids=[f"{c}-{m}" for c, m in I3D_CASE_MODES])
def test_i3d_plan(cid, mode, part, b):
    _i3d_run(cid, mode, b, part)


def test_the_comparison_sees_a_backward_that_reads_the_fill():
    """The control: with the workspace refilled BETWEEN forward and backward -- which the header does not allow, the
    backward reads the forward's state -- the backward reads the fill, and the records differ under both patterns.
    (Safe by the list at the top of this file: what it then reads as integers is only ever compared.)"""
    cid, mode, b = "gray", "fp32", R.MAX_BATCH
    case = R.CASES[cid]
    recs = OrderedDict()
    for pattern in AF.PATTERNS:
        eng = i3d_engine(cid, mode, pattern)
        with AF.filled(pattern):
            x = R.clips(case)[:b].cuda()
            tgt = torch.tensor([(r + 1) % R.NUM_CLASSES for r in range(b)], dtype=torch.int32, device="cuda")
            s = Sequence(eng, pattern)
            s.call("forward", lambda: eng.forward(x))
            s.call("backward after a refill", lambda: eng.backward(b, target=tgt))
        recs[pattern] = s.rec
    torch.cuda.synchronize()
    for p in (0xFF, 0x42):
        d = AF.first_difference(recs[AF.BASELINE], recs[p])
        assert d is not None and d.startswith("backward after a refill"), f"0x{p:02X}: {d}"
        note(f"arena contents control (refill between forward and backward) 0x{p:02X}: first differing buffer {d}")


@pytest.mark.parametrize("part", list(I3D_PARTS))
def test_i3d_plan_without_the_side_stream(part):
    _i3d_run("odd", "fp32", 2, part, overlap=False)


def test_i3d_tuned_plan():
    """The variants the autotuner picks (by timing: they differ from machine to machine) instead of the built-in
    choice: tuned once on the 0x00 plan, the same vector set on the other two."""
    cid, mode, b = "odd", "bf16x6", R.MAX_BATCH
    base = i3d_engine(cid, mode, AF.BASELINE)
    before = base.get_tuning()
    base.autotune(reps=1)
    vec = base.get_tuning()
    try:
        for p in AF.PATTERNS:
            i3d_engine(cid, mode, p).set_tuning(vec)
        _i3d_run(cid, mode, b, "core")
    finally:
        for p in AF.PATTERNS:
            i3d_engine(cid, mode, p).set_tuning(before)
    note(f"arena contents i3d {cid} {mode} tuned: vector {vec}")


@pytest.mark.parametrize("mode", ["bf16x6", "bf16act"])
def test_i3d_plan_at_the_flagship_geometry(mode):
    """16 x 224 x 224 clips, the shapes the search driver runs at (and the only ones at which the LDS-halo convolutions
    have interior boxes, full and short edge boxes side by side): forward / backward, a mid-module Grad-CAM and one
    search step at b = B = 2, then forward / backward at b = 1.  The plans are not kept."""
    import ivf_engine
    clip, K, B = (3, 16, 224, 224), 6, 2
    sd = ivf_recipe.i3d_state_dict(num_classes=K)
    x = torch.from_numpy(np.stack([ivf_recipe.clip(i, *clip) for i in (3, 4)])).cuda()

    def run(pattern):
        with AF.filled(pattern):
            eng = ivf_engine.I3DEngine(K, clip, max_batch=B, softmax=True, math=mode)
            eng.load_state_dict(sd, autotune=False)
            s = Sequence(eng, pattern)
            for b in (B, 1):
                tgt = torch.tensor([1, 4][:b], dtype=torch.int32, device="cuda")
                xb = x[:b].contiguous()
                s.call(f"forward b={b}", lambda: eng.forward(xb, want_logits=True))
                s.read(f"forward b={b}.Mixed_3b", eng.endpoint("Mixed_3b", b))
                s.call(f"backward b={b}", lambda: eng.backward(b, target=tgt), refill=False)
                s.read(f"backward b={b}.Conv3d_2c_3x3:grad", eng.endpoint("Conv3d_2c_3x3:grad", b))
            s.call("gradcam(Mixed_4d)", lambda: eng.gradcam(x, target=tgt.new_tensor([1, 4]), layer="Mixed_4d"))
            raw = ((_rand(7, B, clip[1]) - 0.3) * 4.0).cuda().contiguous()
            s.call("search", lambda: eng.search(x, tgt.new_tensor([1, 4]), raw, 0.01, 0.02, 1))
            s.read("search.raw", raw)
            torch.cuda.synchronize()
        return s.rec
    _compare(f"i3d flagship {clip} {mode} B={B}", run)


# ================================================================================================== CLSTM plan
CLSTM_CASES = ("S1", "S4", "S3", "W1", "P2")


def clstm_engine(cid, pattern):
    import ivf_engine
    key = ("clstm", cid, pattern)
    if key not in _ENGINES:
        case = CR.CASES[cid]
        sd = CR.case_inputs(case, b=1)[1]
        with AF.filled(pattern):
            eng = ivf_engine.CLSTMEngine(CR.K, (case.C, case.T, case.H, case.W), max_batch=case.B, hidden=case.hid,
                                         layers=case.layers, kernel=case.k, stride=case.s, softmax=case.softmax,
                                         batch_norm=case.batch_norm,
                                         out_steps=list(case.out_steps) if case.out_steps else None)
            eng.load_state_dict(sd)
        _ENGINES[key] = eng
    return _ENGINES[key]


_CLSTM_INPUTS = {}


def _clstm_inputs(case):
    if case.id not in _CLSTM_INPUTS:
        x, _, _, _ = CR.case_inputs(case, b=case.B)
        _CLSTM_INPUTS[case.id] = x
    return _CLSTM_INPUTS[case.id]


def _clstm_states(eng, case, b):
    return [eng.layer_state(l, b) for l in range(case.layers)]


def _clstm_sequence(s, case, x, b, tgt):
    eng = s.eng
    T = case.T
    s.call("forward", lambda: eng.forward(x, want_logits=True))
    if case.dout:
        dout = torch.from_numpy(ivf_recipe.uniform(f"clstmk_{case.id}/dout", (case.B, CR.K), -1.0, 1.0))[:b].cuda()
        s.call("backward(dout)", lambda: eng.backward(b, dout=dout), refill=False)
    else:
        s.call("backward(target)", lambda: eng.backward(b, target=tgt), refill=False)
    s.read("backward.states", _clstm_states(eng, case, b))
    for l in range(case.layers):
        for t, name in zip(eng.layer_state(l, case.B), ("X", "dX")):
            _rows_beyond_b_hold(s, t[b:], f"{name}[{l}]")
    mask = _rand(5, case.B, T)[:b].cuda()
    for pmode in ("freeze", "reverse"):
        s.call(f"perturbed_forward({pmode})", lambda: eng.perturbed_forward(x, mask, mode=pmode))
        raw = ((_rand(7, case.B, T) - 0.3) * 4.0)[:b].cuda().contiguous()
        traj, (m, v, _) = s.call(f"search({pmode})", lambda: eng.search(x, tgt, raw, 0.01, 0.02, 3, mode=pmode))
        s.read(f"search({pmode}).state", (raw, m, v))
        s.read(f"search({pmode}).states", _clstm_states(eng, case, b))
    for layer in (None, 0):
        s.call(f"gradcam({layer})", lambda: eng.gradcam(x, target=tgt, layer=layer))
        s.call(f"gradcam({layer}, argmax)", lambda: eng.gradcam(x, layer=layer, per_frame=False, out_hw=(7, 9)))
        s.call(f"cam({layer})", lambda: eng.cam(x, target=tgt, kinds=ALL_KINDS, layer=layer))
        s.call(f"cam_raw({layer})", lambda: eng.cam_raw(x, target=tgt, kinds=ALL_KINDS, layer=layer))
    for pmode in ("freeze", "reverse"):
        s.call(f"blob_scores({pmode})", lambda: eng.blob_scores(x, tgt, max_len=2, mode=pmode))
    s.call("ig", lambda: eng.ig(x, tgt, steps=3))
    s.call("smoothgrad", lambda: eng.smoothgrad(x, tgt, n_samples=3, level=0.15, seed=3))
    # not asked for by the matrix, but the same shared drivers with NCTHW staging (layout 0) instead of 16-byte pixels
    grid, g3 = (2, 3), (2, 1, 2)
    raw = ((_rand(9, case.B, T, *grid) - 0.5) * 2.0)[:b].cuda().contiguous()
    traj, (m, v, _) = s.call("st_search", lambda: eng.st_search(x, tgt, raw, 0.01, 0.02, 2, grid))
    s.read("st_search.state", (raw, m, v))
    M = eng.st_expand(_rand(11, case.B, T, *grid)[:b].cuda(), grid)
    s.call("st_perturbed_forward", lambda: eng.st_perturbed_forward(x, M))
    s.call("box_scores", lambda: eng.box_scores(x, tgt, (2, 2), max_len=1, max_box=(1, 2)))
    s.call("rise_scores", lambda: eng.rise_scores(x, tgt, n_masks=4, p=0.5, grid=(2, 2, 2), seed=3))
    s.call("shap_scores", lambda: eng.shap_scores(x, tgt, n_perms=2, grid=(2, 1, 1), seed=3))
    bits, _ = eng.kshap_rows(4, g3, seed=3)
    s.call("lin_scores", lambda: eng.lin_scores(x, tgt, bits, g3))
    ranks = eng.curve_ranks(_rand(13, case.B, *g3)[:b].cuda(), g3)
    s.call("curve_scores", lambda: eng.curve_scores(x, tgt, ranks, g3, step=2, curves=3))
    F = _rand(15, case.B, 4, *g3)[:b].cuda()
    for perturb in ("freeze", "blank"):
        s.call(f"scorecam_scores({perturb})", lambda: eng.scorecam_scores(x, tgt, F, perturb=perturb))


def _clstm_run(cid, b):
    case = CR.CASES[cid]

    def run(pattern):
        eng = clstm_engine(cid, pattern)
        with AF.filled(pattern):
            x = _clstm_inputs(case)[:b].cuda()
            tgt = torch.tensor([r % CR.K for r in range(b)], dtype=torch.int32, device="cuda")
            s = Sequence(eng, pattern)
            _clstm_sequence(s, case, x, b, tgt)
        return s.rec
    _compare(f"clstm {cid} b={b}/B={case.B}", run)


@pytest.mark.parametrize("full", [True, False], ids=["b=B", "b<B"])
@pytest.mark.parametrize("cid", CLSTM_CASES)
def test_clstm_plan(cid, full):
    """S1: odd pooled map (the unpool writes zeros on the dropped row), its own b = 3 < B = 4 is the partial run.
    P2 at b = 64 takes the persistent kernels, at b = 63 the stepwise ones on the same plan."""
    case = CR.CASES[cid]
    _clstm_run(cid, case.B if full else max(1, min(case.b, case.B - 1)))


# ================================================================================================== TF-style plan
TF_CASES = ("X", "A")       # 'valid' with only_last, 'same' on an odd map with b < B


def tf_engine(cid, pattern):
    import ivf_engine
    key = ("tf", cid, pattern)
    if key not in _ENGINES:
        case = TR.CASES[cid]
        w = TR.case_inputs(case)[1]
        with AF.filled(pattern):
            eng = ivf_engine.TFCLSTMEngine(TR.K, (case.C, case.T, case.H, case.W), units=case.units,
                                           kernel=(case.kh, case.kw), stride=case.s, padding=case.pad,
                                           recurrent_activation="hard_sigmoid" if case.hard else "sigmoid",
                                           only_last_element_for_fc=case.only_last, max_batch=case.B)
            eng.load_weights(w["layers"], w["dense_w"], w["dense_b"])
        _ENGINES[key] = eng
    return _ENGINES[key]


def _tf_states(eng, case, b):
    return [eng.layer_state(l, b) for l in range(len(case.units))]


def _tf_sequence(s, case, x, b, tgt):
    eng = s.eng
    T = case.T
    s.call("forward", lambda: eng.forward(x, want_logits=True))
    s.call("backward", lambda: eng.backward(b, tgt), refill=False)
    s.read("backward.states", _tf_states(eng, case, b))
    for l in range(len(case.units)):
        for t, name in zip(eng.layer_state(l, case.B), ("H", "X", "dX")):
            _rows_beyond_b_hold(s, t[b:], f"{name}[{l}]")
    mask = _rand(5, case.B, T)[:b].cuda()
    s.call("perturbed_forward", lambda: eng.perturbed_forward(x, mask))
    raw = ((_rand(7, case.B, T) - 0.3) * 4.0)[:b].cuda().contiguous()
    traj, (m, v, _) = s.call("search", lambda: eng.search(x, tgt, raw, 0.01, 0.02, 3))
    s.read("search.state", (raw, m, v))
    s.read("search.states", _tf_states(eng, case, b))
    for nm in ("frame", "sequence"):
        s.call(f"gradcam({nm})", lambda: eng.gradcam(x, tgt, normalization_mode=nm))
    s.call("gradcam(masked)", lambda: eng.gradcam(x, tgt, mask=mask, out_hw=(7, 9)))


@pytest.mark.parametrize("full", [True, False], ids=["b=B", "b<B"])
@pytest.mark.parametrize("cid", TF_CASES)
def test_tfclstm_plan(cid, full):
    case = TR.CASES[cid]
    b = case.B if full else max(1, min(case.b, case.B - 1))

    def run(pattern):
        eng = tf_engine(cid, pattern)
        with AF.filled(pattern):
            x = TR.case_inputs(case, b=case.B)[0][:b].cuda()
            tgt = torch.tensor([(r + 1) % TR.K for r in range(b)], dtype=torch.int32, device="cuda")
            s = Sequence(eng, pattern)
            _tf_sequence(s, case, x, b, tgt)
        return s.rec
    _compare(f"tfclstm {cid} b={b}/B={case.B}", run)


# ================================================================================================== stand-alone entries
# Through the C-ABI: scratch and every output buffer hold the pattern, the outputs must be byte-equal across the
# patterns, and the bytes around them (and the ones the header says are not written) must still hold the pattern.
GUARD = 256


class Buf:
    """A device buffer of `shape` x `dtype` between two guards, all of it holding the pattern"""

    def __init__(self, pattern, dtype, *shape):
        self.pattern = pattern
        n = int(torch.empty(0, dtype=dtype).element_size())
        for d in shape:
            n *= int(d)
        self.raw = torch.empty(n + 2 * GUARD, dtype=torch.uint8, device="cuda").fill_(pattern)
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(*shape)

    def guards_ok(self):
        return bool((self.raw[:GUARD] == self.pattern).all()) and bool((self.raw[-GUARD:] == self.pattern).all())


def _abi(what, body):
    """body(mk) -> outputs (a tensor / tuple / dict), with mk(dtype, *shape) -> a pattern-filled tensor; once per pattern"""
    import ivf_lib as L

    def run(pattern):
        bufs = []

        def mk(dtype, *shape):
            bufs.append(Buf(pattern, dtype, *shape))
            return bufs[-1].t
        rec = AF.Record()
        rec.add(what, body(mk, L, pattern))
        torch.cuda.synchronize()
        assert all(b.guards_ok() for b in bufs), f"{what} under 0x{pattern:02X}: bytes outside a buffer were written"
        return rec
    _compare(what, run)


def _cl4(mk, g):
    """g [B,C,T,HW] as 16-byte channels-last rows [B,T,HW,4] whose pad lanes hold the pattern"""
    out = mk(torch.float32, g.shape[0], g.shape[2], g.shape[3], 4)
    out[..., :g.shape[1]] = g.permute(0, 2, 3, 1)
    return out


MASK_SHAPES = [(2, 3, 5, 63), (1, 1, 4, 300), (3, 2, 9, 17)]      # B, C, T, HW


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=str)
def test_mask_backwards_do_not_read_their_workspace(shape):
    """ivf_freeze_bwd (dmask entry 0 is 0, with and without dx, both gradient layouts: the pad lane of a 16-byte
    gradient row is ignored), ivf_reverse_bwd and ivf_stfreeze_bwd (dM[:,0] == 0.0 exactly)"""
    B, C, T, HW = shape
    x, g = _rand(1, B, C, T, HW).cuda(), (_rand(2, B, C, T, HW) - 0.5).cuda()
    mask = _rand(3, B, T).cuda()
    M = _rand(4, B, T, HW).cuda()

    def body(mk, L, pattern):
        lib, out = L.lib(), OrderedDict()
        nws = lib.ivf_freeze_bwd_workspace_bytes(B, T)
        partner, weight = mk(torch.int32, B, T), mk(torch.float32, B, T)
        L.check(lib.ivf_submask_pairs_batched(L.ptr(mask), B, T, 0.1, L.ptr(partner), L.ptr(weight), L.stream()))
        out["pairs"] = (partner, weight)
        for cpad in (0, 4):
            gd = g if cpad == 0 else _cl4(mk, g)
            for want_dx in (False, True):
                dmask, ws = mk(torch.float32, B, T), mk(torch.uint8, nws)
                dx = mk(torch.float32, B, C, T, HW) if want_dx else None
                L.check(lib.ivf_freeze_bwd(L.ptr(x), L.ptr(mask), L.ptr(gd), L.ptr(dmask), L.ptr(dx), B, C, T, HW, 1, cpad,
                                           L.ptr(ws), L.stream()))
                assert bool((dmask[:, 0].view(torch.int32) == 0).all()), "freeze_bwd: dmask entry 0"
                out[f"freeze_bwd cpad {cpad} dx {want_dx}"] = (dmask, dx)
            dmask, ws = mk(torch.float32, B, T), mk(torch.uint8, nws)
            L.check(lib.ivf_reverse_bwd(L.ptr(x), L.ptr(partner), L.ptr(gd), L.ptr(dmask), B, C, T, HW, cpad, L.ptr(ws),
                                        L.stream()))
            out[f"reverse_bwd cpad {cpad}"] = dmask
            dM = mk(torch.float32, B, T, HW)
            L.check(lib.ivf_stfreeze_bwd(L.ptr(x), L.ptr(M), L.ptr(gd), L.ptr(dM), B, C, T, HW, cpad, L.stream()))
            assert bool((dM[:, 0].view(torch.int32) == 0).all()), "stfreeze_bwd: dM[:,0] must be +0.0"
            out[f"stfreeze_bwd cpad {cpad}"] = dM
        return out
    _abi(f"freeze_bwd / reverse_bwd / stfreeze_bwd {shape}", body)


@pytest.mark.parametrize("C", [3, 1])
def test_staging_kernels_write_the_pad_lane(C):
    """Every kernel that stages 16-byte input pixels (out_cpad = 4) writes +0.0 into lanes C .. 3 of every pixel."""
    b, T, H, W = 2, 5, 6, 7
    HW = H * W
    x = (_rand(1, b, C, T, HW) * 255.0).cuda()
    mask, M = _rand(3, b, T).cuda(), _rand(4, b, T, HW).cuda()
    alpha = torch.tensor([0.0, 0.25, 1.0]).cuda()
    sigma = torch.tensor([0.5, 0.0]).cuda()
    gt, gh, gw = 2, 2, 3

    def body(mk, L, pattern):
        lib, out = L.lib(), OrderedDict()
        axes = []
        for n_out, n_in in ((H, gh), (W, gw)):
            a = np.empty((n_out, n_in), dtype=np.float32)
            L.check(lib.ivf_stmask_axis_weights(n_out, n_in, 1.0, a.ctypes.data_as(ctypes.c_void_p)))
            axes.append(torch.from_numpy(a).cuda())
        AH, AW = axes

        def staged(label, rows, call):
            p = mk(torch.float32, rows, T, HW, 4)
            L.check(call(p))
            assert bool((p[..., C:].contiguous().view(torch.int32) == 0).all()), f"{label}: pad lanes must be +0.0"
            out[label] = p
        staged("freeze_fwd", b, lambda p: lib.ivf_freeze_fwd(L.ptr(x), L.ptr(mask), L.ptr(p), b, C, T, HW, 1, 4, L.stream()))
        staged("stfreeze_fwd", b, lambda p: lib.ivf_stfreeze_fwd(L.ptr(x), L.ptr(M), L.ptr(p), b, C, T, HW, 4, L.stream()))
        partner, weight = mk(torch.int32, b, T), mk(torch.float32, b, T)
        L.check(lib.ivf_submask_pairs_batched(L.ptr(mask), b, T, 0.1, L.ptr(partner), L.ptr(weight), L.stream()))
        staged("reverse_fwd_batched", b, lambda p: lib.ivf_reverse_fwd_batched(L.ptr(x), L.ptr(partner), L.ptr(weight), L.ptr(p),
                                                                              b, C, T, HW, 4, L.stream()))
        n = lib.ivf_blob_count(T, 2)
        for mode in (0, 1):
            staged(f"blob_stage mode {mode}", n + 1, lambda p: lib.ivf_blob_stage(L.ptr(x), b, C, T, HW, 2, mode, n - 1, n + 1,
                                                                                L.ptr(p), 4, L.stream()))
        for kind, value in ((0, 0.0), (1, 7.0)):
            staged(f"ig_stage kind {kind}", 4, lambda p: lib.ivf_ig_stage(L.ptr(x), kind, None, value, L.ptr(alpha), b, C, T, HW,
                                                                          3, 1, 4, L.ptr(p), 4, L.stream()))
        staged("sg_stage", 3, lambda p: lib.ivf_sg_stage(L.ptr(x), L.ptr(sigma), b, C, T, HW, 2, 5, 1, 3, L.ptr(p), 4, L.stream()))
        nb = lib.ivf_box_count(T, 1, gh, gw, 1, 2)
        staged("box_stage", 4, lambda p: lib.ivf_box_stage(L.ptr(x), b, C, T, H, W, L.ptr(AH), L.ptr(AW), gh, gw, 1, 1, 2, nb - 2,
                                                           4, L.ptr(p), 4, L.stream()))
        staged("rise_stage", 4, lambda p: lib.ivf_rise_stage(L.ptr(x), b, C, T, H, W, L.ptr(AH), L.ptr(AW), gt, gh, gw, 3, 5,
                                                             1 << 31, 1, 4, L.ptr(p), 4, L.stream()))
        bits = torch.tensor([[0x5], [0xA3A], [0x0]], dtype=torch.int32).cuda()
        staged("lin_stage", 5, lambda p: lib.ivf_lin_stage(L.ptr(x), b, C, T, H, W, L.ptr(AH), L.ptr(AW), gt, gh, gw, 3, L.ptr(bits),
                                                           2, 5, L.ptr(p), 4, L.stream()))
        return out
    _abi(f"staging kernels at out_cpad 4, C = {C}", body)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_cam_reduce_and_resize_do_not_read_their_scratch(bf16):
    """ivf_cam_reduce (two chunks of IVF_CAM_CHUNK positions; the weight rows of HiResCAM and LayerCAM, which have no
    weights, are written too: 0), then ivf_cam_resize_normalise (minmax_ws) per slice and per clip."""
    B, npos, C = 2, 2 * 5 * 13, 12                      # [2, 5, 13] slices: 130 positions
    feat, grad = (_rand(1, B, npos, C) - 0.3).cuda(), (_rand(2, B, npos, C) - 0.5).cuda()
    if bf16:
        feat, grad = feat.bfloat16().contiguous(), grad.bfloat16().contiguous()

    def body(mk, L, pattern):
        lib, out = L.lib(), OrderedDict()
        kinds, ids = L.cam_kind_ids(ALL_KINDS)
        w, cam = mk(torch.float32, 5, B, C), mk(torch.float32, 5, B, npos)
        ws = mk(torch.uint8, lib.ivf_cam_ws_bytes(B, npos, C))
        fn = lib.ivf_cam_reduce_bf16 if bf16 else lib.ivf_cam_reduce
        L.check(fn(L.ptr(feat), L.ptr(grad), 5, ids, L.ptr(w), L.ptr(cam), L.ptr(ws), B, npos, C, L.stream()))
        out["cam_reduce"] = (w, cam)
        for k in ("hirescam", "layercam"):
            assert bool((w[kinds.index(k)].view(torch.int32) == 0).all()), f"cam_reduce: weights of {k}"
        for per_frame in (1, 0):
            res, mm = mk(torch.float32, B, 2 * 3, 9, 11), mk(torch.float32, B, 2, 2)
            L.check(lib.ivf_cam_resize_normalise(L.ptr(cam[0]), L.ptr(res), L.ptr(mm), B, 2, 5, 13, 9, 11, 3, per_frame,
                                                 L.stream()))
            out[f"resize per_frame {per_frame}"] = res
        return out
    _abi(f"cam_reduce{'_bf16' if bf16 else ''} + cam_resize_normalise", body)


def test_viz_blend_does_not_read_frame_max():
    T, H, W = 2, 5, 7
    clip, pert = (_rand(1, 3, T, H, W) * 255.0).cuda(), (_rand(2, 3, T, H, W) * 255.0).cuda()
    cam = _rand(3, T, H, W).cuda()
    lut = (torch.arange(768) % 251).to(torch.uint8).view(256, 3).cuda()

    def body(mk, L, pattern):
        fmax, out = mk(torch.float32, T), mk(torch.uint8, T, H, 3 * W, 3)
        L.check(L.lib().ivf_viz_blend(L.ptr(clip), L.ptr(cam), L.ptr(pert), L.ptr(lut), L.ptr(fmax), L.ptr(out), T, H, W,
                                      L.stream()))
        return out, fmax
    _abi("viz_blend", body)


@pytest.mark.parametrize("kind", ["kernelshap", "lime"])
def test_lin_moments_and_solve_do_not_read_their_work(kind):
    """ivf_lin_moments -> ivf_lin_solve -> ivf_lin_fit through _Engine.lin_solve: its factor workspace comes from
    ivf_engine._arena and every moment and output from torch.empty, all of which hold the pattern here.  P = 70: three
    words of bits, two column blocks of the factorisation."""
    import ivf_engine
    grid, n, b = (2, 5, 7), 96, 3
    P = grid[0] * grid[1] * grid[2]
    scores, score_x = _rand(1, b, n + 1).cuda(), (_rand(2, b) + 1.0).cuda()
    eng = clstm_engine("S4", AF.BASELINE)

    def run(pattern):
        with AF.filled(pattern):
            bits = eng.kshap_rows(n, grid, seed=3)[0] if kind == "kernelshap" else eng.lime_rows(n, 0.5, grid, seed=3)
            wtab = None if kind == "kernelshap" else ivf_engine._Engine.lime_weight_table(P)
            rec = AF.Record()
            rec.add("rows", bits)
            rec.add("lin_solve", eng.lin_solve(kind, scores, score_x, bits, P, wtab, 0.0 if kind == "kernelshap" else 1.0))
        return rec
    _compare(f"lin_moments + lin_solve + lin_fit {kind} P={P}", run)


PACK_MODES = ("fp32", "bf16x3", "bf16x6", "bf16act")


@pytest.mark.parametrize("mode", PACK_MODES)
def test_weight_packs_write_every_element(mode):
    """ivf_conv3d_pack_fwd / _pack_bwd / _pack_bwd_fused1x1 into a filled destination at K % 8 == 4 (forward rows of
    9 taps x CinPad 4 = 36, backward rows of 9 taps x Cout 4 = 36, fused rows of Ktotal 12): every one of the
    *_elems() floats is written, the same under every pattern, in either order of the fused units."""
    import ivf_lib as LL
    mm = LL.MATH_MODES[mode]
    cout, cin, cinp, k = 4, 3, 4, (1, 3, 3)
    w = (_rand(1, cout, cin, *k) - 0.5).cuda()
    scale = (_rand(2, cout) + 0.5).cuda()
    units = [(4, (_rand(3, 4, cin, 1, 1, 1) - 0.5).cuda(), (_rand(4, 4) + 0.5).cuda()),
             (8, (_rand(5, 8, cin, 1, 1, 1) - 0.5).cuda(), (_rand(6, 8) + 0.5).cuda())]

    def body(mk, L, pattern):
        lib, out = L.lib(), OrderedDict()
        nf = lib.ivf_conv3d_pack_fwd_elems(cout, cinp, *k, mm)
        pf = mk(torch.float32, nf)
        L.check(lib.ivf_conv3d_pack_fwd(L.ptr(w), L.ptr(pf), cout, cin, cinp, *k, mm, L.stream()))
        out["pack_fwd"] = pf
        nb = lib.ivf_conv3d_pack_bwd_elems(cout, cinp, *k, 1, 1, 1, 0, 1, 1, mm)
        pb, geom = mk(torch.float32, nb), L.BwdGeom()
        L.check(lib.ivf_conv3d_pack_bwd(L.ptr(w), L.ptr(scale), L.ptr(pb), cout, cin, cinp, *k, 1, 1, 1, 0, 1, 1, mm, geom,
                                        L.stream()))
        out["pack_bwd"] = pb
        nu = lib.ivf_conv3d_pack_bwd_fused1x1_elems(12, cinp, mm)
        for order in ((0, 1), (1, 0)):
            pu = mk(torch.float32, nu)
            for u in order:
                co, wu, su = units[u]
                L.check(lib.ivf_conv3d_pack_bwd_fused1x1(L.ptr(wu), L.ptr(su), L.ptr(pu), co, cin, cinp, 4 * u, 12, mm,
                                                         L.stream()))
            out[f"pack_bwd_fused1x1 order {order}"] = pu
        return out
    _abi(f"weight packs {mode}", body)
