"""GPU: the Grad-CAM family (csrc/cam_ops.hip) -- the reductions directly on the synthetic cases of
tests/cam_refs.py in both storages and both layouts, on the I3D and ConvLSTM plans against the fp64 restatement of the
buffers the plans themselves read, and through GradCamVideo and the find_masks driver.  Every comparison with fp64 uses
the derived gate of cam_refs.bounds (measured / bound <= 1); what has to be equal is compared bit for bit."""
import ctypes
import functools
import pickle

import numpy as np
import pytest
import torch

import cam_refs as R
import i3d_refs as IR
from conftest import note

pytestmark = pytest.mark.gpu

NAN = float("nan")
CH = 128                                             # IVF_CAM_CHUNK (asserted below)
SHAPES = [(1, 1, 1), (2, 8, 1024), (3, 2040, 64), (2, 540, 480), (1, 65, 6), (2, 257, 68)] + \
    [(1, n, 64) for n in (63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1)]


def bits(t):
    return t.contiguous().view(torch.int32)


def _dev(a, bf16):
    if bf16:
        return torch.from_numpy(R.to_bf16_bits(a).view(np.int16)).cuda()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def case(shape, seed=11, signed=False):
    """(A, G, per-clip fp64 family, per-clip bounds) of a synthetic case, computed once"""
    A, G = R.synth(*shape, seed=seed + 13 * shape[1] + shape[2], signed=signed)
    return A, G, [R.family(A[b], G[b]) for b in range(shape[0])], [R.bounds(A[b], G[b]) for b in range(shape[0])]


def reduce_i3d(A, G, kinds, bf16=False, want_w=True):
    """ivf_cam_reduce{,_bf16} -> (weights [n,B,C] or None, cam [n,B,npos]) device tensors; scratch and outputs start as NaN"""
    import ivf_lib as L
    lib = L.lib()
    B, npos, C = A.shape
    names, ids = L.cam_kind_ids(kinds)
    fa, ga = _dev(A, bf16), _dev(G, bf16)
    ws = torch.full((lib.ivf_cam_ws_bytes(B, npos, C),), 255, dtype=torch.uint8, device="cuda")
    w = torch.full((len(names), B, C), NAN, device="cuda") if want_w else None
    cam = torch.full((len(names), B, npos), NAN, device="cuda")
    fn = lib.ivf_cam_reduce_bf16 if bf16 else lib.ivf_cam_reduce
    L.check(fn(L.ptr(fa), L.ptr(ga), len(names), ids, L.ptr(w), L.ptr(cam), L.ptr(ws), B, npos, C, L.stream()))
    torch.cuda.synchronize()
    return w, cam


def check(kinds, w, cam, fam, bnd, what):
    """every kind of every clip against the gate; returns the worst measured / bound"""
    worst = 0.0
    for i, k in enumerate(kinds):
        for b in range(cam.shape[1]):
            ew = R.excess(w[i, b].cpu().numpy(), fam[b][k]["w"], bnd[b][k]["w"]) if w is not None else 0.0
            ec = R.excess(cam[i, b].cpu().numpy().reshape(-1), fam[b][k]["cam"], bnd[b][k]["cam"])
            assert ew <= 1 and ec <= 1, f"{what} {k} clip {b}: weights {ew:.3g}, map {ec:.3g} of the bound"
            worst = max(worst, ew, ec)
    return worst


# ------------------------------------------------------------------------------------------------ 1-4: the kernels
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reduce_matches_fp64_every_kind_alone_and_together(shape, bf16):
    import ivf_lib as L
    assert L.CAM_CHUNK == CH
    A, G, fam, bnd = case(shape)
    worst = 0.0
    for kinds in [(k,) for k in R.KINDS] + [R.KINDS]:
        w, cam = reduce_i3d(A, G, kinds, bf16)
        worst = max(worst, check(kinds, w, cam, fam, bnd, f"{shape} bf16={bf16}"))
        for i, k in enumerate(kinds):
            if k in ("hirescam", "layercam"):
                assert not bits(w[i]).any(), "weights rows of the layer-local kinds are zero"
            if shape[2] >= 4:
                if k == "xgradcam":
                    assert not bits(w[i][:, 1]).any(), "all-zero channel: XGrad-CAM weight 0"
                if k == "gradcam++":
                    assert not bits(w[i][:, 2]).any(), "G <= 0 channel: Grad-CAM++ weight 0"
    _, cam = reduce_i3d(A, G, R.KINDS, bf16, want_w=False)                 # weights may be NULL
    _, cam5 = reduce_i3d(A, G, R.KINDS, bf16)
    assert torch.equal(bits(cam), bits(cam5))
    note(f"cam reduce {shape} {'bf16' if bf16 else 'fp32'}: worst measured/bound {worst:.3f}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 2040, 64), (2, 257, 68), (1, 65, 6)], ids=lambda s: "x".join(map(str, s)))
def test_kind_0_is_bit_equal_to_gradcam_reduce(shape, bf16):
    import ivf_lib as L
    A, G, _, _ = case(shape)
    B, npos, C = shape
    w, cam = reduce_i3d(A, G, ("xgradcam", "gradcam"), bf16)
    fa, ga = _dev(A, bf16), _dev(G, bf16)
    w0, cam0 = torch.full((B, C), NAN, device="cuda"), torch.full((B, npos), NAN, device="cuda")
    fn = L.lib().ivf_gradcam_reduce_bf16 if bf16 else L.lib().ivf_gradcam_reduce
    L.check(fn(L.ptr(fa), L.ptr(ga), L.ptr(w0), L.ptr(cam0), B, npos, C, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(w[1]), bits(w0)) and torch.equal(bits(cam[1]), bits(cam0))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 2040, 64), (3, 300, 6)], ids=lambda s: "x".join(map(str, s)))
def test_rows_do_not_depend_on_the_batch_or_on_the_other_kinds(shape, bf16):
    A, G, _, _ = case(shape)
    w5, cam5 = reduce_i3d(A, G, R.KINDS, bf16)
    for row in (0, 2):
        w1, cam1 = reduce_i3d(A[row:row + 1], G[row:row + 1], R.KINDS, bf16)
        assert torch.equal(bits(w1[:, 0]), bits(w5[:, row])) and torch.equal(bits(cam1[:, 0]), bits(cam5[:, row]))
    for i, k in enumerate(R.KINDS):
        w1, cam1 = reduce_i3d(A, G, (k,), bf16)
        assert torch.equal(bits(w1[0]), bits(w5[i])) and torch.equal(bits(cam1[0]), bits(cam5[i])), k
    order = ("layercam", "gradcam++", "gradcam")                          # rows follow the order of the list
    w3, cam3 = reduce_i3d(A, G, order, bf16)
    for i, k in enumerate(order):
        assert torch.equal(bits(cam3[i]), bits(cam5[R.KIND_ID[k]])) and torch.equal(bits(w3[i]), bits(w5[R.KIND_ID[k]]))


def test_bad_arguments_are_refused():
    import ivf_lib as L
    lib = L.lib()
    A, G, _, _ = case((1, 65, 6))
    fa, ga = _dev(A, False), _dev(G, False)
    ws = torch.empty(lib.ivf_cam_ws_bytes(1, 65, 6), dtype=torch.uint8, device="cuda")
    w, cam = torch.full((5, 1, 6), NAN, device="cuda"), torch.full((5, 1, 65), NAN, device="cuda")

    def call(kinds, n, cam_t=cam, fn=lib.ivf_cam_reduce):
        arr = (ctypes.c_int * len(kinds))(*kinds)
        return fn(L.ptr(fa), L.ptr(ga), n, arr, L.ptr(w), L.ptr(cam_t), L.ptr(ws), 1, 65, 6, L.stream())
    for fn in (lib.ivf_cam_reduce, lib.ivf_cam_reduce_bf16):
        for kinds, n, cam_t in (([7], 1, cam), ([1, 1], 2, cam), ([0, 1, 2, 3, 4, 0], 0, cam),
                                ([0, 1, 2, 3, 4, 0], 6, cam), ([3], 1, None), ([-1], 1, cam)):
            assert call(kinds, n, cam_t, fn) == -1 and len(lib.ivf_last_error()) > 0, (kinds, n)
    one = (ctypes.c_int * 1)(9)
    assert lib.ivf_clstm_cam_reduce(L.ptr(fa), L.ptr(ga), None, 1, 1, one, None, L.ptr(cam), 1, 1, 6, 65, L.stream()) == -1
    assert len(lib.ivf_last_error()) > 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(cam).all()) and bool(torch.isnan(w).all()), "a refused call launches nothing"


# ------------------------------------------------------------------------------------------------ 5: the I3D plan
_ENGINES = {}


def i3d_engine(cid, mode):
    import ivf_engine
    if (cid, mode) not in _ENGINES:
        c = IR.CASES[cid]
        eng = ivf_engine.I3DEngine(IR.NUM_CLASSES, c.clip, max_batch=IR.MAX_BATCH, softmax=True, math=mode, **c.engine)
        eng.load_state_dict(IR.state_dict(c), autotune=False)
        _ENGINES[(cid, mode)] = eng
    return _ENGINES[(cid, mode)]


@pytest.mark.parametrize("layer", ["Conv3d_1a_7x7", "Mixed_3c", "Mixed_4f", "Mixed_5c"])
@pytest.mark.parametrize("cid,mode", [("odd", "fp32"), ("odd", "bf16x6"), ("odd", "bf16act"), ("gray", "fp32"),
                                      ("gray", "bf16act")])
def test_i3d_plan(cid, mode, layer):
    import ivf_lib as L
    c = IR.CASES[cid]
    eng = i3d_engine(cid, mode)
    x = IR.clips(c).cuda()
    C, T, H, W = c.clip
    tgt = eng.argmax(eng.forward(x))
    raw = eng.cam_raw(x, tgt, kinds=R.KINDS, layer=layer)
    feat, grad = raw["feat"], raw["grad"]
    assert torch.equal(feat, eng.endpoint(layer, 3).permute(0, 2, 3, 4, 1).contiguous())
    if layer != "Mixed_5c":
        assert torch.equal(grad, eng.endpoint(layer + ":grad", 3).permute(0, 2, 3, 4, 1).contiguous())
    b, Tf, Hf, Wf, Cf = feat.shape
    A, G = feat.reshape(3, -1, Cf).cpu().numpy(), grad.reshape(3, -1, Cf).cpu().numpy()
    assert np.isfinite(A).all() and np.isfinite(G).all() and np.abs(G).max() > 0
    fam, bnd = [R.family(A[i], G[i]) for i in range(3)], [R.bounds(A[i], G[i]) for i in range(3)]
    w = torch.stack([raw[k]["weights"] for k in R.KINDS])
    cam = torch.stack([raw[k]["cam"] for k in R.KINDS])
    worst = check(R.KINDS, w, cam, fam, bnd, f"{cid} {mode} {layer}")
    # the Grad-CAM entry is Grad-CAM's, and the final maps are the resize of the raw ones, bit for bit
    want, probs = eng.gradcam(x, tgt, layer=layer)
    maps, probs2 = eng.cam(x, tgt, kinds=R.KINDS, layer=layer)
    assert torch.equal(bits(maps["gradcam"]), bits(want)) and torch.equal(probs, probs2) and torch.equal(probs, raw["probs"])
    step = T // Tf
    for k in R.KINDS:
        out = torch.full((3, Tf * step, H, W), NAN, device="cuda")
        mm = torch.empty(3 * Tf * 2, device="cuda")
        L.check(L.lib().ivf_cam_resize_normalise(L.ptr(raw[k]["cam"].contiguous()), L.ptr(out), L.ptr(mm), 3, Tf, Hf, Wf, H,
                                                 W, step, 1, L.stream()))
        torch.cuda.synchronize()
        assert maps[k].shape == out.shape and torch.equal(bits(maps[k]), bits(out)), k
    one, _ = eng.cam(x[1:2].contiguous(), tgt[1:2], kinds=("layercam",), layer=layer)      # a row alone, one kind
    assert torch.equal(bits(one["layercam"][0]), bits(maps["layercam"][1]))
    note(f"cam i3d {cid} {mode} {layer}: map {Tf}x{Hf}x{Wf}x{Cf}, worst measured/bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 6: ConvLSTM
CT, EFF = 32, [7, 15, 23, 31]


@pytest.mark.parametrize("signed", [False, True], ids=["post-relu", "signed"])
@pytest.mark.parametrize("hid,plane", [(1, 7), (4, 35), (4, 1200), (32, 70), (32, 299)])
def test_clstm_reduce_matches_fp64(hid, plane, signed):
    import ivf_lib as L
    lib = L.lib()
    B = 2
    for steps in (None, EFF, [5]):
        sel = list(range(CT)) if steps is None else steps
        n = len(sel)
        feat, grad = R.synth_clstm(B, CT, hid, plane, sel, seed=hid * 100 + plane + n, signed=signed)
        A = [R.clstm_positions(feat[b], sel) for b in range(B)]
        G = [R.clstm_positions(grad[b], sel) for b in range(B)]
        fam, bnd = [R.family(a, g) for a, g in zip(A, G)], [R.bounds(a, g) for a, g in zip(A, G)]
        f, g = torch.from_numpy(feat).cuda(), torch.from_numpy(grad).cuda()
        arr = (ctypes.c_int * n)(*sel) if steps is not None else None
        res = {}
        for kinds in [R.KINDS] + [(k,) for k in R.KINDS]:
            names, ids = L.cam_kind_ids(kinds)
            w = torch.full((len(kinds), B, hid), NAN, device="cuda")
            cam = torch.full((len(kinds), B, n, plane), NAN, device="cuda")
            L.check(lib.ivf_clstm_cam_reduce(L.ptr(f), L.ptr(g), arr, n, len(kinds), ids, L.ptr(w), L.ptr(cam), B, CT, hid,
                                             plane, L.stream()))
            torch.cuda.synchronize()
            check(kinds, w, cam, fam, bnd, f"clstm hid {hid} plane {plane} steps {steps}")
            res[kinds] = (w, cam)
        w5, cam5 = res[R.KINDS]
        for i, k in enumerate(R.KINDS):                                   # a kind alone equals its slice; zero rows
            assert torch.equal(bits(res[(k,)][0][0]), bits(w5[i])) and torch.equal(bits(res[(k,)][1][0]), bits(cam5[i]))
        assert not bits(w5[3:]).any()
        w0, cam0 = torch.full((B, hid), NAN, device="cuda"), torch.full((B, n, plane), NAN, device="cuda")
        L.check(lib.ivf_clstm_gradcam_reduce(L.ptr(f), L.ptr(g), arr, n, L.ptr(w0), L.ptr(cam0), B, CT, hid, plane,
                                             L.stream()))
        names, ids = L.cam_kind_ids(("hirescam",))                         # weights may be NULL without kind 0
        cam3 = torch.full((1, B, n, plane), NAN, device="cuda")
        L.check(lib.ivf_clstm_cam_reduce(L.ptr(f), L.ptr(g), arr, n, 1, ids, None, L.ptr(cam3), B, CT, hid, plane,
                                         L.stream()))
        f1, g1 = f[1:2].contiguous(), g[1:2].contiguous()                  # and a clip alone equals its row
        names, ids = L.cam_kind_ids(R.KINDS)
        w1, cam1 = torch.full((5, 1, hid), NAN, device="cuda"), torch.full((5, 1, n, plane), NAN, device="cuda")
        L.check(lib.ivf_clstm_cam_reduce(L.ptr(f1), L.ptr(g1), arr, n, 5, ids, L.ptr(w1), L.ptr(cam1), 1, CT, hid, plane,
                                         L.stream()))
        torch.cuda.synchronize()
        assert torch.equal(bits(w0), bits(w5[0])) and torch.equal(bits(cam0), bits(cam5[0]))
        assert torch.equal(bits(cam3[0]), bits(cam5[3]))
        assert torch.equal(bits(w1[:, 0]), bits(w5[:, 1])) and torch.equal(bits(cam1[:, 0]), bits(cam5[:, 1]))


@pytest.fixture(scope="module")
def clstm_engine():
    import ivf_engine
    import ivf_recipe as RC
    eng = ivf_engine.CLSTMEngine(6, (3, CT, 120, 160), max_batch=2, hidden=4, layers=2, kernel=5, stride=2, softmax=True,
                                 out_step=EFF[-1], out_steps=EFF, effective_steps=EFF)
    eng.load_state_dict(RC.clstm_state_dict(channels=3, tag='clstm3', fc_mult=4))
    return eng


@pytest.mark.parametrize("name,layer", [("clstm", None), ("cell0", 0), ("cell1", 1)])
def test_clstm_plan(clstm_engine, name, layer):
    import ivf_recipe as RC
    eng = clstm_engine
    x = torch.from_numpy(np.stack([RC.clip(c, 3, CT, 120, 160) for c in (7, 8)]) / 255.0).float().cuda()
    raw = eng.cam_raw(x, None, kinds=R.KINDS, layer=layer)
    old = eng.gradcam_raw(x, None, layer=layer)
    assert torch.equal(raw["feat"], old["feat"]) and torch.equal(raw["grad"], old["grad"])
    assert torch.equal(bits(raw["gradcam"]["cam"]), bits(old["cam"]))
    assert torch.equal(bits(raw["gradcam"]["weights"]), bits(old["weights"]))
    b, n, hid, Hp, Wp = raw["feat"].shape
    assert n == (len(EFF) if layer is None else CT)
    feat, grad = raw["feat"].cpu().numpy(), raw["grad"].cpu().numpy()
    A = [R.clstm_positions(feat[i], range(n)) for i in range(b)]
    G = [R.clstm_positions(grad[i], range(n)) for i in range(b)]
    assert all(np.abs(g).max() > 0 for g in G)
    # the maps are post-BN and signed: a Grad-CAM++ denominator 2 + s_k G may come within the error of s_k of 0, and
    # that channel's weight then has no forward bound; every other kind is gated on every element
    fam = [R.family(a, g) for a, g in zip(A, G)]
    bnd = [R.bounds(a, g, singular="inf") for a, g in zip(A, G)]
    open_w = sum(int(np.isinf(q["gradcam++"]["w"]).sum()) for q in bnd)
    assert all(np.isfinite(q[k][e]).all() for q in bnd for k in R.KINDS if k != "gradcam++" for e in ("w", "cam"))
    w = torch.stack([raw[k]["weights"] for k in R.KINDS])
    cam = torch.stack([raw[k]["cam"] for k in R.KINDS])
    worst = check(R.KINDS, w, cam, fam, bnd, f"clstm plan {name}")
    note(f"cam clstm plan {name}: {open_w} of {b * hid} Grad-CAM++ weights without a forward bound")
    maps, probs = eng.cam(x, None, kinds=R.KINDS, layer=layer, out_hw=(60, 80))
    want, _ = eng.gradcam(x, None, out_hw=(60, 80), layer=layer)
    assert torch.equal(bits(maps["gradcam"]), bits(want)) and torch.equal(probs, raw["probs"])
    assert all(maps[k].shape == (2, CT, 60, 80) for k in R.KINDS)
    note(f"cam clstm plan {name}: {n} maps {Hp}x{Wp}, worst measured/bound {worst:.3f}")


@pytest.mark.parametrize("softmax", [0, 1])
@pytest.mark.parametrize("entire", [0, 1])
def test_clstm_parity_with_the_reference_models_activations(entire, softmax, golden):
    """tests/golden/clstm_gradcam.npz holds the top layer's features and the gradient torch autograd left on them in
    the reference's CLSTM_4.Model: every kind of target 'clstm' on the plan against the fp64 restatement of THOSE
    arrays, under the project's Grad-CAM gate (1e-3 by conftest.rel_err on weights and raw maps)."""
    import ivf_engine
    import ivf_recipe as RC
    from conftest import rel_err
    g = golden("clstm_gradcam")
    eng = ivf_engine.CLSTMEngine(6, (3, CT, 120, 160), max_batch=1, hidden=4, layers=2, kernel=5, stride=2,
                                 softmax=bool(softmax), out_step=EFF[-1], out_steps=EFF if entire else None,
                                 effective_steps=EFF)
    eng.load_state_dict(RC.clstm_state_dict(channels=3, tag='clstm3', fc_mult=4 if entire else 1))
    x = torch.from_numpy(RC.clip(7, 3, CT, 120, 160) / 255.0).float()[None].cuda()
    raw = eng.cam_raw(x, None, kinds=R.KINDS, layer=None)
    A = R.clstm_positions(g["cell1_feat"][EFF], range(4))
    G = R.clstm_positions(g[f"e{entire}_s{softmax}_clstm_grad"], range(4))
    fam = R.family(A, G)
    errs = {}
    for k in R.KINDS:
        errs[k + " map"] = rel_err(raw[k]["cam"][0].cpu().numpy().reshape(-1), fam[k]["cam"])
        if k in R.WEIGHTED:
            errs[k + " w"] = rel_err(raw[k]["weights"][0].cpu().numpy(), fam[k]["w"])
    note(f"cam clstm reference parity e{entire} s{softmax}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 1e-3, f"e{entire} s{softmax}: {k} off by {v:.3e}"


# ------------------------------------------------------------------------------------------------ 7: golden parity
def _golden_case(g, key, raw, maps, sub, what):
    """the project's Grad-CAM gates: 1e-3 by conftest.rel_err on probabilities, weights and raw maps, 1e-3 absolute on
    the normalised maps (NaN pattern equal); the reference's own fp32-vs-fp64 spread is noted beside the measured error"""
    from conftest import rel_err
    assert int(raw["probs"][0].argmax()) == int(g[key + "_index"])
    errs = {"probs": rel_err(raw["probs"].cpu().numpy(), g[key + "_probs"].reshape(1, -1))}
    for k in R.KINDS:
        if k in R.WEIGHTED:
            errs[k + " w"] = rel_err(raw[k]["weights"][0].cpu().numpy(), g[f"{key}_{k}_w"])
        errs[k + " raw"] = rel_err(raw[k]["cam"][0].cpu().numpy()[sub], g[f"{key}_{k}_cam"])
        for pf in (1, 0):
            got, want = maps[pf][k][0].cpu().numpy()[::4, ::8, ::8], g[f"{key}_{k}_pf{pf}"]
            assert np.array_equal(np.isnan(got), np.isnan(want)), (key, k, pf)
            ok = ~np.isnan(want)
            errs[f"{k} pf{pf}"] = float(np.abs(got - want)[ok].max()) if ok.any() else 0.0
        note(f"cam golden {what} {key} {k}: reference fp32-vs-fp64 spread (w, raw, normalised) "
             + " ".join(f"{v:.1e}" for v in g[f"{key}_{k}_spread"]))
    note(f"cam golden {what} {key}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 1e-3, f"{key}: {k} off by {v:.3e}"


@pytest.fixture(scope="module")
def kth_i3d():
    import ivf_engine
    import ivf_recipe as RC
    # plain fp32 arithmetic: the layer-local kinds see the gradient position by position, and a max-pool near-tie that
    # the split-bf16 modes' 1e-4 forward error breaks the other way moves gradient between positions (the channel means
    # of Grad-CAM do not notice, test_gpu_i3d.py::test_gradcam_other_target_layers)
    eng = ivf_engine.I3DEngine(6, (3, CT, 120, 160), max_batch=1, head_hw=(4, 5), head_time_base=4, softmax=False,
                               math="fp32")
    eng.load_state_dict(RC.i3d_state_dict(num_classes=6, tag='i3d_kth'), autotune=False)
    return eng


@pytest.mark.parametrize("layer", ["Mixed_4f", "Mixed_5b", "Mixed_5c"])
def test_golden_parity_i3d(kth_i3d, layer, golden):
    import ivf_recipe as RC
    g = golden("cam_family")
    x = torch.from_numpy(RC.clip(11, 3, CT, 120, 160))[None].cuda()
    raw = kth_i3d.cam_raw(x, None, kinds=R.KINDS, layer=layer)
    tgt = [int(g[f"i3d_s0_{layer}_index"])]
    maps = {pf: kth_i3d.cam(x, tgt, kinds=R.KINDS, per_frame=bool(pf), out_hw=(120, 160), layer=layer)[0] for pf in (1, 0)}
    _golden_case(g, f"i3d_s0_{layer}", raw, maps, (slice(None, None, 2),) * 3, "i3d")


@pytest.mark.parametrize("name,layer", [("clstm", None), ("cell1", 1)])
@pytest.mark.parametrize("softmax", [0, 1])
def test_golden_parity_clstm(softmax, name, layer, golden):
    import ivf_engine
    import ivf_recipe as RC
    g = golden("cam_family")
    eng = ivf_engine.CLSTMEngine(6, (3, CT, 120, 160), max_batch=1, hidden=4, layers=2, kernel=5, stride=2,
                                 softmax=bool(softmax), out_step=EFF[-1], effective_steps=EFF)
    eng.load_state_dict(RC.clstm_state_dict(channels=3, tag='clstm3'))
    x = torch.from_numpy(RC.clip(7, 3, CT, 120, 160) / 255.0).float()[None].cuda()
    raw = eng.cam_raw(x, None, kinds=R.KINDS, layer=layer)
    tgt = [int(g[f"clstm_s{softmax}_{name}_index"])]
    maps = {pf: eng.cam(x, tgt, kinds=R.KINDS, per_frame=bool(pf), out_hw=(120, 160), layer=layer)[0] for pf in (1, 0)}
    _golden_case(g, f"clstm_s{softmax}_{name}", raw, maps, (slice(None),) * 3, "clstm")


# ------------------------------------------------------------------------------------------------ 8-9: public surface
@pytest.fixture(scope="module")
def smth_model():
    import ivf_recipe as RC
    from models import I3D_doubled
    m = I3D_doubled.Model(174, last_stride=1, stride_mod_layers="", softMax=1)
    m.load_state_dict(RC.to_torch(RC.i3d_state_dict(num_classes=174)))
    return m.cuda().eval()


def test_gradcam_video_takes_a_kind(smth_model):
    import ivf_lib as L
    import ivf_recipe as RC
    from grad_cam_videos import GradCamVideo
    x = torch.from_numpy(RC.clip(21))[None]
    lc, out = GradCamVideo(smth_model, ["Mixed_3c"], None, True, 224, True, kind="layercam")(x)
    assert lc.shape == (16, 224, 224) and lc.dtype == np.float32 and tuple(out.shape) == (1, 174)
    eng = smth_model._engine_for(x.cuda())
    maps, probs = eng.cam(x.cuda(), [int(out[0].argmax())], kinds=("layercam",), per_frame=True, out_hw=(224, 224),
                          layer="Mixed_3c")
    assert np.array_equal(lc.view(np.uint32), maps["layercam"][0].cpu().numpy().view(np.uint32))
    plain, _ = GradCamVideo(smth_model, ["Mixed_5c"], None, True, 224, True)(x)
    named, _ = GradCamVideo(smth_model, ["Mixed_5c"], None, True, 224, True, kind="gradcam")(x)
    assert np.array_equal(plain.view(np.uint32), named.view(np.uint32))
    with pytest.raises(L.IvfError, match="gradcam, gradcam\\+\\+, xgradcam, hirescam, layercam"):
        GradCamVideo(smth_model, ["Mixed_5c"], None, True, 224, True, kind="scorecam")


def test_driver_writes_the_family_and_ranks_it(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)
    hp = {"batch_size": 2, "gradCamType": "guessed"}
    drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "freeze", classOI=None, doGradCam=True,
                   runTempMask=False, verbose=False, doCurves=True, curveStep=8, camKinds=("gradcam++", "layercam"),
                   camTarget="Mixed_3c")
    fam = pickle.load(open(tmp_path / "results" / "allCamFamilyResults_run0_None_.p", "rb"))
    gc = pickle.load(open(tmp_path / "results" / "allGradCamResults_run0_None_.p", "rb"))
    cv = pickle.load(open(tmp_path / "results" / "allCurvesResults_run0_None_.p", "rb"))
    assert len(fam) == len(gc) == len(cv) == 2
    for rec, g, c in zip(fam, gc, cv):
        assert set(rec) == {"true_class", "pred_class", "video_id", "gradcam++", "layercam"}
        assert (rec["video_id"], rec["pred_class"]) == (g["video_id"], g["pred_class"])
        for k in ("gradcam++", "layercam"):
            assert rec[k].shape == (16, 224, 224) and rec[k].dtype == np.float32
            assert set(c[k]) >= {"ranks", "deletion", "insertion", "del_auc", "ins_auc"} and c[k]["deletion"].shape == (3,)
        assert "gradcam" in c and "xgradcam" not in c
        assert not np.array_equal(rec["layercam"], g["GCHeatMap"])


def test_files_are_the_same_without_extra_kinds(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    runs = []
    for sub, extra in (("plain", {}), ("kwargs", dict(camKinds=(), camTarget="Mixed_3c")),
                       ("same", dict(camKinds=("hirescam",)))):
        d = tmp_path / sub
        d.mkdir()
        monkeypatch.chdir(d)
        loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 16, 224, 224), 174, first_id=40)
        drv.find_masks(loader, smth_model, {"batch_size": 1, "gradCamType": "guessed"}, 0.01, 0.02, 2, "central",
                       "freeze", classOI=None, doGradCam=True, runTempMask=False, verbose=False, **extra)
        files = sorted(str(q.relative_to(d)) for q in d.rglob("*") if q.is_file())
        runs.append((files, pickle.load(open(d / "results" / "allGradCamResults_run0_None_.p", "rb"))))
    assert runs[0][0] == runs[1][0] and not any("CamFamily" in f for f in runs[0][0])
    assert [f for f in runs[2][0] if f not in runs[0][0]] == ["results/allCamFamilyResults_run0_None_.p"]
    for files, recs in runs[1:]:          # Grad-CAM from the family's shared passes is Grad-CAM, bit for bit
        assert np.array_equal(recs[0]["GCHeatMap"].view(np.uint32), runs[0][1][0]["GCHeatMap"].view(np.uint32))
