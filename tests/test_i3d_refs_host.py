"""CPU proof of tests/i3d_refs.py: the op-wise restatement IS the reference network (chained in fp64 it reproduces
oracle.i3d_ref and fp64 autograd), the cases contain what their table claims, the floors are finite and bounded, and
every wiring mutant sits at least MUTANT_DISTANCE gates away.  No GPU, no HIP library."""
import math

import pytest
import torch

import i3d_refs as R
from conftest import note

CASE_IDS = list(R.CASES)


def _oracle_kwargs(case):
    sml, ls = R.stride_mod(case)
    return dict(stride_mod_layers=sml, last_stride=ls)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_chained_restatement_is_the_reference_network(cid):
    """mode 'exact' (fp64 fold, no planes, no storage rounding), each op reading the op before it: every endpoint,
    the logits, the probabilities and dx equal oracle.i3d_ref on a float64 state dict and its autograd, to fp64
    rounding, for a dense dout and for arg-max targets.  The clips carry a seeded fraction per pixel, and no window of
    the pools that read a convolution with taps (2a, 3a) has two equal positive maxima.  Further up equal maxima are
    structural and no perturbation of the clip removes them: the module pools of Mixed_3b / 4b / 5b read a pool's
    output, where neighbouring cells hold the same source value, and on maps of a few positions the stride-1 pool's
    windows coincide, so b3b's outputs are equal cell by cell.  They are counted for the record; both sides take the
    first cell in scan order there (test_gpu_pool_blocks.test_numpy_rule_matches_reference_goldens), which the equality
    of dx below confirms."""
    import ivf_recipe as recipe
    from oracle import i3d_ref
    case = R.CASES[cid]
    x = R.untied_clips(case)
    sd = {k: v.double() for k, v in recipe.to_torch(R.state_dict(case)).items()}
    fres, bufs = R.forward(case, "exact", x)
    xin = x.clone().requires_grad_()
    eps = {}
    feat = i3d_ref.features(xin, sd, endpoints=eps, **_oracle_kwargs(case))
    logits, probs = i3d_ref.head(feat, sd, R.head_window(case), True)
    logits, probs = logits.reshape(3, -1), probs.reshape(3, -1)
    for name, v in eps.items():
        scale = float(v.detach().abs().max())
        assert float((bufs[name] - v.detach()).abs().max()) <= 1e-12 * scale, name
    assert float((bufs["logits"] - logits.detach()).abs().max()) <= 1e-12 * float(logits.detach().abs().max())
    assert float((bufs["probs"] - probs.detach()).abs().max()) <= 1e-13
    ties = {op.key: R.windows_with_ties(bufs[op.src], op) for op in R.pool_sites(case)}
    assert ties["MaxPool3d_2a_3x3"] == 0 and ties["MaxPool3d_3a_3x3"] == 0
    note(f"i3d host {cid}: windows with two equal positive maxima (structural) {sum(ties.values())} of the pools "
         f"{[k for k, v in ties.items() if v]}")
    target = probs.detach().argmax(1)
    for variant, kw, loss in (("dout", dict(dout=R.dout(case).double()), (probs * R.dout(case).double()).sum()),
                              ("target", dict(target=target.to(torch.int32)), probs[torch.arange(3), target].sum())):
        dx, = torch.autograd.grad(loss, xin, retain_graph=True)
        bres, grads = R.backward(case, "exact", bufs, bufs["probs"], **kw)
        got = grads["input"][:, :case.clip[0]]
        assert bool((grads["input"][:, case.clip[0]:] == 0).all())
        err = float((got - dx).abs().max()) / float(dx.abs().max())
        note(f"i3d host {cid} {variant}: chained restatement vs fp64 autograd dx {err:.2e}, |dx| {float(dx.norm()):.3e}")
        assert err <= 1e-10, (variant, err)
        # a healthy gradient: per clip, not a vanishing one behind a negligible probability
        per_clip = dx.reshape(3, -1).norm(dim=1)
        assert float(per_clip.min()) > 1e-6, per_clip


@pytest.mark.parametrize("cid", CASE_IDS)
def test_geometry_is_what_the_table_claims(cid):
    import ivf_arch as arch
    case = R.CASES[cid]
    bufs, ops = R.plan(case)
    names = ("Conv3d_1a_7x7", "MaxPool3d_2a_3x3", "MaxPool3d_3a_3x3", "MaxPool3d_4a_3x3", "MaxPool3d_5a_2x2")
    assert [bufs[n][1:4] for n in names] == R.MAPS[cid]
    assert bufs["Mixed_5c"][1:4] == R.head_window(case)
    for op in ops:
        dims = bufs[op.src][1:4]
        assert op.pads == tuple(arch.same_pad(n, k, s)[0] for n, k, s in zip(dims, op.k, op.s)), op.key
        assert bufs[op.dst][1:4] == tuple(arch.out_size(n, k, s) for n, k, s in zip(dims, op.k, op.s)), op.key
    k3 = [op for op in ops if op.k == (3, 3, 3)]
    pad_dims = [p for op in ops if max(op.k) > 1 for p, k in zip(op.pads, op.k) if k > 1 and op.s != (1, 1, 1)]
    if cid == "odd":
        assert 0 in pad_dims and 1 in pad_dims                     # a front pad cell at some strided site, none at another
        assert any(n % 2 for n in bufs["Mixed_3b"][1:4]) and case.clip[1] % 2 == 1
        assert any(max(bufs[op.src][1:4]) < 4 for op in k3 if op.kind == "conv")       # a map below 4x4x4 under a 3x3x3 conv
    if cid == "smod":
        sites = {op.key: op for op in ops}
        assert sites["Conv3d_1a_7x7"].s == (1, 2, 2)
        assert sites["MaxPool3d_4a_3x3"].s == (1, 2, 2) and sites["MaxPool3d_4a_3x3"].k == (3, 3, 3)   # a (1,2,2) 3-tap pool
        assert sites["MaxPool3d_5a_2x2"].s == (1, 2, 2)
        assert all(bufs[n][1] == 8 for n in bufs)
    if cid == "gray":
        assert case.clip[0] == 1
        single = [op for op in k3 if bufs[op.src][1:4] == (1, 1, 1)]
        assert {op.kind for op in single} == {"conv", "pool"}       # 3x3x3 convs and the stride-1 pool on one position
    assert all(0 <= p <= 3 for op in ops for p in op.pads)


@pytest.mark.parametrize("cid,mode", R.CASE_MODES)
def test_floors_are_finite_and_bounded(cid, mode):
    """Every op's floor (float32 evaluation against the fp64 ideal, on the chain's buffers) is finite and below the
    any-order fp32 sum bound of its term count; the arg-max targets carry a healthy probability."""
    case = R.CASES[cid]
    ref = R.reference(case, mode)
    assert len(ref["floor"]) == 87          # 3 trunk units + 9 x 5 forward, 9 x 4 + 3 backward: every conv site both ways
    for key, fl in ref["floor"].items():
        assert math.isfinite(fl) and fl >= R.U, key
        assert fl <= R.sum_bound(1.0, R.n_terms(case, key, mode)), (key, fl)
    worst = max(ref["floor"], key=ref["floor"].get)
    note(f"i3d host {cid} {mode}: {len(ref['floor'])} floors, largest {ref['floor'][worst]:.2e} at {worst}")
    assert float(ref["probs"][torch.arange(3), ref["target"].long()].min()) > 1.0 / R.NUM_CLASSES
    for variant, (bres, grads) in ref["back"].items():
        assert float(grads["input"].reshape(3, -1).norm(dim=1).min()) > 1e-6, variant


@pytest.mark.parametrize("name", list(R.MUTANTS))
def test_every_wiring_mutant_leaves_the_gate(name):
    d = R.mutant_distance(name)
    note(f"i3d host mutant {name} on {R.MUTANTS[name][0]} at {R.MUTANTS[name][1]}: {d:.3g} gates")
    assert d >= R.MUTANT_DISTANCE, (name, d)


def test_fold_is_the_unfused_fp32_fold():
    """scale = gamma / sqrtf(var + eps), shift = beta - mean * scale and wb = scale * w are fp32 numbers, each one
    rounding away from the fp64 fold."""
    case = R.CASES["gray"]
    w32, w64 = R.weights(case), R.weights(case, exact=True)
    for name in ("Conv3d_1a_7x7", "Mixed_4c.b1a"):
        for q in ("scale", "shift", "wb"):
            a, b = w32[name][q], w64[name][q]
            assert bool((a.float().double() == a).all())
            assert float(((a - b).abs() / (b.abs() + 0.2)).max()) < 4 * R.U, (name, q)
