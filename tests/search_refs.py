"""Cases, start masks and the float64 chain reference of the temporal mask search driver (csrc/search_driver.h,
run_search): test_gpu_search_driver.py on the GPU, test_search_refs_host.py on the CPU.  Both iterate the tables below, so
the host test proves the reference, the mutant distances, the ambiguity cap and the threshold margin on exactly the
inputs the driver is later compared on.  Nothing here needs a GPU or the HIP library.

One iteration's differentiable chain (`chain`): sigmoid(raw) -> oracle.mask_ref.freeze / reverse (per-clip masks) -> the
functional model of clstm_refs or tfclstm_refs -> probs[clip, target[clip]].  It returns sig, probs, score and
d score / d sig in the dtype asked for, as float64 numpy.  As stmask_refs._chain_run, the model's own dx is pushed
back through the perturbation by autograd.

Gate (DESIGN.md "Temporal search driver gate"): per tensor, floor = clstm_refs.elem_err(float32 chain, float64 chain)
on the SAME raw, the largest over the clips and never below U; for the persistent ConvLSTM case the larger of the libm
and the fast-gate float32 runs, as clstm_refs.floors.  gate = clstm_refs.GATE_MARGIN * floor.  A clip whose float64 run
has an ambiguous pool window (clstm_refs.ambiguous_windows; for the TF plan also a recurrent gate at the hard-sigmoid
kink, tfclstm_refs.kink_ambiguous) is left out of the d score / d sig comparison only.

Reverse-mode start masks (`rev_rows`).  A row is built from an on/off pattern: on frames start at raw in [-0.8, 2]
(sigmoid >= 0.31; the first on frame of a row in [-0.8, -0.2], sigmoid <= 0.45, so that mutant (d) pairs other
frames), off frames at raw in [-4.5, -3.4] (sigmoid <= 0.033).  Adam moves a raw value by at most lr = 0.2 an
iteration (|m_hat| / sqrt(v_hat) <= 1 over the first steps from zero moments), so over N_ITERS = 3 iterations an on
frame stays above sigmoid(-1.4) = 0.198 and an off frame below sigmoid(-2.8) = 0.057: every sigmoid(raw) keeps
THRESH_MARGIN from the pairing threshold 0.1f, in float32 and float64 alike, and both pair the same frames.  The
host test asserts the margin along the float64 run.  Rows cycle through REV_KINDS; the first three together hold
every named property (REV_PROPERTIES), so every batch of b >= 3 rows has them all.  A plan batch of 1 or 2 rows
cannot hold an all-on and an all-off row beside the mixed row; it has the leading rows of the same table.  T >= 4
everywhere (with T < 3 the TV term is the reference's 0/0).
"""
import ctypes
import ctypes.util
import functools
import zlib
from collections import OrderedDict, namedtuple

import numpy as np
import torch

import clstm_refs as CR
import tfclstm_refs as TR
from leaf_refs import THRESH
from oracle import mask_ref
from stmask_refs import tv_pairs

N_ITERS = 3
LAM1, LAM2 = 0.01, 0.02
ADAM = dict(lr=0.2, b1=0.9, b2=0.999, eps=1e-8)
MODES = ("freeze", "reverse")
THRESH_MARGIN = 1e-3
TENSORS = ("sig", "probs", "score", "dsig")

Plan = namedtuple("Plan", "id kind case b sizes modes")
# seed of the TF plan's clips: the first from tfclstm_refs' 11 on for which no clip of the float64 loop has an ambiguous
# element at any iteration (pick_clip_ids below)
TF_XSEED = 15

# kind 'clstm' (clstm_refs) or 'tf' (tfclstm_refs); b: the batch of the fp64 comparison; sizes: the batches the driver
# is replayed at (b = 1, 1 < b < B, b = B where the plan has them).  S2 keeps its geometry and weights with a third
# clip, so that a batch holds the three leading start-mask rows; P3 runs the persistent recurrence, which needs
# b >= 64; TF is the plan of test_gpu_tfclstm._setup (tfclstm_refs' case X) with a third clip.
PLANS = OrderedDict((p.id, p) for p in [
    Plan("S1", "clstm", CR.CASES["S1"], 3, (1, 3, 4), MODES),
    Plan("S2", "clstm", CR.CASES["S2"]._replace(b=3, B=3), 3, (1, 2, 3), MODES),
    Plan("P3", "clstm", CR.CASES["P3"], 64, (64,), MODES),
    Plan("TF", "tf", TR.CASES["X"]._replace(b=3, B=3, xseed=TF_XSEED), 3, (1, 2, 3), ("freeze",)),
])
RUNS = [(p.id, m) for p in PLANS.values() for m in p.modes]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7fffffff)


# Clip ids of P3.  clstm_refs' ids are chosen for the unperturbed clips; here a clip runs frozen or reversed by its row's
# masks for N_ITERS iterations in both modes, and with 64 clips a few of those runs have a pool window near a tie.
# pick_clip_ids below chose, row by row, the first id from the case's id0 on whose float64 loop has no ambiguous window
# in either mode (`python tests/search_refs.py P3`); the cap of 1/16 then remains for what float32 moves.
CLIP_IDS = {
    "P3": (1300, 1364, 1302, 1303, 1304, 1305, 1378, 1379, 1367, 1309, 1310, 1368, 1312, 1313, 1314, 1315,
           1316, 1317, 1369, 1319, 1320, 1370, 1322, 1323, 1324, 1325, 1326, 1327, 1328, 1329, 1330, 1331,
           1371, 1372, 1334, 1373, 1336, 1337, 1338, 1374, 1340, 1341, 1342, 1343, 1375, 1345, 1346, 1347,
           1348, 1349, 1350, 1351, 1352, 1353, 1354, 1355, 1356, 1357, 1376, 1380, 1360, 1361, 1362, 1363),
}


@functools.lru_cache(maxsize=None)
def _inputs(pid, ids):
    plan = PLANS[pid]
    if plan.kind == "tf":
        return TR.case_inputs(plan.case, plan.case.B)
    x, sd, targets, _ = CR.case_inputs(plan.case, plan.case.B)
    if ids is not None:
        assert len(set(ids)) == plan.case.B
        x = torch.from_numpy(CR.clips(plan.case, ids))
    return x, sd, targets


def inputs(pid, ids=None):
    """(x [B,C,T,H,W] float32, weights, targets [B]) of all B clips of a plan: distinct clips, targets that differ from
    one clip to the next.  ids: other clips than the table's (pick_clip_ids)."""
    return _inputs(pid, tuple(ids) if ids is not None else CLIP_IDS.get(pid))


# ------------------------------------------------------------------------------------------------ start masks
REV_KINDS = ("mixed", "all_off", "all_on", "even_mid", "odd_mid", "random")
REV_PROPERTIES = ("even", "odd", "first", "last", "all_on", "all_off")


def rev_pattern(kind, T, g):
    """on/off pattern [T] (bool) of a named row.  mixed: an even run touching frame 0 and an odd run touching frame
    T - 1 (three frames from T = 6 on, below that a single frame: an odd run whose middle frame is all of it)."""
    assert T >= 4
    on = torch.zeros(T, dtype=torch.bool)
    if kind == "mixed":
        on[:2] = True
        on[T - 3 if T >= 6 else T - 1:] = True
    elif kind == "all_on":
        on[:] = True
    elif kind == "even_mid":
        on[1:3] = True
    elif kind == "odd_mid":
        on[1:4] = True
    elif kind == "random":
        on = torch.rand(T, generator=g) < 0.5
    else:
        assert kind == "all_off"
    return on


def rev_properties(on):
    """which of REV_PROPERTIES an on/off pattern has (runs as oracle.mask_ref.find_submasks_from_mask finds them)"""
    T = len(on)
    runs = mask_ref.find_submasks_from_mask(on.float(), 0.5)
    props = set()
    for r in runs:
        props.add("even" if len(r) % 2 == 0 else "odd")
        if r[0] == 0:
            props.add("first")
        if r[-1] == T - 1:
            props.add("last")
    if bool(on.all()):
        props.add("all_on")
    if not bool(on.any()):
        props.add("all_off")
    return props


def rev_rows(pid, B, T):
    """(raw [B,T] float32, on [B,T] bool): row r is of kind REV_KINDS[r % 6] (module docstring)"""
    g = _gen("revraw", pid)
    raws, ons = [], []
    for r in range(B):
        on = rev_pattern(REV_KINDS[r % len(REV_KINDS)], T, g)
        hi = torch.rand(T, generator=g) * 2.8 - 0.8
        lo = torch.rand(T, generator=g) * 1.1 - 4.5
        if bool(on.any()):                      # the first on frame below 0.5: a threshold of 0.5 pairs other frames
            hi[int(on.int().argmax())] = -0.8 + 0.6 * float(torch.rand(1, generator=g))
        raws.append(torch.where(on, hi, lo))
        ons.append(on)
    return torch.stack(raws).float().contiguous(), torch.stack(ons)


@functools.lru_cache(maxsize=None)
def start_raw(pid, mode, B, T):
    """raw [B,T] float32 of a plan's B clips; a batch of b clips starts from its leading b rows.  freeze: seeded values
    in +-2, distinct per clip."""
    if mode == "reverse":
        return rev_rows(pid, B, T)[0]
    return (torch.rand(B, T, generator=_gen("raw", pid)) * 4 - 2).float().contiguous()


# ------------------------------------------------------------------------------------------------ the chain
MUTANTS = OrderedDict([
    ("partner_weight", "(a) reverse blends the partner with m[b] instead of m[a]"),
    ("target0", "(b) every clip scored with target[0]"),
    ("freeze_prev", "(c) the freeze recurrence reads m[u-1]"),
    ("thresh", "(d) pairing threshold 0.5 instead of 0.1"),
    ("logits", "(e) the score taken from the logits instead of the probabilities"),
])


def mutant_applies(mutant, mode):
    return {"partner_weight": mode == "reverse", "thresh": mode == "reverse", "freeze_prev": mode == "freeze"}.get(mutant, True)


def perturb(x, sig, mode, mutant=None):
    """the perturbed clips [b,C,T,H,W], differentiable in sig [b,T]: oracle.mask_ref.freeze, or .reverse clip by clip"""
    b, T = sig.shape
    if mode == "freeze":
        if mutant != "freeze_prev":
            return mask_ref.freeze(x, sig)
        frames = [x[:, :, 0]]
        for u in range(1, T):
            mu = sig[:, u - 1].view(-1, 1, 1, 1)
            frames.append((1 - mu) * x[:, :, u] + mu * frames[-1])
        return torch.stack(frames, dim=2)
    thresh = 0.5 if mutant == "thresh" else THRESH
    if mutant != "partner_weight":
        return torch.cat([mask_ref.reverse(x[r:r + 1], sig[r], thresh) for r in range(b)])
    out = x.clone()
    for r in range(b):
        for run in mask_ref.find_submasks_from_mask(sig[r].detach(), thresh):
            for u in range(len(run) // 2):
                a, p = run[u], run[-(u + 1)]
                out[r, :, a] = (1 - sig[r, a]) * x[r, :, a] + sig[r, a] * x[r, :, p]
                out[r, :, p] = (1 - sig[r, p]) * x[r, :, p] + sig[r, p] * x[r, :, a]
    return out


def chain(pid, x, net, targets, raw, mode, dtype=torch.float64, mutant=None, fast_gates=False):
    """One iteration's chain on the clips x [b,...] with masks raw [b,T], in `dtype`.  Returns float64 numpy arrays sig
    [b,T], probs [b,K], score [b,1], dsig [b,T] = d score[clip] / d sig, and `run`, the model's result dict on the
    perturbed clips (for the ConvLSTM it holds `pre`, the pool pre-activations clstm_refs.ambiguous_windows needs)."""
    plan = PLANS[pid]
    b = raw.shape[0]
    sig = torch.sigmoid(raw.to(dtype)).requires_grad_()
    P = perturb(x.to(dtype), sig, mode, mutant)
    tg = [targets[0]] * b if mutant == "target0" else [int(t) for t in targets]
    if plan.kind == "clstm":
        case = plan.case._replace(softmax=False) if mutant == "logits" else plan.case
        res = CR.run(case, P.detach(), net, dtype, fast_gates=fast_gates, targets=tg)
    else:
        res = TR.run(plan.case, P.detach(), net, dtype, targets=tg)
        if mutant == "logits":
            res["score"] = res["logits"][np.arange(b), tg]
    if P.requires_grad:                       # (reverse with every row off: the clips do not depend on the masks)
        P.backward(torch.from_numpy(res["dx"]).to(dtype))
    dsig = sig.grad if sig.grad is not None else torch.zeros_like(sig)
    return {"sig": sig.detach().double().numpy(), "probs": res["probs"], "score": np.asarray(res["score"]).reshape(b, 1),
            "dsig": dsig.detach().double().numpy(), "run": res}


def errors(res, ref):
    """tensor name -> per-clip clstm_refs.elem_err against the float64 chain"""
    return OrderedDict((n, CR.elem_err(res[n], ref[n])) for n in TENSORS)


def measure(pid, x, net, targets, raw, mode):
    """Everything a comparison on `raw` needs, all from the CPU: the float64 chain, the float32 floor and gate of every
    tensor, and per clip the number of ambiguous elements of the float64 run (module docstring)."""
    plan = PLANS[pid]
    ref = chain(pid, x, net, targets, raw, mode, torch.float64)
    variants = [chain(pid, x, net, targets, raw, mode, torch.float32)]
    if plan.kind == "clstm" and plan.case.path == "P":
        variants.append(chain(pid, x, net, targets, raw, mode, torch.float32, fast_gates=True))
    floor = OrderedDict((n, max(CR.U, max(float(np.max(errors(v, ref)[n])) for v in variants))) for n in TENSORS)
    mod = CR if plan.kind == "clstm" else TR
    fwd = [mod.errors(v["run"], ref["run"], True) for v in variants]
    fwd_floor = {n: max(CR.U, max(float(np.max(f[n])) for f in fwd)) for n in fwd[0]}
    if plan.kind == "clstm":
        amb = CR.ambiguous_windows(ref["run"]["pre"], fwd_floor)[0]
    else:
        amb = (TR.ambiguous_windows(ref["run"]["H"], fwd_floor)[0]
               + TR.kink_ambiguous(plan.case, ref["run"]["z"], fwd_floor)[0])
    return {"ref": ref, "f32": variants[0], "floor": floor, "ambiguous": amb,
            "gate": OrderedDict((n, CR.GATE_MARGIN * v) for n, v in floor.items())}


def ambiguous_cap(pid, b):
    """how many clips of a batch may be left out of the d score / d sig comparison: none, but for the persistent case"""
    plan = PLANS[pid]
    return int(CR.AMBIGUOUS_CAP * b) if plan.kind == "clstm" and plan.case.path == "P" else 0


# ------------------------------------------------------------------------------------------------ the loop on the CPU
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = _libm.sqrtf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.sqrtf.argtypes = [ctypes.c_float]


def eps_hat32(eps, beta2, step):
    """tf.train.Adam's epsilon in torch's form, eps / sqrtf(1 - powf(beta2, step)), every operation in float32 with the
    C library's powf and sqrtf, as the host code of ivf_tfclstm_search forms it"""
    p = np.float32(_libm.powf(beta2, float(step)))
    return float(np.float32(eps) / np.float32(_libm.sqrtf(float(np.float32(1.0) - p))))


def eps_at(pid, step, plain=False):
    """the epsilon handed to ivf_search_step at `step`: the TF plan's eps_hat(step), else eps itself"""
    eps = ADAM["eps"]
    return eps_hat32(eps, ADAM["b2"], step) if pid in PLANS and PLANS[pid].kind == "tf" and not plain else eps


def reg_grad(sig):
    """d (lam1 sum |s| + lam2 TV33(s)) / d s per row, float64; TV33 as the sum over frame pairs of w |s[k+1] - s[k]|^3
    (stmask_refs.tv_pairs: interior pairs twice), which is calc_tv_norm(s, 3, 3) without its 0/0 at a constant row"""
    s = sig.clone().requires_grad_()
    w = tv_pairs(s.shape[1]).view(1, -1)
    (LAM1 * s.abs().sum() + LAM2 * (w * (s[:, 1:] - s[:, :-1]).abs() ** 3).sum()).backward()
    return s.grad


def free_run(pid, mode, b=None, n=N_ITERS, ids=None):
    """The loop in float64 from the plan's start masks: yields (raw float32 [b,T] of the iteration, measure(...) on it),
    then steps raw with Adam (torch's form with eps_at(step)) on the float64 gradient."""
    plan = PLANS[pid]
    b = plan.b if b is None else b
    x, net, targets = inputs(pid, ids)
    x, targets = x[:b], targets[:b]
    raw = start_raw(pid, mode, plan.case.B, plan.case.T)[:b].double()
    m, v = torch.zeros_like(raw), torch.zeros_like(raw)
    lr, b1, b2 = ADAM["lr"], ADAM["b1"], ADAM["b2"]
    for step in range(1, n + 1):
        ms = measure(pid, x, net, targets, raw.float(), mode)
        yield raw.float(), ms
        s = torch.sigmoid(raw)
        g = (reg_grad(s) + torch.from_numpy(ms["ref"]["dsig"])) * s * (1 - s)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        raw = raw - lr / (1 - b1 ** step) * m / (v.sqrt() / (1 - b2 ** step) ** 0.5 + eps_at(pid, step))


def pick_clip_ids(pid, tries=8):
    """Row by row, the first clip id from the case's id0 on whose float64 loop has no ambiguous element at any of the
    N_ITERS iterations in any mode of the plan.  A clip's run depends on its own row alone, so the rows that fail are
    replaced together and the loop is run again."""
    plan = PLANS[pid]
    if plan.kind == "tf":
        for seed in range(plan.case.xseed, plan.case.xseed + 8 * tries):
            PLANS[pid] = plan._replace(case=plan.case._replace(xseed=seed))
            _inputs.cache_clear()
            if not any((ms["ambiguous"] > 0).any() for _, ms in free_run(pid, "freeze", b=plan.case.B)):
                return seed
        raise RuntimeError(f"plan {pid}: no seed")
    ids = list(range(plan.case.id0, plan.case.id0 + plan.case.B))
    nxt = ids[-1] + 1
    for _ in range(tries):
        bad = np.zeros(plan.case.B, bool)
        for mode in plan.modes:
            for _, ms in free_run(pid, mode, b=plan.case.B, ids=ids):
                bad |= ms["ambiguous"] > 0
        if not bad.any():
            return tuple(ids)
        for r in np.nonzero(bad)[0]:
            ids[r], nxt = nxt, nxt + 1
    raise RuntimeError(f"plan {pid}: no clip ids in {tries} rounds")


if __name__ == "__main__":
    import sys
    for pid in sys.argv[1:]:
        print(f'    "{pid}": {pick_clip_ids(pid)},')
