"""CPU: which kernel variant serves a convolution descriptor.  ivf_conv3d_variants (the candidates the tuner times)
and ivf_conv3d_default_variant (what IVF_CONV_AUTO launches) are host-only calls; over a grid of descriptors both
must equal what the selection code of the commit before the variant table returned, recorded in
tests/golden/conv_dispatch.json (its "about" key says how), and every built-in choice must be one of the candidates."""
import ctypes
import hashlib
import itertools
import json
import os

import pytest

from conftest import GOLDEN

KS = (1, 2, 3, 4, 7)
STRIDES = (1, 2)
CINS = (4, 8, 16, 20)
COUTS = (32, 40, 64, 96, 128, 192, 200)
TOS = (2, 4)
MATHS = ("fp32", "bf16x3", "bf16x6", "bf16act")
FLAGS = ("plain", "d2s", "out2", "gate_out", "gate_in", "in2", "out2+gate_out")
PTR = 64      # stands for a device address: the host calls never follow it


def descriptor(k, s, cin, cout, to, math, flag):
    """One legal descriptor of the grid (an 8 x 8 output map, SAME-style front pads), or None where the flag is not
    defined for the shape (ivf_conv3d's own argument rules)."""
    import ivf_lib as L
    d = L.ConvDesc()
    d.B, d.To, d.Ho, d.Wo = 1, to, 8, 8
    d.Ti, d.Hi, d.Wi = to * s, 8 * s, 8 * s
    d.Cin, d.in_ld, d.Cout, d.out_ld = cin, cin, cout, cout
    d.kT = d.kH = d.kW = k
    d.sT = d.sH = d.sW = s
    d.pT = d.pH = d.pW = (k - 1) // 2
    d.relu, d.math = 1, L.MATH_MODES[math]
    n0 = cout // 2 // 8 * 8
    if flag == "d2s":                       # Cout = 8 parities x 4 channels
        if cout != 32:
            return None
        d.d2s, d.relu = 1, 0
        d.bsT = d.bsH = d.bsW = 2
        d.dT, d.dH, d.dW, d.dC, d.out_ld = 2 * to, 16, 16, 4, 4
    if flag in ("out2", "out2+gate_out"):
        d.out2, d.N0, d.out2_ld = PTR, n0, cout - n0
    if flag in ("gate_out", "out2+gate_out"):
        d.gate_out, d.gate_out_ld = PTR, cout // 8
    if flag == "out2+gate_out":
        d.gate_out2, d.gate_out2_ld = PTR, (cout - n0) // 8
    if flag == "gate_in":
        d.gate_in, d.gate_in_ld = PTR, cout // 8
    if flag == "in2":                       # 1x1x1 only, channels [K0, Cin) from the second buffer
        if k != 1 or cin < 8:
            return None
        d.K0 = 4 if cin == 8 else 8
        d.in2, d.in2_ld = PTR, cin - d.K0
    return d


def grid():
    for k, s, cin, cout, to, math, flag in itertools.product(KS, STRIDES, CINS, COUTS, TOS, MATHS, FLAGS):
        d = descriptor(k, s, cin, cout, to, math, flag)
        if d is not None:
            yield f"k{k} s{s} cin{cin} cout{cout} to{to} {math} {flag}", d


def selection(lib):
    """[(key, candidate ids, built-in id or negative error)] over the grid, from `lib`."""
    out = []
    ids = (ctypes.c_int * 96)()
    for key, d in grid():
        n = lib.ivf_conv3d_variants(ctypes.byref(d), ids, 96)
        out.append((key, list(ids)[:n], lib.ivf_conv3d_default_variant(ctypes.byref(d))))
    return out


def grid_digest(keys):
    return hashlib.sha1("\n".join(keys).encode()).hexdigest()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "conv_dispatch.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def selected():
    import ivf_lib as L
    return selection(L.lib())


def test_grid_is_the_recorded_one(recorded, selected):
    assert len(selected) == len(recorded["list"]) == len(recorded["default"]) > 10000
    assert grid_digest([k for k, _, _ in selected]) == recorded["grid_sha1"]


def test_variant_lists_equal_the_recorded_ones(recorded, selected):
    lists = recorded["lists"]
    bad = [(k, ids, lists[i]) for (k, ids, _), i in zip(selected, recorded["list"]) if ids != lists[i]]
    assert not bad, f"{len(bad)} descriptors list other candidates, e.g. {bad[:3]}"


def test_default_variants_equal_the_recorded_ones(recorded, selected):
    bad = [(k, got, want) for (k, _, got), want in zip(selected, recorded["default"]) if got != want]
    assert not bad, f"{len(bad)} descriptors resolve IVF_CONV_AUTO differently (got, recorded), e.g. {bad[:3]}"
    assert any(v > 0 for _, _, v in selected) and any(v < 0 for _, _, v in selected)


def test_every_default_is_a_listed_candidate(selected):
    bad = [(k, v, ids) for k, ids, v in selected if v > 0 and v not in ids]
    assert not bad, f"{len(bad)} built-in choices are not among the candidates, e.g. {bad[:3]}"
