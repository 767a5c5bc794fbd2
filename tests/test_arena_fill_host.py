"""The arena-contents tests can fail, and need both non-zero patterns: numpy mutants of two rules of the plans, fed
the three fills of tests/arena_fill.py (test_gpu_arena_contents.py runs the real kernels the same way)."""
import numpy as np

import arena_fill as AF


def _pixels(C=3, b=2, T=2, HW=5):
    rng = np.random.default_rng(3)
    return rng.standard_normal((b, C, T, HW)).astype(np.float32)


def test_patterns_are_what_the_kernels_would_read():
    a = {p: AF.arena(16, p) for p in AF.PATTERNS}
    assert np.isnan(a[0xFF].view(np.float32)).all() and (a[0xFF].view(np.int32) == -1).all()
    assert (a[0xFF].view(np.uint16).astype(np.uint32) << 16).view(np.float32).tolist() != [0.0] * 8    # bf16 NaN
    assert np.isnan((a[0xFF].view(np.uint16).astype(np.uint32) << 16).view(np.float32)).all()
    f = a[0x42].view(np.float32)
    assert np.all(f > 48.5) and np.all(f < 48.6)
    assert np.all((a[0x42].view(np.uint16).astype(np.uint32) << 16).view(np.float32) == 48.5)
    assert (a[0x00].view(np.float32) == 0).all()


def test_staging_rule_is_independent_of_the_arena():
    x = _pixels()
    staged = [AF.stage_cl4(x, AF.arena(x.size // 3 * 16 + 64, p)).tobytes() for p in AF.PATTERNS]
    assert staged[0] == staged[1] == staged[2]


def test_staging_mutant_without_the_pad_lane_store_differs_under_both_patterns():
    """The staged buffer (what endpoint('input') reads) differs under 0xFF and under 0x42.  Through a weight whose pad
    lanes are zero only the NaN reaches a result: 0 x 48.5 = 0, 0 x NaN = NaN."""
    x = _pixels()
    nbytes = x.size // 3 * 16
    px = {p: AF.stage_cl4(x, AF.arena(nbytes, p), skip_pad=True) for p in AF.PATTERNS}
    good = AF.stage_cl4(x, AF.arena(nbytes, 0xFF))
    assert px[0x00].tobytes() == good.tobytes()                 # on zero memory the mutant is invisible
    assert px[0xFF].tobytes() != good.tobytes() and px[0x42].tobytes() != good.tobytes()
    w4 = np.array([0.5, -1.0, 2.0, 0.0], np.float32)
    taps = {p: AF.stem_tap(px[p], w4) for p in AF.PATTERNS}
    assert np.array_equal(taps[0x42], taps[0x00]) and np.isnan(taps[0xFF]).all()


def test_relu_accumulate_mutant_shows_under_0x42_alone_where_the_true_value_is_zero():
    """max(old + v, 0) on an `old` nobody wrote, at cells whose value is not positive (a dead window, the row a pool
    dropped): fmaxf swallows the NaN of 0xFF, the answer is the right 0; under 0x42 it is 48.56 + v > 0."""
    v = -np.abs(_pixels(C=1)).reshape(-1)
    out = {p: AF.relu_accumulate(v, AF.arena(v.size * 4, p), first_writer=False).copy() for p in AF.PATTERNS}
    good = AF.relu_accumulate(v, AF.arena(v.size * 4, 0x42), first_writer=True)
    assert np.array_equal(out[0x00], good)
    assert np.array_equal(out[0xFF], good), "the NaN pattern alone would have missed this mutant"
    assert not np.array_equal(out[0x42], good) and np.all(out[0x42] > 0)
    # where the value is positive the NaN pattern shows it too (as 0), so 0xFF is not redundant either way round:
    # the staging mutant above is invisible in a product under 0x42
    vp = np.abs(v)
    outp = {p: AF.relu_accumulate(vp, AF.arena(v.size * 4, p), first_writer=False).copy() for p in AF.PATTERNS}
    assert np.array_equal(outp[0x00], vp) and not np.array_equal(outp[0xFF], vp) and not np.array_equal(outp[0x42], vp)


def test_correct_first_writer_is_independent_of_the_arena():
    v = _pixels(C=1).reshape(-1)
    outs = [AF.relu_accumulate(v, AF.arena(v.size * 4, p)).tobytes() for p in AF.PATTERNS]
    assert outs[0] == outs[1] == outs[2]


def test_record_and_verdict_name_the_first_differing_buffer():
    import torch
    recs = {}
    for p in AF.PATTERNS:
        r = AF.Record()
        r.add("forward", (torch.ones(3), None, {"a": torch.full((2,), float("nan"))}))
        r.add("forward.read", torch.full((4,), 1.0 if p != 0x42 else 2.0), entry=False)
        recs[p] = r
    line, ok = AF.verdict(recs)
    assert not ok and "0x42" in line and "forward.read" in line and line.startswith("1 entries, 3 buffers")
    line, ok = AF.verdict({p: recs[p] for p in (0x00, 0xFF)})           # NaNs compare by their bits
    assert ok and line.endswith("byte-equal across 0x00 / 0xFF")
