"""Arena contents as a test variable (not a conftest: import it).

Every plan works inside caller-owned arenas that ivf_engine._arena allocates with torch.empty, and the engine's entry
points allocate their outputs the same way.  `filled(pattern)` makes both start from a byte pattern instead of from
whatever the allocator hands out; `refill(eng, pattern)` puts the pattern back before an entry.  A result that depends
on a cell its own entry never wrote then differs between the patterns:

  0x00  the de-facto state of a fresh process (the baseline the others are compared with)
  0xFF  fp32 NaN, bf16 NaN, int32 -1, uint8 255 (the pools' "no route" code): any float read of an unwritten cell that
        reaches a result shows
  0x42  fp32 48.56..., bf16 48.5, uint8 66: finite and positive, so a ReLU, an fmaxf(., 0) or a gate epilogue cannot
        swallow it the way it swallows a NaN or a negative

The numpy part at the bottom (stage_cl4, relu_accumulate and their mutants) is the proof, on the host, that a test built
on these patterns can fail, and that it needs both of them (test_arena_fill_host.py)."""
import contextlib
from collections import OrderedDict

import numpy as np

PATTERNS = (0x00, 0xFF, 0x42)
BASELINE = 0x00
# scratch an engine keeps between calls of st_search, ig and smoothgrad (lin_solve takes a fresh arena per call)
CACHED_SCRATCH = ("_st_ws", "_ig_ws", "_sg_ws")


def fill_bytes(t, pattern):
    """every byte of a contiguous torch tensor := pattern, on the current stream"""
    import torch
    if t.numel():
        assert t.is_contiguous()
        t.view(torch.uint8).fill_(int(pattern))
    return t


class _FillingTorch:
    """`torch` as ivf_engine sees it inside `filled`: empty / empty_like return tensors holding the pattern."""

    def __init__(self, torch, pattern):
        self._torch, self._pattern = torch, pattern

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def empty(self, *a, **kw):
        return fill_bytes(self._torch.empty(*a, **kw), self._pattern)

    def empty_like(self, *a, **kw):
        return fill_bytes(self._torch.empty_like(*a, **kw).contiguous(), self._pattern)


@contextlib.contextmanager
def filled(pattern, outputs=True):
    """Inside: ivf_engine._arena returns arenas filled with `pattern` (an engine built here has a filled weights arena
    and workspace; st_search, ig, smoothgrad and lin_solve called here get filled scratch), and with outputs=True every
    output tensor the engine allocates starts from the pattern as well."""
    import ivf_engine
    arena, torch = ivf_engine._arena, ivf_engine.torch

    def filled_arena(nbytes, device):
        return fill_bytes(arena(nbytes, device), pattern)
    ivf_engine._arena = filled_arena
    if outputs:
        ivf_engine.torch = _FillingTorch(torch, pattern)
    try:
        yield
    finally:
        ivf_engine._arena, ivf_engine.torch = arena, torch


def refill(eng, pattern):
    """eng's workspace := pattern on the current stream (and the scratch it keeps between calls, where it has any).
    The weights arena is left alone: it holds the loaded weights."""
    fill_bytes(eng._ws, pattern)
    for name in CACHED_SCRATCH:
        ws = eng.__dict__.get(name)
        if ws is not None:
            fill_bytes(ws, pattern)


def as_bytes(t):
    """a uint8 copy of a tensor's bytes: NaNs compare by their bits"""
    import torch
    return t.detach().contiguous().view(-1).view(torch.uint8).clone()


class Record:
    """What a call sequence returned, buffer by buffer: name -> bytes, in call order; `entries` counts the calls."""

    def __init__(self):
        self.bufs, self.entries = OrderedDict(), 0

    def add(self, label, value, entry=True):
        """value: a tensor, None, or a tuple / list / dict of such (nested); entry: a call of its own (not a read of
        what the previous one left)"""
        import torch
        self.entries += int(entry)
        if value is None or isinstance(value, (int, float)):
            return
        if torch.is_tensor(value):
            assert label not in self.bufs, label
            self.bufs[label] = as_bytes(value)
        elif isinstance(value, dict):
            for k, v in value.items():
                self.add(f"{label}.{k}", v, entry=False)
        else:
            for i, v in enumerate(value):
                self.add(f"{label}[{i}]", v, entry=False)


def first_difference(base, other):
    """None, or the name of the first buffer of `other` that is not byte-equal to `base`'s (with how many bytes differ)"""
    import torch
    assert list(base.bufs) == list(other.bufs)
    for name, want in base.bufs.items():
        got = other.bufs[name]
        if got.shape != want.shape or not torch.equal(got, want):
            n = int((got != want).sum()) if got.shape == want.shape else -1
            return f"{name} ({n} of {want.numel()} bytes)"
    return None


def verdict(records):
    """(line, ok) for note(): records = {pattern: Record}; every pattern against BASELINE"""
    base = records[BASELINE]
    for p, rec in records.items():
        if p == BASELINE:
            continue
        d = first_difference(base, rec)
        if d is not None:
            return f"{base.entries} entries, {len(base.bufs)} buffers: under 0x{p:02X} first differing buffer {d}", False
    names = " / ".join(f"0x{p:02X}" for p in records)
    return f"{base.entries} entries, {len(base.bufs)} buffers: byte-equal across {names}", True


# ---------------------------------------------------------------------------------------------------- host models
def arena(nbytes, pattern):
    return np.full(nbytes, pattern, np.uint8)


def stage_cl4(x, dst, skip_pad=False):
    """The staging rule of the 16-byte input pixels (ncthw_to_cl4_kernel and every *_stage kernel at out_cpad = 4):
    x [b,C,T,HW] fp32 -> dst viewed as [b,T,HW,4], channels C .. 3 := 0.  skip_pad: the mutant that stores the C real
    channels only."""
    b, C, T, HW = x.shape
    px = dst[:b * T * HW * 16].view(np.float32).reshape(b, T, HW, 4)
    px[..., :C] = np.transpose(x, (0, 2, 3, 1))
    if not skip_pad:
        px[..., C:] = 0.0
    return px


def stem_tap(px, w4):
    """what a consumer of the pixels computes: all four lanes times a weight whose pad lanes are zero"""
    with np.errstate(invalid="ignore"):
        return (px * w4).sum(-1)


def relu_accumulate(v, dst, first_writer=True):
    """The epilogue of a gradient buffer's writers: the first stores max(v, 0), later ones max(old + v, 0).
    first_writer=False on a buffer nobody wrote is the mutant."""
    old = dst[:v.size * 4].view(np.float32).reshape(v.shape)
    with np.errstate(invalid="ignore"):
        old[...] = np.maximum(v, 0.0) if first_writer else np.fmax(old + v, 0.0)   # fmaxf(NaN, 0) = 0, as on the device
    return old
