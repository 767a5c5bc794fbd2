"""LDS-halo convolutions on maps with short edge boxes (a narrow last box column, a last box row half live or less):
a launch whose planes (clips x t-boxes) divide by 8 runs the short-boxes-last kernel, which deals those boxes after
the full ones inside each eighth of the grid that one XCD runs; every other launch keeps the box order
(csrc/conv3d_halo_impl.h: the SL tile decode, halo_short_edges).  Every box must still compute its own outputs: every
map against torch fp64, and bit for bit against the same variant on the map zero-embedded in 32 x 32, where no
8-column box is narrow and no 8-row box is short -- the operands, the padding zeros and the order of every sum are the
same."""
import ctypes

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

EXT = 32          # H and W of the embedding map
B = 2
HALO_BASE = 16    # IVF_CONV_HALO_BASE; the tiles below are rows of kHaloTiles (TT, BN, WROWS, WCOLS, KS, BKH, TH, TW, TPS)
BOX8, BOX7, KS2 = HALO_BASE + 61, HALO_BASE + 50, HALO_BASE + 37   # (4,128,32,64,1,16,8,8,1) (4,96,32,96,1,16,7,8,1) (4,32,32,32,2,16,8,8,1)
WIDE = HALO_BASE + 60                                              # (4,192,32,96,1,16,8,8,1): the 16-wave tile of the headline
X3_BKH16, X3_BKH32 = HALO_BASE + 21, HALO_BASE + 0                 # (4,64,32,64,1,16,8,8,1) (4,192,32,96,1,32,8,8,1)
MAPS = [(28, 28),   # narrow last column, short last row, corner
        (20, 28),
        (28, 20),
        (12, 12),   # 2 x 2 boxes: one of each kind
        (12, 20),
        (24, 24)]   # no short edge: the box order


def to_cl(x):
    """NCTHW -> channels-last [B,T,H,W,C] on the GPU."""
    return x.permute(0, 2, 3, 4, 1).contiguous().cuda()


def extend(y, fill=0):
    """[B,T,H,W,C] -> [B,T,EXT,EXT,C], the original in the low corner."""
    e = torch.full(y.shape[:2] + (EXT, EXT) + y.shape[4:], fill, device=y.device, dtype=y.dtype)
    e[:, :, :y.shape[2], :y.shape[3]] = y
    return e


class Case:
    """Seeded operands of one conv (k = 3, stride 1, same padding), its fp64 results, and the launches."""

    def __init__(self, T, H, W, cin, cout, math, seed, B=B):
        import torch.nn.functional as F
        import ivf_lib as L
        self.L, self.lib = L, L.lib()
        gen = torch.Generator().manual_seed(seed)
        self.B, self.thw, self.cin, self.cout, self.mm = B, (T, H, W), cin, cout, L.MATH_MODES[math]
        x = torch.randn((B, cin, T, H, W), generator=gen)
        w = torch.randn(cout, cin, 3, 3, 3, generator=gen) * 0.1
        scale = torch.rand(cout, generator=gen) + 0.5
        shift = torch.randn(cout, generator=gen) * 0.1
        self.ref = F.conv3d(x.double(), w.double(), padding=1).permute(0, 2, 3, 4, 1)   # [B,T,H,W,cout]
        self.ref_relu = torch.relu(self.ref * scale.double() + shift.double()).numpy()
        self.wf = torch.empty(self.lib.ivf_conv3d_pack_fwd_elems(cout, cin, 3, 3, 3, self.mm), device='cuda')
        self.keep = (w.cuda(), scale.cuda(), shift.cuda())   # (kept alive: L.ptr only takes the address)
        L.check(self.lib.ivf_conv3d_pack_fwd(L.ptr(self.keep[0]), L.ptr(self.wf), cout, cin, cin, 3, 3, 3, self.mm, L.stream()))
        self.x = to_cl(x)
        self.x_e = extend(self.x)
        self.gen = gen

    def desc(self, h, w, variant):
        d = self.L.ConvDesc()
        d.B, d.Ti, d.Hi, d.Wi = self.B, self.thw[0], h, w
        d.Cin, d.in_ld, d.in_coff = self.cin, self.cin, 0
        d.To, d.Ho, d.Wo = self.thw[0], h, w
        d.Cout, d.out_ld, d.out_coff = self.cout, self.cout, 0
        d.kT = d.kH = d.kW = 3
        d.sT = d.sH = d.sW = 1
        d.pT = d.pH = d.pW = 1
        d.math, d.variant = self.mm, variant
        d.mask_ld, d.mask_coff = self.cout, 0
        return d

    def forward(self, variant, embedded):
        """relu(conv * scale + shift) into a NaN-filled output, on the map itself or on the embedding map."""
        L, (T, H, W) = self.L, self.thw
        h, w = (EXT, EXT) if embedded else (H, W)
        d = self.desc(h, w, variant)
        d.relu = 1
        y = torch.full((self.B, T, h, w, self.cout), float('nan'), device='cuda')
        L.check(self.lib.ivf_conv3d(ctypes.byref(d), L.ptr(self.x_e if embedded else self.x), L.ptr(self.wf),
                                    L.ptr(self.keep[1]), L.ptr(self.keep[2]), None, L.ptr(y), L.stream()))
        return y[:, :, :H, :W]

    def backward_form(self, variant, embedded, base, bits):
        """out = gate ? base + conv : 0 with the gate read from 1-bit records: a backward-data epilogue."""
        L, (T, H, W) = self.L, self.thw
        h, w = (EXT, EXT) if embedded else (H, W)
        d = self.desc(h, w, variant)
        d.accumulate = 1
        out = extend(base) if embedded else base.clone()
        gb = extend(bits, 0xFF) if embedded else bits
        d.gate_in, d.gate_in_ld, d.gate_in_coff = gb.data_ptr(), self.cout // 8, 0
        L.check(self.lib.ivf_conv3d(ctypes.byref(d), L.ptr(self.x_e if embedded else self.x), L.ptr(self.wf), None, None,
                                    None, L.ptr(out), L.stream()))
        return out[:, :, :H, :W]


@pytest.mark.parametrize("cin,cout", [(16, 32), (24, 96)])   # whole and partial 16-channel chunk; one and several column tiles
@pytest.mark.parametrize("T", [4, 6])                        # whole t-boxes; a t-edge box (2 and 4 planes: the box order)
@pytest.mark.parametrize("hw", MAPS)
def test_short_boxes_last_match_torch_and_the_box_order(hw, T, cin, cout):
    c = Case(T, hw[0], hw[1], cin, cout, "bf16x6", seed=31)
    for v in (BOX8, BOX7, KS2):
        y = c.forward(v, embedded=False)
        err = rel_err(y.cpu().numpy(), c.ref_relu)
        assert err < 1e-5, f"variant {v}: {err:.3g} from torch fp64"
        assert torch.equal(c.forward(v, embedded=True), y), f"variant {v}: differs from the embedded map"


@pytest.mark.parametrize("Bn,T", [(2, 16),    # 8 planes: one per range
                                  (4, 14),    # 16 planes, two per range, the last t-box of a clip with 2 live frames
                                  (2, 32)])   # 16 planes, two per range
@pytest.mark.parametrize("hw", MAPS)
def test_short_boxes_last_kernel(hw, Bn, T):
    """Planes in eighths: the grid is ordered inside each of the eight ranges that xcd_remap hands the XCDs."""
    c = Case(T, hw[0], hw[1], 16, 32, "bf16x6", seed=43, B=Bn)
    for v in (BOX8, BOX7, KS2, WIDE):
        y = c.forward(v, embedded=False)
        err = rel_err(y.cpu().numpy(), c.ref_relu)
        assert err < 1e-5, f"variant {v}: {err:.3g} from torch fp64"
        assert torch.equal(c.forward(v, embedded=True), y), f"variant {v}: differs from the embedded map"


@pytest.mark.parametrize("Bn,T", [(2, 6), (4, 14)])   # the box order; short boxes last with two planes per range
def test_accumulate_and_gate_bits(Bn, T):
    """The backward-data epilogue (accumulate, 1-bit gate) behind every kind of box of a 28 x 28 map with a t-edge box;
    a partial channel chunk and several column tiles."""
    c = Case(T, 28, 28, 24, 96, "bf16x6", seed=37, B=Bn)
    base = torch.randn((Bn, T, 28, 28, 96), generator=c.gen)
    gate = torch.rand((Bn, T, 28, 28, 96), generator=c.gen) > 0.3
    want = ((base.double() + c.ref) * gate).numpy()
    bits = (gate.view(Bn, T, 28, 28, 12, 8).to(torch.uint8) << torch.arange(8, dtype=torch.uint8)).sum(-1).to(torch.uint8).cuda()
    base = base.cuda()
    for v in (BOX8, BOX7, KS2, WIDE):
        out = c.backward_form(v, False, base, bits)
        err = rel_err(out.cpu().numpy(), want)
        assert err < 1e-5, f"variant {v}: {err:.3g} from torch fp64"
        assert torch.equal(c.backward_form(v, True, base, bits), out), f"variant {v}: differs from the embedded map"


@pytest.mark.parametrize("variant", [X3_BKH16, X3_BKH32])
def test_bf16x3(variant):
    """Split-bf16 (two activation planes), 16- and 32-channel chunks; 8 planes: short boxes last."""
    c = Case(16, 28, 28, 16, 96, "bf16x3", seed=41)
    y = c.forward(variant, embedded=False)
    err = rel_err(y.cpu().numpy(), c.ref_relu)
    assert err < 1e-4, f"{err:.3g} from torch fp64"   # (the split-bf16 bound of tests/test_gpu_halo_edge_boxes.py)
    assert torch.equal(c.forward(variant, embedded=True), y)
