"""LDS-halo convolutions on maps whose boxes hang over the H and W edges: a box there issues MFMAs only for the
waves that hold live tiles, and a box whose map ends within its first 4 columns runs a second row order.  Every
variant, on shapes that put boxes on the H edge, the narrow W edge and the corner, with Cout past the last column
tile -- against torch fp64, and bit for bit against the same variant on the zero-extended 16 x 16 map, where the
8 x 8 boxes are all interior."""
import ctypes

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

EXT = 16   # H and W of the zero-extended map: whole 8 x 8 boxes only


def to_cl(x):
    """NCTHW -> channels-last [B,T,H,W,C] on the GPU."""
    return x.permute(0, 2, 3, 4, 1).contiguous().cuda()


def extend(y, fill=0.0):
    """[B,T,H,W,C] -> [B,T,EXT,EXT,C], the original in the low corner."""
    B, T, H, W, C = y.shape
    e = torch.full((B, T, EXT, EXT, C), fill, device=y.device, dtype=y.dtype)
    e[:, :, :H, :W] = y
    return e


@pytest.mark.parametrize("math", ["fp32", "bf16x3", "bf16x6"])
@pytest.mark.parametrize("k,cin,cout,thw", [
    (3, 16, 40, (4, 12, 12)),    # H edge, narrow W edge and corner: 4 live h-rows of 8
    (3, 16, 200, (4, 14, 14)),   # 6 live h-rows in the standard order; dead column tiles at 192 / 128 / 96 columns
    (3, 24, 40, (4, 14, 12)),    # 7-row boxes with a narrow W edge; partial channel chunk
    (4, 8, 32, (4, 12, 12)),     # halo row pitch 11, plain (not depth-to-space) epilogue
])
def test_edge_boxes_match_torch_and_the_interior_path(k, cin, cout, thw, math):
    import torch.nn.functional as F
    import ivf_lib as L
    lib = L.lib()
    gen = torch.Generator().manual_seed(23)
    B = 2
    T, H, W = thw
    x = torch.randn((B, cin) + thw, generator=gen)
    w = torch.randn(cout, cin, k, k, k, generator=gen) * 0.1
    scale = torch.rand(cout, generator=gen) + 0.5
    shift = torch.randn(cout, generator=gen) * 0.1
    pf, pb = (k - 1) // 2, k - 1 - (k - 1) // 2
    ref = F.conv3d(F.pad(x.double(), (pf, pb, pf, pb, pf, pb)), w.double())
    ref_relu = torch.relu(ref * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1))
    ref_relu = ref_relu.permute(0, 2, 3, 4, 1).numpy()
    mm = L.MATH_MODES[math]
    tol = 1e-4 if math == "bf16x3" else 1e-5
    wf = torch.empty(lib.ivf_conv3d_pack_fwd_elems(cout, cin, k, k, k, mm), device='cuda')
    wd, scd, shd = w.cuda(), scale.cuda(), shift.cuda()   # (kept alive: L.ptr only takes the address)
    L.check(lib.ivf_conv3d_pack_fwd(L.ptr(wd), L.ptr(wf), cout, cin, cin, k, k, k, mm, L.stream()))
    base = torch.randn((B,) + thw + (cout,), generator=gen).cuda()
    gate = (torch.rand((B,) + thw + (cout,), generator=gen) > 0.3).float().cuda()
    want_acc = ((base.double().cpu() + ref.permute(0, 2, 3, 4, 1)) * gate.double().cpu()).numpy()
    xcl = to_cl(x)
    # the same data on the extended map: zeros beyond H x W are what the padding of the small map reads
    xcl_e, base_e, gate_e = extend(xcl), extend(base), extend(gate, 1.0)

    def desc(h, wd_):
        d = L.ConvDesc()
        d.B, d.Ti, d.Hi, d.Wi = B, T, h, wd_
        d.Cin, d.in_ld, d.in_coff = cin, cin, 0
        d.To, d.Ho, d.Wo = T, h, wd_
        d.Cout, d.out_ld, d.out_coff = cout, cout, 0
        d.kT = d.kH = d.kW = k
        d.sT = d.sH = d.sW = 1
        d.pT = d.pH = d.pW = pf
        d.math = mm
        d.mask_ld, d.mask_coff = cout, 0
        return d

    d, e = desc(H, W), desc(EXT, EXT)
    ids = (ctypes.c_int * 96)()
    n = lib.ivf_conv3d_variants(ctypes.byref(d), ids, 96)
    assert n >= 3
    ran = 0
    for v in list(ids)[:n]:
        d.variant = e.variant = v
        d.relu = e.relu = 1
        d.accumulate = e.accumulate = 0
        y = torch.full((B,) + thw + (cout,), float('nan'), device='cuda')
        rc = lib.ivf_conv3d(ctypes.byref(d), L.ptr(xcl), L.ptr(wf), L.ptr(scd), L.ptr(shd), None, L.ptr(y), L.stream())
        if rc != 0:
            continue   # variant not applicable to this shape (LDS budget)
        ran += 1
        assert rel_err(y.cpu().numpy(), ref_relu) < tol, f"variant {v}"
        y_e = torch.full((B, T, EXT, EXT, cout), float('nan'), device='cuda')
        L.check(lib.ivf_conv3d(ctypes.byref(e), L.ptr(xcl_e), L.ptr(wf), L.ptr(scd), L.ptr(shd), None, L.ptr(y_e),
                               L.stream()))
        assert torch.equal(y_e[:, :, :H, :W], y), f"variant {v}: edge boxes differ from interior boxes"
        d.relu = e.relu = 0
        d.accumulate = e.accumulate = 1
        acc = base.clone()
        L.check(lib.ivf_conv3d(ctypes.byref(d), L.ptr(xcl), L.ptr(wf), None, None, L.ptr(gate), L.ptr(acc), L.stream()))
        assert rel_err(acc.cpu().numpy(), want_acc) < tol, f"variant {v} (accumulate)"
        acc_e = base_e.clone()
        L.check(lib.ivf_conv3d(ctypes.byref(e), L.ptr(xcl_e), L.ptr(wf), None, None, L.ptr(gate_e), L.ptr(acc_e),
                               L.stream()))
        assert torch.equal(acc_e[:, :, :H, :W], acc), f"variant {v} (accumulate): edge boxes differ from interior boxes"
    assert ran >= 3
