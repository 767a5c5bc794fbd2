"""CPU: the caller-owned scratch of the spacetime search and of Integrated Gradients is the sum of its documented
pieces, each rounded up to 256 bytes (include/ivf_hip.h; StScratch and IgScratch of csrc/search_driver.h).  The piece
order and sizes are part of the ABI: callers allocate by these two queries."""
import pytest


def _sum256(pieces):
    return sum((n + 255) // 256 * 256 for n in pieces)


@pytest.mark.parametrize("B,T,H,W,gh,gw", [(2, 16, 120, 160, 4, 5), (1, 1, 7, 7, 1, 1)])
def test_stsearch_workspace_is_the_sum_of_its_pieces(B, T, H, W, gh, gw):
    import ivf_lib as L
    px, cells = B * T * H * W * 4, B * T * gh * gw * 4
    pieces = [px, px, cells, cells, cells, B * 3 * 4, B * 4]           # M, dM, sig, dreg, dsig, terms [B,3], score [B]
    assert L.lib().ivf_stsearch_workspace_bytes(B, T, H, W, gh, gw) == _sum256(pieces)


@pytest.mark.parametrize("b,C,T,HW,K", [(3, 3, 16, 49, 5), (1, 1, 1, 1, 1)])
def test_ig_workspace_is_the_sum_of_its_pieces(b, C, T, HW, K):
    import ivf_lib as L
    pieces = [b * C * T * HW * 4, b * K * 4, b * K * 4]                # Gsum [b,C,T,HW], row targets [b,K], row scores [b,K]
    assert L.lib().ivf_ig_workspace_bytes(b, C, T, HW, K) == _sum256(pieces)
