// LDS-halo convolution (conv3d_halo_impl.h): the AM_X3 instantiations (fp32 activations split hi/lo, 3 MFMA passes)
// and the mode-independent host side: applicability, tile dispatch by arithmetic mode, built-in tile choice.
#include "conv3d_halo_impl.h"

namespace ivf {

template int conv_halo_launch_variant_am<AM_X3>(ConvKArgs& a, int v, hipStream_t s);
// the other two modes are instantiated in their own translation units (conv3d_halo_x6.hip, conv3d_halo_bf16.hip)
extern template int conv_halo_launch_variant_am<AM_X6>(ConvKArgs& a, int v, hipStream_t s);
extern template int conv_halo_launch_variant_am<AM_BF16>(ConvKArgs& a, int v, hipStream_t s);

int conv_halo_supported(const ConvKArgs& a) {
  if (a.sT != 1 || a.sH != 1 || a.sW != 1) return 0;
  if (a.kT * a.kH * a.kW <= 1 || a.kT > 4 || a.kH > 4 || a.kW > 4) return 0;
  if (a.Cin % 8) return 0;
  return 1;
}

int conv_halo_num_variants() { return HALO_NUM_VARIANTS; }

int conv_halo_launch_variant(ConvKArgs& a, int math, int v, hipStream_t s) {
  switch (math) {
    case IVF_MATH_BF16X3: return conv_halo_launch_variant_am<AM_X3>(a, v, s);
    case IVF_MATH_BF16X6: return conv_halo_launch_variant_am<AM_X6>(a, v, s);
    case IVF_MATH_BF16ACT: return conv_halo_launch_variant_am<AM_BF16>(a, v, s);
  }
  set_error("conv3d_halo: arithmetic mode %d has no LDS-halo kernel", math);
  return IVF_ERR_UNSUPPORTED;
}

// Built-in choice when the plan has not been tuned: tile index per output-channel width, for maps with 4-frame boxes
// (To >= 4) and for shallower ones.
struct HaloDefault { int width, deep, shallow; };
static const HaloDefault kHaloDefault[5] = {{192, 0, 8}, {128, 1, 9}, {96, 3, 10}, {64, 5, 11}, {32, 7, 12}};
// three activation planes: 16-channel chunks (4-frame boxes) or 2-frame boxes with at most 128 columns
// (68 = the 8-wave form of tile 60: as fast or faster on data, and not at the register budget's edge)
static const HaloDefault kHaloDefaultX6[5] = {{192, 68, 18}, {128, 61, 9}, {96, 20, 10}, {64, 21, 11}, {32, 37, 12}};

int conv_halo_default(const ConvKArgs& a, int math) {
  const HaloDefault* tab = math == IVF_MATH_BF16X6 ? kHaloDefaultX6 : kHaloDefault;
  // Output-channel tile width: every tile re-stages the halo, so weigh padded columns against
  // the number of tiles (a staging pass costs about as much as ~40 columns of MFMA work).
  int best = 4, best_cost = 1 << 30;
  for (int i = 0; i < 5; ++i) {
    int w = tab[i].width;
    int cost = cdiv(a.Cout, w) * (w + 40);
    if (cost < best_cost) { best_cost = cost; best = i; }
  }
  return a.To >= 4 ? tab[best].deep : tab[best].shallow;
}

}  // namespace ivf
