// (implementation header: included by conv3d_halo.hip / conv3d_halo_x6.hip / conv3d_halo_bf16.hip, one operand mode each)
// Stride-1 k x k x k (k <= 4) convolution, split-bf16 MFMA, with the input
// neighbourhood held in LDS: the kernel that carries the 3x3x3 Inception branches, their
// backward-data, and the stem's 4x4x4 depth-to-space backward-data.
//
// The plain implicit GEMM (conv3d.hip) re-loads every input element once per tap and per
// output-channel tile; at split-bf16 MFMA speed that load stream (~10 TB/s through L1/L2),
// not the matrix cores, bounds it.  Here a workgroup owns a TT x 8 x 8 box of output
// positions; per 32-channel chunk it stages the (TT+k-1) x (8+k-1) x (8+k-1) input halo
// ONCE (global -> registers -> split hi/lo bf16 -> LDS), then sweeps all k^3 taps over it:
// a tap only changes the LDS row offset of the A fragments.  Only the small weight tile
// (BN x 32) streams per tap, double-buffered so its loads fly under the previous tap's MFMAs
// (one barrier per tap).  Input bytes per MAC drop ~8x for 3x3x3.
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "conv_common.h"

namespace ivf {

// Diagnostic build only (make stamps -> libivf_hip_stamps.so, tools/halo_stamps.py): thread 0 of every
// workgroup adds its cycles per phase to g_halo_stamps; the product build compiles none of it.
#ifdef IVF_HALO_STAMPS
static __device__ unsigned long long g_halo_stamps[8];
#define IVF_STAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define IVF_STAMP_RT(var) const unsigned long long var = __builtin_amdgcn_s_memrealtime()   // 100 MHz
#define IVF_STAMP_ADD(slot, t1, t0) \
  do { if (threadIdx.x == 0) atomicAdd(&g_halo_stamps[slot], (t1) - (t0)); } while (0)
#else
#define IVF_STAMP(var) do {} while (0)
#define IVF_STAMP_RT(var) do {} while (0)
#define IVF_STAMP_ADD(slot, t1, t0) do {} while (0)
#endif

// Position (h, w) inside the 8 x 8 plane of a tile for plane-row p in [0,64): two 32-row MFMA
// tiles (4 h-rows x 8 w each).  Which lane bit feeds which coordinate bit is free as long as
// the A operand and the epilogue agree; the choice per halo width minimises LDS bank conflicts
// of the 16-byte fragment reads (rows are 80 B apart; 3-way with the natural order, 2-way so).
__device__ __forceinline__ void tile_hw(int p, int hw_pitch, int* h, int* w) {
  const int b0 = p & 1, b1 = (p >> 1) & 1, b2 = (p >> 2) & 1, b3 = (p >> 3) & 1, b4 = (p >> 4) & 1;
  const int half = p >> 5;
  int hl, ww;
  if (hw_pitch == 10) {          // k = 3
    ww = b0 | (b2 << 1) | (b1 << 2);
    hl = b3 | (b4 << 1);
  } else if (hw_pitch == 11) {   // k = 4
    ww = b0 | (b2 << 1) | (b3 << 2);
    hl = b1 | (b4 << 1);
  } else {
    ww = p & 7;
    hl = (p >> 3) & 3;
  }
  *h = half * 4 + hl;
  *w = ww;
}

// Box row -> (t, h, w) inside a TT x TH x TW box.
//  * 4 x 8 x 8 boxes: a 32-row MFMA tile is one h-row of the box across its 4 planes (4 t x 8 w).
//    The halo plane stride of a 3x3x3 conv is 100 rows = 4 (mod 16), so the four planes' 8-row runs
//    start at 16-byte bank slots 0, 4, 8, 12 of the 256-byte LDS bank row: putting planes {0,2} on
//    one ds_read_b128 lane group ({0-3,12-15,20-27}, MI355X_MICROARCH.md) and {1,3} on the other
//    makes the A-fragment reads conflict-free (the earlier one-plane tiles could not be: one slot
//    is hit three times by any 4 h x 8 w cell set at row pitch 10).  For k = 2 and 4 this order is
//    as good as the old one (2-way).
//  * other 8 x 8 boxes (TT = 2) keep the permuted one-plane order above;
//  * other plane shapes (4 x 14: the 28 x 28 and 14 x 14 maps of Mixed_3*/4*, which 8 x 8 boxes
//    cover with 23 % of their rows outside the map) use raster order.
template <int TT, int TH, int TW>
__device__ __forceinline__ void box_pos(int row, int hw_pitch, int* t, int* h, int* w) {
  if constexpr (TT == 4 && TW == 8) {   // (any TH: a tile is one h-row of the box)
    const int li = row & 31, q = li >> 2, ql = q & 3;
    const int sel = ((ql + 1) >> 1) & 1;
    *t = (q >> 2) ? 3 - sel : sel;
    *w = (ql >> 1) * 4 + (li & 3);
    *h = row >> 5;
  } else if constexpr (TH == 8 && TW == 8) {
    tile_hw(row & 63, hw_pitch, h, w);
    *t = row >> 6;
  } else {
    const int p = row % (TH * TW);
    *t = row / (TH * TW);
    *h = p / TW;
    *w = p % TW;
  }
}

// Narrow row order of a 4 x TH x 8 box whose map ends within its first 4 columns (the W-edge boxes of the 28 x 28
// maps): a 32-row MFMA tile is TWO h-rows of the box across its 4 planes (4 t x 2 h x 4 w), so ceil(TH / 2) tiles
// cover the live half of the box and the others issue nothing (see the live-tile mask in the kernel).  Lane bits
// feed t and the low two bits of w as in box_pos; the bit that picks the w half there picks the h-row of the pair
// here.  Rows with h >= TH (the second half of the last tile of a 7-row box, every later tile) are not part of the
// box: the kernel clamps their LDS address into it and stores nothing for them.
struct BoxPos { int t, h, w; };
__host__ __device__ constexpr BoxPos narrow_box_pos(int row) {
  const int li = row & 31, q = li >> 2, ql = q & 3;
  const int sel = ((ql + 1) >> 1) & 1;
  return BoxPos{(q >> 2) ? 3 - sel : sel, 2 * (row >> 5) + (ql >> 1), li & 3};
}
// the rows of a box that the narrow order keeps (h < TH) hit every (t < 4, h < TH, w < 4) exactly once
template <int TH>
constexpr bool narrow_order_is_exact() {
  bool seen[4 * TH * 4] = {};
  int n = 0;
  for (int row = 0; row < 4 * TH * 8; ++row) {
    const BoxPos p = narrow_box_pos(row);
    if (p.t < 0 || p.t >= 4 || p.w < 0 || p.w >= 4 || p.h < 0) return false;
    if (p.h >= TH) continue;
    const int k = (p.t * TH + p.h) * 4 + p.w;
    if (seen[k]) return false;
    seen[k] = true;
    ++n;
  }
  return n == 4 * TH * 4;
}
static_assert(narrow_order_is_exact<8>() && narrow_order_is_exact<7>(), "narrow row order must be injective onto t<4, h<TH, w<4");

// LDS rows per halo plane.  The 4 x 8 x 8 boxes want the plane stride = 4 (mod 8) rows (see
// box_pos): 100 for k = 3 as it is, 121 -> 124 for k = 4, 81 -> 84 for k = 2 (pad rows are
// never staged nor read).
template <int TT, int TH, int TW>
__host__ __device__ constexpr int halo_plane_rows(int HH, int HW) {
  int ps = HH * HW;
  if (TT == 4 && TW == 8) ps += (4 - ps % 8 + 8) % 8;
  return ps;
}

// KS = 2 splits the taps of a chunk between two groups of waves (each wave then owns a
// bigger output sub-tile, i.e. fewer LDS fragment reads per MFMA: what narrow outputs such as
// the stem's 32-column backward-data need); the two partial sums meet in LDS at the end.
// BKH = channels per chunk: 32, or 16 to halve the LDS footprint so that TWO workgroups are
// resident per CU and one's halo staging / weight pipeline overlaps the other's MFMAs.
// TPS = taps per barrier interval ("step"): the weight tiles of TPS taps sit in each LDS buffer and the waves sweep
// them without meeting.  Every barrier costs the MFMA pipe about 1000 idle cycles (the waves re-issue their fragment
// reads together; profiles/r02_halo_phase_stamps.txt), which a narrow tile (32 columns: 6 MFMAs per wave per
// tap) cannot amortise over one tap.
// DMA = the weight tiles go from global memory straight into LDS (global_load_lds_dwordx4: no register ring, no
// ds_write_b128, no wait on the data inside the step): unpadded 64-byte rows, the 16-byte slot of a row XOR-ed
// with (row >> 2) & 3 -- the permutation is applied to the SOURCE address of every lane (the DMA writes lane i's
// 16 bytes at M0 + 16 i), and a lane's fragment address is a per-lane constant, so the tap loop pays nothing for it.
// AM = operand mode (conv_common.h): NPA activation planes and NPB weight planes sit in LDS, the tap loop issues the
// mode's MFMA sequence per 16-deep k-step (3 / 2 / 6 passes); AM_BF16 stages bf16 activations as they are and its
// epilogue stores bf16 (the depth-to-space forms always write fp32: the stem's input gradient).
// SL = short boxes last: the tile decode below for launches with short edge boxes (halo_short_edges != 0); every other
// launch runs the SL = false kernel, whose decode is the plain box order and which never reads short_edges.
template <int AM, int TT, int BN, int WROWS, int WCOLS, int KS, int BKH, int TH, int TW, int TPS, bool DMA, bool SL>
__global__ __launch_bounds__((TT * TH * TW / WROWS) * (BN / WCOLS) * KS * 64) void conv3d_halo_kernel(ConvKArgs a,
                                                                                                int tilesT,
                                                                                                int tilesH,
                                                                                                int tilesW,
                                                                                                int short_edges) {
  constexpr int BM = TT * TH * TW;
  constexpr int NPA = OpPlanes<AM>::A, NPB = OpPlanes<AM>::B;
  static_assert(BM % WROWS == 0 && WROWS % 32 == 0 && BN % WCOLS == 0 && WCOLS % 32 == 0, "tile");
  static_assert((KS * BN * (BKH / 8)) % 64 == 0, "weight-stream slots must fill whole waves");
  constexpr int WM = BM / WROWS, WN = BN / WCOLS;
  constexpr int NT = WM * WN * KS * 64;
  constexpr int TM = WROWS / 32, TN = WCOLS / 32;
  constexpr int ROWB = (BKH + 8) * 2;   // bytes per LDS row per plane (80 / 48: conflict-free 16-byte reads)
  constexpr int ROWB_B = DMA ? BKH * 2 : ROWB;   // weight rows: unpadded + swizzled in DMA mode
  static_assert(!DMA || BKH == 32, "the LDS-DMA weight stream is written for 32-channel chunks");
  constexpr int G4 = BKH / 4;           // float4 groups per halo row
  constexpr int G8 = BKH / 8;           // 16-byte weight groups per row per plane
  constexpr int BLOADS = (TPS * KS * BN * G8 + NT - 1) / NT;   // 16-byte weight loads per thread per plane per step

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  IVF_STAMP(st_begin);
  IVF_STAMP_RT(rt_begin);
  const int HT = TT + a.kT - 1, HH = TH + a.kH - 1, HW = TW + a.kW - 1;
  const int PS = halo_plane_rows<TT, TH, TW>(HH, HW);   // LDS rows per halo plane (>= HH * HW)
  const int HR = HT * PS;
  unsigned char* a_hi = smem;                              // NPA planes of HR rows, APL bytes apart
  const size_t APL = (size_t)HR * ROWB;
  unsigned char* b_base = smem + (size_t)NPA * HR * ROWB;   // [2 buffers][TPS taps][KS groups][NPB planes][BN rows]
  int* rowoff = reinterpret_cast<int*>(b_base + (size_t)2 * NPB * TPS * KS * BN * ROWB_B);   // [HR] input offset of a halo row / in_ld, or -1

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: tap decode and tile bases stay on the scalar unit
  const int wk = wave / (WM * WN);               // tap group of this wave
  // A workgroup's waves go to the four SIMDs cyclically (MI355X_MICROARCH.md), so wave % 4 names a wave's SIMD.  With
  // two column halves the half alternates with the h-row PAIR: then the live waves are spread evenly over the SIMDs
  // when the box's last h-rows are dead (any even number of them) and also when one column half is (see below).
  const int wm = (wave % (WM * WN)) / WN;
  const int wn = WN == 2 ? (wave & 1) ^ ((wm >> 1) & 1) : wave % WN;
  const int li = lane & 31, lh = lane >> 5;

  // tile decode: n-tile fastest, then w, h, t, b
  int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int nt = tile % a.ntiles;
  tile /= a.ntiles;
  int tw, th;
  if constexpr (SL) {
    // Short boxes last (halo_short_edges: the narrow last box column, a last box row half live or less).  A short box
    // takes about half to two thirds of a full box's time and the wide tiles run one workgroup per CU, a few rounds of
    // them per launch (32 clips on a 28 x 28 map: 1024 boxes, 4 per CU, 7 of every 16 short).  Dealt in box order the
    // short ones leave the CUs uneven when the launch ends; dealt after the full ones they fill its last round
    // (profiles/halo_edge_order.txt).  "Last" is per XCD: xcd_remap hands each XCD one contiguous eighth of the grid,
    // so the order is made inside each eighth, ppc = planes / 8 planes (clips x t-boxes) each.  The launch asks for
    // this order only when the planes divide into eighths: over the whole grid it would give the low XCDs all the
    // full boxes and the high ones all the short ones.  Which workgroup computes a box changes nothing in the box.
    static_assert(TT == 4 && TW == 8, "short boxes exist in the 4 x TH x 8 tiles only");
    const int CI = tilesW - (short_edges & 1), RI = tilesH - (short_edges >> 1);
    const int ppc = (a.B * tilesT) >> 3;
    const int range = tile / (ppc * tilesH * tilesW);
    int r = tile - range * (ppc * tilesH * tilesW), pl;
    th = tilesH - 1, tw = tilesW - 1;
    if (r < ppc * RI * CI) {                                     // full boxes: w, h, plane
      tw = r % CI;
      r /= CI;
      th = r % RI;
      pl = r / RI;
    } else if ((r -= ppc * RI * CI) < ppc * RI * (tilesW - CI)) {   // last column above the corner
      th = r % RI;
      pl = r / RI;
    } else if ((r -= ppc * RI * (tilesW - CI)) < ppc * CI * (tilesH - RI)) {   // last row left of the corner
      tw = r % CI;
      pl = r / CI;
    } else {                                                     // the corner
      pl = r - ppc * CI * (tilesH - RI);
    }
    tile = range * ppc + pl;
  } else {
    tw = tile % tilesW;
    tile /= tilesW;
    th = tile % tilesH;
    tile /= tilesH;
  }
  const int tt = tile % tilesT;
  const int b = tile / tilesT;
  const int t0 = tt * TT, h0 = th * TH, w0 = tw * TW;
  const int n0 = nt * BN;

  // Live waves (wave-uniform, kept in scalars).  A box that hangs over the map's H edge, or a column tile past Cout,
  // holds 32-row x 32-column MFMA tiles that nobody stores: a wave ALL of whose tiles are such issues no fragment reads
  // and no MFMAs.  It still stages the halo, streams the weights and meets every barrier.
  // In a 4 x TH x 8 box MFMA row tile k is h-row k of the box (box_pos), or, in a box whose map ends within its first
  // 4 columns, h-rows {2k, 2k + 1} of its live half (narrow_box_pos; the depth-to-space epilogue keeps the standard
  // order).  The operands and the order of every stored value's sum are those of a fully live box.
  // (A wave with live AND dead tiles -- 64-row wave tiles, 96-column wave tiles over 288 + 32 columns -- computes them
  // all: a second, tile-masked copy of the tap loop costs the wide tiles 20-30 registers, and the 16-wave 192-column
  // tile, which sits at its 128, went from 20 to 292 bytes of scratch with it.)
  constexpr bool EDGE_TILES = TT == 4 && TW == 8;
  bool narrow = false;
  int live_tiles = WM * TM;
  if constexpr (EDGE_TILES) {
    const int live_h = min(TH, a.Ho - h0);
    narrow = !a.d2s && a.Wo - w0 <= 4;
    live_tiles = narrow ? (live_h + 1) >> 1 : live_h;
  }
  const bool wave_live = wm * TM < live_tiles && n0 + wn * WCOLS < a.Cout;
  // box row -> (t, h, w) in the order this workgroup runs; h >= TH marks a row outside the box (narrow order only)
  auto row_pos = [&](int row, int* t, int* h, int* w) __attribute__((always_inline)) {
    box_pos<TT, TH, TW>(row, HW, t, h, w);
    if constexpr (EDGE_TILES) {
      if (narrow) {
        const BoxPos p = narrow_box_pos(row);
        *t = p.t, *h = p.h, *w = p.w;
      }
    }
  };

  // A-fragment base rows of this lane (one per 32-row MFMA tile of the wave)
  int arow[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    int r = wm * WROWS + i * 32 + li;
    int pt, ph, pw;
    row_pos(r, &pt, &ph, &pw);
    arow[i] = pt * PS + min(ph, TH - 1) * HW + pw;   // (a row outside the box is never stored: any address inside the halo does)
  }
  const int ntaps = a.kT * a.kH * a.kW;
  const int ntg = (ntaps + KS - 1) / KS;         // tap group g handles taps [g*ntg, (g+1)*ntg)
  const int nsteps = (ntg + TPS - 1) / TPS;      // barrier intervals per chunk; step s = group-local taps [s*TPS, (s+1)*TPS)
  const int khw = a.kH * a.kW;
  // halo row -> input position (decoded once; the chunk loop only adds the channel offset)
  for (int row = tid; row < HR; row += NT) {
    int ht = row / PS;
    int rem = row - ht * PS;
    int hh = rem / HW;
    int hw = rem - hh * HW;
    int ti = t0 - a.pT + ht, hi = h0 - a.pH + hh, wi = w0 - a.pW + hw;
    bool ok = hh < HH && (unsigned)ti < (unsigned)a.Ti && (unsigned)hi < (unsigned)a.Hi && (unsigned)wi < (unsigned)a.Wi;
    rowoff[row] = ok ? ((b * a.Ti + ti) * a.Hi + hi) * a.Wi + wi : -1;
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // Weight tiles stream through a register ring PF taps deep (their L2 latency is longer than
  // one tap of MFMAs and there is a single workgroup per CU, so nothing else would hide it) and
  // a double-buffered LDS tile.
  constexpr int PF = 3;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  u32x4 rb[PF][NPB][BLOADS] = {};
  // Per-thread constants of the weight stream, decoded once: the tap loop only adds the tap and the chunk.  (The
  // scalar unit is what a narrow tile runs out of: 75 scalar + 28 vector instructions per tap beside 6 MFMAs
  // measured 53 % scalar-busy at 36 % MFMA-busy on the stem's backward-data.)
  // Every thread loads every step, from an address clamped into the weight array, with no validity branch and no
  // zero fill: a slot outside the step, tap range, layer rows or channels holds finite weights of some other
  // position, which meet staged zeros (channels), are skipped (taps) or land in columns nobody stores (rows).
  // Straight-line loads are what lets the compiler count them (`s_waitcnt vmcnt(N)`): behind a branch it waited
  // for vmcnt(0) right after issuing the prefetch, i.e. exposed a full L2 round trip per tap.
  int b_src[BLOADS];    // element offset min(n, Cout - 1) * ldw into wbf (0 for threads without a slot)
  int b_dst[BLOADS];    // byte offset in one LDS weight buffer [TPS][KS][hi, lo][BN rows]; -1 = no slot
  int b_tap[BLOADS];    // sub-tap + group * ntg: tap of step s = s * TPS + b_tap
  int b_c[BLOADS];      // channel offset inside the chunk
#pragma unroll
  for (int q = 0; q < BLOADS; ++q) {
    const int idx = tid + q * NT;
    const int sub = idx / (KS * BN * G8);
    const int r1 = idx - sub * (KS * BN * G8);
    const int grp = r1 / (BN * G8);
    const int rem = r1 - grp * (BN * G8);
    const int row = BKH == 32 ? perm8(rem / G8) : rem / G8, g2 = rem % G8;
    const int n = min(n0 + row, a.Cout - 1);
    b_src[q] = sub < TPS ? n * a.ldw : 0;
    b_dst[q] = sub < TPS ? ((sub * KS + grp) * NPB * BN + row) * ROWB_B + 16 * g2 : -1;
    b_tap[q] = sub < TPS ? sub + grp * ntg : 0;
    b_c[q] = 8 * g2;
  }
  // Kept straight-line on purpose: no scalar branch around the loads or the stores (lanes without a slot are
  // masked off, which is not a branch for a block this short), and the loop below issues them every step.  Then
  // the compiler can count (`s_waitcnt vmcnt(4)` before a slot is stored); behind any control-flow join it falls
  // back to vmcnt(0) right after issuing the prefetch.  (Hand-issued asm loads were tried: the compiler copies
  // asm outputs between registers while the load is still in flight.)
  auto load_b = [&](int slot, int step, int c0) __attribute__((always_inline)) {
    const int s0 = min(step, nsteps - 1) * TPS;
#pragma unroll
    for (int q = 0; q < BLOADS; ++q) {
      const int tap = min(s0 + b_tap[q], ntaps - 1);
      int c = c0 + b_c[q];
      c = c < a.Cin ? c : 0;
      const unsigned short* p = a.wbf + (size_t)(b_src[q] + tap * a.Cin + c);
      if (b_dst[q] >= 0) {
#pragma unroll
        for (int pl = 0; pl < NPB; ++pl) rb[slot][pl][q] = *reinterpret_cast<const u32x4*>(p + pl * a.w_lo_off);
      }
    }
  };
  auto store_b = [&](int slot, int buf) __attribute__((always_inline)) {
    unsigned char* bb = b_base + (size_t)buf * (TPS * KS * NPB * BN * ROWB_B);
#pragma unroll
    for (int q = 0; q < BLOADS; ++q) {
      if (b_dst[q] >= 0) {
#pragma unroll
        for (int pl = 0; pl < NPB; ++pl) *reinterpret_cast<u32x4*>(bb + b_dst[q] + pl * BN * ROWB_B) = rb[slot][pl][q];
      }
    }
  };
  // tap -> byte offset of its halo row shift, advanced tap by tap on the scalar unit (no divisions in the loop);
  // this wave's tap group starts at tap wk * ntg
  int g_kw, g_kh, g_toff;
  {
    const int tap0 = wk * ntg;
    const int kt = tap0 / khw;
    const int rem = tap0 - kt * khw;
    g_kh = rem / a.kW;
    g_kw = rem - g_kh * a.kW;
    g_toff = (kt * PS + g_kh * HW + g_kw) * ROWB;
  }
  int t_kw = 0, t_kh = 0, t_off = 0;   // running state of the current chunk
  auto tap_advance = [&]() __attribute__((always_inline)) {
    t_off += ROWB;
    if (++t_kw == a.kW) {
      t_kw = 0;
      t_off += (HW - a.kW) * ROWB;
      if (++t_kh == a.kH) {
        t_kh = 0;
        t_off += (PS - a.kH * HW) * ROWB;
      }
    }
  };
  int abase[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) abase[i] = arow[i] * ROWB + 16 * lh;
  // weight-fragment offsets of this lane inside a (tap, group) tile: column tile j, 16-channel slice ks
  auto b_off = [&](int j, int ks) __attribute__((always_inline)) {
    const int row = wn * WCOLS + j * 32 + li;
    if constexpr (DMA) return row * ROWB_B + 16 * ((2 * ks + lh) ^ ((row >> 2) & 3));
    else return row * ROWB_B + ks * 32 + 16 * lh;
  };
  // ---- LDS-DMA weight stream: piece p (16 bytes) of a buffer = [sub][group][plane][row][physical slot], i.e. byte 16 p
  constexpr int NP = TPS * KS * NPB * BN * (BKH / 8), NI = NP / 64, NWV = NT / 64, MAXI = (NI + NWV - 1) / NWV;
  int d_base[MAXI], d_tap[MAXI], d_c[MAXI];
  if constexpr (DMA) {
#pragma unroll
    for (int k = 0; k < MAXI; ++k) {
      const int p = (wave + k * NWV) * 64 + lane;
      const int slot = p % G8, row = (p / G8) % BN, plane = (p / (G8 * BN)) % NPB;
      const int grp = (p / (G8 * BN * NPB)) % KS, sb = p / (G8 * BN * NPB * KS);
      d_base[k] = plane * (int)a.w_lo_off + min(n0 + row, a.Cout - 1) * a.ldw;
      d_tap[k] = sb + grp * ntg;
      d_c[k] = 8 * (slot ^ ((row >> 2) & 3));
    }
  }
  auto dma_b = [&](int step, int buf, int c0) __attribute__((always_inline)) {
    if constexpr (DMA) {
#pragma unroll
      for (int k = 0; k < MAXI; ++k) {
        if (wave + k * NWV >= NI) continue;   // (wave-uniform)
        const int tap = min(step * TPS + d_tap[k], ntaps - 1);
        int c = c0 + d_c[k];
        c = c < a.Cin ? c : 0;
        const unsigned short* g = a.wbf + (size_t)(d_base[k] + tap * a.Cin + c);
        // the compiler's own LDS-DMA builtin: it owns M0 (destination = wave-uniform LDS base, lane i writes 16 bytes
        // at base + 16 i) and knows that LDS is written
        unsigned char* dst = b_base + (size_t)buf * (TPS * KS * NPB * BN * ROWB_B) + (size_t)(wave + k * NWV) * 1024;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
      }
    }
  };
  // One step = the TPS taps of an LDS weight buffer.  Narrow wave tiles (one MFMA tile, 6 MFMAs per tap) run a
  // software pipeline over the (tap, 16-channel slice) units of the step: the fragments of unit u+1 are in flight
  // while unit u's MFMAs issue, so a wave exposes one LDS round trip per step instead of two per slice.
  constexpr int NKS = BKH / 16;
  constexpr bool PIPELINED = (TM == 1 && TN == 1);
  auto mma_tap = [&](int step, int buf, int nks) __attribute__((always_inline)) {
    const int lt0 = step * TPS;
    // valid taps of this wave's group in the step; none for a wave without a live tile
    const int nsub = wave_live ? min(TPS, min(ntg - lt0, ntaps - wk * ntg - lt0)) : 0;
    if (nsub <= 0) return;
    const unsigned char* bstep = b_base + (size_t)(buf * TPS * KS + wk) * NPB * BN * ROWB_B;   // + sub * KS * NPB * BN * ROWB_B
    if constexpr (PIPELINED) {   // (a partial last chunk runs all NKS slices: channels past Cin are staged as zeros)
      bf16x8 fa[2][NPA], fb[2][NPB];
      auto issue = [&](int slot, int sub, int ks) __attribute__((always_inline)) {
        const int aoff = abase[0] + t_off + ks * 32;
        const unsigned char* bh = bstep + (size_t)sub * KS * NPB * BN * ROWB_B + b_off(0, ks);
#pragma unroll
        for (int pl = 0; pl < NPA; ++pl) fa[slot][pl] = *reinterpret_cast<const bf16x8*>(a_hi + pl * APL + aoff);
#pragma unroll
        for (int pl = 0; pl < NPB; ++pl) fb[slot][pl] = *reinterpret_cast<const bf16x8*>(bh + (size_t)pl * BN * ROWB_B);
      };
      issue(0, 0, 0);
#pragma unroll
      for (int u = 0; u < TPS * NKS; ++u) {
        if (u / NKS < nsub) {
          if (u + 1 < TPS * NKS && (u + 1) / NKS < nsub) {
            if ((u + 1) % NKS == 0) tap_advance();
            issue((u + 1) & 1, (u + 1) / NKS, (u + 1) % NKS);
          }
          mma_planes<AM>(fa[u & 1], fb[u & 1], acc[0][0]);
          // keep the source order: next unit's fragment reads, then this unit's MFMAs
          __builtin_amdgcn_sched_group_barrier(0x100, NPA + NPB, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, AM == AM_X6 ? 6 : (AM == AM_BF16 ? 2 : 3), 0);
        }
      }
      tap_advance();
    } else {
#pragma unroll
      for (int sub = 0; sub < TPS; ++sub) {
        if (sub >= nsub) break;
        const unsigned char* bh = bstep + (size_t)sub * KS * NPB * BN * ROWB_B;
        for (int ks = 0; ks < nks; ++ks) {
          bf16x8 fa[TM][NPA];
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const int off = abase[i] + t_off + ks * 32;
#pragma unroll
            for (int pl = 0; pl < NPA; ++pl) fa[i][pl] = *reinterpret_cast<const bf16x8*>(a_hi + pl * APL + off);
          }
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int off = b_off(j, ks);
            bf16x8 fb[NPB];
#pragma unroll
            for (int pl = 0; pl < NPB; ++pl) fb[pl] = *reinterpret_cast<const bf16x8*>(bh + (size_t)pl * BN * ROWB_B + off);
#pragma unroll
            for (int i = 0; i < TM; ++i) mma_planes<AM>(fa[i], fb, acc[i][j]);
          }
        }
        tap_advance();
      }
    }
  };

  // halo staging, synchronous in batches of 4 loads per thread: 8 float4 groups per halo row (fetching the NEXT
  // chunk's halo into registers under the current chunk's taps was measured twice -- 256-thread tiles in round 2,
  // the 512-/1024-thread three-plane tiles in round 3 with 16-28 registers to spare: nothing gained either time;
  // what an ablated staging phase saves (4-12 %) is its memory traffic, not its latency)
  constexpr int NSTG = 4;
  float4 stg[NSTG];
  // (rows are visited in perm8 order, so the item range is padded to whole blocks of 8 rows)
  const int ngroups = BKH == 32 ? ((HR + 7) & ~7) * G4 : HR * G4;
  int stage_base = 0;
  auto stage_load = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NSTG; ++u) {
      int idx = stage_base + u * NT + tid;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < ngroups) {
        int row = BKH == 32 ? perm8(idx / G4) : idx / G4, g = idx % G4;
        if (row >= HR) row = -1;
        int c = c0 + 4 * g;
        int pos = row >= 0 ? rowoff[row] : -1;
        if (pos >= 0 && c < a.Cin) v = load_act4<AM>(a.in, (size_t)pos * a.in_ld + a.in_coff + c);
      }
      stg[u] = v;
    }
  };
  auto stage_store = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NSTG; ++u) {
      int idx = stage_base + u * NT + tid;
      const int srow = BKH == 32 ? perm8(idx / G4) : idx / G4;
      if (idx < ngroups && srow < HR) {
        stage_planes<AM>(a_hi + srow * ROWB + 8 * (idx % G4), APL, stg[u]);
      }
    }
  };
  __syncthreads();   // rowoff table is complete

  for (int c0 = 0; c0 < a.Cin; c0 += BKH) {
    // weight tiles of the first PF taps start flying before the halo is staged
    if constexpr (!DMA) {
      load_b(0, 0, c0);
      load_b(1, 1, c0);
      load_b(2, 2, c0);
    }
    __syncthreads();   // everyone is done with the previous chunk's halo and weight buffers
    dma_b(0, 0, c0);   // (DMA mode: the first step's tiles land in buffer 0 while the halo is staged)
    IVF_STAMP(st_s0);
    for (stage_base = 0; stage_base < ngroups; stage_base += NSTG * NT) {
      stage_load(c0);
      stage_store();
    }
    stage_base = 0;
    // everything the compiler knows to be in flight has landed by now; saying so keeps its conservative
    // `s_waitcnt vmcnt(0)` (staging registers reused by the fragment reads) out of the tap loop, where it would
    // drain the weight prefetch every step
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    if constexpr (!DMA) store_b(0, 0);
    __syncthreads();
    IVF_STAMP(st_s1);
    IVF_STAMP_ADD(1, st_s1, st_s0);

    const int cw = min(BKH, a.Cin - c0);
    const int nks = (cw + 15) >> 4;
    t_kw = g_kw, t_kh = g_kh, t_off = g_toff;
    // tap loop unrolled by PF so the register ring is statically indexed: at tap (slot u)
    // the LDS buffer tap&1 holds its weights; slot u is refilled with tap+PF, and slot u+1's
    // weights (tap+1, loaded PF-1 taps ago) move to the other LDS buffer after the MFMAs.
    auto tap_body = [&](auto U, int tap0) __attribute__((always_inline)) {
      constexpr int u = decltype(U)::value;
      const int tap = tap0 + u;   // step index within the chunk (the last round may run past nsteps: no MFMAs then)
      load_b(u, tap + PF, c0);
      if (tap < nsteps) mma_tap(tap, tap & 1, nks);
      store_b((u + 1) % PF, (tap + 1) & 1);
      __syncthreads();
    };
    static_assert(PF == 3, "tap loop is unrolled by hand for a 3-deep ring");
    if constexpr (DMA) {
      // step t: the tiles of step t+1 start towards the other buffer (free since the barrier that ended step t-1),
      // the MFMAs of step t run, then the wave waits for its own DMA and everybody meets
      for (int tap = 0; tap < nsteps; ++tap) {
        if (tap + 1 < nsteps) dma_b(tap + 1, (tap + 1) & 1, c0);
        mma_tap(tap, tap & 1, nks);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    } else {
      for (int tap0 = 0; tap0 < nsteps; tap0 += PF) {
        tap_body(std::integral_constant<int, 0>{}, tap0);
        tap_body(std::integral_constant<int, 1>{}, tap0);
        tap_body(std::integral_constant<int, 2>{}, tap0);
      }
    }
    IVF_STAMP(st_s2);
    IVF_STAMP_ADD(2, st_s2, st_s1);
  }
  IVF_STAMP(st_loop_end);

  if constexpr (KS == 2) {
    // meet the two tap groups: group 1 parks its partial sums in LDS (the halo is dead now),
    // group 0 adds them and owns the epilogue
    float* red = reinterpret_cast<float*>(smem);
    const int slot = (wm * WN + wn) * TM * TN;
    // (the two waves of an output sub-tile are live or dead together; a dead one's sums are never stored)
    if (wk == 1 && wave_live) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) red[((slot + i * TN + j) * 16 + r) * 64 + lane] = acc[i][j][r];
    }
    __syncthreads();
    if (wk == 0 && wave_live) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] += red[((slot + i * TN + j) * 16 + r) * 64 + lane];
    }
    __syncthreads();   // the reduction buffer may be reused below
  }

  // Depth-to-space output of a full 2x2x2 block conv with 4-channel pixels (the stem's
  // backward-data): every lane quad holds one 16-byte pixel and a wave's direct stores land as
  // 32-byte pieces.  Park the tile in LDS as [2TT][16][16][4] and write whole 256-byte pixel
  // rows instead.
  if (TH == 8 && TW == 8 && BN == 32 && a.d2s && a.Cout == 32 && a.bsT == 2 && a.bsH == 2 && a.bsW == 2 && !a.accumulate && !a.relu &&
      a.dC == 4 && (a.out_ld & 3) == 0 && (a.out_coff & 3) == 0) {
    float* ot = reinterpret_cast<float*>(smem);
    if (wk == 0) {
      const int n = wn * WCOLS + li;          // TN == 1 for BN == 32
      const int par = n >> 2, c = n & 3;
      const int pt = par >> 2, ph = (par >> 1) & 1, pw = par & 1;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm * WROWS + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          int bt, bh, bw;
          box_pos<TT, TH, TW>(row, HW, &bt, &bh, &bw);
          const int tt2 = 2 * bt + pt, hh2 = 2 * bh + ph, ww2 = 2 * bw + pw;
          ot[((tt2 * 16 + hh2) * 16 + ww2) * 4 + c] = acc[i][0][r];
        }
    }
    __syncthreads();
    for (int p = tid; p < 2 * TT * 256; p += NT) {
      const int t = 2 * t0 + (p >> 8), h = 2 * h0 + ((p >> 4) & 15), w = 2 * w0 + (p & 15);
      if (t < a.dT && h < a.dH && w < a.dW)
        *reinterpret_cast<float4*>(a.out + ((size_t)((b * a.dT + t) * a.dH + h) * a.dW + w) * a.out_ld + a.out_coff) =
            *reinterpret_cast<const float4*>(ot + (size_t)p * 4);
    }
    IVF_STAMP(st_end_d2s);
    IVF_STAMP_RT(rt_end_d2s);
    IVF_STAMP_ADD(5, rt_end_d2s, rt_begin);
    IVF_STAMP_ADD(3, st_end_d2s, st_loop_end);
    IVF_STAMP_ADD(0, st_end_d2s, st_begin);
    IVF_STAMP_ADD(4, st_begin + 1, st_begin);      // workgroup count
    return;
  }
  if (wk != 0 || !wave_live) return;   // (every row or every column of a wave without a live tile is outside the output)

  conv_epilogue<AM, TM, TN>(
      a, acc,
      [&](int row) {
        int pt, ph, pw;
        row_pos(row, &pt, &ph, &pw);
        int t = t0 + pt, h = h0 + ph, w = w0 + pw;
        if (ph >= TH || t >= a.To || h >= a.Ho || w >= a.Wo) return -1;
        return ((b * a.To + t) * a.Ho + h) * a.Wo + w;
      },
      wm * WROWS, n0 + wn * WCOLS, li, lh);
  IVF_STAMP(st_end);
  IVF_STAMP_RT(rt_end);
  IVF_STAMP_ADD(5, rt_end, rt_begin);
  IVF_STAMP_ADD(3, st_end, st_loop_end);
  IVF_STAMP_ADD(0, st_end, st_begin);
  IVF_STAMP_ADD(4, st_begin + 1, st_begin);        // workgroup count
}

#if defined(IVF_HALO_STAMPS) && defined(IVF_HALO_STAMPS_OWNER)
}  // namespace ivf
// slots: 0 total, 1 halo staging (+ first weight tile), 2 tap loops, 3 reduction + epilogue, 4 workgroups,
// 5 total in 100 MHz s_memrealtime ticks (slot 0 / slot 5 x 100 MHz = the clock the chip held)
extern "C" int ivf_debug_halo_stamps(unsigned long long* out8, int reset) {
  IVF_CHECK_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(ivf::g_halo_stamps), 8 * sizeof(unsigned long long)));
  if (reset) {
    unsigned long long z[8] = {0};
    IVF_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(ivf::g_halo_stamps), z, sizeof(z)));
  }
  return IVF_OK;
}
namespace ivf {
#endif

// The tiles (ivf_conv3d_desc.variant = IVF_CONV_HALO_BASE + index): the kernel's template arguments after the operand
// mode.  Box TT x TH x TW, BN output columns, wave tile WROWS x WCOLS, KS tap groups, BKH channels per chunk, TPS taps
// per barrier, DMA weight stream.  Declared once: the launch table, the built set and the built-in choice
// (conv3d_halo.hip) all read this array.
struct HaloTile { int TT, BN, WROWS, WCOLS, KS, BKH, TH, TW, TPS; bool DMA; };
constexpr HaloTile kHaloTiles[] = {
    // 4- and 2-frame 8 x 8 boxes, 32-channel chunks, one tap per barrier
    {4, 192, 32,  96, 1, 32, 8,  8, 1, false},   // 0
    {4, 128, 64,  64, 1, 32, 8,  8, 1, false},
    {4, 128, 32,  64, 1, 32, 8,  8, 1, false},
    {4,  96, 32,  96, 1, 32, 8,  8, 1, false},
    {4,  64, 32,  64, 1, 32, 8,  8, 1, false},
    {4,  64, 64,  64, 2, 32, 8,  8, 1, false},   // 5
    {4,  32, 32,  32, 1, 32, 8,  8, 1, false},
    {4,  32, 64,  32, 2, 32, 8,  8, 1, false},
    {2, 192, 32,  96, 1, 32, 8,  8, 1, false},
    {2, 128, 32,  64, 1, 32, 8,  8, 1, false},
    {2,  96, 32,  96, 1, 32, 8,  8, 1, false},   // 10
    {2,  64, 32,  64, 1, 32, 8,  8, 1, false},
    {2,  32, 32,  32, 1, 32, 8,  8, 1, false},
    {2,  64, 64,  64, 2, 32, 8,  8, 1, false},
    {2, 128, 64,  64, 1, 32, 8,  8, 1, false},
    {4,  64, 32,  64, 2, 32, 8,  8, 1, false},   // 15
    {4,  96, 32,  96, 2, 32, 8,  8, 1, false},
    {4,  32, 32,  32, 2, 32, 8,  8, 1, false},
    // 16-channel chunks (two workgroups per CU)
    {2, 192, 32,  96, 1, 16, 8,  8, 1, false},   // 18
    {2, 128, 32,  64, 1, 16, 8,  8, 1, false},
    {4,  96, 32,  96, 1, 16, 8,  8, 1, false},   // 20
    {4,  64, 32,  64, 1, 16, 8,  8, 1, false},
    {2,  96, 32,  96, 1, 16, 8,  8, 1, false},
    // 4 x 4 x 14 boxes (224 rows = 7 MFMA row tiles; exact on 28- and 14-wide maps)
    {4, 192, 32,  96, 1, 32, 4, 14, 1, false},   // 23
    {4, 128, 32,  64, 1, 32, 4, 14, 1, false},
    {4,  96, 32,  96, 1, 32, 4, 14, 1, false},   // 25
    {4,  64, 32,  64, 1, 32, 4, 14, 1, false},
    {4,  32, 32,  32, 1, 32, 4, 14, 1, false},
    {4,  64, 32,  32, 1, 32, 4, 14, 1, false},
    {4,  32, 32,  32, 2, 32, 4, 14, 1, false},
    {4, 128, 32, 128, 1, 32, 4, 14, 1, false},   // 30
    // narrow outputs on 16-channel chunks (two or three workgroups per CU: one's per-tap barrier and LDS round trip
    // hide under another's MFMAs -- what the 32-column stem backward-data is short of)
    {2,  32, 64,  32, 2, 16, 8,  8, 1, false},   // 31
    {2,  32, 32,  32, 2, 16, 8,  8, 1, false},
    {2,  32, 32,  32, 1, 16, 8,  8, 1, false},
    {2,  64, 32,  64, 2, 16, 8,  8, 1, false},
    {2,  64, 64,  64, 2, 16, 8,  8, 1, false},   // 35
    {4,  32, 64,  32, 2, 16, 8,  8, 1, false},
    {4,  32, 32,  32, 2, 16, 8,  8, 1, false},
    // several taps per barrier interval (narrow outputs; 16-channel chunks leave the LDS room; 46: k <= 3)
    {4,  32, 32,  32, 2, 16, 8,  8, 4, false},   // 38
    {4,  32, 64,  32, 2, 16, 8,  8, 4, false},
    {4,  32, 32,  32, 2, 16, 8,  8, 2, false},   // 40
    {2,  32, 32,  32, 2, 32, 8,  8, 2, false},
    {4,  64, 32,  64, 1, 16, 8,  8, 2, false},
    {4,  64, 32,  64, 1, 32, 8,  8, 2, false},
    {4,  32, 32,  32, 1, 16, 8,  8, 4, false},
    {4,  96, 32,  96, 1, 16, 8,  8, 2, false},   // 45
    {4,  32, 32,  32, 2, 32, 8,  8, 2, false},
    {4,  64, 32,  64, 1, 32, 4, 14, 2, false},
    // 4 x 7 x 8 boxes (7 one-h-row tiles, conflict-free like the 4 x 8 x 8 ones; exact in H on 28- and 14-row maps)
    {4, 192, 32,  96, 1, 32, 7,  8, 1, false},   // 48
    {4, 128, 32,  64, 1, 32, 7,  8, 1, false},
    {4,  96, 32,  96, 1, 16, 7,  8, 1, false},   // 50
    {4,  64, 32,  64, 1, 16, 7,  8, 1, false},
    // weight tiles by LDS-DMA (global_load_lds_dwordx4, swizzled 64-byte rows)
    {4, 192, 32,  96, 1, 32, 8,  8, 1, true},    // 52
    {4, 192, 32,  96, 1, 32, 4, 14, 1, true},
    {4, 128, 32,  64, 1, 32, 4, 14, 1, true},
    {4, 128, 32,  64, 1, 32, 8,  8, 1, true},    // 55
    {4,  32, 32,  32, 2, 32, 8,  8, 1, true},
    {4, 128, 32,  64, 1, 32, 7,  8, 1, true},
    {4,  96, 32,  96, 1, 32, 8,  8, 1, true},
    {4,  64, 32,  64, 1, 32, 8,  8, 1, true},
    // wide tiles on 16-channel chunks (what fits beside the THREE activation planes of the 6-pass mode)
    {4, 192, 32,  96, 1, 16, 8,  8, 1, false},   // 60
    {4, 128, 32,  64, 1, 16, 8,  8, 1, false},
    {4, 192, 32,  96, 1, 16, 4, 14, 1, false},
    {4, 128, 32,  64, 1, 16, 4, 14, 1, false},
    {4,  96, 32,  96, 1, 16, 4, 14, 1, false},
    {4,  64, 32,  64, 1, 16, 4, 14, 1, false},   // 65
    {4, 192, 32,  96, 1, 16, 7,  8, 1, false},
    {4, 128, 32,  64, 1, 16, 7,  8, 1, false},
    // the same wide tiles on 8 waves of 64-row wave tiles (two waves per SIMD with 256 registers each, 9 fragment
    // reads per 12 MFMA groups instead of 12 per 9)
    {4, 192, 64,  96, 1, 16, 8,  8, 1, false},   // 68
    {4, 128, 64,  64, 1, 16, 8,  8, 1, false},
};
constexpr int HALO_NUM_VARIANTS = sizeof(kHaloTiles) / sizeof(kHaloTiles[0]);
constexpr size_t HALO_LDS_MAX = 160 * 1024;

// LDS bytes tile V needs with NPA activation and NPB weight planes: halo planes, two weight buffers, the row-offset
// table; or, where larger, a buffer that reuses the LDS from offset 0 once the tap loops are done (everything staged is
// dead by then): the tap-split reduction [BM][BN] floats, the depth-to-space tile [2 TT][16][16][4] floats.
template <int V>
constexpr size_t halo_lds_bytes(int NPA, int NPB, int kT, int kH, int kW, bool d2s) {
  constexpr HaloTile t = kHaloTiles[V];
  constexpr int ROWB = (t.BKH + 8) * 2, ROWB_B = t.DMA ? t.BKH * 2 : ROWB;
  const size_t HR = (size_t)(t.TT + kT - 1) * halo_plane_rows<t.TT, t.TH, t.TW>(t.TH + kH - 1, t.TW + kW - 1);
  size_t shm = NPA * HR * ROWB + (size_t)2 * t.TPS * t.KS * NPB * t.BN * ROWB_B + HR * sizeof(int);
  if (t.KS == 2) shm = std::max(shm, (size_t)t.TT * t.TH * t.TW * t.BN * 4);
  if (d2s) shm = std::max(shm, (size_t)2 * t.TT * 256 * 4 * sizeof(float));
  return shm;
}

// Which edges of the box grid hold short boxes, which the SL kernel deals last: bit 0 = the last box column is narrow
// (4 x TH x 8 boxes whose map ends within their first 4 columns: half the MFMA tiles, narrow_box_pos), bit 1 = the
// last box row is half live or less.  A grid of a single column or row has no "last"; and the order is made per
// eighth of the grid (see the kernel), so a launch whose planes do not divide by 8 keeps the box order.
static int halo_short_edges(const HaloTile& t, const ConvKArgs& a, int tilesT, int tilesH, int tilesW) {
  if (t.TT != 4 || t.TW != 8 || a.d2s || (a.B * tilesT) % 8) return 0;
  const int narrow = tilesW > 1 && a.Wo - (tilesW - 1) * t.TW <= 4;
  const int low = tilesH > 1 && 2 * (a.Ho - (tilesH - 1) * t.TH) <= t.TH;
  return narrow | (low << 1);
}

// A tile is built for an operand mode only if its LDS footprint fits for the 3x3x3 case (the 6-pass mode holds three
// activation planes: mostly the 16-channel-chunk tiles remain); anything else reports IVF_ERR_UNSUPPORTED.
template <int AM, int V>
static int launch_halo(ConvKArgs& a, hipStream_t s) {
  constexpr HaloTile t = kHaloTiles[V];
  if constexpr (halo_lds_bytes<V>(OpPlanes<AM>::A, OpPlanes<AM>::B, 3, 3, 3, false) > HALO_LDS_MAX) {
    set_error("conv3d_halo: variant %d needs more than 160 KB of LDS in this arithmetic mode", V);
    return IVF_ERR_UNSUPPORTED;
  } else {
    constexpr int NT = (t.TT * t.TH * t.TW / t.WROWS) * (t.BN / t.WCOLS) * t.KS * 64;
    const size_t shm = halo_lds_bytes<V>(OpPlanes<AM>::A, OpPlanes<AM>::B, a.kT, a.kH, a.kW, a.d2s);
    if (shm > HALO_LDS_MAX) {
      set_error("conv3d_halo: %zu bytes of LDS needed", shm);
      return IVF_ERR_UNSUPPORTED;
    }
    const int tilesT = cdiv(a.To, t.TT), tilesH = cdiv(a.Ho, t.TH), tilesW = cdiv(a.Wo, t.TW);
    // two kernels per 4 x TH x 8 tile: the box order, and short boxes last for launches that have short boxes
    const int short_edges = halo_short_edges(t, a, tilesT, tilesH, tilesW);
    auto kernel = &conv3d_halo_kernel<AM, t.TT, t.BN, t.WROWS, t.WCOLS, t.KS, t.BKH, t.TH, t.TW, t.TPS, t.DMA, false>;
    static LdsAttrOnce once[2];
    if constexpr (t.TT == 4 && t.TW == 8) {
      if (short_edges) kernel = &conv3d_halo_kernel<AM, t.TT, t.BN, t.WROWS, t.WCOLS, t.KS, t.BKH, t.TH, t.TW, t.TPS, t.DMA, true>;
    }
    IVF_PROPAGATE(raise_lds_limit(reinterpret_cast<const void*>(kernel), HALO_LDS_MAX, once[short_edges != 0]));
    a.ntiles = cdiv(a.Cout, t.BN);
    a.mtiles = a.B * tilesT * tilesH * tilesW;
    prof_name(IVF_CONV_HALO_BASE + V, "conv3d_halo_kernel<%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%s>", AM, t.TT, t.BN, t.WROWS, t.WCOLS,
              t.KS, t.BKH, t.TH, t.TW, t.TPS, t.DMA ? "true" : "false");
    const bool timed = prof_begin(s, IVF_CONV_HALO_BASE + V);
    hipLaunchKernelGGL(kernel, dim3(a.mtiles * a.ntiles), dim3(NT), shm, s, a, tilesT, tilesH, tilesW, short_edges);
    if (timed) prof_end(s);
    IVF_CHECK_LAUNCH();
    return IVF_OK;
  }
}

template <int AM, size_t... V>
static int halo_dispatch(ConvKArgs& a, int v, hipStream_t s, std::index_sequence<V...>) {
  static constexpr int (*launch[])(ConvKArgs&, hipStream_t) = {&launch_halo<AM, (int)V>...};
  return launch[v](a, s);
}

template <int AM>
int conv_halo_launch_variant_am(ConvKArgs& a, int v, hipStream_t s) {
  if (v < 0 || v >= HALO_NUM_VARIANTS) {
    set_error("conv3d_halo: unknown variant %d", v);
    return IVF_ERR_BAD_ARG;
  }
  return halo_dispatch<AM>(a, v, s, std::make_index_sequence<HALO_NUM_VARIANTS>{});
}

}  // namespace ivf
