// Grid-mask staging shared by RISE (rise_ops.hip), Shapley sampling (shapley_ops.hip) and the deletion / insertion
// curves (curve_ops.hip): a row of the flattened candidate list is a clip frozen per pixel by a BINARY mask on a grid
// (gt, gh, gw); the three differ only in which cells a row freezes.  Internal: not part of include/ivf_hip.h.
//
// Frame u belongs to temporal cell kt = (u gt) / T, cell c = (kt gh + i) gw + j.  Staging writes what
// ivf_stmask_expand_fwd + ivf_stfreeze_fwd write for the row's explicit S [T,gh,gw] (S[u] = S_row[kt(u)]), without S or M
// in memory.  With S in {0, 1} the expand's sums lose their zero terms exactly (the comment above box_mask_at in
// stmask_ops.hip), so per pixel and temporal cell
//   tmp[i] = sum_{j set, ascending} A_W[x,j]
//   M      = sum_{i ascending, all i} A_H[y,i] * tmp[i]
// every partial sum rounded as stmask_expand_fwd_kernel rounds it (no contraction: a multiply and an add each), then the
// recurrence expression of ivf_stfreeze_fwd.
//
// A family gives a row source `Rows`, a small struct passed to the kernels by value:
//   rows.cells(r, P) -> { int clip; bool frozen(int c) const; }       row r of the list, P = gt gh gw
// frozen() is asked only while the row's column words are filled into LDS, before the scan; the scan itself is written
// out once in each kernel below and is the same code for every family (a scan pulled into an inlined helper
// cost 34 VGPRs; here the kernel stays whole and only the word fill is the parameter).
#pragma once
#include "ivf_common.h"

namespace ivf {

constexpr int GRID_MAX_SIDE = 32;       // gh, gw: the bits of a grid row are one 32-bit word
constexpr int GRID_MAX_PLAYERS = 4096;  // ranks fit in uint16, a row's keys in 16 KiB of LDS
constexpr int LIN_MAX_PLAYERS = 1024;   // linear surrogates (linsur_ops.hip): the fp64 normal matrix is [P,P], 8 MiB

struct Grid3 {
  int gt, gh, gw;
};

// ---------------------------------------------------------------- hash
// h(seed, k, c) = fmix32( fmix32(seed + 0x9E3779B9 (k + 1)) ^ (0x85EBCA77 (c + 1)) )   (uint32, wrapping), fmix32 the
// finaliser of MurmurHash3: grid_key is the part that belongs to mask / permutation k, grid_hash the rest.
__device__ __forceinline__ unsigned fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ unsigned grid_key(unsigned seed, int k) { return fmix32(seed + 0x9E3779B9u * (unsigned)(k + 1)); }
__device__ __forceinline__ unsigned grid_hash(unsigned key, int c) { return fmix32(key ^ (0x85EBCA77u * (unsigned)(c + 1))); }

// ---------------------------------------------------------------- counting rank
// #{o : (keys[o], o) < (keys[c], c)} over the P keys in LDS (all lanes read the same word: a broadcast, no bank
// conflict); a tie falls to the lower index.  A counting rank, not a sort: it needs one barrier, gives the rank (the
// inverse permutation a sort would still have to scatter) directly, and breaks ties by index for free.
__device__ __forceinline__ int grid_count_rank(const unsigned* keys, int P, int c) {
  const unsigned h = keys[c];
  int r = 0;
  for (int o = 0; o < P; ++o) {
    const unsigned v = keys[o];
    r += (v < h || (v == h && o < c)) ? 1 : 0;
  }
  return r;
}

// ---------------------------------------------------------------- staging
// One workgroup per (row, 256 pixels).  The row's gt * gh column words (bit j = cell (kt, i, j) frozen) are built once
// in LDS; every thread parks row x of A_W in its own LDS column (aw[j * 256 + tid]: a wave reads 64 consecutive words,
// no bank conflict, and nobody reads another thread's column).  The words are the workgroup's, so the loop over the set
// bits is uniform.  M is computed once on entering a temporal cell.
struct GridLds {
  unsigned* word;
  float* aw;
};

template <class Cells>
__device__ __forceinline__ GridLds grid_fill_lds(unsigned* lds, const float* __restrict__ AW, const Grid3& g,
                                                 const Cells& q, int x) {
  GridLds l;
  l.word = lds;
  l.aw = reinterpret_cast<float*>(lds + g.gt * g.gh);
  const int tid = threadIdx.x;
  for (int w = tid; w < g.gt * g.gh; w += 256) {
    unsigned bits = 0;
    for (int j = 0; j < g.gw; ++j) bits |= (q.frozen(w * g.gw + j) ? 1u : 0u) << j;
    l.word[w] = bits;
  }
  for (int j = 0; j < g.gw; ++j) l.aw[j * 256 + tid] = AW[(size_t)x * g.gw + j];
  __syncthreads();
  return l;
}

// M[y,x] of the row's mask on the frames of temporal cell kt; A_H row y is read through the cache (a wave mostly
// shares its row y)
__device__ __forceinline__ float grid_mask_at(const GridLds& l, const float* __restrict__ AHy, int gh, int kt) {
  float m = 0.f;
  for (int i = 0; i < gh; ++i) {
    unsigned w = l.word[kt * gh + i];
    float t = 0.f;
    while (w) {
      t += l.aw[(__ffs(w) - 1) * 256 + threadIdx.x];
      w &= w - 1;
    }
    m += AHy[i] * t;
  }
  return m;
}

// 16-byte channels-last pixels (C <= 4), as box_stage_cl4_kernel: with TT > 0 (T == TT) the 16 frames of a piece are
// requested before the scan goes over them.
template <int TT, class Rows>   // TT: 0, or a multiple of 16
__global__ __launch_bounds__(256) void grid_stage_cl4_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                             const float* __restrict__ AW, float* __restrict__ p, int C,
                                                             int Trun, int W, int HW, Grid3 g, Rows rows,
                                                             long long first) {
  extern __shared__ unsigned grid_lds[];
  const int row = blockIdx.y, T = TT > 0 ? TT : Trun;
  const auto q = rows.cells(first + row, g.gt * g.gh * g.gw);
  const int pxu = blockIdx.x * 256 + threadIdx.x;
  const int px = min(pxu, HW - 1);          // threads past the end stage LDS for a valid pixel, then leave
  const GridLds l = grid_fill_lds(grid_lds, AW, g, q, px % W);
  if (pxu >= HW) return;
  const float* AHy = AH + (size_t)(px / W) * g.gh;
  const float* xc = x + (size_t)q.clip * C * T * HW + px;
  float* pr = p + ((size_t)row * T * HW + px) * 4;
  float prev[4] = {0.f, 0.f, 0.f, 0.f};
  int cur = -1;
  float m = 0.f;
  if constexpr (TT > 0) {
#pragma unroll 1
    for (int u0 = 0; u0 < TT; u0 += 16) {
      float xv[4][16];
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          xv[ch][j] = 0.f;
          if (ch < C) xv[ch][j] = xc[((size_t)ch * TT + u0 + j) * HW];
        }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int u = u0 + j, kt = (u * g.gt) / TT;
        if (kt != cur) {
          cur = kt;
          m = grid_mask_at(l, AHy, g.gh, kt);
        }
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
          if (ch < C) {
            v[ch] = u ? (1.f - m) * xv[ch][j] + m * prev[ch] : xv[ch][j];
            prev[ch] = v[ch];
          }
        *reinterpret_cast<float4*>(pr + (size_t)u * HW * 4) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  } else {
    for (int u = 0; u < T; ++u) {
      const int kt = (u * g.gt) / T;
      if (kt != cur) {
        cur = kt;
        m = grid_mask_at(l, AHy, g.gh, kt);
      }
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      for (int ch = 0; ch < C; ++ch) {
        float xv = xc[((size_t)ch * T + u) * HW];
        v[ch] = u ? (1.f - m) * xv + m * prev[ch] : xv;
        prev[ch] = v[ch];
      }
      *reinterpret_cast<float4*>(pr + (size_t)u * HW * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// NCTHW: channel after channel (the mask value is the pixel's, not the channel's; it is recomputed per channel from LDS)
template <class Rows>
__global__ __launch_bounds__(256) void grid_stage_ncthw_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                               const float* __restrict__ AW, float* __restrict__ p, int C,
                                                               int T, int W, int HW, Grid3 g, Rows rows, long long first) {
  extern __shared__ unsigned grid_lds[];
  const int row = blockIdx.y;
  const auto q = rows.cells(first + row, g.gt * g.gh * g.gw);
  const int pxu = blockIdx.x * 256 + threadIdx.x;
  const int px = min(pxu, HW - 1);
  const GridLds l = grid_fill_lds(grid_lds, AW, g, q, px % W);
  if (pxu >= HW) return;
  const float* AHy = AH + (size_t)(px / W) * g.gh;
  for (int ch = 0; ch < C; ++ch) {
    const float* xp = x + ((size_t)q.clip * C + ch) * T * HW + px;
    float* pp = p + ((size_t)row * C + ch) * T * HW + px;
    float prev = 0.f, m = 0.f;
    int cur = -1;
    for (int u = 0; u < T; ++u) {
      const int kt = (u * g.gt) / T;
      if (kt != cur) {
        cur = kt;
        m = grid_mask_at(l, AHy, g.gh, kt);
      }
      float xv = xp[(size_t)u * HW];
      float v = u ? (1.f - m) * xv + m * prev : xv;
      prev = v;
      pp[(size_t)u * HW] = v;
    }
  }
}

// ---------------------------------------------------------------- host
// The grid of an entry `name`: 1 <= gt <= T <= MAX_T, 1 <= gh, gw <= GRID_MAX_SIDE and, with max_players > 0, at most that
// many cells.  An entry whose clip length is not its own passes MAX_T as T.
static inline int grid_check(const char* name, int T, int gt, int gh, int gw, int max_players = 0) {
  const bool sides = T >= 1 && T <= MAX_T && gt >= 1 && gt <= T && gh >= 1 && gh <= GRID_MAX_SIDE && gw >= 1 &&
                     gw <= GRID_MAX_SIDE;
  if (!max_players)
    IVF_CHECK_ARG(sides, "%s: need 1 <= gt (%d) <= T (%d) <= %d and 1 <= gh (%d), gw (%d) <= %d", name, gt, T, MAX_T, gh,
                  gw, GRID_MAX_SIDE);
  else
    IVF_CHECK_ARG(sides && gt * gh * gw <= max_players,
                  "%s: need 1 <= gt (%d) <= T (%d) <= %d, 1 <= gh (%d), gw (%d) <= %d and gt gh gw <= %d players", name, gt,
                  T, MAX_T, gh, gw, GRID_MAX_SIDE, max_players);
  return IVF_OK;
}

// The arguments the three ivf_*_stage entries share.  An entry refuses in this order: grid_stage_check (null pointers,
// dims, grid), its own arguments, grid_stage_launch (row window, layout, alignment) -- so it calls the two in turn.
struct GridStageArgs {
  const char* name;
  const float* x;
  int b, C, T, H, W;
  const float *A_H, *A_W;
  Grid3 g;
  long long first;
  int count;
  float* p;
  int out_cpad;
  ivf_stream_t stream;
};

// table_ok: the entry's further pointers, if it has any
static inline int grid_stage_check(const GridStageArgs& a, bool table_ok, int max_players) {
  IVF_CHECK_ARG(a.x && a.A_H && a.A_W && table_ok && a.p, "%s: null pointer", a.name);
  IVF_CHECK_ARG(a.b > 0 && a.C > 0 && a.H > 0 && a.W > 0 && (long long)a.H * a.W <= 0x7fffffffLL, "%s: bad dims", a.name);
  return grid_check(a.name, a.T, a.g.gt, a.g.gh, a.g.gw, max_players);
}

// rows [first, first + count) of the b clips' `total` rows (`what` names them in the refusal) into p
template <class Rows>
static int grid_stage_launch(const GridStageArgs& a, const Rows& rows, long long total, const char* what) {
  IVF_CHECK_ARG(a.first >= 0 && a.count > 0 && a.count <= 65535 && a.first + a.count <= total,
                "%s: rows [%lld, %lld) outside the %lld %s of %d clips (at most 65535 rows a call)", a.name, a.first,
                a.first + a.count, total, what, a.b);
  IVF_CHECK_ARG(a.out_cpad == 0 || (a.out_cpad == 4 && a.C <= 4),
                "%s: out_cpad must be 0 (NCTHW) or 4 (16-byte channels-last, C <= 4)", a.name);
  IVF_CHECK_ARG(a.out_cpad == 0 || ((uintptr_t)a.p & 15) == 0, "%s: the channels-last buffer is not 16-byte aligned",
                a.name);
  const int HW = a.H * a.W;
  const size_t lds = ((size_t)a.g.gt * a.g.gh + (size_t)a.g.gw * 256) * 4;      // at most 8 + 32 KiB
  hipStream_t s = (hipStream_t)a.stream;
  const dim3 grid(cdiv(HW, 256), a.count), block(256);
  if (a.out_cpad == 0)
    hipLaunchKernelGGL(grid_stage_ncthw_kernel<Rows>, grid, block, lds, s, a.x, a.A_H, a.A_W, a.p, a.C, a.T, a.W, HW, a.g,
                       rows, a.first);
  else
    with_frames_exact(a.T, [&](auto TT) {
      hipLaunchKernelGGL((grid_stage_cl4_kernel<TT, Rows>), grid, block, lds, s, a.x, a.A_H, a.A_W, a.p, a.C, a.T, a.W, HW,
                         a.g, rows, a.first);
    });
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

}  // namespace ivf
