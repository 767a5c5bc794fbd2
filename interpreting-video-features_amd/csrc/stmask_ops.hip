// Spatio-temporal perturbation masks (maskType 'spacetime'), an EXTENSION with no counterpart in the reference
// (SURVEY A10): a mask value per pixel and frame, parametrised on a coarse gh x gw grid per frame.
//
//   S = sigmoid(R), R [B,T,gh,gw]                                      (ivf_stmask_reg)
//   M[b,t] = A_H S[b,t] A_W^T, M [B,T,H,W]                             (ivf_stmask_expand_fwd; adjoint: _bwd)
//   P[0] = X[0], P[u] = (1 - M[u]) X[u] + M[u] P[u-1] per pixel        (ivf_stfreeze_fwd; dM: ivf_stfreeze_bwd)
//
// A = G U (bilinear upsampling then a Gaussian blur, folded into one matrix per axis on the host in fp64,
// ivf_stmask_axis_weights).  All of it is HBM-bound work beside the network's forward and backward: M is written once
// and read twice, dM written and read once per iteration.  No float atomics anywhere: every sum has a fixed order, so a
// clip's results do not depend on the batch it ran in.
#include <cmath>
#include <vector>

#include "search_driver.h"

namespace ivf {

constexpr int ST_MAX_GRID = 32;   // gh, gw

// ---------------------------------------------------------------- expand forward
// One block per (b*T + t, tile of 32 rows); columns in chunks of 128.  Per chunk: A_W rows of the chunk to LDS, then
// tmp[i][x] = sum_j S[i,j] A_W[x,j] (j ascending) to LDS, then M[y,x] = sum_i A_H[y,i] tmp[i][x] (i ascending), four
// columns per thread, one 16-byte store where the row allows it.  Zero entries of A are multiplied like any other:
// x + 0 * s == x for the finite, non-negative values involved, so the non-zero terms and their order are those of the
// dense sum.
constexpr int EX_ROWS = 32, EX_COLS = 128, EX_AWLD = ST_MAX_GRID + 1;

__global__ __launch_bounds__(256) void stmask_expand_fwd_kernel(const float* __restrict__ S, const float* __restrict__ AH,
                                                                const float* __restrict__ AW, float* __restrict__ M,
                                                                int gh, int gw, int H, int W, int vec_ok) {
  __shared__ float s_s[ST_MAX_GRID * ST_MAX_GRID];
  __shared__ float ah_s[EX_ROWS * ST_MAX_GRID];
  __shared__ float aw_s[EX_COLS * EX_AWLD];
  __shared__ __attribute__((aligned(16))) float tmp_s[ST_MAX_GRID * EX_COLS];
  const int bt = blockIdx.x;
  const int y0 = blockIdx.y * EX_ROWS;
  const int rows = min(EX_ROWS, H - y0);
  const int tid = threadIdx.x;
  for (int i = tid; i < gh * gw; i += 256) s_s[i] = S[(size_t)bt * gh * gw + i];
  for (int i = tid; i < rows * gh; i += 256) ah_s[i] = AH[(size_t)y0 * gh + i];
  float* Mbt = M + (size_t)bt * H * W;
  for (int x0 = 0; x0 < W; x0 += EX_COLS) {
    const int cols = min(EX_COLS, W - x0);
    __syncthreads();   // s_s / ah_s staged; the previous chunk's readers of aw_s / tmp_s are done
    for (int i = tid; i < cols * gw; i += 256) {
      const int xl = i / gw, j = i - xl * gw;
      aw_s[xl * EX_AWLD + j] = AW[(size_t)x0 * gw + i];
    }
    __syncthreads();
    for (int idx = tid; idx < gh * EX_COLS; idx += 256) {
      const int i = idx / EX_COLS, xl = idx % EX_COLS;
      float acc = 0.f;
      if (xl < cols)
        for (int j = 0; j < gw; ++j) acc += s_s[i * gw + j] * aw_s[xl * EX_AWLD + j];
      tmp_s[idx] = acc;
    }
    __syncthreads();
    const int q = tid % (EX_COLS / 4), yl0 = tid / (EX_COLS / 4);      // 32 quads x 8 rows per pass
    for (int yl = yl0; yl < rows; yl += 256 / (EX_COLS / 4)) {
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      for (int i = 0; i < gh; ++i) {
        const float a = ah_s[yl * gh + i];
        const float4 t = *reinterpret_cast<const float4*>(tmp_s + i * EX_COLS + q * 4);
        o[0] += a * t.x;
        o[1] += a * t.y;
        o[2] += a * t.z;
        o[3] += a * t.w;
      }
      const int xl = q * 4;
      float* dst = Mbt + (size_t)(y0 + yl) * W + x0 + xl;
      if (vec_ok && xl + 3 < cols) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
        for (int k = 0; k < 4; ++k)
          if (xl + k < cols) dst[k] = o[k];
      }
    }
  }
}

// ---------------------------------------------------------------- expand backward
// dS = A_H^T dM A_W, one block per (b, t) and one pass over dM, so a clip's result does not depend on the batch (the
// convention of clstm_cam_weights_kernel).  Columns in chunks of 256, one thread per column: tmp[i][x] = sum_y
// A_H[y,i] dM[y,x], y ascending, in registers (A_H rows staged 32 at a time), then to LDS.  Each (i,j) pair belongs to
// one wave: lanes sum tmp[i][x] A_W[x,j] over x = lane, lane + 64, ..., a shuffle tree adds the 64 lanes, and lane 0
// adds the chunk's sum to the pair's LDS cell -- chunks in ascending order.
constexpr int EB_COLS = 256, EB_ROWS = 32;

template <int GH>
__global__ __launch_bounds__(256) void stmask_expand_bwd_kernel(const float* __restrict__ dM, const float* __restrict__ AH,
                                                                const float* __restrict__ AW, float* __restrict__ dS,
                                                                int gh, int gw, int H, int W) {
  __shared__ float ah_s[EB_ROWS * GH];
  __shared__ float tmp_s[GH * EB_COLS];
  __shared__ float ds_s[GH * ST_MAX_GRID];
  const int bt = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* g = dM + (size_t)bt * H * W;
  for (int i = tid; i < gh * gw; i += 256) ds_s[i] = 0.f;
  for (int x0 = 0; x0 < W; x0 += EB_COLS) {
    const int cols = min(EB_COLS, W - x0);
    const int x = x0 + tid;
    float acc[GH];
#pragma unroll
    for (int i = 0; i < GH; ++i) acc[i] = 0.f;
    for (int y0 = 0; y0 < H; y0 += EB_ROWS) {
      const int rows = min(EB_ROWS, H - y0);
      __syncthreads();   // the previous tile's readers of ah_s (and the previous chunk's of tmp_s) are done
      for (int i = tid; i < rows * gh; i += 256) {
        const int yl = i / gh, k = i - yl * gh;
        ah_s[yl * GH + k] = AH[(size_t)y0 * gh + i];
      }
      __syncthreads();
      if (tid < cols) {
#pragma unroll 8
        for (int yl = 0; yl < rows; ++yl) {
          const float v = g[(size_t)(y0 + yl) * W + x];
#pragma unroll
          for (int i = 0; i < GH; ++i)
            if (i < gh) acc[i] += ah_s[yl * GH + i] * v;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < GH; ++i) tmp_s[i * EB_COLS + tid] = acc[i];     // zero beyond `cols` and beyond gh
    __syncthreads();
    for (int p = wave; p < gh * gw; p += 4) {
      const int i = p / gw, j = p - i * gw;
      float v = 0.f;
      for (int xl = lane; xl < cols; xl += 64) v += tmp_s[i * EB_COLS + xl] * AW[(size_t)(x0 + xl) * gw + j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
      if (lane == 0) ds_s[p] += v;       // pair p is this wave's alone
    }
  }
  __syncthreads();
  for (int i = tid; i < gh * gw; i += 256) dS[(size_t)bt * gh * gw + i] = ds_s[i];
}

// ---------------------------------------------------------------- per-pixel freeze backward
// G[T-1] = g[T-1], G[u] = g[u] + M[u+1] G[u+1];  dM[u] = sum_c (P[u-1] - X[u]) G[u], c = 0..C-1 in that order, u >= 1;
// dM[0] = 0.0.  One thread per (b, pixel): the pixel's mask values stay in registers over the channels, each channel's
// frames (and their gradient) are requested before its two scans, as in freeze_bwd_kernel.  No reduction across
// pixels, no workspace.  GL: layout of g -- 0 NCTHW, 1 channels-last rows of g_cpad, 2 16-byte rows (C <= 4; one load
// per frame serves all channels).  Pad lanes of g are never read into the arithmetic.
// Registers: five arrays of TT floats per thread (plus 4 TT for the 16-byte rows).  TT = 16 runs at 2-3 waves per
// SIMD; TT = 32 takes the whole 256-register file (one wave per SIMD); TT = 64 does not fit it in any layout -- the
// compiler parks 85 (NCTHW) to 208 (lane by lane) values in the accumulation registers, and a less lucky allocation
// puts them in scratch.  The results are the same; only TT = 16 (the S16 geometry) has been timed.
template <int TT, int GL>
__global__ __launch_bounds__(256) void stfreeze_bwd_kernel(const float* __restrict__ x, const float* __restrict__ M,
                                                           const float* __restrict__ g, float* __restrict__ dM, int B,
                                                           int C, int T, int HW, int g_cpad) {
  size_t total = (size_t)B * HW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int px = i % HW;
    int b = i / HW;
    float mm[TT], acc[TT];
#pragma unroll
    for (int u = 0; u < TT; ++u) {
      acc[u] = 0.f;
      mm[u] = (u > 0 && u < T) ? M[((size_t)b * T + u) * HW + px] : 0.f;
    }
    float4 gv[GL == 2 ? TT : 1];
    if constexpr (GL == 2) {
#pragma unroll
      for (int u = 0; u < TT; ++u)
        if (u < T) gv[u] = *reinterpret_cast<const float4*>(g + ((size_t)(b * T + u) * HW + px) * 4);
    }
    for (int c = 0; c < C; ++c) {
      const float* xp = x + ((size_t)(b * C + c) * T) * HW + px;
      float xv[TT], pv[TT], gq[TT];
#pragma unroll
      for (int u = 0; u < TT; ++u)
        if (u < T) xv[u] = xp[(size_t)u * HW];
#pragma unroll
      for (int u = 0; u < TT; ++u)
        if (u < T) {
          if constexpr (GL == 0) gq[u] = g[((size_t)(b * C + c) * T + u) * HW + px];
          else if constexpr (GL == 1) gq[u] = g[((size_t)(b * T + u) * HW + px) * g_cpad + c];
          else gq[u] = c == 0 ? gv[u].x : (c == 1 ? gv[u].y : (c == 2 ? gv[u].z : gv[u].w));
        }
#pragma unroll
      for (int u = 0; u < TT; ++u)
        if (u < T) pv[u] = u ? (1.f - mm[u]) * xv[u] + mm[u] * pv[u - 1] : xv[u];
      float G = 0.f;
#pragma unroll
      for (int u = TT - 1; u >= 0; --u) {
        if (u < T) {
          float mnext = (u + 1 < T) ? mm[u + 1 < TT ? u + 1 : u] : 0.f;
          G = gq[u] + mnext * G;
          if (u > 0) acc[u] += (pv[u - 1] - xv[u]) * G;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < TT; ++u)
      if (u < T) dM[((size_t)b * T + u) * HW + px] = u ? acc[u] : 0.f;
  }
}

// ---------------------------------------------------------------- regulariser
// J_reg = lam1 sum S / cells + lam2 TVt / cells + lam3 TVs / cells, cells = gh gw, S = sigmoid(R):
//   TVt = sum_cells sum_{u=1}^{T-2} |S[u-1]-S[u]|^3 + |S[u+1]-S[u]|^3  -- calc_tv_norm's `val` (mask.py:93-96) per cell,
//         i.e. sum over frame pairs (k, k+1) with weight w_k = [k <= T-3] + [k >= 1] (interior pairs count twice);
//         the reference's (val^(1/3))^3 is left out: the identity in value, a NaN gradient at val == 0;
//   TVs = sum_t sum |S[t,i+1,j]-S[t,i,j]|^3 + |S[t,i,j+1]-S[t,i,j]|^3.
// One workgroup per clip.  Every element adds its own S and the pairs it is the lower member of; a thread sums its
// elements in ascending order, then shuffle tree and the four waves in order.  The gradient is gathered per element
// (each pair it belongs to), neighbours' sigmoids recomputed: no scatter.
__device__ __forceinline__ float st_sigmoid(float r) { return 1.f / (1.f + expf(-r)); }
__device__ __forceinline__ float st_cube(float d) {
  d = fabsf(d);
  return d * d * d;
}
// d|a - s|^3 / ds = -3 (a - s)^2 sign(a - s)
__device__ __forceinline__ float st_dcube(float a, float s) {
  float d = a - s;
  float sg = (d > 0.f) - (d < 0.f);
  return -(3.f * (d * d)) * sg;
}

__global__ __launch_bounds__(256) void stmask_reg_kernel(const float* __restrict__ raw, int T, int gh, int gw, float lam1,
                                                         float lam2, float lam3, float* __restrict__ sig,
                                                         float* __restrict__ terms, float* __restrict__ dreg) {
  const int b = blockIdx.x;
  const int cells = gh * gw, n = T * cells;
  const float fc = (float)cells;
  const float* r = raw + (size_t)b * n;
  float l1 = 0.f, tvt = 0.f, tvs = 0.f;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int t = e / cells, cell = e - t * cells, i = cell / gw, j = cell - i * gw;
    const float s = st_sigmoid(r[e]);
    sig[(size_t)b * n + e] = s;
    l1 += fabsf(s);
    float gt = 0.f, gs = 0.f;
    if (T >= 3) {
      if (t + 1 < T) {                                   // pair (t, t+1)
        const float w = (t <= T - 3 ? 1.f : 0.f) + (t >= 1 ? 1.f : 0.f);
        const float a = st_sigmoid(r[e + cells]);
        tvt += w * st_cube(a - s);
        gt += w * st_dcube(a, s);
      }
      if (t >= 1) {                                      // pair (t-1, t)
        const float w = (t - 1 <= T - 3 ? 1.f : 0.f) + (t - 1 >= 1 ? 1.f : 0.f);
        gt += w * st_dcube(st_sigmoid(r[e - cells]), s);
      }
    }
    if (i + 1 < gh) {
      const float a = st_sigmoid(r[e + gw]);
      tvs += st_cube(a - s);
      gs += st_dcube(a, s);
    }
    if (i >= 1) gs += st_dcube(st_sigmoid(r[e - gw]), s);
    if (j + 1 < gw) {
      const float a = st_sigmoid(r[e + 1]);
      tvs += st_cube(a - s);
      gs += st_dcube(a, s);
    }
    if (j >= 1) gs += st_dcube(st_sigmoid(r[e - 1]), s);
    const float sg = (s > 0.f) - (s < 0.f);
    dreg[(size_t)b * n + e] = (lam1 * sg) / fc + (lam2 * gt) / fc + (lam3 * gs) / fc;
  }
  __shared__ float red[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float v[3] = {l1, tvt, tvs};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if (lane == 0) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    const float sum = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    const float lam = k == 0 ? lam1 : (k == 1 ? lam2 : lam3);
    terms[b * 3 + k] = (lam * sum) / fc;
  }
}

// Loop tail, one workgroup per clip: trajectory row (J, l1, tvt, tvs, score), then search_step_kernel's chain through
// the sigmoid and adam_kernel's arithmetic on the clip's T gh gw elements.
__global__ __launch_bounds__(256) void stmask_step_kernel(float* __restrict__ raw, const float* __restrict__ sig,
                                                          const float* __restrict__ dscore_dsig,
                                                          const float* __restrict__ dreg, const float* __restrict__ terms,
                                                          const float* __restrict__ score, float* __restrict__ am,
                                                          float* __restrict__ av, float* __restrict__ traj, int n,
                                                          float step_size, float inv_sqrt_bc2, float b1, float b2,
                                                          float eps) {
  const int b = blockIdx.x;
  if (threadIdx.x == 0 && traj) {
    const float l1 = terms[b * 3], tvt = terms[b * 3 + 1], tvs = terms[b * 3 + 2], sc = score[b];
    traj[b * 5 + 0] = l1 + tvt + tvs + sc;
    traj[b * 5 + 1] = l1;
    traj[b * 5 + 2] = tvt;
    traj[b * 5 + 3] = tvs;
    traj[b * 5 + 4] = sc;
  }
  for (int e = threadIdx.x; e < n; e += 256) {
    const size_t i = (size_t)b * n + e;
    float s = sig[i];
    float gs = dreg[i] + dscore_dsig[i];
    float gi = gs * (s * (1.f - s));
    float mi = am[i] * b1 + (1.f - b1) * gi;
    float vi = av[i] * b2 + (1.f - b2) * gi * gi;
    am[i] = mi;
    av[i] = vi;
    raw[i] = raw[i] - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
  }
}

// ---------------------------------------------------------------- one-box exhaustive search (maskType 'stcombi')
// The gradient-free counterpart of the spacetime search (as 'combi' is of 'central'): every candidate is one temporal
// blob [a, a+L) times one rectangle of grid cells, rows [i0, i0+bh) x columns [j0, j0+bw).  The three axes are three
// one-blob tables in the canonical order of ivf_blob_count; k = (kt n_h + kh) n_w + kw.
//
// Staging writes what ivf_stmask_expand_fwd + ivf_stfreeze_fwd write for the candidate's binary S, without S or M in
// memory.  With S in {0, 1} the expand's sums lose their zero terms exactly (x + 0 * a == x for the finite,
// non-negative values involved; 1 * a == a), so
//   rw[x]   = sum_{j in columns, ascending} A_W[x,j]
//   M[y,x]  = sum_{i in rows, ascending} A_H[y,i] * rw[x]      on the blob's frames, 0 on the others,
// every partial sum rounded as stmask_expand_fwd_kernel rounds it (this file is built without contraction: a multiply
// and an add each).  The recurrence is ivf_stfreeze_fwd's expression with that M; on a frame with M = 0 it returns X[u].
struct BoxAxes {
  int T, gh, gw, n_h, n_w, n;
};

struct Box {
  int clip, a, L, i0, bh, j0, bw;
};

__device__ __forceinline__ Box box_decode(long long g, const BoxAxes& ax) {
  Box c;
  c.clip = (int)(g / ax.n);
  const int k = (int)(g % ax.n);
  const int kw = k % ax.n_w, kh = (k / ax.n_w) % ax.n_h, kt = k / (ax.n_w * ax.n_h);
  blob_decode(kt, ax.T, &c.a, &c.L);
  blob_decode(kh, ax.gh, &c.i0, &c.bh);
  blob_decode(kw, ax.gw, &c.j0, &c.bw);
  return c;
}

// M[y,x] of the box on one of its frames; A_H row y and A_W row x are read through the cache (a workgroup shares its
// candidate, a wave mostly its row y)
__device__ __forceinline__ float box_mask_at(const float* __restrict__ AH, const float* __restrict__ AW, int gh, int gw,
                                             int y, int x, const Box& c) {
  float rw = 0.f;
  for (int j = c.j0; j < c.j0 + c.bw; ++j) rw += AW[(size_t)x * gw + j];
  float m = 0.f;
  for (int i = c.i0; i < c.i0 + c.bh; ++i) m += AH[(size_t)y * gh + i] * rw;
  return m;
}

// 16-byte channels-last pixels (C <= 4): one thread per pixel of row blockIdx.y, as freeze_fwd_cl4_kernel (mask_ops.hip).  With TT > 0
// (T == TT) the 16 frames of a piece are requested before the scan goes over them.
template <int TT>   // 0, or a multiple of 16
__global__ __launch_bounds__(256) void box_stage_cl4_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                            const float* __restrict__ AW, float* __restrict__ p, int C,
                                                            int W, int HW, BoxAxes ax, long long first) {
  const int px = blockIdx.x * 256 + threadIdx.x;
  if (px >= HW) return;
  const int row = blockIdx.y, T = TT > 0 ? TT : ax.T;
  const Box c = box_decode(first + row, ax);
  const float mb = box_mask_at(AH, AW, ax.gh, ax.gw, px / W, px % W, c);
  const float* xc = x + (size_t)c.clip * C * T * HW + px;
  float* pr = p + ((size_t)row * T * HW + px) * 4;
  float prev[4] = {0.f, 0.f, 0.f, 0.f};
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
        const int u = u0 + j;
        const float m = (u >= c.a && u < c.a + c.L) ? mb : 0.f;
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
      const float m = (u >= c.a && u < c.a + c.L) ? mb : 0.f;
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

// NCTHW: one thread per pixel of row blockIdx.y, channel after channel (the mask value is the pixel's, not the channel's)
__global__ __launch_bounds__(256) void box_stage_ncthw_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                              const float* __restrict__ AW, float* __restrict__ p, int C,
                                                              int W, int HW, BoxAxes ax, long long first) {
  const int px = blockIdx.x * 256 + threadIdx.x;
  if (px >= HW) return;
  const int row = blockIdx.y, T = ax.T;
  const Box c = box_decode(first + row, ax);
  const float mb = box_mask_at(AH, AW, ax.gh, ax.gw, px / W, px % W, c);
  for (int ch = 0; ch < C; ++ch) {
    const float* xp = x + ((size_t)(c.clip * C + ch) * T) * HW + px;
    float* pp = p + ((size_t)(row * C + ch) * T) * HW + px;
    float prev = 0.f;
    for (int u = 0; u < T; ++u) {
      const float m = (u >= c.a && u < c.a + c.L) ? mb : 0.f;
      float xv = xp[(size_t)u * HW];
      float v = u ? (1.f - m) * xv + m * prev : xv;
      prev = v;
      pp[(size_t)u * HW] = v;
    }
  }
}

// The regulariser of stmask_reg_kernel on the binary S of a box, in closed form (small integers, exact in fp32):
//   sum S = L bh bw;  TVt = bh bw (w(a-1) [a >= 1] + w(a+L-1) [a+L < T]), w the pair weights of stmask_reg_kernel
//   (interior pairs count twice; nothing at T < 3);  TVs = L (bw ([i0 >= 1] + [i0+bh < gh]) + bh ([j0 >= 1] + [j0+bw < gw])).
// J = l1 + tvt + tvs + score with each term (lam * sum) / cells: the expressions and the order of stmask_reg_kernel's
// terms and stmask_step_kernel's trajectory row.
__device__ __forceinline__ float box_objective(const Box& c, int T, int gh, int gw, float lam1, float lam2, float lam3,
                                               float score) {
  const float fc = (float)(gh * gw);
  const int vol = c.L * c.bh * c.bw;
  int wt = 0;
  if (T >= 3) {
    if (c.a >= 1) wt += (c.a - 1 <= T - 3 ? 1 : 0) + (c.a - 1 >= 1 ? 1 : 0);
    if (c.a + c.L < T) wt += (c.a + c.L - 1 <= T - 3 ? 1 : 0) + (c.a + c.L - 1 >= 1 ? 1 : 0);
  }
  const int tvt = c.bh * c.bw * wt;
  const int tvs = c.L * (c.bw * ((c.i0 >= 1) + (c.i0 + c.bh < gh)) + c.bh * ((c.j0 >= 1) + (c.j0 + c.bw < gw)));
  const float l1 = (lam1 * (float)vol) / fc, t = (lam2 * (float)tvt) / fc, sp = (lam3 * (float)tvs) / fc;
  return l1 + t + sp + score;
}

// Selection, one workgroup per clip: a thread walks k = tid, tid + 256, ... and keeps its own winners; thread 0 then
// goes over the 256 in order.  best = argmin J (NaN skipped, the smaller k on a tie); minimal = the smallest volume
// L bh bw with some r = (orig - s) / (orig - full) >= threshold, the largest r within it, then the smaller k.
__global__ __launch_bounds__(256) void box_select_kernel(const float* __restrict__ scores, const float* __restrict__ orig,
                                                         const float* __restrict__ full, BoxAxes ax, float lam1,
                                                         float lam2, float lam3, float threshold, int* __restrict__ best,
                                                         float* __restrict__ best_obj, float* __restrict__ obj,
                                                         int* __restrict__ minimal) {
  __shared__ float bj_s[256], mr_s[256];
  __shared__ int bk_s[256], mk_s[256], mv_s[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* s = scores + (size_t)b * ax.n;
  const float o = orig[b], den = o - full[b];
  int bk = -1, mk = -1, mv = 0;
  float bj = 0.f, mr = 0.f;
  for (int k = tid; k < ax.n; k += 256) {
    const Box c = box_decode(k, ax);
    const float J = box_objective(c, ax.T, ax.gh, ax.gw, lam1, lam2, lam3, s[k]);
    if (obj) obj[(size_t)b * ax.n + k] = J;
    if (J == J && (bk < 0 || J < bj)) { bk = k; bj = J; }
    const float r = (o - s[k]) / den;
    const int vol = c.L * c.bh * c.bw;
    if (r >= threshold && (mk < 0 || vol < mv || (vol == mv && r > mr))) { mk = k; mv = vol; mr = r; }
  }
  bj_s[tid] = bj; bk_s[tid] = bk; mr_s[tid] = mr; mk_s[tid] = mk; mv_s[tid] = mv;
  __syncthreads();
  if (tid != 0) return;
  for (int t = 1; t < 256; ++t) {
    const int k2 = bk_s[t];
    if (k2 >= 0 && (bk < 0 || bj_s[t] < bj || (bj_s[t] == bj && k2 < bk))) { bk = k2; bj = bj_s[t]; }
    const int m2 = mk_s[t];
    if (m2 >= 0 && (mk < 0 || mv_s[t] < mv || (mv_s[t] == mv && (mr_s[t] > mr || (mr_s[t] == mr && m2 < mk))))) {
      mk = m2; mv = mv_s[t]; mr = mr_s[t];
    }
  }
  for (int which = 0; which < 2; ++which) {
    int* dst = which ? minimal : best;
    const int k = which ? mk : bk;
    if (!dst) continue;
    if (k < 0) {
      for (int q = 0; q < 6; ++q) dst[b * 6 + q] = -1;
    } else {
      const Box c = box_decode(k, ax);
      dst[b * 6 + 0] = c.a; dst[b * 6 + 1] = c.L; dst[b * 6 + 2] = c.i0;
      dst[b * 6 + 3] = c.bh; dst[b * 6 + 4] = c.j0; dst[b * 6 + 5] = c.bw;
    }
  }
  if (best_obj) best_obj[b] = bk < 0 ? __builtin_nanf("") : bj;
}

// Occlusion map from the score grid: drop[b,t,i,j] = mean of (orig_b - s_k) over the candidates whose box covers the
// cell, in ascending k, NaN scores neither summed nor counted.  One thread per cell; it walks only the covering
// candidates: per axis the blobs of length l that contain the position start in [max(0, pos-l+1), min(pos, size-l)].
__device__ __forceinline__ int blob_base(int size, int l) { return (l - 1) * (size + 1) - (l - 1) * l / 2; }

__global__ __launch_bounds__(256) void box_drop_kernel(const float* __restrict__ scores, const float* __restrict__ orig,
                                                       int B, BoxAxes ax, int max_len, int mh, int mw,
                                                       float* __restrict__ drop) {
  const int cells = ax.gh * ax.gw;
  const size_t e = blockIdx.x * (size_t)256 + threadIdx.x;
  if (e >= (size_t)B * ax.T * cells) return;
  const int b = (int)(e / ((size_t)ax.T * cells));
  const int rem = (int)(e - (size_t)b * ax.T * cells);
  const int t = rem / cells, cell = rem - t * cells, i = cell / ax.gw, j = cell - i * ax.gw;
  const float* s = scores + (size_t)b * ax.n;
  const float o = orig[b];
  float sum = 0.f;
  int cnt = 0;
  for (int lt = 1; lt <= max_len; ++lt)
    for (int a = max(0, t - lt + 1); a <= min(t, ax.T - lt); ++a) {
      const int kt = blob_base(ax.T, lt) + a;
      for (int lh = 1; lh <= mh; ++lh)
        for (int i0 = max(0, i - lh + 1); i0 <= min(i, ax.gh - lh); ++i0) {
          const int kh = blob_base(ax.gh, lh) + i0;
          for (int lw = 1; lw <= mw; ++lw)
            for (int j0 = max(0, j - lw + 1); j0 <= min(j, ax.gw - lw); ++j0) {
              const int kw = blob_base(ax.gw, lw) + j0;
              const float v = s[((size_t)kt * ax.n_h + kh) * ax.n_w + kw];
              if (v == v) {
                sum += o - v;
                ++cnt;
              }
            }
        }
    }
  drop[e] = cnt ? sum / (float)cnt : __builtin_nanf("");
}

static bool st_grid_ok(int gh, int gw) { return gh >= 1 && gh <= ST_MAX_GRID && gw >= 1 && gw <= ST_MAX_GRID; }

// the axes of a checked candidate space (ivf_box_count >= 0)
static BoxAxes box_axes(int T, int max_len, int gh, int gw, int mh, int mw) {
  BoxAxes ax;
  ax.T = T; ax.gh = gh; ax.gw = gw;
  ax.n_h = ivf_blob_count(gh, mh);
  ax.n_w = ivf_blob_count(gw, mw);
  ax.n = ivf_blob_count(T, max_len) * ax.n_h * ax.n_w;
  return ax;
}

}  // namespace ivf

using namespace ivf;

extern "C" int ivf_stmask_axis_weights(int n_out, int n_in, float sigma, float* A_host) {
  IVF_CHECK_ARG(A_host, "stmask_axis_weights: null pointer");
  IVF_CHECK_ARG(n_out > 0 && n_in > 0, "stmask_axis_weights: bad sizes (%d from %d)", n_out, n_in);
  IVF_CHECK_ARG(sigma >= 0.f && sigma < 1e6f, "stmask_axis_weights: sigma must be finite and >= 0");
  // U [n_out, n_in]: bilinear, half-pixel centres, clamped edges (F.interpolate(align_corners=False))
  std::vector<double> Um((size_t)n_out * n_in, 0.0);
  const double scale = (double)n_in / (double)n_out;
  for (int y = 0; y < n_out; ++y) {
    double src = scale * (y + 0.5) - 0.5;
    if (src < 0.0) src = 0.0;
    int i0 = (int)std::floor(src);
    if (i0 > n_in - 1) i0 = n_in - 1;
    const int i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
    const double l1 = src - i0, l0 = 1.0 - l1;
    Um[(size_t)y * n_in + i0] += l0;
    Um[(size_t)y * n_in + i1] += l1;
  }
  // G: radius ceil(3 sigma), taps normalised to sum 1, replicated border
  const int rad = sigma > 0.f ? (int)std::ceil(3.0 * (double)sigma) : 0;
  std::vector<double> tap(2 * (size_t)rad + 1, 1.0);
  if (rad > 0) {
    double sum = 0.0;
    for (int d = -rad; d <= rad; ++d) {
      tap[d + rad] = std::exp(-0.5 * (double)d * d / ((double)sigma * sigma));
      sum += tap[d + rad];
    }
    for (double& t : tap) t /= sum;
  }
  std::vector<double> row(n_in);
  for (int y = 0; y < n_out; ++y) {
    for (int j = 0; j < n_in; ++j) row[j] = 0.0;
    for (int d = -rad; d <= rad; ++d) {
      int k = y + d;
      k = k < 0 ? 0 : (k > n_out - 1 ? n_out - 1 : k);
      for (int j = 0; j < n_in; ++j) row[j] += tap[d + rad] * Um[(size_t)k * n_in + j];
    }
    for (int j = 0; j < n_in; ++j) A_host[(size_t)y * n_in + j] = (float)row[j];
  }
  return IVF_OK;
}

extern "C" int ivf_stmask_expand_fwd(const float* S, const float* A_H, const float* A_W, float* M, int B, int T, int gh,
                                     int gw, int H, int W, ivf_stream_t stream) {
  IVF_CHECK_ARG(S && A_H && A_W && M, "stmask_expand_fwd: null pointer");
  IVF_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0, "stmask_expand_fwd: bad dims");
  IVF_CHECK_ARG(st_grid_ok(gh, gw), "stmask_expand_fwd: grid %dx%d outside 1..%d", gh, gw, ST_MAX_GRID);
  IVF_CHECK_ARG((long long)B * T <= 0x7fffffffLL && cdiv(H, EX_ROWS) <= 65535, "stmask_expand_fwd: too many frames or rows");
  const int vec_ok = (W % 4 == 0) && (((uintptr_t)M & 15) == 0);
  hipLaunchKernelGGL(stmask_expand_fwd_kernel, dim3(B * T, cdiv(H, EX_ROWS)), dim3(256), 0, (hipStream_t)stream, S, A_H,
                     A_W, M, gh, gw, H, W, vec_ok);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_stmask_expand_bwd(const float* dM, const float* A_H, const float* A_W, float* dS, int B, int T, int gh,
                                     int gw, int H, int W, ivf_stream_t stream) {
  IVF_CHECK_ARG(dM && A_H && A_W && dS, "stmask_expand_bwd: null pointer");
  IVF_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0, "stmask_expand_bwd: bad dims");
  IVF_CHECK_ARG(st_grid_ok(gh, gw), "stmask_expand_bwd: grid %dx%d outside 1..%d", gh, gw, ST_MAX_GRID);
  IVF_CHECK_ARG((long long)B * T <= 0x7fffffffLL, "stmask_expand_bwd: too many frames");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(B * T), block(256);
  if (gh <= 8)
    hipLaunchKernelGGL(stmask_expand_bwd_kernel<8>, grid, block, 0, s, dM, A_H, A_W, dS, gh, gw, H, W);
  else if (gh <= 16)
    hipLaunchKernelGGL(stmask_expand_bwd_kernel<16>, grid, block, 0, s, dM, A_H, A_W, dS, gh, gw, H, W);
  else
    hipLaunchKernelGGL(stmask_expand_bwd_kernel<32>, grid, block, 0, s, dM, A_H, A_W, dS, gh, gw, H, W);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_stfreeze_fwd(const float* x, const float* M, float* p, int B, int C, int T, int HW, int out_cpad,
                                ivf_stream_t stream) {
  IVF_CHECK_ARG(x && M && p, "stfreeze_fwd: null pointer");
  IVF_CHECK_ARG(B > 0 && C > 0 && T > 0 && HW > 0, "stfreeze_fwd: bad dims");
  IVF_CHECK_ARG(out_cpad == 0 || out_cpad >= C, "stfreeze_fwd: out_cpad (%d) < C (%d)", out_cpad, C);
  // the freeze scan of mask_ops.hip with the mask value of the pixel: a spatially constant M gives ivf_freeze_fwd's bits
  return freeze_fwd(x, M, true, p, B, C, T, HW, 1, out_cpad, (hipStream_t)stream);
}

template <int TT>
static void stfreeze_bwd_launch(const float* x, const float* M, const float* g, float* dM, int B, int C, int T, int HW,
                                int g_cpad, hipStream_t s) {
  const dim3 grid(grid_for((size_t)B * HW, 256, 4096)), block(256);
  if (g_cpad == 0) {
    hipLaunchKernelGGL((stfreeze_bwd_kernel<TT, 0>), grid, block, 0, s, x, M, g, dM, B, C, T, HW, g_cpad);
    return;
  }
  if constexpr (TT <= 32) {     // 64 frames of 16-byte rows spill to scratch outright: T > 32 reads lane by lane (see the kernel)
    if (g_cpad == 4) {
      hipLaunchKernelGGL((stfreeze_bwd_kernel<TT, 2>), grid, block, 0, s, x, M, g, dM, B, C, T, HW, g_cpad);
      return;
    }
  }
  hipLaunchKernelGGL((stfreeze_bwd_kernel<TT, 1>), grid, block, 0, s, x, M, g, dM, B, C, T, HW, g_cpad);
}

extern "C" int ivf_stfreeze_bwd(const float* x, const float* M, const float* g, float* dM, int B, int C, int T, int HW,
                                int g_cpad, ivf_stream_t stream) {
  IVF_CHECK_ARG(x && M && g && dM, "stfreeze_bwd: null pointer");
  IVF_CHECK_ARG(B > 0 && C > 0 && T > 0 && T <= MAX_T && HW > 0, "stfreeze_bwd: bad dims (T <= %d)", MAX_T);
  IVF_CHECK_ARG(g_cpad == 0 || g_cpad >= C, "stfreeze_bwd: g_cpad (%d) < C (%d)", g_cpad, C);
  with_frames_upto(T, [&](auto TT) { stfreeze_bwd_launch<TT>(x, M, g, dM, B, C, T, HW, g_cpad, (hipStream_t)stream); });
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_stmask_reg(const float* raw, int B, int T, int gh, int gw, float lam1, float lam2, float lam3,
                              float* sig, float* terms, float* dreg_dsig, ivf_stream_t stream) {
  IVF_CHECK_ARG(raw && sig && terms && dreg_dsig, "stmask_reg: null pointer");
  IVF_CHECK_ARG(B > 0 && T > 0 && T <= MAX_T, "stmask_reg: bad dims (T <= %d)", MAX_T);
  IVF_CHECK_ARG(st_grid_ok(gh, gw), "stmask_reg: grid %dx%d outside 1..%d", gh, gw, ST_MAX_GRID);
  hipLaunchKernelGGL(stmask_reg_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, raw, T, gh, gw, lam1, lam2, lam3, sig,
                     terms, dreg_dsig);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_stmask_step(float* raw, const float* sig, const float* dscore_dsig, const float* dreg_dsig,
                               const float* terms, const float* score, float* exp_avg, float* exp_avg_sq,
                               float* traj_row, int B, int T, int gh, int gw, int step, float lr, float beta1,
                               float beta2, float eps, ivf_stream_t stream) {
  IVF_CHECK_ARG(raw && sig && dscore_dsig && dreg_dsig && terms && score && exp_avg && exp_avg_sq,
                "stmask_step: null pointer");
  IVF_CHECK_ARG(B > 0 && T > 0 && T <= MAX_T && step >= 1, "stmask_step: bad dims (T <= %d)", MAX_T);
  IVF_CHECK_ARG(st_grid_ok(gh, gw), "stmask_step: grid %dx%d outside 1..%d", gh, gw, ST_MAX_GRID);
  float ss, isb;
  adam_coeffs(step, lr, beta1, beta2, &ss, &isb);
  hipLaunchKernelGGL(stmask_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, raw, sig, dscore_dsig, dreg_dsig,
                     terms, score, exp_avg, exp_avg_sq, traj_row, T * gh * gw, ss, isb, beta1, beta2, eps);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

// Caller-owned scratch of the spacetime search loop (search_driver.h, StScratch): M, dM [B,T,H,W]; sig, dreg, dsig
// [B,T,gh,gw]; terms [B,3]; score [B]; every piece 256-byte aligned.  0 (message set) for arguments the loop refuses.
extern "C" size_t ivf_stsearch_workspace_bytes(int B, int T, int H, int W, int gh, int gw) {
  if (B <= 0 || T <= 0 || T > MAX_T || H <= 0 || W <= 0 || !st_grid_ok(gh, gw)) {
    set_error("stsearch_workspace_bytes: bad dims (T <= %d, grid 1..%d)", MAX_T, ST_MAX_GRID);
    return 0;
  }
  StScratch sc;
  return sc.carve((size_t)B, (size_t)T, (size_t)H * W, (size_t)gh * gw);
}

// ---------------------------------------------------------------- one-box search: C-ABI
extern "C" long long ivf_box_count(int T, int max_len, int gh, int gw, int mh, int mw) {
  if (T < 1 || T > MAX_T || max_len < 1 || max_len > T || !st_grid_ok(gh, gw) || mh < 1 || mh > gh || mw < 1 ||
      mw > gw) {
    set_error("box_count: need 1 <= max_len (%d) <= T (%d) <= %d, 1 <= mh (%d) <= gh (%d) <= %d, 1 <= mw (%d) <= gw (%d) <= %d",
              max_len, T, MAX_T, mh, gh, ST_MAX_GRID, mw, gw, ST_MAX_GRID);
    return -1;
  }
  return (long long)ivf_blob_count(T, max_len) * ivf_blob_count(gh, mh) * ivf_blob_count(gw, mw);   // < 2^31 at the limits
}

extern "C" int ivf_box_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gh,
                             int gw, int max_len, int mh, int mw, long long first, int count, float* p, int out_cpad,
                             ivf_stream_t stream) {
  IVF_CHECK_ARG(x && A_H && A_W && p, "box_stage: null pointer");
  IVF_CHECK_ARG(b > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "box_stage: bad dims");
  const long long n = ivf_box_count(T, max_len, gh, gw, mh, mw);
  if (n < 0) return IVF_ERR_BAD_ARG;
  IVF_CHECK_ARG(first >= 0 && count > 0 && count <= 65535 && first + count <= (long long)b * n,
                "box_stage: rows [%lld, %lld) outside the %lld candidates of %d clips (at most 65535 rows a call)", first,
                first + count, (long long)b * n, b);
  IVF_CHECK_ARG(out_cpad == 0 || (out_cpad == 4 && C <= 4),
                "box_stage: out_cpad must be 0 (NCTHW) or 4 (16-byte channels-last, C <= 4)");
  const BoxAxes ax = box_axes(T, max_len, gh, gw, mh, mw);
  const int HW = H * W;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(HW, 256), count), block(256);
  if (out_cpad == 0)
    hipLaunchKernelGGL(box_stage_ncthw_kernel, grid, block, 0, s, x, A_H, A_W, p, C, W, HW, ax, first);
  else
    with_frames_exact(T, [&](auto TT) {
      hipLaunchKernelGGL(box_stage_cl4_kernel<TT>, grid, block, 0, s, x, A_H, A_W, p, C, W, HW, ax, first);
    });
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_box_select(const float* scores, const float* orig, const float* full, int b, int T, int gh, int gw,
                              int max_len, int mh, int mw, float lam1, float lam2, float lam3, float threshold, int* best,
                              float* best_obj, float* obj, int* minimal, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && orig && full && best, "box_select: null pointer");
  IVF_CHECK_ARG(b > 0, "box_select: bad batch %d", b);
  if (ivf_box_count(T, max_len, gh, gw, mh, mw) < 0) return IVF_ERR_BAD_ARG;
  hipLaunchKernelGGL(box_select_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, scores, orig, full,
                     box_axes(T, max_len, gh, gw, mh, mw), lam1, lam2, lam3, threshold, best, best_obj, obj, minimal);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_box_drop(const float* scores, const float* orig, int b, int T, int gh, int gw, int max_len, int mh,
                            int mw, float* drop, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && orig && drop, "box_drop: null pointer");
  IVF_CHECK_ARG(b > 0, "box_drop: bad batch %d", b);
  if (ivf_box_count(T, max_len, gh, gw, mh, mw) < 0) return IVF_ERR_BAD_ARG;
  const long long cells = (long long)b * T * gh * gw;
  IVF_CHECK_ARG(cdiv(cells, 256) <= 0x7fffffffLL, "box_drop: too many cells");
  hipLaunchKernelGGL(box_drop_kernel, dim3(cdiv(cells, 256)), dim3(256), 0, (hipStream_t)stream, scores, orig, b,
                     box_axes(T, max_len, gh, gw, mh, mw), max_len, mh, mw, drop);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
