// Depthwise convolution (tf.nn.depthwise_conv2d) for gfx950: forward, data gradient, weight gradient.
//
//   x  NHWC [N,H,W,C] (bf16 or fp32), filter w fp32 [R,S,C,M] (TF layout, M = channel multiplier),
//   y  [N,P,Q,C*M]; output channel c*M+m reads input channel c:
//     y[n,p,q,c*M+m]  = sum_{r,s} x[n, p*sh-ph+r*dh, q*sw-pw+s*dw, c] * w[r,s,c,m]
//     dx[n,h,w,c]     = sum_{r,s,m} dy[n,p,q,c*M+m] * w[r,s,c,m]   over the (p,q) with p*sh-ph+r*dh == h,
//                                                                    q*sw-pw+s*dw == w
//     dw[r,s,c,m]     = sum_{n,p,q} x[n, p*sh-ph+r*dh, q*sw-pw+s*dw, c] * dy[n,p,q,c*M+m]
//   A tap whose input coordinate falls outside the image contributes zero. ph, pw, P, Q are all
//   given, so TF's asymmetric SAME needs no padded copy of x. Accumulation is fp32; bf16 results
//   are rounded once (RNE, f2bf / pack8); fp32 inputs compute and stay in fp32.
//
// Two forms behind every entry point (dwconv_plan.h holds the admission rule):
//
// * Fast (bf16, M == 1, C % 8 == 0, 3x3, stride 1 or 2, no dilation, 16-byte aligned bases). A lane
//   owns 8 consecutive channels for the whole launch, so its 9 x 8 filter taps stay in registers
//   as fp32 and every global access is one 16-byte load or store. A work item is a strip of
//   kStrip = 4 consecutive output columns of one output row (data gradient: 4 input columns of
//   one input row): the vectors loaded for one filter row are reused across the strip in
//   registers. Vertical reuse (a row of x is read by up to three output rows) is left to L2: no
//   LDS halo. Work items are ordered strip-fastest, then row, then image; lanes are ordered
//   channel-group-fastest, so a wave reads contiguous runs of a row. The forward and the data
//   gradient issue the loads of all three filter rows of a strip before any arithmetic: a vector
//   outside the image is loaded from the index clamped into it and replaced by zeros, so no load
//   waits behind a branch (2.3x faster at the 14x14 layers than row-by-row loads under range
//   tests). The grid is two blocks per CU; a thread walks several strips with its taps loaded once.
//   The weight gradient keeps its 9 x 8 fp32 accumulators in registers over its slab of output
//   rows; the threads of a block that share a channel group are then summed through LDS in
//   thread order, tap by tap, and the block writes its part of the slab's partial row.
// * Generic (everything else: any C, any M, fp32 or bf16, R, S <= 7, any stride / dilation,
//   unaligned bases): scalar accesses, one thread per output element. The data gradient is a
//   gather with a divisibility and range test per tap.
//
// No atomics anywhere. dx is fully written (no zero fill). The weight gradient splits the N*P
// output rows into T slabs (dwconv_plan.h), each writing one fp32 partial row into the caller's
// workspace; ttdk_colreduce (transformer.hip) folds the rows in a fixed order, so the result is
// bitwise the same on every run. Element offsets are long long. Grids are capped (2048 blocks;
// 512 for the fast forward / data gradient) and grid-strided; the (column, row, image) indices advance by host-computed increments (an add
// and a conditional subtract per level), so the loops hold no division except the generic data
// gradient's per-tap divisibility test.
//
// dt: 0 = fp32, 1 = bf16 (the codes of nn_generic.hip). form: 0 = by the plan, 1 = generic.
//
// Compiler resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
// scratch is 0 for every kernel here; VGPRs and occupancy per kernel are in profiles/dwconv_bench.txt.
#include "common.h"
#include "dwconv_plan.h"

// transformer.hip
extern "C" int ttdk_colreduce(const float* part, int nb, int C, int stride, float* out, int beta, hipStream_t st);

namespace ttdk {
namespace {

namespace dwplan = ::ttdk::dwplan;

constexpr int kDwBlock = 256;
constexpr int kDwMaxBlocks = 256 * 8;
constexpr int kDwFastBlocks = 256 * 2;
constexpr int kStrip = dwplan::kStrip;

// A mixed-radix counter (i[0] fastest, below dim[0]; ...; top unbounded) and the digits of one
// grid stride: advancing is an add and a conditional subtract per level.
template <int L>
struct Walk {
  int dim[L];
  int d[L];
  long long dtop;
};

template <int L>
Walk<L> make_walk(long long stride, const int (&dims)[L]) {
  Walk<L> w;
  for (int l = 0; l < L; ++l) {
    w.dim[l] = dims[l];
    w.d[l] = static_cast<int>(stride % dims[l]);
    stride /= dims[l];
  }
  w.dtop = stride;
  return w;
}

template <int L>
__device__ __forceinline__ void walk_init(long long idx, const Walk<L>& w, int (&i)[L], long long& top) {
#pragma unroll
  for (int l = 0; l < L; ++l) {
    i[l] = static_cast<int>(idx % w.dim[l]);
    idx /= w.dim[l];
  }
  top = idx;
}

template <int L>
__device__ __forceinline__ void walk_step(const Walk<L>& w, int (&i)[L], long long& top) {
  int carry = 0;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    i[l] += w.d[l] + carry;  // < 2 * dim[l]
    carry = i[l] >= w.dim[l];
    if (carry) i[l] -= w.dim[l];
  }
  top += w.dtop + carry;
}

__device__ __forceinline__ uint4 ldg16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }

// Vector `i` of a row of `n` vectors C elements apart, zero outside [0, n) or when !ok. The load
// itself is unconditional, from the index clamped into the row, so the loads of a work item do
// not wait for one another behind branches.
__device__ __forceinline__ uint4 ldg16_or_zero(const bf16_t* row, int i, int n, int C, bool ok) {
  const int ic = i < 0 ? 0 : (i >= n ? n - 1 : i);
  const uint4 v = ldg16(row + static_cast<long long>(ic) * C);
  return (ok && i == ic) ? v : make_uint4(0, 0, 0, 0);
}
__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

__device__ __forceinline__ void load_taps(const float* __restrict__ w, int C, int cg, float (&wt)[9][8]) {
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const float* p = w + static_cast<long long>(t) * C + cg * 8;
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    wt[t][0] = a.x, wt[t][1] = a.y, wt[t][2] = a.z, wt[t][3] = a.w;
    wt[t][4] = b.x, wt[t][5] = b.y, wt[t][6] = b.z, wt[t][7] = b.w;
  }
}

// ------------------------------------------------------------------ fast forward
// Thread gid: channel group gid % CG (fixed), slot gid / CG of tpc; items (strip, p, n) slot, slot + tpc, ...
template <int ST>
__global__ __launch_bounds__(kDwBlock) void dw_fwd_fast(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                        bf16_t* __restrict__ y, TtdkDwConv g, int CG, long long tpc,
                                                        Walk<2> wk) {
  constexpr int NV = (kStrip - 1) * ST + 3;  // input columns under one strip
  const long long gid = static_cast<long long>(blockIdx.x) * kDwBlock + threadIdx.x;
  const int cg = static_cast<int>(gid % CG);
  const long long slot = gid / CG;
  if (slot >= tpc) return;
  float wt[9][8];
  load_taps(w, g.C, cg, wt);
  int i2[2];  // strip, p
  long long n;
  walk_init(slot, wk, i2, n);
  while (n < g.N) {
    const int q0 = i2[0] * kStrip, p = i2[1];
    const int w0 = q0 * ST - g.pw, h0 = p * ST - g.ph;
    const int nq = g.Q - q0 < kStrip ? g.Q - q0 : kStrip;  // >= 1
    const int nv = (nq - 1) * ST + 3;
    float acc[kStrip][8];
#pragma unroll
    for (int i = 0; i < kStrip; ++i)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[i][k] = 0.f;
    uint4 v[3][NV];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int h = h0 + r;
      const bf16_t* row = x + ((n * g.H + clampi(h, g.H)) * g.W) * g.C + cg * 8;
#pragma unroll
      for (int j = 0; j < NV; ++j) v[r][j] = ldg16_or_zero(row, w0 + j, g.W, g.C, h >= 0 && h < g.H && j < nv);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        float f[8];
        unpack8(v[r][j], f);
#pragma unroll
        for (int i = 0; i < kStrip; ++i) {
          const int s = j - i * ST;
          if (s >= 0 && s < 3) {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[i][k] += f[k] * wt[r * 3 + s][k];
          }
        }
      }
    }
    bf16_t* out = y + ((n * g.P + p) * g.Q + q0) * g.C + cg * 8;
#pragma unroll
    for (int i = 0; i < kStrip; ++i)
      if (i < nq) *reinterpret_cast<uint4*>(out + static_cast<long long>(i) * g.C) = pack8(acc[i]);
    walk_step(wk, i2, n);
  }
}

// ------------------------------------------------------------------ fast data gradient
// Items (strip of 4 input columns, h, n). Stride 1: dy columns w + pw - s, six under a strip.
// Stride 2: only even w + pw - s has a q; the strip starts at a multiple of 4, so the parity of
// the first candidate is that of pw (PAR) and the tap of (column i, vector j) is a constant.
template <int ST, int PAR>
__global__ __launch_bounds__(kDwBlock) void dw_dgrad_fast(const bf16_t* __restrict__ dy, const float* __restrict__ w,
                                                          bf16_t* __restrict__ dx, TtdkDwConv g, int CG, long long tpc,
                                                          Walk<2> wk) {
  constexpr int NQ = ST == 1 ? kStrip + 2 : 3;
  const long long gid = static_cast<long long>(blockIdx.x) * kDwBlock + threadIdx.x;
  const int cg = static_cast<int>(gid % CG);
  const long long slot = gid / CG;
  if (slot >= tpc) return;
  float wt[9][8];
  load_taps(w, g.C, cg, wt);
  int i2[2];  // strip, h
  long long n;
  walk_init(slot, wk, i2, n);
  while (n < g.N) {
    const int w0 = i2[0] * kStrip, h = i2[1];
    const int nw = g.W - w0 < kStrip ? g.W - w0 : kStrip;
    const int e0 = w0 + g.pw - 2 + PAR;
    const int qlo = ST == 2 ? e0 >> 1 : e0;  // e0 is even when ST == 2 (arithmetic shift: floor)
    float acc[kStrip][8];
#pragma unroll
    for (int i = 0; i < kStrip; ++i)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[i][k] = 0.f;
    uint4 v[3][NQ];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int t = h + g.ph - r;
      const int p = ST == 2 ? t >> 1 : t;
      const bool ok = !(ST == 2 && (t & 1)) && p >= 0 && p < g.P;
      const bf16_t* row = dy + ((n * g.P + clampi(p, g.P)) * g.Q) * g.C + cg * 8;
#pragma unroll
      for (int j = 0; j < NQ; ++j) v[r][j] = ldg16_or_zero(row, qlo + j, g.Q, g.C, ok);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        float f[8];
        unpack8(v[r][j], f);
#pragma unroll
        for (int i = 0; i < kStrip; ++i) {
          const int s = i + 2 - PAR - ST * j;
          if (s >= 0 && s < 3) {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[i][k] += f[k] * wt[r * 3 + s][k];
          }
        }
      }
    }
    bf16_t* out = dx + ((n * g.H + h) * g.W + w0) * g.C + cg * 8;
#pragma unroll
    for (int i = 0; i < kStrip; ++i)
      if (i < nw) *reinterpret_cast<uint4*>(out + static_cast<long long>(i) * g.C) = pack8(acc[i]);
    walk_step(wk, i2, n);
  }
}

// ------------------------------------------------------------------ fast weight gradient
// Block (channel-group chunk, slab): thread tid owns channel group chunk * LC + tid % LC and the
// items (strip, output row) tid / LC, tid / LC + TL, ... of the slab's rows [r0, r1).
template <int ST>
__global__ __launch_bounds__(kDwBlock) void dw_wgrad_fast(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                          float* __restrict__ part, TtdkDwConv g, int CG, int LC, int TL,
                                                          long long rows_per, long long pstride, Walk<2> wk) {
  constexpr int NV = (kStrip - 1) * ST + 3;
  __shared__ float red[kDwBlock * 8];
  const int tid = threadIdx.x;
  const int cgl = tid % LC, tl = tid / LC;
  const int cg = blockIdx.x * LC + cgl;
  const long long rows = static_cast<long long>(g.N) * g.P;
  const long long r0 = blockIdx.y * rows_per;
  const long long r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
  const int QS = wk.dim[0];
  const long long nitems = (r1 - r0) * QS;
  float acc[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[t][k] = 0.f;
  if (tl < TL && cg < CG && tl < nitems) {
    int i2[2];  // strip, p
    long long n;
    walk_init(r0 * QS + tl, wk, i2, n);
    for (long long left = (nitems - tl + TL - 1) / TL; left > 0; --left) {
      const int q0 = i2[0] * kStrip, p = i2[1];
      const int w0 = q0 * ST - g.pw, h0 = p * ST - g.ph;
      const int nq = g.Q - q0 < kStrip ? g.Q - q0 : kStrip;
      const int nv = (nq - 1) * ST + 3;
      const bf16_t* drow = dy + ((n * g.P + p) * g.Q + q0) * g.C + cg * 8;
      float d[kStrip][8];
#pragma unroll
      for (int i = 0; i < kStrip; ++i)
        unpack8(i < nq ? ldg16(drow + static_cast<long long>(i) * g.C) : make_uint4(0, 0, 0, 0), d[i]);
      // One filter row at a time, behind its range test. Loading the three rows together, as the
      // forward does, costs a wave per SIMD here (72 accumulators are live) and measured 25 %
      // slower at the stride-1 layers.
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int h = h0 + r;
        if (h < 0 || h >= g.H) continue;
        const bf16_t* row = x + ((n * g.H + h) * g.W) * g.C + cg * 8;
        uint4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int wj = w0 + j;
          v[j] = (j < nv && wj >= 0 && wj < g.W) ? ldg16(row + static_cast<long long>(wj) * g.C)
                                                 : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          float f[8];
          unpack8(v[j], f);
#pragma unroll
          for (int i = 0; i < kStrip; ++i) {
            const int s = j - i * ST;
            if (s >= 0 && s < 3) {
#pragma unroll
              for (int k = 0; k < 8; ++k) acc[r * 3 + s][k] += f[k] * d[i][k];
            }
          }
        }
      }
      walk_step(wk, i2, n);
    }
  }
  // sum the TL threads of every channel group in thread order, one tap per round
  float* prow = part + blockIdx.y * pstride;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) red[tid * 8 + k] = acc[t][k];
    __syncthreads();
    if (tid < LC * 8) {
      const int c = tid >> 3, k = tid & 7;
      float s = 0.f;
      for (int u = 0; u < TL; ++u) s += red[(u * LC + c) * 8 + k];
      const int ocg = blockIdx.x * LC + c;
      if (ocg < CG) prow[static_cast<long long>(t) * g.C + ocg * 8 + k] = s;
    }
  }
}

// ------------------------------------------------------------------ generic form
template <typename T>
__device__ __forceinline__ float ldf(const T* p);
template <>
__device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ void stf(float* p, float v) { *p = v; }
__device__ __forceinline__ void stf(bf16_t* p, float v) { *p = f2bf(v); }

// One thread per output element (m, c, q, p | n).
template <typename T>
__global__ __launch_bounds__(kDwBlock) void dw_fwd_generic(const T* __restrict__ x, const float* __restrict__ w,
                                                           T* __restrict__ y, TtdkDwConv g, Walk<4> wk) {
  int i4[4];
  long long n;
  walk_init(static_cast<long long>(blockIdx.x) * kDwBlock + threadIdx.x, wk, i4, n);
  const long long CO = static_cast<long long>(g.C) * g.M;
  while (n < g.N) {
    const int m = i4[0], c = i4[1], q = i4[2], p = i4[3];
    const float* wp = w + static_cast<long long>(c) * g.M + m;
    float acc = 0.f;
    int h = p * g.sh - g.ph;
    for (int r = 0; r < g.R; ++r, h += g.dh) {
      if (h < 0 || h >= g.H) continue;
      const T* row = x + ((n * g.H + h) * g.W) * g.C + c;
      int wc = q * g.sw - g.pw;
      for (int s = 0; s < g.S; ++s, wc += g.dw)
        if (wc >= 0 && wc < g.W) acc += ldf(row + static_cast<long long>(wc) * g.C) * wp[(r * g.S + s) * CO];
    }
    stf(y + ((n * g.P + p) * g.Q + q) * CO + static_cast<long long>(c) * g.M + m, acc);
    walk_step(wk, i4, n);
  }
}

// One thread per dx element (c, w, h | n): gather over the taps.
template <typename T>
__global__ __launch_bounds__(kDwBlock) void dw_dgrad_generic(const T* __restrict__ dy, const float* __restrict__ w,
                                                             T* __restrict__ dx, TtdkDwConv g, Walk<3> wk) {
  int i3[3];
  long long n;
  walk_init(static_cast<long long>(blockIdx.x) * kDwBlock + threadIdx.x, wk, i3, n);
  const long long CO = static_cast<long long>(g.C) * g.M;
  while (n < g.N) {
    const int c = i3[0], wc = i3[1], h = i3[2];
    const float* wp = w + static_cast<long long>(c) * g.M;
    float acc = 0.f;
    for (int r = 0; r < g.R; ++r) {
      const int th = h + g.ph - r * g.dh;
      if (th < 0 || th % g.sh) continue;
      const int p = th / g.sh;
      if (p >= g.P) continue;
      const T* row = dy + ((n * g.P + p) * g.Q) * CO + static_cast<long long>(c) * g.M;
      for (int s = 0; s < g.S; ++s) {
        const int tw = wc + g.pw - s * g.dw;
        if (tw < 0 || tw % g.sw) continue;
        const int q = tw / g.sw;
        if (q >= g.Q) continue;
        const T* dp = row + q * CO;
        const float* wt = wp + (r * g.S + s) * CO;
        for (int m = 0; m < g.M; ++m) acc += ldf(dp + m) * wt[m];
      }
    }
    stf(dx + ((n * g.H + h) * g.W + wc) * g.C + c, acc);
    walk_step(wk, i3, n);
  }
}

// Block (256 filter elements, slab): thread e = (r, s, c, m) sums its slab's rows in order.
// Elements [RSCM, pstride) of the partial row are written as zeros.
template <typename T>
__global__ __launch_bounds__(kDwBlock) void dw_wgrad_generic(const T* __restrict__ x, const T* __restrict__ dy,
                                                             float* __restrict__ part, TtdkDwConv g, long long rows_per,
                                                             long long pstride) {
  const long long e = static_cast<long long>(blockIdx.x) * kDwBlock + threadIdx.x;
  if (e >= pstride) return;
  float* out = part + blockIdx.y * pstride + e;
  const long long CO = static_cast<long long>(g.C) * g.M;
  if (e >= CO * g.R * g.S) {
    *out = 0.f;
    return;
  }
  const int co = static_cast<int>(e % CO), tap = static_cast<int>(e / CO);
  const int c = co / g.M, s = tap % g.S, r = tap / g.S;
  const long long rows = static_cast<long long>(g.N) * g.P;
  const long long r0 = blockIdx.y * rows_per;
  const long long r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
  int p = static_cast<int>(r0 % g.P);
  long long n = r0 / g.P;
  const int wbase = s * g.dw - g.pw;
  float acc = 0.f;
  for (long long row = r0; row < r1; ++row) {
    const int h = p * g.sh - g.ph + r * g.dh;
    if (h >= 0 && h < g.H) {
      const T* xr = x + ((n * g.H + h) * g.W) * g.C + c;
      const T* dr = dy + ((n * g.P + p) * g.Q) * CO + co;
      int wc = wbase;
      for (int q = 0; q < g.Q; ++q, wc += g.sw)
        if (wc >= 0 && wc < g.W) acc += ldf(xr + static_cast<long long>(wc) * g.C) * ldf(dr + q * CO);
    }
    if (++p == g.P) p = 0, ++n;
  }
  *out = acc;
}

// dw (+)= tmp, for a filter gradient the column reduce cannot write in 16-byte vectors.
__global__ __launch_bounds__(kDwBlock) void dw_finish(const float* __restrict__ tmp, float* __restrict__ dw,
                                                      long long n, int beta) {
  for (long long i = static_cast<long long>(blockIdx.x) * kDwBlock + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * kDwBlock)
    dw[i] = beta ? dw[i] + tmp[i] : tmp[i];
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline unsigned capped_blocks(long long threads) {
  long long b = (threads + kDwBlock - 1) / kDwBlock;
  return static_cast<unsigned>(b > kDwMaxBlocks ? kDwMaxBlocks : b);
}

// Grid cap of the fast forward / data gradient: two 256-thread blocks per CU, what the kernels'
// 2 waves per SIMD hold at once, so a thread loads its taps once and walks several strips. Against
// 1024 and 2048 blocks this measured up to 16 % faster at the 14x14 and 7x7 layers and within 4 %
// elsewhere (TTD_DW_FAST_BLOCKS: A/B, at most kDwMaxBlocks).
inline int fast_max_blocks() {
  static const int cap = [] {
    const char* e = getenv("TTD_DW_FAST_BLOCKS");
    const int v = e ? atoi(e) : kDwFastBlocks;
    return v > 0 && v < kDwMaxBlocks ? v : kDwFastBlocks;
  }();
  return cap;
}

// Threads of a fast forward / data-gradient launch over `items` strips per channel group: blocks
// and the slots per channel group (every thread keeps its channel group for the whole launch).
inline unsigned fast_grid(long long items, int CG, long long* tpc) {
  unsigned blocks = capped_blocks(items * CG);
  if (blocks > static_cast<unsigned>(fast_max_blocks())) blocks = fast_max_blocks();
  const unsigned least = static_cast<unsigned>((CG + kDwBlock - 1) / kDwBlock);
  if (blocks < least) blocks = least;
  *tpc = static_cast<long long>(blocks) * kDwBlock / CG;
  return blocks;
}

template <typename T>
int generic_fwd(const void* x, const float* w, void* y, const TtdkDwConv& g, hipStream_t st) {
  const long long total = static_cast<long long>(g.N) * g.P * g.Q * g.C * g.M;
  const unsigned blocks = capped_blocks(total);
  const int dims[4] = {g.M, g.C, g.Q, g.P};
  hipLaunchKernelGGL(dw_fwd_generic<T>, dim3(blocks), dim3(kDwBlock), 0, st, static_cast<const T*>(x), w,
                     static_cast<T*>(y), g, make_walk<4>(static_cast<long long>(blocks) * kDwBlock, dims));
  return hipGetLastError();
}

template <typename T>
int generic_dgrad(const void* dy, const float* w, void* dx, const TtdkDwConv& g, hipStream_t st) {
  const long long total = static_cast<long long>(g.N) * g.H * g.W * g.C;
  const unsigned blocks = capped_blocks(total);
  const int dims[3] = {g.C, g.W, g.H};
  hipLaunchKernelGGL(dw_dgrad_generic<T>, dim3(blocks), dim3(kDwBlock), 0, st, static_cast<const T*>(dy), w,
                     static_cast<T*>(dx), g, make_walk<3>(static_cast<long long>(blocks) * kDwBlock, dims));
  return hipGetLastError();
}

template <typename T>
void generic_wgrad(const void* x, const void* dy, float* part, const TtdkDwConv& g, int T_, hipStream_t st) {
  const long long ps = dwplan::part_stride(g);
  hipLaunchKernelGGL(dw_wgrad_generic<T>, dim3(static_cast<unsigned>((ps + kDwBlock - 1) / kDwBlock), T_),
                     dim3(kDwBlock), 0, st, static_cast<const T*>(x), static_cast<const T*>(dy), part, g,
                     dwplan::rows_per_slab(g), ps);
}

}  // namespace
}  // namespace ttdk

using namespace ttdk;

// Slabs T of the weight gradient and its workspace in floats ((T + 1) padded partial rows).
TTDK_API(int, ttdk_dwconv_wgrad_parts, (const TtdkDwConv* g)) { return dwplan::valid(*g) ? dwplan::wgrad_parts(*g) : 0; }
TTDK_API(long long, ttdk_dwconv_wgrad_ws_floats, (const TtdkDwConv* g)) {
  return dwplan::valid(*g) ? dwplan::wgrad_ws_floats(*g) : 0;
}

// y [N,P,Q,C*M] = dwconv(x [N,H,W,C], w fp32 [R,S,C,M]); x, y of type dt.
TTDK_API(int, ttdk_dwconv_fwd, (const void* x, const float* w, void* y, int dt, const TtdkDwConv* gp, int form,
                                hipStream_t st)) {
  const TtdkDwConv g = *gp;
  if (!dwplan::valid(g) || !x || !w || !y || (dt != 0 && dt != 1)) return hipErrorInvalidValue;
  if (form == 0 && dwplan::fast_takes(g, dt) && aligned16(x) && aligned16(w) && aligned16(y)) {
    const int CG = g.C / 8, QS = (g.Q + kStrip - 1) / kStrip;
    long long tpc;
    const unsigned blocks = fast_grid(static_cast<long long>(g.N) * g.P * QS, CG, &tpc);
    const int dims[2] = {QS, g.P};
    const Walk<2> wk = make_walk<2>(tpc, dims);
    const bf16_t* xb = static_cast<const bf16_t*>(x);
    bf16_t* yb = static_cast<bf16_t*>(y);
    if (g.sh == 1)
      hipLaunchKernelGGL(dw_fwd_fast<1>, dim3(blocks), dim3(kDwBlock), 0, st, xb, w, yb, g, CG, tpc, wk);
    else
      hipLaunchKernelGGL(dw_fwd_fast<2>, dim3(blocks), dim3(kDwBlock), 0, st, xb, w, yb, g, CG, tpc, wk);
    return hipGetLastError();
  }
  return dt == 0 ? generic_fwd<float>(x, w, y, g, st) : generic_fwd<bf16_t>(x, w, y, g, st);
}

// dx [N,H,W,C] from dy [N,P,Q,C*M]; every element of dx is written.
TTDK_API(int, ttdk_dwconv_dgrad, (const void* dy, const float* w, void* dx, int dt, const TtdkDwConv* gp, int form,
                                  hipStream_t st)) {
  const TtdkDwConv g = *gp;
  if (!dwplan::valid(g) || !dy || !w || !dx || (dt != 0 && dt != 1)) return hipErrorInvalidValue;
  if (form == 0 && dwplan::fast_takes(g, dt) && aligned16(dy) && aligned16(w) && aligned16(dx)) {
    const int CG = g.C / 8, WS = (g.W + kStrip - 1) / kStrip;
    long long tpc;
    const unsigned blocks = fast_grid(static_cast<long long>(g.N) * g.H * WS, CG, &tpc);
    const int dims[2] = {WS, g.H};
    const Walk<2> wk = make_walk<2>(tpc, dims);
    const bf16_t* db = static_cast<const bf16_t*>(dy);
    bf16_t* xb = static_cast<bf16_t*>(dx);
    if (g.sh == 1)
      hipLaunchKernelGGL((dw_dgrad_fast<1, 0>), dim3(blocks), dim3(kDwBlock), 0, st, db, w, xb, g, CG, tpc, wk);
    else if (g.pw & 1)
      hipLaunchKernelGGL((dw_dgrad_fast<2, 1>), dim3(blocks), dim3(kDwBlock), 0, st, db, w, xb, g, CG, tpc, wk);
    else
      hipLaunchKernelGGL((dw_dgrad_fast<2, 0>), dim3(blocks), dim3(kDwBlock), 0, st, db, w, xb, g, CG, tpc, wk);
    return hipGetLastError();
  }
  return dt == 0 ? generic_dgrad<float>(dy, w, dx, g, st) : generic_dgrad<bf16_t>(dy, w, dx, g, st);
}

// dw fp32 [R,S,C,M] = (beta ? dw : 0) + the weight gradient of x [N,H,W,C], dy [N,P,Q,C*M] (type
// dt). ws: 16-byte aligned fp32 workspace of at least ttdk_dwconv_wgrad_ws_floats(g) floats.
TTDK_API(int, ttdk_dwconv_wgrad, (const void* x, const void* dy, float* dw, float* ws, long long ws_floats, int dt,
                                  const TtdkDwConv* gp, int beta, int form, hipStream_t st)) {
  const TtdkDwConv g = *gp;
  if (!dwplan::valid(g) || !x || !dy || !dw || !ws || (dt != 0 && dt != 1)) return hipErrorInvalidValue;
  if (!aligned16(ws) || ws_floats < dwplan::wgrad_ws_floats(g)) return hipErrorInvalidValue;
  const int T = dwplan::wgrad_parts(g);
  const long long ps = dwplan::part_stride(g), fe = dwplan::filter_elems(g);
  if (form == 0 && dwplan::fast_takes(g, dt) && aligned16(x) && aligned16(dy)) {
    const int CG = g.C / 8, QS = (g.Q + kStrip - 1) / kStrip;
    const int chunks = (CG + 31) / 32, LC = (CG + chunks - 1) / chunks, TL = kDwBlock / LC;
    const int dims[2] = {QS, g.P};
    const Walk<2> wk = make_walk<2>(TL, dims);
    const bf16_t* xb = static_cast<const bf16_t*>(x);
    const bf16_t* db = static_cast<const bf16_t*>(dy);
    const dim3 grid((CG + LC - 1) / LC, T);
    if (g.sh == 1)
      hipLaunchKernelGGL(dw_wgrad_fast<1>, grid, dim3(kDwBlock), 0, st, xb, db, ws, g, CG, LC, TL,
                         dwplan::rows_per_slab(g), ps, wk);
    else
      hipLaunchKernelGGL(dw_wgrad_fast<2>, grid, dim3(kDwBlock), 0, st, xb, db, ws, g, CG, LC, TL,
                         dwplan::rows_per_slab(g), ps, wk);
  } else if (dt == 0) {
    generic_wgrad<float>(x, dy, ws, g, T, st);
  } else {
    generic_wgrad<bf16_t>(x, dy, ws, g, T, st);
  }
  int rc = hipGetLastError();
  if (rc) return rc;
  if (fe == ps && aligned16(dw)) return ttdk_colreduce(ws, T, static_cast<int>(fe), static_cast<int>(ps), dw, beta, st);
  float* tmp = ws + static_cast<long long>(T) * ps;
  rc = ttdk_colreduce(ws, T, static_cast<int>(ps), static_cast<int>(ps), tmp, 0, st);
  if (rc) return rc;
  hipLaunchKernelGGL(dw_finish, dim3(capped_blocks(fe)), dim3(kDwBlock), 0, st, tmp, dw, fe, beta);
  return hipGetLastError();
}
