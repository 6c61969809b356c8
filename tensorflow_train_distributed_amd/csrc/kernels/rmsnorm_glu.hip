// RMSNorm and SwiGLU: the norm and the feed-forward gate of a LLaMA-style block, for gfx950.
//
// RMSNorm (fast path, bf16, H in {512, 1024, 1536, 2048, 4096}) has the residual / dropout frame of
// the LayerNorm in transformer.hip with one statistic instead of two:
//   s = res + drop_in(x)   (rounded to bf16 before the statistic: backward re-reads that value)
//   rstd = rsqrt(mean_j(s_j^2) + eps);   y = drop_out(s * rstd * gamma)
// backward, n = s * rstd, g = drop_out'(dy) * gamma:
//   ds = rstd * (g - n * mean_j(g_j n_j));  dx = ds * mask_in * scale_in;  dgamma = sum_rows drop_out'(dy) * n
// One wave per row, the row in registers, 16-byte loads and stores, one HBM pass each way. dgamma is
// per-workgroup partial rows [nb][H] folded over the waves in a fixed order plus the column reduce of
// transformer.hip (ttdk_colreduce): no float atomics, bitwise reproducible. The dropout hash index is
// row * H + column, as in LayerNorm.
//
// RMSNorm (generic, any width, fp32 or bf16, no dropout / residual) serves ttd.nn: wave per row,
// scalar accesses, dgamma through column partials summed in a fixed order.
//
// SwiGLU: x2 [rows, 2I] = [gate a | value b], h = a * sigmoid(a) * b; backward with s = sigmoid(a):
//   da = dh * b * s * (1 + a * (1 - s)),  db = dh * a * s,  written as [da | db].
// Every operand has its own row stride (the engine's [tokens, intermediate] buffers are row-padded
// column views). 16-byte accesses when I, the strides and the pointers allow, one element per work
// item otherwise. The grid is capped and grid-strided; the vector form advances (row, chunk) by
// host-computed increments, so its loop holds no integer division. The backward may write over its
// own input (dx2 == x2 with equal strides): a work item reads its (a, b) before it writes (da, db)
// and work items own disjoint elements. No LDS, no atomics.
//
// dt: 0 = fp32, 1 = bf16 (the codes of nn_generic.hip).
//
// Compiler resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage;
// full table in profiles/rmsnorm_swiglu_bench.txt): scratch is 0 for every kernel here. The fast
// backward keeps LayerNorm's waves-per-block choice per width: it holds one accumulator row
// (dgamma) where LayerNorm holds two and needs one wave reduction per row where LayerNorm needs
// two, so every instantiation sits at or under the VGPR count of its LayerNorm twin and none is
// pushed to fewer waves per SIMD. H = 1024 runs 8 waves x 1 row with the next row prefetched.
#include "tile_common.h"

// transformer.hip
extern "C" int ttdk_colreduce(const float* part, int nb, int C, int stride, float* out, int beta, hipStream_t st);
extern "C" int ttdk_ln_bwd_num_blocks(int rows);

namespace ttdk {
namespace {

__device__ __forceinline__ uint4 ldg16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }

// (re-declared from transformer.hip, whose copy lives in that file's anonymous namespace)
struct DropSpec {
  const long long* rng;
  uint32_t site_in, site_out;
  uint32_t thr_in, thr_out;
  float scale_in, scale_out;
};

DropSpec make_drop(const long long* rng, unsigned site_in, float p_in, unsigned site_out, float p_out) {
  DropSpec d;
  d.rng = rng;
  d.site_in = site_in;
  d.site_out = site_out;
  d.thr_in = drop_threshold(p_in);
  d.thr_out = drop_threshold(p_out);
  d.scale_in = p_in > 0.f ? 1.f / (1.f - p_in) : 1.f;
  d.scale_out = p_out > 0.f ? 1.f / (1.f - p_out) : 1.f;
  return d;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ void load_f8(const float* __restrict__ p, float (&f)[8]) {
  *reinterpret_cast<f32x4_t*>(f) = *reinterpret_cast<const f32x4_t*>(p);
  *reinterpret_cast<f32x4_t*>(f + 4) = *reinterpret_cast<const f32x4_t*>(p + 4);
}

// ------------------------------------------------------------------ RMSNorm forward (fast)
// H = NV * 512; wave w of a 256-thread block owns row blockIdx.x * 4 + w; lane holds 16-B chunks
// lane + 64 * v.
template <int NV>
__global__ __launch_bounds__(256) void rms_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ res,
                                                      bf16_t* __restrict__ s_out, bf16_t* __restrict__ y,
                                                      float* __restrict__ rstd_out, const float* __restrict__ gamma,
                                                      int rows, float eps, DropSpec dsp) {
  constexpr int H = NV * 512;
  const int lane = threadIdx.x & 63;
  const long long row = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint32_t kin = dsp.thr_in ? drop_key(dsp.rng, dsp.site_in) : 0u;
  const uint32_t kout = dsp.thr_out ? drop_key(dsp.rng, dsp.site_out) : 0u;
  float f[NV][8];
  float ss = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = (lane + 64 * v) * 8;
    unpack8(ldg16(x + row * H + c), f[v]);
    if (dsp.thr_in) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        f[v][j] = drop_keep(kin, static_cast<unsigned long long>(row) * H + c + j, dsp.thr_in) ? f[v][j] * dsp.scale_in
                                                                                                  : 0.f;
    }
    if (res) {
      float r[8];
      unpack8(ldg16(res + row * H + c), r);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[v][j] += r[j];
    }
    // the statistic of the bf16 value that backward will re-read
    const uint4 pk = pack8(f[v]);
    unpack8(pk, f[v]);
    if (s_out) *reinterpret_cast<uint4*>(s_out + row * H + c) = pk;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += f[v][j] * f[v][j];
  }
  const float rstd = rsqrtf(wave_sum(ss) * (1.f / H) + eps);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = (lane + 64 * v) * 8;
    float o[8], gw[8];
    load_f8(gamma + c, gw);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o[j] = f[v][j] * rstd * gw[j];
      if (dsp.thr_out)
        o[j] = drop_keep(kout, static_cast<unsigned long long>(row) * H + c + j, dsp.thr_out) ? o[j] * dsp.scale_out
                                                                                               : 0.f;
    }
    *reinterpret_cast<uint4*>(y + row * H + c) = pack8(o);
  }
  if (lane == 0) rstd_out[row] = rstd;
}

// ------------------------------------------------------------------ RMSNorm backward (fast)
// ds_out = dL/ds (the residual branch), dx_out = ds * mask_in * scale_in (null: not wanted).
// part: [gridDim.x][H] partial dgamma rows. W waves per block, each wave one row at a time; PF loads
// the next row one iteration ahead so that a load is in flight while the wave reduces and stores.
template <int NV, int W, bool PF>
__global__ __launch_bounds__(W * 64) void rms_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ s,
                                                         const float* __restrict__ rstd_in,
                                                         const float* __restrict__ gamma, bf16_t* __restrict__ ds_out,
                                                         bf16_t* __restrict__ dx_out, float* __restrict__ part,
                                                         int rows, int rows_per_block, DropSpec dsp) {
  constexpr int H = NV * 512, CH = 512;  // a wave's columns for one v: lane * 8 + j
  __shared__ __attribute__((aligned(16))) float red[W][CH];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t kin = dsp.thr_in ? drop_key(dsp.rng, dsp.site_in) : 0u;
  const uint32_t kout = dsp.thr_out ? drop_key(dsp.rng, dsp.site_out) : 0u;
  float dg[NV][8];
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int j = 0; j < 8; ++j) dg[v][j] = 0.f;
  const long long r0 = static_cast<long long>(blockIdx.x) * rows_per_block;
  const long long r1 = min(static_cast<long long>(rows), r0 + rows_per_block);
  // dy after the output dropout (recomputed in both passes; the mask is a hash, not stored)
  auto load_d = [&](const uint4& pk, long long row, int c, float (&d)[8]) {
    unpack8(pk, d);
    if (dsp.thr_out) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        d[j] = drop_keep(kout, static_cast<unsigned long long>(row) * H + c + j, dsp.thr_out) ? d[j] * dsp.scale_out : 0.f;
    }
  };
  uint4 nd[NV], ns[NV];
  float nrstd = 0.f;
  auto fetch = [&](long long r) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = (lane + 64 * v) * 8;
      nd[v] = ldg16(dy + r * H + c);
      ns[v] = ldg16(s + r * H + c);
    }
    nrstd = rstd_in[r];
  };
  if (PF && r0 + w < r1) fetch(r0 + w);
#pragma unroll 1
  for (long long row = r0 + w; row < r1; row += W) {
    if constexpr (!PF) fetch(row);
    uint4 pd[NV], ps[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      pd[v] = nd[v];
      ps[v] = ns[v];
    }
    const float rstd = nrstd;
    if constexpr (PF) {
      if (row + W < r1) fetch(row + W);
    }
    float c2 = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = (lane + 64 * v) * 8;
      float d[8], sv[8], gm[8];
      load_d(pd[v], row, c, d);
      unpack8(ps[v], sv);
      load_f8(gamma + c, gm);  // re-read (L1/L2-resident) where used rather than held in 8*NV VGPRs
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float n = sv[j] * rstd;
        dg[v][j] += d[j] * n;
        c2 += d[j] * gm[j] * n;
      }
    }
    // opaque to the optimiser: pass 2 re-derives d / n from the packed rows instead of keeping
    // pass 1's unpacked floats alive across the reduction
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      asm volatile("" : "+v"(pd[v].x), "+v"(pd[v].y), "+v"(pd[v].z), "+v"(pd[v].w));
      asm volatile("" : "+v"(ps[v].x), "+v"(ps[v].y), "+v"(ps[v].z), "+v"(ps[v].w));
    }
    const float m2 = wave_sum(c2) * (1.f / H);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = (lane + 64 * v) * 8;
      float d[8], sv[8], o[8], gm[8];
      load_d(pd[v], row, c, d);
      unpack8(ps[v], sv);
      load_f8(gamma + c, gm);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = rstd * (d[j] * gm[j] - sv[j] * rstd * m2);
      *reinterpret_cast<uint4*>(ds_out + row * H + c) = pack8(o);
      if (dx_out) {
        if (dsp.thr_in) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            o[j] = drop_keep(kin, static_cast<unsigned long long>(row) * H + c + j, dsp.thr_in) ? o[j] * dsp.scale_in : 0.f;
        }
        *reinterpret_cast<uint4*>(dx_out + row * H + c) = pack8(o);
      }
    }
  }
  // block reduce of dg over the W waves in fixed order, one 512-column slice (v) at a time
  float* out = part + static_cast<long long>(blockIdx.x) * H;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    __syncthreads();
    *reinterpret_cast<f32x4_t*>(&red[w][lane * 8]) = *reinterpret_cast<const f32x4_t*>(dg[v]);
    *reinterpret_cast<f32x4_t*>(&red[w][lane * 8 + 4]) = *reinterpret_cast<const f32x4_t*>(dg[v] + 4);
    __syncthreads();
    for (int col = threadIdx.x; col < CH; col += W * 64) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < W; ++k) t += red[k][col];
      out[v * CH + col] = t;
    }
  }
}

// ------------------------------------------------------------------ RMSNorm (any width)
template <typename T>
__device__ __forceinline__ float ldf(const T* p, long long i);
template <>
__device__ __forceinline__ float ldf<float>(const float* p, long long i) { return p[i]; }
template <>
__device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p, long long i) { return bf2f(p[i]); }

template <typename T>
__device__ __forceinline__ void stf(T* p, long long i, float v);
template <>
__device__ __forceinline__ void stf<float>(float* p, long long i, float v) { p[i] = v; }
template <>
__device__ __forceinline__ void stf<bf16_t>(bf16_t* p, long long i, float v) { p[i] = f2bf(v); }

// one wave per row, 4 rows per block
template <typename T>
__global__ __launch_bounds__(256) void rms_generic_fwd_kernel(const T* __restrict__ x, const float* __restrict__ g,
                                                              T* __restrict__ y, float* __restrict__ rstd,
                                                              long long rows, int H, float eps) {
  const long long row = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const T* xr = x + row * H;
  float ss = 0.f;
  for (int j = lane; j < H; j += 64) {
    const float v = ldf(xr, j);
    ss += v * v;
  }
  const float r = rsqrtf(wave_sum(ss) / H + eps);
  for (int j = lane; j < H; j += 64) stf(y + row * H, j, ldf(xr, j) * r * g[j]);
  if (lane == 0) rstd[row] = r;
}

// dx = rstd * (dy*g - n * mean(dy*g*n)),  n = x * rstd
template <typename T>
__global__ __launch_bounds__(256) void rms_generic_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                 const float* __restrict__ g,
                                                                 const float* __restrict__ rstd, T* __restrict__ dx,
                                                                 long long rows, int H) {
  const long long row = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float r = rstd[row];
  const T* dr = dy + row * H;
  const T* xr = x + row * H;
  float c2 = 0.f;
  for (int j = lane; j < H; j += 64) c2 += ldf(dr, j) * g[j] * ldf(xr, j) * r;
  c2 = wave_sum(c2) / H;
  for (int j = lane; j < H; j += 64) stf(dx + row * H, j, r * (ldf(dr, j) * g[j] - ldf(xr, j) * r * c2));
}

// part[t][c] = sum over rows [t*rpb, (t+1)*rpb) of dy * x * rstd. Block = 64 columns x 4 row groups,
// grid (ceil(H / 64), T); the four row groups are added in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void rms_generic_dgamma_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                 const float* __restrict__ rstd, long long rows, int H,
                                                                 long long rpb, float* __restrict__ part) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const long long r0 = static_cast<long long>(blockIdx.y) * rpb;
  const long long r1 = min(rows, r0 + rpb);
  float acc = 0.f;
  if (c < H)
    for (long long r = r0 + rg; r < r1; r += 4) acc += ldf(dy, r * H + c) * ldf(x, r * H + c) * rstd[r];
  red[rg][cl] = acc;
  __syncthreads();
  if (rg == 0 && c < H) part[static_cast<long long>(blockIdx.y) * H + c] = red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl];
}

__global__ void rms_generic_reduce_kernel(const float* __restrict__ part, int T, int H, float* __restrict__ out,
                                          int acc) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= H) return;
  float t = 0.f;
  for (int b = 0; b < T; ++b) t += part[static_cast<long long>(b) * H + c];
  out[c] = acc ? out[c] + t : t;
}

// ------------------------------------------------------------------ SwiGLU
constexpr int kGluBlock = 256;
// 256 CUs x 8 blocks of 256 threads. At 65536 x 4096 bf16 the forward streams 5.16 TB/s at this cap
// and 5.8 TB/s with a grid that covers every work item; two work items in flight per thread, a
// next-trip prefetch with counted waits and a block-contiguous walk all measured the same as this
// plain loop at this cap (profiles/rmsnorm_swiglu_bench.txt), so the plain loop stayed.
constexpr int kGluMaxBlocks = 256 * 8;

template <typename T>
struct GluVec;

// bf16 results carry 8 mantissa bits: the hardware exp2 / rcp approximations (1 ulp of fp32) are far
// inside the rounding
template <>
struct GluVec<bf16_t> {
  static constexpr int E = 8;  // elements per 16 bytes
  static __device__ __forceinline__ void load(const bf16_t* p, float (&f)[8]) {
    unpack8(*reinterpret_cast<const uint4*>(p), f);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&f)[8]) {
    *reinterpret_cast<uint4*>(p) = pack8(f);
  }
  static __device__ __forceinline__ float ld1(const bf16_t* p) { return bf2f(*p); }
  static __device__ __forceinline__ void st1(bf16_t* p, float v) { *p = f2bf(v); }
  static __device__ __forceinline__ float sigmoid(float a) { return __builtin_amdgcn_rcpf(1.f + __expf(-a)); }
};

// fp32 results are held to 1e-5: the accurate expf and an IEEE division
template <>
struct GluVec<float> {
  static constexpr int E = 4;
  static __device__ __forceinline__ void load(const float* p, float (&f)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    f[0] = v.x, f[1] = v.y, f[2] = v.z, f[3] = v.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&f)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  }
  static __device__ __forceinline__ float ld1(const float* p) { return *p; }
  static __device__ __forceinline__ void st1(float* p, float v) { *p = v; }
  static __device__ __forceinline__ float sigmoid(float a) { return 1.f / (1.f + expf(-a)); }
};

// exp(-a) overflows to +inf for a < -88: sigmoid is then 1 / inf = 0 and every product below is a
// signed zero, not a NaN (a itself is finite).
template <typename T>
__device__ __forceinline__ float glu_fwd1(float a, float b) {
  return a * GluVec<T>::sigmoid(a) * b;
}

template <typename T>
__device__ __forceinline__ void glu_bwd1(float dh, float a, float b, float& da, float& db) {
  const float sg = GluVec<T>::sigmoid(a);
  da = dh * b * sg * (1.f + a * (1.f - sg));
  db = dh * a * sg;
}

// One stride of gridDim.x * 256 work items of the vector form is drow rows and drem chunks further.
struct GluStep {
  int per_row;  // I / E chunks per row
  int drow, drem;
};

template <typename T>
__global__ __launch_bounds__(kGluBlock) void swiglu_fwd_vec_kernel(const T* __restrict__ x2, long long ldx,
                                                                   T* __restrict__ h, long long ldh, long long rows,
                                                                   int I, GluStep st) {
  constexpr int E = GluVec<T>::E;
  const unsigned i0 = blockIdx.x * kGluBlock + threadIdx.x;  // < 2048 * 256
  long long r = i0 / static_cast<unsigned>(st.per_row);
  int j = static_cast<int>(i0 % static_cast<unsigned>(st.per_row));
  while (r < rows) {
    const T* xp = x2 + r * ldx + static_cast<long long>(j) * E;
    float a[E], b[E], o[E];
    GluVec<T>::load(xp, a);
    GluVec<T>::load(xp + I, b);
#pragma unroll
    for (int k = 0; k < E; ++k) o[k] = glu_fwd1<T>(a[k], b[k]);
    GluVec<T>::store(h + r * ldh + static_cast<long long>(j) * E, o);
    j += st.drem;
    r += st.drow;
    if (j >= st.per_row) {
      j -= st.per_row;
      ++r;
    }
  }
}

// x2 and dx2 may be the same buffer: no __restrict__ on them.
template <typename T>
__global__ __launch_bounds__(kGluBlock) void swiglu_bwd_vec_kernel(const T* __restrict__ dh, long long ldh, const T* x2,
                                                                   long long ldx, T* dx2, long long ldd,
                                                                   long long rows, int I, GluStep st) {
  constexpr int E = GluVec<T>::E;
  const unsigned i0 = blockIdx.x * kGluBlock + threadIdx.x;
  long long r = i0 / static_cast<unsigned>(st.per_row);
  int j = static_cast<int>(i0 % static_cast<unsigned>(st.per_row));
  while (r < rows) {
    const long long c = static_cast<long long>(j) * E;
    const T* xp = x2 + r * ldx + c;
    float d[E], a[E], b[E], da[E], db[E];
    GluVec<T>::load(dh + r * ldh + c, d);
    GluVec<T>::load(xp, a);
    GluVec<T>::load(xp + I, b);
#pragma unroll
    for (int k = 0; k < E; ++k) glu_bwd1<T>(d[k], a[k], b[k], da[k], db[k]);
    T* op = dx2 + r * ldd + c;
    GluVec<T>::store(op, da);
    GluVec<T>::store(op + I, db);
    j += st.drem;
    r += st.drow;
    if (j >= st.per_row) {
      j -= st.per_row;
      ++r;
    }
  }
}

// scalar form: one element per work item (any I, any element-aligned stride)
template <typename T>
__global__ __launch_bounds__(kGluBlock) void swiglu_fwd_scalar_kernel(const T* __restrict__ x2, long long ldx,
                                                                      T* __restrict__ h, long long ldh, long long rows,
                                                                      int I) {
  const long long n = rows * I, stride = static_cast<long long>(gridDim.x) * kGluBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kGluBlock + threadIdx.x; i < n; i += stride) {
    const long long r = i / I;
    const int c = static_cast<int>(i - r * I);
    const T* xp = x2 + r * ldx + c;
    GluVec<T>::st1(h + r * ldh + c, glu_fwd1<T>(GluVec<T>::ld1(xp), GluVec<T>::ld1(xp + I)));
  }
}

template <typename T>
__global__ __launch_bounds__(kGluBlock) void swiglu_bwd_scalar_kernel(const T* __restrict__ dh, long long ldh,
                                                                      const T* x2, long long ldx, T* dx2, long long ldd,
                                                                      long long rows, int I) {
  const long long n = rows * I, stride = static_cast<long long>(gridDim.x) * kGluBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kGluBlock + threadIdx.x; i < n; i += stride) {
    const long long r = i / I;
    const int c = static_cast<int>(i - r * I);
    const T* xp = x2 + r * ldx + c;
    const float a = GluVec<T>::ld1(xp), b = GluVec<T>::ld1(xp + I);
    float da, db;
    glu_bwd1<T>(GluVec<T>::ld1(dh + r * ldh + c), a, b, da, db);
    T* op = dx2 + r * ldd + c;
    GluVec<T>::st1(op, da);
    GluVec<T>::st1(op + I, db);
  }
}

inline unsigned glu_blocks(long long items) {
  long long b = (items + kGluBlock - 1) / kGluBlock;
  return static_cast<unsigned>(b > kGluMaxBlocks ? kGluMaxBlocks : b);
}

inline GluStep glu_step(int per_row, unsigned blocks) {
  GluStep s;
  const int stride = static_cast<int>(blocks) * kGluBlock;
  s.per_row = per_row;
  s.drow = stride / per_row;
  s.drem = stride % per_row;
  return s;
}

template <typename T>
int swiglu_fwd_launch(const void* x2, long long ldx, void* h, long long ldh, long long rows, int I, bool vec,
                      hipStream_t st) {
  constexpr int E = GluVec<T>::E;
  if (vec) {
    const unsigned nb = glu_blocks(rows * (I / E));
    hipLaunchKernelGGL(swiglu_fwd_vec_kernel<T>, dim3(nb), dim3(kGluBlock), 0, st, static_cast<const T*>(x2), ldx,
                       static_cast<T*>(h), ldh, rows, I, glu_step(I / E, nb));
  } else {
    hipLaunchKernelGGL(swiglu_fwd_scalar_kernel<T>, dim3(glu_blocks(rows * I)), dim3(kGluBlock), 0, st,
                       static_cast<const T*>(x2), ldx, static_cast<T*>(h), ldh, rows, I);
  }
  return hipGetLastError();
}

template <typename T>
int swiglu_bwd_launch(const void* dh, long long ldh, const void* x2, long long ldx, void* dx2, long long ldd,
                      long long rows, int I, bool vec, hipStream_t st) {
  constexpr int E = GluVec<T>::E;
  if (vec) {
    const unsigned nb = glu_blocks(rows * (I / E));
    hipLaunchKernelGGL(swiglu_bwd_vec_kernel<T>, dim3(nb), dim3(kGluBlock), 0, st, static_cast<const T*>(dh), ldh,
                       static_cast<const T*>(x2), ldx, static_cast<T*>(dx2), ldd, rows, I, glu_step(I / E, nb));
  } else {
    hipLaunchKernelGGL(swiglu_bwd_scalar_kernel<T>, dim3(glu_blocks(rows * I)), dim3(kGluBlock), 0, st,
                       static_cast<const T*>(dh), ldh, static_cast<const T*>(x2), ldx, static_cast<T*>(dx2), ldd, rows,
                       I);
  }
  return hipGetLastError();
}

}  // namespace
}  // namespace ttdk

using namespace ttdk;

#define TTDK_RMS_DISPATCH(KER, ...)                                \
  switch (H) {                                                     \
    case 512: hipLaunchKernelGGL(KER<1>, __VA_ARGS__); break;      \
    case 1024: hipLaunchKernelGGL(KER<2>, __VA_ARGS__); break;     \
    case 1536: hipLaunchKernelGGL(KER<3>, __VA_ARGS__); break;     \
    case 2048: hipLaunchKernelGGL(KER<4>, __VA_ARGS__); break;     \
    case 4096: hipLaunchKernelGGL(KER<8>, __VA_ARGS__); break;     \
    default: return hipErrorInvalidValue;                          \
  }

// Waves per block by width: LayerNorm's choice (see the head of this file).
#define TTDK_RMS_BWD_DISPATCH(...)                                                                                  \
  switch (H) {                                                                                                      \
    case 512: hipLaunchKernelGGL((rms_bwd_kernel<1, 16, false>), dim3(nb), dim3(16 * 64), __VA_ARGS__); break;      \
    case 1024: hipLaunchKernelGGL((rms_bwd_kernel<2, 8, true>), dim3(nb), dim3(8 * 64), __VA_ARGS__); break;        \
    case 1536: hipLaunchKernelGGL((rms_bwd_kernel<3, 8, false>), dim3(nb), dim3(8 * 64), __VA_ARGS__); break;       \
    case 2048: hipLaunchKernelGGL((rms_bwd_kernel<4, 4, false>), dim3(nb), dim3(4 * 64), __VA_ARGS__); break;       \
    case 4096: hipLaunchKernelGGL((rms_bwd_kernel<8, 4, false>), dim3(nb), dim3(4 * 64), __VA_ARGS__); break;       \
    default: return hipErrorInvalidValue;                                                                           \
  }

static bool rms_width_ok(int H) { return H == 512 || H == 1024 || H == 1536 || H == 2048 || H == 4096; }

// x, res (nullable), s_out (nullable), y: bf16 [rows, H] dense, 16-byte aligned; rstd fp32 [rows];
// gamma fp32 [H], 16-byte aligned. Bad arguments return hipErrorInvalidValue without a launch.
TTDK_API(int, ttdk_rms_fwd, (const bf16_t* x, const bf16_t* res, bf16_t* s_out, bf16_t* y, float* rstd,
                             const float* gamma, int rows, int H, float eps, float p_in, unsigned site_in, float p_out,
                             unsigned site_out, const long long* rng, hipStream_t st)) {
  if (!rms_width_ok(H) || rows < 0 || !x || !y || !rstd || !gamma) return hipErrorInvalidValue;
  if (!aligned16(x) || !aligned16(res) || !aligned16(s_out) || !aligned16(y) || !aligned16(gamma))
    return hipErrorInvalidValue;
  if ((p_in > 0.f || p_out > 0.f) && !rng) return hipErrorInvalidValue;
  if (rows == 0) return 0;
  DropSpec d = make_drop(rng, site_in, p_in, site_out, p_out);
  dim3 grid((rows + 3) / 4), block(256);
  TTDK_RMS_DISPATCH(rms_fwd_kernel, grid, block, 0, st, x, res, s_out, y, rstd, gamma, rows, eps, d);
  return hipGetLastError();
}

// Blocks of rms_bwd_kernel (= partial rows of the workspace): LayerNorm's count.
TTDK_API(int, ttdk_rms_bwd_num_blocks, (int rows)) { return ttdk_ln_bwd_num_blocks(rows); }

// part: fp32 [ttdk_rms_bwd_num_blocks(rows)][H] workspace; dgamma written (accumulate = 0) or added to.
TTDK_API(int, ttdk_rms_bwd, (const bf16_t* dy, const bf16_t* s, const float* rstd, const float* gamma, bf16_t* ds_out,
                             bf16_t* dx_out, float* part, float* dgamma, int accumulate, int rows, int H, float p_in,
                             unsigned site_in, float p_out, unsigned site_out, const long long* rng, hipStream_t st)) {
  if (!rms_width_ok(H) || rows <= 0 || !dy || !s || !rstd || !gamma || !ds_out || !part || !dgamma)
    return hipErrorInvalidValue;
  if (!aligned16(dy) || !aligned16(s) || !aligned16(gamma) || !aligned16(ds_out) || !aligned16(dx_out) ||
      !aligned16(part) || !aligned16(dgamma))
    return hipErrorInvalidValue;
  if ((p_in > 0.f || p_out > 0.f) && !rng) return hipErrorInvalidValue;
  DropSpec d = make_drop(rng, site_in, p_in, site_out, p_out);
  const int nb = ttdk_rms_bwd_num_blocks(rows);
  const int rpb = (rows + nb - 1) / nb;
  TTDK_RMS_BWD_DISPATCH(0, st, dy, s, rstd, gamma, ds_out, dx_out, part, rows, rpb, d);
  return ttdk_colreduce(part, nb, H, H, dgamma, accumulate, st);
}

TTDK_API(int, ttdk_rms_generic_fwd, (const void* x, const float* g, void* y, float* rstd, int dt, long long rows, int H,
                                     float eps, hipStream_t st)) {
  if (H <= 0 || rows <= 0 || !x || !g || !y || !rstd) return hipErrorInvalidValue;
  dim3 grid(static_cast<unsigned>((rows + 3) / 4));
  if (dt == 0)
    hipLaunchKernelGGL(rms_generic_fwd_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x), g,
                       static_cast<float*>(y), rstd, rows, H, eps);
  else if (dt == 1)
    hipLaunchKernelGGL(rms_generic_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(x), g,
                       static_cast<bf16_t*>(y), rstd, rows, H, eps);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// Row blocks the generic dgamma kernel splits the rows into (= rows of its [T][H] workspace).
TTDK_API(int, ttdk_rms_generic_parts, (long long rows, int H)) {
  const long long cb = (H + 63) / 64;
  long long t = (rows + 255) / 256;
  const long long cap = 2048 / cb > 1 ? 2048 / cb : 1;
  if (t > cap) t = cap;
  return static_cast<int>(t < 1 ? 1 : t);
}

// dx (nullable: not wanted) and dgamma (fp32 [H], written or added to); part: fp32
// [ttdk_rms_generic_parts(rows, H)][H] workspace.
TTDK_API(int, ttdk_rms_generic_bwd, (const void* dy, const void* x, const float* g, const float* rstd, void* dx,
                                     float* part, float* dgamma, int accumulate, int dt, long long rows, int H,
                                     hipStream_t st)) {
  if (H <= 0 || rows <= 0 || !dy || !x || !g || !rstd || !part || !dgamma || (dt != 0 && dt != 1))
    return hipErrorInvalidValue;
  const int T = ttdk_rms_generic_parts(rows, H);
  const long long rpb = (rows + T - 1) / T;
  dim3 grid(static_cast<unsigned>((rows + 3) / 4)), pgrid((H + 63) / 64, T);
  if (dt == 0) {
    if (dx)
      hipLaunchKernelGGL(rms_generic_bwd_dx_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(dy),
                         static_cast<const float*>(x), g, rstd, static_cast<float*>(dx), rows, H);
    hipLaunchKernelGGL(rms_generic_dgamma_kernel<float>, pgrid, dim3(256), 0, st, static_cast<const float*>(dy),
                       static_cast<const float*>(x), rstd, rows, H, rpb, part);
  } else {
    if (dx)
      hipLaunchKernelGGL(rms_generic_bwd_dx_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(dy),
                         static_cast<const bf16_t*>(x), g, rstd, static_cast<bf16_t*>(dx), rows, H);
    hipLaunchKernelGGL(rms_generic_dgamma_kernel<bf16_t>, pgrid, dim3(256), 0, st, static_cast<const bf16_t*>(dy),
                       static_cast<const bf16_t*>(x), rstd, rows, H, rpb, part);
  }
  hipLaunchKernelGGL(rms_generic_reduce_kernel, dim3((H + 255) / 256), dim3(256), 0, st, part, T, H, dgamma, accumulate);
  return hipGetLastError();
}

// Number of threads the capped SwiGLU grid launches (tests size their grid-stride case from it).
TTDK_API(int, ttdk_swiglu_max_threads, ()) { return kGluMaxBlocks * kGluBlock; }

static bool glu_vec_ok(int dt, int I, long long ld0, long long ld1, long long ld2, const void* p0, const void* p1,
                       const void* p2) {
  const int E = dt == 0 ? 4 : 8;
  return I % E == 0 && ld0 % E == 0 && ld1 % E == 0 && ld2 % E == 0 && aligned16(p0) && aligned16(p1) && aligned16(p2);
}

// h[r, :I] = silu(x2[r, :I]) * x2[r, I:2I]. x2: [rows, >= 2I] with row stride ldx, h: [rows, >= I]
// with row stride ldh (elements), both of type dt and element-aligned. x2 and h must not overlap.
TTDK_API(int, ttdk_swiglu_fwd, (const void* x2, long long ldx, void* h, long long ldh, int dt, long long rows, int I,
                                hipStream_t st)) {
  if ((dt != 0 && dt != 1) || rows < 0 || I <= 0 || !x2 || !h) return hipErrorInvalidValue;
  if (ldx < 2LL * I || ldh < I || rows > (1LL << 40)) return hipErrorInvalidValue;
  const uintptr_t em = dt == 0 ? 3 : 1;
  if ((reinterpret_cast<uintptr_t>(x2) & em) || (reinterpret_cast<uintptr_t>(h) & em)) return hipErrorInvalidValue;
  if (rows == 0) return 0;
  const bool vec = glu_vec_ok(dt, I, ldx, ldh, ldh, x2, h, h);
  if (dt == 0) return swiglu_fwd_launch<float>(x2, ldx, h, ldh, rows, I, vec, st);
  return swiglu_fwd_launch<bf16_t>(x2, ldx, h, ldh, rows, I, vec, st);
}

// dx2[r] = [da | db] from dh [rows, >= I] (row stride ldh) and x2 [rows, >= 2I] (ldx); dx2 [rows, >= 2I]
// (ldd). dx2 == x2 with ldd == ldx is in place; any other overlap is the caller's error.
TTDK_API(int, ttdk_swiglu_bwd, (const void* dh, long long ldh, const void* x2, long long ldx, void* dx2, long long ldd,
                                int dt, long long rows, int I, hipStream_t st)) {
  if ((dt != 0 && dt != 1) || rows < 0 || I <= 0 || !dh || !x2 || !dx2) return hipErrorInvalidValue;
  if (ldh < I || ldx < 2LL * I || ldd < 2LL * I || rows > (1LL << 40)) return hipErrorInvalidValue;
  if (dx2 == x2 && ldd != ldx) return hipErrorInvalidValue;
  const uintptr_t em = dt == 0 ? 3 : 1;
  if ((reinterpret_cast<uintptr_t>(dh) & em) || (reinterpret_cast<uintptr_t>(x2) & em) ||
      (reinterpret_cast<uintptr_t>(dx2) & em))
    return hipErrorInvalidValue;
  if (rows == 0) return 0;
  const bool vec = glu_vec_ok(dt, I, ldh, ldx, ldd, dh, x2, dx2);
  if (dt == 0) return swiglu_bwd_launch<float>(dh, ldh, x2, ldx, dx2, ldd, rows, I, vec, st);
  return swiglu_bwd_launch<bf16_t>(dh, ldh, x2, ldx, dx2, ldd, rows, I, vec, st);
}
