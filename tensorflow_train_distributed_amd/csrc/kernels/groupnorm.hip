// Group normalisation (Keras GroupNormalization(axis=-1), Wu & He 2018) for gfx950: forward and backward.
//
//   x  [N, M, C] channels last (bf16 or fp32; M = product of the spatial extents), G groups of
//   Cg = C / G consecutive channels; group (n, g) is the m = M * Cg elements x[n, :, g*Cg : (g+1)*Cg]:
//     mean = sum / m, var = sum (x - mean)^2 / m (biased), rstd = 1 / sqrt(var + eps)
//     y  = (x - mean) * rstd * gamma[c] + beta[c]                  (gamma = 1 / beta = 0 when absent)
//     xh = (x - mean) * rstd
//     dbeta[c] = sum_{n,p} dy, dgamma[c] = sum_{n,p} dy * xh
//     A[n,g] = sum_{p, c in g} gamma_c * dy, B[n,g] = sum_{p, c in g} gamma_c * dy * xh
//     dx = rstd * (gamma * dy - A / m - xh * B / m)
//   Statistics, gamma, beta and their gradients are fp32; mean and rstd are [N, G]. bf16 tensors
//   are accumulated in fp32 and rounded once (RNE); fp32 tensors compute and stay in fp32.
//
// Structure. The streaming kernels know nothing about groups: the small fold kernels hand them
// per-(n, c) coefficient rows.
//   1 gn_partial<.., false>  the M pixel rows of every image are cut into T slabs (groupnorm_plan.h);
//       block (channel chunk, slab) reads whole NHWC rows, each lane keeps per-channel sums of
//       (x - p_c) and (x - p_c)^2 with the pivot p_c = x[n, 0, c]: a sample of the data, so the
//       one-pass sums do not cancel when the mean is large against the spread. The lanes of a
//       block that share a channel are summed through LDS in thread order: part[n][t][2][C].
//   2 gn_fwd_fold  block (image, chunk of whole groups, about 256 channels): per channel fold the
//       T slabs in slab order into a mean and a centred second moment; per group merge its Cg
//       channels (equal counts: mean_g = first + sum (mean_c - first) / Cg,
//       M2_g = sum M2_c + M * sum (mean_c - mean_g)^2); write mean, rstd [N, G] and the rows
//       mean_c[n][c], scale[n][c] = rstd * gamma_c. Deviation from "in channel order": a wave owns
//       a group, lane l sums channels l, l + 64, ... in that order and the lane sums go through
//       the xor butterfly, a fixed tree. With one block per image, one thread walking a group
//       serially and the apply kernels looping over the channel chunks, the whole forward took
//       42 us at 14x14x1024 and 70 us at 7x7x2048 (Cg = 32, 64) against 20 us now.
//   3 gn_apply<.., false>  y = (x - mean_c) * scale + beta_c, in that form.
//   4 gn_partial<.., true>   part[n][t][2][C] = sum dy, sum dy * (x - mean) * rstd (centred inside
//       the sum). Deviation from "no group logic": each lane looks up mean / rstd of its channels'
//       groups (one integer division per channel) once per slab, outside the row loop, which
//       saves a launch that would only expand [N, G] into [N, C] rows.
//   5 gn_bwd_fold  the blocks and waves of gn_fwd_fold: fold the slabs per channel, form A, B per
//       group, write the rows mean_c, p = rstd * gamma_c, q = -rstd^2 * B / m, r = -rstd * A / m;
//       gn_param_grads then sums the folded rows over n in image order into dgamma / dbeta
//       ((+)= with accumulate). It is a kernel of this file and not ttdk_colreduce because that one
//       wants C % 4 == 0 and 16-byte aligned outputs, and the generic form takes any C.
//   6 gn_apply<.., true>   dx = p * dy + q * (x - mean_c) + r; its own launcher, called only when x
//       needs a gradient.
// Each streaming kernel is one template in two forms (groupnorm_plan.h holds the admission rule):
// * Fast <bf16_t, 8>: bf16, C % 8 == 0, 16-byte aligned bases. A lane owns 8 consecutive channels:
//   16-byte loads and stores, 16-byte fp32 coefficient loads; at most 32 lanes share a row, so a
//   block has at least 8 rows in flight and a thread four loads (two of each tensor in the
//   backward sums) before it does arithmetic.
// * Generic <T, 1>: 64-wide column groups, 4 rows per block, any C, any G | C, fp32 or bf16,
//   scalar accesses.
//
// No atomics anywhere; every reduction goes through partial rows folded in a fixed order, so every
// output is bitwise the same on every run. Element offsets are long long. Grids are capped at
// about 2048 blocks and strided; the row loops advance pointers by host-computed steps and hold no
// division. Launchers allocate nothing and do not synchronise: everything runs on the given stream.
//
// dt: 0 = fp32, 1 = bf16 (the codes of nn_generic.hip). form: 0 = by the plan, 1 = generic.
//
// Compiler resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
// scratch is 0 for every kernel here; VGPRs and occupancy per kernel are in profiles/groupnorm_bench.txt.
#include "common.h"
#include "groupnorm_plan.h"

namespace ttdk {
namespace {

namespace gnplan = ::ttdk::gnplan;

constexpr int kGnBlock = gnplan::kBlock;
constexpr int kGnMaxBlocks = 2048;

// Lanes of a streaming block: LC lanes share a pixel row, TL rows in flight; lane l of chunk k owns
// channel vector k * LC + l of the CGT a row has (V channels each).
struct GnLanes {
  int C, CGT, LC, TL, chunks;
};

template <typename T, int V>
__device__ __forceinline__ void ldv(const T* p, float (&f)[V]) {
  if constexpr (V == 8) {
    unpack8(*reinterpret_cast<const uint4*>(p), f);
  } else if constexpr (sizeof(T) == 2) {
    f[0] = bf2f(*p);
  } else {
    f[0] = *p;
  }
}

template <typename T, int V>
__device__ __forceinline__ void stv(T* p, const float (&f)[V]) {
  if constexpr (V == 8) {
    *reinterpret_cast<uint4*>(p) = pack8(f);
  } else if constexpr (sizeof(T) == 2) {
    *p = f2bf(f[0]);
  } else {
    *p = f[0];
  }
}

// V fp32 coefficients (16-byte loads when V == 8), or `fill` when the row is absent.
template <int V>
__device__ __forceinline__ void ldc(const float* p, float (&f)[V], float fill = 0.f) {
  if (!p) {
#pragma unroll
    for (int k = 0; k < V; ++k) f[k] = fill;
  } else if constexpr (V == 8) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w;
    f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
  } else {
    f[0] = *p;
  }
}

// ------------------------------------------------------------------ kernels 1 and 4: slab partial sums
// Block (channel chunk, slab s = n * Tn + t), both strided. !BWD: a = x, sums of (a - pivot),
// (a - pivot)^2. BWD: a = dy, sums of a, a * (x - mean) * rstd.
template <typename T, int V, bool BWD>
__global__ __launch_bounds__(kGnBlock) void gn_partial(const T* __restrict__ a, const T* __restrict__ x,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       float* __restrict__ part, long long M, GnLanes L, int Cg, int G,
                                                       int Tn, long long rows_per, long long ps, long long slabs) {
  __shared__ float red[2 * kGnBlock * V];
  const int tid = threadIdx.x;
  const int cgl = tid % L.LC, tl = tid / L.LC;
  const long long step = static_cast<long long>(L.TL) * L.C;
  for (long long s = blockIdx.y; s < slabs; s += gridDim.y) {
    const long long n = s / Tn;
    const int t = static_cast<int>(s - n * Tn);
    const long long r0 = t * rows_per;
    const long long r1 = r0 + rows_per < M ? r0 + rows_per : M;
    const long long img = n * M * L.C;
    for (int chunk = blockIdx.x; chunk < L.chunks; chunk += gridDim.x) {
      const int cg = chunk * L.LC + cgl;
      float s1[V], s2[V];
#pragma unroll
      for (int k = 0; k < V; ++k) s1[k] = 0.f, s2[k] = 0.f;
      if (tl < L.TL && cg < L.CGT) {
        const int c0 = cg * V;
        float mu[V], rs[V];  // !BWD: mu = pivot
        if constexpr (BWD) {
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const int g = (c0 + k) / Cg;
            mu[k] = mean[n * G + g];
            rs[k] = rstd[n * G + g];
          }
        } else {
          ldv<T, V>(a + img + c0, mu);
        }
        // U rows per pass, all loads issued before the arithmetic. A row past the slab is loaded
        // from the pass's first row (in range) and enters the sums as zeros, so a short slab has
        // no serial tail. The fast backward holds two tensors: U = 2 keeps it at 4 waves per SIMD.
        constexpr int U = (BWD && V == 8) ? 2 : 4;
        const T* pa = a + img + (r0 + tl) * L.C + c0;
        const T* px = BWD ? x + img + (r0 + tl) * L.C + c0 : nullptr;
        for (long long r = r0 + tl; r < r1; r += U * L.TL, pa += U * step) {
          float va[U][V], vx[U][V];
          bool ok[U];
#pragma unroll
          for (int i = 0; i < U; ++i) {
            ok[i] = r + i * L.TL < r1;
            ldv<T, V>(ok[i] ? pa + i * step : pa, va[i]);
          }
          if constexpr (BWD) {
#pragma unroll
            for (int i = 0; i < U; ++i) ldv<T, V>(ok[i] ? px + i * step : px, vx[i]);
            px += U * step;
          }
#pragma unroll
          for (int i = 0; i < U; ++i)
#pragma unroll
            for (int k = 0; k < V; ++k) {
              if constexpr (BWD) {
                const float d = ok[i] ? va[i][k] : 0.f;
                s1[k] += d;
                s2[k] += d * ((vx[i][k] - mu[k]) * rs[k]);
              } else {
                const float d = ok[i] ? va[i][k] - mu[k] : 0.f;
                s1[k] += d;
                s2[k] += d * d;
              }
            }
        }
      }
      // sum the TL threads of every channel in thread order
      __syncthreads();
#pragma unroll
      for (int k = 0; k < V; ++k) {
        red[tid * V + k] = s1[k];
        red[(kGnBlock + tid) * V + k] = s2[k];
      }
      __syncthreads();
      if (tid < L.LC * V) {
        const int c = tid / V, k = tid % V;
        float t1 = 0.f, t2 = 0.f;
        for (int u = 0; u < L.TL; ++u) {
          t1 += red[(u * L.LC + c) * V + k];
          t2 += red[(kGnBlock + u * L.LC + c) * V + k];
        }
        const int ocg = chunk * L.LC + c;
        if (ocg < L.CGT) {
          float* row = part + s * 2 * ps + ocg * V + k;
          row[0] = t1;
          row[ps] = t2;
        }
      }
    }
  }
}

// ------------------------------------------------------------------ kernel 2: forward fold
// Block (image n strided, group chunk): the gpb consecutive groups [blockIdx.y * gpb, ...) and their
// channels. A wave owns a group at a time: lane l sums channels l, l + 64, ... of the group in that
// order and the 64 lane sums go through the xor butterfly of wave_sum, a fixed tree.
template <typename T>
__global__ __launch_bounds__(kGnBlock) void gn_fwd_fold(const T* __restrict__ x, const float* __restrict__ part,
                                                        const float* __restrict__ gamma, float* __restrict__ chan,
                                                        float* __restrict__ coef, float* __restrict__ mean,
                                                        float* __restrict__ rstd, long long N, long long M, int C, int G,
                                                        int gpb, int Tn, long long ps, float eps) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Cg = C / G;
  const int g0 = blockIdx.y * gpb, g1 = g0 + gpb < G ? g0 + gpb : G;
  const int c_lo = g0 * Cg, c_hi = g1 * Cg;
  const float fM = static_cast<float>(M);
  for (long long n = blockIdx.x; n < N; n += gridDim.x) {
    float* ch = chan + n * 2 * ps;
    float* co = coef + n * 2 * ps;
    const T* x0 = x + n * M * C;
    for (int c = c_lo + tid; c < c_hi; c += kGnBlock) {
      const float* p = part + n * Tn * 2 * ps + c;
      float s1 = 0.f, s2 = 0.f;
#pragma unroll 4
      for (int t = 0; t < Tn; ++t) {
        s1 += p[t * 2 * ps];
        s2 += p[t * 2 * ps + ps];
      }
      float piv[1];
      ldv<T, 1>(x0 + c, piv);
      const float d = s1 / fM;
      const float m2 = s2 - s1 * d;
      ch[c] = piv[0] + d;
      ch[ps + c] = m2 > 0.f ? m2 : 0.f;
    }
    __syncthreads();
    for (int g = g0 + wave; g < g1; g += kGnBlock / 64) {
      const float* mc = ch + g * Cg;
      const float first = mc[0];
      float sd = 0.f;
      for (int j = lane; j < Cg; j += 64) sd += mc[j] - first;
      const float mg = first + wave_sum(sd) / static_cast<float>(Cg);
      float m2 = 0.f;
      for (int j = lane; j < Cg; j += 64) {
        const float d = mc[j] - mg;
        m2 += mc[ps + j] + fM * (d * d);
      }
      const float var = wave_sum(m2) / (fM * static_cast<float>(Cg));
      if (lane == 0) {
        mean[n * G + g] = mg;
        rstd[n * G + g] = 1.0f / sqrtf(var + eps);
      }
    }
    __syncthreads();
    for (int c = c_lo + tid; c < c_hi; c += kGnBlock) {
      const int g = c / Cg;
      co[c] = mean[n * G + g];
      co[ps + c] = rstd[n * G + g] * (gamma ? gamma[c] : 1.0f);
    }
  }
}

// ------------------------------------------------------------------ kernels 3 and 6: apply
// Block (row block, image, channel chunk), all strided. !BWD: y = (a - c0) * c1 + beta
// with coef rows [2][ps]. BWD: a = dy, dx = c1 * dy + c2 * (x - c0) + c3 with coef rows [4][ps].
template <typename T, int V, bool BWD>
__global__ __launch_bounds__(kGnBlock) void gn_apply(const T* __restrict__ a, const T* __restrict__ x,
                                                     const float* __restrict__ coef, const float* __restrict__ beta,
                                                     T* __restrict__ out, long long N, long long M, GnLanes L,
                                                     long long ps) {
  const int tid = threadIdx.x;
  const int cgl = tid % L.LC, tl = tid / L.LC;
  if (tl >= L.TL) return;
  const long long step = static_cast<long long>(gridDim.x) * L.TL * L.C;
  const long long rstep = static_cast<long long>(gridDim.x) * L.TL;
  for (long long n = blockIdx.y; n < N; n += gridDim.y) {
    const float* co = coef + n * (BWD ? 4 : 2) * ps;
    for (int chunk = blockIdx.z; chunk < L.chunks; chunk += gridDim.z) {
      const int cg = chunk * L.LC + cgl;
      if (cg >= L.CGT) continue;
      const int c0 = cg * V;
      float k0[V], k1[V], k2[V], k3[V];
      ldc<V>(co + c0, k0);
      ldc<V>(co + ps + c0, k1);
      if constexpr (BWD) {
        ldc<V>(co + 2 * ps + c0, k2);
        ldc<V>(co + 3 * ps + c0, k3);
      } else {
        ldc<V>(beta ? beta + c0 : nullptr, k3);
      }
      long long r = static_cast<long long>(blockIdx.x) * L.TL + tl;
      const long long off = (n * M + r) * L.C + c0;
      const T* pa = a + off;
      const T* px = BWD ? x + off : nullptr;
      T* po = out + off;
      // four rows per pass, all loads first; a row past the image is loaded from the pass's first
      // row and not stored
      for (; r < M; r += 4 * rstep, pa += 4 * step, po += 4 * step) {
        float va[4][V], vx[4][V];
        bool ok[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ok[i] = r + i * rstep < M;
          ldv<T, V>(ok[i] ? pa + i * step : pa, va[i]);
        }
        if constexpr (BWD) {
#pragma unroll
          for (int i = 0; i < 4; ++i) ldv<T, V>(ok[i] ? px + i * step : px, vx[i]);
          px += 4 * step;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float o[V];
#pragma unroll
          for (int k = 0; k < V; ++k) {
            if constexpr (BWD)
              o[k] = k1[k] * va[i][k] + k2[k] * (vx[i][k] - k0[k]) + k3[k];
            else
              o[k] = (va[i][k] - k0[k]) * k1[k] + k3[k];
          }
          if (ok[i]) stv<T, V>(po + i * step, o);
        }
      }
    }
  }
}

// ------------------------------------------------------------------ kernel 5: backward fold
// The blocks and waves of gn_fwd_fold.
__global__ __launch_bounds__(kGnBlock) void gn_bwd_fold(const float* __restrict__ part, const float* __restrict__ gamma,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        float* __restrict__ fold, float* __restrict__ ab,
                                                        float* __restrict__ coef, long long N, long long M, int C, int G,
                                                        int gpb, int Tn, long long ps) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Cg = C / G;
  const int g0 = blockIdx.y * gpb, g1 = g0 + gpb < G ? g0 + gpb : G;
  const int c_lo = g0 * Cg, c_hi = g1 * Cg;
  const float inv_m = 1.0f / (static_cast<float>(M) * static_cast<float>(Cg));
  for (long long n = blockIdx.x; n < N; n += gridDim.x) {
    float* fo = fold + n * 2 * ps;
    float* gb = ab + n * 2 * ps;
    float* co = coef + n * 4 * ps;
    for (int c = c_lo + tid; c < c_hi; c += kGnBlock) {
      const float* p = part + n * Tn * 2 * ps + c;
      float s1 = 0.f, s2 = 0.f;
#pragma unroll 4
      for (int t = 0; t < Tn; ++t) {
        s1 += p[t * 2 * ps];
        s2 += p[t * 2 * ps + ps];
      }
      fo[c] = s1;
      fo[ps + c] = s2;
    }
    __syncthreads();
    for (int g = g0 + wave; g < g1; g += kGnBlock / 64) {
      float A = 0.f, B = 0.f;
      for (int j = lane; j < Cg; j += 64) {
        const int c = g * Cg + j;
        const float gm = gamma ? gamma[c] : 1.0f;
        A += gm * fo[c];
        B += gm * fo[ps + c];
      }
      A = wave_sum(A);
      B = wave_sum(B);
      if (lane == 0) {
        gb[g] = A;
        gb[ps + g] = B;
      }
    }
    __syncthreads();
    for (int c = c_lo + tid; c < c_hi; c += kGnBlock) {
      const int g = c / Cg;
      const float rs = rstd[n * G + g];
      co[c] = mean[n * G + g];
      co[ps + c] = rs * (gamma ? gamma[c] : 1.0f);
      co[2 * ps + c] = -(rs * rs) * gb[ps + g] * inv_m;
      co[3 * ps + c] = -rs * gb[g] * inv_m;
    }
  }
}

// dbeta[c] (+)= sum_n fold[n][0][c], dgamma[c] (+)= sum_n fold[n][1][c], in image order.
__global__ __launch_bounds__(kGnBlock) void gn_param_grads(const float* __restrict__ fold, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, long long N, int C, long long ps,
                                                           int accumulate) {
  const int c = blockIdx.x * kGnBlock + threadIdx.x;
  if (c >= C) return;
  float sb = 0.f, sg = 0.f;
  const float* p = fold + c;
  for (long long n = 0; n < N; ++n, p += 2 * ps) {
    sb += p[0];
    sg += p[ps];
  }
  if (dbeta) dbeta[c] = accumulate ? dbeta[c] + sb : sb;
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + sg : sg;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline GnLanes make_lanes(int C, bool fast) {
  GnLanes L;
  L.C = C;
  L.CGT = fast ? C / gnplan::kVec : C;
  L.LC = gnplan::lanes(C, fast);
  L.TL = gnplan::rows_per_block(C, fast);
  L.chunks = gnplan::chunks(C, fast);
  return L;
}

inline dim3 partial_grid(long long slabs, const GnLanes& L) {
  const unsigned gy = static_cast<unsigned>(slabs < kGnMaxBlocks ? slabs : kGnMaxBlocks);
  unsigned gx = kGnMaxBlocks / gy;
  if (gx > static_cast<unsigned>(L.chunks)) gx = L.chunks;
  return dim3(gx < 1 ? 1 : gx, gy);
}

// Four rows per thread and pass, so that the coefficient loads are shared, where that still leaves
// 512 blocks; one row per thread and pass otherwise (small images are latency-bound).
inline dim3 apply_grid(long long N, long long M, const GnLanes& L) {
  const unsigned gy = static_cast<unsigned>(N < kGnMaxBlocks ? N : kGnMaxBlocks);
  unsigned gz = kGnMaxBlocks / gy;
  if (gz > static_cast<unsigned>(L.chunks)) gz = L.chunks;
  if (gz > 64) gz = 64;
  if (gz < 1) gz = 1;
  long long gx = (M + 4LL * L.TL - 1) / (4LL * L.TL);
  if (gx * gy * gz < 512) gx = (M + L.TL - 1) / L.TL;
  const long long cap = kGnMaxBlocks / (static_cast<long long>(gy) * gz);
  if (gx > cap) gx = cap;
  return dim3(static_cast<unsigned>(gx < 1 ? 1 : gx), gy, gz);
}

// Groups per fold block: about a block's worth of channels, whole groups; and the fold grid
// (images strided, group chunks).
inline int fold_gpb(int C, int G) {
  const int Cg = C / G;
  const int gpb = kGnBlock / Cg;
  return gpb < 1 ? 1 : gpb;
}
inline dim3 fold_grid(long long N, int C, int G) {
  const int gpb = fold_gpb(C, G);
  const unsigned gy = static_cast<unsigned>((G + gpb - 1) / gpb);
  unsigned gx = kGnMaxBlocks / (gy < kGnMaxBlocks ? gy : kGnMaxBlocks);
  if (gx < 1) gx = 1;
  if (gx > N) gx = static_cast<unsigned>(N);
  return dim3(gx, gy);
}

template <typename T, int V>
int fwd_launch(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, float* ws,
               long long N, long long M, int C, int G, float eps, hipStream_t st) {
  const GnLanes L = make_lanes(C, V == gnplan::kVec);
  const int Tn = gnplan::parts(N, M, C);
  const long long ps = gnplan::part_stride(C), per = gnplan::rows_per_slab(N, M, C), slabs = N * Tn;
  float* part = ws;
  float* chan = part + slabs * 2 * ps;
  float* coef = chan + N * 2 * ps;
  const T* xt = static_cast<const T*>(x);
  hipLaunchKernelGGL((gn_partial<T, V, false>), partial_grid(slabs, L), dim3(kGnBlock), 0, st, xt,
                     static_cast<const T*>(nullptr), static_cast<const float*>(nullptr),
                     static_cast<const float*>(nullptr), part, M, L, C / G, G, Tn, per, ps, slabs);
  hipLaunchKernelGGL(gn_fwd_fold<T>, fold_grid(N, C, G), dim3(kGnBlock), 0, st, xt, part, gamma, chan, coef, mean, rstd,
                     N, M, C, G, fold_gpb(C, G), Tn, ps, eps);
  hipLaunchKernelGGL((gn_apply<T, V, false>), apply_grid(N, M, L), dim3(kGnBlock), 0, st, xt,
                     static_cast<const T*>(nullptr), coef, beta, static_cast<T*>(y), N, M, L, ps);
  return hipGetLastError();
}

template <typename T, int V>
int bwd_stats_launch(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                     float* dgamma, float* dbeta, float* ws, long long N, long long M, int C, int G, int accumulate,
                     hipStream_t st) {
  const GnLanes L = make_lanes(C, V == gnplan::kVec);
  const int Tn = gnplan::parts(N, M, C);
  const long long ps = gnplan::part_stride(C), per = gnplan::rows_per_slab(N, M, C), slabs = N * Tn;
  float* part = ws;
  float* fold = part + slabs * 2 * ps;
  float* ab = fold + N * 2 * ps;
  float* coef = ab + N * 2 * ps;
  hipLaunchKernelGGL((gn_partial<T, V, true>), partial_grid(slabs, L), dim3(kGnBlock), 0, st, static_cast<const T*>(dy),
                     static_cast<const T*>(x), mean, rstd, part, M, L, C / G, G, Tn, per, ps, slabs);
  hipLaunchKernelGGL(gn_bwd_fold, fold_grid(N, C, G), dim3(kGnBlock), 0, st, part, gamma, mean, rstd, fold, ab, coef, N,
                     M, C, G, fold_gpb(C, G), Tn, ps);
  if (dgamma || dbeta)
    hipLaunchKernelGGL(gn_param_grads, dim3((C + kGnBlock - 1) / kGnBlock), dim3(kGnBlock), 0, st, fold, dgamma, dbeta,
                       N, C, ps, accumulate);
  return hipGetLastError();
}

template <typename T, int V>
int bwd_dx_launch(const void* dy, const void* x, const float* ws, void* dx, long long N, long long M, int C,
                  hipStream_t st) {
  const GnLanes L = make_lanes(C, V == gnplan::kVec);
  const long long ps = gnplan::part_stride(C);
  const float* coef = ws + (gnplan::parts(N, M, C) + 2LL) * N * 2 * ps;
  hipLaunchKernelGGL((gn_apply<T, V, true>), apply_grid(N, M, L), dim3(kGnBlock), 0, st, static_cast<const T*>(dy),
                     static_cast<const T*>(x), coef, static_cast<const float*>(nullptr), static_cast<T*>(dx), N, M, L,
                     ps);
  return hipGetLastError();
}

}  // namespace
}  // namespace ttdk

using namespace ttdk;

// y, mean [N,G], rstd [N,G] of x [N,M,C] (type dt). gamma / beta: fp32 [C] or null. ws: 16-byte
// aligned fp32 workspace of at least gnplan::fwd_ws_floats(N, M, C) floats.
TTDK_API(int, ttdk_group_norm_fwd, (const void* x, const float* gamma, const float* beta, void* y, float* mean,
                                    float* rstd, float* ws, long long ws_floats, long long N, long long M, int C, int G,
                                    float eps, int dt, int form, hipStream_t st)) {
  if (!gnplan::valid(N, M, C, G) || !x || !y || !mean || !rstd || !ws || (dt != 0 && dt != 1)) return hipErrorInvalidValue;
  if (!aligned16(ws) || ws_floats < gnplan::fwd_ws_floats(N, M, C)) return hipErrorInvalidValue;
  if (form == 0 && gnplan::fast_takes(N, M, C, G, dt) && aligned16(x) && aligned16(y) && aligned16(beta))
    return fwd_launch<bf16_t, gnplan::kVec>(x, gamma, beta, y, mean, rstd, ws, N, M, C, G, eps, st);
  return dt == 0 ? fwd_launch<float, 1>(x, gamma, beta, y, mean, rstd, ws, N, M, C, G, eps, st)
                 : fwd_launch<bf16_t, 1>(x, gamma, beta, y, mean, rstd, ws, N, M, C, G, eps, st);
}

// The sums of the backward: dgamma / dbeta fp32 [C] (either may be null; (+)= with accumulate) and,
// left in ws for ttdk_group_norm_bwd_dx, the coefficient rows of dx. ws: 16-byte aligned, at least
// gnplan::bwd_ws_floats(N, M, C) floats.
TTDK_API(int, ttdk_group_norm_bwd_stats, (const void* dy, const void* x, const float* gamma, const float* mean,
                                          const float* rstd, float* dgamma, float* dbeta, float* ws, long long ws_floats,
                                          long long N, long long M, int C, int G, int dt, int accumulate, int form,
                                          hipStream_t st)) {
  if (!gnplan::valid(N, M, C, G) || !dy || !x || !mean || !rstd || !ws || (dt != 0 && dt != 1))
    return hipErrorInvalidValue;
  if (!aligned16(ws) || ws_floats < gnplan::bwd_ws_floats(N, M, C)) return hipErrorInvalidValue;
  if (form == 0 && gnplan::fast_takes(N, M, C, G, dt) && aligned16(dy) && aligned16(x))
    return bwd_stats_launch<bf16_t, gnplan::kVec>(dy, x, gamma, mean, rstd, dgamma, dbeta, ws, N, M, C, G, accumulate,
                                                  st);
  return dt == 0 ? bwd_stats_launch<float, 1>(dy, x, gamma, mean, rstd, dgamma, dbeta, ws, N, M, C, G, accumulate, st)
                 : bwd_stats_launch<bf16_t, 1>(dy, x, gamma, mean, rstd, dgamma, dbeta, ws, N, M, C, G, accumulate, st);
}

// dx from the coefficient rows ttdk_group_norm_bwd_stats left in the same ws.
TTDK_API(int, ttdk_group_norm_bwd_dx, (const void* dy, const void* x, const float* ws, long long ws_floats, void* dx,
                                       long long N, long long M, int C, int G, int dt, int form, hipStream_t st)) {
  if (!gnplan::valid(N, M, C, G) || !dy || !x || !dx || !ws || (dt != 0 && dt != 1)) return hipErrorInvalidValue;
  if (!aligned16(ws) || ws_floats < gnplan::bwd_ws_floats(N, M, C)) return hipErrorInvalidValue;
  if (form == 0 && gnplan::fast_takes(N, M, C, G, dt) && aligned16(dy) && aligned16(x) && aligned16(dx))
    return bwd_dx_launch<bf16_t, gnplan::kVec>(dy, x, ws, dx, N, M, C, st);
  return dt == 0 ? bwd_dx_launch<float, 1>(dy, x, ws, dx, N, M, C, st)
                 : bwd_dx_launch<bf16_t, 1>(dy, x, ws, dx, N, M, C, st);
}
