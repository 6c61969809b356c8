// BatchNormalization (training mode, NHWC / channels-last) forward + backward on gfx950.
//
// North-star op (BASELINE.json "LayerNorm/BatchNorm"); the reference has BN commented out
// (/root/reference/distribute_training.py:56) but ResNet-50 needs it in every block.
//
// Forward statistics come either from the conv epilogue (per-tile partial sums, see
// gemm_conv.hip EpiParams::stat) or from ttdk_bn_stats_partial; both produce
// partial[T][2][C] which ttdk_bn_reduce_partials folds (2-D grid, LDS tree, one float
// atomic per block and channel) into sums[2][C]. Finalize kernels turn sums into per-channel
// affine coefficients so the streaming passes are a single FMA per element:
//   fwd:  out = act(y * scale + shift (+ residual)),  scale = gamma*rstd, shift = beta - mean*scale
//   bwd:  g = dy * [out > 0];  dz = a*g + b*y + c with
//         a = gamma*rstd, b = -gamma*rstd^3 * (sum(g*y) - mean*sum(g))/M, c = -a*sum(g)/M - b*mean
// All streaming passes move 16 B (8 bf16 channels) per lane.
#include "common.h"

namespace ttdk {
namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;  // independent 16 B loads per lane per trip in the streaming passes

// Sums over rows of x[M][C] (and of x^2), 8 channels per thread-column. Writes
// partial[blockIdx.x][2][C]. Requires C % 8 == 0.
__global__ __launch_bounds__(kThreads) void stats_partial_kernel(const bf16_t* __restrict__ x, long long M, int C,
                                                                 float* __restrict__ partial, long long rows_per_block) {
  __shared__ float red[2][kThreads][8];
  const int cg = C >> 3;                          // 8-channel groups per row
  const int cols = min(cg, kThreads);             // thread-columns
  const int rlanes = kThreads / cols;             // rows processed concurrently
  const int col = threadIdx.x % cols, rl = threadIdx.x / cols;
  const long long r0 = blockIdx.x * rows_per_block;
  const long long r1 = min(M, r0 + rows_per_block);
  for (int cbase = 0; cbase < cg; cbase += cols) {
    const int c8 = cbase + col;
    float s[8] = {0}, q[8] = {0};
    if (rl < rlanes && c8 < cg) {
      for (long long rb = r0 + rl; rb < r1; rb += static_cast<long long>(rlanes) * kUnroll) {
        uint4 xv[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const long long r = rb + static_cast<long long>(u) * rlanes;
          if (r < r1) xv[u] = *reinterpret_cast<const uint4*>(x + r * C + c8 * 8);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (rb + static_cast<long long>(u) * rlanes >= r1) break;
          float f[8];
          unpack8(xv[u], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            s[j] += f[j];
            q[j] += f[j] * f[j];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[0][threadIdx.x][j] = s[j];
      red[1][threadIdx.x][j] = q[j];
    }
    __syncthreads();
    if (rl == 0 && c8 < cg) {
      for (int k = 1; k < rlanes; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s[j] += red[0][col + k * cols][j];
          q[j] += red[1][col + k * cols][j];
        }
      float* p = partial + static_cast<long long>(blockIdx.x) * 2 * C + c8 * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[j] = s[j];
        p[C + j] = q[j];
      }
    }
    __syncthreads();
  }
}

// Backward partial sums: g = dy * [out > 0] (relu) ; sums of g and g*y. Optionally writes g.
__global__ __launch_bounds__(kThreads) void bwd_partial_kernel(const bf16_t* __restrict__ dy,
                                                               const bf16_t* __restrict__ out,
                                                               const uint8_t* __restrict__ mask,
                                                               const bf16_t* __restrict__ y, long long M, int C,
                                                               float* __restrict__ partial, long long rows_per_block,
                                                               bf16_t* __restrict__ g_out) {
  __shared__ float red[2][kThreads][8];
  const int cg = C >> 3;
  const int cols = min(cg, kThreads);
  const int rlanes = kThreads / cols;
  const int col = threadIdx.x % cols, rl = threadIdx.x / cols;
  const long long r0 = blockIdx.x * rows_per_block;
  const long long r1 = min(M, r0 + rows_per_block);
  for (int cbase = 0; cbase < cg; cbase += cols) {
    const int c8 = cbase + col;
    float s[8] = {0}, q[8] = {0};
    if (rl < rlanes && c8 < cg) {
      // kUnroll rows per trip, all loads issued before the math (several 16 B reads in flight)
      for (long long rb = r0 + rl; rb < r1; rb += static_cast<long long>(rlanes) * kUnroll) {
        uint4 gv[kUnroll], yr[kUnroll], ov[kUnroll];
        uint32_t mb[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const long long r = rb + static_cast<long long>(u) * rlanes;
          if (r < r1) {
            const long long off = r * C + c8 * 8;
            gv[u] = *reinterpret_cast<const uint4*>(dy + off);
            yr[u] = *reinterpret_cast<const uint4*>(y + off);
            if (mask) mb[u] = mask[off >> 3];
            else if (out) ov[u] = *reinterpret_cast<const uint4*>(out + off);
          }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const long long r = rb + static_cast<long long>(u) * rlanes;
          if (r >= r1) break;
          const long long off = r * C + c8 * 8;
          float g[8], yv[8];
          unpack8(gv[u], g);
          if (mask) {
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = (mb[u] >> j) & 1u ? g[j] : 0.f;
            if (g_out) *reinterpret_cast<uint4*>(g_out + off) = pack8(g);
          } else if (out) {
            float o[8];
            unpack8(ov[u], o);
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = o[j] > 0.f ? g[j] : 0.f;
            if (g_out) *reinterpret_cast<uint4*>(g_out + off) = pack8(g);
          }
          unpack8(yr[u], yv);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            s[j] += g[j];
            q[j] += g[j] * yv[j];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[0][threadIdx.x][j] = s[j];
      red[1][threadIdx.x][j] = q[j];
    }
    __syncthreads();
    if (rl == 0 && c8 < cg) {
      for (int k = 1; k < rlanes; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s[j] += red[0][col + k * cols][j];
          q[j] += red[1][col + k * cols][j];
        }
      float* p = partial + static_cast<long long>(blockIdx.x) * 2 * C + c8 * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[j] = s[j];
        p[C + j] = q[j];
      }
    }
    __syncthreads();
  }
}

// sums[2C] += sum over t of partial[t][2C]. grid = (ceil(2C/64), slices); block = 64 x 4.
__global__ __launch_bounds__(kThreads) void reduce_partials_kernel(const float* __restrict__ partial, int T, int C2,
                                                                   float* __restrict__ sums, int t_per_slice) {
  __shared__ float red[4][64];
  const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  const int t0 = blockIdx.y * t_per_slice, t1 = min(T, t0 + t_per_slice);
  float s = 0.f;
  if (c < C2)
    for (int t = t0 + ty; t < t1; t += 4) s += partial[static_cast<long long>(t) * C2 + c];
  red[ty][cx] = s;
  __syncthreads();
  if (ty == 0 && c < C2) atomicAdd(&sums[c], red[0][cx] + red[1][cx] + red[2][cx] + red[3][cx]);
}

__global__ void fwd_finalize_kernel(const float* __restrict__ sums, float count, int C, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, float eps, float momentum, float* running_mean,
                                    float* running_var, float* __restrict__ save_mean, float* __restrict__ save_rstd,
                                    float* __restrict__ scale, float* __restrict__ shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float mean = sums[c] / count;
  const float var = fmaxf(sums[C + c] / count - mean * mean, 0.f);
  const float rstd = rsqrtf(var + eps);
  save_mean[c] = mean;
  save_rstd[c] = rstd;
  const float sc = (gamma ? gamma[c] : 1.f) * rstd;
  scale[c] = sc;
  shift[c] = (beta ? beta[c] : 0.f) - mean * sc;
  if (running_mean) {  // TF/Keras convention: moving = moving * momentum + batch * (1 - momentum)
    const float unbiased = count > 1.f ? var * count / (count - 1.f) : var;
    running_mean[c] = running_mean[c] * momentum + mean * (1.f - momentum);
    running_var[c] = running_var[c] * momentum + unbiased * (1.f - momentum);
  }
}

__global__ void bwd_finalize_kernel(const float* __restrict__ sums, float count, int C, const float* __restrict__ gamma,
                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                    float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ coef,
                                    int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sg = sums[c], sgy = sums[C + c];
  const float m = mean[c], r = rstd[c];
  const float gam = gamma ? gamma[c] : 1.f;
  const float dgam = r * (sgy - m * sg);  // sum(g * xhat)
  if (dgamma) dgamma[c] = dgam + (accumulate ? dgamma[c] : 0.f);
  if (dbeta) dbeta[c] = sg + (accumulate ? dbeta[c] : 0.f);
  const float a = gam * r;
  const float b = -gam * r * r * dgam / count;
  const float cc = -a * sg / count - b * m;
  coef[c] = a;
  coef[C + c] = b;
  coef[2 * C + c] = cc;
}

// Cross-tile reduction + finalize in two fence-free launches (replacing memset + atomic
// reduce + finalize): reduce_slices folds partial[T][2][C] into slab[S][2][C] (grid =
// ceil(C/32) x S, block = 8 row-groups x 32 channels, <= 32 rows per block), finalize folds
// the S slab rows in a fixed order (deterministic, no float atomics) and writes the per-channel
// coefficients. A single-launch "last block finalizes" variant (arrival counter + device-scope
// fence per block; on gfx950 the release fence writes back the XCD's L2) measured ~3x slower
// than the three launches it was meant to replace, so this keeps two.
struct FinalizeArgs {
  float count;
  const float* gamma;
  const float* beta;  // fwd
  float eps, momentum;
  float* running_mean;
  float* running_var;
  float* mean;  // fwd: out; bwd: in
  float* rstd;  // fwd: out; bwd: in
  float* scale;  // fwd: out
  float* shift;  // fwd: out
  float* dgamma;  // bwd
  float* dbeta;   // bwd
  float* coef;    // bwd: [3][C]
  int accumulate;
};

__global__ __launch_bounds__(kThreads) void reduce_slices_kernel(const float* __restrict__ partial, int T, int C,
                                                                 int t_per_slice, float* __restrict__ slab) {
  __shared__ float red[2][8][33];
  const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const int t0 = blockIdx.y * t_per_slice, t1 = min(T, t0 + t_per_slice);
  float s = 0.f, q = 0.f;
  if (c < C) {
#pragma unroll 4
    for (int t = t0 + rg; t < t1; t += 8) {
      const float* p = partial + static_cast<long long>(t) * 2 * C + c;
      s += p[0];
      q += p[C];
    }
  }
  red[0][rg][cl] = s;
  red[1][rg][cl] = q;
  __syncthreads();
  if (rg == 0 && c < C) {
    for (int k = 1; k < 8; ++k) {
      s += red[0][k][cl];
      q += red[1][k][cl];
    }
    slab[(2LL * blockIdx.y) * C + c] = s;
    slab[(2LL * blockIdx.y + 1) * C + c] = q;
  }
}

template <bool BWD>
__global__ __launch_bounds__(kThreads) void finalize_kernel(const float* __restrict__ slab, int S, int C, FinalizeArgs a) {
  __shared__ float red[2][8][33];
  const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float s = 0.f, q = 0.f;
  if (c < C) {
#pragma unroll 4
    for (int y = rg; y < S; y += 8) {
      s += slab[(2LL * y) * C + c];
      q += slab[(2LL * y + 1) * C + c];
    }
  }
  red[0][rg][cl] = s;
  red[1][rg][cl] = q;
  __syncthreads();
  if (rg != 0 || c >= C) return;
  for (int k = 1; k < 8; ++k) {
    s += red[0][k][cl];
    q += red[1][k][cl];
  }
  const float gam = a.gamma ? a.gamma[c] : 1.f;
  if (!BWD) {
    const float mean = s / a.count;
    const float var = fmaxf(q / a.count - mean * mean, 0.f);
    const float rstd = rsqrtf(var + a.eps);
    a.mean[c] = mean;
    a.rstd[c] = rstd;
    const float sc = gam * rstd;
    a.scale[c] = sc;
    a.shift[c] = (a.beta ? a.beta[c] : 0.f) - mean * sc;
    if (a.running_mean) {
      const float unbiased = a.count > 1.f ? var * a.count / (a.count - 1.f) : var;
      a.running_mean[c] = a.running_mean[c] * a.momentum + mean * (1.f - a.momentum);
      a.running_var[c] = a.running_var[c] * a.momentum + unbiased * (1.f - a.momentum);
    }
  } else {
    const float m = a.mean[c], r = a.rstd[c];
    const float dgam = r * (q - m * s);
    if (a.dgamma) a.dgamma[c] = dgam + (a.accumulate ? a.dgamma[c] : 0.f);
    if (a.dbeta) a.dbeta[c] = s + (a.accumulate ? a.dbeta[c] : 0.f);
    const float ca = gam * r;
    const float cb = -gam * r * r * dgam / a.count;
    a.coef[c] = ca;
    a.coef[C + c] = cb;
    a.coef[2 * C + c] = -ca * s / a.count - cb * m;
  }
}

// Streaming passes. A block covers kUnroll*256 consecutive 8-channel vectors; when the
// number of 8-channel groups per row divides 256 (every ResNet width) a thread always sees
// the same channel group, so its per-channel coefficients live in registers (FIXED), and all
// kUnroll loads are issued before any math so each lane keeps several 16 B reads in flight.

// out = act(y*scale[c] + shift[c] (+ residual)); 8 channels per vector. With rscale/rshift
// the residual is itself a raw conv output whose BN is applied here (projection shortcut:
// its normalised tensor is never stored).
template <bool FIXED>
__global__ __launch_bounds__(kThreads) void apply_kernel(const bf16_t* __restrict__ y, const float* __restrict__ scale,
                                                         const float* __restrict__ shift,
                                                         const bf16_t* __restrict__ residual,
                                                         const float* __restrict__ rscale,
                                                         const float* __restrict__ rshift, bf16_t* __restrict__ out,
                                                         uint8_t* __restrict__ mask, uint8_t* __restrict__ q8,
                                                         float* __restrict__ q8_slot, long long n8, int C, int relu) {
  const int cg = C >> 3;
  // fp8 e4m3 copy with the slot's delayed scale; this step's amax goes to q8_slot[1]
  const float qs = q8 ? q8_slot[2] : 1.f;
  float qmax = 0.f;
  float sc[8], sh[8], rsc[8], rsh[8];
  auto load8 = [](const float* p, int c0, float (&d)[8]) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p + c0), b = *reinterpret_cast<const f32x4_t*>(p + c0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d[j] = a[j];
      d[4 + j] = b[j];
    }
  };
  auto load_coef = [&](int c0) {
    load8(scale, c0, sc);
    load8(shift, c0, sh);
    if (rscale) {
      load8(rscale, c0, rsc);
      load8(rshift, c0, rsh);
    }
  };
  if (FIXED) load_coef((threadIdx.x % cg) * 8);
  const long long span = static_cast<long long>(kThreads) * kUnroll;
  for (long long base = blockIdx.x * span; base < n8; base += static_cast<long long>(gridDim.x) * span) {
    uint4 yv[kUnroll], rv[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long long i = base + u * kThreads + threadIdx.x;
      if (i < n8) {
        yv[u] = reinterpret_cast<const uint4*>(y)[i];
        if (residual) rv[u] = reinterpret_cast<const uint4*>(residual)[i];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long long i = base + u * kThreads + threadIdx.x;
      if (i >= n8) break;
      if (!FIXED) load_coef(static_cast<int>(i % cg) * 8);
      float f[8];
      unpack8(yv[u], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = f[j] * sc[j] + sh[j];
      if (residual) {
        float r[8];
        unpack8(rv[u], r);
        if (rscale) {
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] += r[j] * rsc[j] + rsh[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] += r[j];
        }
      }
      if (relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = ttdk::relu(f[j]);
      }
      const uint4 packed = pack8(f);
      if (out) reinterpret_cast<uint4*>(out)[i] = packed;  // null: only the fp8 copy / mask are consumed
      if (mask) {  // 1 bit per element of [stored bf16 > 0]: the ReLU mask backward reads instead of `out`
        const uint32_t w[4] = {packed.x, packed.y, packed.z, packed.w};
        uint32_t mb = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t h = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
          mb |= ((h & 0x7fffu) != 0 && !(h & 0x8000u) ? 1u : 0u) << j;
        }
        mask[i] = static_cast<uint8_t>(mb);
      }
      if (q8) {
        float fq[8];
        unpack8(packed, fq);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          qmax = fmaxf(qmax, fabsf(fq[j]));
          const float v = fminf(fmaxf(fq[j] * qs, -448.f), 448.f);
          const uint32_t b = static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_fp8_f32(v, v, 0, false) & 0xff);
          if (j < 4) lo |= b << (8 * j);
          else hi |= b << (8 * (j - 4));
        }
        reinterpret_cast<uint2*>(q8)[i] = make_uint2(lo, hi);
      }
    }
  }
  if (q8) {  // block max, then one atomic per block spread over the slot's 64 amax lanes
    __shared__ float red[kThreads / 64];
    qmax = wave_max(qmax);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = qmax;
    __syncthreads();
    if (threadIdx.x == 0) {
      float m = red[0];
      for (int w = 1; w < kThreads / 64; ++w) m = fmaxf(m, red[w]);
      atomicMax(reinterpret_cast<unsigned int*>(q8_slot + 8 + (blockIdx.x & 63)), __float_as_uint(m));
    }
  }
}

// dz = a*g + b*y + c, g = dy * [out > 0] (ReLU mask bit, or `out` > 0, or no mask).
// q8: optional OCP e5m2 copy of dz (fp8 data gradients, ResNet config 5) quantised with the
// slot's delayed scale; this step's amax goes to the slot's 64 amax lanes (fp8.hip).
template <bool FIXED>
__global__ __launch_bounds__(kThreads) void bwd_apply_kernel(const bf16_t* __restrict__ dy,
                                                             const bf16_t* __restrict__ out,
                                                             const uint8_t* __restrict__ mask,
                                                             const bf16_t* __restrict__ y,
                                                             const float* __restrict__ coef, bf16_t* __restrict__ dz,
                                                             uint8_t* __restrict__ q8, float* __restrict__ q8_slot,
                                                             long long n8, int C) {
  const int cg = C >> 3;
  const float qs = q8 ? q8_slot[2] : 1.f;
  float qmax = 0.f;
  float ca[8], cb[8], cc[8];
  auto load_coef = [&](int c0) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const f32x4_t a = *reinterpret_cast<const f32x4_t*>(coef + c0 + 4 * k);
      const f32x4_t b = *reinterpret_cast<const f32x4_t*>(coef + C + c0 + 4 * k);
      const f32x4_t c = *reinterpret_cast<const f32x4_t*>(coef + 2 * C + c0 + 4 * k);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ca[4 * k + j] = a[j];
        cb[4 * k + j] = b[j];
        cc[4 * k + j] = c[j];
      }
    }
  };
  if (FIXED) load_coef((threadIdx.x % cg) * 8);
  const long long span = static_cast<long long>(kThreads) * kUnroll;
  for (long long base = blockIdx.x * span; base < n8; base += static_cast<long long>(gridDim.x) * span) {
    uint4 gv[kUnroll], yv[kUnroll], ov[kUnroll];
    uint32_t mb[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long long i = base + u * kThreads + threadIdx.x;
      if (i < n8) {
        gv[u] = reinterpret_cast<const uint4*>(dy)[i];
        yv[u] = reinterpret_cast<const uint4*>(y)[i];
        if (mask) mb[u] = mask[i];
        else if (out) ov[u] = reinterpret_cast<const uint4*>(out)[i];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long long i = base + u * kThreads + threadIdx.x;
      if (i >= n8) break;
      if (!FIXED) load_coef(static_cast<int>(i % cg) * 8);
      float g[8], yf[8];
      unpack8(gv[u], g);
      if (mask) {
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = (mb[u] >> j) & 1u ? g[j] : 0.f;
      } else if (out) {
        float o[8];
        unpack8(ov[u], o);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = o[j] > 0.f ? g[j] : 0.f;
      }
      unpack8(yv[u], yf);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = ca[j] * g[j] + cb[j] * yf[j] + cc[j];
      const uint4 packed = pack8(g);
      if (dz) reinterpret_cast<uint4*>(dz)[i] = packed;  // null: the e5m2 copy is the only consumer
      if (q8) {  // the stored bf16 values, scaled, saturated to the e5m2 range
        float fq[8];
        unpack8(packed, fq);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          qmax = fmaxf(qmax, fabsf(fq[j]));
          const float v = fminf(fmaxf(fq[j] * qs, -57344.f), 57344.f);
          const uint32_t b = static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_bf8_f32(v, v, 0, false) & 0xff);
          if (j < 4) lo |= b << (8 * j);
          else hi |= b << (8 * (j - 4));
        }
        reinterpret_cast<uint2*>(q8)[i] = make_uint2(lo, hi);
      }
    }
  }
  if (q8) {
    __shared__ float red[kThreads / 64];
    qmax = wave_max(qmax);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = qmax;
    __syncthreads();
    if (threadIdx.x == 0) {
      float m = red[0];
      for (int w = 1; w < kThreads / 64; ++w) m = fmaxf(m, red[w]);
      atomicMax(reinterpret_cast<unsigned int*>(q8_slot + 8 + (blockIdx.x & 63)), __float_as_uint(m));
    }
  }
}

inline int grid_for(long long n, int per_block = kThreads, int cap = 8192) {
  long long g = (n + per_block - 1) / per_block;
  return static_cast<int>(g < cap ? (g < 1 ? 1 : g) : cap);
}

}  // namespace
}  // namespace ttdk

using namespace ttdk;

// Number of partial rows ttdk_bn_stats_partial / ttdk_bn_bwd_partial will write.
TTDK_API(int, ttdk_bn_num_partials, (long long M, int C)) {
  const int cg = C >> 3;
  const int cols = cg < kThreads ? cg : kThreads;
  const int rlanes = kThreads / cols;
  long long want = (M + 16LL * rlanes - 1) / (16LL * rlanes);  // >= 16 rows per row-lane
  if (want > 2048) want = 2048;
  if (want < 1) want = 1;
  return static_cast<int>(want);
}

TTDK_API(int, ttdk_bn_stats_partial, (const bf16_t* x, long long M, int C, float* partial, int nblocks, hipStream_t st)) {
  if (C % 8) return hipErrorInvalidValue;
  const long long rpb = (M + nblocks - 1) / nblocks;
  hipLaunchKernelGGL(stats_partial_kernel, dim3(nblocks), dim3(kThreads), 0, st, x, M, C, partial, rpb);
  return hipGetLastError();
}

// ReLU mask source: `mask` (1 bit per element, written by ttdk_bn_apply) if given, else `out`.
TTDK_API(int, ttdk_bn_bwd_partial, (const bf16_t* dy, const bf16_t* out, const uint8_t* mask, const bf16_t* y,
                                    long long M, int C, float* partial, int nblocks, bf16_t* g_out, hipStream_t st)) {
  if (C % 8) return hipErrorInvalidValue;
  const long long rpb = (M + nblocks - 1) / nblocks;
  hipLaunchKernelGGL(bwd_partial_kernel, dim3(nblocks), dim3(kThreads), 0, st, dy, out, mask, y, M, C, partial, rpb,
                     g_out);
  return hipGetLastError();
}

// sums[2C] = sum of partial[T][2C] (sums is zeroed here).
TTDK_API(int, ttdk_bn_reduce_partials, (const float* partial, int T, int C, float* sums, hipStream_t st)) {
  const int C2 = 2 * C;
  hipError_t e = hipMemsetAsync(sums, 0, sizeof(float) * C2, st);
  if (e != hipSuccess) return e;
  int slices = (T + 63) / 64;
  if (slices > 64) slices = 64;
  const int per = (T + slices - 1) / slices;
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((C2 + 63) / 64, slices), dim3(kThreads), 0, st, partial, T, C2, sums,
                     per);
  return hipGetLastError();
}

TTDK_API(int, ttdk_bn_fwd_finalize, (const float* sums, float count, int C, const float* gamma, const float* beta,
                                     float eps, float momentum, float* running_mean, float* running_var,
                                     float* save_mean, float* save_rstd, float* scale, float* shift, hipStream_t st)) {
  hipLaunchKernelGGL(fwd_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, st, sums, count, C, gamma, beta, eps,
                     momentum, running_mean, running_var, save_mean, save_rstd, scale, shift);
  return hipGetLastError();
}

TTDK_API(int, ttdk_bn_bwd_finalize, (const float* sums, float count, int C, const float* gamma, const float* mean,
                                     const float* rstd, float* dgamma, float* dbeta, float* coef, int accumulate,
                                     hipStream_t st)) {
  hipLaunchKernelGGL(bwd_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, st, sums, count, C, gamma, mean, rstd,
                     dgamma, dbeta, coef, accumulate);
  return hipGetLastError();
}

// q8/q8_slot (optional): also write an fp8 e4m3 copy of `out` (delayed scaling, see fp8.hip).
TTDK_API(int, ttdk_bn_apply, (const bf16_t* y, const float* scale, const float* shift, const bf16_t* residual,
                              const float* rscale, const float* rshift, bf16_t* out, uint8_t* mask, uint8_t* q8,
                              float* q8_slot, long long n, int C, int relu, hipStream_t st)) {
  if (C % 8 || n % 8 || (q8 && !q8_slot) || (rscale && (!residual || !rshift)) || (!out && !q8)) return hipErrorInvalidValue;
  const long long n8 = n / 8;
  const int grid = grid_for(n8, kThreads * kUnroll);
  if (kThreads % (C >> 3) == 0)
    hipLaunchKernelGGL(apply_kernel<true>, dim3(grid), dim3(kThreads), 0, st, y, scale, shift, residual, rscale, rshift, out,
                       mask, q8, q8_slot, n8, C, relu);
  else
    hipLaunchKernelGGL(apply_kernel<false>, dim3(grid), dim3(kThreads), 0, st, y, scale, shift, residual, rscale, rshift, out,
                       mask, q8, q8_slot, n8, C, relu);
  return hipGetLastError();
}

TTDK_API(int, ttdk_bn_bwd_apply_q8, (const bf16_t* dy, const bf16_t* out, const uint8_t* mask, const bf16_t* y,
                                     const float* coef, bf16_t* dz, uint8_t* q8, float* q8_slot, long long n, int C,
                                     hipStream_t st)) {
  if (C % 8 || n % 8 || (q8 && !q8_slot) || (!dz && !q8)) return hipErrorInvalidValue;
  const long long n8 = n / 8;
  const int grid = grid_for(n8, kThreads * kUnroll);
  if (kThreads % (C >> 3) == 0)
    hipLaunchKernelGGL(bwd_apply_kernel<true>, dim3(grid), dim3(kThreads), 0, st, dy, out, mask, y, coef, dz, q8, q8_slot,
                       n8, C);
  else
    hipLaunchKernelGGL(bwd_apply_kernel<false>, dim3(grid), dim3(kThreads), 0, st, dy, out, mask, y, coef, dz, q8,
                       q8_slot, n8, C);
  return hipGetLastError();
}

TTDK_API(int, ttdk_bn_bwd_apply, (const bf16_t* dy, const bf16_t* out, const uint8_t* mask, const bf16_t* y,
                                  const float* coef, bf16_t* dz, long long n, int C, hipStream_t st)) {
  return ttdk_bn_bwd_apply_q8(dy, out, mask, y, coef, dz, nullptr, nullptr, n, C, st);
}

// Slab rows (slices) ttdk_bn_reduce_finalize uses for T partial rows: the caller provides a
// slab of slices*2*C floats.
TTDK_API(int, ttdk_bn_finalize_slices, (int T)) {
  int s = (T + 31) / 32;
  return s < 1 ? 1 : (s > 256 ? 256 : s);
}

// bwd == 0: mean/rstd/scale/shift (+ running stats) from the fwd partials;
// bwd == 1: dgamma/dbeta/coef from the bwd partials (mean/rstd inputs).
TTDK_API(int, ttdk_bn_reduce_finalize, (const float* partial, int T, int C, float* slab, int bwd, float count,
                                        const float* gamma, const float* beta, float eps, float momentum,
                                        float* running_mean, float* running_var, float* mean, float* rstd,
                                        float* scale, float* shift, float* dgamma, float* dbeta, float* coef,
                                        int accumulate, hipStream_t st)) {
  const int S = ttdk_bn_finalize_slices(T);
  const int per = (T + S - 1) / S;
  FinalizeArgs a{count, gamma, beta, eps, momentum, running_mean, running_var, mean, rstd, scale, shift,
                 dgamma, dbeta, coef, accumulate};
  const int cgr = (C + 31) / 32;
  if (T <= 256) {
    // few partial rows (persistent producers, small layers): the finalize folds them directly,
    // in the same fixed order, one launch instead of two
    if (bwd)
      hipLaunchKernelGGL(finalize_kernel<true>, dim3(cgr), dim3(kThreads), 0, st, partial, T, C, a);
    else
      hipLaunchKernelGGL(finalize_kernel<false>, dim3(cgr), dim3(kThreads), 0, st, partial, T, C, a);
    return hipGetLastError();
  }
  // (a 16-B-load variant, 16 threads x 4 channels per partial row, measured 0.8 ms/step SLOWER in
  // the ResNet-50 step, 68.76 / 68.55 vs 67.94 / 67.69 ms: these folds are latency-bound next to the
  // side stream; the 32-channel scalar version stays)
  hipLaunchKernelGGL(reduce_slices_kernel, dim3(cgr, S), dim3(kThreads), 0, st, partial, T, C, per, slab);
  if (bwd)
    hipLaunchKernelGGL(finalize_kernel<true>, dim3(cgr), dim3(kThreads), 0, st, slab, S, C, a);
  else
    hipLaunchKernelGGL(finalize_kernel<false>, dim3(cgr), dim3(kThreads), 0, st, slab, S, C, a);
  return hipGetLastError();
}
