// Fused LM-head cross-entropy on gfx950 MFMA (v_mfma_f32_16x16x32_bf16): loss and gradients of
// softmax_cross_entropy(h @ w^T + bias, label) without a [T, V] logits tensor.
//
//   ttdk_linear_xent_fwd   h bf16 [T, H] (row stride ldh), w bf16 [V, H] (row stride ldw: an
//                          embedding table as it lies in memory, so both operands are K-major and
//                          nothing is transposed), bias fp32 [V] or null, labels int32 [T].
//                          Writes lse[T], loss[T] = lse - z[label], correct[T] (int32; TF's in_top_k
//                          at k = 1: the label's logit is finite and no logit is strictly greater).
//                          No logit is stored.
//   ttdk_linear_xent_grad  g[r, :] = (exp(z[r, :] - lse[r]) - onehot(label[r])) * dloss[r] for the
//                          rows [r0, r0 + rows), rounded to bf16 once, into a bf16 workspace
//                          [rows, V]. The caller multiplies the chunk by w and h (dh, dw, dbias) and
//                          hands the same workspace to the next chunk: the backward never holds
//                          more than one chunk of the logits' gradient.
//   A label outside [0, V) marks an ignored row: loss 0, correct 0, gradient row 0 (exactly).
//
// How the work is split. The operand loaders (KDense<128> for both operands), the kmaj_off LDS
// image and the 4-wave 2 x 2 MFMA loop with global -> register -> LDS double buffering are the GEMM
// engine's (gemm_conv.h), in the form grouped_gemm.hip uses: 128 x 128 tile, BK = 64, 256 threads,
// operands swapped in the MFMA so that a lane holds 4 consecutive columns of one row. What is here
// is what happens to a tile of logits once it sits in the accumulators.
//  * forward: the grid is row_tiles x splits. A workgroup owns 128 token rows and a contiguous
//    range of 128-column vocabulary tiles (tile ranges cut evenly, floor(sp * tiles / splits)), and
//    runs the whole K loop over H for each of them. After a tile every lane adds the bias, sets
//    columns >= V to -inf and merges the 16 logits it holds of each of its 4 rows into a running
//    (max, sum of exp(z - max)) that stays in registers over all the tiles of the range:
//    s = s * exp(m - m') + sum exp(z - m'), skipped while m' is still -inf (no -inf - -inf). The
//    lane that holds the label's column writes that logit to zt[row]; a column belongs to one
//    lane of one workgroup, so zt[row] has exactly one writer. Only after the last tile are the
//    lanes' pairs merged: across the four 16-lane groups of a wave by two cross-lane moves, across
//    the two column waves through LDS (the operand buffers, free by then), both in a fixed order,
//    and the row's (m, s) goes to an fp32 workspace [splits, T, 2]. The per-tile cost is 17 expf
//    per row and lane and no barrier beyond the K loop's. A fold kernel, one thread per row, merges
//    the splits in split order and writes lse, loss and correct. No atomics: every output is
//    bitwise the same on every run for a given number of splits.
//    The host picks splits from the shapes alone: about two workgroups on each of 256 CUs
//    (ceil(512 / row_tiles)), never more than the column tiles.
//  * gradient chunk: a plain row_tiles x col_tiles grid through xcd_remap, row tile fastest, so
//    that neighbours share a 128-row panel of w in an XCD's L2. The same loop and the same bias
//    add as the forward (tile_logits below), so a recomputed logit is the forward's bit for bit.
//    The tile is rounded to bf16 in registers, staged through the operand LDS and stored as whole
//    16-byte chunks of full rows (the engine's bf16 epilogue).
// The statistics use expf / logf: __expf's absolute error grows towards the ends of its range
// (it was what the router's softmax lost near -87), and a logit 80 below the maximum is ordinary
// here.
//
// Registers, LDS and occupancy as compiled (-Rpass-analysis=kernel-resource-usage; 0 bytes of
// scratch in every kernel):
//   kernel                          VGPR  AGPR  LDS bytes  waves / SIMD  workgroups / CU
//   linear_xent_fwd                 173   0     65536      2             2 (LDS 128 of 160 KB)
//   linear_xent_grad                150   0     65536      2             2
//   linear_xent_fold                16    0     0          8             -
// Speed: see profiles/linear_xent_bench.txt. Left out: label smoothing, z-loss, soft labels,
// fp32 / fp8 operands, V not a multiple of 8, and a single-kernel backward (the 128 x H fp32 dh
// tile does not fit a workgroup's registers at H >= 512).
#include "gemm_conv.h"

#include <cmath>

namespace ttdk {
namespace {

constexpr int XBM = 128, XBN = 128;
constexpr int kTargetWgs = 512;           // two workgroups on each of 256 CUs
constexpr int kMaxRows = 1 << 30;         // keeps row + tile size and the grid inside int32

using HRows = KDense<XBM>;                // h rows, K-major
using WRows = KDense<XBN>;                // w rows (vocabulary entries), K-major

// The engine's main loop in grouped_gemm.hip's form: loads of step k + 1 issued before the MFMAs of
// step k, their LDS stores after, one barrier per step, ending on a barrier. Operands swapped:
// acc[a][b][j] is row wm * 64 + a * 16 + (lane & 15), column wn * 64 + b * 16 + 4 * (lane >> 4) + j.
__device__ __forceinline__ void mfma_loop(HRows& la, WRows& lb, char* smem, int ksteps, int tid,
                                          f32x4_t (&acc)[XBM / 32][XBN / 32]) {
  constexpr int TM = XBM / 32, TN = XBN / 32;
  const int lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  char* const sA0 = smem;
  char* const sB0 = smem + 2 * HRows::BYTES;
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  la.load(0);
  lb.load(0);
  la.store(sA0, tid);
  lb.store(sB0, tid);
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < ksteps; ++kt) {
    const bool nxt = kt + 1 < ksteps;
    if (nxt) {
      la.load((kt + 1) * BK);
      lb.load((kt + 1) * BK);
    }
    const char* sa = sA0 + cur * HRows::BYTES;
    const char* sb = sB0 + cur * WRows::BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t af[TM], bfr[TN];
#pragma unroll
      for (int a = 0; a < TM; ++a) af[a] = HRows::frag(sa, wm * (XBM / 2) + a * 16, ks, lane);
#pragma unroll
      for (int b = 0; b < TN; ++b) bfr[b] = WRows::frag(sb, wn * (XBN / 2) + b * 16, ks, lane);
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[b], af[a], acc[a][b], 0, 0, 0);
    }
    if (nxt) {
      la.store(sA0 + (cur ^ 1) * HRows::BYTES, tid);
      lb.store(sB0 + (cur ^ 1) * WRows::BYTES, tid);
    }
    __syncthreads();
    cur ^= 1;
  }
}

// One 128 x 128 tile of logits into acc: h @ w[n0 .. n0 + 128)^T + bias, columns >= V set to -inf.
// Both kernels form their logits here and nowhere else, which is what makes the gradient's logits
// the forward's bit for bit. cbase: the lane's first column, n0 + wn * 64 + 4 * (lane >> 4).
__device__ __forceinline__ void tile_logits(HRows& la, const bf16_t* __restrict__ w, long long ldw,
                                            const float* __restrict__ bias, int V, int H, int n0, int cbase,
                                            char* smem, int tid, f32x4_t (&acc)[XBM / 32][XBN / 32]) {
  WRows lb;
  lb.init(DenseParams{w, ldw, V, H}, n0, tid);
  mfma_loop(la, lb, smem, (H + BK - 1) / BK, tid, acc);
#pragma unroll
  for (int b = 0; b < XBN / 32; ++b) {
    const int c = cbase + b * 16;
    const bool cin = c < V;  // V % 8 == 0, c % 4 == 0: the lane's 4 columns are inside or outside together
    f32x4_t bv = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (bias != nullptr && cin) bv = *reinterpret_cast<const f32x4_t*>(bias + c);
#pragma unroll
    for (int a = 0; a < XBM / 32; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[a][b][j] = cin ? acc[a][b][j] + bv[j] : -INFINITY;
  }
}

// (m, s) <- (m, s) merged with (m2, s2): s counts exp(z - m). Two empty sets stay (-inf, 0).
__device__ __forceinline__ void merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  s = s * expf(m - mn) + s2 * expf(m2 - mn);
  m = mn;
}

__global__ __launch_bounds__(NTHR, 2) void linear_xent_fwd_kernel(const bf16_t* __restrict__ h, long long ldh,
                                                                 const bf16_t* __restrict__ w, long long ldw,
                                                                 const float* __restrict__ bias,
                                                                 const int* __restrict__ labels,
                                                                 float* __restrict__ part, float* __restrict__ zt,
                                                                 int T, int V, int H, int row_tiles, int col_tiles,
                                                                 int splits) {
  __shared__ __attribute__((aligned(16))) char smem[2 * (HRows::BYTES + WRows::BYTES)];
  constexpr int TM = XBM / 32, TN = XBN / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, i16 = lane & 15;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int rt = item % row_tiles, sp = item / row_tiles;
  const int ct0 = static_cast<int>(static_cast<long long>(sp) * col_tiles / splits);
  const int ct1 = static_cast<int>(static_cast<long long>(sp + 1) * col_tiles / splits);
  const int rbase = rt * XBM + wm * (XBM / 2) + i16;  // the lane's rows: rbase + a * 16
  HRows la;
  la.init(DenseParams{h, ldh, T, H}, rt * XBM, tid);
  int lab[TM];
  float m[TM], s[TM];
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int row = rbase + a * 16;
    const int l = row < T ? labels[row] : -1;
    lab[a] = (l >= 0 && l < V) ? l : -1;  // -1: no column matches
    m[a] = -INFINITY;
    s[a] = 0.f;
  }
  f32x4_t acc[TM][TN];
  for (int ct = ct0; ct < ct1; ++ct) {
    const int cbase = ct * XBN + wn * (XBN / 2) + 4 * g;
    tile_logits(la, w, ldw, bias, V, H, ct * XBN, cbase, smem, tid, acc);
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      float tm = -INFINITY, zl = 0.f;
      bool hit = false;
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float z = acc[a][b][j];
          tm = fmaxf(tm, z);
          if (cbase + b * 16 + j == lab[a]) {
            hit = true;
            zl = z;
          }
        }
      if (hit) zt[rbase + a * 16] = zl;
      const float mn = fmaxf(m[a], tm);
      if (mn != -INFINITY) {
        float sum = 0.f;
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
          for (int j = 0; j < 4; ++j) sum += expf(acc[a][b][j] - mn);
        s[a] = s[a] * expf(m[a] - mn) + sum;
        m[a] = mn;
      }
    }
  }
  // the four 16-lane groups of a wave hold the other columns of the same rows
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int o = 16; o < kWave; o <<= 1) {
      const float m2 = __shfl_xor(m[a], o, kWave), s2 = __shfl_xor(s[a], o, kWave);
      merge(m[a], s[a], m2, s2);
    }
  // the column waves: wn = 1 hands its rows over through LDS (the K loop ended on a barrier)
  float2* const xch = reinterpret_cast<float2*>(smem);
  if (wn == 1 && g == 0) {
#pragma unroll
    for (int a = 0; a < TM; ++a) xch[wm * (XBM / 2) + a * 16 + i16] = make_float2(m[a], s[a]);
  }
  __syncthreads();
  if (wn == 0 && g == 0) {
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      const int row = rbase + a * 16;
      const float2 o = xch[wm * (XBM / 2) + a * 16 + i16];
      merge(m[a], s[a], o.x, o.y);
      if (row < T)
        *reinterpret_cast<float2*>(part + (static_cast<long long>(sp) * T + row) * 2) = make_float2(m[a], s[a]);
    }
  }
}

__global__ __launch_bounds__(256) void linear_xent_fold_kernel(const float* __restrict__ part,
                                                              const float* __restrict__ zt,
                                                              const int* __restrict__ labels, float* __restrict__ lse,
                                                              float* __restrict__ loss, int* __restrict__ correct,
                                                              int T, int V, int splits) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= T) return;
  float m = -INFINITY, s = 0.f;
  for (int sp = 0; sp < splits; ++sp) {
    const float2 p = *reinterpret_cast<const float2*>(part + (static_cast<long long>(sp) * T + row) * 2);
    merge(m, s, p.x, p.y);
  }
  const float l = m + logf(s);
  lse[row] = l;
  const int lb = labels[row];
  if (lb >= 0 && lb < V) {
    const float z = zt[row];
    loss[row] = l - z;
    correct[row] = (fabsf(z) < INFINITY && z >= m) ? 1 : 0;
  } else {
    loss[row] = 0.f;
    correct[row] = 0;
  }
}

// h, labels, lse, dloss and g all start at the chunk's first row; rows: rows of the chunk.
__global__ __launch_bounds__(NTHR, 2) void linear_xent_grad_kernel(const bf16_t* __restrict__ h, long long ldh,
                                                                  const bf16_t* __restrict__ w, long long ldw,
                                                                  const float* __restrict__ bias,
                                                                  const int* __restrict__ labels,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ dloss,
                                                                  bf16_t* __restrict__ gout, int rows, int V, int H,
                                                                  int row_tiles) {
  __shared__ __attribute__((aligned(16))) char smem[2 * (HRows::BYTES + WRows::BYTES)];
  constexpr int TM = XBM / 32, TN = XBN / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, i16 = lane & 15;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int row0 = (item % row_tiles) * XBM, n0 = (item / row_tiles) * XBN;
  const int cbase = n0 + wn * (XBN / 2) + 4 * g;
  HRows la;
  la.init(DenseParams{h, ldh, rows, H}, row0, tid);
  f32x4_t acc[TM][TN];
  tile_logits(la, w, ldw, bias, V, H, n0, cbase, smem, tid, acc);
  // the loop ended on a barrier: stage the tile through the operand buffers so that every thread
  // stores whole 16-byte chunks of full rows
  constexpr int PITCH = XBN * 2 + 16;
  static_assert(XBM * PITCH <= 2 * (HRows::BYTES + WRows::BYTES), "staged tile must fit in LDS");
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int r = wm * (XBM / 2) + a * 16 + i16;
    const bool rin = row0 + r < rows;
    const int l = rin ? labels[row0 + r] : -1;
    const bool valid = l >= 0 && l < V;
    const float le = valid ? lse[row0 + r] : 0.f;
    const float d = valid ? dloss[row0 + r] : 0.f;
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = expf(acc[a][b][j] - le) - (cbase + b * 16 + j == l ? 1.f : 0.f);
        v[j] = valid ? p * d : 0.f;
      }
      uint2 pk;
      pk.x = pack_bf16x2(v[0], v[1]);
      pk.y = pack_bf16x2(v[2], v[3]);
      *reinterpret_cast<uint2*>(smem + r * PITCH + (wn * (XBN / 2) + b * 16 + 4 * g) * 2) = pk;
    }
  }
  __syncthreads();
  constexpr int CPR = XBN / 8;           // 16-byte chunks per output row
  constexpr int RPP = NTHR / CPR;        // output rows per pass
  const int oc = tid % CPR, orow = tid / CPR;
  const bool cin = n0 + oc * 8 < V;      // V % 8 == 0: a chunk is inside or outside as a whole
  bf16_t* const gp = gout + static_cast<long long>(row0) * V + n0 + oc * 8;
#pragma unroll
  for (int r = orow; r < XBM; r += RPP)
    if (cin && row0 + r < rows)
      *reinterpret_cast<uint4*>(gp + static_cast<long long>(r) * V) =
          *reinterpret_cast<const uint4*>(smem + r * PITCH + oc * 16);
}

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

inline int default_splits(int T, int V) {
  const int row_tiles = ceil_div(T, XBM), col_tiles = ceil_div(V, XBN);
  return std::max(1, std::min(col_tiles, ceil_div(kTargetWgs, row_tiles)));
}

// what both entry points ask of the operands
inline bool operands_ok(const void* h, long long ldh, const void* w, long long ldw, const void* bias,
                        const void* labels, int T, int V, int H) {
  if (T <= 0 || T > kMaxRows || V < 8 || V % 8 || H < 8 || H % 8) return false;
  if (ldh < H || ldw < H || ldh % 8 || ldw % 8) return false;
  if (!h || !w || !labels || !al16(h) || !al16(w) || !al16(bias) || !al4(labels)) return false;
  return true;
}

}  // namespace
}  // namespace ttdk

using namespace ttdk;

// The number of splits the forward runs when the caller has no wish of its own (from shapes alone).
TTDK_API(int, ttdk_linear_xent_splits, (int T, int V)) {
  if (T <= 0 || T > kMaxRows || V < 8) return -1;
  return default_splits(T, V);
}

// Floats of forward workspace ([splits, T, 2]) for splits in [1, column tiles]; -1 otherwise.
TTDK_API(long long, ttdk_linear_xent_ws_floats, (int T, int V, int splits)) {
  if (T <= 0 || T > kMaxRows || V < 8 || splits < 1 || splits > ceil_div(V, XBN)) return -1;
  return 2LL * splits * T;
}

TTDK_API(int, ttdk_linear_xent_fwd, (const void* h, long long ldh, const void* w, long long ldw, const float* bias,
                                     const int* labels, float* ws, float* zt, float* lse, float* loss, int* correct,
                                     int T, int V, int H, int splits, hipStream_t st)) {
  if (!operands_ok(h, ldh, w, ldw, bias, labels, T, V, H)) return hipErrorInvalidValue;
  const int row_tiles = ceil_div(T, XBM), col_tiles = ceil_div(V, XBN);
  if (splits < 1 || splits > col_tiles) return hipErrorInvalidValue;
  if (!ws || !zt || !lse || !loss || !correct || (reinterpret_cast<uintptr_t>(ws) & 7) || !al4(zt) || !al4(lse) ||
      !al4(loss) || !al4(correct))
    return hipErrorInvalidValue;
  const long long blocks = static_cast<long long>(row_tiles) * splits;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(linear_xent_fwd_kernel, dim3(static_cast<unsigned>(blocks)), dim3(NTHR), 0, st,
                     static_cast<const bf16_t*>(h), ldh, static_cast<const bf16_t*>(w), ldw, bias, labels, ws, zt, T, V,
                     H, row_tiles, col_tiles, splits);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(linear_xent_fold_kernel, dim3(ceil_div(T, 256)), dim3(256), 0, st, ws, zt, labels, lse, loss,
                     correct, T, V, splits);
  return hipGetLastError();
}

// g bf16 [rows, V] (contiguous) for the rows [r0, r0 + rows) of the T the other pointers describe.
TTDK_API(int, ttdk_linear_xent_grad, (const void* h, long long ldh, const void* w, long long ldw, const float* bias,
                                      const int* labels, const float* lse, const float* dloss, void* g, int T, int r0,
                                      int rows, int V, int H, hipStream_t st)) {
  if (!operands_ok(h, ldh, w, ldw, bias, labels, T, V, H)) return hipErrorInvalidValue;
  if (r0 < 0 || rows <= 0 || rows > T - r0) return hipErrorInvalidValue;
  if (!lse || !dloss || !g || !al4(lse) || !al4(dloss) || !al16(g)) return hipErrorInvalidValue;
  const int row_tiles = ceil_div(rows, XBM);
  const long long blocks = static_cast<long long>(row_tiles) * ceil_div(V, XBN);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(linear_xent_grad_kernel, dim3(static_cast<unsigned>(blocks)), dim3(NTHR), 0, st,
                     static_cast<const bf16_t*>(h) + static_cast<long long>(r0) * ldh, ldh,
                     static_cast<const bf16_t*>(w), ldw, bias, labels + r0, lse + r0, dloss + r0,
                     static_cast<bf16_t*>(g), rows, V, H, row_tiles);
  return hipGetLastError();
}
