// Grouped ("ragged") matmul for mixture-of-experts feed-forward blocks on gfx950 MFMA
// (v_mfma_f32_16x16x32_bf16): one launch over rows sorted by expert, group boundaries read on the
// device, so a step neither syncs with the host nor changes shape under a captured hipGraph.
//
//   ttdk_grouped_gemm   y[r, :] = x[r, :] @ w[e(r)]      x bf16 [M, K] (row stride ldx),
//                       w bf16 [E, K, N], y bf16 [M, N] (row stride ldy). The data gradient
//                       dx = dy @ w[e]^T runs the same kernel on a transposed copy of the weights:
//                       the form that reads w as [E, N, K] is not in this file (see below).
//   ttdk_grouped_wgrad  dw[e] = x[rows_e]^T @ dy[rows_e]  fp32 [E, K, N], written for every group
//                       (zeros for an empty one).
//   offsets int32 [E + 1] in device memory; group e owns rows [offsets[e], offsets[e + 1]), rows at
//   or past offsets[E] belong to no group and get zero rows of y. The table is data, not trusted:
//   boundary 0 is taken as 0 and boundary i as min(M, max(0, offsets[1..i])) — every boundary
//   clamped into [previous boundary, M] — so a bad table gives wrong numbers, never an access
//   outside the buffers.
//
// How the work is split. The operand loaders, the LDS images (kmaj_off / mnmaj_off: conflict-free
// b128 row reads and ds_read_b64_tr_b16 column reads) and the 4-wave 2x2 MFMA loop with global ->
// register -> LDS double buffering are the GEMM engine's (gemm_conv.h); what is here is the cut of
// M at run-time boundaries.
//  * forward / data gradient: the grid is sized from shapes alone. With the rows of no group as
//    pseudo-group E there are sum_e ceil(m_e / 128) <= (M + (E + 1) * 127) / 128 row tiles; the grid
//    is that bound times the column tiles, row tile fastest (the row tiles of a group share one
//    128-column panel of w[e] in an XCD's L2; xcd_remap keeps neighbours on one XCD). Every wave of
//    a workgroup finds its (group, tile in group) itself, 64 groups per step: a wave-wide prefix
//    max of the boundaries (the clamp), the per-group tile counts, a wave-wide prefix sum of those,
//    and a ballot for the first group whose running total passes the row tile. Workgroups past the
//    total exit. A row tile never spans two groups: the A loader zero-fills rows past the group's
//    end and the epilogue never stores them. Tiles of pseudo-group E store zeros and load nothing.
//  * weight gradient: one workgroup per (group, 128 x 128 tile of dw[e]), k tile fastest. The
//    reduction runs over the group's rows in 64-row steps from the group's first row (any row:
//    rows are 16-byte aligned by ld % 8, nothing more is needed), both operands MN-major through
//    the transposing LDS reads, the last step masked by the loaders' k < m_e test; m_e = 0 runs no
//    step and stores the zero accumulators. One workgroup owns a tile's whole reduction in row
//    order: no float atomics, no workspace, bitwise repeatable. A long group's reduction is NOT
//    split over workgroups: E * ceil(K / 128) * ceil(N / 128) tiles are >= 11000 at
//    mixture-of-experts shapes (E = 8, K = 4096, N = 14336; E = 64, K = 2048, N = 1408), 20 times
//    the 512 workgroups the device holds, so a skewed table costs a tail, not idle CUs. A split
//    through a workspace and ttdk_colreduce was not built; neither form's speed is measured.
//
// Tile: 128 x 128, BK = 64, 256 threads, two workgroups per CU — not the 256 x 256 AGPR tile of
// gemm4w. m_e is a few hundred to a few thousand rows and every group ends in a partial tile: the
// MFMA work wasted on zero rows averages half a tile per group, 64 rows against 128, and at the
// fine-grained shape (m_e = 768) that is 8 % against 17 %; the grid bound overshoots by E tiles of
// either size; and the register-staged loaders zero-fill ragged rows for free where gemm4w's
// LDS-DMA loader would need a separate path. Two workgroups per CU also hide one's epilogue and
// group search behind the other's MFMA loop.
//
// Registers, LDS and occupancy as compiled (-Rpass-analysis=kernel-resource-usage; every launched
// instantiation 0 bytes of scratch):
//   kernel                          VGPR  AGPR  LDS bytes  waves / SIMD  workgroups / CU
//   grouped_gemm                    167   0     65536      2             2 (LDS 128 of 160 KB)
//   grouped_wgrad                   168   0     65536      2             2
// Speed: not measured. Left out: a K-major weight form ([E, N, K], x @ w[e]^T without the copy)
// and a benchmark against the per-expert loop and a padded bmm; a GPU run of the benchmark's data
// gradient comparison at E = 8, K = 14336, N = 4096, M = 16384 ended in an illegal memory access
// whose cause was not found among the three paths it had in flight (that form, the loop over
// ops.gemm.gemm, torch.bmm), so neither is part of this file's change.
#include "gemm_conv.h"

namespace ttdk {
namespace {

constexpr int GBM = 128, GBN = 128;
constexpr int kMaxGroups = 1024;          // E above this is refused
constexpr int kMaxRows = 1 << 30;         // keeps every boundary + tile size inside int32

using XRows = KDense<GBM>;                // x rows, K-major
using WNmaj = MNDense<GBN>;               // w [E, K, N]
using TCols = MNDense<GBM>;               // wgrad operands: element (row of the group, column)

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Row tile rt -> (group, clamped [lo, hi) of the group, tile index in the group); false past the
// total. Group E is the rows of no group, [boundary E, M). Every lane of the wave gets the same
// answer. 64 groups per step; carry_b / carry_t hand the last boundary and the tile total on.
__device__ __forceinline__ bool find_tile(const int* __restrict__ off, int E, int M, int rt, int lane, int& grp,
                                          int& lo, int& hi, int& tin) {
  int carry_b = 0, carry_t = 0;
  for (int e0 = 0; e0 <= E; e0 += kWave) {
    const int e = e0 + lane;
    int b = max(e < E ? off[e + 1] : M, carry_b);  // upper boundary of group e (groups > E: empty at M)
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int v = __shfl_up(b, o, kWave);
      if (lane >= o) b = max(b, v);
    }
    b = min(b, M);
    int l = __shfl_up(b, 1, kWave);
    if (lane == 0) l = carry_b;
    const int nt = (b - l + GBM - 1) / GBM;
    int ps = nt;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int v = __shfl_up(ps, o, kWave);
      if (lane >= o) ps += v;
    }
    const int total = __shfl(ps, kWave - 1, kWave);
    if (rt < carry_t + total) {
      const int idx = __ffsll(static_cast<long long>(__ballot(carry_t + ps > rt))) - 1;
      grp = uniform(e0 + idx);
      lo = uniform(__shfl(l, idx, kWave));
      hi = uniform(__shfl(b, idx, kWave));
      tin = uniform(rt - (carry_t + __shfl(ps - nt, idx, kWave)));
      return true;
    }
    carry_t += total;
    carry_b = __shfl(b, kWave - 1, kWave);
  }
  return false;
}

// Clamped rows [lo, hi) of group e alone (the weight gradient's workgroups know their group).
__device__ __forceinline__ void group_rows(const int* __restrict__ off, int e, int M, int lane, int& lo, int& hi) {
  int mx = 0;
  for (int i = 1 + lane; i <= e; i += kWave) mx = max(mx, off[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, kWave));
  lo = uniform(min(mx, M));
  hi = uniform(min(max(lo, off[e + 1]), M));
}

// The engine's main loop (gemm_conv.h gemm_kernel) over ksteps 64-deep steps: loads of step k + 1
// issued before the MFMAs of step k, their LDS stores after, one barrier per step. Operands are
// swapped in the MFMA so that a lane holds 4 consecutive output columns of one row.
template <class LA, class LB>
__device__ __forceinline__ void mfma_loop(LA& la, LB& lb, char* smem, int ksteps, int tid,
                                          f32x4_t (&acc)[GBM / 32][GBN / 32]) {
  constexpr int TM = GBM / 32, TN = GBN / 32;
  const int lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  char* const sA0 = smem;
  char* const sB0 = smem + 2 * LA::BYTES;
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  if (ksteps > 0) {
    la.load(0);
    lb.load(0);
    la.store(sA0, tid);
    lb.store(sB0, tid);
  }
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < ksteps; ++kt) {
    const bool nxt = kt + 1 < ksteps;
    if (nxt) {
      la.load((kt + 1) * BK);
      lb.load((kt + 1) * BK);
    }
    const char* sa = sA0 + cur * LA::BYTES;
    const char* sb = sB0 + cur * LB::BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t af[TM], bfr[TN];
#pragma unroll
      for (int a = 0; a < TM; ++a) af[a] = LA::frag(sa, wm * (GBM / 2) + a * 16, ks, lane);
#pragma unroll
      for (int b = 0; b < TN; ++b) bfr[b] = LB::frag(sb, wn * (GBN / 2) + b * 16, ks, lane);
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[b], af[a], acc[a][b], 0, 0, 0);
    }
    if (nxt) {
      la.store(sA0 + (cur ^ 1) * LA::BYTES, tid);
      lb.store(sB0 + (cur ^ 1) * LB::BYTES, tid);
    }
    __syncthreads();
    cur ^= 1;
  }
}

__global__ __launch_bounds__(NTHR, 2) void grouped_gemm_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                              const bf16_t* __restrict__ w,
                                                              const int* __restrict__ off, bf16_t* __restrict__ y,
                                                              long long ldy, int M, int N, int K, int E,
                                                              int row_tiles) {
  __shared__ __attribute__((aligned(16))) char smem[2 * (XRows::BYTES + WNmaj::BYTES)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int n0 = (item / row_tiles) * GBN;
  int grp, lo, hi, tin;
  if (!find_tile(off, E, M, item % row_tiles, lane, grp, lo, hi, tin)) return;
  const int row0 = tin * GBM;            // first row of the tile, relative to lo
  const int rows = hi - lo;              // rows of the group
  constexpr int CPR = GBN / 8;           // 16-byte chunks per output row
  constexpr int RPP = NTHR / CPR;        // output rows per pass
  const int oc = tid % CPR, orow = tid / CPR;
  const bool cin = n0 + oc * 8 < N;      // N % 8 == 0: a chunk is inside or outside as a whole
  bf16_t* const yp = y + static_cast<long long>(lo + row0) * ldy + n0 + oc * 8;
  if (grp == E) {  // rows of no group: zeros
    for (int r = orow; r < GBM; r += RPP)
      if (cin && row0 + r < rows) *reinterpret_cast<uint4*>(yp + r * ldy) = make_uint4(0, 0, 0, 0);
    return;
  }
  XRows la;
  WNmaj lb;
  la.init(DenseParams{x + static_cast<long long>(lo) * ldx, ldx, rows, K}, row0, tid);
  const bf16_t* const we = w + static_cast<long long>(grp) * K * N;
  lb.init(DenseParams{we, N, N, K}, n0, tid);
  f32x4_t acc[GBM / 32][GBN / 32];
  mfma_loop(la, lb, smem, (K + BK - 1) / BK, tid, acc);
  // the loop ended on a barrier: stage the tile through the operand buffers so that every thread
  // stores whole 16-byte chunks of full rows (the engine's bf16 epilogue)
  constexpr int PITCH = GBN * 2 + 16;
  static_assert(GBM * PITCH <= 2 * (XRows::BYTES + WNmaj::BYTES), "staged tile must fit in LDS");
  const int wave = tid >> 6, wm = wave >> 1, wn = wave & 1, g = lane >> 4, i16 = lane & 15;
#pragma unroll
  for (int a = 0; a < GBM / 32; ++a)
#pragma unroll
    for (int b = 0; b < GBN / 32; ++b) {
      const int r = wm * (GBM / 2) + a * 16 + i16, c = wn * (GBN / 2) + b * 16 + 4 * g;
      uint2 v;
      v.x = pack_bf16x2(acc[a][b][0], acc[a][b][1]);
      v.y = pack_bf16x2(acc[a][b][2], acc[a][b][3]);
      *reinterpret_cast<uint2*>(smem + r * PITCH + c * 2) = v;
    }
  __syncthreads();
#pragma unroll
  for (int r = orow; r < GBM; r += RPP)
    if (cin && row0 + r < rows)
      *reinterpret_cast<uint4*>(yp + r * ldy) = *reinterpret_cast<const uint4*>(smem + r * PITCH + oc * 16);
}

__global__ __launch_bounds__(NTHR, 2) void grouped_wgrad_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                               const bf16_t* __restrict__ dy, long long lddy,
                                                               const int* __restrict__ off,
                                                               float* __restrict__ dw, int M, int N, int K,
                                                               int tiles_k, int tiles_n) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TCols::BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int k0 = (item % tiles_k) * GBM;
  const int rest = item / tiles_k;
  const int n0 = (rest % tiles_n) * GBN, e = rest / tiles_n;
  int lo, hi;
  group_rows(off, e, M, lane, lo, hi);
  const int me = hi - lo;  // reduction length
  TCols la, lb;
  la.init(DenseParams{x + static_cast<long long>(lo) * ldx, ldx, K, me}, k0, tid);
  lb.init(DenseParams{dy + static_cast<long long>(lo) * lddy, lddy, N, me}, n0, tid);
  f32x4_t acc[GBM / 32][GBN / 32];
  mfma_loop(la, lb, smem, (me + BK - 1) / BK, tid, acc);
  const int wave = tid >> 6, wm = wave >> 1, wn = wave & 1, g = lane >> 4, i16 = lane & 15;
  float* const out = dw + static_cast<long long>(e) * K * N;
#pragma unroll
  for (int a = 0; a < GBM / 32; ++a) {
    const int k = k0 + wm * (GBM / 2) + a * 16 + i16;
#pragma unroll
    for (int b = 0; b < GBN / 32; ++b) {
      const int n = n0 + wn * (GBN / 2) + b * 16 + 4 * g;  // N % 8 == 0: 4 columns inside or outside together
      if (k < K && n < N) *reinterpret_cast<f32x4_t*>(out + static_cast<long long>(k) * N + n) = acc[a][b];
    }
  }
}

inline bool shapes_ok(int M, int N, int K, int E) {
  return M >= 0 && M <= kMaxRows && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0 && E >= 1 && E <= kMaxGroups;
}

}  // namespace
}  // namespace ttdk

using namespace ttdk;

TTDK_API(int, ttdk_grouped_gemm_max_groups, ()) { return kMaxGroups; }

// y bf16 [M, N] = x [M, K] @ w[group of the row], w [E, K, N]; rows of no group are zeros.
// M == 0 succeeds without a launch.
TTDK_API(int, ttdk_grouped_gemm, (const void* x, long long ldx, const void* w, const int* offsets,
                                  void* y, long long ldy, int M, int N, int K, int E, hipStream_t st)) {
  if (!shapes_ok(M, N, K, E) || !w || !offsets || (M > 0 && (!x || !y))) return hipErrorInvalidValue;
  if (ldx < K || ldy < N || ldx % 8 || ldy % 8 || !al16(x) || !al16(w) || !al16(y) ||
      (reinterpret_cast<uintptr_t>(offsets) & 3))
    return hipErrorInvalidValue;
  if (M == 0) return hipSuccess;
  const long long row_tiles = (static_cast<long long>(M) + static_cast<long long>(E + 1) * (GBM - 1)) / GBM;
  const long long blocks = row_tiles * ceil_div(N, GBN);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const bf16_t* xb = static_cast<const bf16_t*>(x);
  const bf16_t* wb = static_cast<const bf16_t*>(w);
  bf16_t* yb = static_cast<bf16_t*>(y);
  hipLaunchKernelGGL(grouped_gemm_kernel, dim3(static_cast<unsigned>(blocks)), dim3(NTHR), 0, st, xb, ldx, wb, offsets,
                     yb, ldy, M, N, K, E, static_cast<int>(row_tiles));
  return hipGetLastError();
}

// dw fp32 [E, K, N] (contiguous) = per group x[rows]^T @ dy[rows]; x bf16 [M, K], dy bf16 [M, N].
// Every dw[e] is written (zeros for an empty group, and for all of them when M == 0).
TTDK_API(int, ttdk_grouped_wgrad, (const void* x, long long ldx, const void* dy, long long lddy, const int* offsets,
                                   float* dw, int M, int N, int K, int E, hipStream_t st)) {
  if (!shapes_ok(M, N, K, E) || !dw || !offsets || (M > 0 && (!x || !dy))) return hipErrorInvalidValue;
  if (ldx < K || lddy < N || ldx % 8 || lddy % 8 || !al16(x) || !al16(dy) || !al16(dw) ||
      (reinterpret_cast<uintptr_t>(offsets) & 3))
    return hipErrorInvalidValue;
  const int tiles_k = ceil_div(K, GBM), tiles_n = ceil_div(N, GBN);
  const long long blocks = static_cast<long long>(E) * tiles_k * tiles_n;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grouped_wgrad_kernel, dim3(static_cast<unsigned>(blocks)), dim3(NTHR), 0, st,
                     static_cast<const bf16_t*>(x), ldx, static_cast<const bf16_t*>(dy), lddy, offsets, dw, M, N, K,
                     tiles_k, tiles_n);
  return hipGetLastError();
}
