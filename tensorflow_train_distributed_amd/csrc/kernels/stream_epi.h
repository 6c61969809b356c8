// Epilogue pieces shared by the persistent streaming conv kernels (pw_gemm.hip, conv3_halo.hip):
// accumulators of v_mfma_f32_16x16x32_bf16 with swapped operands (D = B.A^T, so each lane holds
// 4 consecutive output columns of one row) staged to LDS as bf16 rows, and the per-tile
// reduction of the BatchNorm partial statistics gathered by epi_rows (gemm_conv.h).
#pragma once

#include "gemm_conv.h"

namespace ttdk {
namespace {
namespace sepi {

// acc[a][c] is the 16x16 block (rows wm*WR + a*16.., cols wn*WC + c*16..) of the tile
template <int TM, int TN, int WR, int WC, int PITCH>
__device__ __forceinline__ void stage_acc(char* sS, const f32x4_t (&acc)[TM][TN], int wm, int wn, int lane,
                                          float alpha) {
  const int gq4 = lane >> 4, i16 = lane & 15;
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int c = 0; c < TN; ++c) {
      const int r = wm * WR + a * 16 + i16, cc = wn * WC + c * 16 + 4 * gq4;
      const f32x4_t v = acc[a][c] * alpha;
      *reinterpret_cast<uint2*>(sS + r * PITCH + cc * 2) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
}

// Fold the per-thread column sums (thread owns 16-B chunk c of every RPP-th row) into one
// [2][N] row of E.stat (and E.stat2) for tile t. `red` needs NW*3*BN floats of LDS. Ends with
// the block synchronised.
template <int BN, int NW, int THR, int ECPR>
__device__ __forceinline__ void tile_stats(const EpiParams& E, float* red, float (&s8)[8], float (&q8)[8],
                                           float (&r8)[8], int c, int lane, int wave, int tid, int n0, int N, long long t) {
  static_assert(ECPR <= 64, "one chunk column per lane group");
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int o = ECPR; o < 64; o <<= 1) {
      s8[j] += __shfl_xor(s8[j], o, 64);
      q8[j] += __shfl_xor(q8[j], o, 64);
      if (E.stat2) r8[j] += __shfl_xor(r8[j], o, 64);
    }
  }
  if (lane < ECPR) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[(wave * 3 + 0) * BN + c * 8 + j] = s8[j];
      red[(wave * 3 + 1) * BN + c * 8 + j] = q8[j];
      red[(wave * 3 + 2) * BN + c * 8 + j] = r8[j];
    }
  }
  __syncthreads();
  for (int t2 = tid; t2 < BN; t2 += THR) {
    if (n0 + t2 < N) {
      float ss = 0.f, qq = 0.f, rr = 0.f;
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        ss += red[(k * 3 + 0) * BN + t2];
        qq += red[(k * 3 + 1) * BN + t2];
        rr += red[(k * 3 + 2) * BN + t2];
      }
      E.stat[(t * 2 + 0) * N + n0 + t2] = ss;
      E.stat[(t * 2 + 1) * N + n0 + t2] = qq;
      if (E.stat2) {
        E.stat2[(t * 2 + 0) * N + n0 + t2] = ss;
        E.stat2[(t * 2 + 1) * N + n0 + t2] = rr;
      }
    }
  }
  __syncthreads();
}

// ---- prefetched feeding-BN epilogue of the halo kernels (conv3_halo.hip): the data gradient that
// stores g = bf16(acc) * mask and gathers the consuming BN's backward sums (sum g, sum g*y), with
// by (+ bmask) set and no bias / residual / beta / aux / activation / remap / by2 (anything else
// keeps epi_rows). A thread owns 16-B chunk c of rows r0 + k*RPP, k < NR = ceil(BM / RPP) (7, or 4
// with a row guard). epi_rows<.., true, 2> walked them in `unroll 1` batches of two: four
// dependent round trips per tile, each waiting on its y and mask loads behind a 64-bit row
// multiply and the run-time epilogue flags. Here the y / mask rows, which do not depend on the
// accumulators, are loaded in two batches that the caller issues ahead of use: rows [0, FA) under
// the tap loop, rows [FA, NR) once the accumulators are dead, before the barrier that publishes
// the staged tile; the row loop then only reads LDS, selects, packs, stores and sums. Row
// addresses advance by a constant.
// Arithmetic, rounding and the per-thread order of the sums are those of epi_rows.
template <int NRW>
struct FeedBatch {
  uint4 y[NRW];
  uint32_t mb[NRW];
};

// Rows k0 .. k0 + NRW - 1 of the thread's rows (k0 a constant once the caller is unrolled).
// Always exactly two loads per row (a row outside the tile or the tensor, and an absent bmask,
// read the zero page): the stage-3 kernel counts them into its vmcnt waits.
template <int BM, int RPP, int NRW>
__device__ __forceinline__ void feed_batch_load(FeedBatch<NRW>& f, const EpiParams& E, int k0, int r0, int m0, int M,
                                                int n) {
  const long long o0 = static_cast<long long>(m0 + r0 + k0 * RPP) * E.ldo + n;
  const long long step = static_cast<long long>(RPP) * E.ldo;
  const bf16_t* yp = E.by + o0;
  const uint8_t* mp = E.bmask + (o0 >> 3);  // ldo % 8 == 0, n % 8 == 0 (checked by the caller)
#pragma unroll
  for (int u = 0; u < NRW; ++u) {
    const int r = r0 + (k0 + u) * RPP;
    const bool ok = r < BM && m0 + r < M;
    f.y[u] = ldg16(ok ? yp : reinterpret_cast<const bf16_t*>(big::g_zero));
    f.mb[u] = *((ok && E.bmask) ? mp : reinterpret_cast<const uint8_t*>(big::g_zero));  // (used only with bmask set)
    yp += step;
    mp += step >> 3;
  }
}

template <int BM, int RPP, int PITCH, int NRW>
__device__ __forceinline__ void feed_batch_rows(const FeedBatch<NRW>& f, const EpiParams& E, const char* smem, int k0,
                                                int c, int r0, int m0, int M, int n, float (&s8)[8], float (&q8)[8]) {
  const long long step = static_cast<long long>(RPP) * E.ldo;
  bf16_t* op = static_cast<bf16_t*>(E.out) + static_cast<long long>(m0 + r0 + k0 * RPP) * E.ldo + n;
  // the batch's staged rows first (r < BM stays inside the staged tile), then one row at a time:
  // left to itself the scheduler interleaves all rows of the tile and runs out of registers
  uint4 sv[NRW];
#pragma unroll
  for (int u = 0; u < NRW; ++u) {
    const int r = r0 + (k0 + u) * RPP;
    sv[u] = *reinterpret_cast<const uint4*>(smem + (r < BM ? r : r0) * PITCH + c * 16);
  }
#pragma unroll
  for (int u = 0; u < NRW; ++u, op += step) {
    __builtin_amdgcn_sched_barrier(0);
    const int r = r0 + (k0 + u) * RPP;
    if (r >= BM || m0 + r >= M) break;
    float v[8], yv[8];
    unpack8(sv[u], v);
    const uint32_t mb = E.bmask ? f.mb[u] : 0xffu;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] += 0.f;  // epi_rows adds its (absent) bias: -0 becomes +0 before the pack
      v[j] = (mb >> j) & 1u ? v[j] : 0.f;
    }
    const uint4 packed = pack8(v);
    *reinterpret_cast<uint4*>(op) = packed;
    unpack8(packed, v);  // statistics of the gradient actually stored
    unpack8(f.y[u], yv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s8[j] += v[j];
      q8[j] += v[j] * yv[j];
    }
  }
}

// the case above, from the epilogue flags alone (the host picks the kernel by it)
inline bool feed_case(const EpiParams& E) {
  return E.by && !E.by2 && !E.bias && !E.residual && !E.beta && !E.aux && E.act == kActNone && !E.remap &&
         (E.ldo & 7) == 0;
}

}  // namespace sepi
}  // namespace
}  // namespace ttdk
