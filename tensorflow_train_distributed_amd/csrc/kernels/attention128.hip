// Flash attention forward and backward for head_dim 128 on gfx950 MFMA (v_mfma_f32_16x16x32_bf16):
// the head size of the LLaMA / Mistral / Qwen decoder blocks. Same contract as attention.hip:
//   element (b, s, h, d) of Q/K/V/O/dQ/dK/dV at base + (b*S + s)*ld + h*128 + d (token-major, the
//   fused projection's own layout), lse2 / delta fp32 [B*H][S] in the log2 domain,
//   s2 = (q.k) * log2(e)/sqrt(128), P = exp2(s2 - lse2); per-batch key length, cross-attention
//   (Sk != Sq), CAUSAL (tiles above the diagonal are not streamed; rotated block order of
//   tile::causal_block), GQA (Hk != H) and DROP (the hash of tile_common.h on (seed, step, site,
//   b*H+h, query, key): ops.transformer.attention_keep_mask mirrors it for any head size).
//   No float atomics, no workspace: bwd_q stores delta on its way, bwd_kv runs after it and sums a
//   GQA group in head order in its accumulators.
// Not here (64-wide only): band masks, the fused single-kernel backward, the bwd_kv diagnostics.
//
// What the wider head changes. Per (query, key) pair the MFMA work doubles while the softmax work
// (exp2, hash, selects) stays, and every per-row register array over d doubles. The three kernels
// spend the register file differently:
//
//   fwd    128 query rows per workgroup, 32 per wave, 64-key K / V tiles double-buffered in LDS
//          through register staging. Per lane: Q fragments 32, O accumulators 64, one S tile 32,
//          staging 32. launch_bounds(256, 2): two waves per SIMD, LDS 64 KB, two workgroups per CU.
//   bwd_q  128 query rows per workgroup, 32 per wave. Q and dO fragments 64, dQ accumulators 64,
//          staging 32 leave room for S and dP of 32 keys only (16 + 16), so a 64-key tile runs as
//          two 32-key halves, each S/dP -> dS -> dQ += dS K; a half's S/dP registers are dead
//          before the next half's are written. launch_bounds(256, 2), LDS 64 KB.
//   bwd_kv 128 keys per workgroup, 32 per wave, 64-query tiles of Q / dO. dK^T and dV^T are 128
//          accumulator registers per lane and the K and V fragments 64 more; with S / dP of a tile
//          (64), staging (32) and the hashes this is past the 256 registers of two waves per SIMD.
//          The ways out were (a) one wave per SIMD with 512 registers, the accumulators in AGPRs,
//          (b) 64 keys per workgroup, (c) eight waves of 16 keys. (b) and (c) both halve the keys a
//          wave owns: every Q / dO fragment read from LDS then feeds half the MFMAs (1 KB of LDS
//          reads per MFMA instead of 0.5 KB — at 256 B / clk that alone is half of the MFMA rate),
//          keys k and k + 16 of a dropout pair land in different waves (one hash per probability
//          instead of one per two), and (b) also streams Q / dO from L2 twice as often. So (a):
//          launch_bounds(256, 1), the 64-wide kernel's wave layout, and the tile body in four
//          phases so that the one wave of a SIMD has independent VALU work (P / dS of one half)
//          beside its MFMA work (S / dP or dV / dK of the other half). LDS 65 KB, one workgroup per
//          CU. (b) and (c) were not built, so what (a) costs against them is not measured; the
//          kernel's time is below.
//
// Registers, LDS and occupancy as compiled (-Rpass-analysis=kernel-resource-usage; ranges over the 8
// launched instantiations [gqa][causal][drop] of each kernel; every one 0 bytes of scratch):
//   kernel   VGPR     AGPR     LDS bytes  waves / SIMD  workgroups / CU
//   fwd      242-255  0        65536      2             2 (LDS 128 of 160 KB)
//   bwd_q    245-252  0        65536      2             2
//   bwd_kv   198-256  182-204  66560      1             1 (registers)
// (the two GQA causal bwd_kv instantiations keep 89 / 94 SGPRs in VGPR lanes, not in scratch)
// Measured (profiles/attn_hd128_bench.txt: B = 16, S = 2048, causal, H = 16 against the 64-wide
// kernels at H = 32, the same FLOPs): fwd 486 us against 485 (p = 0.1: 489 against 541), bwd_q 529
// against 588, bwd_kv 788 against 654 — the one wave per SIMD costs bwd_kv 13-20 %, the whole
// backward is within 9 % of the 64-wide one either way.
//
// LDS images: [64 rows][128 bf16], 256-byte rows, 16-byte chunks swizzled by tile::off128 (bank
// arithmetic there, not profiled): b128 row reads and ds_read_b64_tr_b16 column reads both
// conflict-free, one copy of a tile serves both orientations.
#include "tile_common.h"

#include <initializer_list>
#include <type_traits>

namespace ttdk {
namespace {

using tile::causal_block;
using tile::mfma;
using tile::off128;
using tile::pack_frag;
using tile::rd_col128;
using tile::rd_row128;

constexpr int D = 128;
constexpr int KT = 64;    // keys (fwd / bwd_q) or queries (bwd_kv) per streamed tile
constexpr int QBLK = 128; // rows per workgroup
constexpr int TILE_BYTES = KT * D * 2;

struct Attn128Params {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  const bf16_t* o;
  const bf16_t* dout;
  long long ldq, ldk, ldv, ldo, lddo;
  bf16_t* out;   // fwd: O ; bwd_q: dQ ; bwd_kv: dK
  bf16_t* out2;  // bwd_kv: dV
  long long ld_out, ld_out2;
  float* lse;          // [B*H][S] log2 domain
  float* delta;        // [B*H][S]: written by bwd_q, read by bwd_kv
  const int* seqlen;   // [B] or null
  int B, H, S;         // S: query rows per batch
  int Sk;              // key rows per batch
  int Hk, G;           // key/value heads, G = H / Hk query heads to each
  float scale_log2;    // log2(e) / sqrt(128)
  float scale;         // 1 / sqrt(128)
  uint32_t drop_thr;
  float drop_scale;    // 1 / (1 - p)
  const long long* rng;
  uint32_t site;
  int order;           // causal block order: tile::causal_block
};

__device__ __forceinline__ uint4 ldg16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }

__device__ __forceinline__ bf16x8_t ldg_frag(const bf16_t* p) {
  return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(p));
}

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// 64 rows x 128 cols tile loader: thread t moves 16-byte chunk t & 15 of rows (t >> 4) + 16 j,
// j = 0..3 — the 16 lanes of a row write its 16 swizzled slots, every bank once. The lane's row /
// chunk offset is folded into its pointer once; per tile only the block-uniform row0 * ld is formed.
struct TileLoader {
  const bf16_t* lanep;
  long long ld;
  int r, c;
  uint4 v[4];
  __device__ __forceinline__ void init(const bf16_t* b, long long l, int tid) {
    ld = l;
    r = tid >> 4;
    c = tid & 15;
    lanep = b + static_cast<long long>(r) * l + c * 8;
  }
  __device__ __forceinline__ void load(int row0, int nrows) {
    const bf16_t* p = lanep + static_cast<long long>(row0) * ld;
    if (row0 + KT <= nrows) {  // block-uniform: whole tile in range
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ldg16(p + 16 * j * ld);
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = row0 + r + 16 * j < nrows ? ldg16(p + 16 * j * ld) : make_uint4(0, 0, 0, 0);
  }
  __device__ __forceinline__ void store(char* lds) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<uint4*>(lds + off128(r + 16 * j, c * 8)) = v[j];
  }
};

// ------------------------------------------------------------------------------ forward
// As the 64-wide forward: swapped QK^T (4 keys x 1 query per lane, so P feeds the PV MFMA without a
// shuffle), online softmax in registers with the lazy rescale, masked scores -inf before the row
// max. Per 64-key tile and wave: 32 MFMAs for S^T (4 key blocks x 2 query blocks x 4 d-steps) and
// 32 for O += P V (8 d-blocks x 2 query blocks x 2 key steps) against 128 exp2: half the
// elementwise work per MFMA of the 64-wide kernel.
template <bool DROP, bool CAUSAL, bool GQA>
__global__ __launch_bounds__(256, 2) void attn128_fwd_kernel(Attn128Params P) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE_BYTES];
  const int qblocks = P.S / QBLK;
  const int t = tile::xcd_remap(blockIdx.x, gridDim.x);
  const int bh = t / qblocks;
  int qblk = t - bh * qblocks;
  if constexpr (CAUSAL) qblk = causal_block(qblk, bh, qblocks, P.order, true);
  const int b = bh / P.H, h = bh - b * P.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int q0 = qblk * QBLK + wave * 32;
  const int len = P.seqlen ? min(P.seqlen[b], P.Sk) : P.Sk;
  const long long tok0 = static_cast<long long>(b) * P.S;    // query rows
  const long long tokk = static_cast<long long>(b) * P.Sk;   // key rows

  bf16x8_t qf[2][4];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      qf[qb][ks] = ldg_frag(P.q + (tok0 + q0 + qb * 16 + i16) * P.ldq + h * D + ks * 32 + g * 8);

  TileLoader lk, lv;
  const int hk = GQA ? h / P.G : h;  // the key/value head of query head h
  lk.init(P.k + tokk * P.ldk + hk * D, P.ldk, tid);
  lv.init(P.v + tokk * P.ldv + hk * D, P.ldv, tid);

  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
  f32x4_t o[2][8];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int db = 0; db < 8; ++db) o[qb][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const uint32_t key = DROP ? drop_key(P.rng, P.site) : 0u;
  int ntiles = (len + KT - 1) / KT;
  if constexpr (CAUSAL) ntiles = min(ntiles, 2 * qblk + 2);
  if (ntiles > 0) {
    lk.load(0, len);
    lv.load(0, len);
    lk.store(smem);
    lv.store(smem + TILE_BYTES);
  }
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < ntiles; ++kt) {
    const bool nxt = kt + 1 < ntiles;
    if (nxt) {
      lk.load((kt + 1) * KT, len);
      lv.load((kt + 1) * KT, len);
    }
    const char* sK = smem + cur * 2 * TILE_BYTES;
    const char* sV = sK + TILE_BYTES;
    // CAUSAL: every key of the tile lies above every row of this wave (wave-uniform): no work, but
    // the wave still moves its share of the next tile and meets the barrier
    if (!CAUSAL || kt * KT <= q0 + 31) {
      // ---- S^T tile: lane holds keys kb*16 + 4g + i for query qb*16 + i16
      f32x4_t s[2][4];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        s[0][kb] = s[1][kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bf16x8_t kf = rd_row128(sK, kb * 16 + i16, ks * 4 + g);
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) s[qb][kb] = mfma(kf, qf[qb][ks], s[qb][kb]);
        }
      }
      const int kbase = kt * KT;
      if (kbase + KT > len) {  // block-uniform: the last key tile of a padded sequence
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
          for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (kbase + kb * 16 + 4 * g + i >= len) s[qb][kb][i] = -INFINITY;
      }
      if constexpr (CAUSAL) {
        if (kbase + KT - 1 > q0) {
          // wave-uniform: the tile crosses this wave's diagonal; key > query <=> kb*16 + i - qb*16 >
          // qd = query - (kbase + 4g)
          const int qd = q0 + i16 - kbase - 4 * g;
#pragma unroll
          for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (kb * 16 + i - qb * 16 > qd) s[qb][kb][i] = -INFINITY;
        }
      }
      bf16x8_t pf[2][2];
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        // max over the raw scores (scale > 0 commutes with max); the scale rides in the exp2 FMA
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[qb][kb][i]);
        mx = tile::rows4_max(mx);
        // lazy rescale: the running max moves, and the 32 O registers of the row are rescaled, only
        // when some row of the wave saw its max grow by more than 8 (log2 units): P stays below 2^8
        const float mxs = mx * P.scale_log2;
        float alpha = 1.f;
        const bool grow = mxs > m[qb] + 8.f;
        if (__builtin_amdgcn_ballot_w64(grow) != 0) {
          // per row: a row whose max did not grow keeps alpha exactly 1, so its result does not
          // depend on keys that only other rows of its wave see
          const float mnew = grow ? fmaxf(m[qb], mxs) : m[qb];
          alpha = fast_exp2(m[qb] - (mnew == -INFINITY ? 0.f : mnew));
          m[qb] = mnew;
#pragma unroll
          for (int db = 0; db < 8; ++db) o[qb][db] *= alpha;
        }
        const float msub = m[qb] == -INFINITY ? 0.f : m[qb];
        float rs = 0.f;
        const int qrow = q0 + qb * 16 + i16;
        // keys kbase + kb*16 + 4g + i: pair kbase/2 + (kb >> 1)*16 + 4g + i, half kb & 1 — key
        // blocks kb and kb + 1 at the same i share one hash, in one lane
        uint32_t hp[2][4] = {};
        if constexpr (DROP) {
          const uint32_t hbase = attn_row_term(static_cast<uint32_t>(bh * P.S + qrow)) +
                                 (static_cast<uint32_t>(kbase >> 1) + 4u * g) * kAttnPairMul;
#pragma unroll
          for (int kp = 0; kp < 2; ++kp)
#pragma unroll
            for (int i = 0; i < 4; ++i) hp[kp][i] = attn_hash_input(key, hbase + (16u * kp + i) * kAttnPairMul);
        }
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float p = fast_exp2(__builtin_fmaf(s[qb][kb][i], P.scale_log2, -msub));
            rs += p;
            float pd = p;
            if constexpr (DROP) pd = attn_keep_half(hp[kb >> 1][i], kb & 1, P.drop_thr) ? p : 0.f;
            s[qb][kb][i] = pd;
          }
        }
        rs = tile::rows4_sum(rs);
        l[qb] = l[qb] * alpha + rs;
        pf[qb][0] = pack_frag(s[qb][0], s[qb][1]);
        pf[qb][1] = pack_frag(s[qb][2], s[qb][3]);
      }
      // ---- O += P V: one V^T column fragment feeds both query blocks
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int db = 0; db < 8; ++db) {
          const bf16x8_t vf = rd_col128(sV, ks * 32, ks * 32 + 16, db * 16, lane);
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) o[qb][db] = mfma(vf, pf[qb][ks], o[qb][db]);
        }
    }
    if (nxt) {
      lk.store(smem + (cur ^ 1) * 2 * TILE_BYTES);
      lv.store(smem + (cur ^ 1) * 2 * TILE_BYTES + TILE_BYTES);
    }
    __syncthreads();
    cur ^= 1;
  }
  // ---- normalise, store O (bf16) and lse2: lane holds d = db*16 + 4g + i of query qb*16 + i16
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int qrow = q0 + qb * 16 + i16;
    const float inv = l[qb] > 0.f ? (DROP ? P.drop_scale : 1.f) / l[qb] : 0.f;
    bf16_t* op = P.out + (tok0 + qrow) * P.ld_out + h * D + 4 * g;
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const f32x4_t v = o[qb][db] * inv;
      *reinterpret_cast<uint2*>(op + db * 16) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
    if (g == 0 && P.lse)
      P.lse[static_cast<long long>(bh) * P.S + qrow] = l[qb] > 0.f ? m[qb] + __log2f(l[qb]) : -INFINITY;
  }
}

// ------------------------------------------------------------------------------ bwd dQ
// Prologue: Q and dO fragments, delta = rowsum(dO . O) of the wave's rows (O is read once, here),
// stored for bwd_kv. Per 64-key tile two 32-key halves, each: S and dP (2 key blocks x 2 query
// blocks x 4 d-steps x 2 = 32 MFMAs) -> dS in place -> dQ += dS K (8 d-blocks x 2 query blocks =
// 16 MFMAs, K^T by column reads of the same image). Keys >= len need no mask: their K rows are
// zero-filled in LDS, so their dS adds nothing to dQ (and S = 0, dP = 0 keep it finite).
// CAUSAL: per wave a tile runs full, diagonal (score -inf where key > query, before the exp2:
// P = 0 and dS = 0 exactly) or skipped.
template <bool DROP, bool CAUSAL, bool GQA>
__global__ __launch_bounds__(256, 2) void attn128_bwd_q_kernel(Attn128Params P) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE_BYTES];
  const int qblocks = P.S / QBLK;
  const int t = tile::xcd_remap(blockIdx.x, gridDim.x);
  const int bh = t / qblocks;
  int qblk = t - bh * qblocks;
  if constexpr (CAUSAL) qblk = causal_block(qblk, bh, qblocks, P.order, true);
  const int b = bh / P.H, h = bh - b * P.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int q0 = qblk * QBLK + wave * 32;
  const int len = P.seqlen ? min(P.seqlen[b], P.Sk) : P.Sk;
  const long long tok0 = static_cast<long long>(b) * P.S;
  const long long tokk = static_cast<long long>(b) * P.Sk;

  bf16x8_t qf[2][4], df[2][4];
  float lse2[2], del[2];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const long long row = tok0 + q0 + qb * 16 + i16;
    float acc = 0.f;  // this lane's 32 of the row's 128 dims of dO . O
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[qb][ks] = ldg_frag(P.q + row * P.ldq + h * D + ks * 32 + g * 8);
      df[qb][ks] = ldg_frag(P.dout + row * P.lddo + h * D + ks * 32 + g * 8);
      float a[8], d[8];
      unpack8(ldg16(P.o + row * P.ldo + h * D + ks * 32 + g * 8), a);
      unpack8(__builtin_bit_cast(uint4, df[qb][ks]), d);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += a[j] * d[j];
    }
    acc = tile::rows4_sum(acc);  // the 4 lane groups g hold the row's 4 slices
    del[qb] = acc;
    const long long srow = static_cast<long long>(bh) * P.S + q0 + qb * 16 + i16;
    lse2[qb] = P.lse[srow];
    if (g == 0) P.delta[srow] = acc;
    if constexpr (DROP) {
      // dS = P * (keep * dP / (1-p) - delta) = P_d' * dP - P' * (delta * (1-p)) with P' = P / (1-p)
      // = exp2(s - (lse2 - log2(1/(1-p)))) and P_d' = keep ? P' : 0
      lse2[qb] -= __builtin_amdgcn_logf(P.drop_scale);
      del[qb] *= 1.f / P.drop_scale;
    }
  }
  f32x4_t dq[2][8];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int db = 0; db < 8; ++db) dq[qb][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  TileLoader lk, lv;
  const int hk = GQA ? h / P.G : h;
  lk.init(P.k + tokk * P.ldk + hk * D, P.ldk, tid);
  lv.init(P.v + tokk * P.ldv + hk * D, P.ldv, tid);
  const uint32_t key = DROP ? drop_key(P.rng, P.site) : 0u;
  int ntiles = (len + KT - 1) / KT;
  if constexpr (CAUSAL) ntiles = min(ntiles, 2 * qblk + 2);
  if (ntiles > 0) {
    lk.load(0, len);
    lv.load(0, len);
    lk.store(smem);
    lv.store(smem + TILE_BYTES);
  }
  __syncthreads();

  // keys kbase + 32 hh + {0..31} of the tile image sK: lane holds keys j*16 + 4g + i (j = 0, 1: the
  // two halves of the dropout pair kbase/2 + 16 hh + 4g + i) of query qb*16 + i16
  auto half = [&](const char* sK, int kbase, int hh, auto diag_c, int qd) {
    constexpr bool DIAG = decltype(diag_c)::value;
    const char* sV = sK + TILE_BYTES;
    f32x4_t sc[2][2], dp[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int krow = (2 * hh + j) * 16 + i16;
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) sc[qb][j] = dp[qb][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8_t kfr = rd_row128(sK, krow, ks * 4 + g), vfr = rd_row128(sV, krow, ks * 4 + g);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          sc[qb][j] = mfma(kfr, qf[qb][ks], sc[qb][j]);
          dp[qb][j] = mfma(vfr, df[qb][ks], dp[qb][j]);
        }
      }
    }
    bf16x8_t sfr[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      uint32_t hp[4] = {};
      if constexpr (DROP) {
        const uint32_t hbase = attn_row_term(static_cast<uint32_t>(bh * P.S + q0 + qb * 16 + i16)) +
                               (static_cast<uint32_t>(kbase >> 1) + 4u * g + 16u * hh) * kAttnPairMul;
#pragma unroll
        for (int i = 0; i < 4; ++i) hp[i] = attn_hash_input(key, hbase + static_cast<uint32_t>(i) * kAttnPairMul);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float sv = sc[qb][j][i];
          // DIAG: key > query <=> (2 hh + j)*16 + i - qb*16 > qd, qd = the lane's qb = 0 query -
          // (tile's first key + 4g)
          if constexpr (DIAG) sv = (2 * hh + j) * 16 + i - qb * 16 > qd ? -INFINITY : sv;
          const float p = fast_exp2(__builtin_fmaf(sv, P.scale_log2, -lse2[qb]));
          const float dpv = dp[qb][j][i];
          if constexpr (DROP) {
            const float pd = attn_keep_half(hp[i], j, P.drop_thr) ? p : 0.f;
            sc[qb][j][i] = __builtin_fmaf(pd, dpv, -(p * del[qb]));
          } else {
            sc[qb][j][i] = p * (dpv - del[qb]);
          }
        }
      sfr[qb] = pack_frag(sc[qb][0], sc[qb][1]);
    }
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const bf16x8_t kc = rd_col128(sK, hh * 32, hh * 32 + 16, db * 16, lane);
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) dq[qb][db] = mfma(kc, sfr[qb], dq[qb][db]);
    }
  };
  int cur = 0;
  // FORM (causal): 0 full tile, 1 diagonal tile, 2 skipped by this wave
  auto tile = [&](int kt, auto form_c) {
    constexpr int FORM = decltype(form_c)::value;
    const bool nxt = kt + 1 < ntiles;
    if (nxt) {
      lk.load((kt + 1) * KT, len);
      lv.load((kt + 1) * KT, len);
    }
    if constexpr (FORM != 2) {
      const char* sK = smem + cur * 2 * TILE_BYTES;
      const int kbase = kt * KT;
      const int qd = q0 + i16 - kbase - 4 * g;
      half(sK, kbase, 0, std::integral_constant<bool, FORM == 1>{}, qd);
      half(sK, kbase, 1, std::integral_constant<bool, FORM == 1>{}, qd);
    }
    if (nxt) {
      lk.store(smem + (cur ^ 1) * 2 * TILE_BYTES);
      lv.store(smem + (cur ^ 1) * 2 * TILE_BYTES + TILE_BYTES);
    }
    __syncthreads();
    cur ^= 1;
  };
  for (int kt = 0; kt < ntiles; ++kt) {
    if constexpr (CAUSAL) {
      // wave-uniform: all keys above all of the wave's rows | the tile crosses its diagonal
      if (kt * KT > q0 + 31) tile(kt, std::integral_constant<int, 2>{});
      else if (kt * KT + KT - 1 > q0) tile(kt, std::integral_constant<int, 1>{});
      else tile(kt, std::integral_constant<int, 0>{});
    } else {
      tile(kt, std::integral_constant<int, 0>{});
    }
  }
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    bf16_t* op = P.out + (tok0 + q0 + qb * 16 + i16) * P.ld_out + h * D + 4 * g;
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const f32x4_t v = dq[qb][db] * P.scale;
      *reinterpret_cast<uint2*>(op + db * 16) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
  }
}

// ------------------------------------------------------------------------------ bwd dK, dV
// One wave per SIMD (see the file header): 32 keys per wave, K and V fragments and the dK^T / dV^T
// accumulators stay in registers for the whole sweep over the 64-query tiles of Q / dO (one LDS
// image each, read by rows for S, dP and by columns for dV^T += dO^T P_d, dK^T += Q^T dS).
// Per tile four phases, sched_barrier-separated, each pairing MFMA work with independent VALU work
// of the same wave: S/dP of query rows 0-31 + their hashes | S/dP of rows 32-63 + P/dS of rows
// 0-31 | dV/dK over rows 0-31 + P/dS of rows 32-63 | dV/dK over rows 32-63. 64 + 64 MFMAs a tile.
// Keys >= len are not masked inside: a key's P and dS feed only its own dK / dV rows (the key is
// the MFMA column), which are zeroed at the store.
// CAUSAL: the sweep starts at query tile 2 kblk; its first two tiles cross the block's diagonal
// and run the diagonal form (query < key: score -inf, so P_d = 0 and dS = 0 exactly; a wave whose
// keys all lie above the tile's last query skips the tile's work).
// GQA: the workgroup owns 128 keys of key/value head hk (grid B*Hk*Sk/128) and runs the sweep once
// per query head of its group, in head order, into the same accumulators.
template <bool DROP, bool CAUSAL, bool GQA>
__global__ __launch_bounds__(256, 1) void attn128_bwd_kv_kernel(Attn128Params P) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE_BYTES];
  __shared__ float stats[2][2 * KT];  // per buffer: lse2 of the tile's 64 queries, then delta
  const int kblocks = P.Sk / QBLK;
  const int t = tile::xcd_remap(blockIdx.x, gridDim.x);
  const int bhk = t / kblocks;  // (batch, key/value head)
  int kblk = t - bhk * kblocks;
  if constexpr (CAUSAL) kblk = causal_block(kblk, bhk, kblocks, P.order, false);
  const int nkv = GQA ? P.Hk : P.H;
  const int b = bhk / nkv, hk = bhk - b * nkv;
  const int h0 = GQA ? hk * P.G : hk;  // first query head of the group
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int k0 = kblk * QBLK + wave * 32;
  const int len = P.seqlen ? min(P.seqlen[b], P.Sk) : P.Sk;
  const long long tok0 = static_cast<long long>(b) * P.S;
  const long long tokk = static_cast<long long>(b) * P.Sk;

  f32x4_t dk[2][8], dv[2][8];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int db = 0; db < 8; ++db) dk[kb][db] = dv[kb][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  if (kblk * QBLK < len) {  // block-uniform: some key of this block is valid
    bf16x8_t kf[2][4], vf[2][4];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const long long row = tokk + k0 + kb * 16 + i16;
        kf[kb][ks] = ldg_frag(P.k + row * P.ldk + hk * D + ks * 32 + g * 8);
        vf[kb][ks] = ldg_frag(P.v + row * P.ldv + hk * D + ks * 32 + g * 8);
      }
    // per-tile statistics, staged with the dropout scale folded in: lse2 - log2(1/(1-p)) and
    // delta * (1-p). Thread t < 64 moves lse of query t, 64 <= t < 128 delta of query t - 64.
    const float st_add = tid < KT && DROP ? -__builtin_amdgcn_logf(P.drop_scale) : 0.f;
    const float st_mul = tid >= KT && DROP ? 1.f / P.drop_scale : 1.f;
    const uint32_t key = DROP ? drop_key(P.rng, P.site) : 0u;
    const int ntiles = P.S / KT;
    const int qt0 = CAUSAL ? 2 * kblk : 0;
    const int heads = GQA ? P.G : 1;
    for (int hh = 0; hh < heads; ++hh) {
      const int h = h0 + hh, bh = b * P.H + h;
      TileLoader lq, ld;
      lq.init(P.q + tok0 * P.ldq + h * D, P.ldq, tid);
      ld.init(P.dout + tok0 * P.lddo + h * D, P.lddo, tid);
      const float* st_src = (tid < KT ? P.lse : P.delta) + static_cast<long long>(bh) * P.S + (tid & (KT - 1));
      float stv = 0.f;
      auto load = [&](int qt) {
        lq.load(qt * KT, P.S);
        ld.load(qt * KT, P.S);
        if (tid < 2 * KT) stv = st_src[qt * KT];
      };
      auto store = [&](int buf) {
        lq.store(smem + buf * 2 * TILE_BYTES);
        ld.store(smem + buf * 2 * TILE_BYTES + TILE_BYTES);
        if (tid < 2 * KT) stats[buf][tid] = (stv + st_add) * st_mul;
      };
      f32x4_t sc[4][2], dp[4][2];
      // S[q][key] and dP[q][key] for query blocks qb = 2 hq, 2 hq + 1 of the tile image sQ: lane
      // holds q = qb*16 + 4g + i, key = kb*16 + i16
      auto sdp = [&](const char* sQ, int hq) {
        const char* sD = sQ + TILE_BYTES;
#pragma unroll
        for (int qb = 2 * hq; qb < 2 * hq + 2; ++qb) {
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) sc[qb][kb] = dp[qb][kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const bf16x8_t qfr = rd_row128(sQ, qb * 16 + i16, ks * 4 + g);
            const bf16x8_t dfr = rd_row128(sD, qb * 16 + i16, ks * 4 + g);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
              sc[qb][kb] = mfma(qfr, kf[kb][ks], sc[qb][kb]);
              dp[qb][kb] = mfma(dfr, vf[kb][ks], dp[qb][kb]);
            }
          }
        }
      };
      // dropout: keys k0 + i16 and k0 + 16 + i16 (kb = 0, 1) are the halves of pair k0/2 + i16 —
      // one hash per query row, in one lane
      auto hashes = [&](uint32_t hrow, int hq, uint32_t (&hv)[2][4]) {
        if constexpr (DROP)
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              hv[u][i] = attn_hash_input(key, hrow + static_cast<uint32_t>((2 * hq + u) * 16 + i) * 0x9E3779B1u);
      };
      // P_d and dS in place for half hq (sc <- P_d = P * keep / (1-p); dp <- dS).
      // DIAG: query < key <=> qb*16 + i - kb*16 < kd, kd = the lane's kb = 0 key - (tile's first
      // query + 4g)
      auto pds = [&](const float* sL, const uint32_t (&hv)[2][4], int hq, auto diag_c, int kd) {
        constexpr bool DIAG = decltype(diag_c)::value;
#pragma unroll
        for (int qb = 2 * hq; qb < 2 * hq + 2; ++qb)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int ql = qb * 16 + 4 * g + i;
            const float lse2 = sL[ql], del = sL[KT + ql];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
              float sv = sc[qb][kb][i];
              if constexpr (DIAG) sv = qb * 16 + i - kb * 16 < kd ? -INFINITY : sv;
              const float p = fast_exp2(__builtin_fmaf(sv, P.scale_log2, -lse2));
              const float dpv = dp[qb][kb][i];
              if constexpr (DROP) {
                const float pd = attn_keep_half(hv[qb - 2 * hq][i], kb, P.drop_thr) ? p : 0.f;
                sc[qb][kb][i] = pd;
                dp[qb][kb][i] = __builtin_fmaf(pd, dpv, -(p * del));
              } else {
                sc[qb][kb][i] = p;
                dp[qb][kb][i] = p * (dpv - del);
              }
            }
          }
      };
      // dV^T += dO^T P_d ; dK^T += Q^T dS over the 32 queries of half hq: one column fragment of dO
      // and of Q feeds both key blocks
      auto pv = [&](const char* sQ, int hq) {
        const char* sD = sQ + TILE_BYTES;
        bf16x8_t pfr[2], sfr[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          pfr[kb] = pack_frag(sc[2 * hq][kb], sc[2 * hq + 1][kb]);
          sfr[kb] = pack_frag(dp[2 * hq][kb], dp[2 * hq + 1][kb]);
        }
#pragma unroll
        for (int db = 0; db < 8; ++db) {
          const bf16x8_t dof = rd_col128(sD, hq * 32, hq * 32 + 16, db * 16, lane);
          const bf16x8_t qcf = rd_col128(sQ, hq * 32, hq * 32 + 16, db * 16, lane);
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) {
            dv[kb][db] = mfma(dof, pfr[kb], dv[kb][db]);
            dk[kb][db] = mfma(qcf, sfr[kb], dk[kb][db]);
          }
        }
      };
      auto body = [&](int qt, int buf, auto diag_c) {
        const char* sQ = smem + buf * 2 * TILE_BYTES;
        const float* sL = stats[buf];
        const int kd = k0 + i16 - qt * KT - 4 * g;
        const uint32_t hrow = DROP ? attn_row_term(static_cast<uint32_t>(bh * P.S + qt * KT + 4 * g)) +
                                         (static_cast<uint32_t>(k0 >> 1) + i16) * kAttnPairMul
                                   : 0u;
        uint32_t hv0[2][4] = {}, hv1[2][4] = {};
        sdp(sQ, 0);
        hashes(hrow, 0, hv0);
        __builtin_amdgcn_sched_barrier(0);
        sdp(sQ, 1);
        pds(sL, hv0, 0, diag_c, kd);
        hashes(hrow, 1, hv1);
        __builtin_amdgcn_sched_barrier(0);
        pv(sQ, 0);
        pds(sL, hv1, 1, diag_c, kd);
        __builtin_amdgcn_sched_barrier(0);
        pv(sQ, 1);
      };
      // The image of the head's first tile; every wave has left the previous head's last tile (the
      // barrier that ends its loop), so buffer 0 is free.
      load(qt0);
      store(0);
      __syncthreads();
      int cur = 0;
      // one tile: the next one's global loads are in flight meanwhile and go to the other buffer
      auto step = [&](int qt, auto diag_c) {
        const bool nxt = qt + 1 < ntiles;
        if (nxt) load(qt + 1);
        // diagonal form, wave-uniform: not all of this wave's keys lie above the tile's last query
        if (!decltype(diag_c)::value || __builtin_amdgcn_readfirstlane(k0) <= qt * KT + KT - 1) body(qt, cur, diag_c);
        if (nxt) store(cur ^ 1);
        __syncthreads();
        cur ^= 1;
      };
      int qt = qt0;
      // (the diagonal trip as a loop of its own: one loop that chooses the form per tile spills)
      if constexpr (CAUSAL)
        for (; qt < qt0 + 2; ++qt) step(qt, std::true_type{});
      for (; qt < ntiles; ++qt) step(qt, std::false_type{});
    }
  }
  // store dK (scaled by 1/sqrt(128)) and dV: lane holds key kb*16 + i16, d = db*16 + 4g + i; keys
  // >= len get zeros (their accumulators saw unmasked probabilities)
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const long long row = tokk + k0 + kb * 16 + i16;
    bf16_t* pk = P.out + row * P.ld_out + hk * D + 4 * g;
    bf16_t* pv = P.out2 + row * P.ld_out2 + hk * D + 4 * g;
    const bool valid = k0 + kb * 16 + i16 < len;
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
      const f32x4_t a = valid ? dk[kb][db] * P.scale : zero, c = valid ? dv[kb][db] : zero;
      *reinterpret_cast<uint2*>(pk + db * 16) = make_uint2(pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]));
      *reinterpret_cast<uint2*>(pv + db * 16) = make_uint2(pack_bf16x2(c[0], c[1]), pack_bf16x2(c[2], c[3]));
    }
  }
}

Attn128Params make_params(int B, int H, int Hk, int S, int Sk, const int* seqlen, float p_drop, const long long* rng,
                          uint32_t site, int causal) {
  Attn128Params P{};
  P.B = B;
  P.H = H;
  P.Hk = Hk;
  P.G = H / Hk;
  P.S = S;
  P.Sk = Sk;
  P.seqlen = seqlen;
  P.scale = 0.08838834764831845f;  // 1/sqrt(128)
  P.scale_log2 = 0.08838834764831845f * 1.4426950408889634f;
  P.drop_thr = drop_threshold16(p_drop);
  // unbiased for the keep probability the 16-bit threshold actually realises
  P.drop_scale = p_drop > 0.f ? static_cast<float>(65536.0 / (65536.0 - static_cast<double>(P.drop_thr))) : 1.f;
  P.rng = rng;
  P.site = site;
  P.order = causal ? 2 : 0;  // the rotated block order (profiles/attn_causal_bench.txt)
  return P;
}

// What both entry points refuse (as attention.hip): lds is the OR of every leading dimension of
// the call, bases the pointers that have to be 16-byte aligned.
bool args_ok(int B, int H, int Hk, int Sq, int Sk, int causal, float p_drop, const long long* rng, long long lds,
             std::initializer_list<const void*> bases) {
  if (B <= 0 || H <= 0 || Hk <= 0 || H % Hk || Sq <= 0 || Sk <= 0 || Sq % QBLK || Sk % QBLK || (causal && Sq != Sk) ||
      (lds & 7) || (p_drop > 0.f && !rng))
    return false;
  for (const void* p : bases)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}

// Every instantiation that is launched, indexed [gqa][causal][drop] (gqa: Hk != H).
using Attn128Kernel = void (*)(Attn128Params);

constexpr Attn128Kernel kFwd[2][2][2] = {
    {{attn128_fwd_kernel<false, false, false>, attn128_fwd_kernel<true, false, false>},
     {attn128_fwd_kernel<false, true, false>, attn128_fwd_kernel<true, true, false>}},
    {{attn128_fwd_kernel<false, false, true>, attn128_fwd_kernel<true, false, true>},
     {attn128_fwd_kernel<false, true, true>, attn128_fwd_kernel<true, true, true>}}};

constexpr Attn128Kernel kBwdQ[2][2][2] = {
    {{attn128_bwd_q_kernel<false, false, false>, attn128_bwd_q_kernel<true, false, false>},
     {attn128_bwd_q_kernel<false, true, false>, attn128_bwd_q_kernel<true, true, false>}},
    {{attn128_bwd_q_kernel<false, false, true>, attn128_bwd_q_kernel<true, false, true>},
     {attn128_bwd_q_kernel<false, true, true>, attn128_bwd_q_kernel<true, true, true>}}};

constexpr Attn128Kernel kBwdKv[2][2][2] = {
    {{attn128_bwd_kv_kernel<false, false, false>, attn128_bwd_kv_kernel<true, false, false>},
     {attn128_bwd_kv_kernel<false, true, false>, attn128_bwd_kv_kernel<true, true, false>}},
    {{attn128_bwd_kv_kernel<false, false, true>, attn128_bwd_kv_kernel<true, false, true>},
     {attn128_bwd_kv_kernel<false, true, true>, attn128_bwd_kv_kernel<true, true, true>}}};

}  // namespace
}  // namespace ttdk

using namespace ttdk;

// ttdk_attn_fwd for head_dim 128: the same arguments with the same meaning (q / o [B*Sq, >= H*128],
// k / v [B*Sk, >= Hk*128], lse [B*H][Sq]), the same refusals (hipErrorInvalidValue, nothing launched).
TTDK_API(int, ttdk_attn128_fwd, (const bf16_t* q, long long ldq, const bf16_t* k, long long ldk, const bf16_t* v,
                                 long long ldv, bf16_t* o, long long ldo, float* lse, const int* seqlen, int B, int H,
                                 int Hk, int Sq, int Sk, float p_drop, const long long* rng, unsigned site, int causal,
                                 hipStream_t st)) {
  if (!args_ok(B, H, Hk, Sq, Sk, causal, p_drop, rng, ldq | ldk | ldv | ldo, {q, k, v, o})) return hipErrorInvalidValue;
  Attn128Params P = make_params(B, H, Hk, Sq, Sk, seqlen, p_drop, rng, site, causal);
  P.q = q; P.k = k; P.v = v; P.ldq = ldq; P.ldk = ldk; P.ldv = ldv;
  P.out = o; P.ld_out = ldo; P.lse = lse;
  hipLaunchKernelGGL(kFwd[Hk != H][causal != 0][p_drop > 0.f], dim3(B * H * (Sq / QBLK)), dim3(256), 0, st, P);
  return hipGetLastError();
}

// ttdk_attn_bwd for head_dim 128, always the split kernels: bwd_q over B*H*Sq/128 workgroups (it
// stores delta), then bwd_kv over B*Hk*Sk/128. dq / dk / dv may alias one fused
// [tokens, (H + 2*Hk)*128] buffer (different column offsets).
TTDK_API(int, ttdk_attn128_bwd, (const bf16_t* q, long long ldq, const bf16_t* k, long long ldk, const bf16_t* v,
                                 long long ldv, const bf16_t* o, long long ldo, const bf16_t* dout, long long lddo,
                                 const float* lse, float* delta, bf16_t* dq, long long lddq, bf16_t* dk, long long lddk,
                                 bf16_t* dv, long long lddv, const int* seqlen, int B, int H, int Hk, int Sq, int Sk,
                                 float p_drop, const long long* rng, unsigned site, int causal, hipStream_t st)) {
  if (!args_ok(B, H, Hk, Sq, Sk, causal, p_drop, rng, ldq | ldk | ldv | ldo | lddo | lddq | lddk | lddv,
               {q, k, v, o, dout}))
    return hipErrorInvalidValue;
  const bool gqa = Hk != H, drop = p_drop > 0.f;
  Attn128Params P = make_params(B, H, Hk, Sq, Sk, seqlen, p_drop, rng, site, causal);
  P.q = q; P.k = k; P.v = v; P.o = o; P.dout = dout;
  P.ldq = ldq; P.ldk = ldk; P.ldv = ldv; P.ldo = ldo; P.lddo = lddo;
  P.lse = const_cast<float*>(lse);
  P.delta = delta;
  P.out = dq; P.ld_out = lddq;
  hipLaunchKernelGGL(kBwdQ[gqa][causal != 0][drop], dim3(B * H * (Sq / QBLK)), dim3(256), 0, st, P);
  P.out = dk; P.ld_out = lddk; P.out2 = dv; P.ld_out2 = lddv;
  hipLaunchKernelGGL(kBwdKv[gqa][causal != 0][drop], dim3(B * Hk * (Sk / QBLK)), dim3(256), 0, st, P);
  return hipGetLastError();
}
