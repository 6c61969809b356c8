// Fused multi-head attention (flash-style) forward and backward for head_dim 64 on gfx950
// MFMA (v_mfma_f32_16x16x32_bf16): BERT-Large self-attention (SURVEY.md §2.6 [NS] BERT
// kernels; BASELINE.json config 4). The S x S score matrix is never materialised.
//
// Layout: token-major activations straight out of / into the fused QKV projection GEMM:
//   element (b, s, h, d) of Q/K/V/O/dQ/dK/dV at base + (b*S + s)*ld + h*64 + d
// so no transposes surround the kernels. Per (batch, head) softmax statistics lse2 / delta
// are fp32 [B*H][S]. Scores live in the log2 domain: s2 = (q.k) * log2(e)/sqrt(64),
// P = exp2(s2 - lse2).
//
// Options: per-batch key lengths (keys >= len masked), banded masks (BAND: every query row attends
// one contiguous key range — packed documents, sliding windows, causal and the key length folded
// into a table that ttdk_attn_band builds; only the tiles of a block's range are streamed:
// profiles/attn_band_bench.txt), causal masking (query q attends keys
// k <= q; fwd, bwd_q and bwd_kv skip the tiles above the diagonal: 20 of 32 at S = 512), and
// attention-probability dropout whose keep mask is a counter hash of (seed, step, site,
// (b*H+h, q, key)) — regenerated identically in both backward kernels, never stored; the hash
// inputs are absolute indices, so a causal run keeps what a bidirectional run keeps.
// Causal at BERT-Large b128 (S = 512, p = 0.1): fwd 198 us against 277 us bidirectional, bwd_q +
// bwd_kv 577 us against 782 us — with the rotated block order of causal_block(); in natural or
// heavy-first order the causal kernels gain 6 % at most (profiles/attn_causal_bench.txt).
//
//
// One exported pair, ttdk_attn_fwd / ttdk_attn_bwd, takes every form below (B, H, Hk, Sq, Sk, causal);
// self-attention is Hk == H, Sk == Sq. The host code picks the instantiation from a table.
//
// Cross-attention (Sk != Sq): the query length S and the key
// length Sk are separate (a decoder's attention over an encoder's output). Every kernel owns
// 128 rows of one kind and streams 64-row tiles of the other, so only the index arithmetic
// tells them apart:
//   query rows (Q, O, dO, dQ)  token base b*S,  lse / delta row bh*S + q, S/128 blocks in fwd and
//                              bwd_q, S/64 streamed tiles in bwd_kv;
//   key rows (K, V, dK, dV)    token base b*Sk, len = min(seqlen[b], Sk) — seqlen is the memory's
//                              length, queries are never masked — Sk/128 blocks in bwd_kv.
// The dropout hash takes row id bh*S + q and a pair term of the key index alone, so with Sk == S
// it is the self-attention hash and a longer memory extends a shorter one's mask. fwd and bwd_q
// launch B*H*S/128 workgroups, bwd_kv B*H*Sk/128. The causal instantiations and the fused
// backward are for Sk == S only.
//
// Grouped-query attention (Hk != H): H query heads share Hk key/value
// heads, G = H / Hk to each (Hk == 1: multi-query attention); query head h uses key/value head
// h / G, the layout of repeat_interleave over the head axis. K, V, dK, dV hold Hk * 64 columns and
// are never repeated in memory. Again only the index arithmetic differs:
//   what belongs to the query (Q, O, dO, dQ, lse / delta row bh*S + q, the dropout row id
//                              bh*S + q) stays indexed by the query head, bh = b*H + h: the
//                              heads of a group draw independent dropout masks;
//   K / V tiles (fwd, bwd_q)   column (h / G) * 64; the grids stay B*H*S/128;
//   bwd_kv                     B*Hk*Sk/128 workgroups: one owns 128 keys of ONE key/value head and
//                              sweeps the 64-query tiles of its G query heads in turn (Q / dO
//                              column, lse / delta rows and dropout row ids of that head), dK and
//                              dV staying in the same register accumulators, stored once. The sum
//                              over the group runs in fp32 in head order: no atomics, no workspace,
//                              no second pass, the same bits every run. Causal: every head's sweep
//                              starts at qt0 = 2 kblk with its own diagonal trip.
// With Hk == H every kernel is the self-attention kernel: the grouped forms are template
// instantiations of their own (GQA), so the self-attention code is unchanged — a run-time G == 1
// cost the causal p = 0.1 backward 2 us of 573 (profiles/attn_gqa_bench.txt, section 0). The fused backward is
// an Hk == H kernel. Locality (read off the code, not measured): xcd_remap hands each XCD one
// contiguous run of work items, and the G * S/128 fwd / bwd_q work items of a group are
// contiguous, so a group's heads read their shared K / V through one XCD's L2 — except the at
// most 7 groups that straddle the end of an XCD's run (none when B*Hk is a multiple of 8). In
// bwd_kv the group is one workgroup: K and V are read once, into registers.
//
// Kernels (4 waves / workgroup, XCD-aware block order so the Q-blocks of one head share an
// L2):
//   fwd     : 128 query rows per workgroup (32 per wave); K/V tiles of 64 keys double-buffered
//             in LDS (register-staged prefetch); online softmax in registers; the swapped QK^T
//             puts 4 keys x 1 query in each lane, so P feeds the PV MFMA without any shuffle.
//   bwd_kv  : 128 keys per workgroup; loops over 64-query tiles of Q/dO (one LDS image read
//             by rows for S, dP and by columns (ds_read_b64_tr_b16) for dV^T, dK^T); dK, dV
//             accumulate in registers — no cross-workgroup sums.
//   bwd_q   : 128 queries per workgroup; first delta = rowsum(dO * O) of its query rows (the
//             dO fragments are already in registers; O is read once, here) — stored for
//             bwd_kv, which runs after it; then recomputes S, dP per key tile; dQ in registers
//             (deterministic, no float atomics). (A separate delta pass re-read O and dO:
//             227 us per BERT-Large b128 layer, 5.5 ms per step.)
//   bwd_fused (opt-in): all of dQ, dK, dV of one (batch, head) in one workgroup — five MFMA
//             products instead of seven, one dropout hash per element instead of two; slower
//             at BERT-Large's S = 512 (occupancy: see ttdk_attn_set_fused_bwd).
#include "tile_common.h"

#include <initializer_list>
#include <type_traits>

namespace ttdk {
namespace {

using tile::mfma;
using tile::off64;
using tile::pack_frag;
using tile::rd_col;
using tile::rd_row;

constexpr int D = 64;
constexpr int KT = 64;    // keys (fwd/bwd_q) or queries (bwd_kv) per streamed tile
constexpr int QBLK = 128; // rows per workgroup
constexpr int TILE_BYTES = KT * D * 2;

struct AttnParams {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  const bf16_t* o;
  const bf16_t* dout;
  long long ldq, ldk, ldv, ldo, lddo;
  bf16_t* out;   // fwd: O ; bwd_q: dQ ; bwd_kv: dK
  bf16_t* out2;  // bwd_kv: dV ; fused bwd: dK
  bf16_t* out3;  // fused bwd: dV
  long long ld_out, ld_out2, ld_out3;
  float* lse;          // [B*H][S] log2 domain
  float* delta;        // [B*H][S]: written by bwd_q, read by bwd_kv
  const int* seqlen;   // [B] or null
  int B, H, S;         // S: query rows per batch (Q, O, dO, dQ, lse, delta)
  int Sk;              // key rows per batch (K, V, dK, dV); == S for self-attention
  float scale_log2;    // log2(e) / sqrt(D)
  float scale;         // 1 / sqrt(D)
  uint32_t drop_thr;
  float drop_scale;    // 1 / (1 - p)
  const long long* rng;
  uint32_t site;
  int order;           // causal block order within a head: causal_block()
  // (last, so that the fields above keep their kernarg offsets)
  int Hk, G;           // key/value heads and G = H / Hk query heads per key/value head; Hk == H,
                       // G == 1 unless grouped-query attention
  // BAND only: the table of ttdk_attn_band
  const int4* band_tok;  // [B][S] {klo, khi, qlo, qhi}: keys [klo, khi) of a query, queries [qlo, qhi) of a key
  const int4* band_blk;  // [B][S/128] {kt0, kt1, qt0, qt1}: the 64-row tiles a query / key block streams
};

// BAND: a wave's 32 rows are rows i16 and 16 + i16 of every 16-lane group; min / max over them as
// a wave-uniform (scalar) value.
__device__ __forceinline__ int rows_min(int a, int b) {
  int x = min(a, b);
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) x = min(x, __shfl_xor(x, o, 64));
  return __builtin_amdgcn_readfirstlane(x);
}
__device__ __forceinline__ int rows_max(int a, int b) {
  int x = max(a, b);
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) x = max(x, __shfl_xor(x, o, 64));
  return __builtin_amdgcn_readfirstlane(x);
}

// BAND: the ranges of this lane's two rows (row0 + i16 and row0 + 16 + i16 — queries in fwd and
// bwd_q, KEYS in bwd_kv), the union and the intersection of the ranges of the wave's 32 rows, and
// the tile range of the 128-row block.
struct BandRows {
  int lo[2], w[2];         // the range's first index and its length (< 0: empty)
  int ulo, uhi, ilo, ihi;  // wave-uniform
  int t0, t1;              // block-uniform
  // lo / w alone (bwd_kv reads them again in every masked tile and at the store, which is cheaper
  // than four more registers live across its loop)
  template <bool KEYS>
  __device__ __forceinline__ void rows(const AttnParams& P, int b, int row0, int i16) {
    const int4* rp = P.band_tok + static_cast<long long>(b) * P.S + row0 + i16;
    const int2 r0 = reinterpret_cast<const int2*>(rp)[KEYS ? 1 : 0];
    const int2 r1 = reinterpret_cast<const int2*>(rp + 16)[KEYS ? 1 : 0];
    lo[0] = r0.x;
    lo[1] = r1.x;
    w[0] = r0.y - r0.x;
    w[1] = r1.y - r1.x;
  }
  template <bool KEYS>
  __device__ __forceinline__ void init(const AttnParams& P, int b, int blk, int row0, int i16) {
    const int4 bk = P.band_blk[b * (P.S / QBLK) + blk];
    t0 = KEYS ? bk.z : bk.x;
    t1 = KEYS ? bk.w : bk.y;
    rows<KEYS>(P, b, row0, i16);
    ulo = rows_min(lo[0], lo[1]);
    uhi = rows_max(lo[0] + w[0], lo[1] + w[1]);
    ilo = rows_max(lo[0], lo[1]);
    ihi = rows_min(lo[0] + w[0], lo[1] + w[1]);
  }
  // the tile of n indices from base: outside every row's range | inside every row's range
  __device__ __forceinline__ bool skip(int base, int n) const { return base >= uhi || base + n <= ulo; }
  __device__ __forceinline__ bool full(int base, int n) const { return base >= ilo && base + n <= ihi; }
  // index idx is outside the range of row r (one subtract, one unsigned compare; an empty range
  // has lo = S, w = -S: every idx < S is outside)
  __device__ __forceinline__ bool masked(int r, int idx) const {
    return static_cast<unsigned>(idx - lo[r]) >= static_cast<unsigned>(w[r]);
  }
};

__device__ __forceinline__ uint4 ldg16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }

__device__ __forceinline__ bf16x8_t ldg_frag(const bf16_t* p) {
  return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(p));
}

// 64 rows x 64 cols tile loader: thread t moves rows (t >> 3) and (t >> 3) + 32, chunk t & 7.
// The lane's row / chunk offset is folded into its pointer once; per tile only the block-uniform
// row0 * ld is formed (scalar), not a 64-bit vector multiply per row (v_mul_lo_u32 is a
// quarter-rate instruction in these VALU-bound loops).
struct TileLoader {
  const bf16_t* lanep;
  long long ld;
  int r, c;
  uint4 v[2];
  __device__ __forceinline__ void init(const bf16_t* b, long long l, int tid) {
    ld = l;
    r = tid >> 3;
    c = tid & 7;
    lanep = b + static_cast<long long>(r) * l + c * 8;
  }
  __device__ __forceinline__ void load(int row0, int nrows) {
    const bf16_t* p = lanep + static_cast<long long>(row0) * ld;
    if (row0 + 64 <= nrows) {  // block-uniform: whole tile in range, no per-dword selects
#pragma unroll
      for (int j = 0; j < 2; ++j) v[j] = ldg16(p + 32 * j * ld);
      return;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = row0 + r + 32 * j;
      v[j] = row < nrows ? ldg16(p + 32 * j * ld) : make_uint4(0, 0, 0, 0);
    }
  }
  __device__ __forceinline__ void store(char* lds) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) *reinterpret_cast<uint4*>(lds + off64(r + 32 * j, c * 8)) = v[j];
  }
};

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Causal workgroups do unequal work (block b of a head streams 2b + 2 tiles in fwd / bwd_q, and
// 2 (nblk - b) in bwd_kv), and the nblk blocks of a head stay adjacent in the grid (they share
// K / V or Q / dO in one XCD's L2). Which block the j-th work item of head bh takes:
//   order 0  natural (j);
//   order 1  heavy first: the longest block of each head first. Measured no better than natural,
//            and both about as slow as if every block were the longest: the grid then has period
//            nblk, workgroups reach the CUs round-robin, so a CU keeps drawing the same block
//            index and the CUs that draw the long one set the kernel's time;
//   order 2  rotated: j plus the base-4 digit sum of bh. Over every power-of-two stride of the
//            grid the block index then cycles evenly, so every CU gets the same mix.
// (profiles/attn_causal_bench.txt)
__device__ __forceinline__ int causal_block(int j, int bh, int nblk, int order, bool long_last) {
  if (order == 2) {
    uint32_t x = static_cast<uint32_t>(bh);
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    x = (x + (x >> 4)) & 0x0f0f0f0fu;
    x = (x * 0x01010101u) >> 24;  // sum of the base-4 digits (<= 48)
    return static_cast<int>((static_cast<uint32_t>(j) + x) % static_cast<uint32_t>(nblk));
  }
  return order == 1 && long_last ? nblk - 1 - j : j;
}

// ------------------------------------------------------------------------------ forward
// (launch_bounds(256, 4) — 128 VGPRs, 4 waves / SIMD instead of 3, 10-12 spilled — measured
// 10-18 % slower at BERT-Large b128: the spills land in the loop)
//
// CAUSAL (query q attends keys k <= q, and k < len): only key tiles kt <= 2 qblk + 1 are streamed;
// the per-element compare runs on the tiles that cross the wave's diagonal only (wave-uniform,
// as the len mask is block-uniform), and a wave whose 32 rows all lie below a tile's first key
// skips the tile's MFMA / softmax work (it still moves its share of the next tile and meets the
// barrier). Masked scores are -inf BEFORE the row max, so a masked key adds exactly nothing to
// m, l, O; and the running max moves per row (not for every row of a wave whose ballot fired), so
// a row's result does not depend on keys that only other rows of its wave may see.
//
// GQA (launched when Hk != H): K / V tiles from key/value head h / G; everything else as above.
// A template parameter, not a run-time G == 1: the self-attention kernels keep their code, without
// the integer division at the head of every workgroup's address chain.
//
// BAND (never with CAUSAL; Sk == S): row q attends keys [klo, khi) of its band_tok record, which
// folds documents, window, causal and seqlen. The block streams key tiles kt0 .. kt1 - 1 of its
// band_blk record only. Per wave (wave-uniform, from the min / max of its 32 rows' ranges): a tile
// outside the union of the ranges is skipped like a causal tile above the diagonal; a tile inside
// their intersection runs no compare; any other tile masks per element, -inf before the row max.
// A row with an empty range (klo = S, khi = 0: padding) keeps m = -inf, l = 0: O = 0, lse = -inf.
template <bool DROP, bool CAUSAL = false, bool GQA = false, bool BAND = false>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(AttnParams P) {
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
  const int len = BAND ? P.Sk : P.seqlen ? min(P.seqlen[b], P.Sk) : P.Sk;  // BAND: in the table
  const long long tok0 = static_cast<long long>(b) * P.S;    // query rows: Q, O, dO, dQ
  const long long tokk = static_cast<long long>(b) * P.Sk;   // key rows: K, V, dK, dV
  BandRows band;
  if constexpr (BAND) band.init<false>(P, b, qblk, q0, i16);

  bf16x8_t qf[2][2];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      qf[qb][ks] = ldg_frag(P.q + (tok0 + q0 + qb * 16 + i16) * P.ldq + h * D + ks * 32 + g * 8);

  TileLoader lk, lv;
  const int hk = GQA ? h / P.G : h;  // the key/value head of query head h
  lk.init(P.k + tokk * P.ldk + hk * D, P.ldk, tid);
  lv.init(P.v + tokk * P.ldv + hk * D, P.ldv, tid);

  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
  f32x4_t o[2][4];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int db = 0; db < 4; ++db) o[qb][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const uint32_t key = DROP ? drop_key(P.rng, P.site) : 0u;
  int ntiles = (len + KT - 1) / KT;
  if constexpr (CAUSAL) ntiles = min(ntiles, 2 * qblk + 2);
  int kt0 = 0;
  if constexpr (BAND) {
    kt0 = band.t0;
    ntiles = band.t1;
  }
  if (ntiles > kt0) {
    lk.load(kt0 * KT, len);
    lv.load(kt0 * KT, len);
    lk.store(smem);
    lv.store(smem + TILE_BYTES);
  }
  __syncthreads();
  int cur = 0;
  for (int kt = kt0; kt < ntiles; ++kt) {
    const bool nxt = kt + 1 < ntiles;
    if (nxt) {
      lk.load((kt + 1) * KT, len);
      lv.load((kt + 1) * KT, len);
    }
    const char* sK = smem + cur * 2 * TILE_BYTES;
    const char* sV = sK + TILE_BYTES;
    // CAUSAL: every key of the tile lies above every row of this wave (wave-uniform)
    // BAND: the tile lies outside the range of every row of this wave (wave-uniform)
    if (BAND ? !band.skip(kt * KT, KT) : !CAUSAL || kt * KT <= q0 + 31) {
      // ---- S^T tile: lane holds keys kb*16 + 4g + i for query qb*16 + i16
      f32x4_t s[2][4];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const bf16x8_t k0 = rd_row(sK, kb * 16 + i16, g);
        const bf16x8_t k1 = rd_row(sK, kb * 16 + i16, 4 + g);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          s[qb][kb] = mfma(k0, qf[qb][0], f32x4_t{0.f, 0.f, 0.f, 0.f});
          s[qb][kb] = mfma(k1, qf[qb][1], s[qb][kb]);
        }
      }
      const int kbase = kt * KT;
      if constexpr (BAND) {
        if (!band.full(kbase, KT)) {
          // (wave-uniform: some row's range ends inside the tile)
#pragma unroll
          for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (band.masked(qb, kbase + 4 * g + kb * 16 + i)) s[qb][kb][i] = -INFINITY;
        }
      }
      if (!BAND && kbase + KT > len) {
        // (block-uniform: only the last key tile of a padded sequence; the full tiles run no
        // per-element compare / select — the kernel is VALU-bound, profiles/r3_bert_*_pmc_*)
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
          // (wave-uniform: the tile crosses this wave's diagonal; key > query <=> kb*16 + i - qb*16
          // > qd = query - (kbase + 4g), constants against one lane value)
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
        // lazy rescale: the running max moves (and O, l are rescaled) only when some row of the
        // wave saw its max grow by more than 8 (log2 units) — otherwise P = exp2(s - m) stays
        // below 2^8 (exact in fp32, in range for the bf16 P operand) and the 16 O multiplies and
        // the alpha exp2 of the tile are skipped (wave-uniform branch; lse = m + log2 l either way)
        const float mxs = mx * P.scale_log2;
        float alpha = 1.f;
        const bool grow = mxs > m[qb] + 8.f;
        if (__builtin_amdgcn_ballot_w64(grow) != 0) {
          float mnew = fmaxf(m[qb], mxs);
          if constexpr (CAUSAL || BAND) mnew = grow ? mnew : m[qb];  // per row: alpha is exactly 1 elsewhere
          alpha = fast_exp2(m[qb] - (mnew == -INFINITY ? 0.f : mnew));
          m[qb] = mnew;
#pragma unroll
          for (int db = 0; db < 4; ++db) o[qb][db] *= alpha;
        }
        const float msub = m[qb] == -INFINITY ? 0.f : m[qb];
        float rs = 0.f;
        const int qrow = q0 + qb * 16 + i16;
        // keys kbase + kb*16 + 4g + i: pair kbase/2 + (kb >> 1)*16 + 4g + i, half kb & 1 — the
        // hash input is a per-tile base plus constants
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
      // ---- O += P V
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          const bf16x8_t vf = rd_col(sV, ks * 32, ks * 32 + 16, db * 16, lane);
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
  // ---- normalise, store O (bf16) and lse2
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int qrow = q0 + qb * 16 + i16;
    const float inv = l[qb] > 0.f ? (DROP ? P.drop_scale : 1.f) / l[qb] : 0.f;
    bf16_t* op = P.out + (tok0 + qrow) * P.ld_out + h * D + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const f32x4_t v = o[qb][db] * inv;
      uint2 w;
      w.x = pack_bf16x2(v[0], v[1]);
      w.y = pack_bf16x2(v[2], v[3]);
      *reinterpret_cast<uint2*>(op + db * 16) = w;
    }
    if (g == 0 && P.lse)
      P.lse[static_cast<long long>(bh) * P.S + qrow] = l[qb] > 0.f ? m[qb] + __log2f(l[qb]) : -INFINITY;
  }
}

// ------------------------------------------------------------------------------ bwd dK, dV
// Per 64-query tile, four phases that each put one wave's MFMA work beside independent VALU
// work of the same wave (sched_barrier-separated, so the scheduler interleaves within a phase):
// S/dP of query rows 0-31 | S/dP of rows 32-63 + P/dS of rows 0-31 | dV/dK over rows 0-31 + P/dS
// of rows 32-63 | dV/dK over rows 32-63. The previous loop ran all of S/dP, then all P/dS, then
// all dV/dK per wave: 20 % MFMA busy, 50 % of wave cycles waiting at BERT-Large b128
// (profiles/r5_attn_bwd_pmc_before.txt). Two LDS buffers with compile-time offsets (the loop
// handles two tiles per trip), register-staged global loads one tile ahead, one barrier per tile.
// MODE (diagnostics, TTD_ATTN_KV_DIAG; 0 in production): bit 0 skips the elementwise P / dS,
// bit 1 the per-tile Q / dO reloads, bit 2 the per-tile barrier (only with bit 1) — wrong
// results, for attributing the kernel's time; bit 3 writes per-workgroup clock stamps (entry,
// prologue done, loop done, exit as s_memtime; entry / exit as s_memrealtime) over dV as
// int64[grid][8] instead of dV (the script that read them is not in the tree).
//
// CAUSAL (MODE 0 only): the query-tile loop starts at qt0 = 2 kblk (even, so the two-buffer trip
// structure holds); the two tiles of the first trip cross the block's diagonal and run the
// diagonal form of the tile body: queries below the key get P = 0 and dS = 0 in pds, and a wave
// (32 keys from k0) whose keys all lie above the tile's last query skips the tile (no MFMA /
// softmax work, only its share of the next tile's staging and the barrier). Every later trip
// runs today's unmasked body. Block order: causal_block().
//
// GQA (MODE 0 only; launched when Hk != H): the workgroup owns 128 keys of key/value head hk of
// batch b (grid B*Hk*Sk/128; causal_block() and the XCD remap take b*Hk + hk) and runs the sweep
// above once per query head h0 .. h0 + G - 1 of its group, h0 = hk * G, into the same dk / dv.
//
// BAND (MODE 0 only, never with CAUSAL; Sk == S): key k is attended by queries [qlo, qhi) of its
// band_tok record, fixed for the workgroup's keys. The sweep runs query tiles qt0 .. qt1 - 1 of
// the block's band_blk record (both even: whole trips; every head of a GQA group the same range).
// Per trip and wave (wave-uniform): both tiles inside the intersection of the 32 keys' ranges —
// today's unmasked body; otherwise the masked form, which skips a tile outside the union of the
// ranges and selects a score of -inf for the elements outside their key's range: P = exp2(-inf) = 0
// and dS = 0 exactly. The query may be a padding row with lse = -inf: it is staged as +inf, so
// nothing is computed through exp2(-inf + inf).
template <bool DROP, int MODE = 0, bool CAUSAL = false, bool GQA = false, bool BAND = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_kv_kernel(AttnParams P) {
  constexpr int BUF = 2 * TILE_BYTES + 2 * KT * 4;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
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
  const int len = BAND ? P.Sk : P.seqlen ? min(P.seqlen[b], P.Sk) : P.Sk;  // BAND: in the table
  const long long tok0 = static_cast<long long>(b) * P.S;    // query rows: Q, O, dO, dQ
  const long long tokk = static_cast<long long>(b) * P.Sk;   // key rows: K, V, dK, dV
  BandRows band;
  if constexpr (BAND) band.init<true>(P, b, kblk, k0, i16);
  long long stamp[6] = {};
  if constexpr ((MODE & 8) != 0) {
    stamp[0] = __builtin_amdgcn_s_memtime();
    stamp[4] = __builtin_amdgcn_s_memrealtime();
  }

  f32x4_t dk[2][4], dv[2][4];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int db = 0; db < 4; ++db) dk[kb][db] = dv[kb][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // block-uniform: some key of this block is valid (BAND: is attended by some query)
  const bool any = BAND ? band.t0 < band.t1 : kblk * QBLK < len;
  if (any) {
    bf16x8_t kf[2][2], vf[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const long long row = tokk + k0 + kb * 16 + i16;
        kf[kb][ks] = ldg_frag(P.k + row * P.ldk + hk * D + ks * 32 + g * 8);
        vf[kb][ks] = ldg_frag(P.v + row * P.ldv + hk * D + ks * 32 + g * 8);
      }
    // the query head being swept: h0 .. h0 + G - 1 in turn (GQA: the trip loop below moves bh, the
    // two loaders and st_src on by one head)
    int bh = GQA ? b * P.H + h0 : bhk;
    TileLoader lq, ld;
    lq.init(P.q + tok0 * P.ldq + h0 * D, P.ldq, tid);
    ld.init(P.dout + tok0 * P.lddo + h0 * D, P.lddo, tid);
    // per-tile statistics, staged with the dropout scale folded in: lse2 - log2(1/(1-p)) (exp2
    // then gives P / (1-p), a kept probability's value) and delta * (1-p) (the product P * delta
    // unchanged). Thread t < 64 moves lse of query t, 64 <= t < 128 delta of query t - 64.
    const float* st_src = (tid < KT ? P.lse : P.delta) + static_cast<long long>(bh) * P.S + (tid & (KT - 1));
    const float st_add = tid < KT && DROP ? -__builtin_amdgcn_logf(P.drop_scale) : 0.f;
    const float st_mul = tid >= KT && DROP ? 1.f / P.drop_scale : 1.f;
    float stv = 0.f;
    const uint32_t key = DROP ? drop_key(P.rng, P.site) : 0u;
    // query tiles; even: S is a multiple of QBLK = 2 * KT (BAND: the sweep's end, even too)
    const int ntiles = BAND ? band.t1 : P.S / KT;

    auto load = [&](int qt) {
      // (BAND: the sweep ends at a tile the table names, inside the S rows — no partial-tile path)
      lq.load(qt * KT, BAND ? 0x7fffffff : P.S);
      ld.load(qt * KT, BAND ? 0x7fffffff : P.S);
      if (tid < 2 * KT) stv = st_src[qt * KT];
    };
    auto store = [&](char* nb) {
      lq.store(nb);
      ld.store(nb + TILE_BYTES);
      // BAND: a padding row's lse2 = -inf is staged as +inf: exp2(s - lse2) = 0 for every s (see pds)
      if constexpr (BAND) stv = tid < KT && stv == -INFINITY ? INFINITY : stv;
      if (tid < 2 * KT) reinterpret_cast<float*>(nb + 2 * TILE_BYTES)[tid] = (stv + st_add) * st_mul;
    };
    // S[q][key] and dP[q][key] for the query rows of half hq (qb = 2 hq, 2 hq + 1) of the tile
    // image sQ: lane holds q = qb*16 + 4g + i, key = kb*16 + i16
    auto sdp = [&](const char* sQ, int hq, f32x4_t (&sc)[4][2], f32x4_t (&dp)[4][2]) {
      const char* sD = sQ + TILE_BYTES;
#pragma unroll
      for (int qb = 2 * hq; qb < 2 * hq + 2; ++qb) {
        const bf16x8_t q0f = rd_row(sQ, qb * 16 + i16, g), q1f = rd_row(sQ, qb * 16 + i16, 4 + g);
        const bf16x8_t d0f = rd_row(sD, qb * 16 + i16, g), d1f = rd_row(sD, qb * 16 + i16, 4 + g);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          sc[qb][kb] = mfma(q0f, kf[kb][0], f32x4_t{0.f, 0.f, 0.f, 0.f});
          sc[qb][kb] = mfma(q1f, kf[kb][1], sc[qb][kb]);
          dp[qb][kb] = mfma(d0f, vf[kb][0], f32x4_t{0.f, 0.f, 0.f, 0.f});
          dp[qb][kb] = mfma(d1f, vf[kb][1], dp[qb][kb]);
        }
      }
    };
    // P_d and dS in place for half hq (sc <- P_d = P * keep / (1-p); dp <- dS = P * (keep * dP /
    // (1-p) - delta) = P_d * dP - (P / (1-p)) * (delta * (1-p))): exp2, and per element one keep
    // test, one select, one multiply and one FMA. Keys >= len are not masked here: a key's P and
    // dS feed only its own dK / dV rows (the key is the MFMA column), which are zeroed at the
    // store. Dropout: keys k0 + i16 and k0 + 16 + i16 (kb = 0, 1) are the halves of pair
    // k0/2 + i16 — one hash per query row, no lane exchange.
    auto hashes = [&](uint32_t hrow, int hq, uint32_t (&hh)[2][4]) {
      if constexpr (DROP)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            hh[u][i] = attn_hash_input(key, hrow + static_cast<uint32_t>((2 * hq + u) * 16 + i) * 0x9E3779B1u);
    };
    // DIAG (causal, diagonal tile): query < key <=> qb*16 + i - kb*16 < kd, kd = key - (tile's
    // first query + 4g) of the lane's kb = 0 key; the score is -inf there, so P_d = 0 and dS = 0
    // exactly (masking the score, not p, also keeps this form free of spills).
    auto pds = [&](const float* sL, const uint32_t (&hq_hash)[2][4], int hq, f32x4_t (&sc)[4][2], f32x4_t (&dp)[4][2],
                   auto diag_c, int kd, const BandRows& br) {
      constexpr bool DIAG = decltype(diag_c)::value;
      const float* sDel = sL + KT;
#pragma unroll
      for (int qb = 2 * hq; qb < 2 * hq + 2; ++qb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ql = qb * 16 + 4 * g + i;
          const float lse2 = sL[ql], del = sDel[ql];
          const uint32_t hh = hq_hash[qb - 2 * hq][i];
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) {
            float sv = sc[qb][kb][i];
            if constexpr (DIAG && !BAND) sv = qb * 16 + i - kb * 16 < kd ? -INFINITY : sv;
            // BAND (kd: the tile's first query + 4g): the query lies outside this key's range; the
            // select gives p = exp2(-inf) = 0 and dS = 0 exactly — also in a padding row, whose
            // lse2 = -inf was staged as +inf (store()), never exp2(-inf + inf)
            if constexpr (DIAG && BAND) sv = br.masked(kb, kd + qb * 16 + i) ? -INFINITY : sv;
            const float p = fast_exp2(__builtin_fmaf(sv, P.scale_log2, -lse2));
            const float dpv = dp[qb][kb][i];
            if constexpr (DROP) {
              const float pd = attn_keep_half(hh, kb, P.drop_thr) ? p : 0.f;
              sc[qb][kb][i] = pd;
              dp[qb][kb][i] = __builtin_fmaf(pd, dpv, -(p * del));
            } else {
              sc[qb][kb][i] = p;
              dp[qb][kb][i] = p * (dpv - del);
            }
          }
        }
    };
    // dV^T += dO^T P_d ; dK^T += Q^T dS over the 32 queries of half ks
    auto pv = [&](const char* sQ, int ks, const f32x4_t (&sc)[4][2], const f32x4_t (&dp)[4][2]) {
      const char* sD = sQ + TILE_BYTES;
      bf16x8_t pfr[2], sfr[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        pfr[kb] = pack_frag(sc[2 * ks][kb], sc[2 * ks + 1][kb]);
        sfr[kb] = pack_frag(dp[2 * ks][kb], dp[2 * ks + 1][kb]);
      }
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const bf16x8_t dof = rd_col(sD, ks * 32, ks * 32 + 16, db * 16, lane);
        const bf16x8_t qcf = rd_col(sQ, ks * 32, ks * 32 + 16, db * 16, lane);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          dv[kb][db] = mfma(dof, pfr[kb], dv[kb][db]);
          dk[kb][db] = mfma(qcf, sfr[kb], dk[kb][db]);
        }
      }
    };
    // one tile from LDS buffer BUFI (compile-time: every LDS address is a lane base plus an
    // immediate); the next tile's global loads are in flight meanwhile and stored into the other
    // buffer at the end
    f32x4_t sc[4][2], dp[4][2];
    // diag_c (causal): a tile of the diagonal trip — masked in pds, and skipped by a wave whose
    // keys all lie above the tile's last query (wave-uniform)
    // nq: the tile to stage meanwhile (the next one of this head, or a GQA group's next head's
    // first), if nxt
    auto tile = [&](int qt, int nq, bool nxt, auto bufi_c, auto diag_c) {
      constexpr int BUFI = decltype(bufi_c)::value;
      constexpr bool DIAG = decltype(diag_c)::value;
      constexpr int DV = DIAG ? 2 : 0;  // the mask's compare and select per element, per MFMA slot
      const int kd = BAND ? qt * KT + 4 * g : k0 + i16 - qt * KT - 4 * g;
      if constexpr (!GQA) {  // always the head's next tile; the two arguments are not read
        nq = qt + 1;
        nxt = qt + 1 < ntiles;
      }
      nxt = nxt && !(MODE & 2);
      if (nxt) load(nq);
      if (!DIAG || (BAND ? !band.skip(qt * KT, KT) : __builtin_amdgcn_readfirstlane(k0) <= qt * KT + KT - 1)) {
        const char* sQ = smem + BUFI * BUF;
        const float* sL = reinterpret_cast<const float*>(sQ + 2 * TILE_BYTES);
        const uint32_t hrow = DROP ? attn_row_term(static_cast<uint32_t>(bh * P.S + qt * KT + 4 * g)) +
                                         (static_cast<uint32_t>(k0 >> 1) + i16) * kAttnPairMul
                                   : 0u;
        // four phases, MFMA work beside independent VALU work of the same wave, spread one MFMA per
        // few VALU instructions by sched_group_barrier:
        //   S/dP(rows 0-31) + hashes(rows 0-31) | S/dP(rows 32-63) + P/dS(rows 0-31) + hashes(rows
        //   32-63) | dV/dK(rows 0-31) + P/dS(rows 32-63) | dV/dK(rows 32-63)
        uint32_t h0[2][4] = {}, h1[2][4] = {};
        sdp(sQ, 0, sc, dp);
        hashes(hrow, 0, h0);
        // BAND, masked form: the ranges of this lane's two keys, read again per tile (four more
        // registers live across the loop spill)
        BandRows br;
        if constexpr (DIAG && BAND) br.rows<true>(P, b, k0, i16);
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, DROP ? 3 : 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        sdp(sQ, 1, sc, dp);
        if constexpr (!(MODE & 1)) pds(sL, h0, 0, sc, dp, diag_c, kd, br);
        hashes(hrow, 1, h1);
        __builtin_amdgcn_sched_group_barrier(0x100, 12, 1);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
          __builtin_amdgcn_sched_group_barrier(0x002, (DROP ? 10 : 6) + DV, 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        pv(sQ, 0, sc, dp);
        if constexpr (!(MODE & 1)) pds(sL, h1, 1, sc, dp, diag_c, kd, br);
        __builtin_amdgcn_sched_group_barrier(0x100, 20, 2);
        __builtin_amdgcn_sched_group_barrier(0x002, 8, 2);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 2);
          __builtin_amdgcn_sched_group_barrier(0x002, (DROP ? 8 : 5) + DV, 2);
        }
        __builtin_amdgcn_sched_barrier(0);
        pv(sQ, 1, sc, dp);
      }
      if (nxt) store(smem + (BUFI ^ 1) * BUF);
      if constexpr (!(MODE & 4)) __syncthreads();
    };
    using std::integral_constant;
    using std::false_type;
    using std::true_type;
    const int qt0 = BAND ? band.t0 : CAUSAL ? 2 * kblk : 0;
    // BAND, wave-uniform: the two tiles of the trip from tile q lie inside the range of every key of
    // this wave — the unmasked body; the waves of a workgroup may differ (each form has the trip's
    // two barriers)
    auto band_full = [&](int q) { return band.full(q * KT, 2 * KT); };
    load(qt0);
    store(smem);
    __syncthreads();
    if constexpr ((MODE & 8) != 0) stamp[1] = __builtin_amdgcn_s_memtime();
    int qt = qt0;
    if constexpr (!GQA) {
      if constexpr (CAUSAL) {
        // the diagonal trip: waves 0, 1 (keys 0-63 of the block) mask in tile qt0 (and see all of
        // tile qt0 + 1: its compares never hit); waves 2, 3 (keys 64-127) skip tile qt0 and mask in
        // tile qt0 + 1
        tile(qt, 0, false, integral_constant<int, 0>{}, true_type{});
        tile(qt + 1, 0, false, integral_constant<int, 1>{}, true_type{});
        qt += 2;
      }
      if constexpr (BAND) {
        // runs of masked trips and runs of unmasked trips, a loop each (one loop that chooses per
        // trip spills 200-280 bytes)
        while (qt < ntiles) {
          for (; qt < ntiles && !band_full(qt); qt += 2) {
            tile(qt, 0, false, integral_constant<int, 0>{}, true_type{});
            tile(qt + 1, 0, false, integral_constant<int, 1>{}, true_type{});
          }
          for (; qt < ntiles && band_full(qt); qt += 2) {
            tile(qt, 0, false, integral_constant<int, 0>{}, false_type{});
            tile(qt + 1, 0, false, integral_constant<int, 1>{}, false_type{});
          }
        }
      } else {
        for (; qt < ntiles; qt += 2) {  // ntiles - qt is even
          tile(qt, 0, false, integral_constant<int, 0>{}, false_type{});
          tile(qt + 1, 0, false, integral_constant<int, 1>{}, false_type{});
        }
      }
    } else {
      // Grouped-query attention: the G query heads of this key/value head in head order, each
      // swept from qt0 to the end into the same dk / dv accumulators. A head's last tile (always
      // in buffer 1) stages the next head's tile qt0 into buffer 0, so the register-staged
      // prefetch and the one barrier per tile carry across the head boundary and no prologue is
      // repeated: the loaders and st_src move on one head before that tile, bh (the dropout row
      // ids) after it. Causal: every head's first trip is a diagonal trip.
      int heads_left = P.G;
      auto trip = [&](auto diag_c) {
        const bool last = qt + 2 >= ntiles;  // this trip ends the head
        tile(qt, qt + 1, true, integral_constant<int, 0>{}, diag_c);
        if (last) {
          --heads_left;
          lq.lanep += D;
          ld.lanep += D;
          st_src += P.S;
        }
        tile(qt + 1, last ? qt0 : qt + 2, !last || heads_left > 0, integral_constant<int, 1>{}, diag_c);
        qt = last ? qt0 : qt + 2;
        return last;
      };
      // (two loop shapes for one sequence of trips, chosen by the register allocation they get:
      // the causal kernels spill 104 / 248 bytes in the flat shape, the bidirectional one without
      // dropout 24 bytes in the nested shape; as written every instantiation has no scratch)
      if constexpr (BAND) {
        // (runs of masked and of unmasked trips, a loop each, as above. Without dropout that shape —
        // and every other one tried — spills 12 bytes or more, so that one instantiation runs the
        // masked body on every trip: the compare on the unmasked tiles too, but no scratch)
        if constexpr (!DROP) {
          do {
            if (trip(true_type{})) ++bh;
          } while (heads_left > 0);
        } else {
          do {
            bool last = false;
            while (!last && !band_full(qt)) last = trip(true_type{});
            while (!last && band_full(qt)) last = trip(false_type{});
            while (!last) last = trip(true_type{});
            ++bh;
          } while (heads_left > 0);
        }
      } else if constexpr (CAUSAL) {
        do {
          bool last = trip(true_type{});
          while (!last) last = trip(false_type{});
          ++bh;
        } while (heads_left > 0);
      } else {
        do {
          if (trip(false_type{})) ++bh;
        } while (heads_left > 0);
      }
    }
    if constexpr ((MODE & 8) != 0) stamp[2] = __builtin_amdgcn_s_memtime();
  }
  // store dK (scaled by 1/sqrt(D)) and dV: lane holds key kb*16 + i16, d = db*16 + 4g + i; keys
  // >= len get zeros (their accumulators saw unmasked probabilities)
  if constexpr (BAND) band.rows<true>(P, b, k0, i16);
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const long long row = tokk + k0 + kb * 16 + i16;
    bf16_t* pk = P.out + row * P.ld_out + hk * D + 4 * g;
    bf16_t* pv = P.out2 + row * P.ld_out2 + hk * D + 4 * g;
    const bool valid = BAND ? band.w[kb] > 0 : k0 + kb * 16 + i16 < len;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
      const f32x4_t a = valid ? dk[kb][db] * P.scale : zero, c = valid ? dv[kb][db] : zero;
      *reinterpret_cast<uint2*>(pk + db * 16) = make_uint2(pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]));
      if constexpr ((MODE & 8) == 0)
        *reinterpret_cast<uint2*>(pv + db * 16) = make_uint2(pack_bf16x2(c[0], c[1]), pack_bf16x2(c[2], c[3]));
    }
  }
  if constexpr ((MODE & 8) != 0) {
    __builtin_amdgcn_s_waitcnt(0);
    stamp[3] = __builtin_amdgcn_s_memtime();
    stamp[5] = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) {
      long long* o = reinterpret_cast<long long*>(P.out2) + static_cast<long long>(blockIdx.x) * 8;
#pragma unroll
      for (int j = 0; j < 6; ++j) o[j] = stamp[j];
      o[6] = t;
      o[7] = __smid();
    }
  }
}

// ------------------------------------------------------------------------------ bwd dQ
// CAUSAL: as the forward — key tiles kt <= 2 qblk + 1 only; per wave a tile runs full, diagonal
// (score -inf where key > query, before the exp2: P = 0 and dS = 0 exactly) or skipped.
// GQA: as the forward — K / V tiles from key/value head h / G.
// BAND: as the forward — key tiles kt0 .. kt1 - 1 of the block's record; per wave a tile runs full
// (inside every row's range), masked or skipped (outside every row's range). A masked element gets
// a score of -inf by select, so P = 0 and dS = 0 exactly; a padding row's lse = -inf is read as +inf.
template <bool DROP, bool CAUSAL = false, bool GQA = false, bool BAND = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_q_kernel(AttnParams P) {
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
  const int len = BAND ? P.Sk : P.seqlen ? min(P.seqlen[b], P.Sk) : P.Sk;  // BAND: in the table
  const long long tok0 = static_cast<long long>(b) * P.S;    // query rows: Q, O, dO, dQ
  const long long tokk = static_cast<long long>(b) * P.Sk;   // key rows: K, V, dK, dV
  BandRows band;
  if constexpr (BAND) band.init<false>(P, b, qblk, q0, i16);

  bf16x8_t qf[2][2], df[2][2];
  float lse2[2], del[2];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const long long row = tok0 + q0 + qb * 16 + i16;
    float acc = 0.f;  // this lane's 16 of the row's 64 dims of dO . O
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[qb][ks] = ldg_frag(P.q + row * P.ldq + h * D + ks * 32 + g * 8);
      df[qb][ks] = ldg_frag(P.dout + row * P.lddo + h * D + ks * 32 + g * 8);
      float a[8], d[8];
      unpack8(ldg16(P.o + row * P.ldo + h * D + ks * 32 + g * 8), a);
      unpack8(__builtin_bit_cast(uint4, df[qb][ks]), d);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += a[j] * d[j];
    }
    // the 4 lane groups g hold the row's 4 slices
    acc = tile::rows4_sum(acc);
    del[qb] = acc;
    const long long srow = static_cast<long long>(bh) * P.S + q0 + qb * 16 + i16;
    lse2[qb] = P.lse[srow];
    // BAND: a padding row (lse2 = -inf; all its keys masked, s = -inf) takes +inf here, so that
    // exp2(s - lse2) is exp2(-inf) = 0 and dS = 0 exactly, never exp2(-inf + inf)
    if constexpr (BAND) lse2[qb] = lse2[qb] == -INFINITY ? INFINITY : lse2[qb];
    if (g == 0) P.delta[srow] = acc;
    if constexpr (DROP) {
      // dS = P * (keep * dP / (1-p) - delta) = P_d' * dP - P' * (delta * (1-p)) with P' = P / (1-p)
      // = exp2(s - (lse2 - log2(1/(1-p)))) and P_d' = keep ? P' : 0
      lse2[qb] -= __builtin_amdgcn_logf(P.drop_scale);
      del[qb] *= 1.f / P.drop_scale;
    }
  }
  f32x4_t dq[2][4];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int db = 0; db < 4; ++db) dq[qb][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  TileLoader lk, lv;
  const int hk = GQA ? h / P.G : h;  // the key/value head of query head h
  lk.init(P.k + tokk * P.ldk + hk * D, P.ldk, tid);
  lv.init(P.v + tokk * P.ldv + hk * D, P.ldv, tid);
  const uint32_t key = DROP ? drop_key(P.rng, P.site) : 0u;
  int ntiles = (len + KT - 1) / KT;
  if constexpr (CAUSAL) ntiles = min(ntiles, 2 * qblk + 2);
  int kt0 = 0;
  if constexpr (BAND) {
    kt0 = band.t0;
    ntiles = band.t1;
  }
  if (ntiles > kt0) {
    lk.load(kt0 * KT, len);
    lv.load(kt0 * KT, len);
    lk.store(smem);
    lv.store(smem + TILE_BYTES);
  }
  __syncthreads();
  // S, dP for the keys of half hk (kb = 2 hk, 2 hk + 1) of the tile: lane holds keys
  // kb*16 + 4g + i of query qb*16 + i16
  auto sdp = [&](const char* sK, int hk, f32x4_t (&sc)[2][4], f32x4_t (&dp)[2][4]) {
    const char* sV = sK + TILE_BYTES;
#pragma unroll
    for (int kb = 2 * hk; kb < 2 * hk + 2; ++kb) {
      const bf16x8_t k0f = rd_row(sK, kb * 16 + i16, g), k1f = rd_row(sK, kb * 16 + i16, 4 + g);
      const bf16x8_t v0f = rd_row(sV, kb * 16 + i16, g), v1f = rd_row(sV, kb * 16 + i16, 4 + g);
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        sc[qb][kb] = mfma(k0f, qf[qb][0], f32x4_t{0.f, 0.f, 0.f, 0.f});
        sc[qb][kb] = mfma(k1f, qf[qb][1], sc[qb][kb]);
        dp[qb][kb] = mfma(v0f, df[qb][0], f32x4_t{0.f, 0.f, 0.f, 0.f});
        dp[qb][kb] = mfma(v1f, df[qb][1], dp[qb][kb]);
      }
    }
  };
  // dropout pair hashes of the tile at kbase for key half hk (pairs as in the forward kernel:
  // kb = 2 hk, 2 hk + 1 at the same i share one)
  auto hashes = [&](int kbase, int hk, uint32_t (&hp)[2][4]) {
    if constexpr (DROP)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        const uint32_t hbase = attn_row_term(static_cast<uint32_t>(bh * P.S + q0 + qb * 16 + i16)) +
                               (static_cast<uint32_t>(kbase >> 1) + 4u * g + 16u * hk) * kAttnPairMul;
#pragma unroll
        for (int i = 0; i < 4; ++i) hp[qb][i] = attn_hash_input(key, hbase + static_cast<uint32_t>(i) * kAttnPairMul);
      }
  };
  // dS in place for key half hk. (DROP: lse2 / del carry the dropout scale, p is P / (1-p) — see
  // the prologue.) Keys >= len need no mask: their K rows are zero-filled in LDS, so whatever dS
  // they get adds nothing to dQ = dS K (and their S = 0, dP = 0 keep dS finite).
  // DIAG (causal, diagonal tile): key > query <=> kb*16 + i - qb*16 > qd, qd = the lane's qb = 0
  // query - (tile's first key + 4g).
  auto pds = [&](int hk, const uint32_t (&hp)[2][4], f32x4_t (&sc)[2][4], const f32x4_t (&dp)[2][4], auto diag_c,
                 int qd) {
    constexpr bool DIAG = decltype(diag_c)::value;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int kb = 2 * hk; kb < 2 * hk + 2; ++kb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float sv = sc[qb][kb][i];
          if constexpr (DIAG && !BAND) sv = kb * 16 + i - qb * 16 > qd ? -INFINITY : sv;
          // BAND (qd: the tile's first key + 4g): the key lies outside this row's range
          if constexpr (DIAG && BAND) sv = band.masked(qb, qd + kb * 16 + i) ? -INFINITY : sv;
          const float p = fast_exp2(__builtin_fmaf(sv, P.scale_log2, -lse2[qb]));
          const float dpv = dp[qb][kb][i];
          if constexpr (DROP) {
            const float pd = attn_keep_half(hp[qb][i], kb & 1, P.drop_thr) ? p : 0.f;
            sc[qb][kb][i] = __builtin_fmaf(pd, dpv, -(p * del[qb]));
          } else {
            sc[qb][kb][i] = p * (dpv - del[qb]);
          }
        }
  };
  // dQ += dS K over the 32 keys of half ks
  auto dqh = [&](const char* sK, int ks, const f32x4_t (&sc)[2][4]) {
    bf16x8_t sfr[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) sfr[qb] = pack_frag(sc[qb][2 * ks], sc[qb][2 * ks + 1]);
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const bf16x8_t kc = rd_col(sK, ks * 32, ks * 32 + 16, db * 16, lane);
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) dq[qb][db] = mfma(kc, sfr[qb], dq[qb][db]);
    }
  };
  // one 64-key tile in four phases (as attn_bwd_kv_kernel): S/dP(keys 0-31) + hashes | S/dP(keys
  // 32-63) + dS(keys 0-31) | dQ(keys 0-31) + dS(keys 32-63) | dQ(keys 32-63)
  int cur = 0;
  f32x4_t sc[2][4], dp[2][4];
  // FORM (causal): 0 full tile, 1 diagonal tile, 2 skipped by this wave
  auto tile = [&](int kt, auto form_c) {
    constexpr int FORM = decltype(form_c)::value;
    const std::integral_constant<bool, FORM == 1> diag_c{};
    const bool nxt = kt + 1 < ntiles;
    if (nxt) {
      lk.load((kt + 1) * KT, len);
      lv.load((kt + 1) * KT, len);
    }
    if constexpr (FORM == 2) {
      if (nxt) {
        lk.store(smem + (cur ^ 1) * 2 * TILE_BYTES);
        lv.store(smem + (cur ^ 1) * 2 * TILE_BYTES + TILE_BYTES);
      }
      __syncthreads();
      cur ^= 1;
      return;
    }
    const char* sK = smem + cur * 2 * TILE_BYTES;
    const int kbase = kt * KT;
    const int qd = BAND ? kbase + 4 * g : q0 + i16 - kbase - 4 * g;
    uint32_t h0[2][4] = {}, h1[2][4] = {};
    sdp(sK, 0, sc, dp);
    hashes(kbase, 0, h0);
    hashes(kbase, 1, h1);
    __builtin_amdgcn_sched_barrier(0);
    sdp(sK, 1, sc, dp);
    pds(0, h0, sc, dp, diag_c, qd);
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 1);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
      __builtin_amdgcn_sched_group_barrier(0x002, DROP ? 6 : 4, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    dqh(sK, 0, sc);
    pds(1, h1, sc, dp, diag_c, qd);
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 2);
    __builtin_amdgcn_sched_group_barrier(0x002, 4, 2);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 2);
      __builtin_amdgcn_sched_group_barrier(0x002, DROP ? 12 : 8, 2);
    }
    __builtin_amdgcn_sched_barrier(0);
    dqh(sK, 1, sc);
    if (nxt) {
      lk.store(smem + (cur ^ 1) * 2 * TILE_BYTES);
      lv.store(smem + (cur ^ 1) * 2 * TILE_BYTES + TILE_BYTES);
    }
    __syncthreads();
    cur ^= 1;
  };
  for (int kt = kt0; kt < ntiles; ++kt) {
    if constexpr (BAND) {
      // wave-uniform: outside every row's range | some row's range ends inside the tile
      if (band.skip(kt * KT, KT)) tile(kt, std::integral_constant<int, 2>{});
      else if (!band.full(kt * KT, KT)) tile(kt, std::integral_constant<int, 1>{});
      else tile(kt, std::integral_constant<int, 0>{});
    } else if constexpr (CAUSAL) {
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
    for (int db = 0; db < 4; ++db) {
      const f32x4_t v = dq[qb][db] * P.scale;
      *reinterpret_cast<uint2*>(op + db * 16) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
  }
}

// ------------------------------------------------------------------------------ fused bwd
// dQ, dK and dV of one (batch, head) in ONE workgroup (S = 64 * NKB <= 512 keys): five MFMA
// products per (query slice, key tile) instead of the split kernels' seven (both recompute S and
// dP), every dropout hash computed once instead of twice, delta = rowsum(dO . O) formed while the
// query slice is staged, and no cross-workgroup sum for dQ (deterministic, no atomics).
//   * 4 waves, one per SIMD (launch_bounds(256, 1): 512 registers per lane); wave w owns keys
//     [w*16*NKB, (w+1)*16*NKB): its dK^T and dV^T live in accumulators for the whole sweep (key
//     on the MFMA lane, so the S / dP accumulators are already the B operands of dV^T += dO^T P
//     and dK^T += Q^T dS), its V fragments in registers;
//   * LDS: K of all S keys (S rows for the Q.K^T B operand, K^T column reads for dQ), dS^T of
//     the slice for all keys (two 32-column halves, alternating per slice), and the 32-query
//     slice of Q / dO / lse / delta double-buffered (register-staged one slice ahead);
//   * per slice: S, dP -> P, dS for each pair of 16-key tiles; dV^T, dK^T accumulate; dS^T to
//     LDS; one barrier; dQ[32 x 64] = dS . K split over the 4 waves (16 columns each), stored.
template <int NKB, int NW, bool DROP>
__global__ __launch_bounds__(NW * 64, 1) void attn_bwd_fused_kernel(AttnParams P) {
  constexpr int NT = NW * 64;
  constexpr int SK = 16 * NKB * NW;      // keys = queries of one (b, h)
  constexpr int QS = 32;                 // queries per slice
  constexpr int IMG = SK * 128;          // [SK][64] bf16 image
  constexpr int QT = QS * 128;           // [32][64] bf16 slice image
  constexpr int STAGE = 2 * QT + 2 * QS * 4;
  __shared__ __attribute__((aligned(16))) char smem[2 * IMG + 2 * STAGE];
  char* const sK = smem;
  char* const sDS = smem + IMG;
  char* const sStage = smem + 2 * IMG;
  const int bh = tile::xcd_remap(blockIdx.x, gridDim.x);
  const int b = bh / P.H, h = bh - b * P.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int key0 = wave * 16 * NKB;
  const int len = P.seqlen ? min(P.seqlen[b], SK) : SK;
  const long long tok0 = static_cast<long long>(b) * SK;
  const uint32_t key = DROP ? drop_key(P.rng, P.site) : 0u;

  // K image of all keys (keys >= len zeroed: their dS is 0, keep 0 * K finite)
  for (int c = tid; c < SK * 8; c += NT) {
    const int row = c >> 3, ch = c & 7;
    const uint4 v = row < len ? ldg16(P.k + (tok0 + row) * P.ldk + h * D + ch * 8) : make_uint4(0, 0, 0, 0);
    *reinterpret_cast<uint4*>(sK + tile::off64(row, ch * 8)) = v;
  }
  bf16x8_t vf[NKB][2];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      vf[kb][ks] = ldg_frag(P.v + (tok0 + key0 + kb * 16 + i16) * P.ldv + h * D + ks * 32 + g * 8);
  f32x4_t dk[NKB][4], dv[NKB][4];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int db = 0; db < 4; ++db) dk[kb][db] = dv[kb][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // slice staging: thread t moves row (t & 255) >> 3, 16-B chunk t & 7 of Q, dO and O (delta
  // partial); with 512 threads the first 256 take Q, the others dO and O
  constexpr bool SPLIT_STAGE = NT >= 512;
  const int srow = (tid & 255) >> 3, sch = tid & 7;
  const bool do_q = !SPLIT_STAGE || tid < 256, do_d = !SPLIT_STAGE || (tid >= 256 && tid < 512);
  uint4 rq = make_uint4(0, 0, 0, 0), rd = rq, ro = rq;
  float rl = 0.f;
  auto stage_load = [&](int s) {
    const long long row = tok0 + s * QS + srow;
    if (do_q) rq = ldg16(P.q + row * P.ldq + h * D + sch * 8);
    if (do_d) {
      rd = ldg16(P.dout + row * P.lddo + h * D + sch * 8);
      ro = ldg16(P.o + row * P.ldo + h * D + sch * 8);
    }
    if (tid < QS) rl = P.lse[static_cast<long long>(bh) * SK + s * QS + tid];
  };
  auto stage_store = [&](int buf) {
    char* st = sStage + buf * STAGE;
    if (do_q) *reinterpret_cast<uint4*>(st + tile::off64(srow, sch * 8)) = rq;
    float* stats = reinterpret_cast<float*>(st + 2 * QT);
    if (tid < QS) stats[tid] = rl;
    if (!do_d) return;
    *reinterpret_cast<uint4*>(st + QT + tile::off64(srow, sch * 8)) = rd;
    float a[8], d[8];
    unpack8(ro, a);
    unpack8(rd, d);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += a[j] * d[j];
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (sch == 0) stats[QS + srow] = acc;
  };
  constexpr int NSL = SK / QS;
  stage_load(0);
  stage_store(0);
  __syncthreads();

  for (int s = 0; s < NSL; ++s) {
    const int cur = s & 1;
    if (s + 1 < NSL) stage_load(s + 1);
    const char* sQ = sStage + cur * STAGE;
    const char* sD = sQ + QT;
    const float* sL = reinterpret_cast<const float*>(sQ + 2 * QT);
    const int dcol = cur * 32;  // dS^T columns of this slice
#pragma unroll
    for (int pp = 0; pp < NKB / 2; ++pp) {
      const int k0 = key0 + pp * 32;
      // Q / dO row fragments (re-read from LDS per key pair: registers go to dK^T, dV^T, V)
      bf16x8_t qf[2][2], df[2][2];
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          qf[qb][ks] = rd_row(sQ, qb * 16 + i16, ks * 4 + g);
          df[qb][ks] = rd_row(sD, qb * 16 + i16, ks * 4 + g);
        }
      // S[q][key], dP[q][key]: lane holds q = qb*16 + 4g + i, key = k0 + j*16 + i16
      f32x4_t sc[2][2], dp[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16x8_t k0f = rd_row(sK, k0 + j * 16 + i16, g), k1f = rd_row(sK, k0 + j * 16 + i16, 4 + g);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          sc[qb][j] = mfma(qf[qb][0], k0f, f32x4_t{0.f, 0.f, 0.f, 0.f});
          sc[qb][j] = mfma(qf[qb][1], k1f, sc[qb][j]);
          dp[qb][j] = mfma(df[qb][0], vf[2 * pp + j][0], f32x4_t{0.f, 0.f, 0.f, 0.f});
          dp[qb][j] = mfma(df[qb][1], vf[2 * pp + j][1], dp[qb][j]);
        }
      }
      // P, dS in place (sc <- P * keep * scale, dp <- dS). Dropout: keys k0 + i16 and k0 + 16 + i16
      // (j = 0, 1) are the two halves of pair k0/2 + i16: one hash per lane per query row
      const uint32_t pair = static_cast<uint32_t>(k0 >> 1) + i16;
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        // this lane's query rows qb*16 + 4g + i: lse2 and delta
        const f32x4_t ls = *reinterpret_cast<const f32x4_t*>(sL + qb * 16 + 4 * g);
        const f32x4_t dl = *reinterpret_cast<const f32x4_t*>(sL + QS + qb * 16 + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t hh = 0u;
          if constexpr (DROP) {
            const int qg = s * QS + qb * 16 + 4 * g + i;
            hh = attn_pair_hash(key, attn_row_term(static_cast<uint32_t>(bh * SK + qg)), pair);
          }
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int kcol = k0 + j * 16 + i16;
            const float p = kcol < len ? fast_exp2(sc[qb][j][i] * P.scale_log2 - ls[i]) : 0.f;
            float dpv = dp[qb][j][i];
            float pd = p;
            if constexpr (DROP) {
              const bool kp = attn_keep_half(hh, j, P.drop_thr);
              pd = kp ? p * P.drop_scale : 0.f;
              dpv = kp ? dpv * P.drop_scale : 0.f;
            }
            sc[qb][j][i] = pd;
            dp[qb][j][i] = p * (dpv - dl[i]);
          }
        }
      }
      bf16x8_t pfr[2], sfr[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        pfr[j] = pack_frag(sc[0][j], sc[1][j]);
        sfr[j] = pack_frag(dp[0][j], dp[1][j]);
        // dS^T rows (keys) x this slice's 32 query columns, for dQ
        const uint4 w = __builtin_bit_cast(uint4, sfr[j]);
        *reinterpret_cast<uint2*>(sDS + tile::off64(k0 + j * 16 + i16, dcol + 4 * g)) = make_uint2(w.x, w.y);
        *reinterpret_cast<uint2*>(sDS + tile::off64(k0 + j * 16 + i16, dcol + 16 + 4 * g)) = make_uint2(w.z, w.w);
      }
      // dV^T += dO^T P ; dK^T += Q^T dS (contraction over the slice's 32 queries)
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const bf16x8_t dof = rd_col(sD, 0, 16, db * 16, lane);
        const bf16x8_t qcf = rd_col(sQ, 0, 16, db * 16, lane);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          dv[2 * pp + j][db] = mfma(dof, pfr[j], dv[2 * pp + j][db]);
          dk[2 * pp + j][db] = mfma(qcf, sfr[j], dk[2 * pp + j][db]);
        }
      }
    }
    if (s + 1 < NSL) stage_store(cur ^ 1);
    __syncthreads();
    // dQ^T[d][q] of the slice: 8 tiles of 16 d x 16 q, tile t = (qb = t >> 2, db = t & 3);
    // wave w takes tiles w, w + NW, ...
    constexpr int TPW = 8 / NW;
    f32x4_t dq[TPW];
#pragma unroll
    for (int u = 0; u < TPW; ++u) dq[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int ks = 0; ks < SK / 32; ++ks) {
#pragma unroll
      for (int u = 0; u < TPW; ++u) {
        const int t = wave + u * NW, qb = t >> 2, db = t & 3;
        dq[u] = mfma(rd_col(sK, ks * 32, ks * 32 + 16, db * 16, lane),
                     rd_col(sDS, ks * 32, ks * 32 + 16, dcol + qb * 16, lane), dq[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      const int t = wave + u * NW, qb = t >> 2, db = t & 3;
      const f32x4_t v = dq[u] * P.scale;
      bf16_t* op = P.out + (tok0 + s * QS + qb * 16 + i16) * P.ld_out + h * D + db * 16 + 4 * g;
      *reinterpret_cast<uint2*>(op) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
  }
  // dK (scaled by 1/sqrt(D)) and dV: lane holds key key0 + kb*16 + i16, d = db*16 + 4g + i
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const long long row = tok0 + key0 + kb * 16 + i16;
    bf16_t* pk = P.out2 + row * P.ld_out2 + h * D + 4 * g;
    bf16_t* pv = P.out3 + row * P.ld_out3 + h * D + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const f32x4_t a = dk[kb][db] * P.scale, c = dv[kb][db];
      *reinterpret_cast<uint2*>(pk + db * 16) = make_uint2(pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]));
      *reinterpret_cast<uint2*>(pv + db * 16) = make_uint2(pack_bf16x2(c[0], c[1]), pack_bf16x2(c[2], c[3]));
    }
  }
}

// ------------------------------------------------------------------------------ band table
// One workgroup per batch row builds the BAND kernels' table (AttnParams::band_tok / band_blk) from
// segment ids (a token attends its own maximal run of equal ids; id < 0: padding), the key length,
// the window (wl / wr < 0: unbounded) — causal is wr = 0 by now. Linear in S: thread t owns a
// contiguous chunk of tokens; the run start of a token is the last run boundary at or before it,
// the run end the first boundary after it — a carry across the chunks (through LDS) and one pass
// over the chunk each way. Then wave w reduces the records of blocks w, w + 4, ... to tile ranges.
__global__ __launch_bounds__(256) void attn_band_kernel(const int* ids, const int* seqlen, int S, int wl, int wr,
                                                        int4* tok, int4* blk) {
  __shared__ int s_last[256], s_first[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const int per = (S + 255) / 256;
  const int c0 = min(t * per, S), c1 = min(c0 + per, S);
  const int* id = ids ? ids + static_cast<long long>(b) * S : nullptr;
  const int len = seqlen ? min(max(seqlen[b], 0), S) : S;
  int4* row = tok + static_cast<long long>(b) * S;
  auto starts = [&](int s) { return s == 0 || (id != nullptr && id[s] != id[s - 1]); };
  int last = 0, first = S;  // the chunk's last and first run boundary
  for (int s = c1 - 1; s >= c0; --s)
    if (starts(s)) {
      first = s;
      last = max(last, s);
    }
  s_last[t] = last;
  s_first[t] = first;
  __syncthreads();
  int rs = 0, nx = S;  // the run start carried into the chunk, the first boundary after it
  for (int u = 0; u < t; ++u) rs = max(rs, s_last[u]);
  for (int u = t + 1; u < 256; ++u) nx = min(nx, s_first[u]);
  for (int s = c0; s < c1; ++s) {
    if (starts(s)) rs = s;
    row[s].x = rs;
  }
  for (int s = c1 - 1; s >= c0; --s) {
    const int r0 = row[s].x, r1 = nx;  // the run [r0, r1) of token s
    if (starts(s)) nx = s;
    int klo = r0, khi = min(r1, len), qlo = r0, qhi = r1;
    if (wl >= 0) {
      klo = max(klo, s - wl);
      qhi = min(qhi, s + wl + 1);
    }
    if (wr >= 0) {
      khi = min(khi, s + wr + 1);
      qlo = max(qlo, s - wr);
    }
    const bool pad = id != nullptr && id[s] < 0;
    const bool ek = pad || klo >= khi, eq = pad || s >= len || qlo >= qhi;
    row[s] = make_int4(ek ? S : klo, ek ? 0 : khi, eq ? S : qlo, eq ? 0 : qhi);
  }
  __syncthreads();  // the records of this row, written by this workgroup, are read back below
  const int lane = t & 63, nblk = S / QBLK;
  for (int j = t >> 6; j < nblk; j += 4) {
    const int4 a = row[j * QBLK + lane], c = row[j * QBLK + 64 + lane];
    int klo = min(a.x, c.x), khi = max(a.y, c.y), qlo = min(a.z, c.z), qhi = max(a.w, c.w);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      klo = min(klo, __shfl_xor(klo, o, 64));
      khi = max(khi, __shfl_xor(khi, o, 64));
      qlo = min(qlo, __shfl_xor(qlo, o, 64));
      qhi = max(qhi, __shfl_xor(qhi, o, 64));
    }
    // the key-side sweep in whole trips of two tiles: first tile even, end even
    if (lane == 0)
      blk[b * nblk + j] = make_int4(khi > 0 ? klo / KT : 0, (khi + KT - 1) / KT, qhi > 0 ? (qlo / KT) & ~1 : 0,
                                    (qhi + QBLK - 1) / QBLK * 2);
  }
}

AttnParams make_params(int B, int H, int Hk, int S, int Sk, const int* seqlen, float p_drop, const long long* rng,
                       uint32_t site) {
  AttnParams P{};
  P.B = B;
  P.H = H;
  P.Hk = Hk;
  P.G = H / Hk;
  P.S = S;
  P.Sk = Sk;
  P.seqlen = seqlen;
  P.scale = 0.125f;  // 1/sqrt(64)
  P.scale_log2 = 0.125f * 1.4426950408889634f;
  P.drop_thr = drop_threshold16(p_drop);
  // unbiased for the keep probability the 16-bit threshold actually realises
  P.drop_scale = p_drop > 0.f ? static_cast<float>(65536.0 / (65536.0 - static_cast<double>(P.drop_thr))) : 1.f;
  P.rng = rng;
  P.site = site;
  return P;
}

// Block order of the causal grids (causal_block()): rotated unless TTD_ATTN_CAUSAL_ORDER is
// "natural" or "heavy" (kept for the A/B in profiles/attn_causal_bench.txt).
int causal_order() {
  static const int v = [] {
    const char* e = getenv("TTD_ATTN_CAUSAL_ORDER");
    if (e != nullptr && e[0] == 'n') return 0;
    if (e != nullptr && e[0] == 'h') return 1;
    return 2;
  }();
  return v;
}

// What both entry points refuse: lds is the OR of every leading dimension of the call, bases the
// pointers that have to be 16-byte aligned.
bool args_ok(int H, int Hk, int Sq, int Sk, int causal, float p_drop, const long long* rng, long long lds,
             std::initializer_list<const void*> bases) {
  if (Hk <= 0 || H % Hk || Sq <= 0 || Sk <= 0 || Sq % QBLK || Sk % QBLK || (causal && Sq != Sk) || (lds & 7) ||
      (p_drop > 0.f && !rng))
    return false;
  for (const void* p : bases)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}

// Every instantiation that is launched, indexed [gqa][causal][drop] (gqa: Hk != H).
using AttnKernel = void (*)(AttnParams);

constexpr AttnKernel kFwd[2][2][2] = {
    {{attn_fwd_kernel<false, false, false>, attn_fwd_kernel<true, false, false>},
     {attn_fwd_kernel<false, true, false>, attn_fwd_kernel<true, true, false>}},
    {{attn_fwd_kernel<false, false, true>, attn_fwd_kernel<true, false, true>},
     {attn_fwd_kernel<false, true, true>, attn_fwd_kernel<true, true, true>}}};

constexpr AttnKernel kBwdQ[2][2][2] = {
    {{attn_bwd_q_kernel<false, false, false>, attn_bwd_q_kernel<true, false, false>},
     {attn_bwd_q_kernel<false, true, false>, attn_bwd_q_kernel<true, true, false>}},
    {{attn_bwd_q_kernel<false, false, true>, attn_bwd_q_kernel<true, false, true>},
     {attn_bwd_q_kernel<false, true, true>, attn_bwd_q_kernel<true, true, true>}}};

constexpr AttnKernel kBwdKv[2][2][2] = {
    {{attn_bwd_kv_kernel<false, 0, false, false>, attn_bwd_kv_kernel<true, 0, false, false>},
     {attn_bwd_kv_kernel<false, 0, true, false>, attn_bwd_kv_kernel<true, 0, true, false>}},
    {{attn_bwd_kv_kernel<false, 0, false, true>, attn_bwd_kv_kernel<true, 0, false, true>},
     {attn_bwd_kv_kernel<false, 0, true, true>, attn_bwd_kv_kernel<true, 0, true, true>}}};

// The BAND instantiations, indexed [gqa][drop]: causal and the key length are in the table.
constexpr AttnKernel kFwdBand[2][2] = {
    {attn_fwd_kernel<false, false, false, true>, attn_fwd_kernel<true, false, false, true>},
    {attn_fwd_kernel<false, false, true, true>, attn_fwd_kernel<true, false, true, true>}};

constexpr AttnKernel kBwdQBand[2][2] = {
    {attn_bwd_q_kernel<false, false, false, true>, attn_bwd_q_kernel<true, false, false, true>},
    {attn_bwd_q_kernel<false, false, true, true>, attn_bwd_q_kernel<true, false, true, true>}};

constexpr AttnKernel kBwdKvBand[2][2] = {
    {attn_bwd_kv_kernel<false, 0, false, false, true>, attn_bwd_kv_kernel<true, 0, false, false, true>},
    {attn_bwd_kv_kernel<false, 0, false, true, true>, attn_bwd_kv_kernel<true, 0, false, true, true>}};

// TTD_ATTN_KV_DIAG=<mode>: the diagnostic forms of bwd_kv (MODE above). They are self-attention
// dropout kernels: honoured only for Hk == H, non-causal, p_drop > 0; any other value runs MODE 0.
struct KvDiag {
  int mode;
  AttnKernel kernel;
};
constexpr KvDiag kKvDiag[] = {
    {1, attn_bwd_kv_kernel<true, 1>}, {2, attn_bwd_kv_kernel<true, 2>}, {6, attn_bwd_kv_kernel<true, 6>},
    {7, attn_bwd_kv_kernel<true, 7>}, {8, attn_bwd_kv_kernel<true, 8>}, {15, attn_bwd_kv_kernel<true, 15>}};

int kv_diag() {
  static const int v = [] {
    const char* e = getenv("TTD_ATTN_KV_DIAG");
    return e ? atoi(e) : 0;
  }();
  return v;
}

// Single-kernel backward (attn_bwd_fused_kernel), one workgroup per (batch, head), for these S only;
// kernel[drop]. S = 512: 8 waves x 64 keys (two waves per SIMD); S = 256 / 128: 4 waves x 64 / 32.
struct FusedBwd {
  int S, threads;
  AttnKernel kernel[2];
};
constexpr FusedBwd kFusedBwd[] = {
    {128, 256, {attn_bwd_fused_kernel<2, 4, false>, attn_bwd_fused_kernel<2, 4, true>}},
    {256, 256, {attn_bwd_fused_kernel<4, 4, false>, attn_bwd_fused_kernel<4, 4, true>}},
    {512, 512, {attn_bwd_fused_kernel<4, 8, false>, attn_bwd_fused_kernel<4, 8, true>}}};

// The fused backward is opt-in (TTD_ATTN_FUSED_BWD=1 or ttdk_attn_set_fused_bwd(1)). Measured at
// BERT-Large b128 (S = 512, p = 0.1): 1190 us standalone vs 980 us for the split dQ / dK-dV
// kernels, BERT step 185.2 vs 177.2 ms — one workgroup per (b, h) holds 4 waves (the S = 512
// dK^T / dV^T accumulators need 256 AGPRs per lane: one wave per SIMD, LDS 145 KB: one workgroup
// per CU), too little occupancy to hide the MFMA -> softmax dependencies; the 8-wave form spills
// 65 VGPRs.
int g_attn_fused = -1;
bool attn_fused_bwd() {
  if (g_attn_fused < 0) {
    const char* e = getenv("TTD_ATTN_FUSED_BWD");
    g_attn_fused = (e != nullptr && e[0] == '1') ? 1 : 0;
  }
  return g_attn_fused != 0;
}

}  // namespace
}  // namespace ttdk

using namespace ttdk;

// The one forward / backward pair: self-attention is Hk == H, Sq == Sk.
// Shapes: head_dim 64, Sq % 128 == 0 and Sk % 128 == 0, every ld % 8 == 0 and bases 16-B aligned
// (checked). Returns hipErrorInvalidValue on violation (the Python wrapper raises).
// q / o have Sq rows per batch, k / v have Sk rows (cross-attention: the memory); lse is
// [B*H][Sq]; seqlen[b] is the keys' valid length (keys >= it masked; queries are never masked).
// causal != 0: query q attends keys k <= q (and k < seqlen[b]); needs Sq == Sk.
// Grouped-query attention: k / v hold Hk heads (Hk * 64 columns), H % Hk == 0; query head h reads
// key/value head h / (H / Hk). lse stays [B*H][Sq].
TTDK_API(int, ttdk_attn_fwd, (const bf16_t* q, long long ldq, const bf16_t* k, long long ldk, const bf16_t* v,
                              long long ldv, bf16_t* o, long long ldo, float* lse, const int* seqlen, int B, int H,
                              int Hk, int Sq, int Sk, float p_drop, const long long* rng, unsigned site, int causal,
                              hipStream_t st)) {
  if (!args_ok(H, Hk, Sq, Sk, causal, p_drop, rng, ldq | ldk | ldv | ldo, {q, k, v, o})) return hipErrorInvalidValue;
  AttnParams P = make_params(B, H, Hk, Sq, Sk, seqlen, p_drop, rng, site);
  P.q = q; P.k = k; P.v = v; P.ldq = ldq; P.ldk = ldk; P.ldv = ldv;
  P.out = o; P.ld_out = ldo; P.lse = lse;
  if (causal) P.order = causal_order();
  hipLaunchKernelGGL(kFwd[Hk != H][causal != 0][p_drop > 0.f], dim3(B * H * (Sq / QBLK)), dim3(256), 0, st, P);
  return hipGetLastError();
}

TTDK_API(int, ttdk_attn_set_fused_bwd, (int on)) {
  g_attn_fused = on ? 1 : 0;
  return 0;
}

// The backward of ttdk_attn_fwd with the same arguments. dq has Sq rows per batch, dk / dv have Sk
// rows and Hk heads; lse / delta are [B*H][Sq]. dq / dk / dv may alias one fused
// [tokens, (H + 2*Hk)*64] buffer (different column offsets).
// Split kernels: bwd_q over B*H*Sq/128 workgroups (the query blocks of the H query heads), then
// bwd_kv over B*Hk*Sk/128 (the key blocks of the Hk key/value heads, each summing its group's
// H / Hk query heads in head order). The fused kernel, when switched on, takes only what it has a
// form for: not causal, Sq == Sk, Hk == H, S in kFusedBwd; everything else runs the split kernels
// whatever the switch says.
TTDK_API(int, ttdk_attn_bwd, (const bf16_t* q, long long ldq, const bf16_t* k, long long ldk, const bf16_t* v,
                              long long ldv, const bf16_t* o, long long ldo, const bf16_t* dout, long long lddo,
                              const float* lse, float* delta, bf16_t* dq, long long lddq, bf16_t* dk, long long lddk,
                              bf16_t* dv, long long lddv, const int* seqlen, int B, int H, int Hk, int Sq, int Sk,
                              float p_drop, const long long* rng, unsigned site, int causal, hipStream_t st)) {
  if (!args_ok(H, Hk, Sq, Sk, causal, p_drop, rng, ldq | ldk | ldv | ldo | lddo | lddq | lddk | lddv,
               {q, k, v, o, dout}))
    return hipErrorInvalidValue;
  const bool gqa = Hk != H, drop = p_drop > 0.f;
  AttnParams P = make_params(B, H, Hk, Sq, Sk, seqlen, p_drop, rng, site);
  P.q = q; P.k = k; P.v = v; P.o = o; P.dout = dout;
  P.ldq = ldq; P.ldk = ldk; P.ldv = ldv; P.ldo = ldo; P.lddo = lddo;
  P.lse = const_cast<float*>(lse);
  P.delta = delta;
  if (!causal && Sq == Sk && !gqa && attn_fused_bwd()) {
    for (const FusedBwd& f : kFusedBwd) {
      if (f.S != Sq) continue;
      P.out = dq; P.ld_out = lddq; P.out2 = dk; P.ld_out2 = lddk; P.out3 = dv; P.ld_out3 = lddv;
      hipLaunchKernelGGL(f.kernel[drop], dim3(B * H), dim3(f.threads), 0, st, P);
      return hipGetLastError();
    }
  }
  if (causal) P.order = causal_order();
  // dQ first: it computes delta (rowsum dO . O) on the way and stores it for dK / dV
  P.out = dq; P.ld_out = lddq; P.out2 = nullptr;
  hipLaunchKernelGGL(kBwdQ[gqa][causal != 0][drop], dim3(B * H * (Sq / QBLK)), dim3(256), 0, st, P);
  P.out = dk; P.ld_out = lddk; P.out2 = dv; P.ld_out2 = lddv;
  AttnKernel kv = kBwdKv[gqa][causal != 0][drop];
  if (!gqa && !causal && drop) {
    for (const KvDiag& d : kKvDiag)
      if (d.mode == kv_diag()) kv = d.kernel;
  }
  hipLaunchKernelGGL(kv, dim3(B * Hk * (Sk / QBLK)), dim3(256), 0, st, P);
  return hipGetLastError();
}

// ---- banded masks (packed documents, sliding windows, causal, key length: attn_band_kernel)
// The table: int32 [4*B*S + 4*B*(S/128)], 16-byte aligned — per token {klo, khi, qlo, qhi}, then per
// 128-token block {kt0, kt1, qt0, qt1}. segment_ids int32 [B][S] or null, seqlen [B] or null,
// window_left / window_right < 0: unbounded; causal clamps the right side to 0. One launch on st,
// no allocation, no host synchronisation: it can be captured. Built once per step and shared by
// every layer's forward and backward.
TTDK_API(int, ttdk_attn_band, (const int* segment_ids, const int* seqlen, int B, int S, int window_left,
                               int window_right, int causal, int* table, hipStream_t st)) {
  if (B <= 0 || S <= 0 || S % QBLK || table == nullptr || (reinterpret_cast<uintptr_t>(table) & 15))
    return hipErrorInvalidValue;
  const int wl = window_left < 0 ? -1 : min(window_left, S);
  const int wr = causal ? 0 : window_right < 0 ? -1 : min(window_right, S);
  int4* tok = reinterpret_cast<int4*>(table);
  hipLaunchKernelGGL(attn_band_kernel, dim3(B), dim3(256), 0, st, segment_ids, seqlen, S, wl, wr, tok,
                     tok + static_cast<long long>(B) * S);
  return hipGetLastError();
}

namespace {
bool band_params(AttnParams& P, const int* band, int B, int Sq, int Sk) {
  if (band == nullptr || (reinterpret_cast<uintptr_t>(band) & 15) || Sq != Sk) return false;
  P.band_tok = reinterpret_cast<const int4*>(band);
  P.band_blk = P.band_tok + static_cast<long long>(B) * Sq;
  return true;
}
}  // namespace

// ttdk_attn_fwd with the table of ttdk_attn_band in the place of seqlen and causal (both are in the
// table). Self-attention only: Sq != Sk is refused.
TTDK_API(int, ttdk_attn_band_fwd, (const bf16_t* q, long long ldq, const bf16_t* k, long long ldk, const bf16_t* v,
                                   long long ldv, bf16_t* o, long long ldo, float* lse, const int* band, int B, int H,
                                   int Hk, int Sq, int Sk, float p_drop, const long long* rng, unsigned site,
                                   hipStream_t st)) {
  if (!args_ok(H, Hk, Sq, Sk, 1, p_drop, rng, ldq | ldk | ldv | ldo, {q, k, v, o})) return hipErrorInvalidValue;
  AttnParams P = make_params(B, H, Hk, Sq, Sk, nullptr, p_drop, rng, site);
  if (!band_params(P, band, B, Sq, Sk)) return hipErrorInvalidValue;
  P.q = q; P.k = k; P.v = v; P.ldq = ldq; P.ldk = ldk; P.ldv = ldv;
  P.out = o; P.ld_out = ldo; P.lse = lse;
  hipLaunchKernelGGL(kFwdBand[Hk != H][p_drop > 0.f], dim3(B * H * (Sq / QBLK)), dim3(256), 0, st, P);
  return hipGetLastError();
}

// The backward of ttdk_attn_band_fwd: always the split kernels (the fused backward has no band
// form), bwd_q then bwd_kv as in ttdk_attn_bwd.
TTDK_API(int, ttdk_attn_band_bwd, (const bf16_t* q, long long ldq, const bf16_t* k, long long ldk, const bf16_t* v,
                                   long long ldv, const bf16_t* o, long long ldo, const bf16_t* dout, long long lddo,
                                   const float* lse, float* delta, bf16_t* dq, long long lddq, bf16_t* dk,
                                   long long lddk, bf16_t* dv, long long lddv, const int* band, int B, int H, int Hk,
                                   int Sq, int Sk, float p_drop, const long long* rng, unsigned site, hipStream_t st)) {
  if (!args_ok(H, Hk, Sq, Sk, 1, p_drop, rng, ldq | ldk | ldv | ldo | lddo | lddq | lddk | lddv, {q, k, v, o, dout}))
    return hipErrorInvalidValue;
  const bool gqa = Hk != H, drop = p_drop > 0.f;
  AttnParams P = make_params(B, H, Hk, Sq, Sk, nullptr, p_drop, rng, site);
  if (!band_params(P, band, B, Sq, Sk)) return hipErrorInvalidValue;
  P.q = q; P.k = k; P.v = v; P.o = o; P.dout = dout;
  P.ldq = ldq; P.ldk = ldk; P.ldv = ldv; P.ldo = ldo; P.lddo = lddo;
  P.lse = const_cast<float*>(lse);
  P.delta = delta;
  P.out = dq; P.ld_out = lddq; P.out2 = nullptr;
  hipLaunchKernelGGL(kBwdQBand[gqa][drop], dim3(B * H * (Sq / QBLK)), dim3(256), 0, st, P);
  P.out = dk; P.ld_out = lddk; P.out2 = dv; P.ld_out2 = lddv;
  hipLaunchKernelGGL(kBwdKvBand[gqa][drop], dim3(B * Hk * (Sk / QBLK)), dim3(256), 0, st, P);
  return hipGetLastError();
}
