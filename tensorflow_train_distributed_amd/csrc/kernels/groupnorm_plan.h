#pragma once
// Launch plan of the group normalisation kernels (groupnorm.hip): everything that depends on the
// shape alone — validity, which form takes it, the lanes of a block, the partition of the M pixel
// rows of every image into slabs and the sizes of the two workspaces — as pure host arithmetic, no
// HIP headers. groupnorm.hip includes this header; libttd_rt.so exports the same functions
// (runtime/groupnorm_plan.cc) to ops/_plan.py, and tests/test_groupnorm_cpu.py pins them without a
// GPU. Pointer alignment is checked by the launchers.
//
// Shape: x [N, M, C] channels last (M = product of the spatial extents), G groups of C / G channels.

namespace ttdk {
namespace gnplan {

constexpr int kBlock = 256;     // threads of every streaming block
constexpr int kVec = 8;         // fast form: channels per lane (one 16-byte bf16 vector)
constexpr int kFastLanes = 32;  // fast form: at most this many lanes share a pixel row in a block
constexpr int kGenericCols = 64;  // generic form: channels (= lanes) of a block's column group
constexpr int kMaxSlabs = 512;  // at most this many partial rows over all images ...
constexpr long long kMaxWsFloats = 1LL << 22;  // ... and at most 16 MiB of them (dwconv_plan.h's caps)
constexpr long long kMaxDim = 1LL << 30;

inline bool valid(long long N, long long M, long long C, long long G) {
  return N > 0 && M > 0 && C > 0 && G > 0 && N <= kMaxDim && M <= kMaxDim && C <= kMaxDim && C % G == 0 &&
         N * C <= kMaxDim;
}

// Fast form: bf16 (dt 1), 8 channels per lane. Groups exist only in the fold kernels, so there is
// no condition on C / G. At every shape measured (profiles/groupnorm_bench.txt: ResNet-50-GN's
// sites at batch 32, 64x64x320 and 32x32x640, G = 32) this form ran in 0.36-0.82 of the generic
// form's time, forward and backward, so the rule has no size condition.
inline bool fast_takes(long long N, long long M, long long C, long long G, int dt) {
  return valid(N, M, C, G) && dt == 1 && C % kVec == 0;
}

// Lanes that share one pixel row in a block, and the pixel rows a block has in flight. The fast
// form cuts the C / 8 vectors of a row into chunks of at most kFastLanes lanes of equal size.
inline int lanes(long long C, bool fast) {
  if (!fast) return kGenericCols;
  const long long cg = C / kVec, chunks = (cg + kFastLanes - 1) / kFastLanes;
  return static_cast<int>((cg + chunks - 1) / chunks);
}
inline int chunks(long long C, bool fast) {
  const long long cg = fast ? C / kVec : C, lc = lanes(C, fast);
  return static_cast<int>((cg + lc - 1) / lc);
}
inline int rows_per_block(long long C, bool fast) { return kBlock / lanes(C, fast); }

// Partial and coefficient rows are padded to 4 floats (16-byte coefficient loads).
inline long long part_stride(long long C) { return (C + 3) / 4 * 4; }

// Slabs an image may be cut into: N * T <= kMaxSlabs and N * T * 2 * stride <= kMaxWsFloats,
// unless N (or N * C) alone exceeds them: then one slab per image.
inline long long slab_cap(long long N, long long C) {
  long long cap = kMaxWsFloats / (N * 2 * part_stride(C));
  if (cap > kMaxSlabs / N) cap = kMaxSlabs / N;
  return cap < 1 ? 1 : cap;
}
// Pixel rows per slab; slab t of every image covers rows [t * per, min(M, (t + 1) * per)).
inline long long rows_per_slab(long long N, long long M, long long C) {
  const long long cap = slab_cap(N, C);
  return (M + cap - 1) / cap;
}
// Number of slabs T per image (none empty, T >= 1).
inline int parts(long long N, long long M, long long C) {
  const long long per = rows_per_slab(N, M, C);
  return static_cast<int>((M + per - 1) / per);
}
inline void slab_rows(long long N, long long M, long long C, int t, long long* r0, long long* r1) {
  const long long per = rows_per_slab(N, M, C);
  *r0 = t * per < M ? t * per : M;
  *r1 = (t + 1) * per < M ? (t + 1) * per : M;
}

// Workspaces in floats, in rows of [2][stride] per image.
//   forward:  part[N][T] | per-channel (mean, centred second moment)[N] | (mean_c, scale)[N]
//   backward: part[N][T] | folded (sum dy, sum dy*xhat)[N] | per-group (A, B)[N] | (mean_c, p | q, r)[N][2]
inline long long fwd_ws_floats(long long N, long long M, long long C) {
  return (parts(N, M, C) + 2LL) * N * 2 * part_stride(C);
}
inline long long bwd_ws_floats(long long N, long long M, long long C) {
  return (parts(N, M, C) + 4LL) * N * 2 * part_stride(C);
}

}  // namespace gnplan
}  // namespace ttdk
