#pragma once
// Launch plan of the depthwise convolution kernels (depthwise.hip): everything that depends on the
// shape alone — which form takes it, the strip width of the fast form, the partition of the N*P
// output rows into weight-gradient slabs and the size of the partial workspace — as pure host
// arithmetic, no HIP headers. depthwise.hip includes this header; libttd_rt.so exports the same
// functions (runtime/dwconv_plan.cc) to ops/_plan.py, and tests/test_depthwise_cpu.py pins them
// without a GPU. Pointer alignment is checked by the launchers.

#include "abi.h"

// Geometry passed from Python (ops/_lib.py DwConvGeom, identical layout): input NHWC [N,H,W,C],
// filter fp32 [R,S,C,M], output [N,P,Q,C*M]; output channel c*M+m reads input channel c.
struct TtdkDwConv {
  int N, H, W, C;
  int M, R, S;
  int P, Q;
  int sh, sw, ph, pw, dh, dw;
};
template <>
struct ttd_abi::Code<const TtdkDwConv*> {
  static constexpr char code = 'D';
};

namespace ttdk {
namespace dwplan {

constexpr int kMaxTap = 7;      // R, S <= 7
constexpr int kStrip = 4;       // fast form: consecutive output (dgrad: input) columns per thread
constexpr int kMaxSlabs = 512;  // weight gradient: at most this many partial rows ...
constexpr long long kMaxWsFloats = 1LL << 22;  // ... and at most 16 MiB of them

inline bool valid(const TtdkDwConv& g) {
  return g.N > 0 && g.H > 0 && g.W > 0 && g.C > 0 && g.M > 0 && g.P > 0 && g.Q > 0 && g.R > 0 && g.S > 0 &&
         g.R <= kMaxTap && g.S <= kMaxTap && g.sh > 0 && g.sw > 0 && g.dh > 0 && g.dw > 0 && g.ph >= 0 && g.pw >= 0 &&
         static_cast<long long>(g.C) * g.M <= 0x7fffffffLL / (kMaxTap * kMaxTap);
}

// Fast form: bf16 (dt 1), one filter per channel, 8 channels per lane, 3x3, stride 1 or 2 (equal),
// no dilation. Every MobileNet-v1 layer measured (profiles/dwconv_bench.txt) ran no slower on this
// form than on the generic one, in all three directions, so the rule has no size condition.
inline bool fast_takes(const TtdkDwConv& g, int dt) {
  return valid(g) && dt == 1 && g.M == 1 && g.C % 8 == 0 && g.R == 3 && g.S == 3 && g.sh == g.sw &&
         (g.sh == 1 || g.sh == 2) && g.dh == 1 && g.dw == 1;
}

inline long long filter_elems(const TtdkDwConv& g) { return static_cast<long long>(g.R) * g.S * g.C * g.M; }
// Partial rows are padded to 4 floats (the column reduce reads and writes 16-byte vectors).
inline long long part_stride(const TtdkDwConv& g) { return (filter_elems(g) + 3) / 4 * 4; }
inline long long out_rows(const TtdkDwConv& g) { return static_cast<long long>(g.N) * g.P; }

// Output rows per slab; slab t covers rows [t * rows_per_slab, min(rows, (t + 1) * rows_per_slab)).
inline long long rows_per_slab(const TtdkDwConv& g) {
  long long cap = kMaxWsFloats / part_stride(g);
  if (cap > kMaxSlabs) cap = kMaxSlabs;
  if (cap < 1) cap = 1;
  const long long rows = out_rows(g);
  return (rows + cap - 1) / cap;
}
// Number of slabs T (none empty).
inline int wgrad_parts(const TtdkDwConv& g) {
  const long long per = rows_per_slab(g);
  return static_cast<int>((out_rows(g) + per - 1) / per);
}
inline void slab_rows(const TtdkDwConv& g, int t, long long* r0, long long* r1) {
  const long long per = rows_per_slab(g), rows = out_rows(g);
  *r0 = t * per < rows ? t * per : rows;
  *r1 = (t + 1) * per < rows ? (t + 1) * per : rows;
}
// Workspace in floats: T partial rows and one row for the folded sum (used when the filter
// gradient cannot be written in 16-byte vectors).
inline long long wgrad_ws_floats(const TtdkDwConv& g) { return (wgrad_parts(g) + 1LL) * part_stride(g); }

}  // namespace dwplan
}  // namespace ttdk
