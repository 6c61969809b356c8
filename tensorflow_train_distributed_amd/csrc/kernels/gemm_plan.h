#pragma once
// Launch plans of the GEMM / convolution kernels: every decision that depends on the shape
// alone — which kernel takes it, its tile, the split-K clamp, the sub-pixel phase order, the
// rows of a statistics buffer — as pure host arithmetic, no HIP headers. The launchers
// (gemm_conv.h, conv_*.hip, gemm4w.hip, gemm4t.hip) include this header; libttd_rt.so exports
// the same functions (runtime/gemm_plan.cc) to ops/_plan.py, which sizes buffers and picks
// paths before it calls a launcher; tests/test_gemm_plan.py pins them on the CPU. Environment
// switches are read by the callers and passed in; pointer and epilogue checks stay in the launchers.

#include "abi.h"

// Convolution geometry passed from Python (ops/_lib.py ConvGeom, identical layout).
struct TtdkConv {
  int N, H, W, C;   // input NHWC
  int K, R, S;      // filters [K][R][S][C]
  int P, Q;         // output spatial
  int sh, sw, ph, pw, dh, dw;
};
template <>
struct ttd_abi::Code<const TtdkConv*> {
  static constexpr char code = 'G';
};

namespace ttdk {
namespace plan {

inline int cdiv(long long a, long long b) { return static_cast<int>((a + b - 1) / b); }

inline bool is_pointwise(const TtdkConv& g) {
  return g.R == 1 && g.S == 1 && g.sh == 1 && g.sw == 1 && g.ph == 0 && g.pw == 0;
}
inline bool unit_no_dilation(const TtdkConv& g) { return g.sh == 1 && g.sw == 1 && g.dh == 1 && g.dw == 1; }
inline long long out_pixels(const TtdkConv& g) { return static_cast<long long>(g.N) * g.P * g.Q; }
inline long long in_pixels(const TtdkConv& g) { return static_cast<long long>(g.N) * g.H * g.W; }

// ------------------------------------------------------------------ tiles
// Tile width of the 256-row LDS-DMA kernel for an M x N x K GEMM, or 0 when the 4-wave
// kernel is the better fit (small tiles / small GEMMs).
inline int big_bn(int M, int N, int K) {
  if (M < 256 || N < 128 || K % 64 || N % 8 || static_cast<long long>(M) * N < (1LL << 20)) return 0;
  return N >= 256 ? 256 : 128;
}
// Weight gradients have a long K (pixels) and split-K fills the machine, so only the tile
// shape (not M*N) decides.
inline int big_bn_wgrad(int M, int N, int K) {
  if (M < 256 || N < 128 || K % 64 || N % 8) return 0;
  return N >= 256 ? 256 : 128;
}
// 4-wave kernel: prefer 128x128; shrink a dimension when it is small.
inline void pick_tile(int M, int N, int* bm, int* bn) {
  *bm = (M <= 64) ? 64 : 128;
  *bn = (N <= 64) ? 64 : 128;
}
// Tile rows of gemm4t.hip: 128 when the output has at most 128 rows (a 256-row tile would run half
// its MFMAs on padding), else 256; the bias row sums (BERT) use the 256-row form (TTD_G4T_BM128).
inline int g4t_bm(int M, bool rowsum, bool bm128_enabled) {
  return (bm128_enabled && !rowsum && M <= 128) ? 128 : 256;
}

// ------------------------------------------------------------------ split-K
// Every split gets at least one K-tile and no split is empty; K-tiles per split = cdiv(ktiles, result).
inline int clamp_splits(int ktiles, int splits) {
  if (ktiles < 1) return 1;
  if (splits < 1) splits = 1;
  if (splits > ktiles) splits = ktiles;
  return cdiv(ktiles, cdiv(ktiles, splits));
}
// gemm4t.hip: at least two K-tiles per split (its pipeline prologue).
inline int clamp_splits_4t(int ktiles, int splits) {
  if (ktiles < 1) return 1;
  splits = splits < ktiles / 2 ? splits : ktiles / 2;
  if (splits < 1) splits = 1;
  return cdiv(ktiles, cdiv(ktiles, splits));
}

// ------------------------------------------------------------------ sub-pixel phases
// Strided data gradient by phases (conv_dgrad.hip): along one axis, phase a of stride s covers
// the input pixels s*i + a; first tap r0, tap count T, padding offset off, extent n.
struct Phase {
  int r0, T, off, n;
};
inline Phase phase_of(int a, int s, int pad, int R, int H) {
  Phase ph;
  ph.r0 = (a + pad) % s;
  ph.T = ph.r0 < R ? (R - ph.r0 + s - 1) / s : 0;
  ph.off = (a + pad - ph.r0) / s;
  ph.n = a < H ? (H - a + s - 1) / s : 0;
  return ph;
}
// The phase pairs in launch order: idx = a * s + b over [0, s * s), s = g.sh. false: that pair
// covers no pixel (an extent smaller than the stride) and is skipped.
inline bool phase_pair(const TtdkConv& g, int idx, Phase* row, Phase* col) {
  *row = *col = Phase{0, 0, 0, 0};
  if (g.sh < 1) return false;
  *row = phase_of(idx / g.sh, g.sh, g.ph, g.R, g.H);
  *col = phase_of(idx % g.sh, g.sh, g.pw, g.S, g.W);
  return row->n != 0 && col->n != 0;
}

// ------------------------------------------------------------------ data-gradient statistics
// Tile rows (= rows per statistics tile) of one unit-stride data-gradient GEMM: 256, the
// 256-row kernel, where it fits and a K-tile stays inside one tap (kc = channels of dy), else
// the 4-wave kernel's tile. *bn = the tile width.
inline int dgrad_tile(int M, int N, int K, int kc, int* bn) {
  const int bbn = big_bn(M, N, K);
  if (bbn && kc % 64 == 0) {
    *bn = bbn;
    return 256;
  }
  int bm;
  pick_tile(M, N, &bm, bn);
  return bm;
}
// Unit-stride data gradient with statistics: the (bm, bn) ttdk_conv_dgrad is asked for and the
// rows of the partial-sum buffer. stat_4w_k (TTD_DGRAD_STAT_4W_K): pointwise gradients with a
// reduction up to it run on the 4-wave kernel.
inline void dgrad_stat_plan(const TtdkConv& g, int stat_4w_k, int* bm, int* bn, int* rows) {
  const int M = static_cast<int>(in_pixels(g)), N = g.C, K = g.R * g.S * g.K;
  if (g.R == 1 && g.S == 1 && g.ph == 0 && g.pw == 0 && K <= stat_4w_k) {
    pick_tile(M, N, bm, bn);
  } else {
    *bm = dgrad_tile(M, N, K, g.K, bn);
  }
  *rows = cdiv(M, *bm);
}
// Sub-pixel data gradient with statistics: each phase GEMM owns its own block of tile rows.
// -1: not a sub-pixel geometry.
inline long long subpixel_stat_rows(const TtdkConv& g) {
  const int s = g.sh;
  if (g.sw != s || s < 2) return -1;
  long long rows = 0;
  for (int i = 0; i < s * s; ++i) {
    Phase pr, pc;
    if (!phase_pair(g, i, &pr, &pc)) continue;
    const int M = g.N * pr.n * pc.n, K = pr.T * pc.T * g.K;
    int bn;
    rows += cdiv(M, dgrad_tile(M, g.C, K, g.K, &bn));
  }
  return rows;
}

// ------------------------------------------------------------------ admission
// One predicate per launcher: the conditions of its admission test that depend on the geometry alone.
// ttdk_conv_fwd4w (bf16, 4-wave): a K-tile inside one tap, 32-bit operand offsets.
inline bool conv_fwd4w_takes(const TtdkConv& g) {
  const long long M = out_pixels(g), N = g.K, K = static_cast<long long>(g.R) * g.S * g.C;
  const long long xb = in_pixels(g) * g.C * 2;
  const long long shift = (static_cast<long long>(g.ph) * g.W + g.pw) * g.C * 2;
  return !(g.C % 64 || K < 128 || N % 8 || g.dh != 1 || g.dw != 1 || g.R * g.S > 32 || M < 1 ||
           xb + shift >= (1LL << 31) || (N + 256) * K * 2 >= (1LL << 32) || M * N * 2 >= (1LL << 40));
}
// ttdk_conv_dgrad4w: dy gathered as a forward conv with padding (R - 1 - ph, S - 1 - pw).
inline bool conv_dgrad4w_takes(const TtdkConv& g) {
  const long long M = in_pixels(g), N = g.C, K = static_cast<long long>(g.R) * g.S * g.K;
  const long long yb = out_pixels(g) * g.K * 2;
  const int pho = g.R - 1 - g.ph, pwo = g.S - 1 - g.pw;
  const long long shift = (static_cast<long long>(pho) * g.Q + pwo) * g.K * 2;
  return !(!unit_no_dilation(g) || g.K % 64 || K < 128 || N % 8 || g.R * g.S > 32 || pho < 0 || pwo < 0 || M < 1 ||
           yb + shift >= (1LL << 31) || (N + 256) * K * 2 >= (1LL << 32));
}
// ttdk_conv_fwd4k8 (fp8, 4-wave); the dense rows of a pointwise conv carry 32-bit offsets.
inline bool conv_fwd4k8_takes(const TtdkConv& g) {
  const long long M = out_pixels(g), N = g.K, K = static_cast<long long>(g.R) * g.S * g.C;
  const long long xb = in_pixels(g) * g.C;
  const long long shift = (static_cast<long long>(g.ph) * g.W + g.pw) * g.C;
  if (g.C % 128 || N % 8 || N < 8 || M < 1 || g.dh != 1 || g.dw != 1 || g.R * g.S > 32 ||
      xb + shift >= (1LL << 31) || (N + 256) * K >= (1LL << 32))
    return false;
  return !(is_pointwise(g) && M * g.C >= (1LL << 32));
}
// ttdk_conv_dgrad4k8
inline bool conv_dgrad4k8_takes(const TtdkConv& g) {
  const long long M = in_pixels(g), N = g.C, K = static_cast<long long>(g.R) * g.S * g.K;
  const long long yb = out_pixels(g) * g.K;
  const int pho = g.R - 1 - g.ph, pwo = g.S - 1 - g.pw;
  const long long shift = (static_cast<long long>(pho) * g.Q + pwo) * g.K;
  return !(!unit_no_dilation(g) || g.K % 128 || N % 8 || N < 8 || g.R * g.S > 32 || pho < 0 || pwo < 0 || M < 1 ||
           yb + shift >= (1LL << 31) || (N + 256) * K >= (1LL << 32));
}
// ttdk_conv_wgrad_fp8 (8-wave 256 x 128 tiles, 32-bit im2col offsets)
inline bool conv_wgrad_fp8_takes(const TtdkConv& g) {
  const long long M = g.K, N = static_cast<long long>(g.R) * g.S * g.C, K = out_pixels(g);
  return !(g.C % 16 || g.K % 16 || K % 128 || N < 256 || M < 16 || in_pixels(g) * g.C >= (1LL << 32));
}
// ttdk_conv_wgrad_bn: the 4-wave im2col-gather path only
inline bool conv_wgrad_bn_takes(const TtdkConv& g) {
  return !(g.C % 8 || g.K % 8 || is_pointwise(g) ||
           big_bn_wgrad(g.K, g.R * g.S * g.C, static_cast<int>(out_pixels(g))));
}
// ttdk_conv_dgrad_bnpro / ttdk_conv_fwd_bnpro: a pointwise conv on the 256-row kernel
inline bool conv_dgrad_bnpro_takes(const TtdkConv& g) {
  return is_pointwise(g) && g.K % 64 == 0 && big_bn(static_cast<int>(out_pixels(g)), g.C, g.K) != 0;
}
inline bool conv_fwd_bnpro_takes(const TtdkConv& g) {
  return is_pointwise(g) && g.C % 64 == 0 && big_bn(static_cast<int>(out_pixels(g)), g.K, g.C) != 0;
}
// ttdk_gemm4t_wgrad: dW[M,N] over K tokens, operands under 2 GiB
inline bool gemm4t_takes(long long M, long long N, long long K) {
  return !(K % 64 || K < 128 || M < 8 || N < 8 || M % 8 || N % 8 || K * M * 2 >= (1LL << 31) ||
           K * N * 2 >= (1LL << 31));
}
// ttdk_conv_wgrad4t: its im2col gather on top of gemm4t
inline bool conv_wgrad4t_takes(const TtdkConv& g) {
  const long long K = out_pixels(g);
  if (g.C % 8 || g.K % 8 || K % 64 || K < 128 || g.dh != 1 || g.dw != 1 || in_pixels(g) * g.C * 2 >= (1LL << 31) ||
      K * g.K * 2 >= (1LL << 31) || g.P * g.Q < 2 || g.Q < 2)
    return false;
  return gemm4t_takes(g.K, static_cast<long long>(g.R) * g.S * g.C, K);
}
// ttdk_conv_wgrad4t8: 16-B DMA chunks of 16 channels, whole 128-pixel K-tiles
inline bool conv_wgrad4t8_takes(const TtdkConv& g) {
  const long long M = g.K, N = static_cast<long long>(g.R) * g.S * g.C, K = out_pixels(g);
  return !(g.C % 16 || g.K % 16 || M < 16 || N < 16 || K % 128 || K < 128 || g.dh != 1 || g.dw != 1 ||
           in_pixels(g) * g.C >= (1LL << 31) || K * g.K >= (1LL << 31) ||
           (!is_pointwise(g) && (g.P * g.Q < 2 || g.Q < 2)));
}

}  // namespace plan
}  // namespace ttdk
