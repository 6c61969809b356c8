// CPU export of the GEMM / convolution launch plans (kernels/gemm_plan.h): ops/_plan.py sizes
// buffers and picks kernel paths with the very functions the launchers use, and
// tests/test_gemm_plan.py checks them without a GPU.
#include "../kernels/gemm_plan.h"

#include "common.h"

namespace plan = ttdk::plan;

TTD_API(int, ttd_plan_conv_size, ()) { return static_cast<int>(sizeof(TtdkConv)); }

TTD_API(int, ttd_plan_big_bn, (int M, int N, int K)) { return plan::big_bn(M, N, K); }
TTD_API(int, ttd_plan_big_bn_wgrad, (int M, int N, int K)) { return plan::big_bn_wgrad(M, N, K); }
TTD_API(void, ttd_plan_pick_tile, (int M, int N, int* bm, int* bn)) { plan::pick_tile(M, N, bm, bn); }
TTD_API(int, ttd_plan_g4t_bm, (int M, int rowsum, int bm128_enabled)) {
  return plan::g4t_bm(M, rowsum != 0, bm128_enabled != 0);
}

TTD_API(int, ttd_plan_clamp_splits, (int ktiles, int splits)) { return plan::clamp_splits(ktiles, splits); }
TTD_API(int, ttd_plan_clamp_splits_4t, (int ktiles, int splits)) { return plan::clamp_splits_4t(ktiles, splits); }

// out: r0, T, off, n of the row phase, then of the column phase
TTD_API(int, ttd_plan_phase_pair, (const TtdkConv* g, int idx, int* out)) {
  plan::Phase r, c;
  const bool any = plan::phase_pair(*g, idx, &r, &c);
  const int v[8] = {r.r0, r.T, r.off, r.n, c.r0, c.T, c.off, c.n};
  std::memcpy(out, v, sizeof(v));
  return any;
}

TTD_API(void, ttd_plan_dgrad_stat, (const TtdkConv* g, int stat_4w_k, int* bm, int* bn, int* rows)) {
  plan::dgrad_stat_plan(*g, stat_4w_k, bm, bn, rows);
}
TTD_API(long long, ttd_plan_subpixel_stat_rows, (const TtdkConv* g)) { return plan::subpixel_stat_rows(*g); }

#define TTD_PLAN_TAKES(NAME) \
  TTD_API(int, ttd_plan_##NAME##_takes, (const TtdkConv* g)) { return plan::NAME##_takes(*g); }
TTD_PLAN_TAKES(conv_fwd4w)
TTD_PLAN_TAKES(conv_dgrad4w)
TTD_PLAN_TAKES(conv_fwd4k8)
TTD_PLAN_TAKES(conv_dgrad4k8)
TTD_PLAN_TAKES(conv_wgrad_fp8)
TTD_PLAN_TAKES(conv_wgrad_bn)
TTD_PLAN_TAKES(conv_dgrad_bnpro)
TTD_PLAN_TAKES(conv_fwd_bnpro)
TTD_PLAN_TAKES(conv_wgrad4t)
TTD_PLAN_TAKES(conv_wgrad4t8)
#undef TTD_PLAN_TAKES
TTD_API(int, ttd_plan_gemm4t_takes, (long long M, long long N, long long K)) { return plan::gemm4t_takes(M, N, K); }
