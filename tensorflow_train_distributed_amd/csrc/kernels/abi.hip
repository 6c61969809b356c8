// The signature table of libttd_hip.so (abi.h): ttdk_abi_count / ttdk_abi_entry, and the layout
// of the three structs Python passes by pointer, so ops/_lib.py can check its ctypes mirrors
// field by field when it loads the library.
#include "dwconv_plan.h"
#include "gemm_conv.h"

TTD_ABI_TABLE(ttdk_abi)

// Struct behind signature letter `code` ('E', 'G', 'D'): out[0] = sizeof, out[1..] = offsetof of
// every field in declaration order, at most cap values. Returns the number of values, -1 for
// another letter.
TTDK_API(int, ttdk_abi_layout, (int code, long long* out, int cap)) {
#define F(f) offsetof(T, f)
  const auto put = [&](std::initializer_list<size_t> v) {
    int n = 0;
    for (size_t x : v)
      if (n++ < cap) out[n - 1] = static_cast<long long>(x);
    return n;
  };
  if (code == 'E') {
    using T = TtdkEpilogue;
    return put({sizeof(T), F(mode), F(out), F(ldo), F(slab_stride), F(bias), F(residual), F(ldr), F(act), F(beta),
                F(remap), F(rP), F(rQ), F(rOH), F(rOW), F(rs), F(stat), F(alpha), F(aux), F(ascale0), F(ascale1),
                F(by), F(bmask), F(by2), F(stat2), F(bH), F(bW)});
  }
  if (code == 'G') {
    using T = TtdkConv;
    return put({sizeof(T), F(N), F(H), F(W), F(C), F(K), F(R), F(S), F(P), F(Q), F(sh), F(sw), F(ph), F(pw), F(dh),
                F(dw)});
  }
  if (code == 'D') {
    using T = TtdkDwConv;
    return put({sizeof(T), F(N), F(H), F(W), F(C), F(M), F(R), F(S), F(P), F(Q), F(sh), F(sw), F(ph), F(pw), F(dh),
                F(dw)});
  }
#undef F
  return -1;
}
