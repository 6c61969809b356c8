// Rotary position embeddings (RoPE), half-split convention ("rotate_half", LLaMA / GPT-NeoX), head
// size 64. For a token at position p and i in [0, 32), theta_i = base^(-i/32):
//   y[i]      = x[i]      * cos(p theta_i) - x[i + 32] * sin(p theta_i)
//   y[i + 32] = x[i + 32] * cos(p theta_i) + x[i]      * sin(p theta_i)
// inverse uses -sin: the transpose of the rotation, so both its inverse and its backward.
//
// One pass over the first `heads` 64-wide heads of every row of a token-major [tokens, >= heads*64]
// buffer; no other column is read or written. On the fused [q | k | v] projection the caller passes
// heads = H + Hk and q and k are rotated in one launch, in place.
//
// * No trigonometry on the device: cos / sin come from a host-built fp32 table [rows][2][32] (cos
//   row, then sin row). The position of row r is pos0 + r % S, so everything that bounds the table
//   read is checked on the host; there is no per-token position array.
// * All global traffic is 16-byte vector accesses. A work item owns one 16-byte chunk of the low half
//   of a head and the matching chunk of the high half (bf16: 8 + 8 columns, 4 items per head; fp32:
//   4 + 4 columns, 8 items per head), loads both and the matching cos / sin floats, computes in fp32
//   and rounds bf16 results with the project-wide RNE v_cvt_pk_bf16_f32 (pack8).
// * In place (y == x, ldy == ldx) is supported: a work item reads both of its chunks before it
//   writes either, and work items own disjoint elements. Any other overlap of x and y is the
//   caller's error and is not checked.
// * Work items are ordered chunk-fastest, then head, then token, so a wave covers contiguous row
//   segments. The grid is capped at 256 CUs x 8 blocks of 256 threads and grid-strided; the row /
//   in-row / position indices advance by host-computed increments (an add and a conditional
//   subtract per step) so the loop holds no integer division.
// * No LDS.
//
// dt: 0 = fp32, 1 = bf16 (the codes of nn_generic.hip); x and y share it.
#include "common.h"

namespace ttdk {
namespace {

constexpr int kRopeBlock = 256;
constexpr int kRopeMaxBlocks = 256 * 8;

template <typename T>
struct RopeVec;

template <>
struct RopeVec<bf16_t> {
  static constexpr int E = 8;  // elements per 16 bytes
  static __device__ __forceinline__ void load(const bf16_t* p, float (&f)[8]) {
    unpack8(*reinterpret_cast<const uint4*>(p), f);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&f)[8]) {
    *reinterpret_cast<uint4*>(p) = pack8(f);
  }
};

template <>
struct RopeVec<float> {
  static constexpr int E = 4;
  static __device__ __forceinline__ void load(const float* p, float (&f)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    f[0] = v.x, f[1] = v.y, f[2] = v.z, f[3] = v.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&f)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  }
};

template <int E>
__device__ __forceinline__ void load_table(const float* __restrict__ p, float (&f)[E]) {
#pragma unroll
  for (int i = 0; i < E; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + i);
    f[i] = v.x, f[i + 1] = v.y, f[i + 2] = v.z, f[i + 3] = v.w;
  }
}

// Step of the grid-stride loop, in (row, in-row item, position) form: one stride of
// gridDim.x * 256 work items is drow rows and drem items further, dpos = drow % S.
struct RopeStep {
  int per_row;  // heads * (32 / E) work items per row
  int drow, drem, dpos;
};

// x and y may be the same buffer: no __restrict__ on them.
template <typename T>
__global__ __launch_bounds__(kRopeBlock) void rope_kernel(const T* x, long long ldx, T* y, long long ldy,
                                                          const float* __restrict__ table, long long tokens, int S,
                                                          int pos0, float sgn, RopeStep st) {
  constexpr int E = RopeVec<T>::E;
  constexpr int CH = 32 / E;  // chunks per half head
  const unsigned i0 = blockIdx.x * kRopeBlock + threadIdx.x;  // < 2048 * 256
  long long r = i0 / static_cast<unsigned>(st.per_row);
  int j = static_cast<int>(i0 % static_cast<unsigned>(st.per_row));
  int p = static_cast<int>(r % S);
  while (r < tokens) {
    const int h = j / CH, c = j % CH;
    const long long col = static_cast<long long>(h) * 64 + c * E;
    const T* xp = x + r * ldx + col;
    const float* tp = table + static_cast<long long>(pos0 + p) * 64 + c * E;
    float lo[E], hi[E], cs[E], sn[E], ylo[E], yhi[E];
    RopeVec<T>::load(xp, lo);
    RopeVec<T>::load(xp + 32, hi);
    load_table<E>(tp, cs);
    load_table<E>(tp + 32, sn);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const float s = sn[k] * sgn;
      ylo[k] = lo[k] * cs[k] - hi[k] * s;
      yhi[k] = hi[k] * cs[k] + lo[k] * s;
    }
    T* yp = y + r * ldy + col;
    RopeVec<T>::store(yp, ylo);
    RopeVec<T>::store(yp + 32, yhi);
    // advance one grid stride
    j += st.drem;
    r += st.drow;
    p += st.dpos;
    if (j >= st.per_row) {
      j -= st.per_row;
      ++r;
      ++p;
    }
    if (p >= S) p -= S;  // p < 2S here: dpos < S and at most one carry
  }
}

template <typename T>
int rope_launch(const void* x, long long ldx, void* y, long long ldy, const float* table, long long tokens, int S,
                int heads, int pos0, int inverse, hipStream_t st) {
  constexpr int E = RopeVec<T>::E;
  RopeStep step;
  step.per_row = heads * (32 / E);
  const long long items = tokens * step.per_row;
  long long blocks = (items + kRopeBlock - 1) / kRopeBlock;
  if (blocks > kRopeMaxBlocks) blocks = kRopeMaxBlocks;
  const int stride = static_cast<int>(blocks) * kRopeBlock;
  step.drow = stride / step.per_row;
  step.drem = stride % step.per_row;
  step.dpos = step.drow % S;
  hipLaunchKernelGGL(rope_kernel<T>, dim3(static_cast<unsigned>(blocks)), dim3(kRopeBlock), 0, st,
                     static_cast<const T*>(x), ldx, static_cast<T*>(y), ldy, table, tokens, S, pos0,
                     inverse ? -1.f : 1.f, step);
  return hipGetLastError();
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace ttdk

using namespace ttdk;

// Number of threads the capped grid launches (tests size their grid-stride case from it).
TTDK_API(int, ttdk_rope_max_threads, ()) { return kRopeMaxBlocks * kRopeBlock; }

// y[r, :heads*64] = rotation of x[r, :heads*64] at position pos0 + r % S (inverse != 0: the inverse
// rotation). x, y: [tokens, >= heads*64], row strides ldx / ldy in elements, type dt (0 fp32, 1 bf16);
// table fp32 [table_rows][2][32]. y == x with ldy == ldx is in place; any other overlap is the
// caller's error (not checked). Bad arguments return hipErrorInvalidValue without a launch;
// tokens == 0 returns 0 without a launch.
TTDK_API(int, ttdk_rope, (const void* x, long long ldx, void* y, long long ldy, int dt, const float* table,
                          int table_rows, long long tokens, int S, int heads, int pos0, int inverse, hipStream_t st)) {
  if (heads <= 0 || heads > (1 << 20) || S <= 0 || tokens < 0) return hipErrorInvalidValue;
  if (tokens % S != 0) return hipErrorInvalidValue;
  if (pos0 < 0 || static_cast<long long>(pos0) + S > table_rows) return hipErrorInvalidValue;
  if (dt != 0 && dt != 1) return hipErrorInvalidValue;
  const long long width = static_cast<long long>(heads) * 64;
  if (ldx < width || ldy < width) return hipErrorInvalidValue;
  const long long esz = dt == 0 ? 4 : 2;
  if (!x || !y || !table || !aligned16(x) || !aligned16(y) || !aligned16(table)) return hipErrorInvalidValue;
  if ((ldx * esz) % 16 != 0 || (ldy * esz) % 16 != 0) return hipErrorInvalidValue;
  if (tokens == 0) return 0;
  if (dt == 0) return rope_launch<float>(x, ldx, y, ldy, table, tokens, S, heads, pos0, inverse, st);
  return rope_launch<bf16_t>(x, ldx, y, ldy, table, tokens, S, heads, pos0, inverse, st);
}
