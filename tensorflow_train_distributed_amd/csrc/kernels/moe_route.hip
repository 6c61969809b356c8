// Mixture-of-experts routing on the device, everything around the two grouped matmuls of a
// token-choice MoE block (grouped_gemm.hip): the router's softmax / top-k / renormalise and its
// backward, the counting sort of the T * k (token, choice) slots by expert, the row gather that
// dispatches tokens to sorted rows and the weighted k-way sum that combines them again. No entry
// reads routing data on the host and every grid is sized from shapes alone, so a step can be captured
// into a hipGraph and replayed on other routings. No float atomics and no result that depends on the
// order in which workgroups run: every output is bitwise repeatable (the only atomics are integer
// adds into LDS histograms).
//
//   ttdk_moe_topk      probs = softmax(logits) fp32 [T, E]; expert int32 [T, k] = the k largest
//                      LOGITS of the row in descending order, ties to the lowest index, NaN above
//                      everything (torch.topk's order); gate fp32 [T, k] = the selected probs over
//                      their sum. Selecting on the logits makes the ids exact integers: softmax is
//                      monotone, its rounding is not.
//   ttdk_moe_topk_bwd  dlogits = softmax Jacobian applied to (dprobs + the renormalisation's Jacobian
//                      applied to dgate, scattered onto the selected columns); either gradient may
//                      be absent.
//   ttdk_moe_sort      stable counting sort of expert[S] (S = T * k slots, slot t * k + j): offsets
//                      int32 [E + 1] (the table ttdk_grouped_gemm reads), order [S] sorted row ->
//                      slot, inv [S] slot -> sorted row. Ids are data, not trusted: an id outside
//                      [0, E) sorts into pseudo-group E, the rows at and after offsets[E] that the
//                      grouped kernels zero; no id indexes anything before that clamp.
//   ttdk_moe_gather    out[r] = scale[idx[r]] * src[idx[r] / k] (scale optional), bf16 or fp32 in and
//                      out, converted in flight. With h and dgate it is the combine's backward in one
//                      pass: also dgate[idx[r]] = dot(h[r], src[idx[r] / k]).
//   ttdk_moe_combine   out[t] = sum_j w[t, j] * src[inv[t * k + j]] (w optional), fp32 accumulation in
//                      increasing j. With w the block's weighted combine, without it the dispatch's
//                      data gradient: both directions of both permutes are gathers, nothing scatters.
//   An idx / inv entry outside its range contributes a zero row instead of being followed.
//
// How the work is split.
//  * top-k, forward and backward: one wave owns 64 / L token rows, L = 8, 16, 32 or 64 lanes per
//    row (the smallest power of two >= E), expert e of a row in lane e % L, register e / L: V = 1,
//    2 or 4 values per lane (E <= 64, 128, 256). At E = 8 a wave holds 8 rows and no lane idles.
//    Row max, row sum and the backward's dot are xor butterflies over the row's L lanes (__shfl_xor,
//    every lane ends with the same bits). Each of the k selection rounds is one butterfly max over a
//    64-bit key: the logit mapped to an unsigned integer of the same order (NaN -> all ones, -0 ->
//    +0) in the high word, ~index in the low word, so one max yields value order and the lowest index
//    among equals; the winner's owner clears it with a bit in a lane-private mask. Lane j of the row
//    keeps the j-th winner and stores it. No LDS, no loop over E in one lane.
//  * sort: three launches over fixed chunks of 1024 consecutive slots. (1) 256 threads per chunk add
//    their clamped ids into an LDS histogram of E + 1 counters and write it to ws[chunk][0..E].
//    (2) one workgroup, a thread per expert: walks its column of ws down the chunks replacing every
//    count by the running sum before it, then an exclusive scan of the column totals over the
//    experts (wave __shfl_up scan, 4 wave sums through LDS, a carry between rounds of 256 experts)
//    gives offsets. (3) one wave per chunk: LDS counters start at offsets[e] + ws[chunk][e]; the chunk
//    is re-read 64 slots at a time in slot order; a lane's sorted row is its expert's counter plus the
//    number of lower lanes with the same expert, found with one ballot per bit of the id (11 at E = 1024)
//    instead of a loop over distinct ids; the lowest lane of each expert adds the step's count.
//    Slot order within an expert is kept at every level, so the sort is stable and equals
//    torch.argsort(stable=True).
//  * gather / combine: a grid of at most 2048 x 256 threads strided over (row, 8-column chunk) work
//    items, chunk fastest, the (row, chunk) pair advanced by host-computed increments (rope.hip's
//    scheme: no division in the loop; idx / k is a multiply by a host-made reciprocal and a shift).
//    All row traffic is 16-byte vector accesses. With the fused dot a wave owns a row instead
//    (512 columns per trip) and reduces its partial dot with the butterfly: fixed order.
//  * LDS: the two sort kernels' E + 1 counters, sized at launch (4100 bytes at E = 1024; E up to
//    ttdk_grouped_gemm_max_groups(), and below 16384 so that they fit 64 KB), 16 bytes of the scan; none
//    elsewhere.
//
// Registers, LDS and scratch as compiled (-Rpass-analysis=kernel-resource-usage; every kernel 0 bytes
// of scratch):
//   kernel                      VGPR      LDS bytes
//   moe_topk <8|16|32|64,1>     20 - 22   0
//   moe_topk <64,2> / <64,4>    27 / 33   0
//   moe_topk_bwd (all six)      16 - 26   0
//   moe_hist / scan / scatter   50/22/35  4 (E + 1) / 16 / 4 (E + 1), the counters sized at launch
//   moe_gather (4 type pairs)   16 - 18   0
//   moe_gather_dot (4)          48 - 54   0
//   moe_combine (4)             28 - 30   0
// Speed: see profiles/moe_route_bench.txt (tools/moe_route_bench.py, eager calls, forward + backward
// of each piece against the torch expressions it replaces). At T = 16384, E = 8, k = 2, D = 4096 /
// E = 64, k = 4, D = 2048: top-k 29 / 25 us against 142 / 149 us (2 launches against 17), sort 19 / 29
// us against 164 / 173 us (3 against 30), dispatch 173 / 164 us against 291 / 253 us (4.7 / 4.1 TB/s
// of the bytes that must move), combine 307 / 240 us against 1279 / 1251 us (4.4 / 4.5 TB/s). No piece
// is slower than what it replaces. The sort's single-workgroup scan and wave-per-chunk placement are
// latency, not bandwidth: at these sizes (32768 / 65536 slots) they are not what a step waits for.
#include "common.h"

extern "C" int ttdk_grouped_gemm_max_groups();

namespace ttdk {
namespace {

constexpr int kMoeMaxExperts = 256;  // router: 64 lanes x 4 values
constexpr int kMoeMaxTopk = 8;       // lane j of a row keeps winner j, and a row has >= 8 lanes
constexpr int kRouteBlock = 256;
constexpr int kSortChunk = 1024;     // slots per chunk of the counting sort
constexpr int kSortBlock = 256;
constexpr int kSortMaxExperts = 16383;  // E + 1 counters in the 64 KB of LDS a workgroup may ask for
constexpr int kRowBlock = 256;
constexpr int kRowMaxBlocks = 256 * 8;
constexpr int kMaxRows = 1 << 30;
constexpr int kMaxDivisor = 256;     // the k of idx / k (DivK below)

typedef unsigned long long u64;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------------------- router top-k
// (logit, index) -> a key whose unsigned order is: larger logit first, then lower index; NaN largest.
// Every real key is > 0, the key of "nothing here".
__device__ __forceinline__ u64 route_key(float x, int idx) {
  const uint32_t b = __float_as_uint(x + 0.f);  // -0 -> +0
  const uint32_t k = x != x ? 0xffffffffu : (b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u));
  return (static_cast<u64>(k) << 32) | static_cast<uint32_t>(~idx);
}

template <int L>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

template <int L>
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

template <int L>
__device__ __forceinline__ u64 row_max_key(u64 v) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, kWave);
    v = w > v ? w : v;
  }
  return v;
}

template <int L, int V>
__global__ __launch_bounds__(kRouteBlock) void moe_topk_kernel(const float* __restrict__ logits, long long ld,
                                                               float* __restrict__ probs, int* __restrict__ expert,
                                                               float* __restrict__ gate, int T, int E, int k) {
  static_assert(kMoeMaxTopk <= 8 && L >= 8 && L * V <= kMoeMaxExperts, "lane j of a row keeps winner j");
  const int lane = threadIdx.x & 63, sub = lane % L, first = lane - sub;
  const long long t = (static_cast<long long>(blockIdx.x) * (kRouteBlock / kWave) + (threadIdx.x >> 6)) * (kWave / L) + lane / L;
  const bool row = t < T;
  float x[V], p[V];
  float m = -INFINITY;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int e = v * L + sub;
    x[v] = row && e < E ? logits[t * ld + e] : -INFINITY;
    m = fmaxf(m, x[v]);
  }
  m = row_max<L>(m);
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    p[v] = v * L + sub < E ? expf(x[v] - m) : 0.f;
    s += p[v];
  }
  s = row_sum<L>(s);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    p[v] = p[v] / s;
    if (row && v * L + sub < E) probs[t * E + v * L + sub] = p[v];
  }
  unsigned taken = 0;
  int my_id = 0;
  float my_p = 0.f, sel = 0.f;
  for (int j = 0; j < k; ++j) {  // k <= E: every round finds a real key
    u64 best = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int e = v * L + sub;
      const u64 c = e < E && !((taken >> v) & 1) ? route_key(x[v], e) : 0;
      best = c > best ? c : best;
    }
    best = row_max_key<L>(best);
    const int idx = static_cast<int>(~static_cast<uint32_t>(best)) & (L * V - 1);
    const int wv = idx / L, wl = idx % L;
    float pv = p[0];
#pragma unroll
    for (int v = 1; v < V; ++v) pv = wv == v ? p[v] : pv;
    const float pw = __shfl(pv, first + wl, kWave);
    if (sub == wl) taken |= 1u << wv;
    if (sub == j) my_id = idx, my_p = pw;
    sel += pw;  // the same sum in every lane, in selection order
  }
  if (row && sub < k) {
    expert[t * k + sub] = my_id;
    gate[t * k + sub] = my_p / sel;
  }
}

template <int L, int V>
__global__ __launch_bounds__(kRouteBlock) void moe_topk_bwd_kernel(const float* __restrict__ probs,
                                                                   const int* __restrict__ expert,
                                                                   const float* __restrict__ gate,
                                                                   const float* __restrict__ dgate,
                                                                   const float* __restrict__ dprobs,
                                                                   float* __restrict__ dlogits, int T, int E, int k) {
  const int lane = threadIdx.x & 63, sub = lane % L, first = lane - sub;
  const long long t = (static_cast<long long>(blockIdx.x) * (kRouteBlock / kWave) + (threadIdx.x >> 6)) * (kWave / L) + lane / L;
  const bool row = t < T;
  float p[V], dp[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int e = v * L + sub;
    const bool in = row && e < E;
    p[v] = in ? probs[t * E + e] : 0.f;
    dp[v] = in && dprobs ? dprobs[t * E + e] : 0.f;
  }
  if (dgate) {
    // gate_j = p_j / s over the selected: d p_j = (dgate_j - sum_i dgate_i gate_i) / s
    int ej = -1;
    float gd = 0.f, dj = 0.f, pj = 0.f;
    if (row && sub < k) {
      ej = expert[t * k + sub];
      if (static_cast<unsigned>(ej) < static_cast<unsigned>(E)) {
        dj = dgate[t * k + sub];
        gd = dj * gate[t * k + sub];
        pj = probs[t * E + ej];
      } else {
        ej = -1;  // not an expert: no gradient through it, and it matches no column below
      }
    }
    float c = 0.f, s = 0.f;
    for (int j = 0; j < k; ++j) {
      c += __shfl(gd, first + j, kWave);
      s += __shfl(pj, first + j, kWave);
    }
    const float g = (dj - c) / s;
    for (int j = 0; j < k; ++j) {
      const int e = __shfl(ej, first + j, kWave);
      const float gj = __shfl(g, first + j, kWave);
#pragma unroll
      for (int v = 0; v < V; ++v) dp[v] += e == v * L + sub ? gj : 0.f;
    }
  }
  float dot = 0.f;
#pragma unroll
  for (int v = 0; v < V; ++v) dot += p[v] * dp[v];
  dot = row_sum<L>(dot);
#pragma unroll
  for (int v = 0; v < V; ++v)
    if (row && v * L + sub < E) dlogits[t * E + v * L + sub] = p[v] * (dp[v] - dot);
}

// KERNEL<L, V> for the E at hand; GRID(L) blocks.
#define TTDK_MOE_ROUTE(KERNEL, E, ...)                                                                              \
  do {                                                                                                              \
    if ((E) <= 8) hipLaunchKernelGGL((KERNEL<8, 1>), dim3(route_grid(T, 8)), dim3(kRouteBlock), 0, st, __VA_ARGS__); \
    else if ((E) <= 16) hipLaunchKernelGGL((KERNEL<16, 1>), dim3(route_grid(T, 16)), dim3(kRouteBlock), 0, st, __VA_ARGS__); \
    else if ((E) <= 32) hipLaunchKernelGGL((KERNEL<32, 1>), dim3(route_grid(T, 32)), dim3(kRouteBlock), 0, st, __VA_ARGS__); \
    else if ((E) <= 64) hipLaunchKernelGGL((KERNEL<64, 1>), dim3(route_grid(T, 64)), dim3(kRouteBlock), 0, st, __VA_ARGS__); \
    else if ((E) <= 128) hipLaunchKernelGGL((KERNEL<64, 2>), dim3(route_grid(T, 64)), dim3(kRouteBlock), 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<64, 4>), dim3(route_grid(T, 64)), dim3(kRouteBlock), 0, st, __VA_ARGS__);       \
  } while (0)

inline unsigned route_grid(int T, int L) {
  const int rows = (kRouteBlock / kWave) * (kWave / L);  // token rows per workgroup
  return static_cast<unsigned>((static_cast<long long>(T) + rows - 1) / rows);
}

inline bool route_shape_ok(int T, int E, int k) {
  return T >= 0 && T <= kMaxRows && E >= 1 && E <= kMoeMaxExperts && k >= 1 && k <= kMoeMaxTopk && k <= E;
}

// ------------------------------------------------------------------------------ counting sort
__device__ __forceinline__ int sort_key(int id, int E) {
  return static_cast<unsigned>(id) < static_cast<unsigned>(E) ? id : E;
}

__global__ __launch_bounds__(kSortBlock) void moe_hist_kernel(const int* __restrict__ expert, int S, int E,
                                                              int* __restrict__ ws) {
  extern __shared__ int hist[];  // E + 1 counters
  for (int i = threadIdx.x; i <= E; i += kSortBlock) hist[i] = 0;
  __syncthreads();
  const long long base = static_cast<long long>(blockIdx.x) * kSortChunk;
  for (int i = threadIdx.x; i < kSortChunk; i += kSortBlock)
    if (base + i < S) atomicAdd(&hist[sort_key(expert[base + i], E)], 1);
  __syncthreads();
  int* const w = ws + static_cast<long long>(blockIdx.x) * (E + 1);
  for (int i = threadIdx.x; i <= E; i += kSortBlock) w[i] = hist[i];
}

// ws[c][e] <- sum of ws[c' < c][e]; offsets[e] <- sum of every count of the experts < e, e = 0..E.
__global__ __launch_bounds__(kSortBlock) void moe_scan_kernel(int* __restrict__ ws, int chunks, int E,
                                                              int* __restrict__ offsets) {
  __shared__ int wsum[kSortBlock / kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int e0 = 0; e0 <= E; e0 += kSortBlock) {
    const int e = e0 + threadIdx.x;
    int run = 0;
    if (e <= E) {
      int* q = ws + e;
      for (int c = 0; c < chunks; ++c, q += E + 1) {
        const int h = *q;
        *q = run;
        run += h;
      }
    }
    int inc = run;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int v = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += v;
    }
    if (lane == kWave - 1) wsum[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSortBlock / kWave; ++w) {
      before += w < wave ? wsum[w] : 0;
      total += wsum[w];
    }
    if (e <= E) offsets[e] = carry + before + inc - run;
    carry += total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kWave) void moe_scatter_kernel(const int* __restrict__ expert, int S, int E, int nbits,
                                                            const int* __restrict__ ws,
                                                            const int* __restrict__ offsets, int* __restrict__ order,
                                                            int* __restrict__ inv) {
  extern __shared__ int next[];  // E + 1: the sorted row the next slot of expert e goes to
  const int lane = threadIdx.x;
  const int* const w = ws + static_cast<long long>(blockIdx.x) * (E + 1);
  for (int i = lane; i <= E; i += kWave) next[i] = offsets[i] + w[i];
  __syncthreads();
  const long long base = static_cast<long long>(blockIdx.x) * kSortChunk;
  for (int i0 = 0; i0 < kSortChunk && base + i0 < S; i0 += kWave) {
    const long long s = base + i0 + lane;
    const bool active = s < S;
    const int key = active ? sort_key(expert[s], E) : 0;
    u64 peers = __ballot(active);  // ... the active lanes with my key
    for (int b = 0; b < nbits; ++b) {
      const bool bit = (key >> b) & 1;
      const u64 set = __ballot(bit);
      peers &= bit ? set : ~set;
    }
    const int below = __popcll(peers & ((1ull << lane) - 1));
    const int pos = active ? next[key] : 0;
    __syncthreads();
    if (active && below == 0) next[key] = pos + __popcll(peers);
    __syncthreads();
    const int r = pos + below;
    if (active && static_cast<unsigned>(r) < static_cast<unsigned>(S)) {  // holds unless expert[] changed under us
      order[r] = static_cast<int>(s);
      inv[s] = r;
    }
  }
}

inline int sort_max_experts() {
  const int g = ttdk_grouped_gemm_max_groups();
  return g < kSortMaxExperts ? g : kSortMaxExperts;
}
inline long long sort_chunks(long long S) { return (S + kSortChunk - 1) / kSortChunk; }

// --------------------------------------------------------------------------- gather / combine
template <typename T>
struct Row8;  // 8 consecutive columns of a row as fp32

template <>
struct Row8<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float (&f)[8]) {
    unpack8(*reinterpret_cast<const uint4*>(p), f);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&f)[8]) {
    *reinterpret_cast<uint4*>(p) = pack8(f);
  }
};

template <>
struct Row8<float> {
  static __device__ __forceinline__ void load(const float* p, float (&f)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&f)[8]) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
  }
};

// One grid stride in (row, chunk) form: drow rows and drem chunks further.
struct RowStep {
  int per_row;  // D / 8 work items per row
  int drow, drem;
};

inline unsigned row_grid(long long rows, int D, RowStep& st) {
  st.per_row = D / 8;
  long long blocks = (rows * st.per_row + kRowBlock - 1) / kRowBlock;
  if (blocks > kRowMaxBlocks) blocks = kRowMaxBlocks;
  const int stride = static_cast<int>(blocks) * kRowBlock;
  st.drow = stride / st.per_row;
  st.drem = stride % st.per_row;
  return static_cast<unsigned>(blocks);
}

// slot / k for slot < 2^31, k <= 256: (slot * ceil(2^40 / k)) >> 40.
struct DivK {
  u64 magic;
  int shift;
};
// With l = ceil(log2 k): magic = ceil(2^(32 + l) / k) lies in [2^32, 2^33], so slot * magic stays below
// 2^64 for every slot < 2^31, and (slot * magic) >> (32 + l) == slot / k for every slot < 2^32
// (Granlund & Montgomery 1994, theorem 4.2 with N = 32). k = 1: magic = 2^32, shift = 32.
__host__ __device__ constexpr DivK div_magic(int k) {
  int l = 0;
  while ((1 << l) < k) ++l;
  return DivK{((1ull << (32 + l)) + k - 1) / k, 32 + l};
}
__host__ __device__ constexpr long long div_k(int slot, DivK d) {
  return static_cast<long long>((static_cast<u64>(slot) * d.magic) >> d.shift);
}
constexpr bool div_exact(int k) {  // at the ends of the admitted range and around the powers of two
  const DivK d = div_magic(k);
  for (int b = 0; b <= 30; ++b)
    for (long long slot = (1ll << b) - 2 * k; slot <= (1ll << b) + 2 * k; ++slot)
      if (slot >= 0 && slot <= kMaxRows && div_k(static_cast<int>(slot), d) != slot / k) return false;
  return true;
}
static_assert(div_exact(1) && div_exact(2) && div_exact(3) && div_exact(7) && div_exact(8), "slot / k by multiply and shift");
static_assert(div_exact(255), "slot / k by multiply and shift");
static_assert(div_exact(kMaxDivisor), "slot / k by multiply and shift");

template <typename S, typename O>
__global__ __launch_bounds__(kRowBlock) void moe_gather_kernel(const S* __restrict__ src, long long lds,
                                                               const int* __restrict__ idx,
                                                               const float* __restrict__ scale, O* __restrict__ out,
                                                               long long ldo, int rows, int slots, DivK magic,
                                                               RowStep st) {
  const unsigned i0 = blockIdx.x * kRowBlock + threadIdx.x;  // < 2048 * 256
  int r = static_cast<int>(i0 / static_cast<unsigned>(st.per_row));
  int c = static_cast<int>(i0 % static_cast<unsigned>(st.per_row));
  while (r < rows) {
    const int slot = idx[r];
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (static_cast<unsigned>(slot) < static_cast<unsigned>(slots)) {
      Row8<S>::load(src + div_k(slot, magic) * lds + c * 8, f);
      if (scale) {
        const float a = scale[slot];
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] *= a;
      }
    }
    Row8<O>::store(out + r * ldo + c * 8, f);
    c += st.drem;
    r += st.drow;
    if (c >= st.per_row) c -= st.per_row, ++r;
  }
}

// The gather with dgate[idx[r]] = dot(h[r], src[idx[r] / k]) on the way: a wave per output row.
template <typename S, typename O>
__global__ __launch_bounds__(kRowBlock) void moe_gather_dot_kernel(const S* __restrict__ src, long long lds,
                                                                   const int* __restrict__ idx,
                                                                   const float* __restrict__ scale,
                                                                   O* __restrict__ out, long long ldo,
                                                                   const O* __restrict__ h, long long ldh,
                                                                   float* __restrict__ dgate, int rows, int slots,
                                                                   DivK magic, int D) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * (kRowBlock / kWave);
  for (int r = blockIdx.x * (kRowBlock / kWave) + (threadIdx.x >> 6); r < rows; r += nw) {
    const int slot = idx[r];
    const bool valid = static_cast<unsigned>(slot) < static_cast<unsigned>(slots);
    const S* const sp = src + (valid ? div_k(slot, magic) : 0) * lds;
    const float a = valid ? (scale ? scale[slot] : 1.f) : 0.f;
    float acc = 0.f;
    for (int c = lane * 8; c < D; c += kWave * 8) {
      float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, g[8];
      if (valid) Row8<S>::load(sp + c, f);
      Row8<O>::load(h + r * ldh + c, g);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        acc = fmaf(f[i], g[i], acc);
        f[i] *= a;
      }
      Row8<O>::store(out + r * ldo + c, f);
    }
    acc = wave_sum(acc);
    if (valid && lane == 0) dgate[slot] = acc;
  }
}

template <typename S, typename O>
__global__ __launch_bounds__(kRowBlock) void moe_combine_kernel(const S* __restrict__ src, long long lds,
                                                                const int* __restrict__ inv,
                                                                const float* __restrict__ w, O* __restrict__ out,
                                                                long long ldo, int T, int k, int src_rows,
                                                                RowStep st) {
  const unsigned i0 = blockIdx.x * kRowBlock + threadIdx.x;
  int t = static_cast<int>(i0 / static_cast<unsigned>(st.per_row));
  int c = static_cast<int>(i0 % static_cast<unsigned>(st.per_row));
  while (t < T) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const long long s0 = static_cast<long long>(t) * k;
    for (int j = 0; j < k; ++j) {
      const int r = inv[s0 + j];
      if (static_cast<unsigned>(r) >= static_cast<unsigned>(src_rows)) continue;
      float f[8];
      Row8<S>::load(src + r * lds + c * 8, f);
      const float a = w ? w[s0 + j] : 1.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(a, f[i], acc[i]);
    }
    Row8<O>::store(out + t * ldo + c * 8, acc);
    c += st.drem;
    t += st.drow;
    if (c >= st.per_row) c -= st.per_row, ++t;
  }
}

// A [rows, D] operand of the row kernels: dt 0 fp32 / 1 bf16, D and ld multiples of 8, 16-byte base.
inline bool row_operand_ok(const void* p, long long ld, int dt, int D) {
  return p && aligned16(p) && (dt == 0 || dt == 1) && ld >= D && ld % 8 == 0;
}

// F<S, O>(...) for the (src, out) type codes.
#define TTDK_MOE_TYPES(SDT, ODT, CALL)              \
  do {                                              \
    if ((SDT) == 0 && (ODT) == 0) CALL(float, float);     \
    else if ((SDT) == 0) CALL(float, bf16_t);       \
    else if ((ODT) == 0) CALL(bf16_t, float);       \
    else CALL(bf16_t, bf16_t);                      \
  } while (0)

}  // namespace
}  // namespace ttdk

using namespace ttdk;

TTDK_API(int, ttdk_moe_max_experts, ()) { return kMoeMaxExperts; }
TTDK_API(int, ttdk_moe_max_topk, ()) { return kMoeMaxTopk; }
// The largest E of ttdk_moe_sort: everything ttdk_grouped_gemm takes.
TTDK_API(int, ttdk_moe_sort_max_experts, ()) { return sort_max_experts(); }
TTDK_API(int, ttdk_moe_sort_chunk, ()) { return kSortChunk; }
// Threads of the capped grid of ttdk_moe_gather / ttdk_moe_combine (tests size their grid-stride case from it).
TTDK_API(int, ttdk_moe_row_max_threads, ()) { return kRowMaxBlocks * kRowBlock; }

// logits fp32 [T, E] with row stride ld; probs fp32 [T, E], expert int32 [T, k], gate fp32 [T, k]
// contiguous. Outside 1 <= k <= min(E, ttdk_moe_max_topk()), E <= ttdk_moe_max_experts():
// hipErrorInvalidValue without a launch. T == 0 returns 0 without a launch.
TTDK_API(int, ttdk_moe_topk, (const float* logits, long long ld, float* probs, int* expert, float* gate, int T, int E,
                              int k, hipStream_t st)) {
  if (!route_shape_ok(T, E, k) || ld < E) return hipErrorInvalidValue;
  if (T == 0) return 0;
  if (!logits || !probs || !expert || !gate) return hipErrorInvalidValue;
  TTDK_MOE_ROUTE(moe_topk_kernel, E, logits, ld, probs, expert, gate, T, E, k);
  return hipGetLastError();
}

// dlogits fp32 [T, E] from probs / expert / gate of ttdk_moe_topk and dgate [T, k] and / or dprobs
// [T, E] (either may be null: taken as zeros). All contiguous.
TTDK_API(int, ttdk_moe_topk_bwd, (const float* probs, const int* expert, const float* gate, const float* dgate,
                                  const float* dprobs, float* dlogits, int T, int E, int k, hipStream_t st)) {
  if (!route_shape_ok(T, E, k)) return hipErrorInvalidValue;
  if (T == 0) return 0;
  if (!probs || !dlogits || (dgate && (!expert || !gate))) return hipErrorInvalidValue;
  TTDK_MOE_ROUTE(moe_topk_bwd_kernel, E, probs, expert, gate, dgate, dprobs, dlogits, T, E, k);
  return hipGetLastError();
}

// Bytes of the workspace ttdk_moe_sort needs (the [chunks, E + 1] table); -1 outside the limits.
TTDK_API(long long, ttdk_moe_sort_ws_bytes, (long long S, int E)) {
  if (S < 0 || S > kMaxRows || E < 1 || E > sort_max_experts()) return -1;
  return sort_chunks(S) * (E + 1) * static_cast<long long>(sizeof(int));
}

// expert int32 [S] -> offsets int32 [E + 1], order int32 [S], inv int32 [S]; ws as sized above.
// S == 0 returns 0 without a launch (the caller zeroes offsets).
TTDK_API(int, ttdk_moe_sort, (const int* expert, long long S, int E, int* offsets, int* order, int* inv, int* ws,
                              hipStream_t st)) {
  if (S < 0 || S > kMaxRows || E < 1 || E > sort_max_experts()) return hipErrorInvalidValue;
  if (S == 0) return 0;
  if (!expert || !offsets || !order || !inv || !ws) return hipErrorInvalidValue;
  const unsigned chunks = static_cast<unsigned>(sort_chunks(S));
  const unsigned lds = static_cast<unsigned>(E + 1) * sizeof(int);
  int nbits = 0;
  while ((E >> nbits) != 0) ++nbits;  // keys are 0 .. E
  hipLaunchKernelGGL(moe_hist_kernel, dim3(chunks), dim3(kSortBlock), lds, st, expert, static_cast<int>(S), E, ws);
  hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(kSortBlock), 0, st, ws, static_cast<int>(chunks), E, offsets);
  hipLaunchKernelGGL(moe_scatter_kernel, dim3(chunks), dim3(kWave), lds, st, expert, static_cast<int>(S), E, nbits, ws,
                     offsets, order, inv);
  return hipGetLastError();
}

// out[r, :D] = scale[idx[r]] * src[idx[r] / k, :D] for r < rows; src has src_rows rows, idx entries
// outside [0, src_rows * k) give a zero row. sdt / odt: 0 fp32, 1 bf16; row strides in elements. scale
// fp32 [src_rows * k] or null. With h (type odt, [rows, D], stride ldh) and dgate (fp32 [src_rows * k])
// also dgate[idx[r]] = dot(h[r], src[idx[r] / k]); both or neither.
TTDK_API(int, ttdk_moe_gather, (const void* src, long long lds, int sdt, const int* idx, const float* scale, void* out,
                                long long ldo, int odt, const void* h, long long ldh, float* dgate, long long rows,
                                long long src_rows, int k, int D, hipStream_t st)) {
  if (rows < 0 || rows > kMaxRows || src_rows < 0 || k < 1 || k > kMaxDivisor || src_rows * k > kMaxRows) return hipErrorInvalidValue;
  if (D < 8 || D % 8) return hipErrorInvalidValue;
  if ((h == nullptr) != (dgate == nullptr)) return hipErrorInvalidValue;
  if (rows == 0) return 0;
  if (!idx || !row_operand_ok(src, lds, sdt, D) || !row_operand_ok(out, ldo, odt, D)) return hipErrorInvalidValue;
  if (h && !row_operand_ok(h, ldh, odt, D)) return hipErrorInvalidValue;
  const int n = static_cast<int>(rows), slots = static_cast<int>(src_rows * k);
  const DivK magic = div_magic(k);
  if (h) {
    long long blocks = (rows + kRowBlock / kWave - 1) / (kRowBlock / kWave);
    if (blocks > kRowMaxBlocks) blocks = kRowMaxBlocks;
#define TTDK_CALL(S, O)                                                                                           \
  hipLaunchKernelGGL((moe_gather_dot_kernel<S, O>), dim3(static_cast<unsigned>(blocks)), dim3(kRowBlock), 0, st,  \
                     static_cast<const S*>(src), lds, idx, scale, static_cast<O*>(out), ldo,                      \
                     static_cast<const O*>(h), ldh, dgate, n, slots, magic, D)
    TTDK_MOE_TYPES(sdt, odt, TTDK_CALL);
#undef TTDK_CALL
  } else {
    RowStep step;
    const unsigned blocks = row_grid(rows, D, step);
#define TTDK_CALL(S, O)                                                                                    \
  hipLaunchKernelGGL((moe_gather_kernel<S, O>), dim3(blocks), dim3(kRowBlock), 0, st,                      \
                     static_cast<const S*>(src), lds, idx, scale, static_cast<O*>(out), ldo, n, slots, magic, step)
    TTDK_MOE_TYPES(sdt, odt, TTDK_CALL);
#undef TTDK_CALL
  }
  return hipGetLastError();
}

// out[t, :D] = sum_{j < k} w[t, j] * src[inv[t * k + j], :D] for t < T, fp32 accumulation in
// increasing j; w fp32 [T, k] or null (ones); inv entries outside [0, src_rows) add nothing.
TTDK_API(int, ttdk_moe_combine, (const void* src, long long lds, int sdt, const int* inv, const float* w, void* out,
                                 long long ldo, int odt, long long T, long long src_rows, int k, int D,
                                 hipStream_t st)) {
  if (T < 0 || T > kMaxRows || src_rows < 0 || src_rows > kMaxRows || k < 1 || k > kMaxDivisor || T * k > kMaxRows) return hipErrorInvalidValue;
  if (D < 8 || D % 8) return hipErrorInvalidValue;
  if (T == 0) return 0;
  if (!inv || !row_operand_ok(out, ldo, odt, D)) return hipErrorInvalidValue;
  if (src_rows > 0 && !row_operand_ok(src, lds, sdt, D)) return hipErrorInvalidValue;
  RowStep step;
  const unsigned blocks = row_grid(T, D, step);
#define TTDK_CALL(S, O)                                                                                       \
  hipLaunchKernelGGL((moe_combine_kernel<S, O>), dim3(blocks), dim3(kRowBlock), 0, st,                        \
                     static_cast<const S*>(src), lds, inv, w, static_cast<O*>(out), ldo, static_cast<int>(T), k, \
                     static_cast<int>(src_rows), step)
  TTDK_MOE_TYPES(sdt, odt, TTDK_CALL);
#undef TTDK_CALL
  return hipGetLastError();
}
