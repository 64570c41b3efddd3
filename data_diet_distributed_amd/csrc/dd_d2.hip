// D2 pruning (Maharana, Yadav & Bansal: message passing for balancing diversity and difficulty) on
// a k-nearest-neighbour graph (include/dd_capi.h states the semantics):
//   dd_d2_weights          w = exp(-coef dist^2) per graph slot
//   dd_d2_propagate        forward message passing, one round: a row absorbs its neighbours' scores
//   dd_d2_workspace_bytes  bytes of the workspace of one dd_d2_select call (host only)
//   dd_d2_select           the sequential selection: argmax, retire, reverse messages, repeat
//
// dd_d2_select is two launches on one stream, no allocation, no synchronisation, nothing read back:
//   init    workgroup b copies rows [256 b, 256 b + 256) of x into the workspace (a non-finite score
//           is counted and stored as -inf, "retired", so the loop below is defined on any input),
//           pads the last block with -inf, leaves the block's maximum in the workspace, counts the
//           groups outside [0, G) and fills picked / value with -1.
//   select  ONE workgroup of 1024 threads (16 waves) runs the whole loop.  No other workgroup exists,
//           so nothing waits on another workgroup and the outcome cannot depend on a launch geometry.
//
// The score array stays in the workspace (4 n bytes: L2-resident, 200 KB at N = 50 000, 8 MB at
// the limit); LDS holds a three-level maximum over it with a fan-out one wave covers in one step:
//   m1[b]   the maximum of rows [256 b, 256 b + 256)         <= 8192 entries (32 KiB at n = 2^21)
//   m2[c]   the maximum of m1[64 c .. 64 c + 64)             <= 128 entries
//   top     wave 0 holds m2 two entries per lane
// and the groups' remaining quotas (int32, <= DD_D2_MAX_GROUPS = 16384 of them: 64 KiB).
//
// 256 rows per block, not 64: (a) at 2^21 rows the table is 32 KiB where 64-row blocks need 128 KiB,
// which with the quotas would not fit the 160 KiB of a workgroup; (b) with 64 x 64 x 128 the descent
// top -> m2 entry -> m1 entry -> row is three single-wave steps, so ONE wave walks it without a
// barrier, where 64-row blocks need a fourth level; (c) a block is 1 KiB contiguous: one 16-byte
// load per lane, issued at once, so scanning or recomputing a block costs one L2 round trip exactly
// as a 64-row block would.
//
// One pick:
//   1  wave 0: the maximum M of m2 (group_max, the shuffle butterfly), the lowest m2 entry, then the
//      lowest m1 entry, holding M (ballots), and in that block the lowest row with x == M.  The
//      blocks ascend with the rows, so that is the lowest row holding the maximum.
//   2  wave 0: retire the row (x = -inf); read its group and, on lanes 0 .. k - 1, its k slots; if
//      the group's quota is not exhausted record the pick, and lane j sends slot j's message.  Slots
//      naming the same row are folded in ascending slot order on the last of them, so the result is
//      the sequential one.  The touched blocks (the pick's, then one per slot) go to LDS.
//      --- barrier ---
//   3  wave i recomputes the maximum of touched block i (17 entries at most over 16 waves) -> m1
//      --- barrier ---
//   4  wave i recomputes the m2 entry above touched block i (two waves on one entry compute the same
//      value from the same settled m1) -> m2
//      --- barrier ---
// Workgroup barriers are the only ordering; the waves of a workgroup share their compute unit's
// vector cache, so the barrier's workgroup-scope release / acquire makes wave 0's stores to x
// visible to the recomputing waves.
#include "dd_common.h"

namespace dd {
namespace d2 {

constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / kWave;
constexpr int kBlock = DD_D2_BLOCK_ROWS;  // rows per m1 entry
constexpr int kFan = 64;                  // m1 entries per m2 entry
constexpr int kTop = 128;                 // m2 entries, at most
constexpr int kMaxK = DD_KNN_MAX_K;
constexpr int kTouched = kMaxK + 1;
constexpr int64_t kMaxRows = DD_D2_MAX_ROWS;
constexpr int kMaxGroups = DD_D2_MAX_GROUPS;
static_assert(kMaxRows == (int64_t)kTop * kFan * kBlock, "the three levels cover the row limit");
static_assert(kBlock == 4 * kWave, "a lane takes four consecutive rows of a block");

constexpr int kThreads = 256;

inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }
inline int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

// the workspace: the scores padded to whole blocks, then the blocks' maxima
struct Layout {
  int64_t x, m1, total;
};
static Layout layout(int64_t n) {
  Layout L;
  const int64_t nb = blocks_of(n);
  L.x = 0;
  L.m1 = L.x + align256(nb * kBlock * 4);
  L.total = L.m1 + align256(nb * 4);
  return L;
}

// the select kernel's dynamic LDS: m1 padded to whole m2 entries, m2, the quotas
struct Lds {
  int nb1p, m2_off, quota_off, bytes;
};
static Lds lds_layout(int64_t n, int G) {
  Lds s;
  s.nb1p = (int)((blocks_of(n) + kFan - 1) / kFan * kFan);
  s.m2_off = s.nb1p;
  s.quota_off = s.m2_off + kTop;
  s.bytes = (s.quota_off + G) * 4;
  return s;
}

static bool dims_ok(const char* what, int64_t n, int32_t k, int32_t G) {
  if (n < 0 || n > kMaxRows || k < 1 || k > kMaxK || G < 1 || G > kMaxGroups) {
    if (what)
      set_error("%s: need 0 <= n <= DD_D2_MAX_ROWS = %lld, 1 <= k <= %d, 1 <= G <= "
                "DD_D2_MAX_GROUPS = %d (n=%lld, k=%d, G=%d)", what, (long long)kMaxRows, kMaxK,
                kMaxGroups, (long long)n, k, G);
    return false;
  }
  return true;
}

// The products, sums and differences below are rounded one by one.  hipcc contracts a * b + c to an
// fma by default, also through the __fmul_rn / __fadd_rn of the HIP headers (plain operators
// there), so the unit switches contraction off for its own code and uses operators of its own.
#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

// (false for a NaN)
__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) < INFINITY; }

__global__ __launch_bounds__(kThreads) void weights_kernel(const float* __restrict__ dist,
                                                           const int64_t* __restrict__ nbr,
                                                           int64_t total, float coef,
                                                           float* __restrict__ w) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const float d = dist[e];
  float v = 0.f;
  if (nbr[e] >= 0 && is_finite(d)) v = expf(-mul_rn(mul_rn(coef, d), d));
  w[e] = v;
}

// One thread per row; the slots in ascending order, every product and sum rounded on its own.
__global__ __launch_bounds__(kThreads) void propagate_kernel(const float* __restrict__ x0,
                                                             const int64_t* __restrict__ nbr,
                                                             const float* __restrict__ w,
                                                             int64_t n, int k,
                                                             float* __restrict__ x1,
                                                             int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float own = x0[i];
  float acc = own;
  for (int j = 0; j < k; ++j) {
    const int64_t v = nbr[i * k + j];
    if (v < 0 || v >= n) continue;
    acc = add_rn(acc, mul_rn(w[i * k + j], x0[v]));
  }
  x1[i] = acc;
  if (!is_finite(own) || !is_finite(acc)) atomicAdd(bad, 1);
}

// Workgroup b: block b of the scores (see the head of the file).  The `total` entries of picked /
// value are spread over the grid.
__global__ __launch_bounds__(kBlock) void init_kernel(const float* __restrict__ x,
                                                      const int64_t* __restrict__ group, int64_t n,
                                                      int G, int64_t total, float* __restrict__ xs,
                                                      float* __restrict__ m1,
                                                      int64_t* __restrict__ picked,
                                                      float* __restrict__ value,
                                                      int* __restrict__ bad) {
  __shared__ float s_max[kBlock / kWave];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  float v = -INFINITY;
  int wrong = 0;
  if (i < n) {
    v = x[i];
    if (!is_finite(v)) {
      v = -INFINITY;
      wrong = 1;
    }
    if (group != nullptr) {
      const int64_t g = group[i];
      wrong += g < 0 || g >= G;
    }
  }
  xs[i] = v;  // (the pad of the last block too: the workspace holds whole blocks)
  if (wrong) atomicAdd(bad, wrong);
  const float m = group_max<kWave>(v);
  if (threadIdx.x % kWave == 0) s_max[threadIdx.x / kWave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float b = s_max[0];
#pragma unroll
    for (int wv = 1; wv < kBlock / kWave; ++wv) b = fmaxf(b, s_max[wv]);
    m1[blockIdx.x] = b;
  }
  for (int64_t t = i; t < total; t += (int64_t)gridDim.x * kBlock) {
    picked[t] = -1;
    value[t] = -1.f;
  }
}

// the maximum of block b's 256 rows, on every lane
__device__ __forceinline__ float block_max(const float* xs, int b, int lane) {
  const float4 v = *reinterpret_cast<const float4*>(xs + (int64_t)b * kBlock + 4 * lane);
  return group_max<kWave>(fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
}

__device__ __forceinline__ int first_lane(unsigned long long mask) { return __ffsll(mask) - 1; }

// The whole selection (see the head of the file).  xs is read and written through one plain
// pointer: the barriers order the accesses.
__global__ __launch_bounds__(kSelThreads) void select_kernel(
    float* xs, const float* __restrict__ m1_in, const int64_t* __restrict__ nbr,
    const float* __restrict__ w, const int64_t* __restrict__ group,
    const int64_t* __restrict__ quota, int64_t n, int k, int G, int64_t total, int nb1, int nb1p,
    int64_t* __restrict__ picked, float* __restrict__ value, int* __restrict__ bad) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  float* m1 = s_mem;                                        // [nb1p]
  float* m2 = s_mem + nb1p;                                 // [kTop]
  int* s_quota = reinterpret_cast<int*>(s_mem + nb1p + kTop);  // [G]
  __shared__ int s_touch[kTouched];  // blocks whose maximum is stale (-1: none)
  __shared__ int s_done;

  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  for (int b = tid; b < nb1p; b += kSelThreads) m1[b] = b < nb1 ? m1_in[b] : -INFINITY;
  for (int g = tid; g < G; g += kSelThreads) {
    const int64_t q = quota[g];
    s_quota[g] = q < 0 ? 0 : q > n ? (int)n : (int)q;
  }
  if (tid == 0) s_done = 0;
  __syncthreads();
  for (int c = wave; c < kTop; c += kSelWaves) {
    const float m = c * kFan < nb1p ? group_max<kWave>(m1[c * kFan + lane]) : -INFINITY;
    if (lane == 0) m2[c] = m;
  }
  __syncthreads();

  int64_t t = 0;  // picks recorded (wave 0's copy is the one that counts)
  // every trip retires one row, so n trips end the loop whatever the tables hold
  for (int64_t trip = 0; trip < n; ++trip) {
    if (wave == 0) {
      // stage 1: the maximum and the lowest row holding it
      const float a = m2[lane], b = m2[lane + kWave];
      const float M = group_max<kWave>(fmaxf(a, b));
      int s = -1;
      if (t < total && M > -INFINITY) {
        unsigned long long hit = __ballot(a == M);
        int c = first_lane(hit);
        if (hit == 0ull) c = kWave + first_lane(__ballot(b == M));
        // (a table that named a maximum nothing below holds would end the loop, never index past)
        hit = c >= 0 ? __ballot(m1[c * kFan + lane] == M) : 0ull;
        if (hit != 0ull) {
          const int b1 = c * kFan + first_lane(hit);
          const float4 v = *reinterpret_cast<const float4*>(xs + (int64_t)b1 * kBlock + 4 * lane);
          const int j = v.x == M ? 0 : v.y == M ? 1 : v.z == M ? 2 : v.w == M ? 3 : 4;
          hit = __ballot(j < 4);
          if (hit != 0ull) s = b1 * kBlock + 4 * first_lane(hit) + __shfl(j, first_lane(hit));
        }
      }
      if (s < 0) {
        if (lane == 0) s_done = 1;
      } else {
        // stage 2: retire, the quota, the messages
        const bool slot = lane < k;
        const int64_t g = group != nullptr ? group[s] : 0;
        int64_t v = -1;
        float wj = 0.f;
        if (slot) {
          v = nbr[(int64_t)s * k + lane];
          wj = w[(int64_t)s * k + lane];
        }
        if (lane == 0) xs[s] = -INFINITY;
        const bool in_range = g >= 0 && g < G;
        const bool take = in_range && s_quota[in_range ? g : 0] > 0;
        int touched = -1;
        if (take) {
          const bool valid = slot && v >= 0 && v < n && v != s;
          float xv = valid ? xs[v] : -INFINITY;
          const bool live = xv > -INFINITY;  // (a retired row holds -inf)
          // slots naming one row: slot j folds the messages of slots i <= j in ascending order,
          // and only the last of them stores
          bool last = true;
          for (int i = 0; i < k; ++i) {
            const int64_t vi = __shfl(v, i);
            const float wi = __shfl(wj, i);
            if (vi == v && i <= lane) xv = sub_rn(xv, mul_rn(wi, M));
            if (vi == v && i > lane) last = false;
          }
          if (live) {
            if (last) {
              if (!is_finite(xv)) {  // (an overflow: the row would read as retired)
                atomicAdd(bad, 1);
                xv = -INFINITY;
              }
              xs[v] = xv;
            }
            touched = (int)(v / kBlock);
          }
          if (lane == 0) {
            picked[t] = s;
            value[t] = M;
            s_quota[g] -= 1;
          }
          ++t;
        }
        if (lane < kMaxK) s_touch[1 + lane] = touched;
        if (lane == 0) s_touch[0] = s / kBlock;
      }
    }
    __syncthreads();
    if (s_done) break;
    // stage 3: the touched blocks' maxima
    for (int i = wave; i < kTouched; i += kSelWaves) {
      const int b = s_touch[i];
      if (b < 0) continue;  // (the whole wave)
      const float m = block_max(xs, b, lane);
      if (lane == 0) m1[b] = m;
    }
    __syncthreads();
    // stage 4: the entries above them
    for (int i = wave; i < kTouched; i += kSelWaves) {
      const int b = s_touch[i];
      if (b < 0) continue;
      const int c = b / kFan;
      const float m = group_max<kWave>(m1[c * kFan + lane]);
      if (lane == 0) m2[c] = m;
    }
    __syncthreads();
  }
}

}  // namespace d2
}  // namespace dd

using namespace dd;

extern "C" {

int dd_d2_weights(const float* dist, const int64_t* nbr_id, int64_t n, int32_t k, float coef,
                  float* w, void* stream) {
  clear_error();
  if (!d2::dims_ok("dd_d2_weights", n, k, 1)) return DD_EINVAL;
  DD_REQUIRE(coef >= 0.f && coef < INFINITY,
             "dd_d2_weights: coef must be finite and >= 0 (got %g)", (double)coef);
  if (n == 0) return DD_OK;
  DD_REQUIRE(dist != nullptr && nbr_id != nullptr && w != nullptr,
             "dd_d2_weights: null dist / nbr_id / w");
  const int64_t total = n * k;
  d2::weights_kernel<<<(unsigned)ceil_div(total, d2::kThreads), d2::kThreads, 0,
                       as_stream(stream)>>>(dist, nbr_id, total, coef, w);
  DD_CHECK_LAUNCH("dd_d2_weights");
  return DD_OK;
}

int dd_d2_propagate(const float* x0, const int64_t* nbr_id, const float* w, int64_t n, int32_t k,
                    float* x1, int32_t* bad, void* stream) {
  clear_error();
  if (!d2::dims_ok("dd_d2_propagate", n, k, 1)) return DD_EINVAL;
  if (n == 0) return DD_OK;
  DD_REQUIRE(x0 != nullptr && nbr_id != nullptr && w != nullptr && x1 != nullptr && bad != nullptr,
             "dd_d2_propagate: null x0 / nbr_id / w / x1 / bad");
  DD_REQUIRE(x0 != x1, "dd_d2_propagate: x1 must not be x0 (every row reads the original scores)");
  d2::propagate_kernel<<<(unsigned)ceil_div(n, d2::kThreads), d2::kThreads, 0,
                         as_stream(stream)>>>(x0, nbr_id, w, n, k, x1, bad);
  DD_CHECK_LAUNCH("dd_d2_propagate");
  return DD_OK;
}

size_t dd_d2_workspace_bytes(int64_t n, int32_t G) {
  if (!d2::dims_ok(nullptr, n, 1, G)) return 0;
  return (size_t)d2::layout(n > 0 ? n : 1).total;
}

int dd_d2_select(const float* x, const int64_t* nbr_id, const float* w, const int64_t* group,
                 const int64_t* quota, int64_t n, int32_t k, int32_t G, int64_t total,
                 int64_t* picked, float* value, int32_t* bad, void* workspace,
                 size_t workspace_bytes, void* stream) {
  clear_error();
  if (!d2::dims_ok("dd_d2_select", n, k, G)) return DD_EINVAL;
  DD_REQUIRE(total >= 0 && total <= n, "dd_d2_select: need 0 <= total <= n (total=%lld, n=%lld)",
             (long long)total, (long long)n);
  DD_REQUIRE(group != nullptr || G == 1, "dd_d2_select: G = %d groups need `group`", G);
  if (n == 0) return DD_OK;
  DD_REQUIRE(x != nullptr && nbr_id != nullptr && w != nullptr && quota != nullptr &&
                 bad != nullptr,
             "dd_d2_select: null x / nbr_id / w / quota / bad");
  DD_REQUIRE(total == 0 || (picked != nullptr && value != nullptr),
             "dd_d2_select: null picked / value with total > 0");
  const d2::Layout L = d2::layout(n);
  DD_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)L.total,
             "dd_d2_select: workspace of %zu bytes, need %lld (dd_d2_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, (long long)L.total);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_d2_select: the workspace must be 16-byte aligned");
  char* ws = static_cast<char*>(workspace);
  float* xs = reinterpret_cast<float*>(ws + L.x);
  float* m1 = reinterpret_cast<float*>(ws + L.m1);
  const int nb1 = (int)d2::blocks_of(n);
  const d2::Lds S = d2::lds_layout(n, G);
  hipStream_t st = as_stream(stream);
  d2::init_kernel<<<(unsigned)nb1, d2::kBlock, 0, st>>>(x, group, n, G, total, xs, m1, picked,
                                                        value, bad);
  static bool attr = false;  // the largest LDS any call asks for, set once
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&d2::select_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              d2::lds_layout(d2::kMaxRows, d2::kMaxGroups).bytes);
    attr = true;
  }
  d2::select_kernel<<<1, d2::kSelThreads, (size_t)S.bytes, st>>>(
      xs, m1, nbr_id, w, group, quota, n, k, G, total, nb1, S.nb1p, picked, value, bad);
  DD_CHECK_LAUNCH("dd_d2_select");
  return DD_OK;
}

}  // extern "C"
