// Distance to the class prototype in feature space (include/dd_capi.h states the semantics):
//   dd_class_feature_sums  per-class sums of the feature rows in 2^-24 fixed point (int64)
//   dd_class_centroids     sums / counts -> fp32 centroids (NaN for a poisoned class)
//   dd_proto_scores        || f_b - centroid[y_b] ||_2 per row
//
// The class mean is taken over the whole dataset, across launch chunks, lanes and ranks.  A float
// sum over shards could not be bitwise independent of that layout; an integer sum is exact and
// order-free, so the sums are the same whatever the launch geometry, the row order or the split
// of the rows over calls and ranks.  Integer atomics only, no float atomics.
//
// Sums kernel: a 256-thread workgroup owns a run of consecutive `order` entries and ALL D
// columns (thread t owns columns t, t + 256, ...: at most 16 for D <= 4096, in int64 registers),
// so it sees whole rows and can reject a row with a non-finite or out-of-range element before
// any of it is added.  It accumulates in registers while the class stays the same and issues one
// global 64-bit atomic per column when the class changes and at the end of its run: about
// (n / rows-per-workgroup + C) D atomics with `order` sorted by label, instead of n D.
#include "dd_feat.h"

namespace dd {
namespace proto {

using feat::kMaxD;
using feat::kRows;
using feat::kThreads;
using feat::wave_row_sqdist;

constexpr int64_t kMaxC = 1ll << 20;    // dd_select_topk_by_class's bound
constexpr float kRange = 32768.f;       // |v| < 2^15: |q(v)| < 2^39
constexpr double kScale = 16777216.0;   // 2^24

// q(v) = round-to-nearest-even(v * 2^24); exact in double for |v| < 2^15
__device__ __forceinline__ long long quantise(float v) {
  return __double2ll_rn((double)v * kScale);
}

// CPT columns per thread, R rows in flight per step (R * CPT = 16 loads per thread)
template <int CPT, int R>
__global__ __launch_bounds__(kThreads) void class_sums_kernel(
    const float* __restrict__ feat, const int64_t* __restrict__ labels,
    const int64_t* __restrict__ order, int64_t n, int D, int64_t C, int rows_per_wg,
    long long* __restrict__ sums, int* __restrict__ bad_feat) {
  // bit r: row r of the step holds an element outside the range.  Three slots in rotation: the
  // slot of step s + 1 is cleared before the barrier of step s, after its last readers (step
  // s - 2) have passed the barrier of step s - 1.
  __shared__ unsigned flags[3];
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t i1 = i0 + rows_per_wg < n ? i0 + rows_per_wg : n;
  if (t < 3) flags[t] = 0u;
  __syncthreads();

  long long acc[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) acc[j] = 0;
  int64_t cur = -1;  // the class the registers hold (uniform over the workgroup)

  auto flush = [&]() {
    if (cur >= 0) {
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        const int d = t + j * kThreads;
        if (d < D && acc[j] != 0)
          atomicAdd(reinterpret_cast<unsigned long long*>(sums + cur * D + d),
                    (unsigned long long)acc[j]);
        acc[j] = 0;
      }
    }
  };

  int step = 0;
  for (int64_t i = i0; i < i1; i += R, ++step) {
    float v[R][CPT];
    int64_t y[R];
    unsigned bad = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      y[r] = -1;
      if (i + r < i1) {
        const int64_t row = order ? order[i + r] : i + r;
        if (row >= 0 && row < n) {  // an `order` entry outside [0, n) names no row
          const int64_t lab = labels[row];
          if (lab >= 0 && lab < C) {
            y[r] = lab;
            const float* __restrict__ x = feat + row * (int64_t)D;
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
              const int d = t + j * kThreads;
              v[r][j] = d < D ? x[d] : 0.f;
              if (!(fabsf(v[r][j]) < kRange)) bad |= 1u << r;  // NaN, inf, |v| >= 2^15
            }
          }
        }
      }
    }
    const int slot = step % 3;
    if (bad) atomicOr(&flags[slot], bad);
    if (t == 0) flags[(step + 1) % 3] = 0u;
    __syncthreads();
    const unsigned rowbad = flags[slot];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (y[r] < 0) continue;  // (uniform: past the run, or a label outside [0, C))
      if (rowbad >> r & 1u) {
        if (t == 0) atomicAdd(bad_feat + y[r], 1);
        continue;
      }
      if (y[r] != cur) {
        flush();
        cur = y[r];
      }
#pragma unroll
      for (int j = 0; j < CPT; ++j) acc[j] += quantise(v[r][j]);  // (columns >= D add 0)
    }
  }
  flush();
}

template <int CPT>
static void launch_class_sums(const float* feat, const int64_t* labels, const int64_t* order,
                              int64_t n, int D, int64_t C, long long* sums, int* bad_feat,
                              hipStream_t st) {
  constexpr int R = 16 / CPT;
  // rows per workgroup: ~4 workgroups per CU, at least 32 rows (the flushes per row fall with
  // it).  The sums are exact integers: the geometry changes no result.
  int64_t rows = ceil_div(n, 4 * (int64_t)device_cus());
  rows = rows < 32 ? 32 : rows;
  rows = ceil_div(rows, R) * R;
  class_sums_kernel<CPT, R><<<(unsigned)ceil_div(n, rows), kThreads, 0, st>>>(
      feat, labels, order, n, D, C, (int)rows, sums, bad_feat);
}

__global__ __launch_bounds__(kThreads) void centroids_kernel(
    const long long* __restrict__ sums, const int64_t* __restrict__ counts,
    const int* __restrict__ bad_feat, int64_t total, int D, float* __restrict__ centroids) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
    const int64_t c = i / D;
    const int64_t cnt = counts[c];
    float out = 0.f;  // an empty class: nothing reads it
    if (bad_feat[c] != 0)
      out = __builtin_nanf("");
    else if (cnt > 0)
      out = (float)(((double)sums[i] / (double)cnt) * (1.0 / kScale));
    centroids[i] = out;
  }
}

// one row per wave64 (dd_logit_scores' mid-width dispatch), reduced by feat::wave_row_sqdist:
// scalar loads (no alignment-dependent path), an order of additions that depends on D alone
__global__ __launch_bounds__(kThreads) void proto_scores_kernel(
    const float* __restrict__ feat, const int64_t* __restrict__ labels,
    const float* __restrict__ centroids, int64_t B, int D, int64_t C, float* __restrict__ score,
    float* __restrict__ accum) {
  const int lane = threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / kWave;
  if (row >= B) return;  // (a whole wave: the shuffles below stay within one wave)
  const int64_t y = labels[row];
  const bool bad_label = y < 0 || y >= C;
  bool bad;
  const float s = wave_row_sqdist(feat + row * (int64_t)D,
                                  centroids + (bad_label ? 0 : y) * (int64_t)D, D, lane, true, &bad);
  if (lane == 0) {
    const float r = (bad_label || bad) ? __builtin_nanf("") : sqrtf(s);
    if (score) score[row] = r;
    if (accum) accum[row] += r;
  }
}

static bool dims_ok(const char* what, int64_t n, int32_t D, int64_t C) {
  if (n < 0 || n >= (1ll << 31)) {
    set_error("%s: need 0 <= n < 2^31 (n=%lld)", what, (long long)n);
    return false;
  }
  if (D < 1 || D > kMaxD) {
    set_error("%s: need 1 <= D <= %d (D=%d)", what, kMaxD, D);
    return false;
  }
  if (C < 1 || C > kMaxC) {
    set_error("%s: need 1 <= C <= 2^20 (C=%lld)", what, (long long)C);
    return false;
  }
  return true;
}

}  // namespace proto
}  // namespace dd

using namespace dd;

extern "C" {

int dd_class_feature_sums(const float* feat, const int64_t* labels, const int64_t* order,
                          int64_t n, int32_t D, int64_t C, int64_t* sums, int32_t* bad_feat,
                          void* stream) {
  clear_error();
  if (!proto::dims_ok("dd_class_feature_sums", n, D, C)) return DD_EINVAL;
  DD_REQUIRE(sums != nullptr && bad_feat != nullptr,
             "dd_class_feature_sums: null sums / bad_feat");
  if (n == 0) return DD_OK;
  DD_REQUIRE(feat != nullptr && labels != nullptr, "dd_class_feature_sums: null feat / labels");
  hipStream_t st = as_stream(stream);
  long long* s = reinterpret_cast<long long*>(sums);
  if (D <= 256)
    proto::launch_class_sums<1>(feat, labels, order, n, D, C, s, bad_feat, st);
  else if (D <= 512)
    proto::launch_class_sums<2>(feat, labels, order, n, D, C, s, bad_feat, st);
  else if (D <= 1024)
    proto::launch_class_sums<4>(feat, labels, order, n, D, C, s, bad_feat, st);
  else if (D <= 2048)
    proto::launch_class_sums<8>(feat, labels, order, n, D, C, s, bad_feat, st);
  else
    proto::launch_class_sums<16>(feat, labels, order, n, D, C, s, bad_feat, st);
  DD_CHECK_LAUNCH("dd_class_feature_sums");
  return DD_OK;
}

int dd_class_centroids(const int64_t* sums, const int64_t* counts, const int32_t* bad_feat,
                       int64_t C, int32_t D, float* centroids, void* stream) {
  clear_error();
  if (!proto::dims_ok("dd_class_centroids", 0, D, C)) return DD_EINVAL;
  DD_REQUIRE(sums != nullptr && counts != nullptr && bad_feat != nullptr && centroids != nullptr,
             "dd_class_centroids: null buffer");
  const int64_t total = C * D;
  const int64_t nb = ceil_div(total, proto::kThreads);
  proto::centroids_kernel<<<(unsigned)(nb < 65536 ? nb : 65536), proto::kThreads, 0,
                            as_stream(stream)>>>(reinterpret_cast<const long long*>(sums),
                                                 counts, bad_feat, total, D, centroids);
  DD_CHECK_LAUNCH("dd_class_centroids");
  return DD_OK;
}

int dd_proto_scores(const float* feat, const int64_t* labels, const float* centroids, int64_t B,
                    int32_t D, int64_t C, float* score, float* accum, void* stream) {
  clear_error();
  if (!proto::dims_ok("dd_proto_scores", B, D, C)) return DD_EINVAL;
  DD_REQUIRE(score != nullptr || accum != nullptr,
             "dd_proto_scores: no output requested (score and accum both null)");
  if (B == 0) return DD_OK;
  DD_REQUIRE(feat != nullptr && labels != nullptr && centroids != nullptr,
             "dd_proto_scores: null feat / labels / centroids");
  proto::proto_scores_kernel<<<(unsigned)ceil_div(B, proto::kRows), proto::kThreads, 0,
                               as_stream(stream)>>>(feat, labels, centroids, B, D, C, score,
                                                    accum);
  DD_CHECK_LAUNCH("dd_proto_scores");
  return DD_OK;
}

}  // extern "C"
