// Distance to the nearest k-means centroid in feature space (include/dd_capi.h states the
// semantics):
//   dd_kmeans_workspace_bytes  bytes of the workspace of the dd_kmeans_assign calls of one run
//   dd_kmeans_assign           one Lloyd assignment: per row the nearest centroid and its distance,
//                              and the fixed-point sums and counts of the rows each centroid took
//   dd_kmeans_centroids        sums / counts -> the fp32 centroids, in place (an empty cluster
//                              keeps its centroid)
//
// dd_kmeans_assign on one stream, no allocation, no synchronisation, integer atomics only;
// dd_feat.h defines the pack, the key scan and the row reducer:
//   pack    feat::pack_kernel on the Kc centroids (every call: they move) and, with repack_rows,
//           on the rows (once per run: they do not; the centroids' ids 0 .. Kc - 1, which
//           scan_keys stages beside the norms, are written with them).
//   assign  a 256-thread workgroup owns a tile of 128 rows, which it reads from HBM once, and runs
//           three phases:
//     search  feat::scan_keys over the centroids [0, Kc), 128 at a time through LDS.  The scan
//             leaves the ROW on the lane, so the running minimum of (key, cluster) is per lane and
//             the two lane halves are combined with one cross-lane exchange; one pick per row goes
//             to LDS.
//     value   wave w takes rows 32 w .. of the tile one at a time: the range test of the
//             fixed-point sums (a row that fails it has pick -1) and
//             sqrt(feat::wave_row_sqdist(row, centroid[pick])).
//     sums    the grouped sum WITHOUT a global sort: the tile's 128 (pick, position) pairs are
//             ranked by comparison in LDS (128 x 128, whatever Kc), then thread t owns columns t,
//             t + 256, ... in int64 registers (dd_class_feature_sums' layout), walks the tile's
//             rows in cluster order, adds q(f) while the cluster stays the same and issues one
//             64-bit atomic per column when it changes and at the end of the tile; one thread
//             counts the rows the same way.  About (n / 128) min(128, clusters met in the tile) D
//             atomics instead of n D.
//
// Invariance: a key is a function of the row, the centroid and D alone (dd_feat.h), the minimum of
// (key, cluster) pairs under one total order does not depend on the order in which they are met,
// and the sums are exact integers.  So every output depends on the row SET and the centroids, not
// on the tiling of the rows, their order, the split of the rows over calls or the launch geometry.
#include "dd_feat.h"

namespace dd {
namespace kmeans {

using namespace feat;

constexpr float kRange = 32768.f;      // |v| < 2^15: |q(v)| < 2^39 (dd_class_feature_sums' rule)
constexpr double kScale = 16777216.0;  // 2^24

// q(v) = round-to-nearest-even(v * 2^24); exact in double for |v| < 2^15
__device__ __forceinline__ long long quantise(float v) {
  return __double2ll_rn((double)v * kScale);
}

// the workspace: feat::PackLayout (the centroids are the candidates, the rows the queries), then
// the centroids' ids 0 .. Kc - 1 as scan_keys stages them
struct Layout : PackLayout {
  int64_t ids, total;
};
static Layout layout(int64_t n, int64_t Kc, int D) {
  Layout L;
  static_cast<PackLayout&>(L) = pack_layout(n, Kc, D);
  L.ids = L.end;
  L.total = L.ids + align256(Kc * 8);
  return L;
}

__global__ __launch_bounds__(kThreads) void ids_kernel(int64_t* __restrict__ ids, int Kc) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j < Kc) ids[j] = j;
}

// (key, j) < (bkey, bj) lexicographically; a NaN key is never smaller; j < 0: no pair
__device__ __forceinline__ bool pair_less(float key, int j, float bkey, int bj) {
  return j >= 0 && (key < bkey || (key == bkey && (bj < 0 || j < bj)));
}

// feat::scan_keys' epilogue: one lane's running minimum of (key, cluster).  A centroid past Kc or
// with a non-finite element has a NaN key (never smaller).
struct Pick {
  float key = INFINITY;
  int id = -1;  // the cluster; -1: none yet
  __device__ __forceinline__ void operator()(float k, int lr, int64_t c0) {
    const int j = (int)c0 + lr;
    if (pair_less(k, j, key, id)) {
      key = k;
      id = j;
    }
  }
};

// x holds a NaN, an infinity or |v| >= 2^15 (the same answer on every lane of the row's wave)
__device__ __forceinline__ bool wave_row_unrepresentable(const float* __restrict__ x, int D,
                                                         int lane) {
  float bad = 0.f;
  for (int d = lane; d < D; d += kWave) bad = fabsf(x[d]) < kRange ? bad : 1.f;
  return group_max<kWave>(bad) != 0.f;
}

// CPT columns per thread in the sums phase, R rows in flight per step (R * CPT = 16 loads per
// thread).  Any of sums (with counts) / assign / dist / accum may be null.
template <bool F16, int CPT>
__global__ __launch_bounds__(kThreads) void assign_kernel(
    const float* __restrict__ rows, int64_t n, const uint16_t* __restrict__ q_hi,
    const uint16_t* __restrict__ q_lo, const float* __restrict__ cent,
    const uint16_t* __restrict__ c_hi, const uint16_t* __restrict__ c_lo,
    const float* __restrict__ c_norm, const int64_t* __restrict__ c_id, int Kc, int D, int Dp,
    long long* __restrict__ sums, long long* __restrict__ counts, long long* __restrict__ bad,
    int* __restrict__ assign, float* __restrict__ dist, float* __restrict__ accum) {
  constexpr int R = 16 / CPT;
  __shared__ ScanLds lds;
  __shared__ int s_pick[TQ];   // the tile's picks (-1: no row, no admissible centroid, a bad row)
  __shared__ int s_order[TQ];  // the tile positions with a pick, in (pick, position) order
  __shared__ int s_live;       // how many

  const int tid = threadIdx.x;
  const int lane = tid % kWave, wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * TQ;

  // ---- search ----
  {
    const int r = lane & 31, h = lane >> 5;
    const int64_t qr = row0 + wave * 32 + r;  // this lane's row (both lane halves hold it)
    const bool qvalid = qr < n;
    const uint16_t* __restrict__ qh_row = q_hi + (qvalid ? qr : 0) * (int64_t)Dp;
    const uint16_t* __restrict__ ql_row = q_lo + (qvalid ? qr : 0) * (int64_t)Dp;
    Pick best;
    scan_keys<F16>(lds, qh_row, ql_row, qvalid, c_hi, c_lo, c_norm, c_id, 0, Kc, Dp, best);
    // the other lane half holds the same row's other centroids
    const float o_key = __shfl_xor(best.key, 32, kWave);
    const int o_id = __shfl_xor(best.id, 32, kWave);
    if (pair_less(o_key, o_id, best.key, best.id)) best.id = o_id;
    if (h == 0) s_pick[wave * 32 + r] = qvalid ? best.id : -1;
  }
  __syncthreads();

  // ---- value: wave w owns tile positions 32 w .. 32 w + 31 ----
  const bool want_value = dist != nullptr || accum != nullptr;
  int nbad = 0;
  for (int i = 0; i < 32; ++i) {
    const int t = wave * 32 + i;
    const int64_t row = row0 + t;
    if (row >= n) break;  // (a whole wave)
    const float* __restrict__ x = rows + row * (int64_t)D;
    const bool unrep = wave_row_unrepresentable(x, D, lane);
    const int p = unrep ? -1 : s_pick[t];
    const bool has = p >= 0;
    const float s = wave_row_sqdist(x, cent + (has ? p : 0) * (int64_t)D, D, lane,
                                    has && want_value, nullptr);
    if (lane == 0) {
      if (unrep) {
        s_pick[t] = -1;
        ++nbad;
      }
      const float d = has ? sqrtf(s) : __builtin_nanf("");
      if (assign) assign[row] = p;
      if (dist) dist[row] = d;
      if (accum) accum[row] += d;
    }
  }
  if (lane == 0 && nbad)
    atomicAdd(reinterpret_cast<unsigned long long*>(bad), (unsigned long long)nbad);
  if (!sums) return;  // (uniform)
  __syncthreads();

  // ---- sums: rank the (pick, position) pairs, then walk the rows in cluster order ----
  if (tid < TQ) {
    const int p = s_pick[tid];
    int rank = 0, live = 0;
    for (int u = 0; u < TQ; ++u) {
      const int o = s_pick[u];  // (every thread reads the same word: a broadcast)
      live += o >= 0;
      rank += o >= 0 && (o < p || (o == p && u < tid));
    }
    if (p >= 0) s_order[rank] = tid;
    if (tid == 0) s_live = live;
  }
  __syncthreads();
  const int m = s_live;

  long long acc[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) acc[j] = 0;
  long long cnt = 0;
  int cur = -1;  // the cluster the registers hold (uniform over the workgroup)

  auto flush = [&]() {
    if (cur >= 0) {
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        const int d = tid + j * kThreads;
        if (d < D && acc[j] != 0)
          atomicAdd(reinterpret_cast<unsigned long long*>(sums + cur * (int64_t)D + d),
                    (unsigned long long)acc[j]);
        acc[j] = 0;
      }
      if (tid == 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(counts + cur), (unsigned long long)cnt);
      cnt = 0;
    }
  };

  for (int k = 0; k < m; k += R) {
    float v[R][CPT];
    int c[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      c[r] = -1;
      if (k + r < m) {
        const int t = s_order[k + r];
        c[r] = s_pick[t];
        const float* __restrict__ x = rows + (row0 + t) * (int64_t)D;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
          const int d = tid + j * kThreads;
          v[r][j] = d < D ? x[d] : 0.f;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (c[r] < 0) continue;  // (uniform: past the tile's last row with a pick)
      if (c[r] != cur) {
        flush();
        cur = c[r];
      }
#pragma unroll
      for (int j = 0; j < CPT; ++j) acc[j] += quantise(v[r][j]);  // (columns >= D add 0)
      ++cnt;
    }
  }
  flush();
}

__global__ __launch_bounds__(kThreads) void centroids_kernel(
    const long long* __restrict__ sums, const long long* __restrict__ counts, int64_t total, int D,
    float* __restrict__ centroids) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
    const long long cnt = counts[i / D];
    if (cnt > 0) centroids[i] = (float)(((double)sums[i] / (double)cnt) * (1.0 / kScale));
  }
}

static bool dims_ok(const char* what, int64_t n, int32_t Kc, int32_t D, int32_t operands) {
  if (n < 0 || n >= (1ll << 31)) {
    if (what) set_error("%s: need 0 <= n < 2^31 (n=%lld)", what, (long long)n);
    return false;
  }
  if (!rows_dims_ok(what, 0, 0, D, operands)) return false;
  if (Kc < 1 || Kc > DD_KMEANS_MAX_K) {
    if (what) set_error("%s: need 1 <= Kc <= %d (Kc=%d)", what, DD_KMEANS_MAX_K, Kc);
    return false;
  }
  return true;
}

struct Args {
  const float* rows;
  int64_t n;
  const float* cent;
  int Kc, D;
  bool repack;
  long long *sums, *counts, *bad;
  int* assign;
  float *dist, *accum;
};

template <bool F16, int CPT>
static void launch_assign(const Args& a, char* ws, const Layout& L, hipStream_t st) {
  assign_kernel<F16, CPT><<<(unsigned)ceil_div(a.n, TQ), kThreads, 0, st>>>(
      a.rows, a.n, at<uint16_t>(ws, L.q_hi), at<uint16_t>(ws, L.q_lo), a.cent,
      at<uint16_t>(ws, L.c_hi), at<uint16_t>(ws, L.c_lo), at<float>(ws, L.c_norm),
      at<int64_t>(ws, L.ids), a.Kc, a.D, L.Dp, a.sums, a.counts, a.bad, a.assign, a.dist,
      a.accum);
}

template <bool F16>
static void launch(const Args& a, char* ws, const Layout& L, hipStream_t st) {
  pack_kernel<F16><<<(unsigned)ceil_div(a.Kc, kRows), kThreads, 0, st>>>(
      a.cent, a.Kc, a.D, L.Dp, at<uint16_t>(ws, L.c_hi), at<uint16_t>(ws, L.c_lo),
      at<float>(ws, L.c_norm), nullptr);
  if (a.repack) {  // what stays the same over a run's calls: the rows' halves and the ids
    ids_kernel<<<(unsigned)ceil_div(a.Kc, kThreads), kThreads, 0, st>>>(at<int64_t>(ws, L.ids),
                                                                        a.Kc);
    pack_kernel<F16><<<(unsigned)ceil_div(a.n, kRows), kThreads, 0, st>>>(
        a.rows, a.n, a.D, L.Dp, at<uint16_t>(ws, L.q_hi), at<uint16_t>(ws, L.q_lo), nullptr,
        nullptr);
  }
  if (a.D <= 2 * kThreads)
    launch_assign<F16, 2>(a, ws, L, st);
  else if (a.D <= 4 * kThreads)
    launch_assign<F16, 4>(a, ws, L, st);
  else
    launch_assign<F16, 16>(a, ws, L, st);
}

}  // namespace kmeans
}  // namespace dd

using namespace dd;

extern "C" {

size_t dd_kmeans_workspace_bytes(int64_t n, int32_t Kc, int32_t D, int32_t operands) {
  if (!kmeans::dims_ok(nullptr, n, Kc, D, operands)) return 0;
  return (size_t)kmeans::layout(n, Kc, D).total;
}

int dd_kmeans_assign(const float* rows, int64_t n, const float* centroids, int32_t Kc, int32_t D,
                     int32_t operands, int32_t repack_rows, int64_t* sums, int64_t* counts,
                     int64_t* bad, int32_t* assign, float* dist, float* accum, void* workspace,
                     size_t workspace_bytes, void* stream) {
  clear_error();
  if (!kmeans::dims_ok("dd_kmeans_assign", n, Kc, D, operands)) return DD_EINVAL;
  DD_REQUIRE((sums != nullptr) == (counts != nullptr),
             "dd_kmeans_assign: sums and counts go together (one of them is null)");
  DD_REQUIRE(sums != nullptr || assign != nullptr || dist != nullptr || accum != nullptr,
             "dd_kmeans_assign: no output requested (sums / counts, assign, dist and accum all "
             "null)");
  if (n == 0) return DD_OK;
  DD_REQUIRE(rows != nullptr && centroids != nullptr && bad != nullptr,
             "dd_kmeans_assign: null rows / centroids / bad");
  const kmeans::Layout L = kmeans::layout(n, Kc, D);
  DD_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)L.total,
             "dd_kmeans_assign: workspace of %zu bytes, need %lld (dd_kmeans_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, (long long)L.total);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_kmeans_assign: the workspace must be 16-byte aligned");
  const kmeans::Args a = {rows, n, centroids, Kc, D, repack_rows != 0,
                          reinterpret_cast<long long*>(sums), reinterpret_cast<long long*>(counts),
                          reinterpret_cast<long long*>(bad), assign, dist, accum};
  char* ws = static_cast<char*>(workspace);
  if (operands == DD_OPERANDS_F16X3)
    kmeans::launch<true>(a, ws, L, as_stream(stream));
  else
    kmeans::launch<false>(a, ws, L, as_stream(stream));
  DD_CHECK_LAUNCH("dd_kmeans_assign");
  return DD_OK;
}

int dd_kmeans_centroids(const int64_t* sums, const int64_t* counts, int32_t Kc, int32_t D,
                        float* centroids, void* stream) {
  clear_error();
  if (!kmeans::dims_ok("dd_kmeans_centroids", 0, Kc, D, DD_OPERANDS_F16X3)) return DD_EINVAL;
  DD_REQUIRE(sums != nullptr && counts != nullptr && centroids != nullptr,
             "dd_kmeans_centroids: null buffer");
  const int64_t total = (int64_t)Kc * D;
  kmeans::centroids_kernel<<<(unsigned)ceil_div(total, kmeans::kThreads), kmeans::kThreads, 0,
                             as_stream(stream)>>>(reinterpret_cast<const long long*>(sums),
                                                  reinterpret_cast<const long long*>(counts),
                                                  total, D, centroids);
  DD_CHECK_LAUNCH("dd_kmeans_centroids");
  return DD_OK;
}

}  // extern "C"
