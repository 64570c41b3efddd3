// Distance to the nearest neighbour of the same class in feature space (include/dd_capi.h
// states the semantics):
//   dd_nn_workspace_bytes  bytes of the workspace of one dd_nn_same_class call (host only)
//   dd_nn_same_class       per query row: the nearest other row of its class and its distance
//
// Three steps on one stream, no allocation, no synchronisation, no atomics; dd_feat.h defines
// the pack, the key scan and the row reducer:
//   pack    feat::pack_kernel on every row of the call, exactly once; the queries' picks = -1.
//   search  a 256-thread workgroup owns 128 queries of ONE class and runs feat::scan_keys over
//           that class's candidates.  The scan leaves the QUERY on the lane, so the running
//           minimum of (key, id) is per lane, and only the two lane halves are combined at the
//           end.
//   value   one wave per query: sqrt(feat::wave_row_sqdist(q, c[pick])).
//
// Invariance: a key is a function of the two rows and D alone (dd_feat.h), and the minimum of
// (key, id) pairs under one total order does not depend on the order in which the pairs are met.
// So the pick depends on the query row and on the candidate SET of its class, not on the
// batching of the queries, on nq, on positions or on the launch geometry.
#include "dd_feat.h"

namespace dd {
namespace nn {

using namespace feat;

constexpr int64_t kMaxC = 1ll << 20;   // dd_select_topk_by_class's bound

// the workspace: feat::PackLayout, then [pick] int32 [nq]
struct Layout : PackLayout {
  int64_t pick, total;
};
static Layout layout(int64_t nq, int64_t nc, int D) {
  Layout L;
  static_cast<PackLayout&>(L) = pack_layout(nq, nc, D);
  L.pick = L.end;
  L.total = L.pick + align256(nq * 4);
  return L;
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// (key, id) < (bkey, bid) lexicographically; a NaN key is never smaller
__device__ __forceinline__ bool pair_less(float key, int64_t id, float bkey, int64_t bid) {
  return key < bkey || (key == bkey && id < bid);
}

// feat::scan_keys' epilogue: one lane's running minimum of (key, id).  A ragged candidate has a
// NaN key (never smaller); the query itself is skipped by id.
struct Nearest {
  int64_t my_id;
  const int64_t* s_id;  // the ids scan_keys staged for this step
  float key = INFINITY;
  int64_t id = kNoId;
  int row = -1;
  __device__ __forceinline__ void operator()(float k, int lr, int64_t c0) {
    const int64_t i = s_id[lr];
    if (i != my_id && pair_less(k, i, key, id)) {
      key = k;
      id = i;
      row = (int)(c0 + lr);
    }
  }
};

// Workgroup b serves query tile t of class k where class k owns the tile slots
// [T(k), T(k + 1)), T(k) = q_off[k] / TQ + k: T is computed from the offsets alone (no scan),
// it is increasing, and a class of len rows gets at least ceil(len / TQ) slots.  The grid is
// T(C) = nq / TQ + C workgroups; a slot its class does not need returns at once.
template <bool F16>
__global__ __launch_bounds__(kThreads) void search_kernel(
    const uint16_t* __restrict__ q_hi, const uint16_t* __restrict__ q_lo,
    const int64_t* __restrict__ q_id, const int64_t* __restrict__ q_off, int64_t nq,
    const uint16_t* __restrict__ c_hi, const uint16_t* __restrict__ c_lo,
    const float* __restrict__ c_norm, const int64_t* __restrict__ c_id,
    const int64_t* __restrict__ c_off, int64_t nc, int64_t C, int Dp, int* __restrict__ pick) {
  __shared__ ScanLds lds;

  const int64_t b = blockIdx.x;
  int64_t klo = 0, khi = C - 1;
  while (klo < khi) {  // the last class whose first slot is <= b
    const int64_t mid = (klo + khi + 1) / 2;
    if (clamp64(q_off[mid], 0, nq) / TQ + mid <= b)
      klo = mid;
    else
      khi = mid - 1;
  }
  const int64_t k = klo;
  // offsets that are not increasing or leave the buffers are clamped: never an access outside
  const int64_t qs = clamp64(q_off[k], 0, nq), qe = clamp64(q_off[k + 1], qs, nq);
  const int64_t cs = clamp64(c_off[k], 0, nc), ce = clamp64(c_off[k + 1], cs, nc);
  const int64_t t = b - (qs / TQ + k);
  if (t < 0) return;
  const int64_t q0 = qs + t * TQ;
  if (q0 >= qe) return;  // (uniform over the workgroup)

  const int tid = threadIdx.x;
  const int lane = tid % kWave, wave = tid / kWave;
  const int r = lane & 31, h = lane >> 5;
  const int64_t qr = q0 + wave * 32 + r;  // this lane's query (both lane halves hold it)
  const bool qvalid = qr < qe;
  const int64_t my_id = qvalid ? q_id[qr] : -1;
  const uint16_t* __restrict__ qh_row = q_hi + (qvalid ? qr : 0) * (int64_t)Dp;
  const uint16_t* __restrict__ ql_row = q_lo + (qvalid ? qr : 0) * (int64_t)Dp;

  Nearest best = {my_id, lds.id};
  scan_keys<F16>(lds, qh_row, ql_row, qvalid, c_hi, c_lo, c_norm, c_id, cs, ce, Dp, best);
  // the other lane half holds the same query's other candidates
  const float o_key = __shfl_xor(best.key, 32, kWave);
  const int o_row = __shfl_xor(best.row, 32, kWave);
  const int64_t o_id = shfl_xor64(best.id, 32);
  if (pair_less(o_key, o_id, best.key, best.id)) best.row = o_row;
  if (h == 0 && qvalid) pick[qr] = best.row;  // -1: no admissible candidate
}

// one query per wave64
__global__ __launch_bounds__(kThreads) void value_kernel(
    const float* __restrict__ q, int64_t nq, const float* __restrict__ c,
    const int64_t* __restrict__ c_id, int64_t nc, int D, const int* __restrict__ pick,
    float* __restrict__ dist, int64_t* __restrict__ nn_id, float* __restrict__ accum) {
  const int lane = threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / kWave;
  if (row >= nq) return;  // (a whole wave)
  const int p = pick[row];
  const bool has = p >= 0 && p < nc;
  bool bad;
  const float s = wave_row_sqdist(q + row * (int64_t)D, c + (has ? p : 0) * (int64_t)D, D, lane,
                                  has, &bad);
  if (lane == 0) {
    const float d = bad ? __builtin_nanf("") : (has ? sqrtf(s) : INFINITY);
    if (dist) dist[row] = d;
    if (nn_id) nn_id[row] = (bad || !has) ? -1 : c_id[p];
    if (accum) accum[row] += d;
  }
}

static bool dims_ok(const char* what, int64_t nq, int64_t nc, int32_t D, int64_t C,
                    int32_t operands) {
  if (!rows_dims_ok(what, nq, nc, D, operands)) return false;
  if (C < 1 || C > kMaxC) {
    set_error("%s: need 1 <= C <= 2^20 (C=%lld)", what, (long long)C);
    return false;
  }
  return true;
}

template <bool F16>
static void launch(const float* q, const int64_t* q_id, const int64_t* q_off, int64_t nq,
                   const float* c, const int64_t* c_id, const int64_t* c_off, int64_t nc,
                   int64_t C, int D, char* ws, const Layout& L, hipStream_t st) {
  int* pick = at<int>(ws, L.pick);
  launch_pack<F16>(q, nq, c, nc, D, ws, L, pick, st);
  if (nc > 0)
    search_kernel<F16><<<(unsigned)(nq / TQ + C), kThreads, 0, st>>>(
        at<uint16_t>(ws, L.q_hi), at<uint16_t>(ws, L.q_lo), q_id, q_off, nq,
        at<uint16_t>(ws, L.c_hi), at<uint16_t>(ws, L.c_lo), at<float>(ws, L.c_norm), c_id, c_off,
        nc, C, L.Dp, pick);
}

}  // namespace nn
}  // namespace dd

using namespace dd;

extern "C" {

size_t dd_nn_workspace_bytes(int64_t nq, int64_t nc, int32_t D, int32_t operands) {
  if (!feat::rows_dims_ok(nullptr, nq, nc, D, operands)) return 0;
  return (size_t)nn::layout(nq, nc, D).total;
}

int dd_nn_same_class(const float* q, const int64_t* q_id, const int64_t* q_off, int64_t nq,
                     const float* c, const int64_t* c_id, const int64_t* c_off, int64_t nc,
                     int64_t C, int32_t D, int32_t operands, float* dist, int64_t* nn_id,
                     float* accum, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  if (!nn::dims_ok("dd_nn_same_class", nq, nc, D, C, operands)) return DD_EINVAL;
  DD_REQUIRE(dist != nullptr || nn_id != nullptr || accum != nullptr,
             "dd_nn_same_class: no output requested (dist, nn_id and accum all null)");
  if (nq == 0) return DD_OK;
  DD_REQUIRE(q != nullptr && q_id != nullptr && q_off != nullptr,
             "dd_nn_same_class: null q / q_id / q_off");
  DD_REQUIRE(c_off != nullptr && (nc == 0 || (c != nullptr && c_id != nullptr)),
             "dd_nn_same_class: null c / c_id / c_off");
  const nn::Layout L = nn::layout(nq, nc, D);
  DD_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)L.total,
             "dd_nn_same_class: workspace of %zu bytes, need %lld (dd_nn_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, (long long)L.total);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_nn_same_class: the workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  if (operands == DD_OPERANDS_F16X3)
    nn::launch<true>(q, q_id, q_off, nq, c, c_id, c_off, nc, C, D, ws, L, st);
  else
    nn::launch<false>(q, q_id, q_off, nq, c, c_id, c_off, nc, C, D, ws, L, st);
  nn::value_kernel<<<(unsigned)ceil_div(nq, nn::kRows), nn::kThreads, 0, st>>>(
      q, nq, c, c_id, nc, D, feat::at<const int>(ws, L.pick), dist, nn_id, accum);
  DD_CHECK_LAUNCH("dd_nn_same_class");
  return DD_OK;
}

}  // extern "C"
