// The k nearest neighbours of every row over ALL classes in feature space (include/dd_capi.h
// states the semantics):
//   dd_knn_workspace_bytes  bytes of the workspace of one dd_knn call (host only)
//   dd_knn                  per query row: its k nearest other rows, their distances, the mean
//                           distance and the share of neighbours with another label
//
// Three steps on one stream, no allocation, no synchronisation, no atomics; dd_feat.h defines
// the pack, the key scan and the row reducer:
//   pack    feat::pack_kernel on every row of the call, exactly once.
//   search  a 256-thread workgroup owns 128 queries and ONE of `splits` contiguous candidate
//           segments, over which it runs feat::scan_keys.  The scan leaves the QUERY on the lane:
//           each lane keeps a sorted list of its KCAP smallest (key, row) pairs in registers
//           (KCAP = 1, 4, 8 or 16, the first one >= k); a candidate is compared with the list's
//           worst key first, which rejects almost every one.  The list holds 32-bit row numbers;
//           the 64-bit id is read only to break a key tie.  The two lane halves are merged at the
//           end and the segment's k smallest pairs go to the workspace.
//   merge   one wave per query: the k smallest of its splits * k partial pairs, one per round
//           (a butterfly minimum of (key, id)), and for each sqrt(feat::wave_row_sqdist); then
//           the mean, the label comparison and the accumulators.
//
// Invariance: a key is a function of the two rows and D alone (dd_feat.h), and the k smallest of
// a set of (key, id) pairs under one total order do not depend on how the set is split or
// traversed.  So every output of a row depends on the row, on the candidate SET and on k: not on
// `splits`, the batching of the queries, nq, positions, alignment or the launch geometry.
#include "dd_feat.h"

namespace dd {
namespace knn {

using namespace feat;

constexpr int kMaxK = DD_KNN_MAX_K;
constexpr int kMaxSplits = 64;
constexpr int kCUs = 256;     // the MI355X's compute units: the automatic split count aims at them
constexpr int kPerLane = kMaxSplits * kMaxK / kWave;  // partial pairs per lane of the merge

// splits == 0: from nq and nc alone, two workgroups per compute unit where the sizes allow, a
// segment of at least four 128-candidate steps
static int resolve_splits(int64_t nq, int64_t nc, int splits) {
  if (splits > 0) return splits;
  const int64_t tiles = ceil_div(nq > 0 ? nq : 1, TQ);
  int64_t s = ceil_div(2 * kCUs, tiles);
  const int64_t room = nc / (4 * TC);
  if (s > room) s = room;
  if (s > kMaxSplits) s = kMaxSplits;
  return s < 1 ? 1 : (int)s;
}

// the workspace: feat::PackLayout, then the partial lists [nq][splits][k]: keys fp32, rows int32
struct Layout : PackLayout {
  int S;
  int64_t p_key, p_row, total;
};
static Layout layout(int64_t nq, int64_t nc, int D, int k, int splits) {
  Layout L;
  static_cast<PackLayout&>(L) = pack_layout(nq, nc, D);
  L.S = resolve_splits(nq, nc, splits);
  const int64_t pb = align256(nq * L.S * k * 4);
  L.p_key = L.end;
  L.p_row = L.p_key + pb;
  L.total = L.p_row + pb;
  return L;
}

// One lane's sorted list: Lk ascending, (key, id) lexicographic; an unused slot is (+inf, -1).
// Only finite keys enter, so an entry whose key ties with the newcomer's has a row (>= 0), and
// its id is read from c_id then and only then.
template <int KCAP>
__device__ __forceinline__ void list_insert(float (&Lk)[KCAP], int (&Lr)[KCAP], float key, int row,
                                            int64_t id, const int64_t* __restrict__ c_id) {
  bool lt[KCAP];  // the newcomer sorts before entry i (monotone in i: the list is sorted)
#pragma unroll
  for (int i = 0; i < KCAP; ++i) {
    lt[i] = key < Lk[i];
    if (key == Lk[i]) lt[i] = id < c_id[Lr[i]];
  }
#pragma unroll
  for (int i = KCAP - 1; i >= 0; --i) {
    if (lt[i]) {
      const bool shift = i > 0 && lt[i > 0 ? i - 1 : 0];
      Lk[i] = shift ? Lk[i > 0 ? i - 1 : 0] : key;
      Lr[i] = shift ? Lr[i > 0 ? i - 1 : 0] : row;
    }
  }
}

// feat::scan_keys' epilogue: one lane's list and what deciding on a key needs.  A ragged or
// non-finite candidate has a NaN key: rejected by the first comparison, as is every key above the
// list's worst, and only then is the staged id read.  Only finite keys enter.
template <int KCAP>
struct Offer {
  bool qvalid;
  int64_t my_id;  // the query itself is skipped by id
  const int64_t* __restrict__ c_id;
  const int64_t* s_id;  // the ids scan_keys staged for this step
  float Lk[KCAP];
  int Lr[KCAP];
  __device__ __forceinline__ void operator()(float key, int lr, int64_t c0) {
    if (qvalid && key <= Lk[KCAP - 1] && key < INFINITY) {
      const int64_t id = s_id[lr];
      // a tie with the worst entry: that entry is real (its key is finite), read its id
      if (id != my_id && (key < Lk[KCAP - 1] || id < c_id[Lr[KCAP - 1]]))
        list_insert<KCAP>(Lk, Lr, key, (int)(c0 + lr), id, c_id);
    }
  }
};

// Workgroup b serves query tile b % tiles and candidate segment b / tiles (the workgroups that
// run together share a segment).  Segment s is [s seg, min((s + 1) seg, nc)), seg =
// ceil(nc / S); it may be empty.
// (two workgroups per compute unit: without the bound the lists of 4 and 8 take 196 and 208
// registers and leave room for one)
template <bool F16, int KCAP>
__global__ __launch_bounds__(kThreads, 2) void search_kernel(
    const uint16_t* __restrict__ q_hi, const uint16_t* __restrict__ q_lo,
    const int64_t* __restrict__ q_id, int64_t nq, const uint16_t* __restrict__ c_hi,
    const uint16_t* __restrict__ c_lo, const float* __restrict__ c_norm,
    const int64_t* __restrict__ c_id, int64_t nc, int Dp, int k, int S, int64_t tiles,
    float* __restrict__ p_key, int* __restrict__ p_row) {
  __shared__ ScanLds lds;

  const int64_t b = blockIdx.x;
  const int64_t tile = b % tiles;
  const int seg_i = (int)(b / tiles);
  const int64_t seg = (nc + S - 1) / S;
  const int64_t cs = seg_i * seg < nc ? seg_i * seg : nc;
  const int64_t ce = cs + seg < nc ? cs + seg : nc;
  const int64_t q0 = tile * TQ;

  const int tid = threadIdx.x;
  const int lane = tid % kWave, wave = tid / kWave;
  const int r = lane & 31, h = lane >> 5;
  const int64_t qr = q0 + wave * 32 + r;  // this lane's query (both lane halves hold it)
  const bool qvalid = qr < nq;
  const int64_t my_id = qvalid ? q_id[qr] : -1;
  const uint16_t* __restrict__ qh_row = q_hi + (qvalid ? qr : 0) * (int64_t)Dp;
  const uint16_t* __restrict__ ql_row = q_lo + (qvalid ? qr : 0) * (int64_t)Dp;

  Offer<KCAP> offer = {qvalid, my_id, c_id, lds.id};
  float(&Lk)[KCAP] = offer.Lk;
  int(&Lr)[KCAP] = offer.Lr;
#pragma unroll
  for (int i = 0; i < KCAP; ++i) {
    Lk[i] = INFINITY;
    Lr[i] = -1;
  }
  scan_keys<F16, KCAP <= 8 ? 16 : 8>(lds, qh_row, ql_row, qvalid, c_hi, c_lo, c_norm, c_id, cs, ce,
                                     Dp, offer);
  // the other lane half holds the same query's other candidates: each half inserts the other's
  // entries, so both end with the merged list
  float ok[KCAP];
  int orow[KCAP];
#pragma unroll
  for (int i = 0; i < KCAP; ++i) {
    ok[i] = __shfl_xor(Lk[i], 32, kWave);
    orow[i] = __shfl_xor(Lr[i], 32, kWave);
  }
#pragma unroll
  for (int i = 0; i < KCAP; ++i) {
    if (orow[i] >= 0 && ok[i] <= Lk[KCAP - 1]) {
      const int64_t id = c_id[orow[i]];
      if (ok[i] < Lk[KCAP - 1] || id < c_id[Lr[KCAP - 1]])
        list_insert<KCAP>(Lk, Lr, ok[i], orow[i], id, c_id);
    }
  }
  if (h == 0 && qvalid) {
    const int64_t base = (qr * S + seg_i) * (int64_t)k;
#pragma unroll
    for (int i = 0; i < KCAP; ++i) {
      if (i < k) {
        p_key[base + i] = Lk[i];
        p_row[base + i] = Lr[i];  // -1: fewer than i + 1 admissible candidates in the segment
      }
    }
  }
}

// (key, id, slot) < (bkey, bid, bslot) lexicographically; a NaN key is never smaller
__device__ __forceinline__ bool triple_less(float key, int64_t id, int slot, float bkey,
                                            int64_t bid, int bslot) {
  return key < bkey || (key == bkey && (id < bid || (id == bid && slot < bslot)));
}

// one query per wave64: the k smallest of its S k partial pairs in ascending (key, id) order
__global__ __launch_bounds__(kThreads) void merge_kernel(
    const float* __restrict__ q, const int64_t* __restrict__ q_label, int64_t nq,
    const float* __restrict__ c, const int64_t* __restrict__ c_id,
    const int64_t* __restrict__ c_label, int64_t nc, int D, int k, int S,
    const float* __restrict__ p_key, const int* __restrict__ p_row, float* __restrict__ dist,
    int64_t* __restrict__ nbr_id, float* __restrict__ mean_dist, float* __restrict__ disagree,
    float* __restrict__ accum_dist, float* __restrict__ accum_disagree) {
  const int lane = threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / kWave;
  if (row >= nq) return;  // (a whole wave)
  const float* __restrict__ x = q + row * (int64_t)D;
  const bool bad = wave_row_nonfinite(x, D, lane);

  const int P = S * k;  // <= 64 * 16: at most kPerLane pairs per lane
  float key[kPerLane];
  int64_t id[kPerLane];
  int prow[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int slot = lane + kWave * j;
    key[j] = INFINITY;
    id[j] = kNoId;
    prow[j] = -1;
    if (slot < P) {
      const int pr = p_row[row * (int64_t)P + slot];
      if (pr >= 0 && pr < nc) {
        prow[j] = pr;
        key[j] = p_key[row * (int64_t)P + slot];
        id[j] = c_id[pr];
      }
    }
  }
  const bool labelled = q_label != nullptr && c_label != nullptr;
  const int64_t my_label = labelled ? q_label[row] : 0;
  unsigned taken = 0u;
  double sum = 0.0;  // of the k fp32 distances, in slot order
  int other = 0;
  bool full = true;
  for (int i = 0; i < k; ++i) {
    float bk = INFINITY;
    int64_t bid = kNoId;
    int bslot = INT32_MAX, brow = -1;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const int slot = lane + kWave * j;
      if (prow[j] >= 0 && !((taken >> j) & 1u) && triple_less(key[j], id[j], slot, bk, bid, bslot)) {
        bk = key[j];
        bid = id[j];
        bslot = slot;
        brow = prow[j];
      }
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
      const float ok = __shfl_xor(bk, m, kWave);
      const int64_t oid = shfl_xor64(bid, m);
      const int oslot = __shfl_xor(bslot, m, kWave);
      const int orow = __shfl_xor(brow, m, kWave);
      if (orow >= 0 && (brow < 0 || triple_less(ok, oid, oslot, bk, bid, bslot))) {
        bk = ok;
        bid = oid;
        bslot = oslot;
        brow = orow;
      }
    }
    const bool has = brow >= 0;  // (the same on every lane)
    if (has && (bslot % kWave) == lane) taken |= 1u << (bslot / kWave);
    const float s =
        wave_row_sqdist(x, c + (has ? brow : 0) * (int64_t)D, D, lane, has, nullptr);
    const float dv = bad ? __builtin_nanf("") : (has ? sqrtf(s) : INFINITY);
    if (lane == 0) {
      if (dist) dist[row * (int64_t)k + i] = dv;
      if (nbr_id) nbr_id[row * (int64_t)k + i] = (bad || !has) ? -1 : bid;
    }
    sum += (double)dv;
    if (has && labelled) other += c_label[brow] != my_label ? 1 : 0;
    full = full && has;
  }
  if (lane == 0) {
    const float nanv = __builtin_nanf("");
    const float mean = bad ? nanv : (full ? (float)(sum / (double)k) : INFINITY);
    const float share = (bad || !full) ? nanv : (float)other / (float)k;
    if (mean_dist) mean_dist[row] = mean;
    if (accum_dist) accum_dist[row] += mean;
    if (disagree) disagree[row] = share;
    if (accum_disagree) accum_disagree[row] += share;
  }
}

static bool dims_ok(const char* what, int64_t nq, int64_t nc, int32_t D, int32_t k,
                    int32_t splits, int32_t operands) {
  if (!rows_dims_ok(what, nq, nc, D, operands)) return false;
  if (k < 1 || k > kMaxK) {
    if (what) set_error("%s: need 1 <= k <= %d (k=%d)", what, kMaxK, k);
    return false;
  }
  if (splits < 0 || splits > kMaxSplits) {
    if (what) set_error("%s: need 0 <= splits <= %d (splits=%d)", what, kMaxSplits, splits);
    return false;
  }
  return true;
}

template <bool F16, int KCAP>
static void launch_search(const int64_t* q_id, int64_t nq, const int64_t* c_id, int64_t nc, int k,
                          char* ws, const Layout& L, hipStream_t st) {
  const int64_t tiles = ceil_div(nq, TQ);
  search_kernel<F16, KCAP><<<(unsigned)(tiles * L.S), kThreads, 0, st>>>(
      at<uint16_t>(ws, L.q_hi), at<uint16_t>(ws, L.q_lo), q_id, nq, at<uint16_t>(ws, L.c_hi),
      at<uint16_t>(ws, L.c_lo), at<float>(ws, L.c_norm), c_id, nc, L.Dp, k, L.S, tiles,
      at<float>(ws, L.p_key), at<int>(ws, L.p_row));
}

template <bool F16>
static void launch(const float* q, const int64_t* q_id, int64_t nq, const float* c,
                   const int64_t* c_id, int64_t nc, int D, int k, char* ws, const Layout& L,
                   hipStream_t st) {
  launch_pack<F16>(q, nq, c, nc, D, ws, L, nullptr, st);
  // (with nc == 0 every segment is empty: the search writes lists of unused slots)
  if (k == 1)
    launch_search<F16, 1>(q_id, nq, c_id, nc, k, ws, L, st);
  else if (k <= 4)
    launch_search<F16, 4>(q_id, nq, c_id, nc, k, ws, L, st);
  else if (k <= 8)
    launch_search<F16, 8>(q_id, nq, c_id, nc, k, ws, L, st);
  else
    launch_search<F16, 16>(q_id, nq, c_id, nc, k, ws, L, st);
}

}  // namespace knn
}  // namespace dd

using namespace dd;

extern "C" {

size_t dd_knn_workspace_bytes(int64_t nq, int64_t nc, int32_t D, int32_t k, int32_t splits,
                              int32_t operands) {
  if (!knn::dims_ok(nullptr, nq, nc, D, k, splits, operands)) return 0;
  return (size_t)knn::layout(nq, nc, D, k, splits).total;
}

int dd_knn(const float* q, const int64_t* q_id, const int64_t* q_label, int64_t nq, const float* c,
           const int64_t* c_id, const int64_t* c_label, int64_t nc, int32_t D, int32_t k,
           int32_t splits, int32_t operands, float* dist, int64_t* nbr_id, float* mean_dist,
           float* disagree, float* accum_dist, float* accum_disagree, void* workspace,
           size_t workspace_bytes, void* stream) {
  clear_error();
  if (!knn::dims_ok("dd_knn", nq, nc, D, k, splits, operands)) return DD_EINVAL;
  DD_REQUIRE(dist != nullptr || nbr_id != nullptr || mean_dist != nullptr ||
                 disagree != nullptr || accum_dist != nullptr || accum_disagree != nullptr,
             "dd_knn: no output requested (every output pointer is null)");
  if (nq == 0) return DD_OK;
  DD_REQUIRE(q != nullptr && q_id != nullptr, "dd_knn: null q / q_id");
  DD_REQUIRE(nc == 0 || (c != nullptr && c_id != nullptr), "dd_knn: null c / c_id");
  const bool labels = disagree != nullptr || accum_disagree != nullptr;
  DD_REQUIRE(!labels || (q_label != nullptr && (nc == 0 || c_label != nullptr)),
             "dd_knn: null q_label / c_label with disagree or accum_disagree requested");
  const knn::Layout L = knn::layout(nq, nc, D, k, splits);
  DD_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)L.total,
             "dd_knn: workspace of %zu bytes, need %lld (dd_knn_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, (long long)L.total);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_knn: the workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  if (operands == DD_OPERANDS_F16X3)
    knn::launch<true>(q, q_id, nq, c, c_id, nc, D, k, ws, L, st);
  else
    knn::launch<false>(q, q_id, nq, c, c_id, nc, D, k, ws, L, st);
  knn::merge_kernel<<<(unsigned)ceil_div(nq, knn::kRows), knn::kThreads, 0, st>>>(
      q, labels ? q_label : nullptr, nq, c, c_id, labels ? c_label : nullptr, nc, D, k, L.S,
      feat::at<const float>(ws, L.p_key), feat::at<const int>(ws, L.p_row),
      dist, nbr_id, mean_dist, disagree, accum_dist, accum_disagree);
  DD_CHECK_LAUNCH("dd_knn");
  return DD_OK;
}

}  // extern "C"
