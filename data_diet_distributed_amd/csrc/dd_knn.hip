// The k nearest neighbours of every row over ALL classes in feature space (include/dd_capi.h
// states the semantics):
//   dd_knn_workspace_bytes  bytes of the workspace of one dd_knn call (host only)
//   dd_knn                  per query row: its k nearest other rows, their distances, the mean
//                           distance and the share of neighbours with another label
//
// Three steps on one stream, no allocation, no synchronisation, no atomics:
//   pack    as dd_nn.hip: one wave per row, the row's operand halves (hi, lo; 16-bit, D
//           zero-padded to a multiple of 16) and, for the candidates, ||c||^2 in fp32 (NaN marks a
//           row with a non-finite element).  Every row of the call is split exactly once.
//   search  a 256-thread workgroup owns 128 queries and ONE of `splits` contiguous candidate
//           segments, which it walks 128 candidates at a time with dd_nn.hip's inner loop: the
//           32x32 accumulator has the QUERY on the lane and 16 candidates in the registers.  Each
//           lane keeps a sorted list of its KCAP smallest (key, row) pairs in registers (KCAP =
//           1, 4, 8 or 16, the first one >= k); a candidate is compared with the list's worst key
//           first, which rejects almost every one.  The list holds 32-bit row numbers; the 64-bit
//           id is read only to break a key tie.  The two lane halves are merged at the end and
//           the segment's k smallest pairs go to the workspace.
//   merge   one wave per query: the k smallest of its splits * k partial pairs, one per round
//           (a butterfly minimum of (key, id)), and for each the fp32 distance from the fp32 rows,
//           reduced as dd_proto_scores reduces a row; then the mean, the label comparison and
//           the accumulators.
//
// Invariance: a key is a function of the two rows and D alone (dd_nn.hip), and the k smallest of
// a set of (key, id) pairs under one total order do not depend on how the set is split or
// traversed.  So every output of a row depends on the row, on the candidate SET and on k: not on
// `splits`, the batching of the queries, nq, positions, alignment or the launch geometry.
#include "dd_mfma.h"

#include <math.h>

namespace dd {
namespace knn {

using conv::bf16x8;
using conv::floatx16;

constexpr int kThreads = 256;
constexpr int kMaxD = 4096;   // dd_linear_forward's bound
constexpr int kMaxK = DD_KNN_MAX_K;
constexpr int kMaxSplits = 64;
constexpr int kCUs = 256;     // the MI355X's compute units: the automatic split count aims at them
constexpr int kRows = kThreads / kWave;
constexpr int TQ = 128;                // queries per workgroup (32 per wave)
constexpr int TC = 128;                // candidates per step
constexpr int KC = 64;                 // K elements per LDS chunk
constexpr int kRowBytes = KC * 2 + 16; // LDS row pitch: 16 B of padding against bank conflicts
constexpr int kPerLane = kMaxSplits * kMaxK / kWave;  // partial pairs per lane of the merge
constexpr int64_t kNoId = INT64_MAX;

__host__ __device__ constexpr int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

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

// the workspace: [c hi][c lo][q hi][q lo] 16-bit [rows][Dp], [||c||^2] fp32 [nc], then the
// partial lists [nq][splits][k]: keys fp32, rows int32
struct Layout {
  int Dp, S;
  int64_t c_hi, c_lo, q_hi, q_lo, c_norm, p_key, p_row, total;
};
static Layout layout(int64_t nq, int64_t nc, int D, int k, int splits) {
  Layout L;
  L.Dp = conv::pad_to(D, 16);
  L.S = resolve_splits(nq, nc, splits);
  const int64_t cb = align256(nc * L.Dp * 2), qb = align256(nq * L.Dp * 2);
  const int64_t pb = align256(nq * L.S * k * 4);
  L.c_hi = 0;
  L.c_lo = cb;
  L.q_hi = 2 * cb;
  L.q_lo = 2 * cb + qb;
  L.c_norm = 2 * cb + 2 * qb;
  L.p_key = L.c_norm + align256(nc * 4);
  L.p_row = L.p_key + pb;
  L.total = L.p_row + pb;
  return L;
}

// dd_nn.hip's pack: lane l takes columns l, l + 64, ... in ascending order, then the fixed
// butterfly (the order of the additions of ||x||^2 depends on D alone)
template <bool F16>
__global__ __launch_bounds__(kThreads) void pack_kernel(
    const float* __restrict__ x, int64_t n, int D, int Dp, uint16_t* __restrict__ hi,
    uint16_t* __restrict__ lo, float* __restrict__ norm) {
  const int lane = threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / kWave;
  if (row >= n) return;  // (a whole wave)
  const float* __restrict__ src = x + row * (int64_t)D;
  uint16_t* __restrict__ oh = hi + row * (int64_t)Dp;
  uint16_t* __restrict__ ol = lo + row * (int64_t)Dp;
  float s = 0.f, nf = 0.f;
  for (int d = lane; d < Dp; d += kWave) {
    const float v = d < D ? src[d] : 0.f;
    s = fmaf(v, v, s);
    nf = fabsf(v) < INFINITY ? nf : 1.f;  // NaN or +-inf
    __bf16 h, l;
    conv::split16<F16>(v, h, l);
    oh[d] = __builtin_bit_cast(uint16_t, h);
    ol[d] = __builtin_bit_cast(uint16_t, l);
  }
  s = group_sum<kWave>(s);
  nf = group_max<kWave>(nf);
  if (lane == 0 && norm) norm[row] = nf != 0.f ? __builtin_nanf("") : s;
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
  __shared__ __attribute__((aligned(16))) char s_hi[TC * kRowBytes];
  __shared__ __attribute__((aligned(16))) char s_lo[TC * kRowBytes];
  __shared__ float s_norm[TC];
  __shared__ int64_t s_id[TC];

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

  float Lk[KCAP];
  int Lr[KCAP];
#pragma unroll
  for (int i = 0; i < KCAP; ++i) {
    Lk[i] = INFINITY;
    Lr[i] = -1;
  }

  for (int64_t c0 = cs; c0 < ce; c0 += TC) {
    floatx16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;

    for (int kc = 0; kc < Dp; kc += KC) {
      __syncthreads();  // the previous chunk's reads and the previous step's epilogue are done
      if (kc == 0 && tid < TC) {
        const int64_t j = c0 + tid;
        s_norm[tid] = j < ce ? c_norm[j] : __builtin_nanf("");
        s_id[tid] = j < ce ? c_id[j] : kNoId;
      }
      // TC rows x 8 pieces of 8 halves per operand half: 4 pieces per thread and half
#pragma unroll
      for (int i = 0; i < TC * 8 / kThreads; ++i) {
        const int idx = tid + i * kThreads;
        const int row = idx >> 3, sg = idx & 7;
        const int64_t j = c0 + row;
        const int kk = kc + sg * 8;
        uint4 vh = make_uint4(0u, 0u, 0u, 0u), vl = vh;
        if (j < ce && kk < Dp) {  // ragged rows and the chunk's tail past Dp are zero-filled
          vh = *reinterpret_cast<const uint4*>(c_hi + j * (int64_t)Dp + kk);
          vl = *reinterpret_cast<const uint4*>(c_lo + j * (int64_t)Dp + kk);
        }
        *reinterpret_cast<uint4*>(s_hi + row * kRowBytes + sg * 16) = vh;
        *reinterpret_cast<uint4*>(s_lo + row * kRowBytes + sg * 16) = vl;
      }
      __syncthreads();
      const int steps = (Dp - kc) / 16 < KC / 16 ? (Dp - kc) / 16 : KC / 16;
      for (int s = 0; s < steps; ++s) {
        const int kk = kc + s * 16 + 8 * h;  // B[k = 8 h + j][col r]: 8 consecutive k of query r
        uint4 bh = make_uint4(0u, 0u, 0u, 0u), bl = bh;
        if (qvalid) {
          bh = *reinterpret_cast<const uint4*>(qh_row + kk);
          bl = *reinterpret_cast<const uint4*>(ql_row + kk);
        }
        const bf16x8 fbh = __builtin_bit_cast(bf16x8, bh), fbl = __builtin_bit_cast(bf16x8, bl);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          // A[row r][k = 8 h + j]: 8 consecutive k of candidate 32 a + r
          const int off = (a * 32 + r) * kRowBytes + (s * 16 + 8 * h) * 2;
          const bf16x8 fah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(s_hi + off));
          const bf16x8 fal = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(s_lo + off));
          acc[a] = conv::mfma16<F16>(fah, fbh, acc[a]);
          acc[a] = conv::mfma16<F16>(fah, fbl, acc[a]);
          acc[a] = conv::mfma16<F16>(fal, fbh, acc[a]);
        }
      }
    }
    // accumulator element i of block a: candidate 32 a + (i & 3) + 8 (i >> 2) + 4 h, query r.
    // A ragged or non-finite candidate has a NaN norm, hence a NaN key: rejected by the first
    // comparison, as is every key above the list's worst.  Only finite keys enter.
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int lr = a * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        const float key = fmaf(-2.f, acc[a][i], s_norm[lr]);
        if (qvalid && key <= Lk[KCAP - 1] && key < INFINITY) {
          const int64_t id = s_id[lr];
          // a tie with the worst entry: that entry is real (its key is finite), read its id
          if (id != my_id && (key < Lk[KCAP - 1] || id < c_id[Lr[KCAP - 1]]))
            list_insert<KCAP>(Lk, Lr, key, (int)(c0 + lr), id, c_id);
        }
      }
    }
  }
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

__device__ __forceinline__ int64_t shfl_xor64(int64_t v, int mask) {
  const unsigned hi = (unsigned)__shfl_xor((int)(v >> 32), mask, kWave);
  const unsigned lo = (unsigned)__shfl_xor((int)(v & 0xffffffffll), mask, kWave);
  return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// one query per wave64: the k smallest of its S k partial pairs in ascending (key, id) order,
// each one's distance reduced as dd_proto_scores reduces a row
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
  float nf = 0.f;
  for (int d = lane; d < D; d += kWave) nf = fabsf(x[d]) < INFINITY ? nf : 1.f;  // NaN or +-inf
  const bool bad = group_max<kWave>(nf) != 0.f;

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
    const float* __restrict__ y = c + (has ? brow : 0) * (int64_t)D;
    float s = 0.f;
    for (int d = lane; d < D; d += kWave) {
      const float diff = has ? x[d] - y[d] : 0.f;
      s = fmaf(diff, diff, s);
    }
    s = group_sum<kWave>(s);
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
  if (nq < 0 || nq >= (1ll << 31) || nc < 0 || nc >= (1ll << 31)) {
    set_error("%s: need 0 <= nq, nc < 2^31 (nq=%lld, nc=%lld)", what, (long long)nq,
              (long long)nc);
    return false;
  }
  if (D < 1 || D > kMaxD) {
    set_error("%s: need 1 <= D <= %d (D=%d)", what, kMaxD, D);
    return false;
  }
  if (k < 1 || k > kMaxK) {
    set_error("%s: need 1 <= k <= %d (k=%d)", what, kMaxK, k);
    return false;
  }
  if (splits < 0 || splits > kMaxSplits) {
    set_error("%s: need 0 <= splits <= %d (splits=%d)", what, kMaxSplits, splits);
    return false;
  }
  if (operands != DD_OPERANDS_F16X3 && operands != DD_OPERANDS_BF16X3) {
    set_error("%s: operands must be DD_OPERANDS_BF16X3 or DD_OPERANDS_F16X3 (got %d)", what,
              operands);
    return false;
  }
  return true;
}

template <bool F16, int KCAP>
static void launch_search(const int64_t* q_id, int64_t nq, const int64_t* c_id, int64_t nc, int k,
                          char* ws, const Layout& L, hipStream_t st) {
  const int64_t tiles = ceil_div(nq, TQ);
  search_kernel<F16, KCAP><<<(unsigned)(tiles * L.S), kThreads, 0, st>>>(
      reinterpret_cast<const uint16_t*>(ws + L.q_hi), reinterpret_cast<const uint16_t*>(ws + L.q_lo),
      q_id, nq, reinterpret_cast<const uint16_t*>(ws + L.c_hi),
      reinterpret_cast<const uint16_t*>(ws + L.c_lo), reinterpret_cast<const float*>(ws + L.c_norm),
      c_id, nc, L.Dp, k, L.S, tiles, reinterpret_cast<float*>(ws + L.p_key),
      reinterpret_cast<int*>(ws + L.p_row));
}

template <bool F16>
static void launch(const float* q, const int64_t* q_id, int64_t nq, const float* c,
                   const int64_t* c_id, int64_t nc, int D, int k, char* ws, const Layout& L,
                   hipStream_t st) {
  uint16_t* chi = reinterpret_cast<uint16_t*>(ws + L.c_hi);
  uint16_t* clo = reinterpret_cast<uint16_t*>(ws + L.c_lo);
  uint16_t* qhi = reinterpret_cast<uint16_t*>(ws + L.q_hi);
  uint16_t* qlo = reinterpret_cast<uint16_t*>(ws + L.q_lo);
  if (nc > 0)
    pack_kernel<F16><<<(unsigned)ceil_div(nc, kRows), kThreads, 0, st>>>(
        c, nc, D, L.Dp, chi, clo, reinterpret_cast<float*>(ws + L.c_norm));
  pack_kernel<F16><<<(unsigned)ceil_div(nq, kRows), kThreads, 0, st>>>(q, nq, D, L.Dp, qhi, qlo,
                                                                       nullptr);
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
  if (nq < 0 || nq >= (1ll << 31) || nc < 0 || nc >= (1ll << 31) || D < 1 || D > knn::kMaxD ||
      k < 1 || k > knn::kMaxK || splits < 0 || splits > knn::kMaxSplits ||
      (operands != DD_OPERANDS_F16X3 && operands != DD_OPERANDS_BF16X3))
    return 0;
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
      reinterpret_cast<const float*>(ws + L.p_key), reinterpret_cast<const int*>(ws + L.p_row),
      dist, nbr_id, mean_dist, disagree, accum_dist, accum_disagree);
  DD_CHECK_LAUNCH("dd_knn");
  return DD_OK;
}

}  // extern "C"
