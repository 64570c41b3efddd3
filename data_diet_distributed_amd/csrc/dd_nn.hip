// Distance to the nearest neighbour of the same class in feature space (include/dd_capi.h
// states the semantics):
//   dd_nn_workspace_bytes  bytes of the workspace of one dd_nn_same_class call (host only)
//   dd_nn_same_class       per query row: the nearest other row of its class and its distance
//
// Three steps on one stream, no allocation, no synchronisation, no atomics:
//   pack    one wave per row: the row's operand halves (hi, lo; 16-bit, D zero-padded to a
//           multiple of 16) and, for the candidates, ||c||^2 in fp32 (NaN marks a row with a
//           non-finite element: its keys are NaN and a NaN key never wins).  Every row of the
//           call is split exactly once.
//   search  a 256-thread workgroup owns 128 queries of ONE class and walks that class's
//           candidates 128 at a time.  The candidate halves of a 64-wide K chunk go through
//           LDS (shared by the four waves); wave w owns queries 32 w .. 32 w + 31 and reads
//           their halves as the B operand, the candidates are the A operand, so the 32x32
//           accumulator has the QUERY on the lane and 16 candidates in the registers: the
//           running minimum of (key, id) is per lane, and only the two lane halves are
//           combined at the end.  key = ||c||^2 - 2 q.c with q.c = hi.hi + hi.lo + lo.hi.
//   value   one wave per query: sqrt(sum (q - c[pick])^2) in fp32 from the fp32 rows, reduced
//           as dd_proto_scores reduces a row.  The MFMA rounding decides which row is picked,
//           never the value: an exact duplicate scores exactly 0.
//
// Invariance: a key is a function of the two rows and D alone (the K order is fixed by D, a
// 32x32x16 MFMA computes every output element from its own row and column only, zero-filled
// ragged rows change nothing), and the minimum of (key, id) pairs under one total order does
// not depend on the order in which the pairs are met.  So the pick depends on the query row and
// on the candidate SET of its class, not on the batching of the queries, on nq, on positions or
// on the launch geometry.
#include "dd_mfma.h"

#include <math.h>

namespace dd {
namespace nn {

using conv::bf16x8;
using conv::floatx16;

constexpr int kThreads = 256;
constexpr int kMaxD = 4096;            // dd_linear_forward's bound
constexpr int64_t kMaxC = 1ll << 20;   // dd_select_topk_by_class's bound
constexpr int kRows = kThreads / kWave;
constexpr int TQ = 128;                // queries per workgroup (32 per wave)
constexpr int TC = 128;                // candidates per step
constexpr int KC = 64;                 // K elements per LDS chunk
constexpr int kRowBytes = KC * 2 + 16; // LDS row pitch: 16 B of padding against bank conflicts
constexpr int64_t kNoId = INT64_MAX;

__host__ __device__ constexpr int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// the workspace: [c hi][c lo][q hi][q lo] 16-bit [rows][Dp], [||c||^2] fp32, [pick] int32
struct Layout {
  int Dp;
  int64_t c_hi, c_lo, q_hi, q_lo, c_norm, pick, total;
};
static Layout layout(int64_t nq, int64_t nc, int D) {
  Layout L;
  L.Dp = conv::pad_to(D, 16);
  const int64_t cb = align256(nc * L.Dp * 2), qb = align256(nq * L.Dp * 2);
  L.c_hi = 0;
  L.c_lo = cb;
  L.q_hi = 2 * cb;
  L.q_lo = 2 * cb + qb;
  L.c_norm = 2 * cb + 2 * qb;
  L.pick = L.c_norm + align256(nc * 4);
  L.total = L.pick + align256(nq * 4);
  return L;
}

// one row per wave: lane l takes columns l, l + 64, ... in ascending order, then the fixed
// butterfly (the order of the additions of ||x||^2 depends on D alone)
template <bool F16>
__global__ __launch_bounds__(kThreads) void pack_kernel(
    const float* __restrict__ x, int64_t n, int D, int Dp, uint16_t* __restrict__ hi,
    uint16_t* __restrict__ lo, float* __restrict__ norm, int* __restrict__ pick) {
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
  if (lane == 0) {
    if (norm) norm[row] = nf != 0.f ? __builtin_nanf("") : s;
    if (pick) pick[row] = -1;  // rows outside every segment keep it
  }
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// (key, id) < (bkey, bid) lexicographically; a NaN key is never smaller
__device__ __forceinline__ bool pair_less(float key, int64_t id, float bkey, int64_t bid) {
  return key < bkey || (key == bkey && id < bid);
}

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
  __shared__ __attribute__((aligned(16))) char s_hi[TC * kRowBytes];
  __shared__ __attribute__((aligned(16))) char s_lo[TC * kRowBytes];
  __shared__ float s_norm[TC];
  __shared__ int64_t s_id[TC];

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

  float best = INFINITY;
  int64_t best_id = kNoId;
  int best_row = -1;

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
        const int row = idx >> 3, seg = idx & 7;
        const int64_t j = c0 + row;
        const int kk = kc + seg * 8;
        uint4 vh = make_uint4(0u, 0u, 0u, 0u), vl = vh;
        if (j < ce && kk < Dp) {  // ragged rows and the chunk's tail past Dp are zero-filled
          vh = *reinterpret_cast<const uint4*>(c_hi + j * (int64_t)Dp + kk);
          vl = *reinterpret_cast<const uint4*>(c_lo + j * (int64_t)Dp + kk);
        }
        *reinterpret_cast<uint4*>(s_hi + row * kRowBytes + seg * 16) = vh;
        *reinterpret_cast<uint4*>(s_lo + row * kRowBytes + seg * 16) = vl;
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
    // A ragged candidate has a NaN norm (never smaller); the query itself is skipped by id.
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int lr = a * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        const float key = fmaf(-2.f, acc[a][i], s_norm[lr]);
        const int64_t id = s_id[lr];
        if (id != my_id && pair_less(key, id, best, best_id)) {
          best = key;
          best_id = id;
          best_row = (int)(c0 + lr);
        }
      }
    }
  }
  // the other lane half holds the same query's other candidates
  const float o_key = __shfl_xor(best, 32, kWave);
  const int o_row = __shfl_xor(best_row, 32, kWave);
  const int64_t o_id = (int64_t)(((unsigned long long)(unsigned)__shfl_xor((int)(best_id >> 32), 32, kWave) << 32) |
                                 (unsigned)__shfl_xor((int)(best_id & 0xffffffffll), 32, kWave));
  if (pair_less(o_key, o_id, best, best_id)) {
    best_id = o_id;
    best_row = o_row;
  }
  if (h == 0 && qvalid) pick[qr] = best_row;  // -1: no admissible candidate
}

// one query per wave64, reduced as dd_proto_scores reduces a row
__global__ __launch_bounds__(kThreads) void value_kernel(
    const float* __restrict__ q, int64_t nq, const float* __restrict__ c,
    const int64_t* __restrict__ c_id, int64_t nc, int D, const int* __restrict__ pick,
    float* __restrict__ dist, int64_t* __restrict__ nn_id, float* __restrict__ accum) {
  const int lane = threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / kWave;
  if (row >= nq) return;  // (a whole wave)
  const int p = pick[row];
  const bool has = p >= 0 && p < nc;
  const float* __restrict__ x = q + row * (int64_t)D;
  const float* __restrict__ y = c + (has ? p : 0) * (int64_t)D;
  float s = 0.f, nf = 0.f;
  for (int d = lane; d < D; d += kWave) {
    const float v = x[d];
    const float diff = has ? v - y[d] : 0.f;
    s = fmaf(diff, diff, s);
    nf = fabsf(v) < INFINITY ? nf : 1.f;  // NaN or +-inf
  }
  s = group_sum<kWave>(s);
  nf = group_max<kWave>(nf);
  if (lane == 0) {
    const bool bad = nf != 0.f;
    const float d = bad ? __builtin_nanf("") : (has ? sqrtf(s) : INFINITY);
    if (dist) dist[row] = d;
    if (nn_id) nn_id[row] = (bad || !has) ? -1 : c_id[p];
    if (accum) accum[row] += d;
  }
}

static bool dims_ok(const char* what, int64_t nq, int64_t nc, int32_t D, int64_t C,
                    int32_t operands) {
  if (nq < 0 || nq >= (1ll << 31) || nc < 0 || nc >= (1ll << 31)) {
    set_error("%s: need 0 <= nq, nc < 2^31 (nq=%lld, nc=%lld)", what, (long long)nq,
              (long long)nc);
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
  if (operands != DD_OPERANDS_F16X3 && operands != DD_OPERANDS_BF16X3) {
    set_error("%s: operands must be DD_OPERANDS_BF16X3 or DD_OPERANDS_F16X3 (got %d)", what,
              operands);
    return false;
  }
  return true;
}

template <bool F16>
static void launch(const float* q, const int64_t* q_id, const int64_t* q_off, int64_t nq,
                   const float* c, const int64_t* c_id, const int64_t* c_off, int64_t nc,
                   int64_t C, int D, char* ws, const Layout& L, hipStream_t st) {
  uint16_t* chi = reinterpret_cast<uint16_t*>(ws + L.c_hi);
  uint16_t* clo = reinterpret_cast<uint16_t*>(ws + L.c_lo);
  uint16_t* qhi = reinterpret_cast<uint16_t*>(ws + L.q_hi);
  uint16_t* qlo = reinterpret_cast<uint16_t*>(ws + L.q_lo);
  float* cnorm = reinterpret_cast<float*>(ws + L.c_norm);
  int* pick = reinterpret_cast<int*>(ws + L.pick);
  if (nc > 0)
    pack_kernel<F16><<<(unsigned)ceil_div(nc, kRows), kThreads, 0, st>>>(c, nc, D, L.Dp, chi,
                                                                         clo, cnorm, nullptr);
  pack_kernel<F16><<<(unsigned)ceil_div(nq, kRows), kThreads, 0, st>>>(q, nq, D, L.Dp, qhi, qlo,
                                                                       nullptr, pick);
  if (nc > 0)
    search_kernel<F16><<<(unsigned)(nq / TQ + C), kThreads, 0, st>>>(
        qhi, qlo, q_id, q_off, nq, chi, clo, cnorm, c_id, c_off, nc, C, L.Dp, pick);
}

}  // namespace nn
}  // namespace dd

using namespace dd;

extern "C" {

size_t dd_nn_workspace_bytes(int64_t nq, int64_t nc, int32_t D, int32_t operands) {
  if (nq < 0 || nq >= (1ll << 31) || nc < 0 || nc >= (1ll << 31) || D < 1 || D > nn::kMaxD ||
      (operands != DD_OPERANDS_F16X3 && operands != DD_OPERANDS_BF16X3))
    return 0;
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
      q, nq, c, c_id, nc, D, reinterpret_cast<const int*>(ws + L.pick), dist, nn_id, accum);
  DD_CHECK_LAUNCH("dd_nn_same_class");
  return DD_OK;
}

}  // extern "C"
