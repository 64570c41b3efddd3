// The kernel density of every row among ALL candidate rows in feature space, and the Parzen
// posterior of its own label (include/dd_capi.h states the semantics):
//   dd_kde_workspace_bytes  bytes of the workspace of one dd_kde call (host only)
//   dd_kde                  per query row: nll = -ln sum_j w_j and post = ln sum_j w_j -
//                           ln sum_{j: same label} w_j,  w_j = exp(-d^2(q, c_j) inv)
//
// Three steps on one stream, no allocation, no synchronisation, no atomics; dd_feat.h defines the
// pack and the key scan:
//   pack   feat::pack_kernel on every row of the call, exactly once; the queries' ||q||^2 too.
//   fold   a 256-thread workgroup owns 128 queries and ONE candidate segment of seg_rows rows,
//          over which it runs feat::scan_keys.  The scan leaves the QUERY on the lane and hands
//          over the keys of a 32x32 accumulator block sixteen at a time; the epilogue is a
//          streaming log-sum-exp in base 2 (the online softmax of attention kernels, on
//          distances): t = -d^2 inv log2(e) <= 0, and the lane keeps (m, sigma) with
//          sum_j 2^t_j = sigma 2^m, once over all candidates and once over those of its label.
//          Per block of sixteen: the block's largest t; where it exceeds m, sigma is rescaled
//          (once) and m raised; then the sixteen 2^(t - m) are added in the accumulator's order.
//          The same-label sum takes the same sixteen exponentials under a label compare while
//          its own maximum equals m (a row whose nearest rows share its label: most rows), and
//          exponentials against its own maximum otherwise, so that rows whose own class is far
//          away (the suspicious ones, which the score exists to rank) do not underflow.  No
//          fixed reference point: an isolated row, every t below -1000, keeps full precision.
//          The two lane halves are then combined, h = 0 first, and the four floats of the
//          (query, segment) pair go to the workspace.
//   merge  one thread per query: M = max m over the segments in ascending order,
//          sum sigma 2^(m - M), the logarithms and the accumulators.
//
// d^2 = max(0, key + ||q||^2), ||q||^2 summed by feat::pack_kernel in dd_feat.h's order.  Where a
// block holds a d^2 below 2^-11 ||q||^2 (the rounding of the key itself: a duplicate or a near
// duplicate) those pairs are measured again from the fp32 rows, sum_d (q[d] - c[d])^2 in one
// ascending fmaf chain, so that an exact duplicate has d^2 = 0 and weight exactly 1, as every
// other feature score gives it distance exactly 0.
//
// The candidate labels of a 128-candidate step go through an LDS array of this unit's own
// (1 KiB beside feat::ScanLds), staged once per step by the epilogue's first call: the scan
// already broadcasts norm and id from LDS per key, a third broadcast read costs an LDS cycle,
// whereas a global load per lr would put 64 more loads per lane and step into the vector memory
// queue that the next step's operand staging waits in.
//
// seg_rows == 0: seg_rows = 128 max(4, ceil(nc / 2048)), a function of nc alone: at most 16
// segments, none shorter than four 128-candidate steps (16 x 391 workgroups at 50 000 x 50 000,
// 16 x 49 for an eighth of the queries: the chip stays filled when the rows are sharded).
//
// Invariance: a key is a function of the two rows and D alone (dd_feat.h); the segmentation
// depends on nc and seg_rows only; within a segment the keys arrive in an order fixed by the
// candidate positions, and every combination above has one order.  So every output of a row
// depends on the row, the candidates IN THEIR ORDER, D, inv and seg_rows: not on nq, the batching
// of the queries, their positions, alignment or the launch geometry.
#include "dd_feat.h"

namespace dd {
namespace kde {

using namespace feat;

constexpr int kMaxSegs = 64;
constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;

static int64_t resolve_seg_rows(int64_t nc, int64_t seg_rows) {
  if (seg_rows > 0) return seg_rows;
  const int64_t steps = ceil_div(nc, 16 * TC);
  return TC * (steps < 4 ? 4 : steps);
}

// the workspace: feat::PackLayout, then ||q||^2 fp32 [nq] and the partial sums float4 [S][nq]
struct Layout : PackLayout {
  int S;
  int64_t seg, q_norm, part, total;
};
static Layout layout(int64_t nq, int64_t nc, int D, int64_t seg_rows) {
  Layout L;
  static_cast<PackLayout&>(L) = pack_layout(nq, nc, D);
  L.seg = resolve_seg_rows(nc, seg_rows);
  const int64_t S = ceil_div(nc, L.seg);
  L.S = S < 1 ? 1 : (int)S;
  L.q_norm = L.end;
  L.part = L.q_norm + align256(nq * 4);
  L.total = L.part + align256(nq * L.S * 16);
  return L;
}

// sigma 2^m of two partial sums, the first operand first; (-inf, 0) is the empty sum
__device__ __forceinline__ void combine(float& m, float& s, float m1, float s1) {
  const float M = fmaxf(m, m1);
  if (M > -INFINITY)
    s = s * __builtin_amdgcn_exp2f(m - M) + s1 * __builtin_amdgcn_exp2f(m1 - M);
  m = M;
}

// feat::scan_keys' epilogue.  A key's place i in its block of sixteen and the block a are the
// bits of lr (lr = 32 a + (i & 3) + 8 (i >> 2) + 4 h), which the unrolled scan makes constants.
// A ragged or non-finite candidate has a NaN key, a non-finite query a NaN norm: t = -inf, the
// empty term, as for the pair with equal ids.
template <bool LABELS>
struct Fold {
  int64_t my_id, my_label;
  float qn, scale;  // ||q||^2; inv log2(e)
  float close_t;    // a block's largest t above this: a d^2 within the key's rounding
  const int64_t* s_id;   // the ids scan_keys staged for this step
  int64_t* s_label;      // this unit's LDS array
  const int64_t* __restrict__ c_label;
  const float* __restrict__ q_row;
  const float* __restrict__ c;
  int64_t ce;
  int D;
  float ma, sa, ms, ss;  // (m, sigma) over all candidates and over those with the query's label
  float t[16];
  unsigned same;

  __device__ __forceinline__ float remeasure(int64_t j) const {
    const float* __restrict__ y = c + j * (int64_t)D;
    float s = 0.f;
    for (int d = 0; d < D; ++d) {
      const float diff = q_row[d] - y[d];
      s = fmaf(diff, diff, s);
    }
    return s;
  }

  __device__ __forceinline__ void operator()(float key, int lr, int64_t c0) {
    const int i = (lr & 3) | ((lr >> 1) & 12);
    if (LABELS && (lr & ~4) == 0) {  // the step's first key
      if (threadIdx.x < TC) {
        const int64_t j = c0 + threadIdx.x;
        s_label[threadIdx.x] = j < ce ? c_label[j] : 0;
      }
      __syncthreads();  // (the previous step's reads ended at scan_keys' barriers)
    }
    if (i == 0) same = 0u;
    const float d2 = key + qn;
    const bool live = d2 < INFINITY && s_id[lr] != my_id;  // (NaN: false)
    t[i] = live ? -fmaxf(d2, 0.f) * scale : -INFINITY;
    if (LABELS) same |= (live && s_label[lr] == my_label ? 1u : 0u) << i;
    if (i != 15) return;

    float bm = t[0];
#pragma unroll
    for (int u = 1; u < 16; ++u) bm = fmaxf(bm, t[u]);
    if (bm > close_t) {  // (rare: one rolled loop, the registers stay the common path's)
      const int lr0 = lr & ~27;  // the block's first key: 32 a + 4 h
      unsigned todo = 0u;
#pragma unroll
      for (int u = 0; u < 16; ++u) todo |= (t[u] > close_t ? 1u : 0u) << u;
#pragma unroll 1
      while (todo != 0u) {
        const int u = __builtin_ctz(todo);
        todo &= todo - 1u;
        const float v = -remeasure(c0 + lr0 + (u & 3) + 8 * (u >> 2)) * scale;
#pragma unroll
        for (int w = 0; w < 16; ++w) t[w] = w == u ? v : t[w];
      }
      bm = t[0];
#pragma unroll
      for (int u = 1; u < 16; ++u) bm = fmaxf(bm, t[u]);
    }
    if (bm > ma) {
      sa *= __builtin_amdgcn_exp2f(ma - bm);
      ma = bm;
    }
    if (!(ma > -INFINITY)) return;  // nothing yet
    float e[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      e[u] = __builtin_amdgcn_exp2f(t[u] - ma);
      sa += e[u];
    }
    if (LABELS && same != 0u) {
      float bs = -INFINITY;
#pragma unroll
      for (int u = 0; u < 16; ++u) bs = fmaxf(bs, (same >> u) & 1u ? t[u] : -INFINITY);
      if (bs > ms) {
        ss *= __builtin_amdgcn_exp2f(ms - bs);
        ms = bs;
      }
      if (ms == ma) {
#pragma unroll
        for (int u = 0; u < 16; ++u) ss += (same >> u) & 1u ? e[u] : 0.f;
      } else {
#pragma unroll
        for (int u = 0; u < 16; ++u)
          ss += (same >> u) & 1u ? __builtin_amdgcn_exp2f(t[u] - ms) : 0.f;
      }
    }
  }
};

// Workgroup b serves query tile b % tiles and candidate segment b / tiles (the workgroups that
// run together share a segment).  Segment s is [s seg, min((s + 1) seg, nc)).
template <bool F16, bool LABELS>
__global__ __launch_bounds__(kThreads, 2) void fold_kernel(
    const float* __restrict__ q, const uint16_t* __restrict__ q_hi,
    const uint16_t* __restrict__ q_lo, const float* __restrict__ q_norm,
    const int64_t* __restrict__ q_id, const int64_t* __restrict__ q_label, int64_t nq,
    const float* __restrict__ c, const uint16_t* __restrict__ c_hi,
    const uint16_t* __restrict__ c_lo, const float* __restrict__ c_norm,
    const int64_t* __restrict__ c_id, const int64_t* __restrict__ c_label, int64_t nc, int D,
    int Dp, int64_t seg, int64_t tiles, float scale, float4* __restrict__ part) {
  __shared__ ScanLds lds;
  __shared__ int64_t s_label[TC];

  const int64_t b = blockIdx.x;
  const int64_t tile = b % tiles;
  const int64_t seg_i = b / tiles;
  const int64_t cs = seg_i * seg < nc ? seg_i * seg : nc;
  const int64_t ce = cs + seg < nc ? cs + seg : nc;

  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int r = lane & 31, h = lane >> 5;
  const int64_t qr = tile * TQ + wave * 32 + r;  // this lane's query (both lane halves hold it)
  const bool qvalid = qr < nq;
  const int64_t row = qvalid ? qr : 0;

  Fold<LABELS> fold;
  fold.my_id = qvalid ? q_id[qr] : -1;
  fold.my_label = LABELS ? q_label[row] : 0;
  fold.qn = qvalid ? q_norm[qr] : __builtin_nanf("");
  fold.scale = scale;
  fold.close_t = -0x1p-11f * fold.qn * scale;
  fold.s_id = lds.id;
  fold.s_label = s_label;
  fold.c_label = c_label;
  fold.q_row = q + row * (int64_t)D;
  fold.c = c;
  fold.ce = ce;
  fold.D = D;
  fold.ma = fold.ms = -INFINITY;
  fold.sa = fold.ss = 0.f;
  fold.same = 0u;
  scan_keys<F16, 16>(lds, q_hi + row * (int64_t)Dp, q_lo + row * (int64_t)Dp, qvalid, c_hi, c_lo,
                     c_norm, c_id, cs, ce, Dp, fold);
  // the other lane half holds the same query's other candidates: h = 0 first
  float ma = fold.ma, sa = fold.sa, ms = fold.ms, ss = fold.ss;
  const float oma = __shfl_xor(ma, 32, kWave), osa = __shfl_xor(sa, 32, kWave);
  const float oms = __shfl_xor(ms, 32, kWave), oss = __shfl_xor(ss, 32, kWave);
  if (h == 0 && qvalid) {
    combine(ma, sa, oma, osa);
    combine(ms, ss, oms, oss);
    part[seg_i * nq + qr] = make_float4(ma, sa, ms, ss);
  }
}

// one query per thread: the segments' partial sums in ascending order
__global__ __launch_bounds__(kThreads) void merge_kernel(
    const float4* __restrict__ part, const float* __restrict__ q_norm, int64_t nq, int S,
    float* __restrict__ nll, float* __restrict__ post, float* __restrict__ accum_nll,
    float* __restrict__ accum_post) {
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (row >= nq) return;
  float Ma = -INFINITY, Ms = -INFINITY;
  for (int s = 0; s < S; ++s) {
    const float4 p = part[s * nq + row];
    Ma = fmaxf(Ma, p.x);
    Ms = fmaxf(Ms, p.z);
  }
  float sa = 0.f, ss = 0.f;
  for (int s = 0; s < S; ++s) {
    const float4 p = part[s * nq + row];
    if (p.x > -INFINITY) sa += p.y * __builtin_amdgcn_exp2f(p.x - Ma);
    if (p.z > -INFINITY) ss += p.w * __builtin_amdgcn_exp2f(p.z - Ms);
  }
  const bool bad = !(q_norm[row] < INFINITY);  // a non-finite query row
  const float nanv = __builtin_nanf("");
  // log2 of the two sums (-inf: no candidate)
  const float la = sa > 0.f ? Ma + __builtin_amdgcn_logf(sa) : -INFINITY;
  const float ls = ss > 0.f ? Ms + __builtin_amdgcn_logf(ss) : -INFINITY;
  const float v_nll = bad ? nanv : -la * kLn2;
  const float v_post = bad ? nanv : (ls > -INFINITY ? (la - ls) * kLn2 : INFINITY);
  if (nll) nll[row] = v_nll;
  if (accum_nll) accum_nll[row] += v_nll;
  if (post) post[row] = v_post;
  if (accum_post) accum_post[row] += v_post;
}

static bool dims_ok(const char* what, int64_t nq, int64_t nc, int32_t D, int64_t seg_rows,
                    int32_t operands) {
  if (!rows_dims_ok(what, nq, nc, D, operands)) return false;
  if (seg_rows < 0 || seg_rows % TC != 0 || seg_rows >= (1ll << 31)) {
    if (what)
      set_error("%s: seg_rows must be 0 or a multiple of %d below 2^31 (seg_rows=%lld)", what, TC,
                (long long)seg_rows);
    return false;
  }
  if (seg_rows > 0 && ceil_div(nc, seg_rows) > kMaxSegs) {
    if (what)
      set_error("%s: at most %d candidate segments (nc=%lld, seg_rows=%lld)", what, kMaxSegs,
                (long long)nc, (long long)seg_rows);
    return false;
  }
  return true;
}

template <bool F16, bool LABELS>
static void launch(const float* q, const int64_t* q_id, const int64_t* q_label, int64_t nq,
                   const float* c, const int64_t* c_id, const int64_t* c_label, int64_t nc, int D,
                   float scale, char* ws, const Layout& L, hipStream_t st) {
  // every row of the call is split exactly once: the candidates, then the queries, both with
  // their norms
  if (nc > 0)
    pack_kernel<F16><<<(unsigned)ceil_div(nc, kRows), kThreads, 0, st>>>(
        c, nc, D, L.Dp, at<uint16_t>(ws, L.c_hi), at<uint16_t>(ws, L.c_lo),
        at<float>(ws, L.c_norm), nullptr);
  pack_kernel<F16><<<(unsigned)ceil_div(nq, kRows), kThreads, 0, st>>>(
      q, nq, D, L.Dp, at<uint16_t>(ws, L.q_hi), at<uint16_t>(ws, L.q_lo),
      at<float>(ws, L.q_norm), nullptr);
  // (with nc == 0 the one segment is empty: the fold writes empty sums)
  const int64_t tiles = ceil_div(nq, TQ);
  fold_kernel<F16, LABELS><<<(unsigned)(tiles * L.S), kThreads, 0, st>>>(
      q, at<uint16_t>(ws, L.q_hi), at<uint16_t>(ws, L.q_lo), at<float>(ws, L.q_norm), q_id,
      q_label, nq, c, at<uint16_t>(ws, L.c_hi), at<uint16_t>(ws, L.c_lo),
      at<float>(ws, L.c_norm), c_id, c_label, nc, D, L.Dp, L.seg, tiles, scale,
      at<float4>(ws, L.part));
}

}  // namespace kde
}  // namespace dd

using namespace dd;

extern "C" {

size_t dd_kde_workspace_bytes(int64_t nq, int64_t nc, int32_t D, int64_t seg_rows,
                              int32_t operands) {
  if (!kde::dims_ok(nullptr, nq, nc, D, seg_rows, operands)) return 0;
  return (size_t)kde::layout(nq, nc, D, seg_rows).total;
}

int dd_kde(const float* q, const int64_t* q_id, const int64_t* q_label, int64_t nq, const float* c,
           const int64_t* c_id, const int64_t* c_label, int64_t nc, int32_t D, float inv,
           int64_t seg_rows, int32_t operands, float* nll, float* post, float* accum_nll,
           float* accum_post, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  if (!kde::dims_ok("dd_kde", nq, nc, D, seg_rows, operands)) return DD_EINVAL;
  DD_REQUIRE(inv > 0.f && inv < INFINITY, "dd_kde: inv must be finite and > 0 (inv=%g)",
             (double)inv);
  DD_REQUIRE(nll != nullptr || post != nullptr || accum_nll != nullptr || accum_post != nullptr,
             "dd_kde: no output requested (every output pointer is null)");
  if (nq == 0) return DD_OK;
  DD_REQUIRE(q != nullptr && q_id != nullptr, "dd_kde: null q / q_id");
  DD_REQUIRE(nc == 0 || (c != nullptr && c_id != nullptr), "dd_kde: null c / c_id");
  const bool labels = post != nullptr || accum_post != nullptr;
  DD_REQUIRE(!labels || (q_label != nullptr && (nc == 0 || c_label != nullptr)),
             "dd_kde: null q_label / c_label with post or accum_post requested");
  const kde::Layout L = kde::layout(nq, nc, D, seg_rows);
  DD_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)L.total,
             "dd_kde: workspace of %zu bytes, need %lld (dd_kde_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, (long long)L.total);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_kde: the workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  const float scale = inv * kde::kLog2e;
  const bool f16 = operands == DD_OPERANDS_F16X3;
  auto go = f16 ? (labels ? kde::launch<true, true> : kde::launch<true, false>)
                : (labels ? kde::launch<false, true> : kde::launch<false, false>);
  go(q, q_id, q_label, nq, c, c_id, c_label, nc, D, scale, ws, L, st);
  kde::merge_kernel<<<(unsigned)ceil_div(nq, kde::kThreads), kde::kThreads, 0, st>>>(
      feat::at<const float4>(ws, L.part), feat::at<const float>(ws, L.q_norm), nq, L.S, nll,
      labels ? post : nullptr, accum_nll, labels ? accum_post : nullptr);
  DD_CHECK_LAUNCH("dd_kde");
  return DD_OK;
}

}  // extern "C"
