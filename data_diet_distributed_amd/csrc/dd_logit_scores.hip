// The logit-score family beside EL2N: cross-entropy loss, logit margin, predictive entropy,
// misclassification, wrong-class probability mass and its Welford (mean, M2) pair, all from one
// read of the logits (include/dd_capi.h states the formulas and the NaN rules).
//
// HBM/latency-bound row kernels on dd_el2n's row families: narrow rows staged through LDS with
// several rows per wave64, mid-width rows at 64 lanes per row, very wide rows at one block per
// row.  A row's sums are reduced in an order fixed by C alone (which lane holds which class, then
// a fixed butterfly), so its results are bitwise independent of B, of the row's position and of
// the buffers' alignment.  No float atomics; every statistic is computed whatever subset is asked
// for, and only the requested ones are stored.
#include "dd_common.h"

#include <math.h>

namespace dd {

// where the requested statistics go (NULL: not requested)
struct LogitOut {
  float* loss;
  float* margin;
  float* entropy;
  float* error;
  float* wrong_mass;
  float* var_mean;
  float* var_m2;
  int k;  // 1-based checkpoint ordinal of the Welford update
  int* bad_labels;
};

// what a row reduces to: max, sum of e_j = exp(z_j - m), the same sum without the label, the
// entropy numerator sum e_j (z_j - m), the label's logit, the largest other logit
struct RowSums {
  float m, s, so, t, zy, mo;
};

// one lane's share of a row, second pass: element j with logit v, row max m
__device__ __forceinline__ void row_term(RowSums& r, float v, int j, int64_t y) {
  const float d = v - r.m;
  const float ev = expf(d);
  r.s += ev;
  r.t += ev > 0.f ? ev * d : 0.f;  // a term with e_j == 0 contributes 0 (not 0 * -inf)
  if (j == y) {
    r.zy = v;
  } else {
    r.so += ev;
    r.mo = fmaxf(r.mo, v);
  }
}

// the row's statistics from its reduced sums, by the one lane that owns the row.
// invalid: a label outside [0, C), or a NaN / +inf logit (fmaxf drops NaN, and m = +inf makes
// the margin -inf rather than NaN: both are turned into NaN here, for every statistic)
__device__ __forceinline__ void row_store(const LogitOut& o, int64_t row, bool bad_label,
                                          bool nonfinite, const RowSums& r) {
  const float nan = __builtin_nanf("");
  const bool invalid = bad_label || nonfinite;
  const float ls = logf(r.s);
  if (o.loss) o.loss[row] += invalid ? nan : (r.m - r.zy) + ls;
  if (o.margin) o.margin[row] += invalid ? nan : r.mo - r.zy;
  if (o.entropy) o.entropy[row] += invalid ? nan : ls - r.t / r.s;
  if (o.error) o.error[row] += invalid ? nan : (r.mo >= r.zy ? 1.f : 0.f);
  const float w = invalid ? nan : r.so / r.s;
  if (o.wrong_mass) o.wrong_mass[row] += w;
  if (o.var_mean) {
    // Welford, checkpoint order 1..K (a sum and a sum of squares would cancel)
    if (o.k == 1) {
      o.var_mean[row] = w;
      o.var_m2[row] = invalid ? nan : 0.f;
    } else {
      const float mean = o.var_mean[row];
      const float d = w - mean;
      const float mean_k = mean + d / (float)o.k;
      o.var_mean[row] = mean_k;
      o.var_m2[row] += d * (w - mean_k);
    }
  }
  if (bad_label && o.bad_labels) atomicAdd(o.bad_labels, 1);
}

// NaN or +inf (-inf pads the lanes past C)
__device__ __forceinline__ float nonfinite_flag(float v) { return v < INFINITY ? 0.f : 1.f; }

// ------------------------------------------------------------------------------------------
// Mid-width rows (128 < C <= 2048): LPR lanes per row, each lane keeps EPL logits in registers
// ------------------------------------------------------------------------------------------
template <int LPR, int EPL>
__global__ __launch_bounds__(256) void logit_rows_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ labels,
                                                         int64_t B, int C, LogitOut o) {
  constexpr int ROWS = 256 / LPR;
  const int lane = threadIdx.x % LPR;
  const int64_t row = (int64_t)blockIdx.x * ROWS + threadIdx.x / LPR;
  const bool live = row < B;  // keep every lane in the shuffles
  const float* x = logits + (live ? row : 0) * (int64_t)C;

  float v[EPL];
  float m = -INFINITY, nf = 0.f;
#pragma unroll
  for (int i = 0; i < EPL; ++i) {
    const int j = lane + i * LPR;
    v[i] = (live && j < C) ? x[j] : -INFINITY;
    m = fmaxf(m, v[i]);
    nf = (j < C) ? fmaxf(nf, nonfinite_flag(v[i])) : nf;
  }
  m = group_max<LPR>(m);
  nf = group_max<LPR>(nf);
  const int64_t y = live ? labels[row] : -1;
  RowSums r{m, 0.f, 0.f, 0.f, -INFINITY, -INFINITY};
#pragma unroll
  for (int i = 0; i < EPL; ++i) {
    const int j = lane + i * LPR;
    if (j < C) row_term(r, v[i], j, y);
  }
  r.s = group_sum<LPR>(r.s);
  r.so = group_sum<LPR>(r.so);
  r.t = group_sum<LPR>(r.t);
  r.zy = group_max<LPR>(r.zy);
  r.mo = group_max<LPR>(r.mo);
  if (live && lane == 0) row_store(o, row, y < 0 || y >= C, nf != 0.f, r);
}

// ------------------------------------------------------------------------------------------
// Very wide rows (C > 2048): one 256-thread block per row, logits re-read from cache
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void logit_wide_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ labels,
                                                         int64_t B, int C, LogitOut o) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const float* x = logits + row * (int64_t)C;
  const int t = threadIdx.x, w = t / kWave, l = t % kWave;
  auto block_reduce = [&](float v, bool is_max) -> float {
    v = is_max ? group_max<kWave>(v) : group_sum<kWave>(v);
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float q = red[0];
    for (int i = 1; i < 4; ++i) q = is_max ? fmaxf(q, red[i]) : q + red[i];
    return q;
  };
  float m = -INFINITY, nf = 0.f;
  for (int j = t; j < C; j += 256) {
    const float v = x[j];
    m = fmaxf(m, v);
    nf = fmaxf(nf, nonfinite_flag(v));
  }
  m = block_reduce(m, true);
  nf = block_reduce(nf, true);
  const int64_t y = labels[row];
  RowSums r{m, 0.f, 0.f, 0.f, -INFINITY, -INFINITY};
  for (int j = t; j < C; j += 256) row_term(r, x[j], j, y);
  r.s = block_reduce(r.s, false);
  r.so = block_reduce(r.so, false);
  r.t = block_reduce(r.t, false);
  r.zy = block_reduce(r.zy, true);
  r.mo = block_reduce(r.mo, true);
  if (t == 0) row_store(o, row, y < 0 || y >= C, nf != 0.f, r);
}

// ------------------------------------------------------------------------------------------
// Narrow rows (C <= 128), dd_el2n's layout: a one-wave block owns R = 64 / LPR consecutive
// rows, one contiguous span of logits, streamed into LDS with 16-byte loads where the span
// starts 16-byte aligned (scalar loads otherwise: the same values, the same arithmetic) and
// scattered to rows of odd stride CP = C | 1; then LPR lanes reduce a row from LDS in
// registers (lane part p takes classes p, p + LPR, ...).
// ------------------------------------------------------------------------------------------
template <int EPL, int LPR>
__global__ __launch_bounds__(64) void logit_lds_kernel(const float* __restrict__ logits,
                                                       const int64_t* __restrict__ labels,
                                                       int64_t B, int C, uint32_t cmag,
                                                       LogitOut o, int vec) {
  constexpr int R = 64 / LPR;
  extern __shared__ __attribute__((aligned(16))) float sl[];  // R rows x CP floats
  const int tid = threadIdx.x, CP = C | 1;
  const int lr = tid / LPR, part = tid % LPR;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int rows = (int)(B - row0 < R ? B - row0 : R);
  const int cnt = rows * C;
  // flat index i of the span -> LDS slot (i / C) * CP + i % C; i < 64 * 128, so the
  // multiply-high by cmag = ceil(2^32 / C) is exact (cmag = 0: C = 1)
  auto slot = [&](uint32_t i) {
    const uint32_t q = cmag ? __umulhi(i, cmag) : i;
    return q * CP + (i - q * C);
  };
  const float* __restrict__ src = logits + row0 * C;
  int tail = 0;
  if (vec) {
    const int n4 = cnt >> 2;
    for (int i = tid; i < n4; i += 64) {
      const float4 q = reinterpret_cast<const float4*>(src)[i];
      sl[slot(4 * i)] = q.x;
      sl[slot(4 * i + 1)] = q.y;
      sl[slot(4 * i + 2)] = q.z;
      sl[slot(4 * i + 3)] = q.w;
    }
    tail = n4 << 2;
  }
  for (int i = tail + tid; i < cnt; i += 64) sl[slot(i)] = src[i];
  const bool live = lr < rows;
  const int64_t y = live ? labels[row0 + lr] : -1;
  __syncthreads();
  const float* row = sl + lr * CP;  // rows >= `rows` read stale LDS: their results are dropped
  float v[EPL];
  float m = -INFINITY, nf = 0.f;
#pragma unroll
  for (int i = 0; i < EPL; ++i) {
    const int j = part + LPR * i;
    v[i] = j < C ? row[j] : -INFINITY;
    m = fmaxf(m, v[i]);
    nf = (j < C) ? fmaxf(nf, nonfinite_flag(v[i])) : nf;
  }
  m = group_max<LPR>(m);
  nf = group_max<LPR>(nf);
  RowSums r{m, 0.f, 0.f, 0.f, -INFINITY, -INFINITY};
#pragma unroll
  for (int i = 0; i < EPL; ++i) {
    const int j = part + LPR * i;
    if (j < C) row_term(r, v[i], j, y);
  }
  r.s = group_sum<LPR>(r.s);
  r.so = group_sum<LPR>(r.so);
  r.t = group_sum<LPR>(r.t);
  r.zy = group_max<LPR>(r.zy);
  r.mo = group_max<LPR>(r.mo);
  if (live && part == 0) row_store(o, row0 + lr, y < 0 || y >= C, nf != 0.f, r);
}

template <int EPL, int LPR>
static void launch_logit_lds(const float* logits, const int64_t* labels, int64_t B, int C,
                             const LogitOut& o, hipStream_t st) {
  constexpr int R = 64 / LPR;
  // 16-B staging: block spans start at R C floats from the base
  const int vec = ((uintptr_t)logits % 16 == 0) && (R * C) % 4 == 0;
  const uint32_t cmag = C == 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + C - 1) / C);
  logit_lds_kernel<EPL, LPR><<<(unsigned)ceil_div(B, R), 64, (size_t)R * (C | 1) * 4, st>>>(
      logits, labels, B, C, cmag, o, vec);
}

template <int LPR, int EPL>
static void launch_logit_rows(const float* logits, const int64_t* labels, int64_t B, int C,
                              const LogitOut& o, hipStream_t st) {
  constexpr int ROWS = 256 / LPR;
  logit_rows_kernel<LPR, EPL><<<(unsigned)ceil_div(B, ROWS), 256, 0, st>>>(logits, labels, B, C,
                                                                          o);
}

__global__ __launch_bounds__(256) void variability_finalize_kernel(const float* __restrict__ m2,
                                                                   int64_t n, int K,
                                                                   float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float v = m2[i];
    // rounding can leave M2 a few ulps^2 below 0 where the K values agree; NaN stays NaN
    out[i] = sqrtf((v < 0.f ? 0.f : v) / (float)K);
  }
}

}  // namespace dd

using namespace dd;

extern "C" {

int dd_logit_scores(const float* logits, const int64_t* labels, int64_t B, int32_t C,
                    float* loss_accum, float* margin_accum, float* entropy_accum,
                    float* error_accum, float* wrong_mass_accum, float* var_mean, float* var_m2,
                    int32_t k, int32_t* bad_labels, void* stream) {
  clear_error();
  DD_REQUIRE(B >= 0, "dd_logit_scores: B < 0");
  DD_REQUIRE(C > 0, "dd_logit_scores: C must be positive (got %d)", C);
  DD_REQUIRE(loss_accum || margin_accum || entropy_accum || error_accum || wrong_mass_accum ||
                 var_mean || var_m2,
             "dd_logit_scores: no statistic requested");
  DD_REQUIRE(C >= 2 || !(margin_accum || error_accum),
             "dd_logit_scores: margin and error need C >= 2 (got %d)", C);
  DD_REQUIRE((var_mean != nullptr) == (var_m2 != nullptr),
             "dd_logit_scores: the Welford pair needs both var_mean and var_m2");
  DD_REQUIRE(!var_mean || k >= 1,
             "dd_logit_scores: the Welford update needs the checkpoint ordinal k >= 1 (got %d)",
             k);
  if (B == 0) return DD_OK;
  DD_REQUIRE(logits && labels, "dd_logit_scores: null logits/labels");
  hipStream_t st = as_stream(stream);
  const LogitOut o{loss_accum, margin_accum, entropy_accum, error_accum, wrong_mass_accum,
                   var_mean,   var_m2,       k,             bad_labels};
  if (C <= 16)
    launch_logit_lds<16, 1>(logits, labels, B, C, o, st);
  else if (C <= 32)
    launch_logit_lds<32, 1>(logits, labels, B, C, o, st);
  else if (C <= 64)
    launch_logit_lds<32, 2>(logits, labels, B, C, o, st);
  else if (C <= 128)
    launch_logit_lds<32, 4>(logits, labels, B, C, o, st);
  else if (C <= 256)
    launch_logit_rows<64, 4>(logits, labels, B, C, o, st);
  else if (C <= 1024)
    launch_logit_rows<64, 16>(logits, labels, B, C, o, st);
  else if (C <= 2048)
    launch_logit_rows<64, 32>(logits, labels, B, C, o, st);
  else
    logit_wide_kernel<<<(unsigned)B, 256, 0, st>>>(logits, labels, B, C, o);
  DD_CHECK_LAUNCH("dd_logit_scores");
  return DD_OK;
}

int dd_variability_finalize(const float* m2, int64_t n, int32_t K, float* out, void* stream) {
  clear_error();
  DD_REQUIRE(n >= 0 && K >= 1, "dd_variability_finalize: bad n/K");
  if (n == 0) return DD_OK;
  DD_REQUIRE(m2 && out, "dd_variability_finalize: null buffer");
  variability_finalize_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, as_stream(stream)>>>(
      m2, n, K, out);
  DD_CHECK_LAUNCH("dd_variability_finalize");
  return DD_OK;
}

}  // extern "C"
