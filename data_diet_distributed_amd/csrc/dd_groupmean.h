// The group means and the rows' squared distances to them, as the fills that read a group's mean
// take them (dd_herding.hip, dd_cover.hip): the three kernels both include, so that mu and P have
// one definition.  The caller zeroes `sums` and `bad` on the stream before launch_mean_p.
//   sums    workgroup (b, g) adds its slice of group g's rows in dd_class_feature_sums' 2^-24
//           fixed point (thread k owns columns k, k + 256, ...; one 64-bit atomic per column and
//           workgroup).  Integer sums are exact, so they do not depend on `blocks`.
//   mean    mu[g][d] = (float)(((double)S[g][d] / n_g) * 2^-24), dd_class_centroids' formula.
//   p       one row per wave: P_i = feat::wave_row_sqdist(f_i, mu_g) in fp32 (the fixed lane
//           order and butterfly); a row with an element that is NaN, infinite or has |v| >= 2^15
//           gets P = NaN and is counted in `bad`.
// The kernels are static: each unit that includes this header has its own copy.
#pragma once
#include "dd_distmat.h"

namespace dd {
namespace groupmean {

using namespace distmat;

constexpr int kMaxBlocks = DD_KCENTER_MAX_BLOCKS;
constexpr float kRange = 32768.f;      // |v| < 2^15: |q(v)| < 2^39 (dd_class_feature_sums' rule)
constexpr double kScale = 16777216.0;  // 2^24

// q(v) = round-to-nearest-even(v * 2^24); exact in double for |v| < 2^15
__device__ __forceinline__ long long quantise(float v) {
  return __double2ll_rn((double)v * kScale);
}

// workgroups per group of the sums launch (0: from the largest group and G alone)
inline int resolve_blocks(int64_t max_rows, int G, int blocks) {
  if (blocks > 0) return blocks;
  int64_t b = ceil_div(max_rows > 0 ? max_rows : 1, 64);  // at least 64 rows per workgroup
  const int64_t cap = kTargetBlocks / G > 1 ? kTargetBlocks / G : 1;
  return (int)(b > cap ? cap : b);
}

// Workgroup (b, g): rows [i0, i1) of group g, 256 columns at a time; an element outside the
// range adds nothing (p_kernel counts its row, and the caller rejects the call's results).
static __global__ __launch_bounds__(kThreads) void sums_kernel(const float* __restrict__ rows,
                                                               const int64_t* __restrict__ off,
                                                               int D,
                                                               long long* __restrict__ sums) {
  const int g = blockIdx.y;
  const int64_t r0 = off[g];
  const int ng = (int)(off[g + 1] - r0);
  const int chunk = (ng + (int)gridDim.x - 1) / (int)gridDim.x;
  const int i0 = (int)blockIdx.x * chunk, i1 = i0 + chunk < ng ? i0 + chunk : ng;
  if (i0 >= i1) return;  // (the whole workgroup)
  for (int d = threadIdx.x; d < D; d += kThreads) {
    const float* __restrict__ col = rows + r0 * (int64_t)D + d;
    long long acc = 0;
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
      const float v = col[i * (int64_t)D];
      acc += fabsf(v) < kRange ? quantise(v) : 0ll;
    }
    if (acc != 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(sums + (int64_t)g * D + d),
                (unsigned long long)acc);
  }
}

static __global__ __launch_bounds__(kThreads) void mean_kernel(const long long* __restrict__ sums,
                                                               const int64_t* __restrict__ off,
                                                               int64_t total, int D,
                                                               float* __restrict__ mu) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int64_t g = i / D;
  const int64_t ng = off[g + 1] - off[g];
  mu[i] = ng > 0 ? (float)(((double)sums[i] / (double)ng) * (1.0 / kScale)) : 0.f;
}

// one row per wave: workgroup (x, g) takes rows [4 x, 4 x + 4) of group g
static __global__ __launch_bounds__(kThreads) void p_kernel(const float* __restrict__ rows,
                                                            const int64_t* __restrict__ off,
                                                            const float* __restrict__ mu, int D,
                                                            float* __restrict__ P,
                                                            int* __restrict__ bad) {
  const int g = blockIdx.y;
  const int lane = threadIdx.x % kWave;
  const int64_t r0 = off[g];
  const int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x / kWave;
  if (i >= off[g + 1] - r0) return;  // (a whole wave: the shuffles below stay within one wave)
  const float* __restrict__ x = rows + (r0 + i) * (int64_t)D;
  float oor = 0.f;
  for (int d = lane; d < D; d += kWave) oor = fabsf(x[d]) < kRange ? oor : 1.f;
  oor = group_max<kWave>(oor);
  const float s = wave_row_sqdist(x, mu + (int64_t)g * D, D, lane, true, nullptr);
  if (lane == 0) {
    P[r0 + i] = oor != 0.f ? __builtin_nanf("") : s;
    if (oor != 0.f) atomicAdd(bad, 1);
  }
}

// sums (already zero) -> mu -> P, for groups of at most `max_rows` > 0 rows
inline void launch_mean_p(const float* rows, const int64_t* off, int D, int G, int64_t max_rows,
                          int blocks, long long* sums, float* mu, float* P, int* bad,
                          hipStream_t st) {
  const int64_t nsums = (int64_t)G * D;
  sums_kernel<<<dim3((unsigned)blocks, (unsigned)G), kThreads, 0, st>>>(rows, off, D, sums);
  mean_kernel<<<(unsigned)ceil_div(nsums, kThreads), kThreads, 0, st>>>(sums, off, nsums, D, mu);
  p_kernel<<<dim3((unsigned)ceil_div(max_rows, kRows), (unsigned)G), kThreads, 0, st>>>(
      rows, off, mu, D, P, bad);
}

}  // namespace groupmean
}  // namespace dd
