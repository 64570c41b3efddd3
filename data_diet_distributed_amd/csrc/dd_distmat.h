// The per-group squared-distance matrices of the centre-based fills (dd_kmedoids.hip,
// dd_herding.hip): the one builder both include, so that an entry of M has one definition.
//   pack    feat::pack_kernel on the group-sorted rows: operand halves and ||f||^2 (NaN marks a
//           non-finite row).
//   layout  one workgroup: moff[g], the float offset of group g's matrix, from `off`.
//   matrix  once per call.  Workgroup (x, g) takes 128 points of group g against a range of its
//           centres, 128 at a time, through feat::scan_keys: THE key, so its invariance argument
//           stays in dd_feat.h.  The scan leaves the POINT on the lane, so the epilogue stores
//           M[c][.] with consecutive lanes on consecutive points: 128-byte runs per half wave.
//           Rows are pitched to a multiple of 64 floats, the tail past n_g holds +0 and the
//           diagonal is forced to 0.  Only rows M[c][.] are ever read afterwards: one source of
//           every distance, and the matrix need not be symmetric (it is not, bit for bit: the
//           second and third split products swap with the operands).
#pragma once
#include "dd_feat.h"

namespace dd {
namespace distmat {

using namespace feat;

constexpr int kMaxRows = DD_KMEDOIDS_MAX_GROUP_ROWS;
constexpr int kMaxGroups = DD_KCENTER_MAX_GROUPS;
constexpr int kTargetBlocks = 1024;  // workgroups of one launch the automatic counts aim at

__host__ __device__ constexpr int64_t pitch_of(int64_t ng) { return (ng + 63) / 64 * 64; }

// the head of a workspace: feat::PackLayout with no queries (the rows are points and centres at
// once: the "candidate" halves and norms serve both), then the matrices' offsets and the
// matrices; a caller's own buffers start at `mat_end`
struct MatLayout : PackLayout {
  int64_t moff, mat, mat_end;
  int64_t max_rows;
};
inline MatLayout mat_layout(int64_t n, int D, int G, const int64_t* sizes) {
  MatLayout L;
  static_cast<PackLayout&>(L) = pack_layout(0, n, D);
  int64_t floats = 0;
  L.max_rows = 0;
  for (int g = 0; g < G; ++g) {
    floats += sizes[g] * pitch_of(sizes[g]);
    if (sizes[g] > L.max_rows) L.max_rows = sizes[g];
  }
  L.moff = L.end;
  L.mat = L.moff + align256(((int64_t)G + 1) * 8);
  L.mat_end = L.mat + align256(floats * 4);
  return L;
}

// `what` null: no error text (the *_workspace_bytes entry points answer 0)
inline bool dims_ok(const char* what, int64_t n, int32_t D, int32_t G, const int64_t* sizes,
                    int64_t steps, int32_t operands) {
  if (!rows_dims_ok(what, 0, n, D, operands)) return false;
  if (G < 1 || G > kMaxGroups || steps < 0 || steps > n || sizes == nullptr) {
    if (what)
      set_error("%s: need 1 <= G <= %d, 0 <= steps <= n and the groups' sizes (G=%d, "
                "steps=%lld, n=%lld)", what, kMaxGroups, G, (long long)steps, (long long)n);
    return false;
  }
  int64_t sum = 0;
  for (int g = 0; g < G; ++g) {
    if (sizes[g] < 0 || sizes[g] > kMaxRows) {
      if (what)
        set_error("%s: group %d has %lld rows; a group's distance matrix holds at most "
                  "DD_KMEDOIDS_MAX_GROUP_ROWS = %d", what, g, (long long)sizes[g], kMaxRows);
      return false;
    }
    sum += sizes[g];
  }
  if (sum > n) {
    if (what)
      set_error("%s: the groups' sizes sum to %lld, above n=%lld", what, (long long)sum,
                (long long)n);
    return false;
  }
  return true;
}

// moff[g] = sum over h < g of n_h pitch_h, g = 0 .. G (one workgroup; thread k sums a run of
// consecutive groups, thread 0 scans the 256 partial sums; static: each unit that includes this
// header has its own copy of the one kernel here that is no template)
static __global__ __launch_bounds__(kThreads) void layout_kernel(const int64_t* __restrict__ off,
                                                                 int G,
                                                                 int64_t* __restrict__ moff) {
  __shared__ int64_t s_part[kThreads];
  const int per = (G + kThreads - 1) / kThreads;
  const int g0 = threadIdx.x * per, g1 = g0 + per < G ? g0 + per : G;
  int64_t sum = 0;
  for (int g = g0; g < g1; ++g) {
    const int64_t ng = off[g + 1] - off[g];
    sum += ng * pitch_of(ng);
  }
  s_part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int k = 0; k < kThreads; ++k) {
      const int64_t v = s_part[k];
      s_part[k] = run;
      run += v;
    }
    moff[G] = run;
  }
  __syncthreads();
  int64_t run = s_part[threadIdx.x];
  for (int g = g0; g < g1; ++g) {
    const int64_t ng = off[g + 1] - off[g];
    moff[g] = run;
    run += ng * pitch_of(ng);
  }
}

// Workgroup (x, g): points [128 pt, 128 pt + 128) of group g against the centres of split sp,
// x = pt csplit + sp (a split is a run of whole 128-centre steps).
template <bool F16>
__global__ __launch_bounds__(kThreads) void matrix_kernel(
    const uint16_t* __restrict__ hi, const uint16_t* __restrict__ lo,
    const float* __restrict__ norm, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ off, const int64_t* __restrict__ moff, int Dp, int csplit,
    float* __restrict__ mat) {
  __shared__ ScanLds lds;
  const int g = blockIdx.y;
  const int64_t r0 = off[g], r1 = off[g + 1];
  const int ng = (int)(r1 - r0);
  if (ng <= 0) return;  // (the whole workgroup, here and below)
  float* __restrict__ M = mat + moff[g];
  const int pitch = (int)pitch_of(ng);
  if (ng == 1) {  // one row: its own distance and the tail
    if (blockIdx.x == 0 && threadIdx.x < pitch) M[threadIdx.x] = 0.f;
    return;
  }
  const int pt = blockIdx.x / csplit, sp = blockIdx.x % csplit;
  if (pt * TQ >= ng) return;
  const int ctiles = (ng + TC - 1) / TC;
  const int64_t span = (int64_t)((ctiles + csplit - 1) / csplit) * TC;  // centres per split
  const int64_t cs = r0 + sp * span, ce = cs + span < r1 ? cs + span : r1;
  if (cs >= ce) return;

  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int li = pt * TQ + wave * 32 + (lane & 31);  // this lane's point (both lane halves hold it)
  const int64_t qr = r0 + li;
  const bool qvalid = li < ng;
  const uint16_t* __restrict__ qh_row = hi + (qvalid ? qr : r0) * (int64_t)Dp;
  const uint16_t* __restrict__ ql_row = lo + (qvalid ? qr : r0) * (int64_t)Dp;
  const float fn = qvalid ? norm[qr] : 0.f;
  const bool store = li < pitch;  // the tail [n_g, pitch) is written too: +0
  scan_keys<F16>(lds, qh_row, ql_row, qvalid, hi, lo, norm, ids, cs, ce, Dp,
                 [&](float key, int lr, int64_t c0) {
                   const int64_t c = c0 + lr;
                   if (!store || c >= ce) return;
                   const float d2 = qvalid && c != qr ? fmaxf(fn + key, 0.f) : 0.f;
                   M[(c - r0) * pitch + li] = d2;
                 });
}

// pack, layout and, unless every group is empty, the matrices: 128-point tiles of the largest
// group, the centres split until the launch has about kTargetBlocks workgroups (smaller groups
// leave at once where they have no tile)
template <bool F16>
inline void launch_matrices(const float* rows, const int64_t* ids, const int64_t* off, int64_t n,
                            int D, int G, char* ws, const MatLayout& L, hipStream_t st) {
  uint16_t *hi = at<uint16_t>(ws, L.c_hi), *lo = at<uint16_t>(ws, L.c_lo);
  float* norm = at<float>(ws, L.c_norm);
  int64_t* moff = at<int64_t>(ws, L.moff);
  pack_kernel<F16><<<(unsigned)ceil_div(n, kRows), kThreads, 0, st>>>(rows, n, D, L.Dp, hi, lo,
                                                                      norm, nullptr);
  layout_kernel<<<1, kThreads, 0, st>>>(off, G, moff);
  if (L.max_rows == 0) return;
  const int tiles = (int)ceil_div(L.max_rows, TQ);
  int csplit = (int)ceil_div(kTargetBlocks, (int64_t)tiles * G);
  if (csplit > tiles) csplit = tiles;
  matrix_kernel<F16><<<dim3((unsigned)(tiles * csplit), (unsigned)G), kThreads, 0, st>>>(
      hi, lo, norm, ids, off, moff, L.Dp, csplit, at<float>(ws, L.mat));
}

}  // namespace distmat
}  // namespace dd
