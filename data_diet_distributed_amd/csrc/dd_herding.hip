// Kernel herding over feature rows, inside groups: the keep-set whose mean tracks the group's
// mean (include/dd_capi.h states the semantics):
//   dd_herding_workspace_bytes  bytes of the workspace of one dd_herding_greedy call (host only)
//   dd_herding_greedy           per group: the distance matrix once, P_i = ||f_i - mu||^2, the
//                               seeds folded into A, then `picks[g]` times take the unkept row
//                               with the largest A_i - (t + 1) P_i and add its matrix row to A
//
// Launches on one stream, no allocation, no synchronisation, nothing read back:
//   pack, layout, matrix  dd_distmat.h: bit for bit the matrices dd_kmedoids_greedy builds.
//   init    the groups' int64 sums = 0, picked = -1, value = -1.
//   sums, mean, p  dd_groupmean.h: the groups' exact fixed-point means mu and P_i = ||f_i - mu||^2
//           in fp32; a row the fixed point cannot hold gets P = NaN (it never wins) and is
//           counted in `bad`.
//   select  ONE launch: workgroup g, 1024 threads, runs group g's whole loop.  Thread k owns rows
//           k, k + 1024, ... of the group and keeps their A and P in REGISTERS (EPT = 1, 4 or 16
//           rows per thread, by the largest group: 32 registers at 16 384 rows); LDS holds only
//           the sixteen waves' candidates, twice (256 bytes).  The seed fold and every pick read
//           exactly one row M[j][.], every thread its EPT entries with all loads in flight at
//           once, consecutive threads on consecutive floats.  A pick: every thread forms
//           v_i = fma(-(t + 1), P_i, A_i) for its rows and the candidate
//               (ordered(v_i) << 32) | ~position,
//           ordered() the order-preserving map of a float onto unsigned integers (the sign bit
//           flipped for v >= 0, all bits for v < 0; -0 as +0), 0 for a NaN: "none".  The maximum
//           of its candidates, a six-step butterfly across the wave, one LDS entry per wave, ONE
//           barrier (the entries are double-buffered by the parity of t), and every thread takes
//           the maximum of the sixteen: the largest value with the smallest position, which is
//           the smallest id, whatever the arrival order.  Thread 0 writes picked[t][g] and
//           value[t][g]; then A_i += M[pick][i] and the pick's own A becomes NaN (kept: never a
//           candidate again).  No launch per pick, no host sync, no waiting on another workgroup.
//
// Invariance.  An entry of M is a function of the two rows and D alone (dd_feat.h); S is an exact
// integer sum, so mu is a function of the group's row SET; P_i of row i, mu and D.  A_i is one
// fp32 add chain: the seeds in ascending position, then the picks in pick order, an order the
// group's contents fix by induction over t (pick t is the maximum of a total order on values
// that depend on the earlier picks alone).  Which thread owns a row, EPT, `blocks`, the other
// groups and where the group lies in the call change none of these values, so the picks are
// bitwise independent of the launch geometry, the other groups, the chunk size, the lanes and the
// world size.
#include "dd_groupmean.h"

namespace dd {
namespace herding {

using namespace groupmean;

constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / kWave;
constexpr int kMaxEpt = kMaxRows / kSelThreads;
static_assert(kMaxEpt == 16 && kMaxEpt * kSelThreads == kMaxRows, "16 rows per thread at most");

// the workspace: distmat::MatLayout, then the groups' sums, their means and P
struct Layout : MatLayout {
  int64_t sums, mu, p, total;
};
static Layout layout(int64_t n, int D, int G, const int64_t* sizes) {
  Layout L;
  static_cast<MatLayout&>(L) = mat_layout(n, D, G, sizes);
  L.sums = L.mat_end;
  L.mu = L.sums + align256((int64_t)G * D * 8);
  L.p = L.mu + align256((int64_t)G * D * 4);
  L.total = L.p + align256(n * 4);
  return L;
}

__global__ __launch_bounds__(kThreads) void init_kernel(int64_t nsums, int64_t nslots,
                                                        long long* __restrict__ sums,
                                                        int64_t* __restrict__ picked,
                                                        float* __restrict__ value) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < nsums) sums[i] = 0;
  if (i < nslots) {
    picked[i] = -1;
    value[i] = -1.f;
  }
}

// The order-preserving map: a < b as floats <=> ordered(a) < ordered(b) as unsigned; -0 maps as
// +0.  Never 0 (-inf maps to 0x007fffff), so a candidate of 0 is free to mean "none".
__device__ __forceinline__ unsigned ordered(float v) {
  const unsigned u = __float_as_uint(v);
  if (v == 0.f) return 0x80000000u;
  return u & 0x80000000u ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float unordered(unsigned m) {
  return __uint_as_float(m & 0x80000000u ? m ^ 0x80000000u : ~m);
}
// position < 2^14, so ~position ascends as the position (and with it the id) descends
__device__ __forceinline__ unsigned long long candidate(float v, int pos) {
  if (v != v) return 0ull;  // kept (A is NaN), the tail and unrepresentable rows (P is NaN)
  return ((unsigned long long)ordered(v) << 32) | (unsigned)~(unsigned)pos;
}

// Workgroup g: the whole loop of group g (see the head of the file).
template <int EPT>
__global__ __launch_bounds__(kSelThreads) void select_kernel(
    const float* __restrict__ mat, const float* __restrict__ P, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ off, const int64_t* __restrict__ moff,
    const int64_t* __restrict__ seeds, const int64_t* __restrict__ seed_off, int64_t max_seeds,
    const int64_t* __restrict__ picks, int64_t steps, int G, int64_t* __restrict__ picked,
    float* __restrict__ value) {
  __shared__ unsigned long long s_best[2][kSelWaves];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int64_t r0 = off[g], r1 = off[g + 1];
  const int ng = (int)(r1 - r0);
  const int64_t quota = picks[g] < steps ? picks[g] : steps;
  if (ng <= 0 || quota <= 0) return;  // (the whole workgroup: nothing to pick)
  const float* __restrict__ M = mat + moff[g];
  const int pitch = (int)pitch_of(ng);

  float A[EPT], Pi[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * kSelThreads;
    A[e] = 0.f;
    Pi[e] = i < ng ? P[r0 + i] : __builtin_nanf("");  // the tail never wins
  }
  // A += M[j][.], and row j is kept from here on.  A row of M has `pitch` floats: nothing is
  // read past it.
  auto add_row = [&](int j) {
    const float* __restrict__ row = M + (int64_t)j * pitch;
    float m[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int i = tid + e * kSelThreads;
      m[e] = i < pitch ? row[i] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      A[e] += m[e];
      if (tid + e * kSelThreads == j) A[e] = __builtin_nanf("");
    }
  };

  int cnt = 0;  // |S|: the rows kept so far
  const int64_t s0 = seed_off ? seed_off[g] : 0;
  int64_t s1 = seed_off ? seed_off[g + 1] : 0;
  if (s1 - s0 > max_seeds) s1 = s0 + max_seeds;
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t p = seeds[s];
    if (p < r0 || p >= r1) continue;  // (outside the group: ignored)
    add_row((int)(p - r0));
    ++cnt;
  }

  const int lane = tid % kWave, wave = tid / kWave;
  for (int64_t t = 0; t < quota; ++t) {
    const float mult = -(float)(cnt + 1);
    unsigned long long best = 0ull;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const unsigned long long c = candidate(fmaf(mult, Pi[e], A[e]), tid + e * kSelThreads);
      best = c > best ? c : best;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      const unsigned long long c = (unsigned long long)shfl_xor64((int64_t)best, o);
      best = c > best ? c : best;
    }
    // Double-buffered by the parity of t: a wave reaches the write of pick t + 2 only past the
    // barrier of pick t + 1, which every wave reaches after its reads of pick t.
    if (lane == 0) s_best[t & 1][wave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kSelWaves; ++w) {
      const unsigned long long c = s_best[t & 1][w];
      best = c > best ? c : best;
    }
    if (best == 0ull) break;  // (the whole workgroup: no admissible row is left)
    const int j = (int)(~(unsigned)(best & 0xffffffffull) & (unsigned)(kMaxRows - 1));
    if (tid == 0) {
      picked[t * G + g] = ids[r0 + j];
      value[t * G + g] = unordered((unsigned)(best >> 32));
    }
    ++cnt;
    if (t + 1 < quota) add_row(j);
  }
}

struct Args {
  const float* rows;
  const int64_t *ids, *off, *seeds, *seed_off, *picks;
  int64_t n, max_seeds, steps;
  int D, G, blocks;
  int64_t* picked;
  float* value;
  int* bad;
};

template <bool F16>
static void launch(const Args& a, char* ws, const Layout& L, hipStream_t st) {
  float *mat = at<float>(ws, L.mat), *mu = at<float>(ws, L.mu), *P = at<float>(ws, L.p);
  long long* sums = at<long long>(ws, L.sums);
  const int64_t* moff = at<int64_t>(ws, L.moff);
  const int64_t nsums = (int64_t)a.G * a.D, nslots = a.steps * a.G;
  launch_matrices<F16>(a.rows, a.ids, a.off, a.n, a.D, a.G, ws, L, st);
  init_kernel<<<(unsigned)ceil_div(nsums > nslots ? nsums : nslots, kThreads), kThreads, 0, st>>>(
      nsums, nslots, sums, a.picked, a.value);
  if (L.max_rows == 0) return;  // every group is empty
  launch_mean_p(a.rows, a.off, a.D, a.G, L.max_rows, a.blocks, sums, mu, P, a.bad, st);
  if (a.steps == 0) return;
  auto select = L.max_rows <= kSelThreads       ? &select_kernel<1>
                : L.max_rows <= 4 * kSelThreads ? &select_kernel<4>
                                                : &select_kernel<kMaxEpt>;
  select<<<(unsigned)a.G, kSelThreads, 0, st>>>(mat, P, a.ids, a.off, moff, a.seeds, a.seed_off,
                                                a.max_seeds, a.picks, a.steps, a.G, a.picked,
                                                a.value);
}

}  // namespace herding
}  // namespace dd

using namespace dd;

extern "C" {

size_t dd_herding_workspace_bytes(int64_t n, int32_t D, int32_t G, const int64_t* sizes,
                                  int64_t steps, int32_t operands) {
  if (!herding::dims_ok(nullptr, n, D, G, sizes, steps, operands)) return 0;
  return (size_t)herding::layout(n, D, G, sizes).total;
}

int dd_herding_greedy(const float* rows, const int64_t* ids, int64_t n, int32_t D,
                      const int64_t* off, const int64_t* sizes, int32_t G, const int64_t* seeds,
                      const int64_t* seed_off, int64_t max_seeds, const int64_t* picks,
                      int64_t steps, int32_t operands, int32_t blocks, int64_t* picked,
                      float* value, int32_t* bad, void* workspace, size_t workspace_bytes,
                      void* stream) {
  clear_error();
  if (!herding::dims_ok("dd_herding_greedy", n, D, G, sizes, steps, operands)) return DD_EINVAL;
  DD_REQUIRE(max_seeds >= 0 && max_seeds <= n && blocks >= 0 && blocks <= herding::kMaxBlocks,
             "dd_herding_greedy: need 0 <= max_seeds <= n, 0 <= blocks <= %d (max_seeds=%lld, "
             "blocks=%d)", herding::kMaxBlocks, (long long)max_seeds, blocks);
  if (n == 0) return DD_OK;
  DD_REQUIRE(rows != nullptr && ids != nullptr && off != nullptr && picks != nullptr &&
                 bad != nullptr,
             "dd_herding_greedy: null rows / ids / off / picks / bad");
  DD_REQUIRE(max_seeds == 0 || (seeds != nullptr && seed_off != nullptr),
             "dd_herding_greedy: null seeds / seed_off with max_seeds > 0");
  DD_REQUIRE(steps == 0 || (picked != nullptr && value != nullptr),
             "dd_herding_greedy: null picked / value with steps > 0");
  const herding::Layout L = herding::layout(n, D, G, sizes);
  DD_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)L.total,
             "dd_herding_greedy: workspace of %zu bytes, need %lld (dd_herding_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, (long long)L.total);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_herding_greedy: the workspace must be 16-byte aligned");
  const herding::Args a = {rows, ids, off, max_seeds > 0 ? seeds : nullptr,
                           max_seeds > 0 ? seed_off : nullptr, picks, n, max_seeds, steps, D, G,
                           herding::resolve_blocks(L.max_rows, G, blocks), picked, value, bad};
  char* ws = static_cast<char*>(workspace);
  if (operands == DD_OPERANDS_F16X3)
    herding::launch<true>(a, ws, L, as_stream(stream));
  else
    herding::launch<false>(a, ws, L, as_stream(stream));
  DD_CHECK_LAUNCH("dd_herding_greedy");
  return DD_OK;
}

}  // extern "C"
