// Greedy k-medoids (the facility-location / inertia greedy) over feature rows, inside groups
// (include/dd_capi.h states the semantics):
//   dd_kmedoids_workspace_bytes  bytes of the workspace of one dd_kmedoids_greedy call (host only)
//   dd_kmedoids_greedy           per group: the distance matrix once, the seeds folded into cur,
//                                then `picks[g]` times take the row whose addition lowers
//                                sum_i cur_i the most and fold it in
//
// Launches on one stream, no allocation, no synchronisation, nothing read back:
//   pack, layout, matrix  dd_distmat.h (shared with dd_herding.hip): the rows' operand halves and
//           norms, moff[g], and once per call the groups' squared-distance matrices M, rows
//           pitched to a multiple of 64 floats, the tail +0, the diagonal 0.  Only rows M[c][.]
//           are ever read afterwards (by the seed fold, the pick fold and the gain alike).
//   init    cur (both buffers and the caller's) = +inf, the slots = 0, the NaN norms counted.
//   seed    launch j folds seeds [j S, (j + 1) S) of every group: cur_i = min(cur_i, M[s][i]), a
//           seed's own entry -1 (kept).
//   pick    launch t (t = 0 .. max picks): workgroup (b, g) leaves at once when t > picks[g].
//           Otherwise it forms v_i = min(cur_i, M[p][i]) in LDS for the row p that launch t - 1
//           published (none at t = 0), v_p = -1, the whole group: n_g <= 16384 rows are 64 KiB.
//           cur is double-buffered by the parity of t: the launch reads buffer t & 1, and every
//           workgroup writes ITS slice of v into the other buffer, so no workgroup reads what
//           another writes in the same launch.  Then, when t < picks[g], wave w streams its rows
//           M[j][.] (j unkept) against v,
//               gain_j = sum_i max(v_i - M[j][i], 0),
//           and the workgroup publishes its best candidate with one 64-bit atomic maximum into
//           slot [t][g]:  (bits(gain) << 32) | ~position.  Gains are >= 0 and order as their bit
//           patterns; positions ascend with the ids, so the maximum is the largest gain with the
//           smallest id whatever the order of arrival.  The launch boundary on the stream is the
//           only ordering between workgroups: no kernel waits for another workgroup.
//   finish  slot [t][g] -> picked[t][g] and gain[t][g]; the buffer group g wrote last -> cur.
//
// The gain's order: lane l of the wave that owns j takes positions l, l + 64, ... ascending in one
// add chain (kept rows and the tail add exact zeros: max(-1 - M, 0) = max(0 - 0, 0) = 0), then the
// fixed butterfly.  The order depends on n_g alone, so a gain does not depend on the launch
// geometry, the other groups or which wave computes it.
#include "dd_distmat.h"

namespace dd {
namespace kmedoids {

using namespace distmat;

constexpr int kWaves = kThreads / kWave;
constexpr int kMaxSeedBatch = DD_KCENTER_MAX_SEED_BATCH;
constexpr int kMaxBlocks = DD_KCENTER_MAX_BLOCKS;
constexpr int kCheckBlocks = 256;    // workgroups per group from which the slot is read first
constexpr int kGainUnroll = 8;       // matrix loads a lane has in flight

// workgroups per group of the seed and pick launches (0: from the largest group and G alone)
static int resolve_blocks(int64_t max_rows, int G, int blocks) {
  if (blocks > 0) return blocks;
  int64_t b = ceil_div(max_rows > 0 ? max_rows : 1, 4 * kWaves);  // at least four rows per wave
  const int64_t cap = kTargetBlocks / G > 1 ? kTargetBlocks / G : 1;
  if (b > cap) b = cap;
  return (int)b;
}

// the workspace: distmat::MatLayout (the halves, the norms, the matrices' offsets and the
// matrices), then the two cur buffers and the slots
struct Layout : MatLayout {
  int64_t cur, slots, total;
};
static Layout layout(int64_t n, int D, int G, const int64_t* sizes, int64_t steps) {
  Layout L;
  static_cast<MatLayout&>(L) = mat_layout(n, D, G, sizes);
  L.cur = L.mat_end;
  L.slots = L.cur + align256(2 * n * 4);
  L.total = L.slots + align256((steps > 0 ? steps : 1) * (int64_t)G * 8);
  return L;
}

__global__ __launch_bounds__(kThreads) void init_kernel(const float* __restrict__ norm, int64_t n,
                                                        int64_t nslots, float* __restrict__ cur,
                                                        float* __restrict__ buf,
                                                        unsigned long long* __restrict__ slots,
                                                        int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < nslots) slots[i] = 0ull;
  if (i >= n) return;
  cur[i] = INFINITY;
  buf[i] = INFINITY;
  buf[n + i] = INFINITY;
  const float s = norm[i];
  if (s != s) atomicAdd(bad, 1);  // (pack_kernel's mark of a row with a NaN or an infinity)
}

// Seed launch `batch`: workgroup (b, g) folds centres seeds[s0 + batch S .. + S) of group g, whose
// seed list is seeds[seed_off[g] .. seed_off[g + 1]) (positions of rows), into cur.
__global__ __launch_bounds__(kThreads) void seed_kernel(
    const float* __restrict__ mat, const int64_t* __restrict__ off,
    const int64_t* __restrict__ moff, const int64_t* __restrict__ seeds,
    const int64_t* __restrict__ seed_off, int batch, int S, float* __restrict__ cur) {
  __shared__ int64_t s_pos[kMaxSeedBatch];
  const int g = blockIdx.y;
  const int64_t s0 = seed_off[g] + (int64_t)batch * S;
  const int64_t left = seed_off[g + 1] - s0;
  if (left <= 0) return;  // (the whole workgroup: this group's seeds are folded)
  const int cnt = left < S ? (int)left : S;
  const int64_t r0 = off[g], r1 = off[g + 1];
  const int ng = (int)(r1 - r0);
  const float* __restrict__ M = mat + moff[g];
  const int pitch = (int)pitch_of(ng);
  if (threadIdx.x < cnt) {
    const int64_t p = seeds[s0 + threadIdx.x];
    s_pos[threadIdx.x] = p >= r0 && p < r1 ? p - r0 : -1;  // (outside the group: ignored)
  }
  __syncthreads();
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < ng; i += gridDim.x * kThreads) {
    float m = cur[r0 + i];
    if (m < 0.f) continue;  // kept already
    bool kept = false;
    for (int s = 0; s < cnt; ++s) {
      const int64_t p = s_pos[s];
      if (p < 0) continue;
      m = fminf(m, M[p * pitch + i]);
      kept = kept || p == i;
    }
    cur[r0 + i] = kept ? -1.f : m;
  }
}

// The candidate of a row: 0 is "none" (a gain that is NaN).  n < 2^31, so ~position is never 0 and
// a candidate with gain 0 still beats "none": a quota is always met.
__device__ __forceinline__ unsigned long long candidate(float gain, int64_t pos) {
  if (!(gain >= 0.f)) return 0ull;
  return ((unsigned long long)__float_as_uint(gain) << 32) | (unsigned)~(unsigned)pos;
}

// THE gain routine: sum_i max(v[i] - row[i], 0) over the pitched row, as the wave's sum (the same
// value on every lane).  Lane l takes positions l, l + 64, ... ascending in one add chain; the
// loads of kGainUnroll positions are issued before their adds.  pitch is a multiple of 64, so
// every lane makes the same trips.
__device__ __forceinline__ float row_gain(const float* __restrict__ row,
                                          const float* __restrict__ v, int pitch, int lane) {
  float s = 0.f;
  int i = lane;
  for (; i + (kGainUnroll - 1) * kWave < pitch; i += kGainUnroll * kWave) {
    float m[kGainUnroll];
#pragma unroll
    for (int e = 0; e < kGainUnroll; ++e) m[e] = __builtin_nontemporal_load(row + i + e * kWave);
#pragma unroll
    for (int e = 0; e < kGainUnroll; ++e) s += fmaxf(v[i + e * kWave] - m[e], 0.f);
  }
  for (; i < pitch; i += kWave) s += fmaxf(v[i] - __builtin_nontemporal_load(row + i), 0.f);
  return group_sum<kWave>(s);
}

// Pick launch t (see the head of the file).  slots: [steps][G], zeroed by init_kernel; buf: the
// two cur buffers [2][n].
__global__ __launch_bounds__(kThreads) void pick_kernel(
    const float* __restrict__ mat, const int64_t* __restrict__ off,
    const int64_t* __restrict__ moff, const int64_t* __restrict__ picks, int64_t n, int t,
    int64_t steps, int G, unsigned long long* __restrict__ slots, float* __restrict__ buf) {
  extern __shared__ __attribute__((aligned(16))) float s_v[];  // [pitch]
  __shared__ unsigned long long s_best[kWaves];
  const int g = blockIdx.y;
  const int64_t quota = picks[g];
  if (t > quota) return;  // (the whole workgroup: the group has met its quota)
  const int64_t r0 = off[g], r1 = off[g + 1];
  const int ng = (int)(r1 - r0);
  if (ng <= 0) return;
  const float* __restrict__ M = mat + moff[g];
  const int pitch = (int)pitch_of(ng);
  int cpos = -1;  // the newest centre: the pick of launch t - 1, as a position in the group
  if (t > 0) {
    const unsigned long long prev = slots[(int64_t)(t - 1) * G + g];
    if (prev != 0ull) {
      const int64_t p = (int64_t)(unsigned)~(unsigned)(prev & 0xffffffffull);
      if (p >= r0 && p < r1) cpos = (int)(p - r0);
    }
  }
  const float* __restrict__ cur_in = buf + (int64_t)(t & 1) * n + r0;
  float* __restrict__ cur_out = buf + (int64_t)((t + 1) & 1) * n + r0;
  const float* __restrict__ prow = M + (int64_t)(cpos >= 0 ? cpos : 0) * pitch;
  for (int i = threadIdx.x; i < pitch; i += kThreads) {
    float v = 0.f;  // (the tail: max(0 - 0, 0) adds nothing)
    if (i < ng) {
      v = cur_in[i];
      if (cpos >= 0) v = i == cpos ? -1.f : fminf(v, prow[i]);  // (kept: min(-1, M >= 0) = -1)
    }
    s_v[i] = v;
  }
  __syncthreads();
  // this workgroup's slice of the next buffer
  const int chunk = (ng + (int)gridDim.x - 1) / (int)gridDim.x;
  const int i0 = (int)blockIdx.x * chunk, i1 = i0 + chunk < ng ? i0 + chunk : ng;
  for (int i = i0 + threadIdx.x; i < i1; i += kThreads) cur_out[i] = s_v[i];
  if (!(t < quota && t < steps)) return;  // (no slot [t][g]: the last fold of the group)

  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  unsigned long long best = 0ull;
  for (int j = (int)blockIdx.x * kWaves + wave; j < ng; j += (int)gridDim.x * kWaves) {
    if (s_v[j] < 0.f) continue;  // kept: never a candidate again (the whole wave)
    const unsigned long long c = candidate(row_gain(M + (int64_t)j * pitch, s_v, pitch, lane),
                                           r0 + j);
    best = c > best ? c : best;
  }
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) best = s_best[w] > best ? s_best[w] : best;
    // The slot only grows, so a candidate that does not beat the value read here (however stale)
    // cannot win: with many workgroups per group most skip the atomic, which every one of them
    // would otherwise issue on ONE address (dd_kcenter.hip's rule).
    unsigned long long* slot = &slots[(int64_t)t * G + g];
    if (best != 0ull &&
        (gridDim.x < kCheckBlocks ||
         best > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
      atomicMax(slot, best);
  }
}

// slot [t][g] -> picked[t][g] (the id) and gain[t][g] (the float)
__global__ __launch_bounds__(kThreads) void finish_kernel(
    const unsigned long long* __restrict__ slots, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ picks, int64_t n, int64_t steps, int G,
    int64_t* __restrict__ picked, float* __restrict__ gain) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= steps * G) return;
  const int64_t t = i / G;
  const int g = (int)(i % G);
  const unsigned long long v = slots[i];
  const int64_t p = (int64_t)(unsigned)~(unsigned)(v & 0xffffffffull);
  const bool has = t < picks[g] && v != 0ull && p < n;
  picked[i] = has ? ids[p] : -1;
  gain[i] = has ? __uint_as_float((unsigned)(v >> 32)) : -1.f;
}

// group g's final cur: launch picks[g] was its last and wrote buffer (picks[g] + 1) & 1
__global__ __launch_bounds__(kThreads) void final_cur_kernel(
    const int64_t* __restrict__ off, const int64_t* __restrict__ picks, int64_t n,
    const float* __restrict__ buf, float* __restrict__ cur) {
  const int g = blockIdx.y;
  const int64_t r0 = off[g], r1 = off[g + 1];
  const float* __restrict__ src = buf + ((picks[g] + 1) & 1) * n;
  for (int64_t r = r0 + (int64_t)blockIdx.x * kThreads + threadIdx.x; r < r1;
       r += (int64_t)gridDim.x * kThreads)
    cur[r] = src[r];
}

struct Args {
  const float* rows;
  const int64_t *ids, *off, *seeds, *seed_off, *picks;
  int64_t n, max_seeds, steps;
  int D, G, S, blocks;
  int64_t* picked;
  float *gain, *cur;
  int* bad;
};

template <bool F16>
static void launch(const Args& a, char* ws, const Layout& L, hipStream_t st) {
  float *norm = at<float>(ws, L.c_norm), *mat = at<float>(ws, L.mat), *buf = at<float>(ws, L.cur);
  int64_t* moff = at<int64_t>(ws, L.moff);
  unsigned long long* slots = at<unsigned long long>(ws, L.slots);
  const int64_t nslots = a.steps * a.G;
  launch_matrices<F16>(a.rows, a.ids, a.off, a.n, a.D, a.G, ws, L, st);
  init_kernel<<<(unsigned)ceil_div(a.n > nslots ? a.n : nslots, kThreads), kThreads, 0, st>>>(
      norm, a.n, nslots, a.cur, buf, slots, a.bad);
  if (L.max_rows == 0) return;  // every group is empty
  const dim3 grid((unsigned)a.blocks, (unsigned)a.G);
  for (int64_t j = 0; j * a.S < a.max_seeds; ++j)
    seed_kernel<<<grid, kThreads, 0, st>>>(mat, a.off, moff, a.seeds, a.seed_off, (int)j, a.S,
                                           buf);
  conv::lds_attr<&pick_kernel>(kMaxRows * 4);
  const size_t lds = (size_t)pitch_of(L.max_rows) * sizeof(float);
  for (int64_t t = 0; t <= a.steps; ++t)
    pick_kernel<<<grid, kThreads, lds, st>>>(mat, a.off, moff, a.picks, a.n, (int)t, a.steps, a.G,
                                             slots, buf);
  final_cur_kernel<<<dim3((unsigned)ceil_div(L.max_rows, 4 * kThreads), (unsigned)a.G), kThreads,
                     0, st>>>(a.off, a.picks, a.n, buf, a.cur);
  if (a.steps > 0)
    finish_kernel<<<(unsigned)ceil_div(nslots, kThreads), kThreads, 0, st>>>(
        slots, a.ids, a.picks, a.n, a.steps, a.G, a.picked, a.gain);
}

}  // namespace kmedoids
}  // namespace dd

using namespace dd;

extern "C" {

size_t dd_kmedoids_workspace_bytes(int64_t n, int32_t D, int32_t G, const int64_t* sizes,
                                   int64_t steps, int32_t operands) {
  if (!kmedoids::dims_ok(nullptr, n, D, G, sizes, steps, operands)) return 0;
  return (size_t)kmedoids::layout(n, D, G, sizes, steps).total;
}

int dd_kmedoids_greedy(const float* rows, const int64_t* ids, int64_t n, int32_t D,
                       const int64_t* off, const int64_t* sizes, int32_t G, const int64_t* seeds,
                       const int64_t* seed_off, int64_t max_seeds, const int64_t* picks,
                       int64_t steps, int32_t operands, int32_t seed_batch, int32_t blocks,
                       int64_t* picked, float* gain, float* cur, int32_t* bad, void* workspace,
                       size_t workspace_bytes, void* stream) {
  clear_error();
  if (!kmedoids::dims_ok("dd_kmedoids_greedy", n, D, G, sizes, steps, operands)) return DD_EINVAL;
  DD_REQUIRE(max_seeds >= 0 && max_seeds <= n && seed_batch >= 0 &&
                 seed_batch <= kmedoids::kMaxSeedBatch && blocks >= 0 &&
                 blocks <= kmedoids::kMaxBlocks,
             "dd_kmedoids_greedy: need 0 <= max_seeds <= n, 0 <= seed_batch <= %d, 0 <= blocks "
             "<= %d (max_seeds=%lld, seed_batch=%d, blocks=%d)",
             kmedoids::kMaxSeedBatch, kmedoids::kMaxBlocks, (long long)max_seeds, seed_batch,
             blocks);
  if (n == 0) return DD_OK;
  DD_REQUIRE(rows != nullptr && ids != nullptr && off != nullptr && picks != nullptr &&
                 cur != nullptr && bad != nullptr,
             "dd_kmedoids_greedy: null rows / ids / off / picks / cur / bad");
  DD_REQUIRE(max_seeds == 0 || (seeds != nullptr && seed_off != nullptr),
             "dd_kmedoids_greedy: null seeds / seed_off with max_seeds > 0");
  DD_REQUIRE(steps == 0 || (picked != nullptr && gain != nullptr),
             "dd_kmedoids_greedy: null picked / gain with steps > 0");
  const kmedoids::Layout L = kmedoids::layout(n, D, G, sizes, steps);
  DD_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)L.total,
             "dd_kmedoids_greedy: workspace of %zu bytes, need %lld "
             "(dd_kmedoids_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, (long long)L.total);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_kmedoids_greedy: the workspace must be 16-byte aligned");
  const kmedoids::Args a = {rows, ids, off, seeds, seed_off, picks, n, max_seeds, steps, D, G,
                            seed_batch > 0 ? seed_batch : 8,
                            kmedoids::resolve_blocks(L.max_rows, G, blocks), picked, gain, cur,
                            bad};
  char* ws = static_cast<char*>(workspace);
  if (operands == DD_OPERANDS_F16X3)
    kmedoids::launch<true>(a, ws, L, as_stream(stream));
  else
    kmedoids::launch<false>(a, ws, L, as_stream(stream));
  DD_CHECK_LAUNCH("dd_kmedoids_greedy");
  return DD_OK;
}

}  // extern "C"
