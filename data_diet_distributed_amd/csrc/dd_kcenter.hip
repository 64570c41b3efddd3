// Greedy k-center (farthest-first traversal) over feature rows, inside groups (include/dd_capi.h
// states the semantics):
//   dd_kcenter_workspace_bytes  bytes of the workspace of one dd_kcenter_greedy call (host only)
//   dd_kcenter_greedy           per group: fold the seeds into mind2, then `picks[g]` times take
//                               the row with the largest mind2 and fold it in
//
// Launches on one stream, no allocation, no synchronisation, nothing read back:
//   init    one wave per row: mind2 = +inf, and the rows with a non-finite element are counted.
//   seed    launch j folds centres [j S, (j + 1) S) of every group's seed list: a workgroup stages
//           its group's centres of the batch in LDS, reads each of its rows ONCE and takes the
//           minimum over the staged centres.  A row that is one of the centres becomes -1 (kept).
//   pick    launch t (t = 0 .. max picks): workgroup (b, g) leaves at once when t > picks[g];
//           otherwise it stages the centre that launch t - 1 published for its group (none at
//           t = 0: the seeds are folded already), updates its rows' mind2 against it, reduces
//           (mind2, position) over its rows and, when t < picks[g], publishes its best candidate
//           with one 64-bit atomic maximum into slot [t][g]:
//               (bits(mind2) << 32) | ~position
//           Non-negative floats order as their bit patterns and the rows of a group are in
//           ascending id, so the maximum is the largest mind2 with the smallest id, whatever the
//           order in which the workgroups arrive.  Launch t + 1 reads the slot as its centre.
//           The launch boundary on the stream is the only ordering between workgroups: no
//           kernel waits for another workgroup.
//   finish  slot [t][g] -> picked[t][g] (the id) and radius2[t][g] (the float).
//
// d2(row, centre) is ONE routine (pair_d2): lane l of the wave that owns the row takes columns
// 256 j + 4 l + e (j ascending, e = 0..3) into one fmaf chain, columns past D contributing exact
// zeros, then the fixed butterfly.  The order depends on D alone, so a d2 does not depend on the
// launch geometry, the group layout, the other rows, the seed batch, the rows' alignment (a row
// that is not 16-byte aligned is read with scalar loads into the SAME lanes) or on whether the
// centre arrives as a seed or as a pick; min and max are order-independent.
#include "dd_feat.h"

namespace dd {
namespace kcenter {

using feat::align256;
using feat::kMaxD;
using feat::kThreads;

constexpr int kWaves = kThreads / kWave;
constexpr int kPass = 4 * kWave;      // columns a wave covers with one 16-byte load per lane
constexpr int kSeedLds = 48 * 1024;   // bytes of staged centres per seed workgroup, at most
constexpr int kMaxSeedBatch = DD_KCENTER_MAX_SEED_BATCH;
constexpr int kMaxBlocks = DD_KCENTER_MAX_BLOCKS;
constexpr int kMaxGroups = DD_KCENTER_MAX_GROUPS;
constexpr int kTargetBlocks = 1024;   // workgroups of one launch the automatic count aims at
constexpr int kCheckBlocks = 256;     // workgroups per group from which the slot is read first

// passes of 256 columns, rounded up to a power of two (the row's registers: 4 NP per lane)
static int passes_of(int D) {
  int np = 1;
  while (np * kPass < D) np *= 2;
  return np;
}

// the centres one seed launch stages: at most `seed_batch` (0: 8), within kSeedLds
static int resolve_seed_batch(int D, int seed_batch) {
  const int room = kSeedLds / (passes_of(D) * kPass * 4);
  int s = seed_batch > 0 ? seed_batch : 8;
  if (s > room) s = room;
  return s < 1 ? 1 : s;
}

// workgroups per group (0: from n and G alone)
static int resolve_blocks(int64_t n, int G, int blocks) {
  if (blocks > 0) return blocks;
  int64_t b = ceil_div(n > 0 ? n : 1, 4 * kWaves);  // at least four rows per wave
  const int64_t cap = kTargetBlocks / G > 1 ? kTargetBlocks / G : 1;
  if (b > cap) b = cap;
  return (int)b;
}

// A row's columns into registers: x[j] = columns 256 j + 4 lane + 0..3, zeros past D.  One 16-byte
// load where the row is 16-byte aligned and the four columns exist, else guarded scalar loads.
template <int NP>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int D, int lane,
                                         float4 (&x)[NP]) {
  const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;  // (the same on every lane)
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int col = j * kPass + 4 * lane;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (aligned && col + 3 < D) {
      v = *reinterpret_cast<const float4*>(p + col);
    } else {
      if (col < D) v.x = p[col];
      if (col + 1 < D) v.y = p[col + 1];
      if (col + 2 < D) v.z = p[col + 2];
      if (col + 3 < D) v.w = p[col + 3];
    }
    x[j] = v;
  }
}

// THE per-pair routine: || x - c ||^2 of a row in registers and a centre staged in LDS
// (zero-padded to NP passes), as the wave's sum; the same value on every lane.
template <int NP>
__device__ __forceinline__ float pair_d2(const float4 (&x)[NP], const float* __restrict__ c,
                                         int lane) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const float4 cv = *reinterpret_cast<const float4*>(c + j * kPass + 4 * lane);
    float d = x[j].x - cv.x;
    s = fmaf(d, d, s);
    d = x[j].y - cv.y;
    s = fmaf(d, d, s);
    d = x[j].z - cv.z;
    s = fmaf(d, d, s);
    d = x[j].w - cv.w;
    s = fmaf(d, d, s);
  }
  return group_sum<kWave>(s);
}

// centre row `src` into LDS `dst` [NP * 256], zeros past D (every thread of the workgroup)
template <int NP>
__device__ __forceinline__ void stage_centre(const float* __restrict__ src, int D,
                                             float* __restrict__ dst) {
  for (int i = threadIdx.x; i < NP * kPass; i += kThreads) dst[i] = i < D ? src[i] : 0.f;
}

__global__ __launch_bounds__(kThreads) void init_kernel(const float* __restrict__ rows, int64_t n,
                                                        int D, float* __restrict__ mind2,
                                                        int* __restrict__ bad) {
  const int lane = threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kWaves + threadIdx.x / kWave;
  if (row >= n) return;  // (a whole wave)
  const bool nonfinite = feat::wave_row_nonfinite(rows + row * (int64_t)D, D, lane);
  if (lane == 0) {
    mind2[row] = INFINITY;
    if (nonfinite) atomicAdd(bad, 1);
  }
}

// The candidate of a row: 0 is "none" (a kept row, or a mind2 that is NaN).  n < 2^31, so
// ~position is never 0 and a candidate at distance 0 still beats "none".
__device__ __forceinline__ unsigned long long candidate(float m, int64_t pos) {
  if (!(m >= 0.f)) return 0ull;
  return ((unsigned long long)__float_as_uint(m) << 32) | (unsigned)~(unsigned)pos;
}

// Seed launch `batch`: workgroup (b, g) folds centres seeds[s0 + batch S .. + S) of group g, whose
// seed list is seeds[seed_off[g] .. seed_off[g + 1]) (positions of rows), into its rows.
template <int NP>
__global__ __launch_bounds__(kThreads) void seed_kernel(
    const float* __restrict__ rows, int D, const int64_t* __restrict__ off,
    const int64_t* __restrict__ seeds, const int64_t* __restrict__ seed_off, int64_t n,
    int batch, int S, float* __restrict__ mind2) {
  extern __shared__ __attribute__((aligned(16))) float s_c[];  // [S][NP * 256]
  __shared__ int64_t s_pos[kMaxSeedBatch];
  const int g = blockIdx.y;
  const int64_t s0 = seed_off[g] + (int64_t)batch * S;
  const int64_t left = seed_off[g + 1] - s0;
  if (left <= 0) return;  // (the whole workgroup: this group's seeds are folded)
  const int cnt = left < S ? (int)left : S;
  const int64_t r0 = off[g] > 0 ? off[g] : 0, r1 = off[g + 1] < n ? off[g + 1] : n;
  if (threadIdx.x < cnt) {
    int64_t p = seeds[s0 + threadIdx.x];
    s_pos[threadIdx.x] = p >= 0 && p < n ? p : -1;  // (a position outside the rows is ignored)
  }
  __syncthreads();
  for (int s = 0; s < cnt; ++s) {
    const int64_t p = s_pos[s];
    if (p >= 0) stage_centre<NP>(rows + p * (int64_t)D, D, s_c + s * NP * kPass);
  }
  __syncthreads();
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int64_t stride = (int64_t)gridDim.x * kWaves;
  for (int64_t r = r0 + (int64_t)blockIdx.x * kWaves + wave; r < r1; r += stride) {
    float m = mind2[r];
    if (m < 0.f) continue;  // kept already (the whole wave)
    float4 x[NP];
    load_row<NP>(rows + r * (int64_t)D, D, lane, x);
    bool kept = false;
    for (int s = 0; s < cnt; ++s) {
      const int64_t p = s_pos[s];
      if (p < 0) continue;
      const float d2 = pair_d2<NP>(x, s_c + s * NP * kPass, lane);
      m = fminf(m, d2);
      kept = kept || p == r;
    }
    if (lane == 0) mind2[r] = kept ? -1.f : m;
  }
}

// Pick launch t (see the head of the file).  slots: [steps][G], zeroed before the first launch.
template <int NP>
__global__ __launch_bounds__(kThreads) void pick_kernel(
    const float* __restrict__ rows, int D, const int64_t* __restrict__ off,
    const int64_t* __restrict__ picks, int64_t n, int t, int64_t steps, int G,
    unsigned long long* __restrict__ slots, float* __restrict__ mind2) {
  __shared__ __attribute__((aligned(16))) float s_c[NP * kPass];
  __shared__ unsigned long long s_best[kWaves];
  const int g = blockIdx.y;
  const int64_t quota = picks[g];
  if (t > quota) return;  // (the whole workgroup: the group has met its quota)
  const int64_t r0 = off[g] > 0 ? off[g] : 0, r1 = off[g + 1] < n ? off[g + 1] : n;
  int64_t cpos = -1;  // the newest centre: the pick of launch t - 1
  if (t > 0) {
    const unsigned long long prev = slots[(int64_t)(t - 1) * G + g];
    if (prev != 0ull) {
      const int64_t p = (int64_t)(unsigned)~(unsigned)(prev & 0xffffffffull);
      if (p >= r0 && p < r1) cpos = p;
    }
  }
  const bool fold = cpos >= 0;     // (the same on every thread)
  const bool publish = t < quota && t < steps;  // (slot [t][g] exists)
  if (!fold && !publish) return;
  if (fold) {
    stage_centre<NP>(rows + cpos * (int64_t)D, D, s_c);
    __syncthreads();
  }
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int64_t stride = (int64_t)gridDim.x * kWaves;
  unsigned long long best = 0ull;
  for (int64_t r = r0 + (int64_t)blockIdx.x * kWaves + wave; r < r1; r += stride) {
    float m = mind2[r];
    if (m < 0.f) continue;  // kept: never a candidate again (the whole wave)
    if (fold) {
      if (r == cpos) {
        m = -1.f;
      } else {
        float4 x[NP];
        load_row<NP>(rows + r * (int64_t)D, D, lane, x);
        m = fminf(m, pair_d2<NP>(x, s_c, lane));
      }
      if (lane == 0) mind2[r] = m;
    }
    const unsigned long long c = candidate(m, r);
    best = c > best ? c : best;
  }
  if (!publish) return;
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) best = s_best[w] > best ? s_best[w] : best;
    // The slot only grows, so a candidate that does not beat the value read here (however
    // stale) cannot win: with many workgroups per group most skip the atomic, which every one
    // of them would otherwise issue on ONE address.  With few per group the extra dependent
    // read costs more than it saves, so they publish directly.
    unsigned long long* slot = &slots[(int64_t)t * G + g];
    if (best != 0ull &&
        (gridDim.x < kCheckBlocks ||
         best > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
      atomicMax(slot, best);
  }
}

__global__ __launch_bounds__(kThreads) void finish_kernel(
    const unsigned long long* __restrict__ slots, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ picks, int64_t n, int64_t steps, int G,
    int64_t* __restrict__ picked, float* __restrict__ radius2) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= steps * G) return;
  const int64_t t = i / G;
  const int g = (int)(i % G);
  const unsigned long long v = slots[i];
  const int64_t p = (int64_t)(unsigned)~(unsigned)(v & 0xffffffffull);
  const bool has = t < picks[g] && v != 0ull && p < n;
  picked[i] = has ? ids[p] : -1;
  radius2[i] = has ? __uint_as_float((unsigned)(v >> 32)) : -1.f;
}

static bool dims_ok(int64_t n, int32_t D, int32_t G, int64_t steps, int64_t max_seeds,
                    int32_t seed_batch, int32_t blocks) {
  return n >= 0 && n < (1ll << 31) && D >= 1 && D <= kMaxD && G >= 1 && G <= kMaxGroups &&
         steps >= 0 && steps <= n && max_seeds >= 0 && max_seeds <= n && seed_batch >= 0 &&
         seed_batch <= kMaxSeedBatch && blocks >= 0 && blocks <= kMaxBlocks;
}

template <int NP>
static void launch(const float* rows, int64_t n, int D, const int64_t* off, int G,
                   const int64_t* seeds, const int64_t* seed_off, int64_t max_seeds,
                   const int64_t* picks, int64_t steps, int S, int blocks,
                   unsigned long long* slots, float* mind2, hipStream_t st) {
  const dim3 grid((unsigned)blocks, (unsigned)G);
  const size_t lds = (size_t)S * NP * kPass * sizeof(float);
  for (int64_t j = 0; j * S < max_seeds; ++j)
    seed_kernel<NP><<<grid, kThreads, lds, st>>>(rows, D, off, seeds, seed_off, n, (int)j, S,
                                                 mind2);
  for (int64_t t = 0; t <= steps; ++t)
    pick_kernel<NP><<<grid, kThreads, 0, st>>>(rows, D, off, picks, n, (int)t, steps, G, slots,
                                              mind2);
}

}  // namespace kcenter
}  // namespace dd

using namespace dd;

extern "C" {

size_t dd_kcenter_workspace_bytes(int64_t n, int32_t D, int32_t G, int64_t steps) {
  if (!kcenter::dims_ok(n, D, G, steps, 0, 0, 0)) return 0;
  return (size_t)kcenter::align256((steps > 0 ? steps : 1) * (int64_t)G * 8);
}

int32_t dd_kcenter_seed_batch(int32_t D, int32_t seed_batch) {
  if (D < 1 || D > kcenter::kMaxD || seed_batch < 0 || seed_batch > kcenter::kMaxSeedBatch)
    return 0;
  return kcenter::resolve_seed_batch(D, seed_batch);
}

int dd_kcenter_greedy(const float* rows, const int64_t* ids, int64_t n, int32_t D,
                      const int64_t* off, int32_t G, const int64_t* seeds,
                      const int64_t* seed_off, int64_t max_seeds, const int64_t* picks,
                      int64_t steps, int32_t seed_batch, int32_t blocks, int64_t* picked,
                      float* radius2, float* mind2, int32_t* bad, void* workspace,
                      size_t workspace_bytes, void* stream) {
  clear_error();
  DD_REQUIRE(kcenter::dims_ok(n, D, G, steps, max_seeds, seed_batch, blocks),
             "dd_kcenter_greedy: need 0 <= n < 2^31, 1 <= D <= %d, 1 <= G <= %d, 0 <= steps, "
             "max_seeds <= n, 0 <= seed_batch <= %d, 0 <= blocks <= %d (n=%lld, D=%d, G=%d, "
             "steps=%lld, max_seeds=%lld, seed_batch=%d, blocks=%d)",
             kcenter::kMaxD, kcenter::kMaxGroups, kcenter::kMaxSeedBatch, kcenter::kMaxBlocks,
             (long long)n, D, G,
             (long long)steps, (long long)max_seeds, seed_batch, blocks);
  if (n == 0) return DD_OK;
  DD_REQUIRE(rows != nullptr && ids != nullptr && off != nullptr && picks != nullptr &&
                 mind2 != nullptr && bad != nullptr,
             "dd_kcenter_greedy: null rows / ids / off / picks / mind2 / bad");
  DD_REQUIRE(max_seeds == 0 || (seeds != nullptr && seed_off != nullptr),
             "dd_kcenter_greedy: null seeds / seed_off with max_seeds > 0");
  DD_REQUIRE(steps == 0 || (picked != nullptr && radius2 != nullptr),
             "dd_kcenter_greedy: null picked / radius2 with steps > 0");
  const size_t need = dd_kcenter_workspace_bytes(n, D, G, steps);
  DD_REQUIRE(workspace != nullptr && workspace_bytes >= need,
             "dd_kcenter_greedy: workspace of %zu bytes, need %zu (dd_kcenter_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, need);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
             "dd_kcenter_greedy: the workspace must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  unsigned long long* slots = static_cast<unsigned long long*>(workspace);
  DD_CHECK_HIP(hipMemsetAsync(slots, 0, need, st), "dd_kcenter_greedy (slots)");
  kcenter::init_kernel<<<(unsigned)ceil_div(n, kcenter::kWaves), kcenter::kThreads, 0, st>>>(
      rows, n, D, mind2, bad);
  const int S = kcenter::resolve_seed_batch(D, seed_batch);
  const int B = kcenter::resolve_blocks(n, G, blocks);
  switch (kcenter::passes_of(D)) {
#define DD_KC_CASE(NP)                                                                         \
  case NP:                                                                                     \
    kcenter::launch<NP>(rows, n, D, off, G, seeds, seed_off, max_seeds, picks, steps, S, B,    \
                        slots, mind2, st);                                                     \
    break;
    DD_KC_CASE(1)
    DD_KC_CASE(2)
    DD_KC_CASE(4)
    DD_KC_CASE(8)
    DD_KC_CASE(16)
#undef DD_KC_CASE
    default:
      set_error("dd_kcenter_greedy: D=%d", D);
      return DD_EINVAL;
  }
  if (steps > 0)
    kcenter::finish_kernel<<<(unsigned)ceil_div(steps * G, kcenter::kThreads), kcenter::kThreads,
                             0, st>>>(slots, ids, picks, n, steps, G, picked, radius2);
  DD_CHECK_LAUNCH("dd_kcenter_greedy");
  return DD_OK;
}

}  // extern "C"
