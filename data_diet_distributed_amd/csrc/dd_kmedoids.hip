// Greedy k-medoids (the facility-location / inertia greedy) over feature rows, inside groups
// (include/dd_capi.h states the semantics):
//   dd_kmedoids_workspace_bytes  bytes of the workspace of one dd_kmedoids_greedy call (host only)
//   dd_kmedoids_greedy           per group: the distance matrix once, the seeds folded into cur,
//                                then `picks[g]` times take the row whose addition lowers
//                                sum_i cur_i the most and fold it in
//
// Launches on one stream, no allocation, no synchronisation, nothing read back:
//   pack    feat::pack_kernel on the group-sorted rows: operand halves and ||f||^2 (NaN marks a
//           non-finite row).
//   layout  one workgroup: moff[g], the float offset of group g's matrix, from `off`.
//   init    cur (both buffers and the caller's) = +inf, the slots = 0, the NaN norms counted.
//   matrix  once per call.  Workgroup (x, g) takes 128 points of group g against a range of its
//           centres, 128 at a time, through feat::scan_keys: THE key, so its invariance argument
//           stays in dd_feat.h.  The scan leaves the POINT on the lane, so the epilogue stores
//           M[c][.] with consecutive lanes on consecutive points: 128-byte runs per half wave.
//           Rows are pitched to a multiple of 64 floats, the tail past n_g holds +0 and the
//           diagonal is forced to 0.  Only rows M[c][.] are ever read afterwards (by the seed
//           fold, the pick fold and the gain alike): one source of every distance, and the matrix
//           need not be symmetric (it is not, bit for bit: the second and third split products
//           swap with the operands).
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
#include "dd_feat.h"

namespace dd {
namespace kmedoids {

using namespace feat;

constexpr int kWaves = kThreads / kWave;
constexpr int kMaxRows = DD_KMEDOIDS_MAX_GROUP_ROWS;
constexpr int kMaxSeedBatch = DD_KCENTER_MAX_SEED_BATCH;
constexpr int kMaxBlocks = DD_KCENTER_MAX_BLOCKS;
constexpr int kMaxGroups = DD_KCENTER_MAX_GROUPS;
constexpr int kTargetBlocks = 1024;  // workgroups of one launch the automatic count aims at
constexpr int kCheckBlocks = 256;    // workgroups per group from which the slot is read first
constexpr int kGainUnroll = 8;       // matrix loads a lane has in flight

__host__ __device__ constexpr int64_t pitch_of(int64_t ng) { return (ng + 63) / 64 * 64; }

// workgroups per group of the seed and pick launches (0: from the largest group and G alone)
static int resolve_blocks(int64_t max_rows, int G, int blocks) {
  if (blocks > 0) return blocks;
  int64_t b = ceil_div(max_rows > 0 ? max_rows : 1, 4 * kWaves);  // at least four rows per wave
  const int64_t cap = kTargetBlocks / G > 1 ? kTargetBlocks / G : 1;
  if (b > cap) b = cap;
  return (int)b;
}

// the workspace: feat::PackLayout with no queries (the rows are points and centres at once: the
// "candidate" halves and norms serve both), then the matrices' offsets, the matrices, the two cur
// buffers and the slots
struct Layout : PackLayout {
  int64_t moff, mat, cur, slots, total;
  int64_t max_rows;
};
static Layout layout(int64_t n, int D, int G, const int64_t* sizes, int64_t steps) {
  Layout L;
  static_cast<PackLayout&>(L) = pack_layout(0, n, D);
  int64_t floats = 0;
  L.max_rows = 0;
  for (int g = 0; g < G; ++g) {
    floats += sizes[g] * pitch_of(sizes[g]);
    if (sizes[g] > L.max_rows) L.max_rows = sizes[g];
  }
  L.moff = L.end;
  L.mat = L.moff + align256(((int64_t)G + 1) * 8);
  L.cur = L.mat + align256(floats * 4);
  L.slots = L.cur + align256(2 * n * 4);
  L.total = L.slots + align256((steps > 0 ? steps : 1) * (int64_t)G * 8);
  return L;
}

// `what` null: no error text (dd_kmedoids_workspace_bytes answers 0)
static bool dims_ok(const char* what, int64_t n, int32_t D, int32_t G, const int64_t* sizes,
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
// consecutive groups, thread 0 scans the 256 partial sums)
__global__ __launch_bounds__(kThreads) void layout_kernel(const int64_t* __restrict__ off, int G,
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
  uint16_t *hi = at<uint16_t>(ws, L.c_hi), *lo = at<uint16_t>(ws, L.c_lo);
  float *norm = at<float>(ws, L.c_norm), *mat = at<float>(ws, L.mat), *buf = at<float>(ws, L.cur);
  int64_t* moff = at<int64_t>(ws, L.moff);
  unsigned long long* slots = at<unsigned long long>(ws, L.slots);
  const int64_t nslots = a.steps * a.G;
  pack_kernel<F16><<<(unsigned)ceil_div(a.n, kRows), kThreads, 0, st>>>(a.rows, a.n, a.D, L.Dp, hi,
                                                                        lo, norm, nullptr);
  layout_kernel<<<1, kThreads, 0, st>>>(a.off, a.G, moff);
  init_kernel<<<(unsigned)ceil_div(a.n > nslots ? a.n : nslots, kThreads), kThreads, 0, st>>>(
      norm, a.n, nslots, a.cur, buf, slots, a.bad);
  if (L.max_rows == 0) return;  // every group is empty
  // the matrix: 128-point tiles of the largest group, the centres split until the launch has
  // about kTargetBlocks workgroups (smaller groups leave at once where they have no tile)
  const int tiles = (int)ceil_div(L.max_rows, TQ);
  int csplit = (int)ceil_div(kTargetBlocks, (int64_t)tiles * a.G);
  if (csplit > tiles) csplit = tiles;
  matrix_kernel<F16><<<dim3((unsigned)(tiles * csplit), (unsigned)a.G), kThreads, 0, st>>>(
      hi, lo, norm, a.ids, a.off, moff, L.Dp, csplit, mat);
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
