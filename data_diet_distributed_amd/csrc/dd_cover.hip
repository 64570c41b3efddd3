// Ball cover over feature rows, inside groups: greedy maximum coverage at a fixed radius, the dual
// of the k-center fill (ProbCover's rule; include/dd_capi.h states the semantics):
//   dd_cover_workspace_bytes  bytes of the workspace of one dd_cover_greedy call (host only)
//   dd_cover_greedy           per group: the distance matrix once, theta from the mean squared
//                             pairwise distance, the matrix thresholded into BITS, the seeds
//                             covered, then `picks[g]` times take the unkept row whose ball holds
//                             the most uncovered rows and cover them
//
// Launches on one stream, no allocation, no synchronisation, nothing read back:
//   pack, layout, matrix  dd_distmat.h: bit for bit the matrices dd_kmedoids_greedy builds.
//   init    the groups' int64 sums = 0, picked = -1, gain = -1, covered = 0.
//   sums, mean, p  dd_groupmean.h: mu and P_i = ||f_i - mu||^2, herding's; P = NaN marks a row
//           that is not valid (counted in `bad`).
//   theta   workgroup g: S = the sum of the valid P_i in float64, thread k its rows k, k + 256, ...
//           in ascending order, then a fixed binary tree over the 256 partial sums: the order is a
//           function of n_g alone.  theta_g = (float)(cover_radius * (2 / n_g) * S); the mean
//           squared distance between two rows of a group is (2 / n_g) sum_i P_i.
//   bits    workgroup (i, g): row i of M, wave v its floats [64 w, 64 w + 64) for w = v, v + 4,
//           ...: one coalesced load, the compare with theta_g, __ballot, one 64-bit store.  The
//           bit is 0 past n_g and where row i or row j is not valid; the diagonal of a valid row
//           is 1.  A group's bits are stored WORD-MAJOR, word w of row i at [w n_g + i], so that
//           the threads of the select kernel, which own consecutive rows, read consecutive words.
//           M is not read again: 1/32 of its bytes from here on.
//   select  ONE launch: workgroup g, 1024 threads, runs group g's whole loop.  Thread k owns rows
//           k, k + 1024, ... (EPT = 1, 4 or 16 by the largest group) and keeps their covered-degree
//           deg and their tie-break key in REGISTERS; LDS holds `uncovered` and `new`, 256 64-bit
//           words each, four words that say which words of `new` are non-zero, and the sixteen
//           waves' candidates twice.  deg_i starts as the popcount of row i against `uncovered`.
//           A pick: the candidate of an unkept valid row is
//               ((deg + 1) << 32) | ((2^14 - 1 - prio) << 14) | position
//           (0: none), the order of (deg << 32) | ~prio with the position carried along: prio is
//           unique in a group, so the position never decides.  The maximum goes through the wave
//           butterfly, one LDS entry per wave and ONE barrier, as in dd_herding.hip.  With a gain
//           of 0 nothing changes but the pick's own key.  Otherwise thread w < W reads word w of
//           the pick's bit row, new[w] = row & uncovered[w], uncovered[w] &= ~row; waves 0..3
//           ballot new[w] != 0; a second barrier; and every thread subtracts
//           popcount(adj_i[w] & new[w]) for the words with new[w] != 0 alone, a loop over the set
//           bits of the four ballots that is uniform over the workgroup.  A bit of `uncovered` is
//           cleared once in a run, so the words walked over all picks are at most
//           min(picks W, n_g): the updates are bounded by what gets covered.  No launch per pick,
//           no host sync, no waiting on another workgroup.
//
// Invariance.  M and P are functions of the group's rows in id order and D alone, mu of the row
// set, S of P in position order with an order n_g fixes, so theta and every bit are too.  After
// the compare everything is integer arithmetic, and pick t is the maximum of a total order
// (prio is unique), so by induction over t the picks, the gains and `covered` are functions of the
// group's rows, prio and the seeds alone: EPT, `blocks`, the other groups and the group's place in
// the call change no output bit.
#include "dd_groupmean.h"

namespace dd {
namespace cover {

using namespace groupmean;

constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / kWave;
constexpr int kMaxEpt = kMaxRows / kSelThreads;
constexpr int kMaxWords = kMaxRows / 64;  // words of a bit row
constexpr int kPosBits = 14;
constexpr unsigned kPosMask = (1u << kPosBits) - 1;
constexpr unsigned kDead = 0xffffffffu;  // the key of a kept row, a row that is not valid, the tail
static_assert(kMaxEpt == 16 && kMaxEpt * kSelThreads == kMaxRows, "16 rows per thread at most");
static_assert(kMaxRows == 1 << kPosBits && kMaxWords == 4 * kWave, "14-bit positions, 4 ballots");

// the workspace: distmat::MatLayout, then the groups' sums, their means, P, theta and the bits
// (n_g W_g words per group, at word moff[g] / 64: a row of M has 64 W_g floats)
struct Layout : MatLayout {
  int64_t sums, mu, p, theta, bits, total;
};
static Layout layout(int64_t n, int D, int G, const int64_t* sizes) {
  Layout L;
  static_cast<MatLayout&>(L) = mat_layout(n, D, G, sizes);
  L.sums = L.mat_end;
  L.mu = L.sums + align256((int64_t)G * D * 8);
  L.p = L.mu + align256((int64_t)G * D * 4);
  L.theta = L.p + align256(n * 4);
  L.bits = L.theta + align256((int64_t)G * 4);
  L.total = L.bits + align256((L.mat_end - L.mat) / 32);  // one bit per float
  return L;
}

__global__ __launch_bounds__(kThreads) void init_kernel(int64_t nsums, int64_t nslots, int G,
                                                        long long* __restrict__ sums,
                                                        int64_t* __restrict__ picked,
                                                        int* __restrict__ gain,
                                                        int64_t* __restrict__ covered) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < nsums) sums[i] = 0;
  if (i < nslots) {
    picked[i] = -1;
    gain[i] = -1;
  }
  if (i < G) covered[i] = 0;
}

// workgroup g: theta_g (see the head of the file); an empty group gets 0
__global__ __launch_bounds__(kThreads) void theta_kernel(const float* __restrict__ P,
                                                         const int64_t* __restrict__ off,
                                                         double radius, float* __restrict__ th_ws,
                                                         float* __restrict__ th_out) {
  __shared__ double s_part[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int64_t r0 = off[g];
  const int ng = (int)(off[g + 1] - r0);
  double s = 0.0;
  for (int i = tid; i < ng; i += kThreads) {
    const float p = P[r0 + i];
    s += p == p ? (double)p : 0.0;
  }
  s_part[tid] = s;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s_part[tid] += s_part[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float th = ng > 0 ? (float)(radius * (2.0 / (double)ng) * s_part[0]) : 0.f;
    th_ws[g] = th;
    th_out[g] = th;
  }
}

// workgroup (i, g): the bit row of row i of group g (see the head of the file).  A row of M has
// pitch = 64 W floats, so every load is inside it; P is read below n_g only.
__global__ __launch_bounds__(kThreads) void bits_kernel(const float* __restrict__ mat,
                                                        const float* __restrict__ P,
                                                        const float* __restrict__ theta,
                                                        const int64_t* __restrict__ off,
                                                        const int64_t* __restrict__ moff,
                                                        unsigned long long* __restrict__ bits) {
  const int g = blockIdx.y, i = blockIdx.x;
  const int64_t r0 = off[g];
  const int ng = (int)(off[g + 1] - r0);
  if (i >= ng) return;  // (the whole workgroup)
  const int W = (ng + 63) / 64;
  const int lane = threadIdx.x % kWave;
  const float* __restrict__ row = mat + moff[g] + (int64_t)i * (W * 64);
  unsigned long long* __restrict__ out = bits + moff[g] / 64;
  const float th = theta[g], pi = P[r0 + i];
  for (int w = threadIdx.x / kWave; w < W; w += kRows) {
    const int j = w * 64 + lane;
    const float d2 = row[j];
    const float pj = j < ng ? P[r0 + j] : __builtin_nanf("");
    const bool set = pi == pi && pj == pj && (d2 <= th || j == i);
    const unsigned long long word = __ballot(set);
    if (lane == 0) out[(int64_t)w * ng + i] = word;
  }
}

// Workgroup g: the whole loop of group g (see the head of the file).
template <int EPT>
__global__ __launch_bounds__(kSelThreads) void select_kernel(
    const unsigned long long* __restrict__ bits, const float* __restrict__ P,
    const int* __restrict__ prio, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ off, const int64_t* __restrict__ moff,
    const int64_t* __restrict__ seeds, const int64_t* __restrict__ seed_off, int64_t max_seeds,
    const int64_t* __restrict__ picks, int64_t steps, int G, int64_t* __restrict__ picked,
    int* __restrict__ gain, int64_t* __restrict__ covered) {
  __shared__ unsigned long long s_unc[kMaxWords], s_new[kMaxWords], s_nz[4];
  __shared__ unsigned long long s_best[2][kSelWaves];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int lane = tid % kWave, wave = tid / kWave;
  const int64_t r0 = off[g], r1 = off[g + 1];
  const int ng = (int)(r1 - r0);
  if (ng <= 0) return;  // (the whole workgroup; covered[g] is 0)
  const int W = (ng + 63) / 64;  // <= 16 EPT: only these words of the LDS arrays are ever used
  const unsigned long long* __restrict__ B = bits + moff[g] / 64;
  const int64_t quota = picks[g] < steps ? picks[g] : steps;

  // uncovered = the valid rows: row e 1024 + 64 wave + lane is bit `lane` of word 16 e + wave
  int deg[EPT];
  unsigned key[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * kSelThreads;
    const float p = i < ng ? P[r0 + i] : __builtin_nanf("");
    const bool valid = p == p;
    key[e] = valid ? ((kPosMask - ((unsigned)prio[r0 + (i < ng ? i : 0)] & kPosMask)) << kPosBits) |
                         (unsigned)i
                   : kDead;
    const unsigned long long word = __ballot(valid);
    if (lane == 0) s_unc[e * kSelWaves + wave] = word;
    deg[e] = 0;
  }
  __syncthreads();
  // deg_i += sign popcount(adj_i[w] & m) for the thread's rows: word w of EPT consecutive runs
  // of 1024 rows, at most eight loads in flight (sixteen 64-bit values would spill at EPT = 16)
  constexpr int CH = EPT < 8 ? EPT : 8;
  auto sweep = [&](int w, unsigned long long m, int sign) {
    const unsigned long long* __restrict__ col = B + (int64_t)w * ng;
#pragma unroll
    for (int e0 = 0; e0 < EPT; e0 += CH) {
      unsigned long long a[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        const int i = tid + (e0 + e) * kSelThreads;
        a[e] = i < ng ? col[i] : 0ull;
      }
#pragma unroll
      for (int e = 0; e < CH; ++e) deg[e0 + e] += sign * __popcll(a[e] & m);
    }
  };
  int nvalid = 0;  // (wave 0 alone uses it)
  for (int w = lane; w < W; w += kWave) nvalid += __popcll(s_unc[w]);
  for (int w = 0; w < W; ++w) sweep(w, s_unc[w], 1);

  // cover(j): the caller has put a barrier between the last read of s_new and this call
  auto cover = [&](int j) {
    if (tid < W) {
      const unsigned long long a = B[(int64_t)tid * ng + j], u = s_unc[tid];
      s_new[tid] = a & u;
      s_unc[tid] = u & ~a;
    }
    if (tid < kMaxWords) {  // waves 0..3, whole
      const unsigned long long nz = __ballot(tid < W && s_new[tid] != 0ull);
      if (lane == 0) s_nz[wave] = nz;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q * kWave >= W) break;
      for (unsigned long long nz = s_nz[q]; nz != 0ull; nz &= nz - 1) {
        const int w = q * kWave + __ffsll((long long)nz) - 1;
        sweep(w, s_new[w], -1);
      }
    }
  };
  auto keep = [&](int j) {
#pragma unroll
    for (int e = 0; e < EPT; ++e)
      if (tid + e * kSelThreads == j) key[e] = kDead;
  };

  const int64_t s0 = seed_off ? seed_off[g] : 0;
  int64_t s1 = seed_off ? seed_off[g + 1] : 0;
  if (s1 - s0 > max_seeds) s1 = s0 + max_seeds;
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t p = seeds[s];
    if (p < r0 || p >= r1) continue;  // (outside the group: ignored)
    __syncthreads();
    cover((int)(p - r0));
    keep((int)(p - r0));
  }

  for (int64_t t = 0; t < quota; ++t) {
    unsigned long long best = 0ull;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const unsigned long long c =
          key[e] == kDead ? 0ull : ((unsigned long long)(unsigned)(deg[e] + 1) << 32) | key[e];
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
    const int j = (int)((unsigned)best & kPosMask);
    const int d = (int)(best >> 32) - 1;
    if (tid == 0) {
      picked[t * G + g] = ids[r0 + j];
      gain[t * G + g] = d;
    }
    if (d > 0) cover(j);  // (uniform; with d = 0 the ball holds no uncovered row)
    keep(j);
  }

  __syncthreads();
  if (wave == 0) {
    for (int w = lane; w < W; w += kWave) nvalid -= __popcll(s_unc[w]);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) nvalid += __shfl_xor(nvalid, o, kWave);
    if (lane == 0) covered[g] = nvalid;
  }
}

struct Args {
  const float* rows;
  const int64_t *ids, *off, *seeds, *seed_off, *picks;
  const int* prio;
  int64_t n, max_seeds, steps;
  int D, G, blocks;
  double radius;
  int64_t* picked;
  int* gain;
  float* theta;
  int64_t* covered;
  int* bad;
};

template <bool F16>
static void launch(const Args& a, char* ws, const Layout& L, hipStream_t st) {
  float *mat = at<float>(ws, L.mat), *mu = at<float>(ws, L.mu), *P = at<float>(ws, L.p);
  float* theta = at<float>(ws, L.theta);
  long long* sums = at<long long>(ws, L.sums);
  unsigned long long* bits = at<unsigned long long>(ws, L.bits);
  const int64_t* moff = at<int64_t>(ws, L.moff);
  const int64_t nsums = (int64_t)a.G * a.D, nslots = a.steps * a.G;
  int64_t ninit = nsums > nslots ? nsums : nslots;
  if (a.G > ninit) ninit = a.G;
  launch_matrices<F16>(a.rows, a.ids, a.off, a.n, a.D, a.G, ws, L, st);
  init_kernel<<<(unsigned)ceil_div(ninit, kThreads), kThreads, 0, st>>>(
      nsums, nslots, a.G, sums, a.picked, a.gain, a.covered);
  if (L.max_rows > 0)
    launch_mean_p(a.rows, a.off, a.D, a.G, L.max_rows, a.blocks, sums, mu, P, a.bad, st);
  theta_kernel<<<(unsigned)a.G, kThreads, 0, st>>>(P, a.off, a.radius, theta, a.theta);
  if (L.max_rows == 0) return;  // every group is empty
  bits_kernel<<<dim3((unsigned)L.max_rows, (unsigned)a.G), kThreads, 0, st>>>(mat, P, theta, a.off,
                                                                              moff, bits);
  auto select = L.max_rows <= kSelThreads       ? &select_kernel<1>
                : L.max_rows <= 4 * kSelThreads ? &select_kernel<4>
                                                : &select_kernel<kMaxEpt>;
  select<<<(unsigned)a.G, kSelThreads, 0, st>>>(bits, P, a.prio, a.ids, a.off, moff, a.seeds,
                                                a.seed_off, a.max_seeds, a.picks, a.steps, a.G,
                                                a.picked, a.gain, a.covered);
}

}  // namespace cover
}  // namespace dd

using namespace dd;

extern "C" {

size_t dd_cover_workspace_bytes(int64_t n, int32_t D, int32_t G, const int64_t* sizes,
                                int64_t steps, int32_t operands) {
  if (!cover::dims_ok(nullptr, n, D, G, sizes, steps, operands)) return 0;
  return (size_t)cover::layout(n, D, G, sizes).total;
}

int dd_cover_greedy(const float* rows, const int64_t* ids, int64_t n, int32_t D,
                    const int64_t* off, const int64_t* sizes, int32_t G, const int64_t* seeds,
                    const int64_t* seed_off, int64_t max_seeds, const int64_t* picks,
                    int64_t steps, int32_t operands, int32_t blocks, double cover_radius,
                    const int32_t* prio, int64_t* picked, int32_t* gain, float* theta,
                    int64_t* covered, int32_t* bad, void* workspace, size_t workspace_bytes,
                    void* stream) {
  clear_error();
  if (!cover::dims_ok("dd_cover_greedy", n, D, G, sizes, steps, operands)) return DD_EINVAL;
  DD_REQUIRE(max_seeds >= 0 && max_seeds <= n && blocks >= 0 && blocks <= cover::kMaxBlocks,
             "dd_cover_greedy: need 0 <= max_seeds <= n, 0 <= blocks <= %d (max_seeds=%lld, "
             "blocks=%d)", cover::kMaxBlocks, (long long)max_seeds, blocks);
  DD_REQUIRE(cover_radius > 0.0 && cover_radius < (double)INFINITY,
             "dd_cover_greedy: cover_radius must be finite and > 0 (got %g)", cover_radius);
  if (n == 0) return DD_OK;
  DD_REQUIRE(rows != nullptr && ids != nullptr && off != nullptr && picks != nullptr &&
                 prio != nullptr && theta != nullptr && covered != nullptr && bad != nullptr,
             "dd_cover_greedy: null rows / ids / off / picks / prio / theta / covered / bad");
  DD_REQUIRE(max_seeds == 0 || (seeds != nullptr && seed_off != nullptr),
             "dd_cover_greedy: null seeds / seed_off with max_seeds > 0");
  DD_REQUIRE(steps == 0 || (picked != nullptr && gain != nullptr),
             "dd_cover_greedy: null picked / gain with steps > 0");
  const cover::Layout L = cover::layout(n, D, G, sizes);
  DD_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)L.total,
             "dd_cover_greedy: workspace of %zu bytes, need %lld (dd_cover_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, (long long)L.total);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_cover_greedy: the workspace must be 16-byte aligned");
  const cover::Args a = {rows, ids, off, max_seeds > 0 ? seeds : nullptr,
                         max_seeds > 0 ? seed_off : nullptr, picks, prio, n, max_seeds, steps, D,
                         G, cover::resolve_blocks(L.max_rows, G, blocks), cover_radius, picked,
                         gain, theta, covered, bad};
  char* ws = static_cast<char*>(workspace);
  if (operands == DD_OPERANDS_F16X3)
    cover::launch<true>(a, ws, L, as_stream(stream));
  else
    cover::launch<false>(a, ws, L, as_stream(stream));
  DD_CHECK_LAUNCH("dd_cover_greedy");
  return DD_OK;
}

}  // extern "C"
