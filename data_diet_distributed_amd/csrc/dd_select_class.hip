// Keep-set selection with per-class quotas: dd_class_counts, dd_select_topk_by_class.
//
// Class c keeps its members at in-class ranks [skip_c, skip_c + quota_c) (score descending, ties
// by ascending index); the kept indices come out in the global order of dd_select_topk.
//
//   order       dd_select_topk with k = n: the full stable descending order (NaN last), int64
//   class_hist  per block over its contiguous chunk of the order: the chunk's class histogram
//               (LDS counters up to 2048 classes, global integer atomics on the block's own row
//               above that); labels outside [0, C) are counted into err
//   class_scan  one thread per class: its row entries become the class's members in the blocks
//               before (an exclusive scan over blocks); a class whose skip + quota exceeds its
//               size is counted into err
//   rank        per block, tile by tile (2048 entries) in order: the tile's (class, position)
//               pairs are sorted in LDS (bitonic; the pairs are distinct), so a class's entries
//               of the tile lie together in order of position; the last entry of each run adds
//               the run's length to the block's running count of the class and the old value is
//               the in-class rank of the run's first entry.  Writes a keep flag per position of
//               the order and the block's number of kept entries
//   compact     stable compaction of the flagged positions (block offsets from the blocks' kept
//               counts), at most k_total entries; a total other than k_total is counted into err
// Nothing is allocated and the host learns no count; the per-call state (block rows, kept
// counts, err) is cleared on the stream first, so a call is reusable and graph-capturable.
// Integer atomics only.
#include "dd_common.h"

#include <algorithm>

namespace dd {
namespace selc {

constexpr int kThreads = 256;
constexpr int kPosBits = 11;
constexpr int kTile = 1 << kPosBits;          // entries ranked per LDS sort
constexpr int kPer = kTile / kThreads;        // consecutive sorted entries per thread
constexpr int kMaxBlocks = 128;               // blocks over the order (one row of C counts each)
constexpr int kLdsClasses = 2048;             // class_hist / class_counts count in LDS up to here
constexpr int64_t kMaxClasses = 1 << 20;      // (class << 11 | position) fits 32 bits
constexpr int64_t kRowWords = 1 << 24;        // nb * C at most (64 MiB of block rows)
constexpr uint32_t kNoClass = (1u << (32 - kPosBits)) - 1;  // bad label / past the chunk's end

struct Layout {
  size_t rows, kept, order, flags, sel, total;
  size_t sel_bytes;
  int nb;
  int64_t per;  // entries per block (whole tiles)
};

static Layout layout(int64_t n, int64_t C) {
  Layout L{};
  const int64_t tiles = std::max<int64_t>(1, ceil_div(n, kTile));
  const int64_t nb = std::min<int64_t>(std::min<int64_t>(tiles, kMaxBlocks),
                                       std::max<int64_t>(1, kRowWords / std::max<int64_t>(C, 1)));
  L.nb = (int)nb;
  L.per = ceil_div(tiles, nb) * kTile;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) / 256 * 256;
    return at;
  };
  L.rows = take((size_t)nb * (size_t)C * 4);  // [rows, order) zeroed per call
  L.kept = take((size_t)nb * 4);
  L.order = take((size_t)n * 8);
  L.flags = take((size_t)n);
  L.sel_bytes = dd_select_workspace_bytes(n);
  L.sel = take(L.sel_bytes);
  L.total = o;
  return L;
}

__device__ __forceinline__ void chunk_of(int64_t n, int64_t per, int64_t& lo, int64_t& hi) {
  lo = (int64_t)blockIdx.x * per;
  hi = lo + per;
  if (lo > n) lo = n;
  if (hi > n) hi = n;
}

// the class of position j of the order, or kNoClass for a label outside [0, C)
__device__ __forceinline__ uint32_t class_at(const int64_t* __restrict__ order,
                                             const int64_t* __restrict__ labels, int64_t j,
                                             int64_t C) {
  const int64_t c = labels[order[j]];
  return (c >= 0 && c < C) ? (uint32_t)c : kNoClass;
}

__global__ __launch_bounds__(kThreads) void clear_kernel(uint4* __restrict__ p, int64_t n16,
                                                         int32_t* err) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n16;
       i += (int64_t)gridDim.x * kThreads)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
  if (blockIdx.x == 0 && threadIdx.x == 0) *err = 0;
}

// add the wave's `bad` counts to *err (one integer atomic per wave that saw any)
__device__ __forceinline__ void report(uint32_t bad, int32_t* err) {
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(err, (int32_t)bad);
}

__global__ __launch_bounds__(kThreads) void class_hist_kernel(
    const int64_t* __restrict__ order, const int64_t* __restrict__ labels, int64_t n, int64_t per,
    int64_t C, uint32_t* __restrict__ rows, int32_t* err) {
  __shared__ uint32_t h[kLdsClasses];
  const int tid = threadIdx.x;
  const bool lds = C <= kLdsClasses;
  uint32_t* row = rows + (size_t)blockIdx.x * (size_t)C;
  if (lds) {
    for (int i = tid; i < (int)C; i += kThreads) h[i] = 0;
    __syncthreads();
  }
  int64_t lo, hi;
  chunk_of(n, per, lo, hi);
  uint32_t bad = 0;
  for (int64_t j = lo + tid; j < hi; j += kThreads) {
    const uint32_t c = class_at(order, labels, j, C);
    if (c == kNoClass) ++bad;
    else atomicAdd(lds ? &h[c] : &row[c], 1u);
  }
  report(bad, err);
  if (lds) {
    __syncthreads();
    for (int i = tid; i < (int)C; i += kThreads) row[i] = h[i];
  }
}

__global__ __launch_bounds__(kThreads) void class_scan_kernel(
    uint32_t* __restrict__ rows, int nb, int64_t C, const int64_t* __restrict__ skip,
    const int64_t* __restrict__ quota, int32_t* err) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  uint32_t bad = 0;
  if (c < C) {
    uint32_t run = 0;
    for (int b = 0; b < nb; ++b) {
      const size_t at = (size_t)b * (size_t)C + (size_t)c;
      const uint32_t v = rows[at];
      rows[at] = run;
      run += v;
    }
    const int64_t s = skip[c], q = quota[c];
    bad = s < 0 || q < 0 || s > (int64_t)run || q > (int64_t)run - s;
  }
  report(bad, err);
}

// exclusive maximum over the threads before this one (thread order); `red` holds kThreads / 64
// words; -1 where there is none
__device__ __forceinline__ int block_excl_max(int v, int* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(s, o);
    if (lane >= o) s = max(s, t);
  }
  if (lane == 63) red[wv] = s;
  int e = __shfl_up(s, 1);
  if (lane == 0) e = -1;
  __syncthreads();
  for (int w = 0; w < kThreads / 64; ++w)
    if (w < wv) e = max(e, red[w]);
  return e;
}

__global__ __launch_bounds__(kThreads) void rank_kernel(
    const int64_t* __restrict__ order, const int64_t* __restrict__ labels, int64_t n, int64_t per,
    int64_t C, const int64_t* __restrict__ skip, const int64_t* __restrict__ quota,
    uint32_t* __restrict__ rows, uint8_t* __restrict__ flags, uint32_t* __restrict__ kept) {
  __shared__ uint32_t sk[kTile];     // (class << 11 | position in the tile), sorted
  __shared__ uint32_t sbase[kTile];  // at a run's first entry: the in-class rank of that entry
  __shared__ int red[kThreads / 64];
  __shared__ uint32_t s_kept;
  const int tid = threadIdx.x;
  uint32_t* row = rows + (size_t)blockIdx.x * (size_t)C;
  if (tid == 0) s_kept = 0;
  int64_t lo, hi;
  chunk_of(n, per, lo, hi);
  for (int64_t t0 = lo; t0 < hi; t0 += kTile) {
    for (int p = tid; p < kTile; p += kThreads) {
      const int64_t j = t0 + p;
      const uint32_t c = j < hi ? class_at(order, labels, j, C) : kNoClass;
      sk[p] = (c << kPosBits) | (uint32_t)p;
    }
    __syncthreads();
    for (int k = 2; k <= kTile; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < kTile / 2; t += kThreads) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int l = i | j;
          const uint32_t a = sk[i], b = sk[l];
          if ((a > b) == ((i & k) == 0)) {
            sk[i] = b;
            sk[l] = a;
          }
        }
        __syncthreads();
      }
    }
    // this thread's sorted entries [i0, i0 + kPer): the first entry of each one's run
    const int i0 = tid * kPer;
    uint32_t key[kPer];
    int head[kPer];
    uint32_t prev = i0 ? sk[i0 - 1] >> kPosBits : 0u;
    const uint32_t next = i0 + kPer < kTile ? sk[i0 + kPer] >> kPosBits : 0u;
    int h = -1;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      key[e] = sk[i0 + e];
      const uint32_t c = key[e] >> kPosBits;
      if (i0 + e == 0 || c != prev) h = i0 + e;
      head[e] = h;
      prev = c;
    }
    const int before = block_excl_max(h, red);  // (entry 0 is a head: defined wherever needed)
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      if (head[e] < 0) head[e] = before;
      const uint32_t c = key[e] >> kPosBits;
      const uint32_t cn = e + 1 < kPer ? key[(e + 1) % kPer] >> kPosBits : next;
      const bool tail = i0 + e == kTile - 1 || cn != c;
      if (tail && c != kNoClass)
        sbase[head[e]] = atomicAdd(&row[c], (uint32_t)(i0 + e - head[e] + 1));
    }
    __syncthreads();
    uint32_t mine = 0;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const uint32_t c = key[e] >> kPosBits;
      const int64_t j = t0 + (int64_t)(key[e] & (kTile - 1));
      if (j < hi) {
        bool f = false;
        if (c != kNoClass) {
          const int64_t r = (int64_t)sbase[head[e]] + (i0 + e - head[e]);
          const int64_t s = skip[c], q = quota[c];
          f = r >= s && r - s < q;
        }
        flags[j] = f;
        mine += f;
      }
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((tid & 63) == 0 && mine) atomicAdd(&s_kept, mine);
    __syncthreads();  // sk / sbase are rewritten by the next tile
  }
  __syncthreads();
  if (tid == 0) kept[blockIdx.x] = s_kept;
}

__global__ __launch_bounds__(kThreads) void compact_kernel(
    const int64_t* __restrict__ order, const uint8_t* __restrict__ flags, int64_t n, int64_t per,
    const uint32_t* __restrict__ kept, int64_t k_total, int64_t* __restrict__ out, int32_t* err) {
  __shared__ uint32_t wc[2][kThreads / 64];
  __shared__ uint32_t s_base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (wv == 0) {
    uint32_t s = 0;
    for (int i = lane; i < (int)blockIdx.x; i += 64) s += kept[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) s_base = s;
  }
  __syncthreads();
  int64_t run = s_base;
  int64_t lo, hi;
  chunk_of(n, per, lo, hi);
  int par = 0;
  for (int64_t b0 = lo; b0 < hi; b0 += kThreads, par ^= 1) {  // workgroup-uniform
    const int64_t j = b0 + tid;
    const bool f = j < hi && flags[j];
    const uint64_t bs = __ballot(f);
    if (lane == 0) wc[par][wv] = (uint32_t)__popcll(bs);
    __syncthreads();  // (double-buffered counts: one barrier per round)
    int64_t p = run + __popcll(bs & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      const uint32_t c = wc[par][w];
      if (w < wv) p += c;
      run += c;
    }
    if (f && p < k_total) out[p] = order[j];
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0 && run != k_total) atomicAdd(err, 1);
}

// ---- dd_class_counts ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void counts_clear_kernel(int64_t* __restrict__ counts,
                                                                int64_t C, int32_t* bad) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < C;
       i += (int64_t)gridDim.x * kThreads)
    counts[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *bad = 0;
}

__global__ __launch_bounds__(kThreads) void counts_kernel(const int64_t* __restrict__ labels,
                                                          int64_t n, int64_t C,
                                                          int64_t* __restrict__ counts,
                                                          int32_t* bad_out) {
  __shared__ uint32_t h[kLdsClasses];
  const int tid = threadIdx.x;
  const bool lds = C <= kLdsClasses;
  auto* out = reinterpret_cast<unsigned long long*>(counts);
  if (lds) {
    for (int i = tid; i < (int)C; i += kThreads) h[i] = 0;
    __syncthreads();
  }
  uint32_t bad = 0;
  for (int64_t j = (int64_t)blockIdx.x * kThreads + tid; j < n;
       j += (int64_t)gridDim.x * kThreads) {
    const int64_t c = labels[j];
    if (c < 0 || c >= C) ++bad;
    else if (lds) atomicAdd(&h[c], 1u);
    else atomicAdd(&out[c], 1ull);
  }
  report(bad, bad_out);
  if (lds) {
    __syncthreads();
    for (int i = tid; i < (int)C; i += kThreads)
      if (h[i]) atomicAdd(&out[i], (unsigned long long)h[i]);
  }
}

}  // namespace selc
}  // namespace dd

using namespace dd;

extern "C" {

int dd_class_counts(const int64_t* labels, int64_t n, int64_t num_classes, int64_t* counts_out,
                    int32_t* bad_label_out, void* stream) {
  clear_error();
  DD_REQUIRE(n >= 0 && n < (1ll << 31), "dd_class_counts: need 0 <= n < 2^31 (n=%lld)",
             (long long)n);
  DD_REQUIRE(num_classes >= 1 && num_classes < (1ll << 31),
             "dd_class_counts: need 1 <= num_classes < 2^31 (got %lld)", (long long)num_classes);
  DD_REQUIRE(counts_out != nullptr && bad_label_out != nullptr,
             "dd_class_counts: null counts_out / bad_label_out");
  DD_REQUIRE(n == 0 || labels != nullptr, "dd_class_counts: null labels");
  hipStream_t s = as_stream(stream);
  selc::counts_clear_kernel<<<(unsigned)std::min<int64_t>(ceil_div(num_classes, selc::kThreads),
                                                          1024),
                              selc::kThreads, 0, s>>>(counts_out, num_classes, bad_label_out);
  DD_CHECK_LAUNCH("dd_class_counts(clear)");
  if (n == 0) return DD_OK;
  const unsigned nb = (unsigned)std::min<int64_t>(ceil_div(n, 16 * selc::kThreads), 256);
  selc::counts_kernel<<<nb, selc::kThreads, 0, s>>>(labels, n, num_classes, counts_out,
                                                    bad_label_out);
  DD_CHECK_LAUNCH("dd_class_counts");
  return DD_OK;
}

size_t dd_select_by_class_workspace_bytes(int64_t n, int64_t num_classes) {
  if (n < 0 || n >= (1ll << 31) || num_classes < 1 || num_classes > selc::kMaxClasses) return 0;
  return selc::layout(n, num_classes).total;
}

int dd_select_topk_by_class(const float* keys, const int64_t* labels, int64_t n,
                            int64_t num_classes, const int64_t* skip, const int64_t* quota,
                            int64_t k_total, int64_t* idx_out, int32_t* nan_count_out,
                            int32_t* err_out, void* workspace, size_t workspace_bytes,
                            void* stream) {
  clear_error();
  DD_REQUIRE(n >= 0 && k_total >= 0 && k_total <= n,
             "dd_select_topk_by_class: need 0 <= k_total <= n (k_total=%lld n=%lld)",
             (long long)k_total, (long long)n);
  DD_REQUIRE(n < (1ll << 31), "dd_select_topk_by_class: n >= 2^31 unsupported");
  DD_REQUIRE(num_classes >= 1 && num_classes <= selc::kMaxClasses,
             "dd_select_topk_by_class: need 1 <= num_classes <= 2^20 (got %lld)",
             (long long)num_classes);
  DD_REQUIRE(skip != nullptr && quota != nullptr && err_out != nullptr,
             "dd_select_topk_by_class: null skip / quota / err_out");
  DD_REQUIRE(n == 0 || (keys != nullptr && labels != nullptr),
             "dd_select_topk_by_class: null keys / labels");
  DD_REQUIRE(k_total == 0 || idx_out != nullptr, "dd_select_topk_by_class: null idx_out");
  const selc::Layout L = selc::layout(n, num_classes);
  if (!workspace || workspace_bytes < L.total) {
    set_error("dd_select_topk_by_class: workspace %zu < %zu bytes", workspace_bytes, L.total);
    return DD_EWORKSPACE;
  }
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_select_topk_by_class: workspace must be 16-byte aligned");
  hipStream_t s = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  auto* rows = reinterpret_cast<uint32_t*>(ws + L.rows);
  auto* kept = reinterpret_cast<uint32_t*>(ws + L.kept);
  auto* order = reinterpret_cast<int64_t*>(ws + L.order);
  auto* flags = reinterpret_cast<uint8_t*>(ws + L.flags);
  const int64_t n16 = (int64_t)((L.order - L.rows) / 16);
  selc::clear_kernel<<<(unsigned)std::min<int64_t>(ceil_div(n16, selc::kThreads), 2048),
                       selc::kThreads, 0, s>>>(reinterpret_cast<uint4*>(ws + L.rows), n16,
                                               err_out);
  DD_CHECK_LAUNCH("dd_select_topk_by_class(clear)");
  const int rc = dd_select_topk(keys, n, n, order, nullptr, nan_count_out, ws + L.sel,
                                L.sel_bytes, stream);
  if (rc != DD_OK) return rc;
  selc::class_hist_kernel<<<L.nb, selc::kThreads, 0, s>>>(order, labels, n, L.per, num_classes,
                                                          rows, err_out);
  selc::class_scan_kernel<<<(unsigned)ceil_div(num_classes, selc::kThreads), selc::kThreads, 0,
                            s>>>(rows, L.nb, num_classes, skip, quota, err_out);
  selc::rank_kernel<<<L.nb, selc::kThreads, 0, s>>>(order, labels, n, L.per, num_classes, skip,
                                                    quota, rows, flags, kept);
  selc::compact_kernel<<<L.nb, selc::kThreads, 0, s>>>(order, flags, n, L.per, kept, k_total,
                                                       idx_out, err_out);
  DD_CHECK_LAUNCH("dd_select_topk_by_class");
  return DD_OK;
}

}  // extern "C"
