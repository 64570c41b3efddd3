// Class-conditional Mahalanobis distance with a tied covariance in feature space
// (include/dd_capi.h states the semantics):
//   dd_maha_workspace_bytes  bytes of the workspace either call below needs
//   dd_maha_segment_rows     the rows per segment of the scatter's sum over the rows
//   dd_maha_scatter          S = sum_i a_i a_i^T (D x D float64), a_i = f_i - mu_{y_i}, and the
//                            count of the rows with a non-finite element
//   dd_maha_dist             maha_i = || W a_i ||_2, W lower triangular (the caller's L^-1)
//
// Both on one stream, no allocation, no synchronisation, plain vector stores and one 64-bit
// integer atomic per non-finite row; the split (hi, lo) halves, the 32x32x16 MFMA and the
// fragment layout are dd_mfma.h's and dd_feat.h's.
//
// scatter = A^T A, A the centred rows [n][D]: the MFMA's K dimension is the ROW index i, so a
// fragment is 8 consecutive rows of one column, the transpose of how the rows lie in memory.
//   class    cls_kernel: per row the class to centre by (int32; -1: the class's only row, which
//            is centred to exact zeros; -2: a label outside [0, C), zeros too).
//   tiles    only the nb (nb + 1) / 2 upper-triangular 128 x 128 output tiles (ti <= tj) exist, nb
//            = ceil(D / 128); the rows are cut into segments of dd_maha_segment_rows(n, D) rows.
//            Workgroup (tile, segment), 256 threads, walks its segment 32 rows at a time:
//     stage  thread (col, g) = (tid & 127, tid >> 7) takes column col of each of the tile's two
//            column slabs and the rows 16 p + 8 g .. + 7 (p = 0, 1) of the chunk: 8 fp32 loads
//            down a column (coalesced across the lanes, which run along the columns, so a row
//            needs 4-byte alignment only), minus the class mean gathered by cls, split into
//            halves, packed as two 16-byte pieces and written to LDS as [col][row]: the
//            transpose happens in registers, the LDS reads are whole fragments.  The next
//            chunk's loads are issued before the current chunk's MFMAs.  A diagonal tile stages
//            one slab.  Columns past D and rows past the segment are exact zeros.
//     mfma   wave w owns the 32 rows 32 w .. of the output tile and its four 32-wide column
//            blocks (64 accumulator registers): per 16-row step 2 + 8 fragment reads and the
//            products hi.hi, hi.lo, lo.hi per block.  On a diagonal tile the blocks below the
//            diagonal (b < w) are skipped: the reducer never reads them.
//     out    the fp32 partial tile, [tile][segment][128][128] in the workspace.
//   reduce   reduce_kernel: per element of an upper tile the partials over the segments in
//            ascending order in float64, written to S[k][l] and S[l][k] (a diagonal tile from its
//            k <= l half, so S is exactly symmetric).  The same launch's trailing workgroups scan
//            the rows one per wave and count those with a NaN or an infinity.
//
// dist: rows on the lane, W through LDS (feat::scan_keys' arrangement).
//   pack     the rows, centred and split, [n][Dp] in the workspace (one wave per row), and W's
//            halves (feat::pack_kernel).  The rows' halves cannot stay in LDS: 128 rows x D x 4
//            bytes is 256 KB at D = 512; each lane reads its own row's fragments from the
//            workspace instead, which the output blocks re-read from L2.
//   dist     a 256-thread workgroup owns 128 rows (32 per wave, the row on the lane, both lane
//            halves).  Output block c0 (W's rows c0 .. c0 + 127, the outputs y_j = (W a)_j) takes
//            the K chunks kc = 0, 64, ... < min(Dp, c0 + 128) of W through LDS; the chunks at
//            kc >= c0 + 128 lie wholly above the diagonal (k > j for every j of the block), hold
//            zeros only and are SKIPPED: (nb + 1) / (2 nb) of the MFMA work remains.  After a
//            block each lane adds its 64 outputs squared to one fp32 register in the order a = 0
//            .. 3, i = 0 .. 15; after the last block the two lane halves are added and the square
//            root taken.  W a_i is never written.
//
// Invariance.  Every MFMA output depends on its own row and column alone; the K order is fixed
// (scatter: the rows of a segment ascending, the segments by n and D; dist: by D), so S is a
// function of the rows in their order, and maha_i of row i, its class mean and W: not of the
// tile the row falls in, the buffer's alignment or the launch geometry.
#include "dd_feat.h"

namespace dd {
namespace maha {

using namespace feat;

constexpr int TT = 128;              // output tile edge
constexpr int KR = 32;               // rows per LDS chunk of the scatter: two MFMA steps
constexpr int kPitch = KR * 2 + 16;  // LDS pitch of one column's KR halves (+ 16 B of padding)
constexpr int kSegMin = 256;         // rows per segment, at least
constexpr int kSegMax = 8192;        // ... and at most: (8192 + 2) 2^-24 = 4.9e-4 of sum |a a|
constexpr int kWgTarget = 1024;      // workgroups the segments aim at (4 per CU)
constexpr int64_t kMaxC = 1ll << 20;
constexpr int kReduceWgs = TT * TT / kThreads;  // reducer workgroups per tile

static int64_t tiles_of(int D) {
  const int64_t nb = ceil_div(D, TT);
  return nb * (nb + 1) / 2;
}

// a function of n and D alone; capped, so that the length of an fp32 accumulation (and with it
// S's error bound) does not grow with n: past the cap there are more segments (more workspace)
// and the float64 reducer carries the rest of the sum
static int64_t segment_rows(int64_t n, int D) {
  const int64_t want = kWgTarget / tiles_of(D) > 0 ? kWgTarget / tiles_of(D) : 1;
  const int64_t rows = ceil_div(ceil_div(n, want), KR) * KR;
  return rows < kSegMin ? kSegMin : rows > kSegMax ? kSegMax : rows;
}

struct Layout {
  int Dp;
  int64_t nseg, seg_rows, tiles;
  int64_t cls, partial, scatter_total;        // the scatter's view
  int64_t a_hi, a_lo, w_hi, w_lo, dist_total;  // dist's view
  int64_t total;
};
static Layout layout(int64_t n, int D) {
  Layout L;
  L.Dp = conv::pad_to(D, 16);
  L.tiles = tiles_of(D);
  L.seg_rows = segment_rows(n, D);
  L.nseg = ceil_div(n, L.seg_rows);
  L.cls = 0;
  L.partial = align256(n * 4);
  L.scatter_total = L.partial + L.tiles * L.nseg * TT * TT * 4;
  const int64_t ab = align256(n * L.Dp * 2), wb = align256((int64_t)D * L.Dp * 2);
  L.a_hi = 0;
  L.a_lo = ab;
  L.w_hi = 2 * ab;
  L.w_lo = 2 * ab + wb;
  L.dist_total = 2 * ab + 2 * wb;
  L.total = L.scatter_total > L.dist_total ? L.scatter_total : L.dist_total;
  return L;
}

// the class a row is centred by; -1: its class's only row (centred to zeros), -2: no class
__device__ __forceinline__ int row_class(const int64_t* __restrict__ labels,
                                         const int64_t* __restrict__ counts, int64_t C,
                                         int64_t i) {
  const int64_t y = labels[i];
  if (y < 0 || y >= C) return -2;
  return counts[y] == 1 ? -1 : (int)y;
}

__global__ __launch_bounds__(kThreads) void cls_kernel(const int64_t* __restrict__ labels,
                                                       const int64_t* __restrict__ counts,
                                                       int64_t n, int64_t C,
                                                       int* __restrict__ cls) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) cls[i] = row_class(labels, counts, C, i);
}

// 8 values -> the 16-byte pieces of their hi and lo halves
template <bool F16>
__device__ __forceinline__ void split8(const float (&a)[8], uint4& hi, uint4& lo) {
  bf16x8 h, l;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    __bf16 eh, el;
    conv::split16<F16>(a[e], eh, el);
    h[e] = eh;
    l[e] = el;
  }
  hi = __builtin_bit_cast(uint4, h);
  lo = __builtin_bit_cast(uint4, l);
}

// tile -> (ti, tj), ti <= tj < nb, row by row of the upper triangle
__device__ __forceinline__ void tile_of(int tile, int nb, int& ti, int& tj) {
  ti = 0;
  while (tile >= nb - ti) {
    tile -= nb - ti;
    ++ti;
  }
  tj = ti + tile;
}

template <bool F16>
__global__ __launch_bounds__(kThreads) void scatter_kernel(
    const float* __restrict__ rows, const int* __restrict__ cls, const float* __restrict__ mean,
    int64_t n, int D, int64_t seg_rows, int nseg, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) char lds[2][2][TT * kPitch];  // [slab][hi, lo]
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int r = lane & 31, h = lane >> 5;
  const int tile = blockIdx.x / nseg, seg = blockIdx.x % nseg;
  int ti, tj;
  tile_of(tile, (D + TT - 1) / TT, ti, tj);
  const bool diag = ti == tj;
  const int nslab = diag ? 1 : 2;
  const int64_t r0 = seg * seg_rows;
  const int64_t r1 = r0 + seg_rows < n ? r0 + seg_rows : n;
  const int col = tid & (TT - 1), g = tid >> 7;
  const int dcol[2] = {ti * TT + col, tj * TT + col};

  // one chunk's values of this thread: [slab][p][e], row 16 p + 8 g + e of the chunk
  float fv[2][2][8], mv[2][2][8];
  auto load = [&](int64_t i0) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t i = i0 + 16 * p + 8 * g + e;
        const int c = i < r1 ? cls[i] : -1;  // (uniform over the columns)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bool live = s < nslab && c >= 0 && dcol[s] < D;
          fv[s][p][e] = live ? rows[i * (int64_t)D + dcol[s]] : 0.f;
          mv[s][p][e] = live ? mean[c * (int64_t)D + dcol[s]] : 0.f;
        }
      }
  };

  floatx16 acc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;

  load(r0);
  for (int64_t i0 = r0; i0 < r1; i0 += KR) {
    __syncthreads();  // the previous chunk's fragment reads are done
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s >= nslab) break;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = fv[s][p][e] - mv[s][p][e];  // the one fp32 subtraction
        uint4 hi, lo;
        split8<F16>(a, hi, lo);
        const int off = col * kPitch + (16 * p + 8 * g) * 2;
        *reinterpret_cast<uint4*>(&lds[s][0][off]) = hi;
        *reinterpret_cast<uint4*>(&lds[s][1][off]) = lo;
      }
    }
    __syncthreads();
    if (i0 + KR < r1) load(i0 + KR);  // in flight during the MFMAs below
    const int sb = diag ? 0 : 1;
#pragma unroll
    for (int s = 0; s < KR / 16; ++s) {
      // A[row = column 32 w + r of slab ti][k = rows 16 s + 8 h .. + 7 of the chunk]
      const int aoff = (wave * 32 + r) * kPitch + (16 * s + 8 * h) * 2;
      const bf16x8 fah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(&lds[0][0][aoff]));
      const bf16x8 fal = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(&lds[0][1][aoff]));
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (diag && b < wave) continue;  // below the diagonal: never read
        // B[k = the same rows][col = column 32 b + r of slab tj]
        const int boff = (b * 32 + r) * kPitch + (16 * s + 8 * h) * 2;
        const bf16x8 fbh = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(&lds[sb][0][boff]));
        const bf16x8 fbl = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(&lds[sb][1][boff]));
        acc[b] = conv::mfma16<F16>(fah, fbh, acc[b]);
        acc[b] = conv::mfma16<F16>(fah, fbl, acc[b]);
        acc[b] = conv::mfma16<F16>(fal, fbh, acc[b]);
      }
    }
  }

  // element i of lane (r, h): tile row 32 w + (i & 3) + 8 (i >> 2) + 4 h, tile column 32 b + r
  float* __restrict__ out = partial + ((int64_t)tile * nseg + seg) * (TT * TT);
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int kk = wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      out[kk * TT + b * 32 + r] = acc[b][i];
    }
}

// workgroups [0, tiles * kReduceWgs): the partials' float64 sums; after them: the non-finite rows
__global__ __launch_bounds__(kThreads) void reduce_kernel(
    const float* __restrict__ partial, int nseg, int D, int64_t tile_wgs,
    double* __restrict__ S, const float* __restrict__ rows, int64_t n,
    long long* __restrict__ bad) {
  if ((int64_t)blockIdx.x >= tile_wgs) {
    const int lane = threadIdx.x % kWave;
    const int64_t row = ((int64_t)blockIdx.x - tile_wgs) * kRows + threadIdx.x / kWave;
    if (row >= n) return;  // (a whole wave)
    if (wave_row_nonfinite(rows + row * (int64_t)D, D, lane) && lane == 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(bad), 1ull);
    return;
  }
  const int tile = blockIdx.x / kReduceWgs;
  const int e = (blockIdx.x % kReduceWgs) * kThreads + threadIdx.x;
  const int kk = e / TT, ll = e % TT;
  int ti, tj;
  tile_of(tile, (D + TT - 1) / TT, ti, tj);
  const int k = ti * TT + kk, l = tj * TT + ll;
  if (k >= D || l >= D || (ti == tj && kk > ll)) return;
  const float* __restrict__ p = partial + (int64_t)tile * nseg * (TT * TT) + e;
  double s = 0.0;
  for (int sg = 0; sg < nseg; ++sg) s += (double)p[(int64_t)sg * (TT * TT)];
  S[k * (int64_t)D + l] = s;
  S[l * (int64_t)D + k] = s;
}

// one row per wave: a = f - mu_y (zeros for a class's only row and outside every class) as
// operand halves [n][Dp], the columns past D zero
template <bool F16>
__global__ __launch_bounds__(kThreads) void pack_centred_kernel(
    const float* __restrict__ rows, const int64_t* __restrict__ labels,
    const int64_t* __restrict__ counts, const float* __restrict__ mean, int64_t n, int D, int Dp,
    int64_t C, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
  const int lane = threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / kWave;
  if (row >= n) return;  // (a whole wave)
  const int c = row_class(labels, counts, C, row);
  const float* __restrict__ src = rows + row * (int64_t)D;
  const float* __restrict__ mu = mean + (c >= 0 ? c : 0) * (int64_t)D;
  for (int d = lane; d < Dp; d += kWave) {
    const float a = (c >= 0 && d < D) ? src[d] - mu[d] : 0.f;
    __bf16 h, l;
    conv::split16<F16>(a, h, l);
    hi[row * (int64_t)Dp + d] = __builtin_bit_cast(uint16_t, h);
    lo[row * (int64_t)Dp + d] = __builtin_bit_cast(uint16_t, l);
  }
}

template <bool F16>
__global__ __launch_bounds__(kThreads) void dist_kernel(
    const uint16_t* __restrict__ a_hi, const uint16_t* __restrict__ a_lo,
    const uint16_t* __restrict__ w_hi, const uint16_t* __restrict__ w_lo,
    const int64_t* __restrict__ labels, int64_t n, int D, int Dp, int64_t C,
    float* __restrict__ dist, float* __restrict__ accum) {
  __shared__ __attribute__((aligned(16))) char s_hi[TC * kRowBytes];
  __shared__ __attribute__((aligned(16))) char s_lo[TC * kRowBytes];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int r = lane & 31, h = lane >> 5;
  const int64_t row = (int64_t)blockIdx.x * TQ + wave * 32 + r;  // both lane halves hold it
  const bool valid = row < n;
  const uint16_t* __restrict__ ah_row = a_hi + (valid ? row : 0) * (int64_t)Dp;
  const uint16_t* __restrict__ al_row = a_lo + (valid ? row : 0) * (int64_t)Dp;

  float ssq = 0.f;  // this lane's share of sum_j y_j^2
  for (int c0 = 0; c0 < D; c0 += TC) {
    floatx16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;
    // W[j][k] = 0 for k > j: the chunks at kc >= c0 + 128 are zeros for every row j < c0 + 128
    // of this block and are not visited
    const int kend = Dp < c0 + TC ? Dp : c0 + TC;
    for (int kc = 0; kc < kend; kc += KC) {
      __syncthreads();  // the previous chunk's fragment reads are done
#pragma unroll
      for (int i = 0; i < TC * 8 / kThreads; ++i) {
        const int idx = tid + i * kThreads;
        const int wr = idx >> 3, sg = idx & 7;
        const int j = c0 + wr, kk = kc + sg * 8;
        uint4 vh = make_uint4(0u, 0u, 0u, 0u), vl = vh;
        if (j < D && kk < Dp) {  // W's rows past D and the chunk's tail past Dp are zeros
          vh = *reinterpret_cast<const uint4*>(w_hi + j * (int64_t)Dp + kk);
          vl = *reinterpret_cast<const uint4*>(w_lo + j * (int64_t)Dp + kk);
        }
        *reinterpret_cast<uint4*>(s_hi + wr * kRowBytes + sg * 16) = vh;
        *reinterpret_cast<uint4*>(s_lo + wr * kRowBytes + sg * 16) = vl;
      }
      __syncthreads();
      const int steps = (Dp - kc) / 16 < KC / 16 ? (Dp - kc) / 16 : KC / 16;
      for (int s = 0; s < steps; ++s) {
        const int kk = kc + s * 16 + 8 * h;  // B[k = 8 h + e][col r]: 8 consecutive k of row r
        uint4 bh = make_uint4(0u, 0u, 0u, 0u), bl = bh;
        if (valid) {
          bh = *reinterpret_cast<const uint4*>(ah_row + kk);
          bl = *reinterpret_cast<const uint4*>(al_row + kk);
        }
        const bf16x8 fbh = __builtin_bit_cast(bf16x8, bh), fbl = __builtin_bit_cast(bf16x8, bl);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          // A[row r][k = 8 h + e]: 8 consecutive k of W's row c0 + 32 a + r
          const int off = (a * 32 + r) * kRowBytes + (s * 16 + 8 * h) * 2;
          const bf16x8 fah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(s_hi + off));
          const bf16x8 fal = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(s_lo + off));
          acc[a] = conv::mfma16<F16>(fah, fbh, acc[a]);
          acc[a] = conv::mfma16<F16>(fah, fbl, acc[a]);
          acc[a] = conv::mfma16<F16>(fal, fbh, acc[a]);
        }
      }
    }
    // the outputs c0 + 32 a + (i & 3) + 8 (i >> 2) + 4 h of this lane's row, squared, in the
    // order a, i (outputs past D are exact zeros)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) ssq = fmaf(acc[a][i], acc[a][i], ssq);
  }
  ssq += __shfl_xor(ssq, 32, kWave);  // the other lane half: the row's other outputs
  if (h == 0 && valid) {
    const int64_t y = labels[row];
    const float d = (y < 0 || y >= C) ? __builtin_nanf("") : sqrtf(ssq);
    if (dist) dist[row] = d;
    if (accum) accum[row] += d;
  }
}

static bool dims_ok(const char* what, int64_t n, int32_t D, int64_t C, int32_t operands) {
  if (n < 0 || n >= (1ll << 31)) {
    if (what) set_error("%s: need 0 <= n < 2^31 (n=%lld)", what, (long long)n);
    return false;
  }
  if (!rows_dims_ok(what, 0, 0, D, operands)) return false;
  if (C < 1 || C > kMaxC) {
    if (what) set_error("%s: need 1 <= C <= 2^20 (C=%lld)", what, (long long)C);
    return false;
  }
  return true;
}

template <bool F16>
static void launch_scatter(const float* rows, const int64_t* labels, const int64_t* counts,
                           const float* mean, int64_t n, int D, int64_t C, double* S,
                           long long* bad, char* ws, const Layout& L, hipStream_t st) {
  if (n > 0) {
    cls_kernel<<<(unsigned)ceil_div(n, kThreads), kThreads, 0, st>>>(labels, counts, n, C,
                                                                     at<int>(ws, L.cls));
    scatter_kernel<F16><<<(unsigned)(L.tiles * L.nseg), kThreads, 0, st>>>(
        rows, at<int>(ws, L.cls), mean, n, D, L.seg_rows, (int)L.nseg, at<float>(ws, L.partial));
  }
  const int64_t tile_wgs = L.tiles * kReduceWgs;
  reduce_kernel<<<(unsigned)(tile_wgs + ceil_div(n, kRows)), kThreads, 0, st>>>(
      at<float>(ws, L.partial), (int)L.nseg, D, tile_wgs, S, rows, n, bad);
}

template <bool F16>
static void launch_dist(const float* rows, const int64_t* labels, const int64_t* counts,
                        const float* mean, int64_t n, int D, int64_t C, const float* W,
                        float* dist, float* accum, char* ws, const Layout& L, hipStream_t st) {
  pack_kernel<F16><<<(unsigned)ceil_div(D, kRows), kThreads, 0, st>>>(
      W, D, D, L.Dp, at<uint16_t>(ws, L.w_hi), at<uint16_t>(ws, L.w_lo), nullptr, nullptr);
  pack_centred_kernel<F16><<<(unsigned)ceil_div(n, kRows), kThreads, 0, st>>>(
      rows, labels, counts, mean, n, D, L.Dp, C, at<uint16_t>(ws, L.a_hi),
      at<uint16_t>(ws, L.a_lo));
  dist_kernel<F16><<<(unsigned)ceil_div(n, TQ), kThreads, 0, st>>>(
      at<uint16_t>(ws, L.a_hi), at<uint16_t>(ws, L.a_lo), at<uint16_t>(ws, L.w_hi),
      at<uint16_t>(ws, L.w_lo), labels, n, D, L.Dp, C, dist, accum);
}

}  // namespace maha
}  // namespace dd

using namespace dd;

extern "C" {

size_t dd_maha_workspace_bytes(int64_t n, int32_t D, int32_t operands) {
  if (!maha::dims_ok(nullptr, n, D, 1, operands)) return 0;
  return (size_t)maha::layout(n, D).total;
}

int64_t dd_maha_segment_rows(int64_t n, int32_t D) {
  if (!maha::dims_ok(nullptr, n, D, 1, DD_OPERANDS_F16X3)) return 0;
  return maha::segment_rows(n, D);
}

int dd_maha_scatter(const float* rows, const int64_t* labels, const int64_t* counts,
                    const float* mean, int64_t n, int32_t D, int64_t C, int32_t operands,
                    double* S, int64_t* bad, void* workspace, size_t workspace_bytes,
                    void* stream) {
  clear_error();
  if (!maha::dims_ok("dd_maha_scatter", n, D, C, operands)) return DD_EINVAL;
  DD_REQUIRE(S != nullptr && bad != nullptr, "dd_maha_scatter: null S / bad");
  DD_REQUIRE(n == 0 || (rows != nullptr && labels != nullptr && counts != nullptr &&
                        mean != nullptr),
             "dd_maha_scatter: null rows / labels / counts / mean");
  const maha::Layout L = maha::layout(n, D);
  DD_REQUIRE(n == 0 || (workspace != nullptr && workspace_bytes >= (size_t)L.scatter_total),
             "dd_maha_scatter: workspace of %zu bytes, need %lld (dd_maha_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, (long long)L.scatter_total);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_maha_scatter: the workspace must be 16-byte aligned");
  char* ws = static_cast<char*>(workspace);
  long long* b = reinterpret_cast<long long*>(bad);
  if (operands == DD_OPERANDS_F16X3)
    maha::launch_scatter<true>(rows, labels, counts, mean, n, D, C, S, b, ws, L,
                               as_stream(stream));
  else
    maha::launch_scatter<false>(rows, labels, counts, mean, n, D, C, S, b, ws, L,
                                as_stream(stream));
  DD_CHECK_LAUNCH("dd_maha_scatter");
  return DD_OK;
}

int dd_maha_dist(const float* rows, const int64_t* labels, const int64_t* counts,
                 const float* mean, int64_t n, int32_t D, int64_t C, const float* W,
                 int32_t operands, float* dist, float* accum, void* workspace,
                 size_t workspace_bytes, void* stream) {
  clear_error();
  if (!maha::dims_ok("dd_maha_dist", n, D, C, operands)) return DD_EINVAL;
  DD_REQUIRE(dist != nullptr || accum != nullptr,
             "dd_maha_dist: no output requested (dist and accum both null)");
  if (n == 0) return DD_OK;
  DD_REQUIRE(rows != nullptr && labels != nullptr && counts != nullptr && mean != nullptr &&
                 W != nullptr,
             "dd_maha_dist: null rows / labels / counts / mean / W");
  const maha::Layout L = maha::layout(n, D);
  DD_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)L.dist_total,
             "dd_maha_dist: workspace of %zu bytes, need %lld (dd_maha_workspace_bytes)",
             workspace ? workspace_bytes : (size_t)0, (long long)L.dist_total);
  DD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
             "dd_maha_dist: the workspace must be 16-byte aligned");
  char* ws = static_cast<char*>(workspace);
  if (operands == DD_OPERANDS_F16X3)
    maha::launch_dist<true>(rows, labels, counts, mean, n, D, C, W, dist, accum, ws, L,
                            as_stream(stream));
  else
    maha::launch_dist<false>(rows, labels, counts, mean, n, D, C, W, dist, accum, ws, L,
                             as_stream(stream));
  DD_CHECK_LAUNCH("dd_maha_dist");
  return DD_OK;
}

}  // extern "C"
