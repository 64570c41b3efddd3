// The feature-space scores' shared definitions (dd_nn.hip, dd_knn.hip, dd_proto.hip,
// dd_kcenter.hip): every step whose arithmetic order the scores' bitwise claims rest on is
// written here and nowhere else.
//   pack_kernel      a fp32 row -> operand halves (hi, lo; 16-bit, D zero-padded to a multiple of
//                    16), ||row||^2 in fp32 for the candidates (NaN marks a non-finite row: its
//                    keys are NaN and a NaN key never wins)
//   scan_keys        key(q, c) = ||c||^2 - 2 q.c of 128 queries against a candidate range, 128
//                    candidates at a time, q.c = hi.hi + hi.lo + lo.hi on 32x32x16 MFMAs; each key
//                    goes to the caller's epilogue (nn: a running minimum; knn: a sorted list)
//   wave_row_sqdist  one wave's fp32 sum (x[d] - y[d])^2 from the fp32 rows: the VALUE of every
//                    distance.  The MFMA rounding decides which row is picked, never the value: an
//                    exact duplicate scores exactly 0.
//
// Invariance.  A key is a function of the two rows and D alone:
//   * the K order is fixed by D: chunks of 64 ascending, steps of 16 ascending within a chunk,
//     and per step the three products in the order hi.hi, hi.lo, lo.hi;
//   * a 32x32x16 MFMA computes every output element from its own row and column only, so which
//     other queries and candidates share the tile changes nothing;
//   * ragged rows and the K tail past Dp are zero-filled, and a zero product adds exactly 0;
//   * ||c||^2 and the row reducer add in one order: lane l takes columns l, l + 64, ... ascending
//     in one fmaf chain, then the fixed butterfly.
// So a key does not depend on the batching of the queries, on nq or nc, on positions, on how the
// candidates are split into ranges, or on the launch geometry; what a caller selects from the
// keys under a total order of (key, id) is then as independent (see each caller).
#pragma once
#include "dd_mfma.h"

#include <math.h>

namespace dd {
namespace feat {

using conv::bf16x8;
using conv::floatx16;

constexpr int kThreads = 256;
constexpr int kRows = kThreads / kWave;  // rows per workgroup of the one-wave-per-row kernels
constexpr int kMaxD = 4096;              // dd_linear_forward's bound
constexpr int TQ = 128;                  // queries per workgroup (32 per wave)
constexpr int TC = 128;                  // candidates per step
constexpr int KC = 64;                   // K elements per LDS chunk
constexpr int kRowBytes = KC * 2 + 16;   // LDS row pitch: 16 B of padding against bank conflicts
constexpr int64_t kNoId = INT64_MAX;

__host__ __device__ constexpr int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

__device__ __forceinline__ int64_t shfl_xor64(int64_t v, int mask) {
  const unsigned hi = (unsigned)__shfl_xor((int)(v >> 32), mask, kWave);
  const unsigned lo = (unsigned)__shfl_xor((int)(v & 0xffffffffll), mask, kWave);
  return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// the range checks every rows-against-rows call shares; `what` null: no error text (the
// *_workspace_bytes entry points answer 0)
inline bool rows_dims_ok(const char* what, int64_t nq, int64_t nc, int32_t D, int32_t operands) {
  if (nq < 0 || nq >= (1ll << 31) || nc < 0 || nc >= (1ll << 31)) {
    if (what)
      set_error("%s: need 0 <= nq, nc < 2^31 (nq=%lld, nc=%lld)", what, (long long)nq,
                (long long)nc);
    return false;
  }
  if (D < 1 || D > kMaxD) {
    if (what) set_error("%s: need 1 <= D <= %d (D=%d)", what, kMaxD, D);
    return false;
  }
  if (operands != DD_OPERANDS_F16X3 && operands != DD_OPERANDS_BF16X3) {
    if (what)
      set_error("%s: operands must be DD_OPERANDS_BF16X3 or DD_OPERANDS_F16X3 (got %d)", what,
                operands);
    return false;
  }
  return true;
}

// the head of a workspace: [c hi][c lo][q hi][q lo] 16-bit [rows][Dp], [||c||^2] fp32 [nc]; a
// caller's own buffers start at `end`
struct PackLayout {
  int Dp;
  int64_t c_hi, c_lo, q_hi, q_lo, c_norm, end;
};
inline PackLayout pack_layout(int64_t nq, int64_t nc, int D) {
  PackLayout L;
  L.Dp = conv::pad_to(D, 16);
  const int64_t cb = align256(nc * L.Dp * 2), qb = align256(nq * L.Dp * 2);
  L.c_hi = 0;
  L.c_lo = cb;
  L.q_hi = 2 * cb;
  L.q_lo = 2 * cb + qb;
  L.c_norm = 2 * cb + 2 * qb;
  L.end = L.c_norm + align256(nc * 4);
  return L;
}
// the buffer at byte `off` of the workspace
template <typename T>
inline T* at(char* ws, int64_t off) {
  return reinterpret_cast<T*>(ws + off);
}

// The fp32 sum of (x[d] - y[d])^2 over a row, the same value on every lane of the wave that owns
// the row (`has` false: y is not read and the sum is 0).  *nonfinite (may be null): x holds a NaN
// or an infinity.
__device__ __forceinline__ float wave_row_sqdist(const float* __restrict__ x,
                                                 const float* __restrict__ y, int D, int lane,
                                                 bool has, bool* nonfinite) {
  float s = 0.f, nf = 0.f;
  for (int d = lane; d < D; d += kWave) {
    const float v = x[d];
    const float diff = has ? v - y[d] : 0.f;
    s = fmaf(diff, diff, s);
    nf = fabsf(v) < INFINITY ? nf : 1.f;  // NaN or +-inf
  }
  if (nonfinite) *nonfinite = group_max<kWave>(nf) != 0.f;
  return group_sum<kWave>(s);
}

// x holds a NaN or an infinity (the same answer on every lane of the wave that owns the row)
__device__ __forceinline__ bool wave_row_nonfinite(const float* __restrict__ x, int D, int lane) {
  float nf = 0.f;
  for (int d = lane; d < D; d += kWave) nf = fabsf(x[d]) < INFINITY ? nf : 1.f;
  return group_max<kWave>(nf) != 0.f;
}

// one row per wave; norm (candidates) and pick (nn's queries: -1, "no pick yet") may be null
template <bool F16>
__global__ __launch_bounds__(kThreads) void pack_kernel(
    const float* __restrict__ x, int64_t n, int D, int Dp, uint16_t* __restrict__ hi,
    uint16_t* __restrict__ lo, float* __restrict__ norm, int* __restrict__ pick) {
  const int lane = threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / kWave;
  if (row >= n) return;  // (a whole wave)
  const float* __restrict__ src = x + row * (int64_t)D;
  uint16_t* __restrict__ oh = hi + row * (int64_t)Dp;
  uint16_t* __restrict__ ol = lo + row * (int64_t)Dp;
  float s = 0.f, nf = 0.f;
  for (int d = lane; d < Dp; d += kWave) {
    const float v = d < D ? src[d] : 0.f;
    s = fmaf(v, v, s);
    nf = fabsf(v) < INFINITY ? nf : 1.f;  // NaN or +-inf
    __bf16 h, l;
    conv::split16<F16>(v, h, l);
    oh[d] = __builtin_bit_cast(uint16_t, h);
    ol[d] = __builtin_bit_cast(uint16_t, l);
  }
  s = group_sum<kWave>(s);
  nf = group_max<kWave>(nf);
  if (lane == 0) {
    if (norm) norm[row] = nf != 0.f ? __builtin_nanf("") : s;
    if (pick) pick[row] = -1;  // rows outside every segment keep it
  }
}

// every row of the call is split exactly once: the candidates (with their norms), then the queries
template <bool F16>
inline void launch_pack(const float* q, int64_t nq, const float* c, int64_t nc, int D, char* ws,
                        const PackLayout& L, int* pick, hipStream_t st) {
  if (nc > 0)
    pack_kernel<F16><<<(unsigned)ceil_div(nc, kRows), kThreads, 0, st>>>(
        c, nc, D, L.Dp, at<uint16_t>(ws, L.c_hi), at<uint16_t>(ws, L.c_lo),
        at<float>(ws, L.c_norm), nullptr);
  pack_kernel<F16><<<(unsigned)ceil_div(nq, kRows), kThreads, 0, st>>>(
      q, nq, D, L.Dp, at<uint16_t>(ws, L.q_hi), at<uint16_t>(ws, L.q_lo), nullptr, pick);
}

// what scan_keys stages per 128-candidate step (38 400 bytes): a 64-wide K chunk of the halves,
// and the candidates' norms and ids (NaN and kNoId for the rows past the range)
struct __attribute__((aligned(16))) ScanLds {
  char hi[TC * kRowBytes];
  char lo[TC * kRowBytes];
  int64_t id[TC];
  float norm[TC];
};

// The keys of this workgroup's 128 queries against the candidates [cs, ce), by all 256 threads
// (cs, ce and Dp uniform).  Wave w owns queries 32 w .. 32 w + 31: lane (r, h) = (lane & 31,
// lane >> 5) passes the packed halves of ITS query 32 w + r (qvalid false: it has none, and zeros
// are used).  The candidate halves go through LDS (shared by the four waves) as the A operand, the
// queries are the B operand, so the 32x32 accumulator has the query on the lane and 16 candidates
// in the registers.  After each step the epilogue runs once per accumulator element,
//   epi(key, lr, c0)   the key of candidate c0 + lr, lr = 32 a + (i & 3) + 8 (i >> 2) + 4 h,
// for a = 0..3, i = 0..15 in that order; lds.id[lr] is that candidate's id (the epilogue reads it
// when it needs it).  A candidate past ce has a NaN key.  Each lane half sees half of the
// candidates of its query: the caller combines the two.
template <bool F16, int EPI_UNROLL = 16, typename Epi>
__device__ __forceinline__ void scan_keys(ScanLds& lds, const uint16_t* __restrict__ qh_row,
                                          const uint16_t* __restrict__ ql_row, bool qvalid,
                                          const uint16_t* __restrict__ c_hi,
                                          const uint16_t* __restrict__ c_lo,
                                          const float* __restrict__ c_norm,
                                          const int64_t* __restrict__ c_id, int64_t cs, int64_t ce,
                                          int Dp, Epi&& epi) {
  const int tid = threadIdx.x;
  const int lane = tid % kWave;
  const int r = lane & 31, h = lane >> 5;
  for (int64_t c0 = cs; c0 < ce; c0 += TC) {
    floatx16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;

    for (int kc = 0; kc < Dp; kc += KC) {
      __syncthreads();  // the previous chunk's reads and the previous step's epilogue are done
      if (kc == 0 && tid < TC) {
        const int64_t j = c0 + tid;
        lds.norm[tid] = j < ce ? c_norm[j] : __builtin_nanf("");
        lds.id[tid] = j < ce ? c_id[j] : kNoId;
      }
      // TC rows x 8 pieces of 8 halves per operand half: 4 pieces per thread and half
#pragma unroll
      for (int i = 0; i < TC * 8 / kThreads; ++i) {
        const int idx = tid + i * kThreads;
        const int row = idx >> 3, seg = idx & 7;
        const int64_t j = c0 + row;
        const int kk = kc + seg * 8;
        uint4 vh = make_uint4(0u, 0u, 0u, 0u), vl = vh;
        if (j < ce && kk < Dp) {  // ragged rows and the chunk's tail past Dp are zero-filled
          vh = *reinterpret_cast<const uint4*>(c_hi + j * (int64_t)Dp + kk);
          vl = *reinterpret_cast<const uint4*>(c_lo + j * (int64_t)Dp + kk);
        }
        *reinterpret_cast<uint4*>(lds.hi + row * kRowBytes + seg * 16) = vh;
        *reinterpret_cast<uint4*>(lds.lo + row * kRowBytes + seg * 16) = vl;
      }
      __syncthreads();
      const int steps = (Dp - kc) / 16 < KC / 16 ? (Dp - kc) / 16 : KC / 16;
      for (int s = 0; s < steps; ++s) {
        const int kk = kc + s * 16 + 8 * h;  // B[k = 8 h + j][col r]: 8 consecutive k of query r
        uint4 bh = make_uint4(0u, 0u, 0u, 0u), bl = bh;
        if (qvalid) {
          bh = *reinterpret_cast<const uint4*>(qh_row + kk);
          bl = *reinterpret_cast<const uint4*>(ql_row + kk);
        }
        const bf16x8 fbh = __builtin_bit_cast(bf16x8, bh), fbl = __builtin_bit_cast(bf16x8, bl);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          // A[row r][k = 8 h + j]: 8 consecutive k of candidate 32 a + r
          const int off = (a * 32 + r) * kRowBytes + (s * 16 + 8 * h) * 2;
          const bf16x8 fah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds.hi + off));
          const bf16x8 fal = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds.lo + off));
          acc[a] = conv::mfma16<F16>(fah, fbh, acc[a]);
          acc[a] = conv::mfma16<F16>(fah, fbl, acc[a]);
          acc[a] = conv::mfma16<F16>(fal, fbh, acc[a]);
        }
      }
    }
    // (the blocks by a compile-time loop: were the unroller to decline this loop around a large
    // epilogue, acc[a] would be indexed at run time, which doubled dd_knn's time when tried)
    conv::static_for<4>([&](auto a) {
#pragma unroll 1
      for (int t = 0; t < 16 / EPI_UNROLL; ++t)
        conv::static_for<EPI_UNROLL>([&](auto u) {
          constexpr int ua = u;
          float v = acc[a][ua];  // element i = t EPI_UNROLL + u, by selects on the pass number
          conv::static_for<16 / EPI_UNROLL - 1>([&](auto p) {
            constexpr int pa = p + 1;
            v = t == pa ? acc[a][pa * EPI_UNROLL + ua] : v;
          });
          const int i = t * EPI_UNROLL + ua;
          const int lr = a * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          epi(fmaf(-2.f, v, lds.norm[lr]), lr, c0);
        });
    });
  }
}

}  // namespace feat
}  // namespace dd
