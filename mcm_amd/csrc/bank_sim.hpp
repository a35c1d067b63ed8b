// bank_sim.hpp — what the bank-streamed scores share.
// The walk (knn.hip, neglabel.hip, vim.hip, glmcm.hip): a workgroup of 256 threads takes 64 query rows and a range of bank
// rows and sees the exact-fp32 similarities 64 x 256 at a time in LDS, without the [B, N] matrix ever existing in HBM.  A
// score is what its kernel does with a tile (the callback of walk) and the state it keeps *behind* the tile: its dynamic
// LDS is TILE_BYTES plus what it states for itself.
// The fold (neglabel.hip, vim.hip, glmcm.hip; not knn.hip, which selects and sums nothing): the online log-sum-exp of tile
// rows.  lse_fold takes columns of a tile row into a query's open pair (max, sum exp((s - max) / T)), the sum in fp64; the
// open pairs of a workgroup's queries lie behind the tile (PAIR_BYTES, pair_sums, pair_maxima, pair_reset); lse_merge adds
// the pairs that the splits of a bank left (neglabel.hip, vim.hip; glmcm.hip walks the whole bank in one workgroup).
// score_stream.hip walks like the others and folds with softmax_moments_fold, which carries two more sums than lse_fold.
#pragma once
#include "common.hpp"

namespace bank_sim {
constexpr int Q = 64;             // queries of a workgroup
constexpr int TN = 256;           // bank rows of a tile
constexpr int KC = 32;            // feature columns of a staged chunk
constexpr int LDA = KC + 4;       // LDS row stride of a staged operand (floats; rows stay 16-byte aligned)
constexpr int LDSIM = TN + 4;     // LDS row stride of the similarity tile
constexpr int THREADS = 256;
constexpr int STAGE_FLOATS = (Q + TN) * LDA;
constexpr int SIM_FLOATS = Q * LDSIM;  // the similarity tile lies over the staging buffers (they are dead by then)
constexpr int TILE_BYTES = SIM_FLOATS * (int)sizeof(float);  // a score's own LDS starts here
static_assert(STAGE_FLOATS <= SIM_FLOATS, "the staging buffers must fit under the similarity tile");

// split s of a bank of N rows cut into ranges of `per` rows holds rows [lo, hi) = [s per, min(N, (s + 1) per))
__device__ __forceinline__ void split_bounds(int64_t s, int64_t per, int64_t N, int64_t& lo, int64_t& hi) {
  lo = s * per < N ? s * per : N;
  hi = lo + per < N ? lo + per : N;
}

// Walks bank rows [lo, hi) in tiles of TN for the nq <= Q query rows from q0 (feats [B, P], bank [N, P], P % 4 == 0, both
// 16-byte aligned).  Per tile: the Q x TN similarities are accumulated by the exact-fp32 MFMA, both operands staged
// through LDS in KC-column chunks (the next chunk in registers under the MFMAs), and stored to lds[q * LDSIM + j],
// j < ncols, with PlusZero -0 as +0 (for a score that must not see which of two equal zeros came first); behind a
// barrier tile(n0, ncols) is called by every thread.  Rows q >= nq and columns j >= ncols hold the similarities of zero
// rows.  The tile is overwritten after the next barrier all threads reach, which the walk's next turn provides: a
// callback needs none of its own to be done reading.  s[b, n] is one fixed sum for given rows, wherever the row falls.
// A callback captures by value: with reference captures knn_partial_kernel came out with other registers and layout.
template <bool PlusZero, class Tile>
__device__ __forceinline__ void walk(const float* feats, const float* bank, int P, int q0, int nq, int64_t lo,
                                     int64_t hi, float* lds, Tile&& tile) {
  float* As = lds;             // [Q][LDA]
  float* Bs = lds + Q * LDA;   // [TN][LDA]
  float* Sim = lds;            // [Q][LDSIM], over As / Bs
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, r = lane & 15;
  const int nchunks = (P + KC - 1) / KC;
  const int ld_row = tid >> 3, ld_c4 = (tid & 7) * 4;  // a thread's share of a chunk: rows ld_row + 32 i, 4 columns
  for (int64_t n0 = lo; n0 < hi; n0 += TN) {
    const int ncols = hi - n0 < TN ? (int)(hi - n0) : TN;
    f32x4_t acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    float4 ra[2], rb[8];
    auto gload = [&](int kc) {
      const int col = kc * KC + ld_c4;
      const bool cok = col < P;  // P % 4 == 0: four columns are in or out together
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = ld_row + 32 * i;
        ra[i] = (cok && row < nq) ? *(const float4*)(feats + (int64_t)(q0 + row) * P + col) : float4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int row = ld_row + 32 * i;
        rb[i] = (cok && row < ncols) ? *(const float4*)(bank + (n0 + row) * (int64_t)P + col) : float4{0.f, 0.f, 0.f, 0.f};
      }
    };
    gload(0);
    for (int kc = 0; kc < nchunks; ++kc) {
      __syncthreads();  // the chunk (or the similarity tile) under these bytes has been read
#pragma unroll
      for (int i = 0; i < 2; ++i) *(float4*)(As + (ld_row + 32 * i) * LDA + ld_c4) = ra[i];
#pragma unroll
      for (int i = 0; i < 8; ++i) *(float4*)(Bs + (ld_row + 32 * i) * LDA + ld_c4) = rb[i];
      __syncthreads();
      if (kc + 1 < nchunks) gload(kc + 1);  // in flight under the MFMAs
#pragma unroll
      for (int sub = 0; sub < KC / 16; ++sub) {
        // lane (g, r) takes columns 16 sub + 4 g .. + 3 of its rows as one 16-byte read; MFMA t of the four then
        // multiplies column 16 sub + 4 g + t of both operands: the same column on both sides, so the sum over the
        // four MFMAs covers the 16 columns once each (in an order of its own, which a dot product may have)
        f32x4_t av[4], bv[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          av[mi] = __builtin_bit_cast(f32x4_t, *(const float4*)(As + (mi * 16 + r) * LDA + sub * 16 + g * 4));
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          bv[ni] = __builtin_bit_cast(f32x4_t, *(const float4*)(Bs + (w * 64 + ni * 16 + r) * LDA + sub * 16 + g * 4));
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi][t], bv[ni][t], acc[mi][ni], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave is done with As / Bs
    // D[i = 4 g + e][j = r]: i a query of block mi, j a bank row of this wave's block ni
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = acc[mi][ni][e];
          Sim[(mi * 16 + 4 * g + e) * LDSIM + w * 64 + ni * 16 + r] = PlusZero && v == 0.f ? 0.f : v;
        }
    __syncthreads();
    tile(n0, ncols);
  }
}

// ---- the fold: an online log-sum-exp over tile rows ---------------------------------------------------------------------
// The open pair of every query of the workgroup lies behind the tile: the sums [Q] fp64 at TILE_BYTES, then `own` fp64
// arrays [Q] that a score keeps there for itself (vim.hip's sums of squares), then the maxima [Q] fp32.
constexpr int PAIR_BYTES = Q * (int)(sizeof(double) + sizeof(float));
static_assert(TILE_BYTES % sizeof(double) == 0, "the fp64 sums must be 8-byte aligned");
__device__ __forceinline__ double* pair_sums(float* lds) { return (double*)(lds + SIM_FLOATS); }
__device__ __forceinline__ float* pair_maxima(double* last) { return (float*)(last + Q); }  // last: the fp64 array before them
// Thread tid < Q empties pair tid, and entry tid of the score's `own` arrays with it; the kernel's barrier follows.  The
// `if (tid < Q)` stands at the call, in the kernel: with the branch in here the kernels' q0 / nq arithmetic was placed
// on the other side of it and the three kernels came out with other instructions.
template <class... Own>
__device__ __forceinline__ void pair_reset(int tid, double* st_sum, float* st_max, Own*... own) {
  st_sum[tid] = 0.0;
  ((own[tid] = 0.0), ...);
  st_max[tid] = -INFINITY;
}

// One wave folds columns [c, ce) of a tile row into the open pair (m, sum): sum becomes sum exp((s - m) / T) over the
// columns folded so far at their maximum m.  Every lane ends with the same m and sum.
__device__ __forceinline__ void lse_fold(const float* row, int c, int ce, int lane, double inv_t, float& m, double& sum) {
  float mx = -INFINITY;
  for (int i = c + lane; i < ce; i += 64) mx = fmaxf(mx, row[i]);  // a NaN is skipped here and poisons the sum below
  const float M = fmaxf(m, wave_max(mx));
  double part = 0.0;
  for (int i = c + lane; i < ce; i += 64) part += exp(((double)row[i] - (double)M) * inv_t);
  part = wave_sum(part);
  if (m != M) sum *= exp(((double)m - (double)M) * inv_t);  // m = -inf: the sum is 0 and stays 0
  sum += part;
  m = M;
}

// The pairs of splits s0 .. s1 (pair(s) = float2{max, sum}, the sum as fp32 as a split stores it) merged: M their largest
// maximum, the return value sum_s sum(s) exp((max(s) - M) / T) in fp64, added in split order.  The log-sum-exp of the rows
// behind them is M / T + log of it.
template <class Pair>
__device__ __forceinline__ double lse_merge(int s0, int s1, double inv_t, float& M, Pair&& pair) {
  M = -INFINITY;
  for (int s = s0; s <= s1; ++s) M = fmaxf(M, pair(s).x);
  double tot = 0.0;
  for (int s = s0; s <= s1; ++s) {
    const float2 v = pair(s);
    tot += v.x == M ? (double)v.y : (double)v.y * exp(((double)v.x - (double)M) * inv_t);
  }
  return tot;
}

// The fold of score_stream.hip: lse_fold with two more sums, for the scores that need more of a softmax than its
// normaliser.  With x = (s - m) / T at the running maximum m the open state is Z = sum exp(x), W = sum x exp(x),
// Q2 = sum exp(2 x), all fp64.  When the maximum rises from m to M, with d = (m - M) / T and a = exp(d):
// Z <- a Z, W <- a (W + d Z), Q2 <- a^2 Q2 (m = -inf: nothing has been folded, the sums are 0 and stay 0).  exp(2 x) is
// the square of the exp(x) that Z takes.  Every lane ends with the same m, Z, W, Q2.  A NaN is skipped by the maximum and
// poisons the three sums.
__device__ __forceinline__ void softmax_moments_fold(const float* row, int c, int ce, int lane, double inv_t, float& m,
                                                     double& Z, double& W, double& Q2) {
  float mx = -INFINITY;
  for (int i = c + lane; i < ce; i += 64) mx = fmaxf(mx, row[i]);
  const float M = fmaxf(m, wave_max(mx));
  double pz = 0.0, pw = 0.0, pq = 0.0;
  for (int i = c + lane; i < ce; i += 64) {
    const double x = ((double)row[i] - (double)M) * inv_t;
    const double e = exp(x);
    pz += e;
    pw = fma(x, e, pw);
    pq = fma(e, e, pq);
  }
  pz = wave_sum(pz);
  pw = wave_sum(pw);
  pq = wave_sum(pq);
  if (m != M && m != -INFINITY) {
    const double d = ((double)m - (double)M) * inv_t;
    const double a = exp(d);
    W = a * fma(d, Z, W);
    Z *= a;
    Q2 *= a * a;
  }
  Z += pz;
  W += pw;
  Q2 += pq;
  m = M;
}

inline unsigned query_tiles(int B) { return (unsigned)(((int64_t)B + Q - 1) / Q); }
}  // namespace bank_sim

// the split count the library picks from B, N and the current device's CU count (splits = 0 of either score)
inline int bank_auto_splits(int B, int64_t N) {
  int cus = device_cu_count();
  if (cus <= 0) cus = 256;
  const int64_t qtiles = bank_sim::query_tiles(B);
  const int64_t tiles = (N + bank_sim::TN - 1) / bank_sim::TN;
  int64_t want = (2 * (int64_t)cus + qtiles - 1) / qtiles;  // two workgroups fit a CU's LDS
  if (want > tiles) want = tiles;
  if (want > MCM_KNN_MAX_SPLITS) want = MCM_KNN_MAX_SPLITS;
  return want < 1 ? 1 : (int)want;
}
