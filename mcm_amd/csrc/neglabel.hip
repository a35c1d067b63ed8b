// neglabel.hip — the NegLabel score (include/mcm.h mcm_neglabel_score_features): the share of a query's
// softmax mass that falls on the ID rows of a bank of K ID prompts and G groups of gs negative prompts, taken against
// every group alone and averaged, without the [B, N] matrix ever existing in HBM.  The bank's rows fall into G + 1
// contiguous *ranges*: range 0 = rows [0, K), range 1 + g = rows [K + g gs, K + (g + 1) gs).  Two launches in stream order:
//   neg_partial_kernel  grid (query tiles of 64) x (bank splits).  A workgroup walks its split's rows (bank_sim.hpp: the
//                       64 x 256 exact-fp32 similarities of a tile in LDS, the s[b, n] that knn.hip sees).  A tile is cut
//                       into segments (a range intersected with the tile); a wave per query folds every segment into
//                       the open pair of its range (bank_sim::lse_fold: max, sum exp((s - max) / T) in fp64).  The
//                       pair is written to work[split, query, range] when its range or the split ends.
//   neg_combine_kernel  one workgroup per query: per range the partial pairs of the splits that hold rows of it, merged
//                       in split order (bank_sim::lse_merge), give its log-sum-exp in fp64;
//                       S[g] = 1 / (1 + exp(LN[g] - LI)); the mean is a fixed tree.
// Which (split, range) slots were written follows from K, gs and the split length alone, and the second launch reads
// exactly those: nothing is pre-filled and no unwritten word of the workspace is read.  Nothing is summed across
// workgroups by atomics, no workgroup waits for another, every loop is bounded by the arguments.
#include <limits.h>
#include <math.h>

#include "bank_sim.hpp"

namespace {

namespace neg {
using namespace bank_sim;
constexpr int LDS_BYTES = TILE_BYTES + PAIR_BYTES;  // behind the tile: the open pair of every query
}  // namespace neg

struct NegArgs {
  const float* feats;  // [B, P]
  const float* bank;   // [N, P]
  float2* work;        // [S, B, G + 1]: (max, sum) of the range's rows inside the split
  double inv_t;        // 1 / (double) T
  int N, per;          // split s holds bank rows [s per, min(N, (s + 1) per))
  int B, P, K, G, gs;
};

__global__ __launch_bounds__(neg::THREADS) void neg_partial_kernel(NegArgs a) {
  using namespace neg;
  extern __shared__ __attribute__((aligned(16))) float neg_lds[];
  double* st_sum = pair_sums(neg_lds);
  float* st_max = pair_maxima(st_sum);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q0 = blockIdx.x * Q;
  const int nq = a.B - q0 < Q ? a.B - q0 : Q;
  const int s = blockIdx.y;
  int64_t lo, hi;
  split_bounds(s, a.per, a.N, lo, hi);

  if (tid < Q) pair_reset(tid, st_sum, st_max);
  __syncthreads();

  // either zero gives the same bits in everything below: the tile is taken as the MFMA left it
  walk<false>(a.feats, a.bank, a.P, q0, nq, lo, hi, neg_lds, [=](int64_t tile0, int ncols) {
    const int n0 = (int)tile0, tile_end = n0 + ncols;  // N <= INT_MAX
    for (int qi = 0; qi < Q / 4; ++qi) {  // wave w owns queries 16 w .. 16 w + 15, their open pairs included
      const int q = w * (Q / 4) + qi;
      if (q >= nq) break;
      const float* row = neg_lds + q * LDSIM;
      float m = st_max[q];
      double sum = st_sum[q];
      int c = 0;
      while (c < ncols) {  // a segment holds at least one row: at most ncols turns
        const int n = n0 + c;
        const int rg = n < a.K ? 0 : 1 + (n - a.K) / a.gs;
        const int rend = rg == 0 ? a.K : a.K + rg * a.gs;  // <= N
        const int ce = rend < tile_end ? rend - n0 : ncols;
        lse_fold(row, c, ce, lane, a.inv_t, m, sum);
        if (rend <= tile_end || tile_end == hi) {  // the range or the split ends here: the pair is complete
          if (lane == 0) a.work[((int64_t)s * a.B + q0 + q) * (int64_t)(a.G + 1) + rg] = float2{m, (float)sum};
          m = -INFINITY;
          sum = 0.0;
        }
        c = ce;
      }
      if (lane == 0) {
        st_max[q] = m;
        st_sum[q] = sum;
      }
    }
  });
}

struct NegCombineArgs {
  const float2* work;
  double inv_t;
  float* scores;  // [B]
  float* group;   // [B, G] or nullptr
  int B, K, G, gs, per;
};

// log-sum-exp of the logits of bank rows [lo, hi) (range rg) of query b from the pairs of splits lo / per .. (hi - 1) / per:
// exactly the splits that hold a row of the range, which are the slots neg_partial_kernel wrote
__device__ __forceinline__ double neg_range_lse(const NegCombineArgs& a, int64_t b, int rg, int lo, int hi) {
  const int s0 = lo / a.per, s1 = (hi - 1) / a.per;  // s1 < S: hi <= N <= S per
  const int64_t stride = (int64_t)a.B * (a.G + 1);
  const float2* p = a.work + b * (int64_t)(a.G + 1) + rg;
  float M;
  const double tot = bank_sim::lse_merge(s0, s1, a.inv_t, M, [=](int s) { return p[s * stride]; });
  return (double)M * a.inv_t + log(tot);
}

__global__ __launch_bounds__(neg::THREADS) void neg_combine_kernel(NegCombineArgs a) {
  __shared__ double red[neg::THREADS];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double LI = neg_range_lse(a, b, 0, 0, a.K);  // every thread forms it: at most S pairs
  double acc = 0.0;
  for (int gi = tid; gi < a.G; gi += neg::THREADS) {
    const int lo = a.K + gi * a.gs;
    const double LN = neg_range_lse(a, b, 1 + gi, lo, lo + a.gs);
    const float Sg = (float)(1.0 / (1.0 + exp(LN - LI)));
    if (a.group) a.group[b * a.G + gi] = Sg;
    acc += (double)Sg;  // the score is the mean of the values group_dev gets, whether it is asked for or not
  }
  red[tid] = acc;
  __syncthreads();
  for (int off = neg::THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) a.scores[b] = (float)(-(red[0] / (double)a.G));
}

}  // namespace

int64_t neglabel_work_bytes(int B, int G, int S) { return (int64_t)S * B * ((int64_t)G + 1) * (int64_t)sizeof(float2); }

hipError_t launch_neglabel(const float* feats, int B, const float* bank, int K, int G, int gs, int P, float T, int S,
                           void* work, float* scores, float* group, hipStream_t s) {
  if (B < 1 || K < 1 || G < 1 || G > MCM_NEG_MAX_GROUPS || gs < 1 || P < 4 || P % 4 || S < 1 || S > MCM_KNN_MAX_SPLITS ||
      !(T > 0.f) || !isfinite(T) || (int64_t)K + (int64_t)G * gs > INT_MAX)
    return hipErrorInvalidValue;
  const int N = K + G * gs;
  NegArgs a;
  a.feats = feats;
  a.bank = bank;
  a.work = (float2*)work;
  a.inv_t = 1.0 / (double)T;
  a.N = N;
  a.per = (int)(((int64_t)N + S - 1) / S);
  a.B = B;
  a.P = P;
  a.K = K;
  a.G = G;
  a.gs = gs;
  const hipError_t e = launch_lds<neg_partial_kernel, neg::LDS_BYTES>(dim3(bank_sim::query_tiles(B), (unsigned)S),
                                                                     dim3(neg::THREADS), neg::LDS_BYTES, s, a);
  if (e != hipSuccess) return e;
  NegCombineArgs c;
  c.work = (const float2*)work;
  c.inv_t = a.inv_t;
  c.scores = scores;
  c.group = group;
  c.B = B;
  c.K = K;
  c.G = G;
  c.gs = gs;
  c.per = a.per;
  hipLaunchKernelGGL(neg_combine_kernel, dim3((unsigned)B), dim3(neg::THREADS), 0, s, c);
  return hipGetLastError();
}
