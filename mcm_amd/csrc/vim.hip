// vim.hip — the ViM score (include/mcm.h mcm_vim_score_features): alpha times the norm of a query's component
// in the null space of the training features' principal subspace, minus the energy (log-sum-exp) of its logits, without
// the [B, K + R] matrix ever existing in HBM.  The bank's rows fall into two contiguous ranges: rows [0, K) the prompts,
// rows [K, K + R) the null-space basis.  Two launches in stream order, modelled on neglabel.hip:
//   vim_partial_kernel  grid (query tiles of 64) x (bank splits).  A workgroup walks its split's rows (bank_sim.hpp: the
//                       64 x 256 exact-fp32 similarities of a tile in LDS, the s[b, n] that knn.hip sees).  A tile is cut
//                       at row K into at most two segments; a wave per query folds the prompt segment into the open
//                       pair (bank_sim::lse_fold: max, sum exp((s - max) / T) in fp64) and adds the basis segment's
//                       (s - off)^2 to an fp64 sum of squares.  When the split ends the query's slot
//                       work[split, query] = {max, (float) sum, ssq} is written.
//   vim_combine_kernel  one thread per query: the log-sum-exp from the slots of the splits that hold prompt rows
//                       (bank_sim::lse_merge), the sum of squares from the slots of the splits that hold basis rows, both
//                       in split order in fp64; then the square root and the score.
// Which slots were written follows from K, R and the split length alone (a split that holds a row writes every query's
// slot), and the second launch reads exactly those: nothing is pre-filled and no unwritten word of the workspace is
// read.  Nothing is summed across workgroups by atomics, no workgroup waits for another, every loop is bounded by the
// arguments.
#include <limits.h>
#include <math.h>

#include "bank_sim.hpp"

namespace {

namespace vim {
using namespace bank_sim;
// behind the tile: the open pair of every query with this score's own ssq [Q] fp64 between its sums and its maxima
constexpr int LDS_BYTES = TILE_BYTES + PAIR_BYTES + Q * (int)sizeof(double);
}  // namespace vim

// what a split knows of a query: the pair of its prompt rows and the sum of squares of its basis rows
struct VimSlot {
  float m;     // max of the split's prompt similarities (-inf: none)
  float sum;   // sum exp((s - m) / T) over them
  double ssq;  // sum (s - off)^2 over the split's basis rows
};
static_assert(sizeof(VimSlot) == 16, "a slot is 16 bytes");

struct VimArgs {
  const float* feats;  // [B, P]
  const float* bank;   // [K + R, P]
  const double* off;   // [R] or nullptr
  VimSlot* work;       // [S, B]
  double inv_t;        // 1 / (double) T
  int N, per;          // split s holds bank rows [s per, min(N, (s + 1) per))
  int B, P, K;
};

__global__ __launch_bounds__(vim::THREADS) void vim_partial_kernel(VimArgs a) {
  using namespace vim;
  extern __shared__ __attribute__((aligned(16))) float vim_lds[];
  double* st_sum = pair_sums(vim_lds);
  double* st_ssq = st_sum + Q;
  float* st_max = pair_maxima(st_ssq);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q0 = blockIdx.x * Q;
  const int nq = a.B - q0 < Q ? a.B - q0 : Q;
  const int s = blockIdx.y;
  int64_t lo, hi;
  split_bounds(s, a.per, a.N, lo, hi);

  if (tid < Q) pair_reset(tid, st_sum, st_max, st_ssq);
  __syncthreads();

  // either zero gives the same bits in everything below: the tile is taken as the MFMA left it
  walk<false>(a.feats, a.bank, a.P, q0, nq, lo, hi, vim_lds, [=](int64_t tile0, int ncols) {
    const int n0 = (int)tile0, tile_end = n0 + ncols;  // N <= INT_MAX
    const int cut = a.K <= n0 ? 0 : (a.K < tile_end ? a.K - n0 : ncols);  // columns [0, cut) prompts, [cut, ncols) basis
    for (int qi = 0; qi < Q / 4; ++qi) {  // wave w owns queries 16 w .. 16 w + 15, their open state included
      const int q = w * (Q / 4) + qi;
      if (q >= nq) break;
      const float* row = vim_lds + q * LDSIM;
      float m = st_max[q];
      double sum = st_sum[q], ssq = st_ssq[q];
      if (cut > 0) lse_fold(row, 0, cut, lane, a.inv_t, m, sum);
      if (cut < ncols) {
        const int j0 = n0 - a.K;  // off[j] belongs to bank row K + j = n0 + i: j = j0 + i in [0, R)
        double part = 0.0;
        for (int i = cut + lane; i < ncols; i += 64) {
          const double d = a.off ? (double)row[i] - a.off[j0 + i] : (double)row[i];
          part = fma(d, d, part);
        }
        ssq += wave_sum(part);
      }
      if (lane == 0) {
        if (tile_end == hi) {  // the split ends here: the slot is complete
          VimSlot v;
          v.m = m;
          v.sum = (float)sum;
          v.ssq = ssq;
          a.work[(int64_t)s * a.B + q0 + q] = v;
        } else {
          st_max[q] = m;
          st_sum[q] = sum;
          st_ssq[q] = ssq;
        }
      }
    }
  });
}

struct VimCombineArgs {
  const VimSlot* work;
  double inv_t, alpha;
  float* scores;  // [B]
  float* parts;   // [B, 3] = resid, lse, maxlogit, or nullptr
  int B, K, N, per;
};

__global__ __launch_bounds__(vim::THREADS) void vim_combine_kernel(VimCombineArgs a) {
  const int64_t b = (int64_t)blockIdx.x * vim::THREADS + threadIdx.x;
  if (b >= a.B) return;
  const VimSlot* p = a.work + b;
  // the splits that hold a prompt row are 0 .. (K - 1) / per, the ones that hold a basis row K / per .. (N - 1) / per:
  // exactly the slots vim_partial_kernel wrote ((N - 1) / per < S: N <= S per)
  const int p1 = (a.K - 1) / a.per, r0 = a.K / a.per, r1 = (a.N - 1) / a.per;
  const int64_t stride = a.B;
  float M;
  const double tot = bank_sim::lse_merge(0, p1, a.inv_t, M, [=](int s) {
    const VimSlot v = p[s * stride];
    return float2{v.m, v.sum};
  });
  const double maxlogit = (double)M * a.inv_t;
  const double lse = maxlogit + log(tot);
  double ssq = 0.0;
  for (int s = r0; s <= r1; ++s) ssq += p[(int64_t)s * a.B].ssq;
  const double resid = sqrt(ssq);
  a.scores[b] = (float)(a.alpha * resid - lse);
  if (a.parts) {
    a.parts[b * 3 + 0] = (float)resid;
    a.parts[b * 3 + 1] = (float)lse;
    a.parts[b * 3 + 2] = (float)maxlogit;
  }
}

}  // namespace

int64_t vim_work_bytes(int B, int S) { return (int64_t)S * B * (int64_t)sizeof(VimSlot); }

hipError_t launch_vim(const float* feats, int B, const float* bank, int K, int R, int P, const double* off, float T,
                      float alpha, int S, void* work, float* scores, float* parts, hipStream_t s) {
  if (B < 1 || K < 1 || R < 1 || P < 4 || P % 4 || S < 1 || S > MCM_KNN_MAX_SPLITS || !(T > 0.f) || !isfinite(T) ||
      !isfinite(alpha) || (int64_t)K + (int64_t)R > INT_MAX)
    return hipErrorInvalidValue;
  const int N = K + R;
  VimArgs a;
  a.feats = feats;
  a.bank = bank;
  a.off = off;
  a.work = (VimSlot*)work;
  a.inv_t = 1.0 / (double)T;
  a.N = N;
  a.per = (int)(((int64_t)N + S - 1) / S);
  a.B = B;
  a.P = P;
  a.K = K;
  const hipError_t e = launch_lds<vim_partial_kernel, vim::LDS_BYTES>(dim3(bank_sim::query_tiles(B), (unsigned)S),
                                                                     dim3(vim::THREADS), vim::LDS_BYTES, s, a);
  if (e != hipSuccess) return e;
  VimCombineArgs c;
  c.work = (const VimSlot*)work;
  c.inv_t = a.inv_t;
  c.alpha = (double)alpha;
  c.scores = scores;
  c.parts = parts;
  c.B = B;
  c.K = K;
  c.N = N;
  c.per = a.per;
  hipLaunchKernelGGL(vim_combine_kernel, dim3((unsigned)(((int64_t)B + vim::THREADS - 1) / vim::THREADS)),
                     dim3(vim::THREADS), 0, s, c);
  return hipGetLastError();
}
