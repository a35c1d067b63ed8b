// score_stream.hip — the streamed tail of the MCM family (include/mcm_score_stream.h mcm_score_features_stream; DESIGN.md
// 4.18): MCM, max-logit, energy, entropy and var of every query row against a prompt bank of any size, and its top-k
// matches, without the [B, K] matrix ever existing in HBM and without one image's similarities having to fit LDS (which is
// what bounds score.hip's tail to (K + P) * 4 <= 150 KiB).  Two launches in stream order, modelled on vim.hip:
//   sst_partial_kernel  grid (query tiles of 64) x (bank splits).  A workgroup walks its split's rows (bank_sim.hpp: the
//                       64 x 256 exact-fp32 similarities of a tile in LDS, the s[b, n] that knn.hip sees).  A wave per
//                       query folds the tile row into the open state (bank_sim::softmax_moments_fold: the fp32 maximum m
//                       and, at x = (s - m) / T, Z = sum exp(x), W = sum x exp(x), Q2 = sum exp(2 x) in fp64) and, with
//                       topk > 0, merges the row into the query's list of the topk best (value, row) pairs.  When the
//                       split ends the query's slot work[split, query] = {Z, W, Q2, m} and its list are written.
//   sst_combine_kernel  one thread per query: the slots of the splits that hold rows merged in split order in fp64, the
//                       five scores from the merged (m, Z, W, Q2), the lists merged in the selection order.
// Which slots were written follows from K and the split length alone (a split that holds a row writes every query's slot
// and list), and the second launch reads exactly those: nothing is pre-filled and no unwritten word of the workspace is
// read.  Nothing is summed across workgroups by atomics, no workgroup waits for another, every loop is bounded by the
// arguments.
// LDS of sst_partial_kernel: TILE_BYTES 66 560 + the open state 64 x (3 x 8 + 4) = 1 792 + the lists 64 x 8 x 8 = 4 096
// = 72 448 bytes; two workgroups take 144 896 of a CU's 163 840, which is what bank_auto_splits counts on.
#include <limits.h>
#include <math.h>

#include "bank_sim.hpp"

namespace {

namespace sst {
using namespace bank_sim;
constexpr int LIST = MCM_TOPK_MAX;                                                  // entries of a query's list
constexpr int STATE_BYTES = Q * (int)(3 * sizeof(double) + sizeof(float));         // Z, W, Q2 [Q] fp64, then m [Q] fp32
constexpr int LIST_BYTES = Q * LIST * (int)(sizeof(float) + sizeof(int));          // values [Q][LIST], then rows [Q][LIST]
constexpr int LDS_BYTES = TILE_BYTES + STATE_BYTES + LIST_BYTES;
static_assert(STATE_BYTES == 1792 && LIST_BYTES == 4096 && 2 * LDS_BYTES <= 160 * 1024, "two workgroups fit a CU's LDS");
}  // namespace sst

// what a split knows of a query
struct SstSlot {
  double Z, W, Q2;  // sum exp(x), sum x exp(x), sum exp(2 x) over the split's rows, x = (s - m) / T
  float m;          // max of the split's similarities (NaN entries skipped)
  float pad;
};
static_assert(sizeof(SstSlot) == 32, "a slot is 32 bytes");

struct SstPair {
  float v;  // similarity
  int i;    // bank row, -1: no candidate
};
static_assert(sizeof(SstPair) == 8, "a list entry is 8 bytes");

// (value, row) pairs under the selection order of mcm_score_features_topk: value descending, then row ascending; row < 0 =
// no candidate.  +0.0 == -0.0, so the lower row wins between them; a NaN never compares and is never a candidate.
__device__ __forceinline__ void sst_better(float& v, int& i, float ov, int oi) {
  if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) {
    v = ov;
    i = oi;
  }
}
// (v, i) comes strictly after (pv, pi) in that order
__device__ __forceinline__ bool sst_after(float v, int i, float pv, int pi) { return v < pv || (v == pv && i > pi); }

struct SstArgs {
  const float* feats;  // [B, P]
  const float* bank;   // [K, P]
  SstSlot* work;       // [S, B]
  SstPair* lists;      // [S, B, topk], behind the slots
  double inv_t;        // 1 / (double) T
  int K, per;          // split s holds bank rows [s per, min(K, (s + 1) per))
  int B, P, topk;
};

template <bool TOPK>
__global__ __launch_bounds__(sst::THREADS) void sst_partial_kernel(SstArgs a) {
  using namespace sst;
  extern __shared__ __attribute__((aligned(16))) float sst_lds[];
  double* st_z = pair_sums(sst_lds);
  double* st_w = st_z + Q;
  double* st_q = st_w + Q;
  float* st_max = pair_maxima(st_q);
  float* list_v = st_max + Q;            // [Q][LIST]
  int* list_i = (int*)(list_v + Q * LIST);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q0 = blockIdx.x * Q;
  const int nq = a.B - q0 < Q ? a.B - q0 : Q;
  const int s = blockIdx.y;
  int64_t lo, hi;
  split_bounds(s, a.per, a.K, lo, hi);

  if (tid < Q) pair_reset(tid, st_z, st_max, st_w, st_q);
  if constexpr (TOPK)
    for (int i = tid; i < Q * LIST; i += THREADS) {
      list_v[i] = 0.f;
      list_i[i] = -1;
    }
  __syncthreads();

  // the tile is taken as the MFMA left it: -0 == +0 in every comparison below, and exp sees no difference
  walk<false>(a.feats, a.bank, a.P, q0, nq, lo, hi, sst_lds, [=](int64_t tile0, int ncols) {
    const int n0 = (int)tile0, tile_end = n0 + ncols;  // K <= INT_MAX
    for (int qi = 0; qi < Q / 4; ++qi) {  // wave w owns queries 16 w .. 16 w + 15, their open state and list included
      const int q = w * (Q / 4) + qi;
      if (q >= nq) break;
      const float* row = sst_lds + q * LDSIM;
      float m = st_max[q];
      double Z = st_z[q], W = st_w[q], Q2 = st_q[q];
      softmax_moments_fold(row, 0, ncols, lane, a.inv_t, m, Z, W, Q2);
      float ov = 0.f;  // lane j < topk holds entry j of the query's list, best first
      int oi = -1;
      if constexpr (TOPK) {
        const int topk = a.topk;
        if (lane < topk) {
          ov = list_v[q * LIST + lane];
          oi = list_i[q * LIST + lane];
        }
        const float wv = __shfl(ov, topk - 1, 64);  // the list's last entry: what a row has to beat once the list is full
        const int wi = __shfl(oi, topk - 1, 64);
        float v[4];
        bool cand = false;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int col = c * 64 + lane;
          v[c] = col < ncols ? row[col] : NAN;
          // a row equal to the last entry loses to it: its row number is the larger one (the walk goes upwards)
          cand = cand || (wi < 0 ? v[c] == v[c] : v[c] > wv);
        }
        if (__ballot(cand)) {  // round r: the best of (tile row, old list) strictly after winner r - 1
          float pv = INFINITY, selv = 0.f;
          int pi = -1, seli = -1;
          for (int r = 0; r < topk; ++r) {
            float bv = 0.f;
            int bi = -1;
#pragma unroll
            for (int c = 0; c < 4; ++c) {  // rows ascending: a strict > keeps the lower one
              const int k = n0 + c * 64 + lane;
              if (sst_after(v[c], k, pv, pi) && (bi < 0 || v[c] > bv)) {
                bv = v[c];
                bi = k;
              }
            }
            if (oi >= 0 && sst_after(ov, oi, pv, pi)) sst_better(bv, bi, ov, oi);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
              const float xv = __shfl_xor(bv, o, 64);
              const int xi = __shfl_xor(bi, o, 64);
              sst_better(bv, bi, xv, xi);
            }
            if (bi < 0) break;  // nothing left: the remaining entries stay empty
            if (lane == r) {
              selv = bv;
              seli = bi;
            }
            pv = bv;
            pi = bi;
          }
          ov = selv;
          oi = seli;
          if (lane < topk) {
            list_v[q * LIST + lane] = ov;
            list_i[q * LIST + lane] = oi;
          }
        }
      }
      if (tile_end == hi) {  // the split ends here: the slot and the list are complete
        const int64_t slot = (int64_t)s * a.B + q0 + q;
        if (lane == 0) {
          SstSlot o;
          o.Z = Z;
          o.W = W;
          o.Q2 = Q2;
          o.m = m;
          o.pad = 0.f;
          a.work[slot] = o;
        }
        if constexpr (TOPK) {
          if (lane < a.topk) {
            SstPair p;
            p.v = ov;
            p.i = oi;
            a.lists[slot * a.topk + lane] = p;
          }
        }
      } else if (lane == 0) {
        st_max[q] = m;
        st_z[q] = Z;
        st_w[q] = W;
        st_q[q] = Q2;
      }
    }
  });
}

struct SstCombineArgs {
  const SstSlot* work;
  const SstPair* lists;
  double inv_t, td;  // 1 / (double) T, (double) T
  float* scores;     // [B]
  float* parts;      // [B, 5] in MCM_SCORE_* order, or nullptr
  int* idx;          // [B, topk] (topk > 0)
  float* prob;       // [B, topk] or nullptr
  int B, K, per, kind, topk;
};

__global__ __launch_bounds__(sst::THREADS) void sst_combine_kernel(SstCombineArgs a) {
  const int64_t b = (int64_t)blockIdx.x * sst::THREADS + threadIdx.x;
  if (b >= a.B) return;
  const SstSlot* p = a.work + b;
  const int s1 = (a.K - 1) / a.per;  // the splits that hold a row are 0 .. s1: exactly the slots sst_partial_kernel wrote
  float M = -INFINITY;
  for (int s = 0; s <= s1; ++s) M = fmaxf(M, p[(int64_t)s * a.B].m);
  double Z = 0.0, W = 0.0, Q2 = 0.0;
  for (int s = 0; s <= s1; ++s) {
    const SstSlot v = p[(int64_t)s * a.B];
    if (v.m == M) {
      Z += v.Z;
      W += v.W;
      Q2 += v.Q2;
    } else {
      const double d = ((double)v.m - (double)M) * a.inv_t;
      const double e = exp(d);
      Z += e * v.Z;
      W += e * fma(d, v.Z, v.W);
      Q2 += (e * e) * v.Q2;
    }
  }
  const bool bad = Z != Z;  // a NaN similarity in this row: every score of the row is NaN (the maximum skipped it)
  const double r = 1.0 / Z, lz = log(Z);
  const float o_mcm = -(float)r;
  const float o_max = bad ? NAN : -M;
  const float o_energy = (float)(-(a.td * ((double)M * a.inv_t + lz)));
  const float o_entropy = (float)(lz - W / Z);
  const float o_var = (float)(-((Q2 / (Z * Z) - 1.0 / (double)a.K) / (double)a.K));  // the softmax's mean is exactly 1 / K
  a.scores[b] = a.kind == MCM_SCORE_MCM ? o_mcm
              : a.kind == MCM_SCORE_MAX_LOGIT ? o_max
              : a.kind == MCM_SCORE_ENERGY ? o_energy
              : a.kind == MCM_SCORE_ENTROPY ? o_entropy : o_var;
  if (a.parts) {
    float* o = a.parts + b * 5;
    o[MCM_SCORE_MCM] = o_mcm;
    o[MCM_SCORE_MAX_LOGIT] = o_max;
    o[MCM_SCORE_ENERGY] = o_energy;
    o[MCM_SCORE_ENTROPY] = o_entropy;
    o[MCM_SCORE_VAR] = o_var;
  }
  // Round r: the best entry of any split's list strictly after winner r - 1.  A list is sorted in the selection order, so
  // its first entry after the winner is its best one.
  float pv = INFINITY;
  int pi = -1;
  for (int t = 0; t < a.topk; ++t) {
    float bv = 0.f;
    int bi = -1;
    for (int s = 0; s <= s1; ++s) {
      const SstPair* l = a.lists + ((int64_t)s * a.B + b) * a.topk;
      for (int j = 0; j < a.topk; ++j) {
        const SstPair e = l[j];
        if (e.i < 0) break;
        if (sst_after(e.v, e.i, pv, pi)) {
          sst_better(bv, bi, e.v, e.i);
          break;
        }
      }
    }
    a.idx[b * a.topk + t] = bi;
    // the same exp((s - max) / T) term and the same fp64 Z as the score: for MCM on a NaN-free row prob[b, 0] =
    // (float)(1.0 / Z) = -scores[b], bit for bit
    if (a.prob) a.prob[b * a.topk + t] = bi < 0 ? NAN : (float)(exp(((double)bv - (double)M) * a.inv_t) / Z);
    if (bi >= 0) {
      pv = bv;
      pi = bi;
    }
  }
}

}  // namespace

int64_t score_stream_work_bytes(int B, int topk, int S) {
  return (int64_t)S * B * (int64_t)(sizeof(SstSlot) + (size_t)topk * sizeof(SstPair));
}

hipError_t launch_score_stream(const float* feats, int B, const float* bank, int K, int P, float T, int kind, int topk, int S,
                               void* work, float* scores, float* parts, int* idx, float* prob, hipStream_t s) {
  if (B < 1 || K < 1 || P < 4 || P % 4 || S < 1 || S > MCM_KNN_MAX_SPLITS || !(T > 0.f) || !isfinite(T) || kind < 0 ||
      kind > MCM_SCORE_VAR || topk < 0 || topk > MCM_TOPK_MAX || (topk > 0 && !idx))
    return hipErrorInvalidValue;
  SstArgs a;
  a.feats = feats;
  a.bank = bank;
  a.work = (SstSlot*)work;
  a.lists = (SstPair*)((char*)work + (int64_t)S * B * (int64_t)sizeof(SstSlot));
  a.inv_t = 1.0 / (double)T;
  a.K = K;
  a.per = (int)(((int64_t)K + S - 1) / S);
  a.B = B;
  a.P = P;
  a.topk = topk;
  const dim3 grid(bank_sim::query_tiles(B), (unsigned)S);
  const hipError_t e =
      topk > 0 ? launch_lds<sst_partial_kernel<true>, sst::LDS_BYTES>(grid, dim3(sst::THREADS), sst::LDS_BYTES, s, a)
               : launch_lds<sst_partial_kernel<false>, sst::LDS_BYTES>(grid, dim3(sst::THREADS), sst::LDS_BYTES, s, a);
  if (e != hipSuccess) return e;
  SstCombineArgs c;
  c.work = a.work;
  c.lists = a.lists;
  c.inv_t = a.inv_t;
  c.td = (double)T;
  c.scores = scores;
  c.parts = parts;
  c.idx = idx;
  c.prob = prob;
  c.B = B;
  c.K = K;
  c.per = a.per;
  c.kind = kind;
  c.topk = topk;
  hipLaunchKernelGGL(sst_combine_kernel, dim3((unsigned)(((int64_t)B + sst::THREADS - 1) / sst::THREADS)),
                     dim3(sst::THREADS), 0, s, c);
  return hipGetLastError();
}
