// knn.hip — the deep k-nearest-neighbour score (include/mcm.h mcm_knn_score_features): the k largest
// fp32 similarities of every query row against a bank of N training features, without the [B, N] matrix ever
// existing in HBM.  Two launches in stream order:
//   knn_partial_kernel  grid (query tiles of 64) x (bank splits).  A workgroup walks its split's rows (bank_sim.hpp:
//                       the 64 x 256 exact-fp32 similarities of a tile in LDS), and every query's k-entry list in the
//                       caller's workspace takes the ones above its threshold (a wave per query; knn_select_row).
//   knn_merge_kernel    one workgroup per query: the S partial lists (S k values, -inf padded to a power of two) are
//                       sorted in LDS, the first k are the result.
// Nothing is summed across workgroups and a top-k multiset does not depend on the order its candidates arrive in, so
// the outputs are a pure function of the inputs: no atomics, no counters, no waits between workgroups.
#include <limits.h>
#include <math.h>

#include "bank_sim.hpp"

namespace {

namespace knn {
using namespace bank_sim;
// behind the tile: threshold, count and minimum's position of every query's list, [Q] each
constexpr int LDS_BYTES = TILE_BYTES + 3 * Q * (int)sizeof(float);
constexpr int MERGE_LDS_MAX = MCM_KNN_MAX_SPLITS * MCM_KNN_MAX_K * (int)sizeof(float);  // 128 KiB
}  // namespace knn

struct KnnArgs {
  const float* feats;  // [B, P]
  const float* bank;   // [N, P]
  float* work;         // [S, B, k]: the partial lists
  int64_t N, per;      // split s holds bank rows [s per, min(N, (s + 1) per))
  int B, P, k, S;
};

// (smallest value, its lowest position) of list[0 .. k): every lane scans a strided share, then a butterfly
__device__ __forceinline__ void knn_list_min(const float* list, int k, int lane, float& mn, int& pos) {
  mn = INFINITY;
  pos = INT_MAX;
  for (int i = lane; i < k; i += 64) {
    const float x = list[i];
    if (pos == INT_MAX || x < mn) {
      mn = x;
      pos = i;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float omn = __shfl_xor(mn, off);
    const int opos = __shfl_xor(pos, off);
    if (opos != INT_MAX && (pos == INT_MAX || omn < mn || (omn == mn && opos < pos))) {
      mn = omn;
      pos = opos;
    }
  }
}

// One wave offers the n values of `row` (LDS) to a k-entry list: the first k candidates fill it, after that a
// candidate above the list's minimum `th` replaces that minimum (at `mp`) and the minimum is found again.  NaN is
// never a candidate.  cnt, th, mp are wave-uniform and carried from tile to tile by the caller.
__device__ __forceinline__ void knn_select_row(const float* row, int n, float* list, int k, int lane, int& cnt,
                                               float& th, int& mp) {
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int col = c0 + lane;
    const float v = col < n ? row[col] : NAN;
    bool ok = v == v;
    if (cnt < k) {
      const uint64_t m = __ballot(ok);
      const int before = __popcll(m & ((1ull << lane) - 1ull));
      const int all = __popcll(m);
      const int take = all < k - cnt ? all : k - cnt;
      if (ok && before < take) list[cnt + before] = v;
      ok = ok && before >= take;
      cnt += take;
      if (cnt == k) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the list is read back by other lanes of this wave
        knn_list_min(list, k, lane, th, mp);
      }
    }
    if (cnt == k) {
      uint64_t m = __ballot(ok && v > th);
      while (m) {  // at most 64 turns
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const float c = __shfl(v, l);
        if (c > th) {
          if (lane == 0) list[mp] = c;
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
          knn_list_min(list, k, lane, th, mp);
        }
      }
    }
  }
}

__global__ __launch_bounds__(knn::THREADS) void knn_partial_kernel(KnnArgs a) {
  using namespace knn;
  extern __shared__ __attribute__((aligned(16))) float knn_lds[];
  float* st_th = knn_lds + SIM_FLOATS;
  int* st_cnt = (int*)(st_th + Q);
  int* st_mp = st_cnt + Q;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q0 = blockIdx.x * Q;
  const int nq = a.B - q0 < Q ? a.B - q0 : Q;
  const int64_t s = blockIdx.y;
  int64_t lo, hi;
  split_bounds(s, a.per, a.N, lo, hi);
  const int k = a.k;

  if (tid < Q) {
    st_th[tid] = -INFINITY;
    st_cnt[tid] = 0;
    st_mp[tid] = 0;
  }
  __syncthreads();

  // -0 arrives as +0, so that which of two equal zeros a list keeps cannot depend on the order they came in
  walk<true>(a.feats, a.bank, a.P, q0, nq, lo, hi, knn_lds, [=](int64_t, int ncols) {
    for (int qi = 0; qi < Q / 4; ++qi) {  // wave w owns queries 16 w .. 16 w + 15, state included
      const int q = w * (Q / 4) + qi;
      if (q >= nq) break;
      float* list = a.work + ((int64_t)s * a.B + q0 + q) * (int64_t)k;
      float th = st_th[q];
      int cnt = st_cnt[q], mp = st_mp[q];
      knn_select_row(knn_lds + q * LDSIM, ncols, list, k, lane, cnt, th, mp);
      if (lane == 0) {
        st_th[q] = th;
        st_cnt[q] = cnt;
        st_mp[q] = mp;
      }
    }
  });
  __syncthreads();
  // slots no candidate reached (k above the split's rows, NaN similarities, an empty split)
  for (int qi = 0; qi < Q / 4; ++qi) {
    const int q = w * (Q / 4) + qi;
    if (q >= nq) break;
    float* list = a.work + ((int64_t)s * a.B + q0 + q) * (int64_t)k;
    for (int i = st_cnt[q] + lane; i < k; i += 64) list[i] = -INFINITY;
  }
}

// npow2: S k rounded up to a power of two (<= 32768): the LDS array this launch gets
__global__ __launch_bounds__(knn::THREADS) void knn_merge_kernel(const float* work, int B, int k, int S, int npow2,
                                                                 float* scores, float* topv) {
  extern __shared__ __attribute__((aligned(16))) float knn_lds[];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int total = S * k;
  for (int i = tid; i < npow2; i += knn::THREADS) {
    float v = -INFINITY;
    if (i < total) v = work[((int64_t)(i / k) * B + b) * (int64_t)k + i % k];
    knn_lds[i] = v;
  }
  __syncthreads();
  // bitonic sort, descending (the lists hold no NaN)
  for (int size = 2; size <= npow2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < npow2 / 2; t += knn::THREADS) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool desc = (i & size) == 0;
        const float x = knn_lds[i], y = knn_lds[j];
        if (desc ? x < y : x > y) {
          knn_lds[i] = y;
          knn_lds[j] = x;
        }
      }
      __syncthreads();
    }
  if (topv)
    for (int i = tid; i < k; i += knn::THREADS) topv[b * k + i] = knn_lds[i];
  if (tid == 0) {
    const double d = 2.0 - 2.0 * (double)knn_lds[k - 1];
    scores[b] = (float)sqrt(d > 0.0 ? d : 0.0);
  }
}

}  // namespace

hipError_t launch_knn(const float* feats, int B, const float* bank, int64_t N, int P, int k, int S, float* work,
                      float* scores, float* topv, hipStream_t s) {
  if (B < 1 || N < 1 || P < 4 || P % 4 || k < 1 || k > MCM_KNN_MAX_K || S < 1 || S > MCM_KNN_MAX_SPLITS)
    return hipErrorInvalidValue;
  hipError_t e = lds_limit<knn_merge_kernel, knn::MERGE_LDS_MAX>();  // both limits stand before the first launch
  if (e != hipSuccess) return e;
  KnnArgs a;
  a.feats = feats;
  a.bank = bank;
  a.work = work;
  a.N = N;
  a.per = (N + S - 1) / S;
  a.B = B;
  a.P = P;
  a.k = k;
  a.S = S;
  e = launch_lds<knn_partial_kernel, knn::LDS_BYTES>(dim3(bank_sim::query_tiles(B), (unsigned)S), dim3(knn::THREADS),
                                                     knn::LDS_BYTES, s, a);
  if (e != hipSuccess) return e;
  int npow2 = 1;
  while (npow2 < S * k) npow2 <<= 1;
  return launch_lds<knn_merge_kernel, knn::MERGE_LDS_MAX>(dim3((unsigned)B), dim3(knn::THREADS), npow2 * (int)sizeof(float), s,
                                                          work, B, k, S, npow2, scores, topv);
}
