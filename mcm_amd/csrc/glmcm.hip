// glmcm.hip — the local term of GL-MCM (include/mcm.h mcm_local_score_features): for every patch row of
// every image the largest softmax probability over the K prompts of the bank, and per image the largest of its R rows,
// without the [B R, K] matrix ever existing in HBM.  The B R patch rows are the queries of the bank walk and the K
// prompts its bank; images do not align with the walk's 64-query tiles, so the per-image maximum is a launch of its own.
//   glm_rows_kernel    grid (query tiles of 64 rows of [B R, P]).  A workgroup walks the whole bank (bank_sim.hpp: the
//                      64 x 256 exact-fp32 similarities of a tile in LDS, the s[b, n] that knn.hip and neglabel.hip see);
//                      a wave per query folds every tile into the row's open pair (bank_sim::lse_fold: max,
//                      sum exp((s - max) / T) in fp64).  At the end row[q] = (float)(1 / sum): the softmax's largest
//                      probability.
//   glm_image_kernel   one workgroup per image: the maximum of its R row values, NaN if any of them is NaN.
// Nothing is combined across workgroups by atomics, no workgroup waits for another, every loop is bounded by the
// arguments; every row's value is one fixed computation wherever the row falls, and a maximum has no order.
// glm_compact_kernel is the last launch of the tower's local pass (mcm_api.hip local_pass): projected token rows
// [B ntok, P] -> unit-norm patch rows [B, R, P], token 0 of every image dropped.
#include <limits.h>
#include <math.h>

#include "bank_sim.hpp"

namespace {

namespace glm {
using namespace bank_sim;
constexpr int LDS_BYTES = TILE_BYTES + PAIR_BYTES;  // behind the tile: the open pair of every query
constexpr int IMG_THREADS = 256;
}  // namespace glm

struct GlmArgs {
  const float* rows;  // [M, P] the patch rows, M = B R
  const float* bank;  // [K, P]
  float* val;         // [M] the row values (the workspace)
  float* patch;       // [M] a second copy for the caller, or nullptr
  double inv_t;       // 1 / (double) T
  int M, P, K;
};

__global__ __launch_bounds__(glm::THREADS) void glm_rows_kernel(GlmArgs a) {
  using namespace glm;
  extern __shared__ __attribute__((aligned(16))) float glm_lds[];
  double* st_sum = pair_sums(glm_lds);
  float* st_max = pair_maxima(st_sum);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q0 = blockIdx.x * Q;  // M <= INT_MAX
  const int nq = a.M - q0 < Q ? a.M - q0 : Q;

  if (tid < Q) pair_reset(tid, st_sum, st_max);
  __syncthreads();

  // either zero gives the same bits in everything below: the tile is taken as the MFMA left it
  walk<false>(a.rows, a.bank, a.P, q0, nq, 0, (int64_t)a.K, glm_lds, [=](int64_t, int ncols) {
    for (int qi = 0; qi < Q / 4; ++qi) {  // wave w owns queries 16 w .. 16 w + 15, their open pairs included
      const int q = w * (Q / 4) + qi;
      if (q >= nq) break;
      const float* row = glm_lds + q * LDSIM;
      float m = st_max[q];
      double sum = st_sum[q];
      lse_fold(row, 0, ncols, lane, a.inv_t, m, sum);
      if (lane == 0) {
        st_max[q] = m;
        st_sum[q] = sum;
      }
    }
  });
  __syncthreads();
  if (tid < nq) {
    // the row's maximum contributes exp(0) = 1, so a finite sum is >= 1; a NaN similarity made it NaN
    const float v = (float)(1.0 / st_sum[tid]);
    a.val[q0 + tid] = v;
    if (a.patch) a.patch[q0 + tid] = v;
  }
}

// scores[b] = -max_i val[b R + i], NaN where a row value is NaN (fmaxf would skip it)
__global__ __launch_bounds__(glm::IMG_THREADS) void glm_image_kernel(const float* val, int R, float* scores) {
  __shared__ float red[glm::IMG_THREADS];
  __shared__ int bad[glm::IMG_THREADS];
  const int tid = threadIdx.x;
  const float* v = val + (int64_t)blockIdx.x * R;
  float mx = -INFINITY;
  int nan = 0;
  for (int i = tid; i < R; i += glm::IMG_THREADS) {
    const float x = v[i];
    nan |= x != x;
    mx = fmaxf(mx, x);
  }
  red[tid] = mx;
  bad[tid] = nan;
  __syncthreads();
  for (int off = glm::IMG_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) {
      red[tid] = fmaxf(red[tid], red[tid + off]);
      bad[tid] |= bad[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) scores[blockIdx.x] = bad[0] ? __builtin_nanf("") : -red[0];
}

// out[b, i, :] = y[b ntok + 1 + i, :] / |y row|, one wave per patch row; the rule of the global rows (embed.hip
// pool_project_kernel): the sum of squares in fp32, the row times 1 / sqrtf of it, a zero row not treated specially
__global__ __launch_bounds__(256) void glm_compact_kernel(const float* y, float* out, int64_t rows, int R, int ntok, int P) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int64_t b = r / R;
  const float* src = y + (b * ntok + 1 + (r - b * R)) * (int64_t)P;
  float ss = 0.f;
  for (int c = lane * 4; c < P; c += 256) {  // P % 4 == 0
    const float4 v = *(const float4*)(src + c);
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  ss = wave_sum(ss);
  const float inv = 1.0f / sqrtf(ss);
  float* dst = out + r * (int64_t)P;
  for (int c = lane * 4; c < P; c += 256) {
    const float4 v = *(const float4*)(src + c);
    *(float4*)(dst + c) = float4{v.x * inv, v.y * inv, v.z * inv, v.w * inv};
  }
}

// out[b] = g[b] + lambda l[b], formed in fp64 (the product and the sum are exact or rounded once there) and rounded to fp32
__global__ __launch_bounds__(256) void glm_combine_kernel(const float* g, const float* l, double lambda, float* out, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) out[b] = (float)((double)g[b] + lambda * (double)l[b]);
}

}  // namespace

hipError_t launch_local_combine(const float* g, const float* l, float lambda, float* out, int B, hipStream_t s) {
  if (B < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(glm_combine_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, g, l, (double)lambda, out, B);
  return hipGetLastError();
}

int64_t local_work_bytes(int B, int R) { return (int64_t)B * R * (int64_t)sizeof(float); }

hipError_t launch_local_score(const float* rows, int B, int R, const float* bank, int K, int P, float T, void* work,
                              float* scores, float* patch, hipStream_t s) {
  if (B < 1 || R < 1 || K < 1 || P < 4 || P % 4 || (int64_t)B * R > INT_MAX || !(T > 0.f) || !isfinite(T))
    return hipErrorInvalidValue;
  GlmArgs a;
  a.rows = rows;
  a.bank = bank;
  a.val = (float*)work;
  a.patch = patch;
  a.inv_t = 1.0 / (double)T;
  a.M = B * R;
  a.P = P;
  a.K = K;
  const hipError_t e =
      launch_lds<glm_rows_kernel, glm::LDS_BYTES>(dim3(bank_sim::query_tiles(a.M)), dim3(glm::THREADS), glm::LDS_BYTES, s, a);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(glm_image_kernel, dim3((unsigned)B), dim3(glm::IMG_THREADS), 0, s, (const float*)work, R, scores);
  return hipGetLastError();
}

hipError_t launch_local_compact(const float* y, float* out, int B, int ntok, int P, hipStream_t s) {
  const int R = ntok - 1;
  if (B < 1 || R < 1 || P < 4 || P % 4) return hipErrorInvalidValue;
  const int64_t rows = (int64_t)B * R;
  hipLaunchKernelGGL(glm_compact_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, y, out, rows, R, ntok, P);
  return hipGetLastError();
}
