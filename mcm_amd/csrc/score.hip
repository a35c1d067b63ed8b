// score.hip — the fused scoring tail of the hot loop: cosine similarity against the prompt
// bank, temperature softmax, and the score reduction, one launch, [B] floats out.
//
// Replaces reference utils/detection_util.py:232-248:
//   output = image_features @ text_features.T                      (:232)   skinny GEMM
//   smax   = softmax(output / T)                                   (:236)
//   MCM / max-logit: -max(smax) / -max(output)                     (:234,:248)
//   energy : -T * logsumexp(output / T)                            (:239)
//   entropy: scipy.stats.entropy(smax, axis=1)  (natural log)      (:243)
//   var    : -np.var(smax, axis=1)              (ddof = 0)         (:246)
// and removes the reference's [B,K] softmax D2H copy (:236): the similarities of one image
// live only in LDS.  HBM-bound on the image features ([B,P] fp32, read once); the text bank
// ([K,P] fp32, 2 MB at K=1000) is re-read per image from L2 / Infinity Cache with fully
// coalesced 1-KiB wave reads (a wave owns a prompt, lanes split the feature dim).
// All arithmetic fp32 with fp64 block reductions (the sums of K terms), independent of the
// towers' MFMA precision mode.
//
// score_kernel<true> (mcm_score_features_topk) additionally answers WHICH concepts matched: the
// reference leaves that to `np.argmax(smax)` on the [B,K] copy it pulls to the host (:236); here
// the top-k indices and their softmax probabilities come out of the same LDS row, [B,K] still
// never reaches HBM.  score_kernel<false> is the plain tail: no run-time branch separates the two.
#include "common.hpp"

namespace {

constexpr int NWV = 16;  // waves per workgroup: the per-prompt dot products are a dependent
                         // load -> fma -> cross-lane chain, so more waves = shorter chain

__device__ __forceinline__ double block_sum_d(double v, double* red, int lane, int wave) {
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < NWV; ++i) t += red[i];
  return t;
}

// (value, index) pairs under the selection order of the top-k form: value descending, then index
// ascending (numpy.argsort(-sim, kind="stable")); index < 0 = no candidate.  +0.0 == -0.0, so the
// lower index wins between them; a NaN never compares and is never a candidate.
__device__ __forceinline__ void pair_better(float& v, int& i, float ov, int oi) {
  if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) {
    v = ov;
    i = oi;
  }
}

// TOPK: also write the `topk` best-matching bank rows of each image to idx [B,topk] and, with
// prob != nullptr, their softmax(sim/T) to prob [B,topk] (slots without a candidate: -1 / NaN).
// The trailing three parameters are not read by the plain instantiation.
template <bool TOPK>
__global__ __launch_bounds__(NWV * 64) void score_kernel(const float* __restrict__ img,
                                                    const float* __restrict__ text, int K, int P,
                                                    float T, int kind, float* __restrict__ scores,
                                                    int topk, int* __restrict__ idx,
                                                    float* __restrict__ prob) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* f = (float*)smem;        // [P]
  float* sim = f + P;             // [K]
  __shared__ double red[NWV];
  __shared__ float redf[NWV];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int d = tid; d < P; d += NWV * 64) f[d] = img[(size_t)b * P + d];
  __syncthreads();
  for (int k = wave; k < K; k += NWV) {
    const float* t = text + (size_t)k * P;
    float a = 0.f;
    for (int d = lane * 4; d < P; d += 256) {
      const float4 tv = *(const float4*)(t + d);
      const float4 fv = *(const float4*)(f + d);
      a = fmaf(tv.x, fv.x, a);
      a = fmaf(tv.y, fv.y, a);
      a = fmaf(tv.z, fv.z, a);
      a = fmaf(tv.w, fv.w, a);
    }
    a = wave_sum(a);
    if (lane == 0) sim[k] = a;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int k = tid; k < K; k += NWV * 64) m = fmaxf(m, sim[k]);
  m = wave_max(m);
  if (lane == 0) redf[wave] = m;
  __syncthreads();
  m = redf[0];
#pragma unroll
  for (int i = 1; i < NWV; ++i) m = fmaxf(m, redf[i]);
  float selv = 0.f;  // thread r < topk keeps winner r: sim[] is about to be overwritten
  int seli = -1;
  if constexpr (TOPK) {
    // Round r: the block-wide best entry strictly after winner r-1 in the selection order.  No
    // masking, sim[] is left as it is; the 16-entry stage is double-buffered, one barrier a round.
    __shared__ float stv[2][NWV];
    __shared__ int sti[2][NWV];
    float pv = INFINITY;
    int pi = -1;
    for (int r = 0; r < topk; ++r) {
      float bv = 0.f;
      int bi = -1;
      for (int k = tid; k < K; k += NWV * 64) {  // k ascending: a strict > keeps the lower index
        const float v = sim[k];
        if ((v < pv || (v == pv && k > pi)) && (bi < 0 || v > bv)) {
          bv = v;
          bi = k;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        pair_better(bv, bi, ov, oi);
      }
      if (lane == 0) {
        stv[r & 1][wave] = bv;
        sti[r & 1][wave] = bi;
      }
      __syncthreads();
      bv = stv[r & 1][0];
      bi = sti[r & 1][0];
#pragma unroll
      for (int i = 1; i < NWV; ++i) pair_better(bv, bi, stv[r & 1][i], sti[r & 1][i]);
      if (bi < 0) break;  // nothing left (topk > K, or NaNs): the remaining slots stay -1
      if (tid == r) {
        selv = bv;
        seli = bi;
      }
      pv = bv;
      pi = bi;
    }
    if (tid < topk) idx[(size_t)b * topk + tid] = seli;
  }
  if (kind == MCM_SCORE_MAX_LOGIT) {
    if (tid == 0) scores[b] = -m;
    if constexpr (TOPK) {
      if (!prob) return;  // with probabilities the softmax below still runs
    } else {
      return;
    }
  }
  const float mt = m / T;
  double z = 0.0, ez = 0.0;
  for (int k = tid; k < K; k += NWV * 64) {
    const float u = sim[k] / T - mt;
    const float e = expf(u);
    sim[k] = e;
    z += (double)e;
    ez += (double)e * (double)u;
  }
  z = block_sum_d(z, red, lane, wave);
  if constexpr (TOPK) {
    // the same expf(sim/T - max/T) term and the same fp64 z as the score: for MCM on a NaN-free
    // row prob[b,0] = (float)(1.0 / z) = -scores[b], bit for bit
    if (prob && tid < topk)
      prob[(size_t)b * topk + tid] = seli < 0 ? NAN : (float)((double)expf(selv / T - mt) / z);
    if (kind == MCM_SCORE_MAX_LOGIT) return;
  }
  if (kind == MCM_SCORE_MCM) {
    if (tid == 0) scores[b] = -(float)(1.0 / z);          // max softmax = exp(0)/z
  } else if (kind == MCM_SCORE_ENERGY) {
    if (tid == 0) scores[b] = -(T * (mt + (float)log(z)));
  } else if (kind == MCM_SCORE_ENTROPY) {
    ez = block_sum_d(ez, red, lane, wave);                // H = log z - sum(e*u)/z
    if (tid == 0) scores[b] = (float)(log(z) - ez / z);
  } else {                                                // variance of the fp32 softmax
    const float rz = (float)(1.0 / z);
    double s1 = 0.0;
    for (int k = tid; k < K; k += NWV * 64) {
      const float p = sim[k] * rz;
      sim[k] = p;
      s1 += (double)p;
    }
    const double mean = block_sum_d(s1, red, lane, wave) / (double)K;
    double s2 = 0.0;
    for (int k = tid; k < K; k += NWV * 64) {
      const double c = (double)sim[k] - mean;
      s2 += c * c;
    }
    s2 = block_sum_d(s2, red, lane, wave);
    if (tid == 0) scores[b] = (float)(-(s2 / (double)K));
  }
}

// ---- Mahalanobis baseline (reference utils/detection_util.py:176-207, --score maha) ------------
// The reference computes, per class c,  -0.5 * (f - mu_c) P (f - mu_c)^T  with two torch.mm per class
// and keeps the max; the function returns its negation = min_c 0.5 d_c.  Expanded,
//   d_c = f P f^T  -  f . (P mu_c + P^T mu_c)  +  mu_c P mu_c^T  =  q - W_c . f + k_c,
// so per image the work is one P x P quadratic form and C dot products instead of C quadratic
// forms (C = 1000: 500x less).  W and k are prepared once per (means, precision) pair.  The three
// terms nearly cancel when f is close to a class mean, so they are accumulated in fp64.
__global__ __launch_bounds__(256) void maha_prepare_kernel(const float* __restrict__ means,
                                                           const float* __restrict__ prec, int P,
                                                           double* __restrict__ w, double* __restrict__ k) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* mu = (double*)smem;   // [P]
  __shared__ double red[4];
  const int c = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < P; j += 256) mu[j] = (double)means[(size_t)c * P + j];
  __syncthreads();
  double kc = 0.0;
  for (int p = tid; p < P; p += 256) {
    double a = 0.0, b = 0.0;  // (P mu)_p and (P^T mu)_p
    for (int j = 0; j < P; ++j) {
      a += (double)prec[(size_t)p * P + j] * mu[j];
      b += (double)prec[(size_t)j * P + p] * mu[j];
    }
    w[(size_t)c * P + p] = a + b;
    kc += mu[p] * a;
  }
  kc = wave_sum(kc);
  if ((tid & 63) == 0) red[tid >> 6] = kc;
  __syncthreads();
  if (tid == 0) k[c] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(NWV * 64) void maha_score_kernel(const float* __restrict__ feats,
                                                              const float* __restrict__ prec,
                                                              const double* __restrict__ w,
                                                              const double* __restrict__ k, int C, int P,
                                                              float* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* f = (double*)smem;  // [P]
  __shared__ double red[NWV];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < P; j += NWV * 64) f[j] = (double)feats[(size_t)b * P + j];
  __syncthreads();
  double qa = 0.0;  // q = f P f^T: a wave per row of P
  for (int p = wave; p < P; p += NWV) {
    double a = 0.0;
    for (int j = lane; j < P; j += 64) a += (double)prec[(size_t)p * P + j] * f[j];
    a = wave_sum(a);
    if (lane == 0) qa += f[p] * a;
  }
  const double q = block_sum_d(lane == 0 ? qa : 0.0, red, lane, wave);
  double best = INFINITY;
  for (int c = wave; c < C; c += NWV) {
    double a = 0.0;
    for (int j = lane; j < P; j += 64) a += w[(size_t)c * P + j] * f[j];
    a = wave_sum(a);
    best = fmin(best, q - a + k[c]);
  }
  __syncthreads();
  if (lane == 0) red[wave] = best;
  __syncthreads();
  if (tid == 0) {
    double m = red[0];
    for (int i = 1; i < NWV; ++i) m = fmin(m, red[i]);
    scores[b] = (float)(0.5 * m);
  }
}

// ---- Mahalanobis fit: the running statistics of get_mean_prec on the device (mcm_maha_fit_accumulate) -------------
// gram [P,P] += sum_b x_b x_b^T and sum [P] += sum_b x_b over the B rows of feats, x_b = (double)f_b - (double)shift.
// The covariance is finalised on the host from (gram, sum, n); the shift (the first batch's column mean) keeps
// gram - sum sum^T / n from cancelling when the features sit far from the origin.
// One workgroup owns one FT x FT tile of the UPPER triangle of gram and walks all B rows, so an element's value is the
// recurrence acc = fma(x_bi, x_bj, acc) over b in row order, started from the value gram already holds: no atomics, no
// split of the B loop, and the same bits whether the rows arrive in one call or in several.  The tile's mirror image
// is written from the same accumulators (gram[j][i] = gram[i][j] bit for bit; what the caller held in the lower
// triangle is overwritten).  The workgroups of the diagonal tiles also carry their FT elements of sum, row by row.
// A thread accumulates a 4 x 4 set of elements, rows ty + 16 r and columns tx + 16 c of the tile: the 16 lanes of a row
// read 16 consecutive doubles of a staged feature row (no bank conflicts), the row operand is a broadcast.
constexpr int FT = 64;  // tile edge
constexpr int FK = 32;  // feature rows staged per step: 2 panels x FK x FT doubles = 32 KiB of LDS

__global__ __launch_bounds__(256) void maha_fit_kernel(const float* __restrict__ feats, int B, int P,
                                                       const float* __restrict__ shift, double* __restrict__ gram,
                                                       double* __restrict__ sum) {
  __shared__ double xs[2][FK][FT];  // the shifted rows of this step: columns of tile-row ti, of tile-column tj
  const int nt = (P + FT - 1) / FT;
  int idx = blockIdx.x, ti = 0;     // blockIdx.x counts the upper-triangle tiles row by row
  while (idx >= nt - ti) {
    idx -= nt - ti;
    ++ti;
  }
  const int tj = ti + idx;
  const bool diag = ti == tj;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  // staging: a thread converts column sc of both panels, rows sr, sr + 4, ... of the step
  const int sc = tid & 63, sr = tid >> 6;
  const int ci = ti * FT + sc, cj = tj * FT + sc;
  const double shi = (shift && ci < P) ? (double)shift[ci] : 0.0;
  const double shj = (shift && cj < P) ? (double)shift[cj] : 0.0;
  const double(*xi)[FT] = xs[0];
  const double(*xj)[FT] = diag ? xs[0] : xs[1];

  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = ti * FT + ty + 16 * r, j = tj * FT + tx + 16 * c;
      acc[r][c] = (i < P && j < P && i <= j) ? gram[(size_t)i * P + j] : 0.0;
    }
  const bool sums = diag && tid < FT;  // wave 0 of a diagonal tile: sum[ci]
  double s = (sums && ci < P) ? sum[ci] : 0.0;

  float ri[FK / 4], rj[FK / 4];
  auto fetch = [&](int b0) {  // rows past B and columns past P read as 0 (neither is used: see the k loop, the stores)
#pragma unroll
    for (int m = 0; m < FK / 4; ++m) {
      const int b = b0 + sr + 4 * m;
      ri[m] = (b < B && ci < P) ? feats[(size_t)b * P + ci] : 0.f;
      rj[m] = (!diag && b < B && cj < P) ? feats[(size_t)b * P + cj] : 0.f;
    }
  };
  fetch(0);
  for (int b0 = 0; b0 < B; b0 += FK) {
    __syncthreads();  // the previous step's readers are done
#pragma unroll
    for (int m = 0; m < FK / 4; ++m) {
      xs[0][sr + 4 * m][sc] = ci < P ? (double)ri[m] - shi : 0.0;
      if (!diag) xs[1][sr + 4 * m][sc] = cj < P ? (double)rj[m] - shj : 0.0;
    }
    __syncthreads();
    if (b0 + FK < B) fetch(b0 + FK);  // the next step's rows travel while this one is multiplied
    const int kmax = min(FK, B - b0);
    for (int k = 0; k < kmax; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = xi[k][ty + 16 * r];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = xj[k][tx + 16 * c];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
    }
    if (sums)
      for (int k = 0; k < kmax; ++k) s += xi[k][sc];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = ti * FT + ty + 16 * r, j = tj * FT + tx + 16 * c;
      if (i < P && j < P && i <= j) {  // (a diagonal tile's lower half was computed for nothing: its mirror writes it)
        gram[(size_t)i * P + j] = acc[r][c];
        if (i != j) gram[(size_t)j * P + i] = acc[r][c];
      }
    }
  if (sums && ci < P) sum[ci] = s;
}

}  // namespace

hipError_t launch_maha_fit(const float* feats, int B, int P, const float* shift, double* gram, double* sum,
                           hipStream_t s) {
  if (B <= 0 || P <= 0 || P > 4096 || !feats || !gram || !sum) return hipErrorInvalidValue;
  const int nt = (P + FT - 1) / FT;
  hipLaunchKernelGGL(maha_fit_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, feats, B, P, shift, gram, sum);
  return hipGetLastError();
}

hipError_t launch_maha_prepare(const float* means, const float* prec, int C, int P, double* w, double* c,
                               hipStream_t s) {
  if (C <= 0 || P <= 0 || P > 4096) return hipErrorInvalidValue;
  hipLaunchKernelGGL(maha_prepare_kernel, dim3(C), dim3(256), P * sizeof(double), s, means, prec, P, w, c);
  return hipGetLastError();
}

hipError_t launch_maha_score(const float* feats, int B, const float* prec, const double* w, const double* c,
                             int C, int P, float* scores, hipStream_t s) {
  if (B <= 0 || C <= 0 || P <= 0 || P > 4096) return hipErrorInvalidValue;
  hipLaunchKernelGGL(maha_score_kernel, dim3(B), dim3(NWV * 64), P * sizeof(double), s, feats, prec, w, c, C,
                     P, scores);
  return hipGetLastError();
}

hipError_t launch_score(const float* img, int B, const float* text, int K, int P, float T, int kind,
                        float* scores, hipStream_t s) {
  if (B <= 0 || K <= 0 || P % 4 || kind < 0 || kind > MCM_SCORE_VAR || !(T > 0.f))
    return hipErrorInvalidValue;
  const int lds = (P + K) * (int)sizeof(float);
  return launch_lds<score_kernel<false>, MCM_SCORE_LDS_MAX_BYTES>(dim3(B), dim3(NWV * 64), lds, s, img, text, K, P, T, kind, scores, 0,
                                                     (int*)nullptr, (float*)nullptr);
}

bool score_shape_ok(int K, int P) { return K > 0 && P > 0 && P % 4 == 0 && (int64_t)(P + (int64_t)K) * 4 <= MCM_SCORE_LDS_MAX_BYTES; }

hipError_t launch_score_topk(const float* img, int B, const float* text, int K, int P, float T, int kind,
                             int topk, float* scores, int* idx, float* prob, hipStream_t s) {
  if (B <= 0 || !score_shape_ok(K, P) || kind < 0 || kind > MCM_SCORE_VAR || !(T > 0.f) || topk < 1 ||
      topk > MCM_TOPK_MAX || !scores || !idx)
    return hipErrorInvalidValue;
  const int lds = (P + K) * (int)sizeof(float);
  return launch_lds<score_kernel<true>, MCM_SCORE_LDS_MAX_BYTES>(dim3(B), dim3(NWV * 64), lds, s, img, text, K, P, T, kind, scores, topk, idx,
                                                    prob);
}
