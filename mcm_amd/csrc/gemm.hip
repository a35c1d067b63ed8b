// gemm.hip — Y[M,N] = X[M,K] · W[N,K]^T (+bias, fused epilogues) on gfx950 MFMA.
//
// Replaces every nn.Linear of the CLIP towers (HF modeling_clip.py:309-311 q/k/v as one
// concatenated [3D,D] weight, :333 out_proj, :347-349 fc1/fc2) and the patch-embedding
// conv (:148-154, non-overlapping patches = a GEMM over gathered rows).  X and W are both
// K-contiguous ("B^T input"), so A- and B-fragments are read from LDS the same way.
//
// One K-step = 128 bytes of K per row (64 bf16 or 32 fp32), so the LDS image, the staging
// code and the fragment reads are identical for both precisions:
//   bf16: 2 x v_mfma_f32_16x16x32_bf16 per fragment pair and K-step
//   fp32: 8 x v_mfma_f32_16x16x4_f32   (exact fp32 = fmaf chain; the parity arm)
// Global→LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave instruction), issued from
// inline asm and counted by hand (common.hpp glds16: the builtin form makes hipcc drain
// vmcnt(0) before every ds_read, i.e. no load/MFMA overlap at all).
//
// LDS layout (per operand tile, R rows x 128 B): rows are paired into 256-B bank rows and
// the 16-B chunk index is XORed with the pair index, so the four 16-lane groups of a
// ds_read_b128 fragment read (16 rows x one chunk) hit 16 distinct 16-B slots:
//   off(r, c) = (r>>1)*256 + ((((r&1)<<3) | ((c ^ (r>>1)) & 7)) << 4)
// LDS-DMA writes lane-linear, so the permutation is applied to each lane's *global*
// source address (guide rule 21: linear dest + inverse-swizzled source + swizzled read).
//
// MFMA operand order is swapped (W fragment as A, X fragment as B) so each lane ends up
// with 4 consecutive output columns of one row: 16-B fp32 / 8-B bf16 epilogue accesses.
//
// The shipped library holds four kernels that share the fragment/epilogue arithmetic and are bit-identical
// on the same inputs (which one runs is a size decision, launch_one):
//   gemm_tile_kernel     128x128 tile, 4 waves, 2 LDS stages, one workgroup per tile,
//                        2 workgroups/CU.  Small problems (text tower, CLS-only last layer, tests).
//   gemm_tile64_kernel   the same with 64x128 tiles: problems that give the 128x128 kernel fewer than two workgroups
//                        per CU (batch <= 32, B/32's short sequences).
//   gemm_p256_kernel     256x256 tile, 8 waves (2x4, 128x64 wave tiles), two 64-KiB stages + a
//                        4-KiB epilogue window per wave (160 KiB), persistent (one workgroup per CU).
//                        Tiles are dealt XCD-first (an XCD's 32 CUs share X row panels in their
//                        private L2), the two waves of a SIMD take turns refilling, whole-row
//                        epilogue stores are streamed (nt).  Takes the large problems with edge tiles.
//   gemm_pp_kernel       the same tile with the "ping-pong" K-loop (the two waves of a SIMD half a K-step
//                        apart): large problems made of whole tiles, i.e. every vision GEMM at batch
//                        256 / 512.  Measurements and what bounds it: DESIGN.md sections 4.1, 5.1, 5.4.
// Split weights (GemmArgs::ksplit, include/mcm.h MCM_WEIGHTS_*): W as W_hi + W_lo, stored K-step-interleaved; every
// kernel stages the X K-step s / 2 with W K-step s, so acc = X W_hi^T + X W_lo^T runs through the unchanged K loop
// (twice the steps; X is re-staged from L2 for the lo step: no third LDS stage, no extra registers).
// A whole-tile problem whose tile count ends in a thin last round of the persistent grid is cut in two launches
// (launch_gemm, "Sliver round"): ping-pong kernel for the rows of the whole rounds, tile kernel for the rest.
// Every arm that was built, measured and not shipped — the 256x128 persistent kernel, the ping-pong loop on 32x32x16
// MFMAs, balanced DMA, staggered epilogues, the LayerNorm fold and the LayerNorm tail, the ablation bits — lives in
// gemm_arms.hpp, which this file includes only in the A/B builds (-DMCM_HARNESS: libmcm_hip_harness.so and
// tools/gemm_bench; -DMCM_LN_FOLD / -DMCM_LN_TAIL): the shipped library holds the four kernels below and nothing else.
#include <type_traits>

#include "common.hpp"
#include "ln_row.hpp"

namespace {

constexpr int ROWB = 128;  // bytes of K per row per K-step

// K-step kt of a kernel's loop -> byte offsets of the X and W K-steps it stages (GemmArgs::ksplit, xsplit: common.hpp).
// Plain operands: both kt.  Split weights: X step kt / 2 against W steps kt (hi, lo interleaved).  Split activations: the
// mirror image.  Both: four passes per logical step t = kt / 4 — (X_hi, W_hi), (X_lo, W_hi), (X_hi, W_lo), (X_lo, W_lo).
// All scalar (kt is uniform).
__device__ __forceinline__ void kstep_off(const GemmArgs& a, int kt, size_t& kox, size_t& kow) {
  const int t = kt >> (a.ksplit + a.xsplit);
  kox = (size_t)((t << a.xsplit) | (kt & a.xsplit)) * ROWB;
  kow = (size_t)((t << a.ksplit) | ((kt >> a.xsplit) & a.ksplit)) * ROWB;
}
// K-steps of the loop: the W image's steps (a.K counts its columns, hi and lo of a split weight included), twice that for a
// split X
__device__ __forceinline__ int ksteps(const GemmArgs& a, int es) { return ((a.K * es) / ROWB) << a.xsplit; }

#if defined(MCM_HARNESS) || defined(MCM_LN_FOLD) || defined(MCM_LN_TAIL)
#define MCM_ARMS 1  // A/B builds: gemm_arms.hpp is compiled in (below, in front of the launch section)
#endif

__device__ __forceinline__ int frag_off(int fr, int g, int kk) {
  return (fr >> 1) * 256 + ((((fr & 1) << 3) | (((kk * 4 + g) ^ (fr >> 1)) & 7)) << 4);
}

// one 32-wide K half (kk = 0 / 1) of a K-step of a (MF*16)x64 wave tile: MF x 4 fragments,
// operands at xs / ws (+ f*2048 per 16 rows); x fragments are consumed four at a time to bound
// live registers
template <int PREC, int MF>
__device__ __forceinline__ void wave_khalf(const char* xs, const char* ws, int foff, f32x4_t (&acc)[4][MF]) {
  uint4 wf[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) wf[f] = *(const uint4*)(ws + f * 2048 + foff);
#pragma unroll
  for (int h = 0; h < MF / 4; ++h) {
    uint4 xf[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) xf[f] = *(const uint4*)(xs + (h * 4 + f) * 2048 + foff);
#pragma unroll
    for (int fj = 0; fj < 4; ++fj)
#pragma unroll
      for (int fq = 0; fq < 4; ++fq) {
        const int fi = h * 4 + fq;
        if constexpr (PREC != MCM_PREC_F32) {
          acc[fj][fi] = mfma16<PREC>(wf[fj], xf[fq], acc[fj][fi]);
        } else {
          const f32x4_t wv = __builtin_bit_cast(f32x4_t, wf[fj]);
          const f32x4_t xv = __builtin_bit_cast(f32x4_t, xf[fq]);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[fj][fi] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[t], xv[t], acc[fj][fi], 0, 0, 0);
        }
      }
  }
}
template <int PREC, int MF>
__device__ __forceinline__ void wave_kstep(const char* xs, const char* ws, const int (&foff)[2],
                                           f32x4_t (&acc)[4][MF]) {
  wave_khalf<PREC, MF>(xs, ws, foff[0], acc);
  wave_khalf<PREC, MF>(xs, ws, foff[1], acc);
}

// W rows are staged into LDS in a permuted order (perm_n below) so that, after the MFMAs, a
// lane holds 16 CONSECUTIVE output columns of one row: fragment fj, accumulator register r
// of lane (fr, g) is column  nw + g*16 + fj*4 + r.  The epilogue then moves 32 B (bf16) /
// 64 B (fp32) contiguous per lane and the 4 g-lanes of a row cover whole 128-B lines.
// LDS row lr (0..63 inside a wave's 64-column panel) holds tile column perm_n(lr).
__device__ __forceinline__ int perm_n(int lr) {
  return ((lr >> 2) & 3) * 16 + (lr >> 4) * 4 + (lr & 3);
}

// epilogue of a (MF*16)x64 wave tile at (mw, nw)
template <int PREC, int EPI, int MF>
__device__ __forceinline__ void wave_epilogue(const GemmArgs& a, const f32x4_t (&acc)[4][MF],
                                              const f32x4_t (&bv)[4], int mw, int nw, int fr, int g, float& amax) {
  const int n = nw + g * 16;
  if (n >= a.N) return;
#pragma unroll
  for (int fi = 0; fi < MF; ++fi) {
    const int m = mw + fi * 16 + fr;
    if (m >= a.M) continue;
    f32x4_t v[4];
#pragma unroll
    for (int fj = 0; fj < 4; ++fj) {
      v[fj] = acc[fj][fi] + bv[fj];
      if constexpr (epi_gelu(EPI)) {  // same form in every kernel variant: results must not
#pragma unroll                        // depend on which variant the size heuristic picks
        for (int t = 0; t < 4; ++t)
          v[fj][t] = epi_erf(EPI)                                ? gelu_erf(v[fj][t])
                     : (PREC != MCM_PREC_F32 && !epi_x2(EPI)) ? quick_gelu_fast(v[fj][t])
                                                              : quick_gelu(v[fj][t]);
      }
    }
    if constexpr (epi_x2(EPI)) {  // split image: the lane's 16 columns as hi[16] at split_col(n), lo[16] 64 elements on
      uint32_t hi[8], lo[8];
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) {
        sat_track<PREC>(amax, v[fj][0], v[fj][1]);
        sat_track<PREC>(amax, v[fj][2], v[fj][3]);
        split2<PREC>(v[fj][0], v[fj][1], hi[2 * fj], lo[2 * fj]);
        split2<PREC>(v[fj][2], v[fj][3], hi[2 * fj + 1], lo[2 * fj + 1]);
      }
      uint4* dst = (uint4*)((uint16_t*)a.out + (size_t)m * a.ldo + split_col(n));
      dst[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
      dst[1] = make_uint4(hi[4], hi[5], hi[6], hi[7]);
      dst[8] = make_uint4(lo[0], lo[1], lo[2], lo[3]);   // + 64 elements = 8 x 16 B
      dst[9] = make_uint4(lo[4], lo[5], lo[6], lo[7]);
    } else if constexpr (EPI == EPI_RESID) {
      f32x4_t* dst = (f32x4_t*)(a.resid + (size_t)m * a.ldo + n);
      f32x4_t r[4];
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) r[fj] = dst[fj];
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) dst[fj] = r[fj] + v[fj];
    } else if constexpr (EPI == EPI_PATCH) {
      const int b = m / a.np, p = m - b * a.np;
      f32x4_t* dst = (f32x4_t*)((float*)a.out + (size_t)(b * (a.np + 1) + 1 + p) * a.ldo + n);
      const f32x4_t* pr = (const f32x4_t*)(a.pos + (size_t)(1 + p) * a.N + n);
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) dst[fj] = v[fj] + pr[fj];
    } else if constexpr (PREC != MCM_PREC_F32) {
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) {
        sat_track<PREC>(amax, v[fj][0], v[fj][1]);
        sat_track<PREC>(amax, v[fj][2], v[fj][3]);
      }
      uint4* dst = (uint4*)((uint16_t*)a.out + out16_off(a, m, n));
      dst[0] = make_uint4(pack2<PREC>(v[0][0], v[0][1]), pack2<PREC>(v[0][2], v[0][3]),
                          pack2<PREC>(v[1][0], v[1][1]), pack2<PREC>(v[1][2], v[1][3]));
      dst[1] = make_uint4(pack2<PREC>(v[2][0], v[2][1]), pack2<PREC>(v[2][2], v[2][3]),
                          pack2<PREC>(v[3][0], v[3][1]), pack2<PREC>(v[3][2], v[3][3]));
    } else {
      f32x4_t* dst = (f32x4_t*)((float*)a.out + (size_t)m * a.ldo + n);
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) dst[fj] = v[fj];
    }
  }
}

// LDS-staged epilogue of a (MF*16)x64 wave tile (persistent 256x256 kernel).  Row-per-lane
// stores at a row stride reach only ~12 B/clk/CU on this chip (each store instruction touches
// 16 partial lines), which made the epilogue cost as much as 40 % of a K=768 tile.  Here each
// wave bounces its tile through a private 4-KiB LDS window (XOR-swizzled, conflict-free both
// ways) and writes whole rows: one store instruction = 8 full 128-B lines (bf16) or 4 x 256 B
// (fp32).  The fp32 residual form reads the matching rows the same way, one chunk ahead.
// 16-byte global store; `stream` adds the non-temporal hint.  A tile round of the persistent
// kernels writes 4 MiB per XCD — the whole L2 — so write-back-allocated output lines evict the
// X / W panels the next K-loop is about to re-read; streamed lines do not (+9 % on the QKV shape).
template <typename V>
__device__ __forceinline__ void store16_stream(void* p, const V& v) {
  typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
  static_assert(sizeof(V) == 16, "16-byte payload");
  const u32x4_t vv = __builtin_bit_cast(u32x4_t, v);
  // s_nop 1: a store of more than 64 bits must be 2 wait states away from a VALU write of its data
  // registers on gfx940+; hipcc pads its own stores but cannot see inside this asm (without the
  // pad, rows of garbage appeared whenever the TA was slow to pick the data up)
  asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(p), "v"(vv) : "memory");
}

// the same with a scalar base and a 32-bit lane offset (bytes)
template <typename V>
__device__ __forceinline__ void store16_stream_s(const void* sbase, uint32_t voff, const V& v) {
  typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
  static_assert(sizeof(V) == 16, "16-byte payload");
  const u32x4_t vv = __builtin_bit_cast(u32x4_t, v);
  asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" ::"v"(voff), "v"(vv), "s"(sbase) : "memory");
}

// INTERIOR (16-bit outputs only; the ping-pong kernel): the caller guarantees a full tile and uniform mw / nw;
// rows are then addressed as a uniform base plus one 32-bit lane offset, without bounds checks.
template <int PREC, int EPI, int MF, bool INTERIOR = false>
__device__ __forceinline__ void wave_epilogue_lds(const GemmArgs& a, const f32x4_t (&acc)[4][MF],
                                                  const f32x4_t (&bv)[4], int mw, int nw, int lane,
                                                  char* scratch, float& amax) {
  const int fr = lane & 15, g = lane >> 4;
  if constexpr (PREC != MCM_PREC_F32 && epi_x2(EPI)) {
    // Split outputs (the re-scoring arm): per 16-row unit the hi image goes through the window's first 2-KiB half and the
    // lo image through the second, then both are read back and stored as whole 128-B segments — hi at split_col(nw), lo
    // right behind it (the wave's 64 columns are exactly one K-step of the consumer).  No overlap between units: this arm
    // re-scores a few hundred images, the store pattern matters, the last 10 % of the epilogue do not.
    const int rrow = lane >> 3, c8 = lane & 7;
    const int sw = fr & 7;
#pragma unroll
    for (int u = 0; u < MF; ++u) {
      uint32_t hi[8], lo[8];
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) {
        f32x4_t v = acc[fj][u] + bv[fj];
        if constexpr (epi_gelu(EPI)) {
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = epi_erf(EPI) ? gelu_erf(v[t]) : quick_gelu(v[t]);
        }
        sat_track<PREC>(amax, v[0], v[1]);
        sat_track<PREC>(amax, v[2], v[3]);
        split2<PREC>(v[0], v[1], hi[2 * fj], lo[2 * fj]);
        split2<PREC>(v[2], v[3], hi[2 * fj + 1], lo[2 * fj + 1]);
      }
      char* w = scratch + fr * 128;
      *(uint4*)(w + (((g * 2) ^ sw) << 4)) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
      *(uint4*)(w + (((g * 2 + 1) ^ sw) << 4)) = make_uint4(hi[4], hi[5], hi[6], hi[7]);
      *(uint4*)(w + 2048 + (((g * 2) ^ sw) << 4)) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
      *(uint4*)(w + 2048 + (((g * 2 + 1) ^ sw) << 4)) = make_uint4(lo[4], lo[5], lo[6], lo[7]);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int row = t * 8 + rrow, m = mw + u * 16 + row;
        const uint4 rh = *(const uint4*)(scratch + row * 128 + ((c8 ^ (row & 7)) << 4));
        const uint4 rl = *(const uint4*)(scratch + 2048 + row * 128 + ((c8 ^ (row & 7)) << 4));
        if (INTERIOR || (m < a.M && nw + c8 * 8 < a.N)) {
          uint16_t* dst = (uint16_t*)a.out + (size_t)m * a.ldo + split_col(nw) + c8 * 8;
          store16_stream(dst, rh);
          store16_stream(dst + 64, rl);
        }
      }
    }
  } else if constexpr (PREC != MCM_PREC_F32 && epi_plain16(EPI)) {
    // 16-row units ping-pong between the two 2-KiB halves of the window: unit u is converted and
    // written while unit u-1 is read back and stored, so the LDS round trip and the store issue
    // (a 1-KiB store blocks its wave like an LDS-DMA piece does) overlap the next unit's VALU work.
    const int rrow = lane >> 3, c8 = lane & 7;  // read-back: 8 lanes per 128-B row
    const int n = nw + c8 * 8;
    auto write_unit = [&](int u) {
      f32x4_t v[4];
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) {
        v[fj] = acc[fj][u] + bv[fj];
        if constexpr (epi_gelu(EPI)) {
#pragma unroll
          for (int t = 0; t < 4; ++t) v[fj][t] = epi_erf(EPI) ? gelu_erf(v[fj][t]) : quick_gelu_fast(v[fj][t]);
        }
        sat_track<PREC>(amax, v[fj][0], v[fj][1]);
        sat_track<PREC>(amax, v[fj][2], v[fj][3]);
      }
      char* w = scratch + (u & 1) * 2048 + fr * 128;
      const int sw = fr & 7;
      *(uint4*)(w + (((g * 2) ^ sw) << 4)) =
          make_uint4(pack2<PREC>(v[0][0], v[0][1]), pack2<PREC>(v[0][2], v[0][3]),
                     pack2<PREC>(v[1][0], v[1][1]), pack2<PREC>(v[1][2], v[1][3]));
      *(uint4*)(w + (((g * 2 + 1) ^ sw) << 4)) =
          make_uint4(pack2<PREC>(v[2][0], v[2][1]), pack2<PREC>(v[2][2], v[2][3]),
                     pack2<PREC>(v[3][0], v[3][1]), pack2<PREC>(v[3][2], v[3][3]));
    };
    auto read_unit = [&](int u, uint4 (&r)[2]) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int row = t * 8 + rrow;
        r[t] = *(const uint4*)(scratch + (u & 1) * 2048 + row * 128 + ((c8 ^ (row & 7)) << 4));
      }
    };
    // head-major outputs (a.hm): the wave's 64 columns are one head's block, whose rows are 128 B apart
    const int ldo_e = MCM_HM(a.hm) ? 64 : a.ldo;
    const int lane_off = rrow * ldo_e + c8 * 8;  // elements
    // INTERIOR: scalar base + one 32-bit lane offset; the base walks down the tile 8 rows per store (two scalar adds
    // per store instead of a 64-bit multiply-add chain and a vector 64-bit add)
    const char* sp = (const char*)a.out + out16_off(a, mw, nw) * 2;
    const size_t sp_step = (size_t)ldo_e * 16;  // bytes per 8 rows
    auto store_unit = [&](int u, const uint4 (&r)[2]) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if constexpr (INTERIOR) {
          store16_stream_s(sp, (uint32_t)lane_off * 2u, r[t]);
          sp += sp_step;
        } else {
          const int m = mw + u * 16 + t * 8 + rrow;
          if (m < a.M && n < a.N) store16_stream((uint16_t*)a.out + out16_off(a, m, n), r[t]);
        }
      }
    };
    write_unit(0);
#pragma unroll
    for (int u = 1; u < MF; ++u) {
      uint4 r[2];
      read_unit(u - 1, r);
      write_unit(u);
      store_unit(u - 1, r);
    }
    {
      uint4 r[2];
      read_unit(MF - 1, r);
      store_unit(MF - 1, r);
    }
  } else {
    // fp32 rows: chunk = 16 rows x 256 B, 16 lanes per row
    const int rrow = lane >> 4, c16 = lane & 15;
    const int n = nw + c16 * 4;
    const bool ncol = n < a.N;
    f32x4_t rnext[4];
    auto row_ptr = [&](int c, int t, bool& ok) -> float* {
      const int m = mw + c * 16 + t * 4 + rrow;
      ok = ncol && m < a.M;
      if constexpr (EPI == EPI_PATCH) {
        const int mm = min(m, a.M - 1), b = mm / a.np, p = mm - b * a.np;
        return (float*)a.out + (size_t)(b * (a.np + 1) + 1 + p) * a.ldo + n;
      } else if constexpr (EPI == EPI_RESID) {
        return a.resid + (size_t)m * a.ldo + n;
      } else {
        return (float*)a.out + (size_t)m * a.ldo + n;
      }
    };
    auto prefetch = [&](int c) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        bool ok;
        const float* ptr;
        if constexpr (EPI == EPI_PATCH) {
          const int m = min(mw + c * 16 + t * 4 + rrow, a.M - 1);
          const int p = m - (m / a.np) * a.np;
          ok = ncol;
          ptr = a.pos + (size_t)(1 + p) * a.N + n;
        } else {
          ptr = row_ptr(c, t, ok);
        }
        rnext[t] = ok ? *(const f32x4_t*)ptr : (f32x4_t){0.f, 0.f, 0.f, 0.f};
      }
    };
    constexpr bool ADD = (EPI == EPI_RESID || EPI == EPI_PATCH);
    if constexpr (ADD) prefetch(0);
#pragma unroll
    for (int c = 0; c < MF; ++c) {
      f32x4_t r[4];
      if constexpr (ADD) {
#pragma unroll
        for (int t = 0; t < 4; ++t) r[t] = rnext[t];
        if (c + 1 < MF) prefetch(c + 1);
      }
      const int sw = fr;  // row = fr inside the chunk
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) {
        f32x4_t v = acc[fj][c] + bv[fj];
        if constexpr (epi_gelu(EPI)) {
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = epi_erf(EPI) ? gelu_erf(v[t]) : quick_gelu(v[t]);
        }
        *(f32x4_t*)(scratch + fr * 256 + (((g * 4 + fj) ^ sw) << 4)) = v;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int row = t * 4 + rrow;
        f32x4_t v = *(const f32x4_t*)(scratch + row * 256 + ((c16 ^ row) << 4));
        if constexpr (ADD) v += r[t];
        bool ok;
        float* dst = row_ptr(c, t, ok);
        if (ok) *(f32x4_t*)dst = v;  // fp32 / residual rows: streaming them measured no gain
      }
    }
  }
}

// bias of the 16 columns a lane owns.  Plain loads, made "consumed" immediately so that no
// compiler-visible VMEM load is ever pending across a loop back-edge (hipcc would then put
// s_waitcnt vmcnt(0) in front of unrelated instructions that reuse the registers and drain
// the hand-counted LDS-DMA pipeline every K-step).
__device__ __forceinline__ void load_bias(const GemmArgs& a, int n, f32x4_t (&bv)[4]) {
  const int nc = min(n, a.N - 16);
#pragma unroll
  for (int fj = 0; fj < 4; ++fj) {
    bv[fj] = a.bias ? *(const f32x4_t*)(a.bias + nc + fj * 4) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int fj = 0; fj < 4; ++fj) asm volatile("" : "+v"(bv[fj]));
}
// the same through inline asm: invisible to hipcc's waitcnt pass, counted by the caller
// (4 VMEM ops per wave); the values may be read only after a covering s_waitcnt vmcnt.
__device__ __forceinline__ void load_bias_async(const GemmArgs& a, int n, f32x4_t (&bv)[4]) {
  const float* p = a.bias + min(n, a.N - 16);
#pragma unroll
  for (int fj = 0; fj < 4; ++fj)
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bv[fj]) : "v"(p + fj * 4) : "memory");
}

template <int MF>
__device__ __forceinline__ void zero_acc(f32x4_t (&acc)[4][MF]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
}

// =========================================================================================
// 128x128 tile kernel (one workgroup per tile)
// =========================================================================================
namespace tile {
constexpr int BM = 128, BN = 128;
constexpr int TILE_BYTES = BM * ROWB;
constexpr int STAGE_BYTES = 2 * TILE_BYTES;
constexpr int LDS_BYTES = 2 * STAGE_BYTES;
}  // namespace tile

template <int PREC, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_tile_kernel(const GemmArgs a) {
  using namespace tile;
  enter_precision_mode<PREC>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = prec_esize(PREC);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // XCD-aware bijective remap: hardware places block b on XCD b%8; give each XCD a
  // contiguous run of logical tiles (same X row panel, W walks through its L2).
  const int nbn = (a.N + BN - 1) / BN;
  const int nbm = (a.M + BM - 1) / BM;
  const int nwg = nbn * nbm;
  int lid;
  {
    const int bid = blockIdx.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int m0 = (lid / nbn) * BM;
  const int n0 = (lid % nbn) * BN;

  const char* gx[4];
  const char* gw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int blk = i * 4 + wave;             // 1-KiB block of the 16-KiB tile
    const int p = blk * 4 + (lane >> 4);      // row pair 0..63
    const int s = lane & 15;                  // 16-B slot inside the 256-B pair row
    const int row = 2 * p + (s >> 3);
    const int chunk = (s & 7) ^ (p & 7);
    const int mr = min(m0 + row, a.M - 1);
    const int nr = min(n0 + (row & 64) + perm_n(row & 63), a.N - 1);
    gx[i] = (const char*)a.x + ((size_t)mr * a.ldx) * ES + chunk * 16;
    gw[i] = (const char*)a.w + ((size_t)nr * a.K) * ES + chunk * 16;
  }
  const uint32_t lds0 = lds_addr(smem);
  auto stage = [&](int st, int kt) {
    const uint32_t base = lds0 + st * STAGE_BYTES;
    size_t kox, kow;
    kstep_off(a, kt, kox, kow);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int blk = i * 4 + wave;
      glds16(gx[i] + kox, __builtin_amdgcn_readfirstlane(base + blk * 1024));
      glds16(gw[i] + kow, __builtin_amdgcn_readfirstlane(base + TILE_BYTES + blk * 1024));
    }
  };

  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, g = lane >> 4;
  const int foff[2] = {frag_off(fr, g, 0), frag_off(fr, g, 1)};
  const int xbase = wr * 64 * ROWB;
  const int wbase = TILE_BYTES + wc * 64 * ROWB;

  f32x4_t acc[4][4];
  zero_acc(acc);
  const int nk = ksteps(a, ES);
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
    const char* sb = smem + (kt & 1) * STAGE_BYTES;
    wave_kstep<PREC, 4>(sb + xbase, sb + wbase, foff, acc);
  }
  f32x4_t bv[4];
  load_bias(a, n0 + wc * 64 + g * 16, bv);
  float amax = 0.f;
  wave_epilogue<PREC, EPI, 4>(a, acc, bv, m0 + wr * 64, n0 + wc * 64, fr, g, amax);
  sat_report<PREC>(amax, a.sat);
}

// =========================================================================================
// 64x128 tile kernel (shipped since round 4; round 3 measured it as harness variant 11: batch 8 +7.5 %, batch 16 +4.5 %,
// profiles/r03_z_tile64_small_batches.txt).  gemm_tile_kernel
// with half the rows per workgroup — 2 x 2 waves of 32 x 64, the same staging, fragment and epilogue code (MF = 2) —
// for problems that give the 128x128 kernel fewer workgroups than the chip has CUs (batch <= 32): twice the
// workgroups, each with half the MFMA work per K-step and the same latency chain.  Same bits (a row's K is summed
// in the same order whatever the tile).
// =========================================================================================
namespace tile64 {
constexpr int BM = 64, BN = 128;
constexpr int X_BYTES = BM * ROWB, W_BYTES = BN * ROWB;  // 8 + 16 KiB
constexpr int STAGE_BYTES = X_BYTES + W_BYTES;
constexpr int LDS_BYTES = 2 * STAGE_BYTES;                // 48 KiB
}  // namespace tile64

template <int PREC, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_tile64_kernel(const GemmArgs a) {
  using namespace tile64;
  enter_precision_mode<PREC>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = prec_esize(PREC);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nbn = (a.N + BN - 1) / BN;
  const int nbm = (a.M + BM - 1) / BM;
  const int nwg = nbn * nbm;
  int lid;
  {
    const int bid = blockIdx.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int m0 = (lid / nbn) * BM;
  const int n0 = (lid % nbn) * BN;
  const char* gx[2];
  const char* gw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int blk = i * 4 + wave;             // 1-KiB block: X has 8 of them, W 16
    const int p = blk * 4 + (lane >> 4);      // row pair
    const int sl = lane & 15;                 // 16-B slot inside the 256-B pair row
    const int row = 2 * p + (sl >> 3);
    const int chunk = (sl & 7) ^ (p & 7);
    if (i < 2) gx[i] = (const char*)a.x + ((size_t)min(m0 + row, a.M - 1) * a.ldx) * ES + chunk * 16;
    const int nr = min(n0 + (row & 64) + perm_n(row & 63), a.N - 1);
    gw[i] = (const char*)a.w + ((size_t)nr * a.K) * ES + chunk * 16;
  }
  const uint32_t lds0 = lds_addr(smem);
  auto stage = [&](int st, int kt) {
    const uint32_t base = lds0 + st * STAGE_BYTES;
    size_t kox, kow;
    kstep_off(a, kt, kox, kow);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int blk = i * 4 + wave;
      if (i < 2) glds16(gx[i] + kox, __builtin_amdgcn_readfirstlane(base + blk * 1024));
      glds16(gw[i] + kow, __builtin_amdgcn_readfirstlane(base + X_BYTES + blk * 1024));
    }
  };
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, g = lane >> 4;
  const int foff[2] = {frag_off(fr, g, 0), frag_off(fr, g, 1)};
  const int xbase = wr * 32 * ROWB;
  const int wbase = X_BYTES + wc * 64 * ROWB;
  f32x4_t acc[4][2];
  zero_acc(acc);
  const int nk = ksteps(a, ES);
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
    const char* sb = smem + (kt & 1) * STAGE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {  // wave_khalf for two row fragments (it walks them four at a time)
      uint4 wf[4], xf[2];
#pragma unroll
      for (int f = 0; f < 4; ++f) wf[f] = *(const uint4*)(sb + wbase + f * 2048 + foff[kk]);
#pragma unroll
      for (int f = 0; f < 2; ++f) xf[f] = *(const uint4*)(sb + xbase + f * 2048 + foff[kk]);
#pragma unroll
      for (int fj = 0; fj < 4; ++fj)
#pragma unroll
        for (int fi = 0; fi < 2; ++fi) {
          if constexpr (PREC != MCM_PREC_F32) {
            acc[fj][fi] = mfma16<PREC>(wf[fj], xf[fi], acc[fj][fi]);
          } else {
            const f32x4_t wv = __builtin_bit_cast(f32x4_t, wf[fj]);
            const f32x4_t xv = __builtin_bit_cast(f32x4_t, xf[fi]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
              acc[fj][fi] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[t], xv[t], acc[fj][fi], 0, 0, 0);
          }
        }
    }
  }
  f32x4_t bv[4];
  load_bias(a, n0 + wc * 64 + g * 16, bv);
  float amax = 0.f;
  wave_epilogue<PREC, EPI, 2>(a, acc, bv, m0 + wr * 32, n0 + wc * 64, fr, g, amax);
  sat_report<PREC>(amax, a.sat);
}

// XCD-local tile enumeration: N-tiles are walked in groups of `gn` (the group's W panel
// stays L2-resident while the XCD sweeps its M-tiles); inside a group the order is
// (mtl, nt) n-fastest, so the 32 CUs of an XCD hold ~32/gn X row panels x gn W panels.
__device__ __forceinline__ void tile_of(int q, int nmt_x, int nbn, int gn, int& mtl, int& nt) {
  int start = 0, g0 = 0;
  for (;;) {
    const int gw = min(gn, nbn - g0), cnt = nmt_x * gw;
    if (q < start + cnt || g0 + gw >= nbn) {
      const int r = q - start;
      mtl = r / gw;
      nt = g0 + (r - mtl * gw);
      return;
    }
    start += cnt;
    g0 += gw;
  }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// =========================================================================================
// persistent 256x256 kernel: 8 waves as 2(M) x 4(N), wave tile 128x64 (acc = 128 VGPRs),
// two 64-KiB LDS stages.  One K-step = 64 MFMAs per wave = 2048 MFMA-cycles per SIMD, and
// the next stage's DMA (issued right after the barrier) has that long to land.  Per flop
// it moves 2/3 of the L2->LDS bytes of the 256x128 tile: on this chip the L1->LDS path
// (~64 B/clk/CU) is what bounds the smaller tiles, not the matrix pipe.
// =========================================================================================
namespace p256 {
constexpr int BM = 256, BN = 256;
constexpr int A_BYTES = BM * ROWB;  // 32 KiB
constexpr int W_BYTES = BN * ROWB;  // 32 KiB
constexpr int STAGE_BYTES = A_BYTES + W_BYTES;
constexpr int LDS_BYTES = 2 * STAGE_BYTES + 8 * 4096;  // 128 KiB of stages + 4 KiB epilogue window per wave
}  // namespace p256

// 16-byte global load / store from inline asm with a scalar base and a 32-bit lane offset: invisible to hipcc's waitcnt
// pass, counted by the caller (used by the fp32 interior epilogue below and by the pixel-gathering A operand of the patch GEMM)
__device__ __forceinline__ void gload16(f32x4_t& dst, const void* sbase, uint32_t voff) {
  asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(sbase) : "memory");
}
__device__ __forceinline__ void gstore16(const void* sbase, uint32_t voff, const f32x4_t& v) {
  asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}

// EPI_PATCH with GemmArgs::px — the im2col-free patch embedding (HF modeling_clip.py:148-154,209-210: a
// Conv2d with kernel = stride = P is a GEMM over gathered pixels).  The A operand is not read from a patch matrix: each
// lane fetches the 8 (fp32 mode: 4) consecutive pixels behind its 16-byte LDS chunk straight from the NCHW fp32 image —
// k = (c, py, px) is the [D,3,P,P] weight flattening, so a chunk is 32 contiguous bytes of one image row — converts them
// (the same single-instruction packs patchify used: same bits) and writes them to the slot the LDS-DMA would have
// filled.  Loads are issued where the DMA for the next K-step is issued and committed to LDS at the end of the current
// step, a whole K-step of MFMAs later.  The 154-MB patch matrix (written by one kernel, read back by this one) is gone.
// PXF is its own instantiation (not a run-time branch): without the X row pointers and the bias registers of the plain form
// the 32 registers of pixel loads in flight fit the 256-register budget; with both forms in one kernel hipcc spilled 13.
template <int PREC, int EPI, bool COUNT_STORES, bool PXF = false>
__global__ __launch_bounds__(512, 2) void gemm_p256_kernel(const GemmArgs a) {
  static_assert(!PXF || EPI == EPI_PATCH, "pixel gathering: the patch embedding only");
  using namespace p256;
  enter_precision_mode<PREC>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = prec_esize(PREC);
  // store instructions per wave per full tile: 8 rows x (2 x 16 B bf16 | 4 x 16 B fp32)
  constexpr int STORES_PER_EPI = (PREC != MCM_PREC_F32 && epi_plain16(EPI)) ? 16 : 32;  // (*_X2: 32 as well)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // 0..7

  const int nbn = (a.N + BN - 1) / BN;
  const int nbm = (a.M + BM - 1) / BM;
  const int G8 = gridDim.x >> 3;
  const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
  const int nmt_x = (nbm - xcd + 7) >> 3;
  const int ntl_x = nmt_x * nbn;
  const int ntl = jx < ntl_x ? (ntl_x - jx + G8 - 1) / G8 : 0;
  if (ntl == 0) return;
  const int nk = ksteps(a, ES);
  const int total = ntl * nk;

  const int r0 = wave * 8 + (lane >> 4) * 2 + ((lane & 15) >> 3);
  const int chunk = (lane & 7) ^ (((wave & 1) << 2) | (lane >> 4));
  const char* gx[4];
  const char* gw[4];
  int ji = 0, kti = 0;
  constexpr int EC = 16 / ES, KS = ROWB / ES;  // elements per 16-B chunk / per K-step
  uint32_t pxoff[4] = {0u, 0u, 0u, 0u};  // PXF: byte offset of this lane's pixels at (c, py) = (0, 0), per piece
  f32x4_t xr[4][2];                        // PXF: the pixel loads in flight
  int xst = 0;                             // ... and the LDS stage they belong to
  // Tile walk.  With the default plain n-fastest order (gn >= nbn) the next tile of this workgroup
  // is G8 tiles further on, so (m-tile, n-tile) advance by a fixed (G8 / nbn, G8 % nbn) with one
  // carry: no division on the tile switch, which sits on the refill path of waves 0-3.  Interior
  // tiles take their 8 row pointers from per-lane bases plus a uniform offset (no clamps, no
  // 64-bit multiplies per pointer).
  const bool plain = a.gn >= nbn;
  const int dmt = G8 / nbn, dnt = G8 - dmt * nbn;
  struct Cursor { int mtl, nt; };
  auto cursor_init = [&](Cursor& c) { tile_of(jx, nmt_x, nbn, a.gn, c.mtl, c.nt); };
  auto cursor_next = [&](Cursor& c, int i) {
    if (plain) {
      c.mtl += dmt;
      c.nt += dnt;
      if (c.nt >= nbn) { c.nt -= nbn; ++c.mtl; }
    } else {
      tile_of(jx + i * G8, nmt_x, nbn, a.gn, c.mtl, c.nt);
    }
  };
  const size_t sx = (size_t)a.ldx * ES, sw = (size_t)a.K * ES;  // row strides in bytes
  const char* xlane = (const char*)a.x + (size_t)r0 * sx + chunk * 16;
  const char* wlane = (const char*)a.w + (size_t)perm_n(r0) * sw + chunk * 16;
  // a.rev: walk this XCD's M tiles from the last to the first (the producer of X wrote its highest
  // rows last, so they are the ones still in L2 / Infinity Cache)
  auto mt_of = [&](int mtl) { return a.rev ? nmt_x - 1 - mtl : mtl; };
  Cursor ci;
  auto set_issue_tile = [&]() {
    const int m0 = (mt_of(ci.mtl) * 8 + xcd) * BM, n0 = ci.nt * BN;
    if (m0 + BM <= a.M && n0 + BN <= a.N) {
      const char* xb = xlane + (size_t)m0 * sx;
      const char* wb = wlane + (size_t)n0 * sw;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if constexpr (!PXF) gx[p] = xb + (size_t)(p * 64) * sx;
        gw[p] = wb + (size_t)(p * 64) * sw;
      }
    } else {  // edge tile: rows past the end re-read the last row (their results are never stored)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if constexpr (!PXF) gx[p] = (const char*)a.x + (size_t)min(m0 + p * 64 + r0, a.M - 1) * sx + chunk * 16;
        gw[p] = (const char*)a.w + (size_t)min(n0 + p * 64 + perm_n(r0), a.N - 1) * sw + chunk * 16;
      }
    }
    if constexpr (PXF) {
      {  // row m = (image b, patch gy * g + gx); this lane's chunk starts at element e of the K-step
        const int P = a.patch, S = a.img, gsz = S / P;
        const int e = chunk * EC, dpy = e / P, pxl = e - dpy * P;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int m = min(m0 + p * 64 + r0, a.M - 1);
          const int b = m / a.np, pp = m - b * a.np, gy = pp / gsz, gxx = pp - gy * gsz;
          pxoff[p] = (uint32_t)((((size_t)b * 3 * S + (size_t)gy * P + dpy) * S + (size_t)gxx * P + pxl) * 4);
        }
      }
    }
  };
  const uint32_t lds0 = lds_addr(smem);
  // PXF: request the pixels of the K-step the issue cursor points at (the cursor is advanced by issue(), called after).
  // Every wave does this at the TOP of a step — also waves 4-7, whose DMA issue sits in the middle of it — so that the
  // loads have the whole step's MFMAs to land in.
  auto issue_px = [&](int st) {
    // K-step -> (channel c, first patch row py0): KS / P patch rows per step
    const int r = (kti >> a.ksplit) * (KS / a.patch), c = r / a.patch, py0 = r - c * a.patch;
    const char* kb = (const char*)a.px + ((size_t)c * a.img + py0) * a.img * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      gload16(xr[p][0], kb, pxoff[p]);
      if constexpr (ES == 2) gload16(xr[p][1], kb, pxoff[p] + 16u);
    }
    xst = st;
  };
  auto issue = [&](int st) {
    const uint32_t base = lds0 + st * STAGE_BYTES;
    size_t ko, kox;
    kstep_off(a, kti, kox, ko);
    if constexpr (PXF) {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        glds16(gw[p] + ko, __builtin_amdgcn_readfirstlane(base + A_BYTES + (p * 8 + wave) * 1024));
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        glds16(gx[p] + kox, __builtin_amdgcn_readfirstlane(base + (p * 8 + wave) * 1024));
        glds16(gw[p] + ko, __builtin_amdgcn_readfirstlane(base + A_BYTES + (p * 8 + wave) * 1024));
      }
    }
    if (++kti == nk) {
      kti = 0;
      if (++ji < ntl) {
        cursor_next(ci, ji);
        set_issue_tile();
      }
    }
  };

  const int wr = wave >> 2, wc = wave & 3;  // 2 x 4 waves, wave tile 128 x 64
  const bool late = wave >= 4;
  const int fr = lane & 15, g = lane >> 4;
  const int foff[2] = {frag_off(fr, g, 0), frag_off(fr, g, 1)};
  const int xbase = wr * 128 * ROWB;
  const int wbase = A_BYTES + wc * 64 * ROWB;

  f32x4_t acc[4][8];
  zero_acc<8>(acc);
  float amax = 0.f;
  f32x4_t bv[4];
#pragma unroll
  for (int fj = 0; fj < 4; ++fj) bv[fj] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  // PXF: the pixels requested by the last issue() -> operand dtype -> the LDS slots the DMA would have filled.  Called
  // where the issuing wave has a whole K-step of MFMAs (waves 4-7: half of one) between the request and this wait.
  auto commit_x = [&]() {
    wait_vmcnt<0>();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      asm volatile("" : "+v"(xr[p][0]));
      if constexpr (ES == 2) asm volatile("" : "+v"(xr[p][1]));
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      char* dst = smem + xst * STAGE_BYTES + (p * 8 + wave) * 1024 + lane * 16;
      if constexpr (PREC != MCM_PREC_F32) {
        *(uint4*)dst = make_uint4(pack2<PREC>(xr[p][0][0], xr[p][0][1]), pack2<PREC>(xr[p][0][2], xr[p][0][3]),
                                  pack2<PREC>(xr[p][1][0], xr[p][1][1]), pack2<PREC>(xr[p][1][2], xr[p][1][3]));
      } else {
        *(f32x4_t*)dst = xr[p][0];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };

  cursor_init(ci);
  set_issue_tile();
  if constexpr (PXF) issue_px(0);
  issue(0);
  if constexpr (PXF) commit_x();
  int issued = 1;
  int jc = 0, ktc = 0;
  Cursor cc;
  cursor_init(cc);
  int cm0 = (mt_of(cc.mtl) * 8 + xcd) * BM, cn0 = cc.nt * BN;
  bool stores_pending = false;
  if (late) __builtin_amdgcn_s_setprio(1);  // the younger half would otherwise lose every arbitration
  for (int s = 0; s < total; ++s) {
    // VMEM issue order: step e (tile end): [DMA stage e+1] ... [stores E]; step e+1:
    // [bias 4] [DMA stage e+2].  Stage s is the youngest DMA at this point, so only the
    // previous tile's stores may stay in flight.
    if (COUNT_STORES && stores_pending) wait_vmcnt<STORES_PER_EPI>();
    else wait_vmcnt<0>();
    stores_pending = false;
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (!PXF) {  // (the patch embedding has no bias: bv stays the constant zero it was initialised to)
      if (ktc == 0 && a.bias) load_bias_async(a, cn0 + wc * 64 + g * 16, bv);
    }
    // The two waves of a SIMD (w and w+4) take turns: an LDS-DMA instruction blocks its wave for
    // 70-155 cycles while the TA takes the 64 addresses (cycle stamps, MCM_GEMM_TRACE), so if both
    // waves refill at the top of the step the matrix pipe idles through 8 of them and then both
    // waves want it at once.  Waves 0-3 refill first and compute after; waves 4-7 (static
    // priority 1) compute the first K half, refill, compute the second.
    const bool refill = issued < total;
    if constexpr (PXF) {
      if (refill) issue_px(issued & 1);
    }
    if (refill && !late) issue(issued & 1);
    const char* sb = smem + (s & 1) * STAGE_BYTES;
    wave_khalf<PREC, 8>(sb + xbase, sb + wbase, foff[0], acc);
    if (refill && late) issue(issued & 1);
    if (refill) ++issued;
    wave_khalf<PREC, 8>(sb + xbase, sb + wbase, foff[1], acc);
    if (++ktc == nk) {
      if constexpr (!PXF) {
        if (nk < 2) wait_vmcnt<0>();  // bias issued in this very step
#pragma unroll
        for (int fj = 0; fj < 4; ++fj) asm volatile("" : "+v"(bv[fj]));
      }
      wave_epilogue_lds<PREC, EPI, 8>(a, acc, bv, cm0 + wr * 128, cn0 + wc * 64, lane,
                                      smem + 2 * STAGE_BYTES + wave * 4096, amax);
      zero_acc<8>(acc);
      stores_pending = (cm0 + BM <= a.M && cn0 + BN <= a.N);
      ktc = 0;
      if (++jc < ntl) {
        cursor_next(cc, jc);
        cm0 = (mt_of(cc.mtl) * 8 + xcd) * BM;
        cn0 = cc.nt * BN;
      }
    }
    if constexpr (PXF) {
      if (refill) commit_x();  // the next step's X pixels, before the barrier that opens it
    }
  }
  sat_report<PREC>(amax, a.sat);
}

// fp32-row epilogue of a full (interior) 128x64 wave tile for the ping-pong kernel: the same LDS bounce and
// the same arithmetic as the fp32 branch of wave_epilogue_lds, but every global access is issued from inline
// asm and waited for by count.  hipcc's own waitcnt pass never sees them, so it has no reason to put a
// vmcnt(0) in front of the fragment reads or the MFMAs of the K loop (it did, once the epilogue's plain
// stores were inlined into the loop: the wait drains the LDS-DMA stream, -20 % on fc2).  The queue at the wait
// of chunk c, oldest first: [older] [loads c] [stores c-1] [loads c+1]  =>  vmcnt <= 8 (<= 4 at both ends).
template <int N>
__device__ __forceinline__ void wait_vmcnt_pin(f32x4_t (&b)[4]) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) : "n"(N) : "memory");
}
template <int EPI, int MF>
__device__ __forceinline__ void wave_epilogue_f32_interior(const GemmArgs& a, const f32x4_t (&acc)[4][MF],
                                                           const f32x4_t (&bv)[4], int mw, int nw, int lane,
                                                           char* scratch) {
  static_assert(EPI != EPI_PATCH, "patch rows are remapped: not an interior form");
  const int fr = lane & 15, g = lane >> 4;
  const int rrow = lane >> 4, c16 = lane & 15;
  const uint32_t voff = (uint32_t)(rrow * a.ldo + c16 * 4) * 4u;  // bytes
  const char* base = (const char*)(EPI == EPI_RESID ? a.resid : (float*)a.out) + ((size_t)mw * a.ldo + nw) * 4;
  // rows are visited in order, 4 at a time: a load pointer and a store pointer walk down the tile by one scalar add
  // each (per-row-group offsets computed up front cost 64 scalar registers and pushed loop state into VGPR lanes)
  const size_t step = (size_t)a.ldo * 16;  // bytes per 4 rows
  const char* lp = base;
  const char* sp = base;
  f32x4_t buf[2][4];
  // EPI_RESID: the bias of the lane's 4 columns AFTER the bounce, loaded here (4 registers, and nothing of this epilogue
  // is live across the K loop; `bv` is not used) - the same (acc + b) + resid as every other form
  f32x4_t bia = {0.f, 0.f, 0.f, 0.f};
  if constexpr (EPI == EPI_RESID) {
    if (a.bias) gload16(bia, a.bias + nw, (uint32_t)c16 * 16u);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      gload16(buf[0][t], lp, voff);
      lp += step;
    }
  }
#pragma unroll
  for (int c = 0; c < MF; ++c) {
    if constexpr (EPI == EPI_RESID) {
      if (c + 1 < MF) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          gload16(buf[(c + 1) & 1][t], lp, voff);
          lp += step;
        }
      }
    }
#pragma unroll
    for (int fj = 0; fj < 4; ++fj) {
      f32x4_t v = acc[fj][c];
      if constexpr (EPI != EPI_RESID) v += bv[fj];
      if constexpr (epi_gelu(EPI)) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = epi_erf(EPI) ? gelu_erf(v[t]) : quick_gelu(v[t]);
      }
      *(f32x4_t*)(scratch + fr * 256 + (((g * 4 + fj) ^ fr) << 4)) = v;
    }
    f32x4_t v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int row = t * 4 + rrow;
      v[t] = *(const f32x4_t*)(scratch + row * 256 + ((c16 ^ row) << 4));
    }
    if constexpr (EPI == EPI_RESID) {
      if (c == 0 || c + 1 == MF) wait_vmcnt_pin<4>(buf[c & 1]);
      else wait_vmcnt_pin<8>(buf[c & 1]);
      if (c == 0) asm volatile("" : "+v"(bia));  // older than the loads the wait above covers
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = (v[t] + bia) + buf[c & 1][t];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      gstore16(sp, voff, v[t]);
      sp += step;
    }
  }
}

// =========================================================================================
// persistent 256x256 "ping-pong" kernel.  Same tile, wave tiles, LDS image and epilogue as
// gemm_p256_kernel, but the two waves of a SIMD (w and w+4) run half a K-step apart: while one
// is in its MEMORY phase (8 LDS-DMA pieces for the next step, then the whole step's 24 fragments
// into 96 registers) the other is in its COMPUTE phase (64 back-to-back MFMAs on registers), and
// they swap at a workgroup barrier — two barriers per K-step instead of one, but the matrix pipe
// of a SIMD always has one wave that does nothing but feed it.  Interior tiles only (M, N multiples
// of 256).
// =========================================================================================
__device__ __forceinline__ void glds16s(const void* sbase, uint32_t voff, uint32_t lds_base) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_base)
      : "memory");
}

template <int PREC, int EPI>
__global__ __launch_bounds__(512, 2) void gemm_pp_kernel(const GemmArgs a) {
  using namespace p256;
  enter_precision_mode<PREC>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = prec_esize(PREC);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // 0..7
  const int grp = wave >> 2, w4 = wave & 3;

  const int nbn = a.N / BN, nbm = a.M / BM;
  const int G8 = gridDim.x >> 3;
  const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
  const int nmt_x = (nbm - xcd + 7) >> 3;
  const int ntl_x = nmt_x * nbn;
  const int ntl = jx < ntl_x ? (ntl_x - jx + G8 - 1) / G8 : 0;
  if (ntl == 0) return;
  const int nk = ksteps(a, ES);
  const int total = ntl * nk;

  const int dmt = G8 / nbn, dnt = G8 - dmt * nbn;
  struct Cursor { int mtl, nt; };
  auto cursor_next = [&](Cursor& c) {
    c.mtl += dmt;
    c.nt += dnt;
    if (c.nt >= nbn) { c.nt -= nbn; ++c.mtl; }
  };
  auto mt_of = [&](int mtl) { return a.rev ? nmt_x - 1 - mtl : mtl; };
  const size_t sx = (size_t)a.ldx * ES, sw = (size_t)a.K * ES;  // row strides in bytes

  // ---- LDS-DMA side.  Waves 0-3 (rows 0-127 of the tile) stage their half of the X panel and all of W,
  // 12 pieces per wave and step; waves 4-7 stage the other X half, which only they read, 4 pieces.  Every
  // piece is issued in the memory phase of step s for step s+1 and waited for at the end of the issuing
  // wave's compute phase, one phase before its first reader.
  // Per-lane constants (DMA source offsets, fragment offsets) are NOT kept across the loop: 128 accumulators
  // + 64 fragments leave hipcc no room, and a spilled loop invariant comes back through a scratch load whose
  // vmcnt(0) drains the DMA stream.  They are rebuilt from an opaque copy of the lane id where needed (~12 VALU).
  struct LaneK { uint32_t voff_x, voff_w; int fo0, fo1; };
  auto lane_consts = [&]() {
    int l = lane;
    asm volatile("" : "+v"(l));
    const int rr = (l >> 4) * 2 + ((l & 15) >> 3);
    const int chunk = (l & 7) ^ (((w4 & 1) << 2) | (l >> 4));
    LaneK c;
    c.voff_x = (uint32_t)(rr * (uint32_t)sx + chunk * 16);
    c.voff_w = (uint32_t)(perm_n(w4 * 8 + rr) * (uint32_t)sw + chunk * 16);
    c.fo0 = frag_off(l & 15, l >> 4, 0);
    c.fo1 = frag_off(l & 15, l >> 4, 1);
    return c;
  };
  Cursor ci{jx / nbn, jx % nbn};
  int ji = 0, kti = 0;
  const char *tx, *tw;  // uniform: first byte of this wave's rows of the tile being staged
  auto set_issue_tile = [&]() {
    const int m0 = (mt_of(ci.mtl) * 8 + xcd) * BM, n0 = ci.nt * BN;
    tx = (const char*)a.x + (size_t)(m0 + grp * 128 + w4 * 8) * sx;
    tw = (const char*)a.w + (size_t)n0 * sw;
  };
  const uint32_t lds0 = lds_addr(smem);
  auto piece = [&](const LaneK& lk, int st, int i) {  // i: 0-3 X pieces, 4-11 W pieces (waves 0-3 only)
    const uint32_t base = lds0 + st * STAGE_BYTES + w4 * 1024;
    size_t ko, kox;  // split weights: X K-step s / 2 meets W' K-steps s (hi), s + 1 (lo); split activations: the mirror image
    kstep_off(a, kti, kox, ko);
    if (i < 4) {
      glds16s(tx + kox + (size_t)(i * 32) * sx, lk.voff_x, base + (grp * 16 + i * 4) * 1024);
    } else {
      const int q = i - 4;
      glds16s(tw + ko + (size_t)((q >> 1) * 64 + (q & 1) * 8) * sw, lk.voff_w, base + A_BYTES + q * 4096);
    }
  };
  constexpr int NP0 = 12;  // pieces per step of waves 0-3
  auto issue_done = [&]() {
    if (++kti == nk) {
      kti = 0;
      if (++ji < ntl) {
        cursor_next(ci);
        set_issue_tile();
      }
    }
  };

  // ---- MFMA side
  const int wr = wave >> 2, wc = wave & 3;  // 2 x 4 waves, wave tile 128 x 64
  const int xbase = wr * 128 * ROWB;
  const int wbase = A_BYTES + wc * 64 * ROWB;
  typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
  // Fragments of a step: the W fragments of both K halves and the X fragments of the first half are read in
  // the memory phase (16 reads, 64 registers); the X fragments of the second half replace those of the first
  // one by one during the compute phase (each after its last use) — the rows they come from are staged by this
  // very wave group, so nobody overwrites them before the group's own next memory phase.
  u32x4_t xf[8], wf[2][4];
  auto readf = [&](const LaneK& lk, int st, int i) {  // memory-phase read i of 16
    const char* sb = smem + st * STAGE_BYTES;
    if (i < 4) wf[0][i] = *(const u32x4_t*)(sb + wbase + i * 2048 + lk.fo0);
    else if (i < 12) xf[i - 4] = *(const u32x4_t*)(sb + xbase + (i - 4) * 2048 + lk.fo0);
    else wf[1][i - 12] = *(const u32x4_t*)(sb + wbase + (i - 12) * 2048 + lk.fo1);
  };
  auto pin_frags = [&]() {  // the fragments are in registers here, not wherever hipcc would sink the reads to
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int f = 0; f < 4; ++f) asm volatile("" : "+v"(wf[0][f]));
#pragma unroll
    for (int f = 0; f < 4; ++f) asm volatile("" : "+v"(wf[1][f]));
#pragma unroll
    for (int f = 0; f < 8; ++f) asm volatile("" : "+v"(xf[f]));
  };
  f32x4_t acc[4][8];
  zero_acc<8>(acc);
  float amax = 0.f;  // fp16 saturation watch (sat_track / sat_report, common.hpp)
  auto mfma_pair = [&](const u32x4_t& wv4, const u32x4_t& xv4, f32x4_t& c) {
    if constexpr (PREC != MCM_PREC_F32) {
      c = mfma16<PREC>(__builtin_bit_cast(uint4, wv4), __builtin_bit_cast(uint4, xv4), c);
    } else {
      const f32x4_t wv = __builtin_bit_cast(f32x4_t, wv4);
      const f32x4_t xv = __builtin_bit_cast(f32x4_t, xv4);
#pragma unroll
      for (int t = 0; t < 4; ++t) c = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[t], xv[t], c, 0, 0, 0);
    }
  };
  auto compute = [&](int fo1, int st) {
    const char* sb = smem + st * STAGE_BYTES;
#pragma unroll
    for (int fi = 0; fi < 8; ++fi) {
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) mfma_pair(wf[0][fj], xf[fi], acc[fj][fi]);
      xf[fi] = *(const u32x4_t*)(sb + xbase + fi * 2048 + fo1);
    }
#pragma unroll
    for (int fi = 0; fi < 8; ++fi)
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) mfma_pair(wf[1][fj], xf[fi], acc[fj][fi]);
  };

  Cursor cc{jx / nbn, jx % nbn};
  int em0 = 0, en0 = 0;  // tile whose epilogue is pending
  f32x4_t bv[4];  // bias of the pending tile: asm loads issued at the top of its last compute phase
#pragma unroll
  for (int fj = 0; fj < 4; ++fj) bv[fj] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  auto epilogue = [&]() {
    // every lane-derived address of the epilogue is recomputed from an opaque copy of the lane id: hoisted out
    // of the K loop they would occupy ~20 registers that the loop (128 accumulators + 64 fragments) does not have
    int le = lane;
    asm volatile("" : "+v"(le));
    if constexpr (EPI != EPI_RESID) {  // (the residual form loads its bias inside the epilogue: a pin would keep 16 zeros
                                       // live across the K loop)
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) asm volatile("" : "+v"(bv[fj]));
    }
    char* win = smem + 2 * STAGE_BYTES + wave * 4096;
    if constexpr (PREC != MCM_PREC_F32 && epi_store16(EPI))
      wave_epilogue_lds<PREC, EPI, 8, true>(a, acc, bv, em0 + wr * 128, en0 + wc * 64, le, win, amax);
    else
      wave_epilogue_f32_interior<EPI, 8>(a, acc, bv, em0 + wr * 128, en0 + wc * 64, le, win);
    zero_acc<8>(acc);
  };
  set_issue_tile();
  {
    const LaneK lk = lane_consts();
#pragma unroll
    for (int i = 0; i < NP0; ++i)
      if (i < 4 || !grp) piece(lk, 0, i);
  }
  issue_done();
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (grp) {  // waves 4-7 run one phase behind
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  int ktc = 0;
  bool pend = false;
  auto phase_barrier = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  for (int s = 0; s < total; ++s) {
    // ---- memory phase of step s: the step's fragments into registers, interleaved with the DMA issues for
    // step s+1 (a DMA issue blocks the wave on the TA, a ds_read on the LDS queue: alternating them lets the two
    // queues drain side by side).  The first instruction is a ds_read on purpose: hipcc puts a vmcnt(0) in
    // front of the first fragment read after an epilogue with compiler-visible stores, which must not have
    // this phase's DMA to wait for.  After the very last step the issue re-reads the last tile (never used).
    // At a tile boundary (`pend`) waves 0-3 issue, pass the barrier, run the epilogue and only then read the
    // fragments; waves 4-7 run the epilogue first: both epilogues fall into the same phase and no fragment
    // is live across them.
    const int sr = s & 1, si = sr ^ 1;
    const bool split = pend && !grp;
    int fo1;
    if (pend) {
      if (!grp) {
        const LaneK lk = lane_consts();
#pragma unroll
        for (int i = 0; i < NP0; ++i) piece(lk, si, i);
        issue_done();
        phase_barrier();
      }
      epilogue();
      if (!grp) {
        const LaneK lk = lane_consts();
        fo1 = lk.fo1;
#pragma unroll
        for (int i = 0; i < 16; ++i) readf(lk, sr, i);
      }
    }
    if (!split) {
      const LaneK lk = lane_consts();
      fo1 = lk.fo1;
      if (!grp) {
#pragma unroll
        for (int i = 0; i < NP0; ++i) {
          if (i < 8) {
            readf(lk, sr, 2 * i);
            readf(lk, sr, 2 * i + 1);
          }
          piece(lk, si, i);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int j = 0; j < 4; ++j) readf(lk, sr, 4 * i + j);
          piece(lk, si, i);
        }
      }
      issue_done();
    }
    pin_frags();
    if (!split) phase_barrier();
    // ---- compute phase of step s
    if (EPI == EPI_RESID) {  // residual form: the bias is loaded inside the epilogue
    } else if (ktc == nk - 1 && a.bias) {
      int le = lane;
      asm volatile("" : "+v"(le));
      load_bias_async(a, cc.nt * BN + wc * 64 + (le >> 4) * 16, bv);  // covered by the wait that ends this phase
    }
    __builtin_amdgcn_s_setprio(1);
    compute(fo1, sr);
    __builtin_amdgcn_s_setprio(0);
    wait_vmcnt<0>();  // this wave's pieces of step s+1, issued a phase ago
    phase_barrier();
    pend = false;
    if (++ktc == nk) {
      ktc = 0;
      pend = true;
      em0 = (mt_of(cc.mtl) * 8 + xcd) * BM;
      en0 = cc.nt * BN;
      cursor_next(cc);
    }
  }
  if (!grp) {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  if (pend) epilogue();
  if constexpr (epi_store16(EPI)) sat_report<PREC>(amax, a.sat);
}

#ifdef MCM_ARMS
// the launch helpers the arms need are declared before the include, the arms' own launchers and routing come with it
int persistent_grid();
#include "gemm_arms.hpp"
#endif

// ---- launch ------------------------------------------------------------------------------

#ifdef MCM_HARNESS
int g_variant = -1;  // -1 auto (the shipped size policy), 0 the 128x128 tile kernel always, 3/4 persistent 256x256 (4: counted
                     // stores), 5 ping-pong 256x256 (whole tiles only, else 3), 11 the 64x128 tile kernel always; 9 the flagged
                     // ping-pong text of gemm_arms.hpp with every flag off (whole tiles, else as 5).  1/2/6/7/8: removed in round 6
int variant() { return g_variant; }
#else
constexpr int variant() { return -1; }  // the shipped library has the size policy of launch_one only
#endif

// Persistent kernels run one workgroup per CU.  The count comes from the device (a partitioned or
// CU-masked lease reports fewer than 256) and is rounded down to a multiple of 8: the tile schedule
// deals M tiles to XCDs by blockIdx % 8.
#ifdef MCM_HARNESS
int g_grid_override = 0;  // A/B (mcm_debug_persistent_grid): workgroups of the persistent kernels, 0 = one per CU
#endif
int persistent_grid() {
#ifdef MCM_HARNESS
  if (g_grid_override > 0) return g_grid_override;
#endif
  return device_cu_count() / 8 * 8;   // (cached per device, common.hpp)
}

template <int PREC, int EPI>
hipError_t launch_tile(const GemmArgs& a, hipStream_t s) {
  const int nbn = (a.N + tile::BN - 1) / tile::BN, nbm = (a.M + tile::BM - 1) / tile::BM;
  return launch_lds<gemm_tile_kernel<PREC, EPI>, tile::LDS_BYTES>(dim3(nbn * nbm), dim3(256), tile::LDS_BYTES, s, a);
}

template <int PREC, int EPI>
hipError_t launch_tile64(const GemmArgs& a, hipStream_t s) {
  const int nbn = (a.N + tile64::BN - 1) / tile64::BN, nbm = (a.M + tile64::BM - 1) / tile64::BM;
  return launch_lds<gemm_tile64_kernel<PREC, EPI>, tile64::LDS_BYTES>(dim3(nbn * nbm), dim3(256), tile64::LDS_BYTES, s, a);
}

template <int PREC, int EPI, bool CS, bool PXF = false>
hipError_t launch_p256(const GemmArgs& a, hipStream_t s) {
  return launch_lds<gemm_p256_kernel<PREC, EPI, CS, PXF>, p256::LDS_BYTES>(dim3(persistent_grid()), dim3(512), p256::LDS_BYTES, s, a);
}

template <int PREC, int EPI>
hipError_t launch_pp(const GemmArgs& a, hipStream_t s) {
  return launch_lds<gemm_pp_kernel<PREC, EPI>, p256::LDS_BYTES>(dim3(persistent_grid()), dim3(512), p256::LDS_BYTES, s, a);
}

// the size policy by tile count alone (a forced variant passes through): 0 a tile kernel, 5 ping-pong (whole tiles) or plain
// persistent.  Asked by gemm_route only, which makes a kernel family of it.
int size_policy(int M, int N) {
  int v = variant();
  if (v < 0) {  // auto: the persistent 256x256 kernel once its tiles cover most of the CUs, else the
                // one-workgroup-per-tile kernel (text tower, CLS-only last layer).  Round 1, bench.py --batch
                // 128 / 256 / 384: p256 wins from ~300 tiles on (+3 / +6 / +7 % end to end against the old >= 1024 rule).
    const long tiles = (long)((M + p256::BM - 1) / p256::BM) * ((N + p256::BN - 1) / p256::BN);
    // Round 3: the crossover is half a round of the persistent grid.  Up to G/2 tiles the tile kernel's 128x128
    // workgroups (4 per tile, 2 per CU) fit one round of their own, which takes ~0.74 of a 256x256 tile's time; one
    // tile more and they need a second round (1.47) where the persistent kernel still needs one.  Measured with the
    // rule at 129 instead of 192 tiles: batch 64 / 72 (out-proj, fc2: 150 / 171 tiles) +12 %, batch 24 +3 %, batch 96
    // and up unchanged (profiles/r03_x_kernel_choice_small_batches.txt).
    v = 2 * tiles > persistent_grid() ? 5 : 0;  // 5 falls back to 3 when the problem has edge tiles
  }
  if (v != 0 && v != 11 && persistent_grid() < 8) v = 0;
  return v;
}

// ---- routing: the ONE answer to "which kernel does this problem get, and is it cut" ------------------------------------
// launch_one switches on `family`; launch_gemm cuts the problem at `cut`; gemm_fold_kind, gemm_ln_tail_ok and
// gemm_patch_takes_pixels read `policy`.  Nothing else decides.
enum GemmFamily : int {
  FAM_TILE,     // gemm_tile_kernel, one workgroup per 128x128 tile
  FAM_TILE64,   // gemm_tile64_kernel, one workgroup per 64x128 tile
  FAM_P256,     // gemm_p256_kernel, persistent 256x256 (edge tiles, the patch epilogue)
  FAM_P256_PX,  // ... its pixel-gathering form (GemmArgs::px)
  FAM_PP,       // gemm_pp_kernel, ping-pong 256x256 (whole tiles only)
  FAM_P256_CS,  // gemm_p256_kernel with counted stores (harness variant 4)
};
struct GemmRoute {
  int policy;         // size_policy(M, N): what the arms' routing (arms::route) and the gemm_* predicates see
  GemmFamily family;  // the shipped kernel launch_one launches
  int cut;            // sliver round: rows [0, cut) and [cut, M) are launched as two problems; 0 = not cut
};
GemmRoute gemm_route(int epi, int M, int N, bool px, int hm) {
  GemmRoute r{size_policy(M, N), FAM_P256, 0};
  const int G = persistent_grid();
  const bool whole = M % p256::BM == 0 && N % p256::BN == 0;
  int v = r.policy;
#ifdef MCM_HARNESS
  if (v == 9) v = 5;  // the arms' ping-pong text took its whole-tile problems in arms::route: what is left goes as 5 does
#endif
  if (epi == EPI_PATCH && px) {
    r.family = FAM_P256_PX;  // the pixel-gathering form of the persistent kernel
  } else if (v == 0 || v == 11) {
    // 64x128 tiles when the 128x128 kernel would get fewer than two workgroups per CU (batch <= 32 at B/16, the text
    // tower's short prompts banks, B/32): twice the workgroups, the same bits (round 3: batch 8 +7.5 %, batch 16 +4.5 %)
    const bool few = (long)((M + 127) / 128) * ((N + 127) / 128) < 2L * G;
    r.family = v == 11 || (variant() < 0 && few && !MCM_HM(hm)) ? FAM_TILE64 : FAM_TILE;
  } else if (v == 4) {
    r.family = FAM_P256_CS;
  } else if (v == 5 && epi != EPI_PATCH && whole) {  // the patch epilogue remaps rows: stays with the plain kernel
    r.family = FAM_PP;
  }
#ifndef MCM_NO_SLIVER_SPLIT
  // Sliver round.  The persistent kernel walks T = row tiles x N tiles on G workgroups; when T is a little more than
  // a whole number of rounds, the last round keeps a few CUs busy for a full tile time while the rest of the chip
  // idles — ViT-B/32 at batch 512: 100 row tiles x 3 = 300 tiles on 256 workgroups, 1 round + 44 tiles, paid as 2.
  // Such a problem is cut at a row-tile boundary: the rows that fill whole rounds on every XCD (row tiles are dealt to
  // the XCDs modulo 8, 1/8 of the workgroups each) go to the ping-pong kernel, the row tiles left over to a tile
  // kernel, whose many small workgroups spread over the whole chip.  The kernels are bit-identical
  // (tests/test_gpu_kernels.py::test_linear_sliver_split_bitwise), so the result does not depend on the cut.
  if (epi != EPI_PATCH && variant() < 0 && G >= 8 && whole && r.policy == 5) {
    const long nbn = N / p256::BN, rt = M / p256::BM, T = rt * nbn, R = T / G, left = T - R * G;
    const long rt1 = 8 * ((R * (G / 8)) / nbn);  // row tiles of R whole rounds on each XCD
    // ... worth it only when the rows left over make enough 128x128 workgroups to occupy the chip: a handful of
    // them, one per CU with nobody to overlap with, take as long over a deep K as the round they replace (measured
    // at ViT-L/14, where one row tile is left: 5 918 vs 5 921 img/s; ViT-B/32, 20 row tiles: +2.9 %)
    const long rest_wgs = (rt - rt1) * 2 * (N / 128);
    // (a last round up to a quarter full; up to half full measured equal or slower at batches 64 ... 512:
    // profiles/r03_x_kernel_choice_small_batches.txt)
    // ... and only when the left-over rows are a problem the size policy hands to the tile kernel (with a wide N the floor
    // in rt1 can leave up to 8 nbn - 1 tiles, more than half a round: those would go back to a persistent kernel as a
    // second ragged round — ADVICE r3)
    if (R >= 1 && left > 0 && left * 4 <= G && rt1 >= 1 && rt1 < rt && rest_wgs * 2 >= G &&
        size_policy((int)(rt1 * p256::BM), N) == 5 && size_policy((int)((rt - rt1) * p256::BM), N) == 0)
      r.cut = (int)(rt1 * p256::BM);
  }
#endif
  return r;
}

template <int PREC, int EPI>
hipError_t launch_one(const GemmArgs& a, hipStream_t s) {
  if constexpr (epi_x2(EPI) && PREC != MCM_PREC_F16) {  // the split-output epilogues: fp16 only
    return hipErrorInvalidValue;
  } else {
    const GemmRoute r = gemm_route(EPI, a.M, a.N, a.px != nullptr, a.hm);
    // (... and the shipped kernels only, never an A/B arm: launch_gemm has refused a forced variant, hm and px with them)
    if constexpr (!epi_x2(EPI)) {
#ifdef MCM_ARMS
      int v = r.policy;
      if constexpr (epi_erf(EPI)) {  // the erf epilogue lives in the shipped kernels only: an arm would apply QuickGELU (or nothing)
        if (a.fold_z || a.fold_rs || a.ln_y || a.lnc || a.wblk || v == 9) return hipErrorInvalidValue;  // (9: the arms' ping-pong text)
      } else {  // A/B builds: the LayerNorm fold / tail forms and the forced arm variants (gemm_arms.hpp)
        hipError_t e;
        if (arms::route<PREC, EPI>(v, a, s, &e)) return e;
      }
#else
      if (a.fold_z || a.fold_rs || a.ln_y || a.lnc || a.wblk) return hipErrorInvalidValue;  // A/B arms: not in the shipped library
#endif
    }
    switch (r.family) {
      case FAM_TILE: return launch_tile<PREC, EPI>(a, s);
      case FAM_TILE64: return launch_tile64<PREC, EPI>(a, s);
      case FAM_PP:
        if constexpr (EPI != EPI_PATCH) return launch_pp<PREC, EPI>(a, s);
        break;
      case FAM_P256_PX:
        if constexpr (EPI == EPI_PATCH) return launch_p256<PREC, EPI, false, true>(a, s);
        break;
      case FAM_P256_CS:
#ifdef MCM_HARNESS
        if constexpr (!epi_x2(EPI)) return launch_p256<PREC, EPI, true>(a, s);
#endif
        break;
      case FAM_P256: break;
    }
    return launch_p256<PREC, EPI, false>(a, s);
  }
}

template <int PREC>
hipError_t launch_prec(int epi, const GemmArgs& a, hipStream_t s) {
  switch (epi) {
    case EPI_STORE_X2: return launch_one<PREC, EPI_STORE_X2>(a, s);
    case EPI_GELU_X2: return launch_one<PREC, EPI_GELU_X2>(a, s);
    case EPI_GELU_ERF_X2: return launch_one<PREC, EPI_GELU_ERF_X2>(a, s);
    case EPI_STORE: return launch_one<PREC, EPI_STORE>(a, s);
    case EPI_GELU: return launch_one<PREC, EPI_GELU>(a, s);
    case EPI_GELU_ERF: return launch_one<PREC, EPI_GELU_ERF>(a, s);
    case EPI_RESID: return launch_one<PREC, EPI_RESID>(a, s);
    case EPI_PATCH: return launch_one<PREC, EPI_PATCH>(a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

#ifdef MCM_HARNESS
void gemm_set_variant(int v) { g_variant = v; }
int g_group_n = 0;  // 0 = heuristic
int g_dbg = 0;
void gemm_set_dbg(int d) { g_dbg = d; }
void gemm_set_group_n(int gn) { g_group_n = gn > 0 ? gn : 0; }
#else
constexpr int g_group_n = 0, g_dbg = 0;
#endif

#ifdef MCM_HARNESS
void gemm_set_persistent_grid(int n) { g_grid_override = n; }
hipError_t launch_lnc_cleanup(int prec, const float* x, const float* g, const float* b, void* y, const float2* part, int M, int D,
                              float eps, unsigned int* ln_state, int ln_rs, int ln_cap8, hipStream_t s, unsigned int* sat) {
  if (prec == MCM_PREC_F16) return arms::launch_lnc_cleanup_p<MCM_PREC_F16>(x, g, b, y, part, M, D, eps, ln_state, ln_rs, ln_cap8, s, sat);
  if (prec == MCM_PREC_BF16) return arms::launch_lnc_cleanup_p<MCM_PREC_BF16>(x, g, b, y, part, M, D, eps, ln_state, ln_rs, ln_cap8, s, sat);
  return hipErrorInvalidValue;
}
hipError_t launch_row64_block_w(const void* w, void* blocked, int N, int K, hipStream_t s) {
  if (N % 16 || K % 32) return hipErrorInvalidValue;
  const size_t nchunks = (size_t)N * K / 8;
  hipLaunchKernelGGL(arms::row64_block_w_kernel, dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0, s, (const uint4*)w, (uint4*)blocked, N, K);
  return hipGetLastError();
}
hipError_t launch_gemm_row64_ln(int prec, const GemmArgs& a, hipStream_t s, int stages) {
  if (prec == MCM_PREC_F16) return arms::launch_row64_ln_p<MCM_PREC_F16>(a, s, stages);
  if (prec == MCM_PREC_BF16) return arms::launch_row64_ln_p<MCM_PREC_BF16>(a, s, stages);
  return hipErrorInvalidValue;
}
#endif
int gemm_persistent_grid() { return persistent_grid(); }  // workgroups of the persistent kernels (one per CU, multiple of 8)
// LayerNorm in the tail: whether launch_gemm takes a residual GEMM of this size with GemmArgs::ln_y set (the ping-pong
// kernel, whole tiles, rows of at most 1024 columns); the host then does not launch the LayerNorm that follows
bool gemm_ln_tail_ok(int prec, int M, int N) {
#if !defined(MCM_HARNESS) && !defined(MCM_LN_TAIL)
  return false;  // the arm is not in this build
#endif
  if (prec == MCM_PREC_F32 || M <= 0 || M % p256::BM || (N != 768 && N != 1024)) return false;
  return gemm_route(EPI_RESID, M, N, false, 0).policy == 5 && persistent_grid() >= 8;
}

// The patch GEMM can gather its A operand from the NCHW fp32 pixels (GemmArgs::px) when the problem is one the persistent
// kernel takes anyway and the patch geometry fits a K-step: P | K-step elements, P a multiple of the chunk, no K padding.
bool gemm_patch_takes_pixels(int prec, int M, int N, int kpad, int patch, int image) {
  const int es = prec_esize(prec), ks = ROWB / es, ec = 16 / es;
  if (patch <= 0 || image % patch || patch % ec || ks % patch || kpad != 3 * patch * patch) return false;
  if ((size_t)M / ((size_t)(image / patch) * (image / patch)) * 3 * image * image * 4 >= (1ull << 32)) return false;  // 32-bit lane offsets
  return gemm_route(EPI_PATCH, M, N, true, 0).policy != 0 && persistent_grid() >= 8;
}

int gemm_fold_kind(int epi, int M, int N) {
  if (epi == EPI_PATCH || epi_erf(epi) || M <= 0 || N <= 0) return 0;  // (the fold's consumer epilogue is QuickGELU's)
  const int v = gemm_route(epi, M, N, false, 0).policy;
  return v == 5 && M % p256::BM == 0 && N % p256::BN == 0 ? 1 : v == 0 ? 2 : 0;
}

static hipError_t launch_gemm_one(int prec, int epi, const GemmArgs& a, hipStream_t s) {
  switch (prec) {
    case MCM_PREC_BF16: return launch_prec<MCM_PREC_BF16>(epi, a, s);
    case MCM_PREC_F16: return launch_prec<MCM_PREC_F16>(epi, a, s);
    case MCM_PREC_F32: return launch_prec<MCM_PREC_F32>(epi, a, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_gemm(int prec, int epi, const GemmArgs& a_in, hipStream_t s) {
  GemmArgs a = a_in;
  const int es = prec_esize(prec);
  if (a.gn <= 0) {
    // L2 grouping of the persistent tile walk (N-tiles per group).  In the standalone harness
    // gn=1 looked 4-7 % faster on the wide short-K shapes, but inside the model (operands
    // still warm in L2 / Infinity Cache from the producing kernel) the plain n-fastest walk
    // wins on every shape: 914 vs 822 TF/s family average (the harness can override).
    const int nbn = (a.N + 255) / 256;
    a.gn = g_group_n > 0 ? g_group_n : nbn;
  }
  a.dbg = g_dbg;
  if (a.M <= 0 || a.N <= 0 || a.K <= 0 || (a.K * es) % ROWB || a.N % 16 || (a.ldx * es) % 16 ||
      a.ldo % 4)
    return hipErrorInvalidValue;
  // split weights: 16-bit modes, an even number of K-steps (hi, lo pairs); the shipped kernels only
  if (a.ksplit && (a.ksplit != 1 || prec == MCM_PREC_F32 || ((a.K * es) / ROWB) % 2 || a.fold_z || a.fold_rs || a.ln_y))
    return hipErrorInvalidValue;
  // split activations / split outputs: fp16, the shipped kernels, rows of whole 64-column blocks; the pixel-gathering patch
  // GEMM reads fp32 pixels, not a split image (the caller runs patchify)
  if ((a.xsplit || epi_x2(epi)) && (prec != MCM_PREC_F16 || (a.xsplit != 0 && a.xsplit != 1) || a.fold_z || a.fold_rs || a.ln_y ||
                                    a.hm || a.px || variant() >= 0))
    return hipErrorInvalidValue;
  if (a.xsplit && a.ldx % 128) return hipErrorInvalidValue;
  if (epi_x2(epi) && (a.N % 64 || a.ldo % 128)) return hipErrorInvalidValue;
  // head-major outputs: the 16-bit store epilogues of the A/B arm only (bias, QuickGELU), whole 64-column blocks
  if (a.hm && (a.hm < a.M || a.N % 64 || !(epi == EPI_STORE || epi == EPI_GELU) || prec == MCM_PREC_F32)) return hipErrorInvalidValue;
#ifndef MCM_HARNESS
  if (a.hm) return hipErrorInvalidValue;  // the head-major store path exists in the harness library only
#endif
  // sliver round (gemm_route): the rows that fill whole rounds of the ping-pong kernel, then the rest on a tile kernel.  The
  // LayerNorm arms take their problems whole.
  const int cut = gemm_route(epi, a.M, a.N, a.px != nullptr, a.hm).cut;
  if (cut && !a.fold_z && !a.fold_rs && !a.ln_y) {
    GemmArgs m = a, r = a;
    const size_t row0 = (size_t)cut;
    m.M = cut;
    r.M = a.M - cut;
    r.x = (const char*)a.x + row0 * a.ldx * es;
    if (a.out) r.out = (char*)a.out + (a.hm ? row0 * 64 : row0 * a.ldo) * es;
    if (a.resid) r.resid = a.resid + row0 * a.ldo;
    hipError_t e = launch_gemm_one(prec, epi, m, s);
    return e != hipSuccess ? e : launch_gemm_one(prec, epi, r, s);
  }
  return launch_gemm_one(prec, epi, a, s);
}

