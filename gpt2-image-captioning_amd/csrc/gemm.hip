#include <cstdlib>

#include "gemm_tile.h"
#include "gemm_launch.h"

namespace icap {

// Skinny-M GEMM (M <= 128: greedy-decode steps over the batch, CLIP projection, mapper input Linear).
// A weight-streaming, latency-bound problem: block = 8 waves over a 16*NT-column slab of B (= W rows) and a
// 16*MT-row slab of A (grid.y walks M, so no block streams all of A through its CU: per-CU L2 bandwidth, not
// HBM, bounded the all-rows form); the waves split the K steps round-robin and keep SK_U steps of MFMA
// fragments in flight each (range-checked buffer loads straight from HBM/L2). The fp32 partial tiles are reduced
// through LDS in two rounds before the shared epilogue. One launch, no slabs.
// Accumulators use the C layout (lane = column, 4 consecutive rows per lane).
// one 16-byte A chunk -> LayerNorm-ed chunk in the input dtype
template <typename TI>
__device__ __forceinline__ uint4 ln_chunk(const uint4 a, float mean, float rs, const float* g, const float* bt);
template <>
__device__ __forceinline__ uint4 ln_chunk<bf16_t>(const uint4 a, float mean, float rs, const float* g, const float* bt) {
  const uint32_t w[4] = {a.x, a.y, a.z, a.w};
  uint32_t o[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float v0 = (__uint_as_float(w[q] << 16) - mean) * rs * g[2 * q] + bt[2 * q];
    const float v1 = (__uint_as_float(w[q] & 0xffff0000u) - mean) * rs * g[2 * q + 1] + bt[2 * q + 1];
    o[q] = f2bf2(v0, v1);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}
template <>
__device__ __forceinline__ uint4 ln_chunk<float>(const uint4 a, float mean, float rs, const float* g, const float* bt) {
  return make_uint4(__float_as_uint((__uint_as_float(a.x) - mean) * rs * g[0] + bt[0]),
                    __float_as_uint((__uint_as_float(a.y) - mean) * rs * g[1] + bt[1]),
                    __float_as_uint((__uint_as_float(a.z) - mean) * rs * g[2] + bt[2]),
                    __float_as_uint((__uint_as_float(a.w) - mean) * rs * g[3] + bt[3]));
}

// v + the same register of lane ^ 16 / lane ^ 32 on the VALU's cross-lane paths (v_permlane16_swap /
// v_permlane32_swap; the bits equal v + __shfl_xor(v, 16 / 32), whose ds_bpermute is an LDS round trip each)
__device__ __forceinline__ float xor16_sum(float v) {
  const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v),
                                                   false, false);
  return __builtin_bit_cast(float, (unsigned)sw[0]) + __builtin_bit_cast(float, (unsigned)sw[1]);
}
__device__ __forceinline__ float xor32_sum(float v) {
  const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v),
                                                   false, false);
  return __builtin_bit_cast(float, (unsigned)sw[0]) + __builtin_bit_cast(float, (unsigned)sw[1]);
}

constexpr int SK_LNK = 1280;  // LN-fused launches up to this K stage gamma / beta in LDS
// NT: 16-column slabs per block (the host picks the fewest that fit the grid in one pass over the CUs);
// SKU: k-steps in flight per wave (the host picks enough for one memory round trip over all of K where the
// registers allow). Neither changes the arithmetic: every wave accumulates its steps in step order and the waves
// are summed in a fixed order, so all (NT, SKU) instantiations store bitwise-identical outputs.
template <typename TI, typename TC, int NT, int MT, int SKU>
__global__ __launch_bounds__(64 * SK_WAVES) void gemm_skinny_kernel(icap_gemm_args p, uint32_t drop_thresh,
                                                                  float inv_keep) {
  constexpr int ES = sizeof(TI);
  constexpr int EPC = 16 / ES;        // K elements per lane chunk
  constexpr int KSTEP = 4 * EPC;      // K elements per MFMA chunk step (4 lane groups)
  constexpr int BN = 16 * NT;
  constexpr int RLD = BN + 4;         // fp32 stride of the LDS partial tiles
  constexpr int HALF = SK_WAVES / 2;
  constexpr int BM = 16 * MT;
  constexpr int QPR = BN / 4;         // 4-column epilogue quads per row
  static_assert(BM * QPR <= 64 * SK_WAVES, "one epilogue quad per thread");
  __shared__ __attribute__((aligned(16))) float red[HALF][BM * RLD];
  __shared__ __attribute__((aligned(16))) float lngb[2 * SK_LNK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int64_t N = p.N, K = p.K;
  const int64_t n0 = (int64_t)blockIdx.x * BN, m0 = (int64_t)blockIdx.y * BM;
  const int64_t M = p.m_dev && (int64_t)*p.m_dev < p.M ? (int64_t)*p.m_dev : p.M;  // device row count
  if (m0 >= M) return;
  const int64_t nrows = N - n0 < BN ? N - n0 : BN;
  const int64_t mrows = M - m0 < BM ? M - m0 : BM;
  const __amdgpu_buffer_rsrc_t ra =
      make_rsrc(reinterpret_cast<const char*>(p.A) + m0 * p.lda * ES, (uint64_t)((mrows - 1) * p.lda + K) * ES);
  const __amdgpu_buffer_rsrc_t rb =
      make_rsrc(reinterpret_cast<const char*>(p.B) + n0 * p.ldb * ES, (uint64_t)((nrows - 1) * p.ldb + K) * ES);
  f32x4_t acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  // rows past M / N lie beyond the descriptor range (zero-filled); K-tail chunks and steps past the end are
  // redirected out of range (zero fragments: the MFMAs on them add nothing)
  uint32_t aoff[MT], boff[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) aoff[i] = (uint32_t)(((i * 16 + fr) * p.lda + fg * EPC) * ES);
#pragma unroll
  for (int j = 0; j < NT; ++j) boff[j] = (uint32_t)(((j * 16 + fr) * p.ldb + fg * EPC) * ES);
  const int64_t nks = (K + KSTEP - 1) / KSTEP;
  uint4 af[SKU][MT], bfr[SKU][NT];
  auto load_steps = [&](int64_t base) {  // steps past the end load zero fragments (the MFMAs add nothing)
#pragma unroll
    for (int u = 0; u < SKU; ++u) {
      const int64_t k0 = (base + (int64_t)u * SK_WAVES) * KSTEP;
      const bool kin = k0 + fg * EPC < K;
      const uint32_t kb = (uint32_t)(k0 * ES);
#pragma unroll
      for (int j = 0; j < NT; ++j) bfr[u][j] = bload(rb, kin ? boff[j] + kb : OOB);
#pragma unroll
      for (int i = 0; i < MT; ++i) af[u][i] = bload(ra, kin ? aoff[i] + kb : OOB);
    }
  };
  // LN gamma / beta (K <= SK_LNK) are loaded first, so storing them to LDS waits for these loads only, not for
  // the fragment loads behind them
  const bool fuse_ln = p.ln_gamma != nullptr;
  const bool ln_lds = fuse_ln && K <= SK_LNK;
  constexpr int LNS = (SK_LNK + 64 * SK_WAVES - 1) / (64 * SK_WAVES);  // gamma (and beta) values per thread
  float lg[LNS], lb[LNS];
  if (ln_lds) {
#pragma unroll
    for (int q = 0; q < LNS; ++q) {
      const int k = threadIdx.x + q * 64 * SK_WAVES;
      lg[q] = k < K ? p.ln_gamma[k] : 0.f;
      lb[q] = k < K ? p.ln_beta[k] : 0.f;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // every wave runs at least one (possibly all-zero) pass, so the LN-stats barrier below is block-uniform
  load_steps(wave);
  // LayerNorm statistics from the fragments (below): each row's first element, issued with the fragment loads
  // (instantiations with few fragment registers only: the others would spill; LN-fused launches have K = D)
  constexpr bool LN_FRAG = ES == 2 && SKU * (MT + NT) <= 24;
  const bool fold = p.ln_wsum != nullptr;
  const bool ln_frag = LN_FRAG && (fuse_ln || fold) && nks <= (int64_t)SK_WAVES * SKU;
  uint4 x0raw[MT];
  if (LN_FRAG && ln_frag) {
#pragma unroll
    for (int i = 0; i < MT; ++i) x0raw[i] = bload(ra, (uint32_t)((i * 16 + fr) * p.lda * ES));  // rows past M: zero
  }
  __builtin_amdgcn_sched_barrier(0);
  if (ln_lds) {
#pragma unroll
    for (int q = 0; q < LNS; ++q) {
      const int k = threadIdx.x + q * 64 * SK_WAVES;
      if (k < K) {
        lngb[k] = lg[q];
        lngb[SK_LNK + k] = lb[q];
      }
    }
  }

  // Epilogue operands, fetched now so their latency hides under the main loop's: one 4-column quad per thread
  // (bias; the bf16 residual, or dact_src in the backward form, for full quads).
  const int er = threadIdx.x / QPR, ec = (threadIdx.x - er * QPR) * 4;
  const int64_t erow = m0 + er, ecol = n0 + ec;
  const bool eact = threadIdx.x < BM * QPR && erow < M && ecol < N;
  float bias4[4] = {0.f, 0.f, 0.f, 0.f};
  float wsum4[4] = {0.f, 0.f, 0.f, 0.f};  // (folded LayerNorm: W row sums, fetched here, not after the reduction)
  uint2 pre = make_uint2(0u, 0u);
  bool use_pre = false;
  if (eact) {
    // one 16-byte load per operand for a full, aligned quad (the bias / wsum vectors of the decode launches)
    auto quad = [&](const float* v, float* dst) {
      if (ecol + 4 <= N && (reinterpret_cast<uintptr_t>(v + ecol) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(v + ecol);
        dst[0] = q.x; dst[1] = q.y; dst[2] = q.z; dst[3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[e] = (ecol + e < N) ? v[ecol + e] : 0.f;
      }
    };
    if (p.bias && p.dact == ICAP_ACT_NONE) quad(p.bias, bias4);
    if (p.ln_wsum) quad(p.ln_wsum, wsum4);
    if constexpr (sizeof(TC) == 2) {
      const bf16_t* src = reinterpret_cast<const bf16_t*>(p.dact != ICAP_ACT_NONE ? p.dact_src : p.resid);
      const int64_t lds_ = p.dact != ICAP_ACT_NONE ? p.ld_dact : p.ldr;
      if (src && ecol + 4 <= N && (lds_ & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 7) == 0) {
        pre = *reinterpret_cast<const uint2*>(src + erow * lds_ + ecol);
        use_pre = true;
      }
    }
  }

  // LayerNorm-fused A (icap_gemm_args.ln_gamma): mean / rstd of the block's rows over all K (two passes: mean,
  // then the centred sum of squares), then (x - mean) * rstd * gamma + beta -> input dtype per fragment.
  // bf16 with every k-step in registers (nks <= 8 SKU, the decode launches): the statistics come from the
  // fragments themselves (lane sums -> the 4 lane groups -> the 8 waves through LDS, fixed order), so LN costs no
  // extra global reads; otherwise the loop form (16 threads per row, the order and rounding of ln_fwd8_kernel).
  // gamma / beta are staged in LDS when K <= SK_LNK (above); the barriers below publish them.
  __shared__ float ln_mr[BM][2];
  __shared__ float lnp[SK_WAVES][BM];
  __shared__ float lnp2[SK_WAVES][BM];
  // folded LayerNorm (icap_gemm_args.ln_wsum): the same row statistics, but only the epilogue needs them
  // (C = rstd (A.B^T - mean wsum) + bias), so the MFMAs run on the raw fragments without waiting for them: the
  // wave partials are computed after the MFMAs are issued (the VALU pass overlaps the matrix cores), go to LDS and
  // are summed by the epilogue threads after the partial-tile reduction barrier
  float ln_mean[MT], ln_rs[MT];
  // one pass over the fragments: per-row sums of (x - x0) and (x - x0)^2 with x0 the row's first element (the
  // shifted-data form: no cancellation between E[x^2] and mean^2 when |mean| >> std), reduced together (lane
  // groups by shuffles, the 8 waves through LDS in a fixed order); mean = x0 + E[d], var = E[d^2] - E[d]^2
  auto frag_stats = [&]() {
    auto chunk_in = [&](int u) { return (int64_t)(wave + u * SK_WAVES) * KSTEP + fg * EPC < K; };
    float part[MT], part2[MT], x0[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float v0[8];
      unpack_bf16(x0raw[i], v0);
      x0[i] = v0[0];
      part[i] = 0.f;
      part2[i] = 0.f;
#pragma unroll
      for (int u = 0; u < SKU; ++u) {
        if (chunk_in(u)) {
          const int64_t kc = (int64_t)(wave + u * SK_WAVES) * KSTEP + fg * EPC;
          float v[8];
          unpack_bf16(af[u][i], v);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float d = kc + e < K ? v[e] - x0[i] : 0.f;
            part[i] += d;
            part2[i] += d * d;
          }
        }
      }
      part[i] = xor32_sum(xor16_sum(part[i]));
      part2[i] = xor32_sum(xor16_sum(part2[i]));
      if (fg == 0) {
        lnp[wave][i * 16 + fr] = part[i];
        lnp2[wave][i * 16 + fr] = part2[i];
        if (fold && wave == 0) ln_mr[i * 16 + fr][0] = x0[i];
      }
    }
  };
  if (LN_FRAG && ln_frag && fuse_ln) {
    frag_stats();
    {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        float t = 0.f, t2 = 0.f;
#pragma unroll
        for (int w = 0; w < SK_WAVES; ++w) {
          t += lnp[w][i * 16 + fr];
          t2 += lnp2[w][i * 16 + fr];
        }
        const float dm = t / (float)K;
        float v0[8];
        unpack_bf16(x0raw[i], v0);
        ln_mean[i] = v0[0] + dm;
        const float var = t2 / (float)K - dm * dm;
        ln_rs[i] = 1.f / sqrtf((var > 0.f ? var : 0.f) + p.ln_eps);
      }
    }
  } else if ((fuse_ln || fold) && !(LN_FRAG && ln_frag)) {
    const int t = threadIdx.x & 15;
    for (int rr = threadIdx.x >> 4; rr < BM; rr += 64 * SK_WAVES / 16) {
      const int64_t row = m0 + rr < M ? m0 + rr : M - 1;
      const TI* xr = reinterpret_cast<const TI*>(p.A) + row * p.lda;
      float s = 0.f;
      for (int64_t k = (int64_t)t * EPC; k < K; k += 16 * EPC) {
        float v[EPC];
        if constexpr (EPC == 8) io<TI>::ld8(xr + k, v); else io<TI>::ld4(xr + k, v);
#pragma unroll
        for (int e = 0; e < EPC; ++e) s += v[e];
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      const float mean = s / (float)K;
      float s2 = 0.f;
      for (int64_t k = (int64_t)t * EPC; k < K; k += 16 * EPC) {
        float v[EPC];
        if constexpr (EPC == 8) io<TI>::ld8(xr + k, v); else io<TI>::ld4(xr + k, v);
#pragma unroll
        for (int e = 0; e < EPC; ++e) s2 += (v[e] - mean) * (v[e] - mean);
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
      if (t == 0) {
        ln_mr[rr][0] = mean;
        ln_mr[rr][1] = 1.f / sqrtf(s2 / (float)K + p.ln_eps);
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      ln_mean[i] = ln_mr[i * 16 + fr][0];
      ln_rs[i] = ln_mr[i * 16 + fr][1];
    }
  }
  for (int64_t base = wave;;) {
    // all SKU steps' loads are issued before the first MFMA waits (without this fence hipcc sinks each load
    // to its use and every MFMA waits out a full memory latency)
    __builtin_amdgcn_sched_barrier(0);
    if (fuse_ln) {
#pragma unroll
      for (int u = 0; u < SKU; ++u) {
        const int64_t k0 = (base + (int64_t)u * SK_WAVES) * KSTEP + fg * EPC;
        if (k0 < K) {  // K-tail / past-the-end chunks stay zero
          float g[EPC], bt[EPC];
          if (ln_lds) {
#pragma unroll
            for (int e = 0; e < EPC; e += 4) {
              const float4 gv = *reinterpret_cast<const float4*>(&lngb[k0 + e]);
              const float4 bv = *reinterpret_cast<const float4*>(&lngb[SK_LNK + k0 + e]);
              g[e] = gv.x; g[e + 1] = gv.y; g[e + 2] = gv.z; g[e + 3] = gv.w;
              bt[e] = bv.x; bt[e + 1] = bv.y; bt[e + 2] = bv.z; bt[e + 3] = bv.w;
            }
          } else if constexpr (EPC == 8) {
            io<float>::ld8(p.ln_gamma + k0, g); io<float>::ld8(p.ln_beta + k0, bt);
          } else {
            io<float>::ld4(p.ln_gamma + k0, g); io<float>::ld4(p.ln_beta + k0, bt);
          }
#pragma unroll
          for (int i = 0; i < MT; ++i) af[u][i] = ln_chunk<TI>(af[u][i], ln_mean[i], ln_rs[i], g, bt);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < SKU; ++u)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) mfma_chunk<TI>(acc[i][j], af[u][i], bfr[u][j]);
    base += SK_WAVES * SKU;
    if (base >= nks) break;
    load_steps(base);
  }
  if (LN_FRAG && ln_frag && !fuse_ln) frag_stats();  // folded: one pass, after the MFMAs are issued
  // round 1: waves [HALF, 2 HALF) park their partials, waves [0, HALF) add them; round 2: the HALF sums -> LDS
  auto park = [&](float* dst) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int v = 0; v < 4; ++v) dst[(i * 16 + fg * 4 + v) * RLD + j * 16 + fr] = acc[i][j][v];
  };
  if (wave >= HALF) park(red[wave - HALF]);
  __syncthreads();
  if (wave < HALF) {
    const float* src = red[wave];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[i][j][v] += src[(i * 16 + fg * 4 + v) * RLD + j * 16 + fr];
    park(red[wave]);  // same addresses this lane just read: no cross-lane hazard
  }
  __syncthreads();
  if (!eact) return;
  const uint64_t seed = drop_thresh != 0u ? eff_seed(p.seed, p.seed_ptr) : 0ull;
  float x[4];
  *reinterpret_cast<float4*>(x) = *reinterpret_cast<const float4*>(&red[0][er * RLD + ec]);
#pragma unroll
  for (int w = 1; w < HALF; ++w) {
    const float4 v = *reinterpret_cast<const float4*>(&red[w][er * RLD + ec]);
    x[0] += v.x; x[1] += v.y; x[2] += v.z; x[3] += v.w;
  }
  if (fold) {  // rstd (acc - mean wsum); the host passed bias = b + W . beta
    float mean, rs;
    if (ln_frag) {  // the wave partials in wave order (the order of the LN-fused form above)
      float t = 0.f, t2 = 0.f;
#pragma unroll
      for (int w = 0; w < SK_WAVES; ++w) {
        t += lnp[w][er];
        t2 += lnp2[w][er];
      }
      const float dm = t / (float)K;
      mean = ln_mr[er][0] + dm;
      const float var = t2 / (float)K - dm * dm;
      rs = 1.f / sqrtf((var > 0.f ? var : 0.f) + p.ln_eps);
    } else {
      mean = ln_mr[er][0];
      rs = ln_mr[er][1];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = ecol + e < N ? rs * (x[e] - mean * wsum4[e]) : x[e];
  }
  // two call sites rather than a selected pointer (a pointer select on a local puts it in scratch)
  if (use_pre) epiw<TC, 4>(p, erow, ecol, x, bias4, ecol + 4 <= N, seed, drop_thresh, inv_keep, &pre);
  else epiw<TC, 4>(p, erow, ecol, x, bias4, ecol + 4 <= N, seed, drop_thresh, inv_keep);
}

// Split-K reduction: sum the fp32 partial slabs of `splits` K-ranges in a fixed order (deterministic) and
// apply the full epilogue. One thread per 4 consecutive columns.
template <typename TC>
__global__ __launch_bounds__(256) void gemm_splitk_reduce(icap_gemm_args p, int splits, uint32_t drop_thresh,
                                                         float inv_keep) {
  const int64_t M = p.M, N = p.N;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n4 = N >> 2;
  if (q >= M * n4) return;
  const int64_t row = q / n4, col = (q - row * n4) * 4;
  if (p.m_dev && row >= (int64_t)*p.m_dev) return;
  const float* ws = reinterpret_cast<const float*>(p.workspace) + row * N + col;
  float x[4];
  *reinterpret_cast<float4*>(x) = *reinterpret_cast<const float4*>(ws);
  for (int s = 1; s < splits; ++s) {
    const float4 v = *reinterpret_cast<const float4*>(ws + (int64_t)s * M * N);
    x[0] += v.x; x[1] += v.y; x[2] += v.z; x[3] += v.w;
  }
  float bias4[4] = {0.f, 0.f, 0.f, 0.f};
  if (p.bias && p.dact == ICAP_ACT_NONE) {
#pragma unroll
    for (int e = 0; e < 4; ++e) bias4[e] = p.bias[col + e];  // flat-parameter views: only 4-byte aligned
  }
  const uint64_t seed = drop_thresh != 0u ? eff_seed(p.seed, p.seed_ptr) : 0ull;
  epi4<TC>(p, row, col, x, bias4, true, seed, drop_thresh, inv_keep);
}


// ---------------------------------------------------------------------------------------------------------------
}  // namespace icap

using namespace icap;

// compute units of the current device (the skinny-GEMM grid rule, the 256 x 256 kernel's pick)
static int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

namespace icap {
int gemm256_launch(const icap_gemm_args& p, uint32_t thr, float inv_keep, hipStream_t s);
int gemm8p_launch(const GemmPlan& pl, const icap_gemm_args& p, hipStream_t s);
}

// ICAP_GEMM_DIAG = 1 / 2 / 3: drop the A / B / both operands' staging loads of the tile kernels (zero-record
// descriptors) — a timing diagnostic for what the operand traffic costs; the outputs are wrong. Never in a real run.
// ICAP_FUSED_ACQUIRE=1: the in-launch split-K's last arriver runs an agent-scope acquire after its ticket poll
static int gemm_acquire() { return diag_env("ICAP_FUSED_ACQUIRE", 0) == 1 ? 1 : 0; }
// (diagnostic build, read per launch: an A/B driver toggles it in one process)
static int gemm_diag() { return diag_env("ICAP_GEMM_DIAG", 0) & 3; }

// the launcher (one translation unit each) of the tile-kernel family plan pl selects, nullptr for a number that is no
// variant
typedef int (*TileLauncher)(const GemmPlan&, const icap_gemm_args&, int, hipStream_t);
static TileLauncher tile_launcher(const GemmPlan& pl, const icap_gemm_args& p) {
  switch (pl.variant) {
    case V_ROLES_KOUT: return launch_tile_roles_kout;
    case V_ROLES: return launch_tile_roles;
    case V_ROLES160: return launch_tile_roles160;
    case V_ROLES96: return launch_tile_roles96;
    case V_ROLES192: return launch_tile_roles192;
    case V_R256: return launch_tile_r256;
    case V_W192: case V_W192_RING: return launch_tile_w192;
    case V_KOUT_DB: case V_KOUT_S3: return launch_tile_kout;
    case V_DB: case V_S3: case V_S4: case V_N12: case V_N13: case V_RING:
      if (pl.actk >= ACT_LNS) return launch_tile_ln;    // the LayerNorm statistics hand-off
      if (pl.actk >= ACT_FWD) return launch_tile_act;   // specialised activations
      return p.in_dtype == ICAP_BF16 ? launch_tile_bf16 : p.in_dtype == ICAP_FP8_MX ? launch_tile_mx : launch_tile_f32;
  }
  return nullptr;
}

extern "C" const char* icap_gemm_kernel_name(const icap_gemm_args* a) {
  if (a == nullptr) return nullptr;
  GemmPlan pl;
  if (gemm_plan(*a, pl, device_cus(), plan_diag()) != ICAP_OK) return nullptr;
  return gemm_plan_kernel_name(*a, pl);
}

extern "C" int icap_gemm_plan_info(const icap_gemm_args* a, int32_t* splits, int32_t* fused) {
  ICAP_REQUIRE(a != nullptr && splits != nullptr && fused != nullptr, "icap_gemm_plan_info: null pointer");
  GemmPlan pl;
  const int rc = gemm_plan(*a, pl, device_cus(), plan_diag());
  if (rc != ICAP_OK) return rc;
  *splits = pl.skinny || pl.g256 || pl.g8p ? 1 : pl.splits;
  *fused = pl.fused ? 1 : 0;
  return ICAP_OK;
}

// ICAP_GROUP128=1: icap_gemm_group keeps the 128 x 128 body for every group (A/B runs and the tests that compare the
// two bodies bit for bit). The one variable the product library reads, at every grouped call and not once, so that one
// process can run both; a captured graph keeps the body it was captured with.
static bool group_force128() {
  const char* e = std::getenv("ICAP_GROUP128");
  return e != nullptr && std::atoi(e) == 1;
}

extern "C" int icap_gemm_group(const icap_gemm_args* a, int32_t n, void* stream) {
  ICAP_REQUIRE(a != nullptr && n >= 1 && n <= ICAP_GEMM_GROUP_MAX, "icap_gemm_group: 1 ... 8 products");
  static_assert(ICAP_GEMM_GROUP_MAX == GROUP_MAX, "the group's planner and its kernel argument hold the same count");
  GemmGroup g;
  g.n = 0;
  g.swap = 0;
  g.tstart[0] = 0;
  int64_t Ms[ICAP_GEMM_GROUP_MAX], Ns[ICAP_GEMM_GROUP_MAX];
  for (int i = 0; i < n; ++i) {
    const icap_gemm_args& p = a[i];
    // (the general argument checks of a single unsplit product on the automatic path, then the group's own
    // preconditions)
    icap_gemm_args q = p;
    q.split_k = 1;
    q.path = 0;
    if (const int rc = gemm_validate(q); rc != ICAP_OK) return rc;
    ICAP_REQUIRE(p.trans_ab && p.in_dtype == ICAP_BF16 && p.c_dtype == ICAP_F32,
                 "icap_gemm_group: K-outer (trans_ab) bf16 products with an fp32 C");
    ICAP_REQUIRE(p.act == ICAP_ACT_NONE && p.dact == ICAP_ACT_NONE && !p.bias && !p.resid && !p.aux && !p.ln_gamma &&
                     !p.ln_wsum && !p.ln_stats_in && !p.ln_stats_out && p.drop_p == 0.f && !p.m_dev,
                 "icap_gemm_group: plain products only (alpha, beta; no epilogue operands)");
    if (p.M == 0 || p.N == 0) continue;
    ICAP_REQUIRE(p.K > 0, "icap_gemm_group: K must be positive");
    const int k = g.n;
    g.a[k] = p;
    g.a[k].split_k = 1;
    g.a[k].tickets = nullptr;
    g.nk[k] = (int)((p.K + 63) / 64) | (gemm_diag() << 28);  // (diagnostic build: ICAP_GEMM_DIAG, as in icap_gemm)
    Ms[k] = p.M, Ns[k] = p.N;
    ++g.n;
  }
  if (g.n == 0) return ICAP_OK;
  const int cus = (int)device_cus();
  const GroupPlan gp = gemm_group_plan(Ms, Ns, g.n, cus, group_force128());
  ICAP_REQUIRE(gp.total < (1ll << 30), "icap_gemm_group: too many tiles");
  for (int k = 0; k < g.n; ++k) {
    if (gp.big && ((gp.swap >> k) & 1)) {  // C^T = B^T A: the narrow operand takes the tile's rows
      icap_gemm_args& p = g.a[k];
      std::swap(p.A, p.B);
      std::swap(p.lda, p.ldb);
      std::swap(p.M, p.N);
    }
    g.tiles_n[k] = gp.tiles_n[k];
    g.tstart[k + 1] = g.tstart[k] + gp.tiles_m[k] * gp.tiles_n[k];
  }
  g.swap = gp.big ? gp.swap : 0u;
  launch_group_kout(g, cus, gp.big, reinterpret_cast<hipStream_t>(stream));
  return check_launch("icap_gemm_group");
}

extern "C" int icap_gemm(const icap_gemm_args* a, void* stream) {
  ICAP_REQUIRE(a != nullptr, "icap_gemm: null args");
  if (a->M == 0 || a->N == 0) return ICAP_OK;
  GemmPlan pl;
  const int prc = gemm_plan(*a, pl, device_cus(), plan_diag());
  if (prc != ICAP_OK) return prc;
  // the kernels take the in-launch combine exactly when tickets reach them: only for the plan that chose it (a
  // reduce-pass split must write its slabs, whatever the caller passed)
  icap_gemm_args pk = *a;
  if (!pl.fused) pk.tickets = nullptr;
  const icap_gemm_args& p = pk;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t thr = pl.thr;
  const float inv_keep = pl.inv_keep;
  if (pl.skinny) {
    const dim3 sgrid(pl.grid_x, pl.grid_y), sblock(pl.block_x);
#define ICAP_SK(TI, TC, NT, U) hipLaunchKernelGGL((gemm_skinny_kernel<TI, TC, NT, 2, U>), sgrid, sblock, 0, s, p, thr, inv_keep)
#define ICAP_SKINNY_BF(TC)                                                                 \
  switch (pl.nt * 100 + pl.sku) {                                                          \
    case 103: ICAP_SK(bf16_t, TC, 1, 3); break;                                            \
    case 104: ICAP_SK(bf16_t, TC, 1, 4); break;                                            \
    case 106: ICAP_SK(bf16_t, TC, 1, 6); break;                                            \
    case 112: ICAP_SK(bf16_t, TC, 1, 12); break;                                           \
    case 203: ICAP_SK(bf16_t, TC, 2, 3); break;                                            \
    case 204: ICAP_SK(bf16_t, TC, 2, 4); break;                                            \
    case 206: ICAP_SK(bf16_t, TC, 2, 6); break;                                            \
    case 303: ICAP_SK(bf16_t, TC, 3, 3); break;                                            \
    case 304: ICAP_SK(bf16_t, TC, 3, 4); break;                                            \
    case 306: ICAP_SK(bf16_t, TC, 3, 6); break;                                            \
    case 403: ICAP_SK(bf16_t, TC, 4, 3); break;                                            \
    case 404: ICAP_SK(bf16_t, TC, 4, 4); break;                                            \
    default: ICAP_SK(bf16_t, TC, 4, 6); break;                                             \
  }
#define ICAP_SKINNY_F32(TC)                                                                \
  switch (pl.nt) {                                                                         \
    case 1: ICAP_SK(float, TC, 1, 6); break;                                               \
    case 2: ICAP_SK(float, TC, 2, 6); break;                                               \
    case 3: ICAP_SK(float, TC, 3, 6); break;                                               \
    default: ICAP_SK(float, TC, 4, 6); break;                                              \
  }
    if (p.in_dtype == ICAP_BF16) {
      if (p.c_dtype == ICAP_BF16) { ICAP_SKINNY_BF(bf16_t) } else { ICAP_SKINNY_BF(float) }
    } else {
      if (p.c_dtype == ICAP_BF16) { ICAP_SKINNY_F32(bf16_t) } else { ICAP_SKINNY_F32(float) }
    }
#undef ICAP_SKINNY_BF
#undef ICAP_SKINNY_F32
#undef ICAP_SK
    return check_launch("icap_gemm(skinny)");
  }
  if (pl.g256) return gemm256_launch(p, thr, inv_keep, s);
  if (pl.g8p) return gemm8p_launch(pl, p, s);
  const int sp = pl.splits;
  const int skew = gemm_plan_skew(p, pl, plan_diag());
  const int nks = pl.nk_split | (skew << 20) | (gemm_diag() << 28) | (gemm_acquire() << 30);
  const dim3 rgrid((unsigned)((p.M * (p.N / 4) + 255) / 256));
  const TileLauncher launch = tile_launcher(pl, p);
  if (launch == nullptr) return gemm_no_instantiation(pl);
  if (const int rc = launch(pl, p, nks, s); rc != ICAP_OK) return rc;
  if (sp > 1 && !pl.fused) {
    if (p.c_dtype == ICAP_BF16)
      hipLaunchKernelGGL((gemm_splitk_reduce<bf16_t>), rgrid, dim3(256), 0, s, p, sp, thr, inv_keep);
    else
      hipLaunchKernelGGL((gemm_splitk_reduce<float>), rgrid, dim3(256), 0, s, p, sp, thr, inv_keep);
  }
  return check_launch("icap_gemm");
}
