// Teacher-forced caption scoring (icap_caption_score, icap_caption_target_ranges): per-caption negative log
// likelihood, target count and correct-token count from the LM-head logits, running totals on the device.
//
// Two launches. The row pass is cross entropy's (csrc/elementwise.hip ce_bf16_reg_kernel / ce_kernel) without the
// dlogits half, with the row's argmax carried beside the online (max, sum-exp): one block per row, one HBM read of
// the row. The tail is ONE block: a wave per sequence adds its rows' fp32 values in row order in double, then one
// wave adds the batch to the running totals in sequence order. No atomics: every output has one writer and every
// sum a fixed order, so two runs (and an eager call and a graph replay) give the same bits.
#include "common.h"

#include <math.h>

namespace icap {

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

// torch.argmax's order (greedy_next_kernel's argmax_better): NaN beats everything, ties (and NaN vs NaN) go to
// the lower index — "higher value, then lower index" with NaN as the highest value
__device__ __forceinline__ bool score_better(float v, int j, float best, int bi) {
  if (v != v) return best == best || j < bi;
  if (best != best) return false;
  return v > best || (v == best && j < bi);
}

// A thread visits its logits in increasing index order, so it keeps its FIRST maximum with a strict compare: take v
// when it is higher, or when it is the thread's first NaN.
#define SCORE_TAKE(v, j)                                  \
  do {                                                    \
    if ((v) > best || ((v) != (v) && best == best)) {     \
      best = (v);                                         \
      bi = (j);                                           \
    }                                                     \
  } while (0)

constexpr int SCORE_NONE = 0x7fffffff;  // index of a thread that holds no logit: loses every tie

// Block combine of the per-thread (max, sum-exp) and (max, first index); thread 0 stores the row's nll and hit.
// lse takes the argmax's value where the sum cannot say it: NaN anywhere in the row -> NaN, a +inf logit -> +inf,
// every logit -inf -> -inf (torch.logsumexp's values).
template <int NW>
__device__ __forceinline__ void score_finish(float m, float s, float best, int bi, float xy, int y, float* redm,
                                             float* reds, float* rv, int* ri, float* nll_row, int32_t* hit_row) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float bm = wave_max(m);
  s = (m == -INFINITY) ? 0.f : s * __expf(m - bm);
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (score_better(ov, oi, best, bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { redm[w] = bm; reds[w] = s; rv[w] = best; ri[w] = bi; }
  __syncthreads();
  if (tid == 0) {
    float M = redm[0], bv = rv[0];
    int bj = ri[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) {
      M = fmaxf(M, redm[k]);
      if (score_better(rv[k], ri[k], bv, bj)) { bv = rv[k]; bj = ri[k]; }
    }
    float Ssum = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) Ssum += (redm[k] == -INFINITY) ? 0.f : reds[k] * __expf(redm[k] - M);
    float lse = M + logf(Ssum);
    if (bv != bv || bv == INFINITY || bv == -INFINITY) lse = bv;
    *nll_row = lse - xy;
    *hit_row = bj == y ? 1 : 0;
  }
}

// bf16 logits, V <= 8 * 512 * R: the row is read from HBM once into registers (R 16-byte groups per thread, all in
// flight together), as ce_bf16_reg_kernel does; nothing is written but the row's two results.
template <int R>
__global__ __launch_bounds__(512) void score_bf16_reg_kernel(int64_t V, const bf16_t* __restrict__ logits, int64_t ld,
                                                            const int32_t* __restrict__ labels,
                                                            const int32_t* __restrict__ rows_dev,
                                                            float* __restrict__ nll_rows,
                                                            int32_t* __restrict__ hit_rows) {
  constexpr int NT = 512, NW = NT / 64;
  __shared__ float redm[NW], reds[NW], rv[NW];
  __shared__ int ri[NW];
  const int64_t r = blockIdx.x;
  if (rows_dev && r >= *rows_dev) return;
  const int y = labels[r];
  const int tid = threadIdx.x;
  if (y < 0 || y >= V) {  // ignored row (-100); a label past the vocabulary is counted and scores NaN
    if (tid == 0) { nll_rows[r] = y < 0 ? 0.f : __uint_as_float(0x7fc00000u); hit_rows[r] = 0; }
    return;
  }
  const bf16_t* x = logits + r * ld;
  const int64_t V8 = V >> 3;
  uint4 wv[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int64_t g = tid + (int64_t)i * NT;
    wv[i] = g < V8 ? *reinterpret_cast<const uint4*>(x + 8 * g) : make_uint4(0xff80ff80u, 0xff80ff80u, 0xff80ff80u,
                                                                                  0xff80ff80u);  // -inf padding
  }
  float m = -INFINITY, s = 0.f, best = -INFINITY;
  int bi = tid < V8 ? 8 * tid : SCORE_NONE;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    float v[8];
    const uint32_t h[4] = {wv[i].x, wv[i].y, wv[i].z, wv[i].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[2 * e] = __uint_as_float(h[e] << 16);
      v[2 * e + 1] = __uint_as_float(h[e] & 0xffff0000u);
    }
    const int jb = 8 * (tid + i * NT);  // -inf padding groups never pass the strict compare
    float mx = v[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) mx = fmaxf(mx, v[e]);
#pragma unroll
    for (int e = 0; e < 8; ++e) SCORE_TAKE(v[e], jb + e);
    if (mx > m) { s *= __expf(m - mx); m = mx; }
    if (m != -INFINITY) {
#pragma unroll
      for (int e = 0; e < 8; ++e) s += __expf(v[e] - m);
    }
  }
  for (int64_t j = 8 * V8 + tid; j < V; j += NT) {  // the last V % 8 logits
    const float v = bf2f(x[j]);
    if (score_better(v, (int)j, best, bi)) { best = v; bi = (int)j; }
    if (v > m) { s *= __expf(m - v); m = v; }
    if (m != -INFINITY) s += __expf(v - m);
  }
  float xy = 0.f;
  if (tid == 0) xy = bf2f(x[y]);
  score_finish<NW>(m, s, best, bi, xy, y, redm, reds, rv, ri, nll_rows + r, hit_rows + r);
}

// Any V, fp32 or bf16: 4-wide loads streamed through the same online update (one read of the row as well: without
// dlogits there is no second pass; what the register form adds is every load of the row in flight at once).
template <typename T>
__global__ __launch_bounds__(256) void score_rows_kernel(int64_t V, const T* __restrict__ logits, int64_t ld,
                                                        const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ rows_dev,
                                                        float* __restrict__ nll_rows, int32_t* __restrict__ hit_rows) {
  constexpr int NT = 256, NW = NT / 64;
  __shared__ float redm[NW], reds[NW], rv[NW];
  __shared__ int ri[NW];
  const int64_t r = blockIdx.x;
  if (rows_dev && r >= *rows_dev) return;
  const int y = labels[r];
  const int tid = threadIdx.x;
  if (y < 0 || y >= V) {
    if (tid == 0) { nll_rows[r] = y < 0 ? 0.f : __uint_as_float(0x7fc00000u); hit_rows[r] = 0; }
    return;
  }
  const T* x = logits + r * ld;
  const int64_t V4 = V >> 2;
  float m = -INFINITY, s = 0.f, best = -INFINITY;
  int bi = tid < V4 ? 4 * tid : SCORE_NONE;
#pragma unroll 4
  for (int64_t g = tid; g < V4; g += NT) {
    float v[4];
    io<T>::ld4(x + 4 * g, v);
    const int jb = (int)(4 * g);
    const float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
    for (int e = 0; e < 4; ++e) SCORE_TAKE(v[e], jb + e);
    if (mx > m) { s *= __expf(m - mx); m = mx; }
    if (m != -INFINITY) s += __expf(v[0] - m) + __expf(v[1] - m) + __expf(v[2] - m) + __expf(v[3] - m);
  }
  for (int64_t j = 4 * V4 + tid; j < V; j += NT) {
    const float v = io<T>::ld(x + j);
    if (score_better(v, (int)j, best, bi)) { best = v; bi = (int)j; }
    if (v > m) { s *= __expf(m - v); m = v; }
    if (m != -INFINITY) s += __expf(v - m);
  }
  float xy = 0.f;
  if (tid == 0) xy = io<T>::ld(x + y);
  score_finish<NW>(m, s, best, bi, xy, y, redm, reds, rv, ri, nll_rows + r, hit_rows + r);
}

// double from lane k of the wave
__device__ __forceinline__ double shfl_f64(double v, int k) {
  const uint64_t u = __double_as_longlong(v);
  const uint32_t lo = __shfl((int)(uint32_t)u, k, 64), hi = __shfl((int)(uint32_t)(u >> 32), k, 64);
  return __longlong_as_double(((uint64_t)hi << 32) | lo);
}

// The tail: one 1024-thread block. Wave w takes sequences w, w + 16, ...: lanes load 64 rows of the sequence's range
// at a time, the counts are ballots, the nll is added lane by lane (row order) in double by every lane alike and
// rounded once. Then token_logprobs, element per thread. Then wave 0 adds the batch's fp32 nll (as double) and
// counts to totals in sequence order, after a barrier (a block sees its own global stores past a barrier).
__global__ __launch_bounds__(1024) void score_tail_kernel(int64_t rows, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ rows_dev, int B,
                                                         const int32_t* __restrict__ ranges,
                                                         const float* __restrict__ nll_rows,
                                                         const int32_t* __restrict__ hit_rows, float* nll,
                                                         int32_t* n_tokens, int32_t* n_correct, float* token_logprobs,
                                                         int P, int Lc, const int32_t* __restrict__ row_slot,
                                                         const int32_t* __restrict__ seq_off,
                                                         const int32_t* __restrict__ seq_len, double* totals) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int64_t lim = rows;
  if (rows_dev && *rows_dev < lim) lim = *rows_dev;
  if (lim < 0) lim = 0;
  for (int b = w; b < B; b += 16) {
    int64_t r0 = ranges[b], r1 = ranges[b + 1];
    if (r0 < 0) r0 = 0;
    if (r1 > lim) r1 = lim;
    double acc = 0.0;
    int ntok = 0, nhit = 0;
    for (int64_t c = r0; c < r1; c += 64) {
      const int64_t r = c + lane;
      const bool live = r < r1 && labels[r] >= 0;
      const double v = live ? (double)nll_rows[r] : 0.0;
      const bool hit = live && hit_rows[r] != 0;
      ntok += __popcll(__ballot(live));
      nhit += __popcll(__ballot(hit));
      const int n = r1 - c < 64 ? (int)(r1 - c) : 64;
      for (int k = 0; k < n; ++k) acc += shfl_f64(v, k);
    }
    if (lane == 0) {
      nll[b] = (float)acc;
      n_tokens[b] = ntok;
      n_correct[b] = nhit;
    }
  }
  if (token_logprobs) {
    const int S = P + Lc;
    for (int i = tid; i < B * Lc; i += 1024) {
      const int b = i / Lc, t = i - b * Lc;
      const int sp = P + t - 1;  // the position that predicts caption token t
      int64_t g = -1;
      if (sp >= 0) {
        if (seq_off) g = sp < seq_len[b] ? (int64_t)seq_off[b] + sp : -1;
        else g = (int64_t)b * S + sp;
      }
      int64_t slot = g;
      if (g >= 0 && row_slot) slot = row_slot[g];
      float v = 0.f;
      if (slot >= 0 && slot < lim && labels[slot] >= 0) v = -nll_rows[slot];
      token_logprobs[i] = v;
    }
  }
  if (totals) {
    __syncthreads();
    if (w == 0) {
      double a0 = totals[0], a1 = totals[1], a2 = totals[2];
      for (int c = 0; c < B; c += 64) {
        const int b = c + lane;
        const double v = b < B ? (double)nll[b] : 0.0;
        const double t = b < B ? (double)n_tokens[b] : 0.0;
        const double h = b < B ? (double)n_correct[b] : 0.0;
        const int n = B - c < 64 ? B - c : 64;
        for (int k = 0; k < n; ++k) {
          a0 += shfl_f64(v, k);
          a1 += shfl_f64(t, k);
          a2 += shfl_f64(h, k);
        }
      }
      if (lane == 0) { totals[0] = a0; totals[1] = a1; totals[2] = a2; }
    }
  }
}

// ranges[b] = number of target rows (row_slot >= 0) before sequence b's rows; a wave counts one sequence's rows
// (ballots), wave 0 then scans the counts in place. Without row_slot every row is its own slot: ranges[b] = b S.
__global__ __launch_bounds__(1024) void target_ranges_kernel(int B, int S, const int32_t* __restrict__ row_slot,
                                                            const int32_t* __restrict__ seq_off,
                                                            const int32_t* __restrict__ seq_len, int32_t* ranges) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (!row_slot) {
    for (int b = tid; b <= B; b += 1024) ranges[b] = b * S;
    return;
  }
  for (int b = w; b < B; b += 16) {
    const int g0 = seq_off ? seq_off[b] : b * S;
    int n = seq_off ? seq_len[b] : S;
    if (n > S) n = S;  // a sequence holds at most S rows
    if (g0 < 0 || (int64_t)g0 + n > (int64_t)B * S) n = 0;  // never past the [B S] row arrays
    int cnt = 0;
    for (int c = 0; c < n; c += 64) cnt += __popcll(__ballot(c + lane < n && row_slot[g0 + c + lane] >= 0));
    if (lane == 0) ranges[b + 1] = cnt;
  }
  __syncthreads();
  if (w == 0) {
    int run = 0;
    if (lane == 0) ranges[0] = 0;
    for (int c = 0; c < B; c += 64) {
      const int b = c + lane;
      int incl = b < B ? ranges[b + 1] : 0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      if (b < B) ranges[b + 1] = run + incl;
      run += __shfl(incl, 63, 64);
    }
  }
}

}  // namespace icap

using namespace icap;

extern "C" size_t icap_caption_score_workspace_bytes(int64_t rows) {
  return (size_t)(rows > 0 ? rows : 1) * (sizeof(float) + sizeof(int32_t));
}

extern "C" int icap_caption_score(int32_t dtype, int64_t rows, int64_t V, const void* logits, int64_t ld,
                                  const int32_t* labels, const int32_t* rows_dev, int32_t B, const int32_t* ranges,
                                  float* nll, int32_t* n_tokens, int32_t* n_correct, float* token_logprobs,
                                  int32_t P, int32_t Lc, const int32_t* row_slot, const int32_t* seq_off,
                                  const int32_t* seq_len, double* totals, void* workspace, void* stream) {
  ICAP_REQUIRE(logits && labels && ranges && nll && n_tokens && n_correct && workspace,
               "icap_caption_score: null pointer");
  ICAP_REQUIRE(dtype == ICAP_BF16 || dtype == ICAP_F32, "icap_caption_score: bad dtype");
  ICAP_REQUIRE(V > 0 && V < (1ll << 31) && ld >= V && ld % 4 == 0,
               "icap_caption_score: ld must be >= V and a multiple of 4");
  ICAP_REQUIRE(rows >= 0 && rows < (1ll << 31) && B >= 1, "icap_caption_score: bad geometry");
  ICAP_REQUIRE((seq_off == nullptr) == (seq_len == nullptr), "icap_caption_score: seq_off and seq_len go together");
  ICAP_REQUIRE(token_logprobs == nullptr || (P >= 0 && Lc >= 0 && (int64_t)B * (P + Lc) < (1ll << 30)),
               "icap_caption_score: token_logprobs needs P, Lc >= 0");
  ICAP_REQUIRE(token_logprobs == nullptr || seq_off == nullptr || row_slot != nullptr,
               "icap_caption_score: packed rows need row_slot");
  const uintptr_t addr = reinterpret_cast<uintptr_t>(logits);
  ICAP_REQUIRE((addr & (dtype == ICAP_BF16 ? 7 : 15)) == 0, "icap_caption_score: logits must be aligned to 4 elements");
  float* nrows = reinterpret_cast<float*>(workspace);
  int32_t* hrows = reinterpret_cast<int32_t*>(nrows + (rows > 0 ? rows : 1));
  if (rows > 0) {
    const bool reg = dtype == ICAP_BF16 && V <= 8 * 512 * 13 && ld % 8 == 0 && (addr & 15) == 0;
    if (reg) {
      hipLaunchKernelGGL(score_bf16_reg_kernel<13>, dim3((unsigned)rows), dim3(512), 0, S_(stream), V,
                         reinterpret_cast<const bf16_t*>(logits), ld, labels, rows_dev, nrows, hrows);
    } else if (dtype == ICAP_BF16) {
      hipLaunchKernelGGL(score_rows_kernel<bf16_t>, dim3((unsigned)rows), dim3(256), 0, S_(stream), V,
                         reinterpret_cast<const bf16_t*>(logits), ld, labels, rows_dev, nrows, hrows);
    } else {
      hipLaunchKernelGGL(score_rows_kernel<float>, dim3((unsigned)rows), dim3(256), 0, S_(stream), V,
                         reinterpret_cast<const float*>(logits), ld, labels, rows_dev, nrows, hrows);
    }
    const int rc = check_launch("icap_caption_score");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(score_tail_kernel, dim3(1), dim3(1024), 0, S_(stream), rows, labels, rows_dev, B, ranges, nrows,
                     hrows, nll, n_tokens, n_correct, token_logprobs, P, Lc, row_slot, seq_off, seq_len, totals);
  return check_launch("icap_caption_score(tail)");
}

extern "C" int icap_caption_target_ranges(int32_t B, int32_t S, const int32_t* row_slot, const int32_t* seq_off,
                                          const int32_t* seq_len, int32_t* ranges, void* stream) {
  ICAP_REQUIRE(ranges, "icap_caption_target_ranges: null pointer");
  ICAP_REQUIRE(B >= 1 && S >= 0 && (int64_t)B * S < (1ll << 30), "icap_caption_target_ranges: bad geometry");
  ICAP_REQUIRE((seq_off == nullptr) == (seq_len == nullptr),
               "icap_caption_target_ranges: seq_off and seq_len go together");
  ICAP_REQUIRE(seq_off == nullptr || row_slot != nullptr, "icap_caption_target_ranges: packed rows need row_slot");
  hipLaunchKernelGGL(target_ranges_kernel, dim3(1), dim3(1024), 0, S_(stream), B, S, row_slot, seq_off, seq_len,
                     ranges);
  return check_launch("icap_caption_target_ranges");
}
