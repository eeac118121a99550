// CLIP text tower glue (HF/models/clip/modeling_clip.py CLIPTextEmbeddings :221-256, the pooled position :561-582):
// the token + position sum with the pooled row of every caption, and the gather of those rows. Both run on the
// padded [B, L] grid: every extent is a host value, and no address is formed from an id or a row index that was not
// range-checked first.
#include "common.h"

namespace icap {

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

// One block per caption. Wave 0 finds the pooled position (lane t, t + 64, ...: a (value, position) pair per lane,
// the larger value and on ties the smaller position winning, so the result is the first maximum); all four waves
// write the caption's L rows of x, four columns per thread.
template <typename T>
__global__ __launch_bounds__(256) void clip_text_embed_kernel(int L, int D, int64_t vocab,
                                                              const int64_t* __restrict__ ids,
                                                              const float* __restrict__ tok,
                                                              const float* __restrict__ pos, int64_t eos,
                                                              T* __restrict__ x, int32_t* __restrict__ pooled_row,
                                                              int32_t* __restrict__ oov) {
  const int b = blockIdx.x;
  const int64_t* row = ids + (int64_t)b * L;
  if (threadIdx.x < 64) {
    // legacy (eos == 2): the value is the id as HF's .to(torch.int) sees it; otherwise 1 where the id is eos, so
    // the first maximum is the first eos and position 0 when there is none
    int best_v = INT32_MIN, best_t = 0x7fffffff;
    for (int t = threadIdx.x; t < L; t += 64) {
      const int v = eos == 2 ? (int)(int32_t)row[t] : (int)(row[t] == eos);
      // (t ascends within a lane: a later equal value never replaces an earlier one)
      if (v > best_v || best_t == 0x7fffffff) {
        best_v = v;
        best_t = t;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int ov = __shfl_xor(best_v, o, 64), ot = __shfl_xor(best_t, o, 64);
      if (ov > best_v || (ov == best_v && ot < best_t)) {
        best_v = ov;
        best_t = ot;
      }
    }
    if (threadIdx.x == 0) pooled_row[b] = b * L + best_t;
  }
  const int D4 = D >> 2;
  const int total = L * D4;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int t = i / D4;
    const int c = (i - t * D4) * 4;
    const int64_t id = row[t];
    const bool ok = (uint64_t)id < (uint64_t)vocab;  // (negative ids wrap above vocab)
    float v[4] = {0.f, 0.f, 0.f, 0.f}, w[4];
    if (ok) io<float>::ld4(tok + id * D + c, v);
    else if (c == 0) atomicAdd(oov, 1);  // once per token
    io<float>::ld4(pos + (int64_t)t * D + c, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += w[e];
    io<T>::st4(x + ((int64_t)b * L + t) * D + c, v);
  }
}

// dst_s[r] = src_s[rows[r]] for s < 2 (src1 == nullptr: one source); a row index outside [0, n_src) reads nothing
// and stores a zero row
template <typename T>
__global__ void rows_gather_kernel(int R, int D, int64_t n_src, const int32_t* __restrict__ rows,
                                   const T* __restrict__ src0, int64_t lds0, T* __restrict__ dst0, int64_t ldd0,
                                   const T* __restrict__ src1, int64_t lds1, T* __restrict__ dst1, int64_t ldd1) {
  const int D4 = D >> 2;
  const int64_t per = (int64_t)R * D4, total = src1 ? 2 * per : per;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const bool second = i >= per;
    const int64_t j = second ? i - per : i;
    const int r = (int)(j / D4);
    const int c = (int)(j - (int64_t)r * D4) * 4;
    const int64_t s = rows[r];
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const T* src = second ? src1 : src0;
    if (s >= 0 && s < n_src) io<T>::ld4(src + s * (second ? lds1 : lds0) + c, v);
    io<T>::st4((second ? dst1 : dst0) + (int64_t)r * (second ? ldd1 : ldd0) + c, v);
  }
}

}  // namespace icap

using namespace icap;

extern "C" int icap_clip_text_embed(int32_t dtype, int32_t B, int32_t L, int32_t D, int64_t vocab, int32_t npos,
                                    const int64_t* ids, const float* tok, const float* pos, int64_t eos_token_id,
                                    void* x, int32_t* pooled_row, int32_t* oov_count, void* stream) {
  ICAP_REQUIRE(dtype == ICAP_F32 || dtype == ICAP_BF16, "icap_clip_text_embed: bad dtype");
  ICAP_REQUIRE(B >= 0 && L >= 1 && D > 0 && D % 4 == 0 && vocab > 0, "icap_clip_text_embed: bad geometry (D % 4 == 0)");
  ICAP_REQUIRE(L <= npos, "icap_clip_text_embed: L exceeds the position table");
  ICAP_REQUIRE((int64_t)B * L < (1ll << 31) && (int64_t)L * (D / 4) < (1ll << 31), "icap_clip_text_embed: too many rows");
  ICAP_REQUIRE(ids && tok && pos && x && pooled_row && oov_count, "icap_clip_text_embed: null pointer");
  if (B == 0) return ICAP_OK;
  if (dtype == ICAP_BF16)
    hipLaunchKernelGGL(clip_text_embed_kernel<bf16_t>, dim3((unsigned)B), dim3(256), 0, S_(stream), L, D, vocab, ids,
                       tok, pos, eos_token_id, reinterpret_cast<bf16_t*>(x), pooled_row, oov_count);
  else
    hipLaunchKernelGGL(clip_text_embed_kernel<float>, dim3((unsigned)B), dim3(256), 0, S_(stream), L, D, vocab, ids,
                       tok, pos, eos_token_id, reinterpret_cast<float*>(x), pooled_row, oov_count);
  return check_launch("icap_clip_text_embed");
}

extern "C" int icap_rows_gather(int32_t dtype, int32_t R, int32_t D, int64_t n_src, const int32_t* rows,
                                const void* src0, int64_t lds0, void* dst0, int64_t ldd0, const void* src1,
                                int64_t lds1, void* dst1, int64_t ldd1, void* stream) {
  ICAP_REQUIRE(dtype == ICAP_F32 || dtype == ICAP_BF16, "icap_rows_gather: bad dtype");
  ICAP_REQUIRE(R >= 0 && D > 0 && D % 4 == 0 && n_src >= 0, "icap_rows_gather: bad geometry (D % 4 == 0)");
  ICAP_REQUIRE(rows && src0 && dst0 && (src1 == nullptr) == (dst1 == nullptr), "icap_rows_gather: null pointer");
  ICAP_REQUIRE(lds0 >= D && ldd0 >= D && lds0 % 4 == 0 && ldd0 % 4 == 0, "icap_rows_gather: row strides must be >= D, multiples of 4");
  ICAP_REQUIRE(!src1 || (lds1 >= D && ldd1 >= D && lds1 % 4 == 0 && ldd1 % 4 == 0), "icap_rows_gather: row strides must be >= D, multiples of 4");
  if (R == 0) return ICAP_OK;
  const int64_t n = (int64_t)R * (D / 4) * (src1 ? 2 : 1);
  int64_t nb = (n + 255) / 256;
  if (nb > 4096) nb = 4096;
  if (dtype == ICAP_BF16)
    hipLaunchKernelGGL(rows_gather_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, S_(stream), R, D, n_src, rows,
                       (const bf16_t*)src0, lds0, (bf16_t*)dst0, ldd0, (const bf16_t*)src1, lds1, (bf16_t*)dst1, ldd1);
  else
    hipLaunchKernelGGL(rows_gather_kernel<float>, dim3((unsigned)nb), dim3(256), 0, S_(stream), R, D, n_src, rows,
                       (const float*)src0, lds0, (float*)dst0, ldd0, (const float*)src1, lds1, (float*)dst1, ldd1);
  return check_launch("icap_rows_gather");
}
