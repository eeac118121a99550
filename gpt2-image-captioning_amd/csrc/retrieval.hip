// Retrieval for the retrieval-augmented captioner (reference: src/models.py:550-785 RetrievalAggregator /
// RetrievalAugmentedTransformer over src/database/faiss_store.py). The reference searches a FAISS index on the host
// in every forward; here the database stays on the device and one forward is three launches after the score GEMM
// S = Q . X^T (icap_gemm, exact-fp32 chain):
//   topk_slice_kernel   grid (rows x column slices of SLICE columns): the K best of each slice (descending, ties ->
//                       lower column) into the workspace. One block per row would leave half the CUs idle at
//                       R = 128 and give each block the whole 473 KB row to walk.
//   topk_merge_kernel   one block per row: the K best of the row's slice lists (and, with `merge`, of the lists
//                       already in top_val / top_idx: a caller that scores the database in column chunks folds
//                       each chunk into the running lists).
//   retrieval_aggregate_kernel  one block per query: the reference's candidate walk (faiss_store.py:163-181,
//                       208-229) on one lane, then the caption-row gather, the aggregation (models.py:589-606) and
//                       query + aggregated (models.py:623) on the whole block.
// The order is beam::better's (beam.hip): higher value first, then lower index; a top-K under a total order is
// unique, so the chunked and the one-call forms give bitwise the same lists.
#include "common.h"

namespace icap {
namespace retr {
constexpr int NT = 256;
constexpr int EPT = 16;            // columns per thread of one slice
constexpr int SLICE = NT * EPT;    // 4096 columns per block
constexpr int KMAX = 32;           // top_i + 10 <= 32 (faiss_store.py:153 searches top_i + 10)
constexpr int TOPK_MAX = 64;       // caption rows per query
constexpr int32_t NONE = 0x7fffffff;  // index of an empty list entry (value -inf): loses to every real entry

// candidate order of beam.hip: higher score first, then lower key
__device__ __forceinline__ bool better(float a, int32_t ka, float b, int32_t kb) {
  return a > b || (a == b && ka < kb);
}

// insertion into a sorted register list (compile-time indices), as beam_rowtop_kernel's
template <int LEN>
__device__ __forceinline__ void insert(float (&v)[LEN], int32_t (&id)[LEN], float cv, int32_t ci) {
  if (!better(cv, ci, v[LEN - 1], id[LEN - 1])) return;
#pragma unroll
  for (int k = 0; k < LEN; ++k) {
    if (better(cv, ci, v[k], id[k])) {
      const float tv = v[k]; const int32_t ti = id[k];
      v[k] = cv; id[k] = ci; cv = tv; ci = ti;
    }
  }
}

// The K best over every thread's sorted list, in order: K rounds of a block-wide best over the list heads.
// Real indices are unique, so exactly one thread owns each winner; once only empty entries are left every round
// writes (-inf, NONE).
template <int LEN>
__device__ __forceinline__ void block_select(const float (&v)[LEN], const int32_t (&id)[LEN], int K,
                                             float* __restrict__ out_val, int32_t* __restrict__ out_idx,
                                             bool final_form) {
  __shared__ float sv[NT / 64];
  __shared__ int32_t si[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int head = 0;
  for (int k = 0; k < K; ++k) {
    float hv = -INFINITY;
    int32_t hi = NONE;
#pragma unroll
    for (int q = 0; q < LEN; ++q)
      if (q == head) { hv = v[q]; hi = id[q]; }
    float bv = hv;
    int32_t bi = hi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int32_t oi = __shfl_xor(bi, o, 64);
      if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();  // the previous round's readers are done with sv / si
    if (lane == 0) { sv[w] = bv; si[w] = bi; }
    __syncthreads();
    float wv = sv[0];
    int32_t wi = si[0];
#pragma unroll
    for (int q = 1; q < NT / 64; ++q)
      if (better(sv[q], si[q], wv, wi)) { wv = sv[q]; wi = si[q]; }
    if (wi != NONE && hi == wi) ++head;
    if (tid == 0) {
      out_val[k] = wv;
      out_idx[k] = (final_form && wi == NONE) ? -1 : wi;  // FAISS pads a short result with index -1
    }
  }
}

__global__ __launch_bounds__(256) void topk_slice_kernel(int64_t N, int64_t nsl, const float* __restrict__ scores,
                                                         int64_t ld, int K, int32_t col0,
                                                         float* __restrict__ ws_val, int32_t* __restrict__ ws_idx) {
  const int64_t r = blockIdx.x / nsl, s = blockIdx.x - r * nsl;
  const float* row = scores + r * ld;
  float v[EPT];
  int32_t id[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) { v[k] = -INFINITY; id[k] = NONE; }
  const int64_t j0 = s * SLICE, j1 = j0 + SLICE < N ? j0 + SLICE : N;
  // coalesced: consecutive lanes read consecutive columns; a thread sees at most EPT columns, so its list keeps all
  for (int64_t j = j0 + threadIdx.x; j < j1; j += NT) insert<EPT>(v, id, row[j], (int32_t)(col0 + j));
  const int64_t o = (r * nsl + s) * K;
  block_select<EPT>(v, id, K, ws_val + o, ws_idx + o, false);
}

__global__ __launch_bounds__(256) void topk_merge_kernel(int64_t nsl, int K, int merge,
                                                         const float* __restrict__ ws_val,
                                                         const int32_t* __restrict__ ws_idx,
                                                         float* __restrict__ top_val, int32_t* __restrict__ top_idx) {
  const int64_t r = blockIdx.x;
  float v[KMAX];
  int32_t id[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { v[k] = -INFINITY; id[k] = NONE; }
  const int64_t n = nsl * K;
  for (int64_t e = threadIdx.x; e < n; e += NT) {
    const int32_t ci = ws_idx[r * n + e];
    if (ci != NONE) insert<KMAX>(v, id, ws_val[r * n + e], ci);
  }
  if (merge) {  // the running lists are candidates too (read here, overwritten only after the barriers below)
    for (int e = threadIdx.x; e < K; e += NT) {
      const int32_t ci = top_idx[r * K + e];
      if (ci >= 0) insert<KMAX>(v, id, top_val[r * K + e], ci);
    }
  }
  block_select<KMAX>(v, id, K, top_val + r * K, top_idx + r * K, true);
}

struct AggArgs {
  int32_t B, D, K, top_i, top_k, agg;
  int64_t N, C;
  const float* top_val; const int32_t* top_idx;
  const int32_t* cap_ptr; const int32_t* cap_rows;
  const float* cap_emb; const float* query; int64_t ldq;
  float* retrieved; int32_t* cap_ids; float* out; int64_t ldo;
};

__device__ __forceinline__ float block_sum(float x, float* red) {
  x = wave_sum(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < NT / 64; ++q) s += red[q];
  return s;
}

__global__ __launch_bounds__(256) void retrieval_aggregate_kernel(AggArgs a) {
  __shared__ int32_t sel[TOPK_MAX];
  __shared__ float inv_norm[TOPK_MAX];
  __shared__ float red[NT / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int top_k = a.top_k, D = a.D;
  if (tid == 0) {
    int kept = 0, n = 0;
    for (int k = 0; k < a.K && kept < a.top_i && n < top_k; ++k) {
      const int32_t img = a.top_idx[(int64_t)b * a.K + k];
      if (img < 0 || img >= a.N) continue;                                  // FAISS padding (faiss_store.py:165)
      if ((double)a.top_val[(int64_t)b * a.K + k] > 0.9999) continue;      // the query's own image (:170-175)
      ++kept;                                                               // top_i kept images (:180)
      // its caption rows, in order; the first top_k are used (:212-219, :229). The loop's n < top_k is the
      // reference's break after an image that fills the list.
      const int32_t p1 = a.cap_ptr[img + 1];
      for (int32_t p = a.cap_ptr[img]; p < p1 && n < top_k; ++p) {
        const int32_t c = a.cap_rows[p];
        if (c >= 0 && c < a.C) sel[n++] = c;
      }
    }
    for (; n < top_k; ++n) sel[n] = -1;  // zero padding (:221-246)
  }
  __syncthreads();
  if (a.cap_ids)
    for (int j = tid; j < top_k; j += NT) a.cap_ids[(int64_t)b * top_k + j] = sel[j];
  const int D4 = D >> 2;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.retrieved) {
    float4* dst = reinterpret_cast<float4*>(a.retrieved + (int64_t)b * top_k * D);
    for (int e = tid; e < top_k * D4; e += NT) {
      const int j = e / D4, d = e - j * D4;
      dst[e] = sel[j] >= 0 ? reinterpret_cast<const float4*>(a.cap_emb + (int64_t)sel[j] * D)[d] : zero4;
    }
  }
  if (!a.out) return;
  if (a.agg == ICAP_AGG_SUM_NORM) {
    // F.normalize(x, dim = -1): x / max(||x||, 1e-12); a zero row stays zero (models.py:600-602)
    const int lane = tid & 63;
    for (int j = tid >> 6; j < top_k; j += NT / 64) {
      float ss = 0.f;
      if (sel[j] >= 0) {
        const float4* src = reinterpret_cast<const float4*>(a.cap_emb + (int64_t)sel[j] * D);
        for (int d = lane; d < D4; d += 64) {
          const float4 x = src[d];
          ss += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) inv_norm[j] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    }
    __syncthreads();
  }
  // a thread owns column quads and walks the top_k rows, zero pads included, in order (models.py:589-606)
  float ss = 0.f;
  for (int d = tid; d < D4; d += NT) {
    float4 acc = zero4;
    for (int j = 0; j < top_k; ++j) {
      const float4 x = sel[j] >= 0 ? reinterpret_cast<const float4*>(a.cap_emb + (int64_t)sel[j] * D)[d] : zero4;
      if (a.agg == ICAP_AGG_MAX) {
        acc = j == 0 ? x : make_float4(fmaxf(acc.x, x.x), fmaxf(acc.y, x.y), fmaxf(acc.z, x.z), fmaxf(acc.w, x.w));
      } else {
        const float w = a.agg == ICAP_AGG_SUM_NORM ? inv_norm[j] : 1.f;
        acc.x += x.x * w; acc.y += x.y * w; acc.z += x.z * w; acc.w += x.w * w;
      }
    }
    if (a.agg == ICAP_AGG_MEAN) {
      const float n = (float)top_k;
      acc = make_float4(acc.x / n, acc.y / n, acc.z / n, acc.w / n);
    }
    if (a.agg == ICAP_AGG_SUM_NORM) {  // the sum is normalised below: park it in out
      ss += acc.x * acc.x + acc.y * acc.y + acc.z * acc.z + acc.w * acc.w;
      reinterpret_cast<float4*>(a.out + (int64_t)b * a.ldo)[d] = acc;
    } else {
      const float4 q = reinterpret_cast<const float4*>(a.query + (int64_t)b * a.ldq)[d];
      reinterpret_cast<float4*>(a.out + (int64_t)b * a.ldo)[d] =
          make_float4(q.x + acc.x, q.y + acc.y, q.z + acc.z, q.w + acc.w);
    }
  }
  if (a.agg == ICAP_AGG_SUM_NORM) {
    const float inv = 1.f / fmaxf(sqrtf(block_sum(ss, red)), 1e-12f);  // models.py:606
    for (int d = tid; d < D4; d += NT) {  // each thread re-reads the quads it wrote itself
      const float4 s = reinterpret_cast<float4*>(a.out + (int64_t)b * a.ldo)[d];
      const float4 q = reinterpret_cast<const float4*>(a.query + (int64_t)b * a.ldq)[d];
      reinterpret_cast<float4*>(a.out + (int64_t)b * a.ldo)[d] =
          make_float4(q.x + s.x * inv, q.y + s.y * inv, q.z + s.z * inv, q.w + s.w * inv);
    }
  }
}
}  // namespace retr
}  // namespace icap

using namespace icap;

static int64_t topk_slices(int64_t N) { return N <= 0 ? 1 : (N + retr::SLICE - 1) / retr::SLICE; }

extern "C" int32_t icap_topk_rows_slice(void) { return retr::SLICE; }

extern "C" size_t icap_topk_rows_workspace_bytes(int64_t R, int64_t N, int32_t K) {
  if (R < 0 || N < 0 || K < 1 || K > retr::KMAX) return 0;
  return (size_t)(R * topk_slices(N) * K) * 8;
}

extern "C" int icap_topk_rows(int64_t R, int64_t N, const float* scores, int64_t ld, int32_t K, int32_t col0,
                              int32_t merge, float* top_val, int32_t* top_idx, void* workspace, void* stream) {
  ICAP_REQUIRE(K >= 1 && K <= retr::KMAX, "icap_topk_rows: K must be in [1, 32]");
  ICAP_REQUIRE(R >= 0 && N >= 0 && ld >= N, "icap_topk_rows: bad R / N / ld");
  ICAP_REQUIRE(col0 >= 0 && (int64_t)col0 + N < (1ll << 31), "icap_topk_rows: col0 + N must be below 2^31");
  if (R == 0) return ICAP_OK;
  ICAP_REQUIRE((scores || N == 0) && top_val && top_idx && workspace, "icap_topk_rows: null pointer");
  const int64_t nsl = topk_slices(N);
  ICAP_REQUIRE(R * nsl < (1ll << 31), "icap_topk_rows: too many (row, slice) blocks");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* ws_val = reinterpret_cast<float*>(workspace);
  int32_t* ws_idx = reinterpret_cast<int32_t*>(workspace) + R * nsl * K;
  hipLaunchKernelGGL(retr::topk_slice_kernel, dim3((unsigned)(R * nsl)), dim3(retr::NT), 0, s, N, nsl, scores, ld,
                     (int)K, col0, ws_val, ws_idx);
  hipLaunchKernelGGL(retr::topk_merge_kernel, dim3((unsigned)R), dim3(retr::NT), 0, s, nsl, (int)K, (int)merge,
                     ws_val, ws_idx, top_val, top_idx);
  return check_launch("icap_topk_rows");
}

extern "C" int icap_retrieval_aggregate(int32_t B, int32_t D, int32_t K, int32_t top_i, int32_t top_k, int32_t agg,
                                        const float* top_val, const int32_t* top_idx, int64_t N,
                                        const int32_t* cap_ptr, const int32_t* cap_rows, int64_t C,
                                        const float* caption_embeddings, const float* query, int64_t ldq,
                                        float* retrieved, int32_t* cap_ids, float* out, int64_t ldo, void* stream) {
  ICAP_REQUIRE(B >= 0 && D >= 4 && D % 4 == 0, "icap_retrieval_aggregate: D must be a positive multiple of 4");
  ICAP_REQUIRE(top_i >= 1 && top_i <= 22, "icap_retrieval_aggregate: top_i must be in [1, 22]");
  ICAP_REQUIRE(top_k >= 1 && top_k <= retr::TOPK_MAX, "icap_retrieval_aggregate: top_k must be in [1, 64]");
  ICAP_REQUIRE(K >= 1 && K <= retr::KMAX, "icap_retrieval_aggregate: K must be in [1, 32]");
  ICAP_REQUIRE(agg == ICAP_AGG_MEAN || agg == ICAP_AGG_MAX || agg == ICAP_AGG_SUM_NORM,
               "icap_retrieval_aggregate: unknown aggregation");
  ICAP_REQUIRE(N >= 0 && N < (1ll << 31) && C >= 0 && C < (1ll << 31), "icap_retrieval_aggregate: N, C below 2^31");
  if (B == 0) return ICAP_OK;
  ICAP_REQUIRE(top_val && top_idx && cap_ptr && (cap_rows || C == 0) && (caption_embeddings || C == 0),
               "icap_retrieval_aggregate: null pointer");
  ICAP_REQUIRE(!out || (query && ldq >= D && ldo >= D && ldq % 4 == 0 && ldo % 4 == 0),
               "icap_retrieval_aggregate: out needs query, ldq / ldo >= D and multiples of 4");
  const uintptr_t al = reinterpret_cast<uintptr_t>(caption_embeddings) | reinterpret_cast<uintptr_t>(query) |
                       reinterpret_cast<uintptr_t>(retrieved) | reinterpret_cast<uintptr_t>(out);
  ICAP_REQUIRE((al & 15) == 0, "icap_retrieval_aggregate: float buffers must be 16-byte aligned");
  retr::AggArgs a{B, D, K, top_i, top_k, agg, N, C, top_val, top_idx, cap_ptr, cap_rows, caption_embeddings, query,
                  ldq, retrieved, cap_ids, out, ldo};
  hipLaunchKernelGGL(retr::retrieval_aggregate_kernel, dim3((unsigned)B), dim3(retr::NT), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return check_launch("icap_retrieval_aggregate");
}
