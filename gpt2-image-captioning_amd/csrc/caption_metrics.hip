// Caption metrics on the device (icap_caption_metrics): the exact integer and fp64 parts of corpus BLEU-1..4,
// ROUGE-L and CIDEr (pycocoevalcap's Bleu(4) / Rouge() / Cider(n = 4, sigma = 6) on raw strings) for one hypothesis
// and m >= 1 references per image. The host tokenises and finishes (icap/metrics.py); this file does the counting.
//
// Four launches on the caller's stream, no allocation, no synchronisation, no wait between workgroups:
//   clear   tables to EMPTY, document frequencies to 0
//   build   exact n-gram identity: the id of a k-gram is the slot its key (id of its (k-1)-gram prefix) << 32 | last
//           word holds in the open-addressing table of order k, claimed with ONE 64-bit atomicCAS (claim and publish
//           are the same store, so a reader sees EMPTY or the final key, never a half-written slot). A k-gram's chain
//           hangs on its own start position only, so one thread walks orders 2, 3, 4 of its position in turn.
//   df      df[order][id] += 1 once per (n-gram, image): one workgroup per image keeps an n-gram's first occurrence
//           among the image's reference positions (ids compared directly); integer atomics, order-independent
//   score   one workgroup per image: the hypothesis in LDS, references streamed one at a time. Thread (order, position)
//           counts by comparing ids. Emits stats [I][10], lcs per (image, reference) and cider fp64 [I]; every fp64
//           sum has a fixed shape (xor tree in a wave, then wave order), so two runs give the same bits.
// Every probe loop is bounded by the table's capacity; the host check capacity > positions makes a full table
// impossible, and a probe that still ends without a slot (a caller that understated positions) writes id -1 and
// raises the overflow flag instead of looping.
#include "common.h"

#include <math.h>

namespace icap {

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int MW = ICAP_METRIC_MAX_WORDS;
constexpr uint64_t EMPTY = ~0ull;  // no key: ids and words are below 2^31
static_assert(MW == 128, "the score kernel maps one thread to (order, position) and the LCS to two 64-bit words");

// the workspace carve-up, shared by the size query and the launcher (bytes from the start, 16-byte aligned parts)
struct metrics_ws {
  size_t table[3], df[3], df1, ids_ref, ids_hyp, total;
};
static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
static metrics_ws ws_layout(int64_t n_vocab, int64_t n_ref_words, int64_t n_hyp_words, const int64_t cap[3]) {
  metrics_ws w;
  size_t o = 0;
  for (int k = 0; k < 3; ++k) { w.table[k] = o; o += up16((size_t)cap[k] * 8); }
  for (int k = 0; k < 3; ++k) { w.df[k] = o; o += up16((size_t)cap[k] * 4); }
  w.df1 = o; o += up16((size_t)(n_vocab > 0 ? n_vocab : 1) * 4);
  w.ids_ref = o; o += up16((size_t)(n_ref_words > 0 ? n_ref_words : 1) * 12);
  w.ids_hyp = o; o += up16((size_t)(n_hyp_words > 0 ? n_hyp_words : 1) * 12);
  w.total = o;
  return w;
}

// what the kernels see: the caller's arrays and the carved workspace
struct metrics_dev {
  int n_images;
  const int32_t *sel, *img_ref_ptr, *ref_ptr_a, *ref_words_a, *ref_ptr_b, *ref_words_b;
  const int32_t *hyp_ptr_a, *hyp_words_a, *hyp_ptr_b, *hyp_words_b, *pair_ptr;
  int64_t n_vocab, n_ref_words, n_hyp_words;
  int64_t cap[3];
  unsigned long long* table[3];
  int32_t* df[3];
  int32_t* df1;
  int32_t *ids_ref, *ids_hyp;  // [3][n_ref_words], [3][n_hyp_words]: ids of the 2-, 3-, 4-gram starting at a word
  int32_t *stats, *lcs, *flag;
  double* cider;
};

__global__ __launch_bounds__(256) void metrics_clear_kernel(metrics_dev a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int k = 0; k < 3; ++k) {
    for (int64_t i = t0; i < a.cap[k]; i += stride) {
      a.table[k][i] = EMPTY;
      a.df[k][i] = 0;
    }
  }
  for (int64_t i = t0; i < a.n_vocab; i += stride) a.df1[i] = 0;
  if (t0 == 0) *a.flag = 0;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64's finaliser
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// The slot of `key`, inserting it if absent. A slot goes EMPTY -> key once and never changes again, so a stale read
// can only show EMPTY (the CAS then tells the truth) and a key read is final. At most `cap` probes; -1 if none fits.
__device__ __forceinline__ int table_insert(unsigned long long* table, int64_t cap, uint64_t key) {
  const uint64_t mask = (uint64_t)cap - 1;
  uint64_t slot = mix64(key) & mask;
  for (int64_t i = 0; i < cap; ++i, slot = (slot + 1) & mask) {
    unsigned long long cur = __hip_atomic_load(table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == EMPTY) cur = atomicCAS(table + slot, (unsigned long long)EMPTY, (unsigned long long)key);
    if (cur == EMPTY || cur == key) return (int)slot;
  }
  return -1;
}

__device__ __forceinline__ int clamp_len(int n) { return n < 0 ? 0 : (n > MW ? MW : n); }

// One workgroup per scored image, a wave per caption (the hypothesis, then the image's references), a lane per start
// position. ids[k][pos] = id of the (k + 2)-gram starting there, -1 where the caption is too short for it.
__global__ __launch_bounds__(256) void metrics_build_kernel(metrics_dev a) {
  const int j = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int img = a.sel[j];
  const int row0 = a.img_ref_ptr[img], m = a.img_ref_ptr[img + 1] - row0;
  for (int c = w; c <= m; c += 4) {
    const int32_t* words;
    int32_t* ids;
    int64_t base, total;
    int len;
    if (c == 0) {
      base = a.hyp_ptr_a[j]; len = clamp_len(a.hyp_ptr_a[j + 1] - (int)base);
      words = a.hyp_words_a; ids = a.ids_hyp; total = a.n_hyp_words;
    } else {
      base = a.ref_ptr_a[row0 + c - 1]; len = clamp_len(a.ref_ptr_a[row0 + c] - (int)base);
      words = a.ref_words_a; ids = a.ids_ref; total = a.n_ref_words;
    }
    if (base < 0 || base + len > total) continue;  // never past the packed arrays
    for (int p = lane; p < len; p += 64) {
      int id = words[base + p];
      for (int k = 0; k < 3; ++k) {
        if (id >= 0 && p + k + 2 <= len) {
          const uint64_t key = ((uint64_t)(uint32_t)id << 32) | (uint32_t)words[base + p + k + 1];
          id = table_insert(a.table[k], a.cap[k], key);
          if (id < 0) atomicOr(a.flag, 1);
        } else {
          id = -1;
        }
        ids[(int64_t)k * total + base + p] = id;
      }
    }
  }
}

// One workgroup per scored image over the word positions of all its references (contiguous rows, so one range).
// A position counts for its n-gram when no earlier position of the image holds the same id.
__global__ __launch_bounds__(256) void metrics_df_kernel(metrics_dev a) {
  const int img = a.sel[blockIdx.x];
  const int row0 = a.img_ref_ptr[img], row1 = a.img_ref_ptr[img + 1];
  int64_t q0 = a.ref_ptr_a[row0], q1 = a.ref_ptr_a[row1];
  if (q0 < 0) q0 = 0;
  if (q1 > a.n_ref_words) q1 = a.n_ref_words;
  for (int64_t q = q0 + threadIdx.x; q < q1; q += blockDim.x) {
    for (int k = 0; k < 4; ++k) {
      const int32_t* ids = k == 0 ? a.ref_words_a : a.ids_ref + (int64_t)(k - 1) * a.n_ref_words;
      const int id = ids[q];
      if (id < 0) continue;
      bool first = true;
      for (int64_t e = q0; e < q && first; ++e) first = ids[e] != id;
      if (!first) continue;
      if (k == 0) {
        if (id < a.n_vocab) atomicAdd(a.df1 + id, 1);
      } else if (id < a.cap[k - 1]) {
        atomicAdd(a.df[k - 1] + id, 1);
      }
    }
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// idf = log N - log max(1, df): an n-gram no reference holds has log N
__device__ __forceinline__ double idf_of(const metrics_dev& a, int k, int id, double logN) {
  int d = 0;
  if (k == 0) d = id < a.n_vocab ? a.df1[id] : 0;
  else d = id < a.cap[k - 1] ? a.df[k - 1][id] : 0;
  return logN - log((double)(d < 1 ? 1 : d));
}

// One workgroup of 512 per scored image: thread (k, p) = (tid / 128, tid % 128) owns the (k + 1)-gram starting at
// position p, of the hypothesis and (in turn) of each reference.
__global__ __launch_bounds__(512) void metrics_score_kernel(metrics_dev a) {
  __shared__ int h_id[4][MW], r_id[4][MW], h_b[MW], r_b[MW];
  __shared__ unsigned long long m_lo[MW], m_hi[MW];
  __shared__ double redc[8], redn[8], normh[4], s_score[4];
  __shared__ int s_correct[4];
  const int j = blockIdx.x, tid = threadIdx.x, k = tid >> 7, p = tid & (MW - 1), lane = tid & 63, w = tid >> 6;
  const int img = a.sel[j];
  const int row0 = a.img_ref_ptr[img], m = a.img_ref_ptr[img + 1] - row0;
  const int64_t hb_a = a.hyp_ptr_a[j], hb_b = a.hyp_ptr_b[j];
  const int len_h = clamp_len(a.hyp_ptr_a[j + 1] - (int)hb_a), len_hb = clamp_len(a.hyp_ptr_b[j + 1] - (int)hb_b);
  const double logN = log((double)a.n_images);

  int hid = -1;
  if (p + k < len_h) hid = k == 0 ? a.hyp_words_a[hb_a + p] : a.ids_hyp[(int64_t)(k - 1) * a.n_hyp_words + hb_a + p];
  h_id[k][p] = hid;
  if (tid < MW) h_b[tid] = tid < len_hb ? a.hyp_words_b[hb_b + tid] : -1;
  if (tid < 4) s_correct[tid] = 0;
  __syncthreads();

  // the hypothesis n-gram of this thread: its count, whether this is its first position, tf * idf
  int cnt_h = 0;
  bool hfirst = hid >= 0;
  double idf_h = 0.0, vh = 0.0, nh = 0.0;
  if (hid >= 0) {
    for (int e = 0; e < len_h; ++e) {
      const bool same = h_id[k][e] == hid;
      cnt_h += same;
      if (same && e < p) hfirst = false;
    }
    if (hfirst) {
      idf_h = idf_of(a, k, hid, logN);
      vh = (double)cnt_h * idf_h;
      nh = vh * vh;
    }
  }
  nh = wave_sum_f64(nh);
  if (lane == 0) redn[w] = nh;
  __syncthreads();
  if (tid < 4) normh[tid] = sqrt(redn[2 * tid] + redn[2 * tid + 1]);
  __syncthreads();

  int maxcnt = 0;
  double score_k = 0.0;         // threads 0..3: sum over references of order tid's similarity
  int best_d = 0x7fffffff, best_l = 0;  // thread 128: BLEU's closest reference length
  const int64_t pair0 = a.pair_ptr[j];
  for (int r = 0; r < m; ++r) {
    const int row = row0 + r;
    const int64_t rb_a = a.ref_ptr_a[row], rb_b = a.ref_ptr_b[row];
    const int len_r = clamp_len(a.ref_ptr_a[row + 1] - (int)rb_a), len_rb = clamp_len(a.ref_ptr_b[row + 1] - (int)rb_b);
    int rid = -1;
    if (p + k < len_r) rid = k == 0 ? a.ref_words_a[rb_a + p] : a.ids_ref[(int64_t)(k - 1) * a.n_ref_words + rb_a + p];
    r_id[k][p] = rid;
    if (tid < MW) r_b[tid] = tid < len_rb ? a.ref_words_b[rb_b + tid] : -2;
    __syncthreads();

    // hypothesis side: the reference's count of this n-gram, the clipped product
    double contrib = 0.0;
    if (hfirst) {
      int cnt_r = 0;
      for (int e = 0; e < len_r; ++e) cnt_r += r_id[k][e] == hid;
      maxcnt = cnt_r > maxcnt ? cnt_r : maxcnt;
      const double vr = (double)cnt_r * idf_h;
      contrib = (vh < vr ? vh : vr) * vr;
    }
    // reference side: this reference n-gram's share of the reference's squared norm
    double nr = 0.0;
    if (rid >= 0) {
      int cnt = 0;
      bool first = true;
      for (int e = 0; e < len_r; ++e) {
        const bool same = r_id[k][e] == rid;
        cnt += same;
        if (same && e < p) first = false;
      }
      if (first) {
        const double t = (double)cnt * idf_of(a, k, rid, logN);
        nr = t * t;
      }
    }
    // ROUGE-L: where the reference's token tid (split(" ")) stands in the hypothesis, as a 128-bit mask
    if (tid < len_rb) {
      const int wd = r_b[tid];
      unsigned long long lo = 0, hi = 0;
      for (int e = 0; e < len_hb; ++e) {
        const unsigned long long bit = h_b[e] == wd ? 1ull : 0ull;
        if (e < 64) lo |= bit << e;
        else hi |= bit << (e - 64);
      }
      m_lo[tid] = lo;
      m_hi[tid] = hi;
    }
    contrib = wave_sum_f64(contrib);
    nr = wave_sum_f64(nr);
    if (lane == 0) { redc[w] = contrib; redn[w] = nr; }
    __syncthreads();

    if (tid < 4) {
      double val = redc[2 * tid] + redc[2 * tid + 1];
      const double normr = sqrt(redn[2 * tid] + redn[2 * tid + 1]);
      if (normh[tid] != 0.0 && normr != 0.0) val /= normh[tid] * normr;
      // the library's "length" is the caption's number of bigrams
      const double delta = (double)((len_h > 0 ? len_h - 1 : 0) - (len_r > 0 ? len_r - 1 : 0));
      val *= exp(-(delta * delta) / 72.0);  // 2 sigma^2, sigma = 6
      score_k += val;
    } else if (tid == 64) {
      // bit-vector LCS (Hyyro): V' = (V + (V & M)) | (V & ~M) per reference token; zeros of V count the LCS
      unsigned long long vlo = ~0ull, vhi = ~0ull;
      for (int e = 0; e < len_rb; ++e) {
        const unsigned long long mlo = m_lo[e], mhi = m_hi[e];
        const unsigned long long ulo = vlo & mlo, uhi = vhi & mhi;
        const unsigned long long slo = vlo + ulo;
        const unsigned long long shi = vhi + uhi + (slo < vlo ? 1ull : 0ull);
        vlo = slo | (vlo & ~mlo);
        vhi = shi | (vhi & ~mhi);
      }
      int l;
      if (len_hb <= 64) {
        l = __popcll(~vlo & (len_hb == 64 ? ~0ull : ((1ull << len_hb) - 1)));
      } else {
        l = __popcll(~vlo) + __popcll(~vhi & (len_hb == 128 ? ~0ull : ((1ull << (len_hb - 64)) - 1)));
      }
      a.lcs[pair0 + r] = l;
    } else if (tid == 128) {
      const int d = len_r > len_h ? len_r - len_h : len_h - len_r;
      if (d < best_d || (d == best_d && len_r < best_l)) { best_d = d; best_l = len_r; }
    }
    __syncthreads();
  }

  if (hfirst) atomicAdd(&s_correct[k], cnt_h < maxcnt ? cnt_h : maxcnt);
  if (tid < 4) s_score[tid] = score_k;
  __syncthreads();
  if (tid == 128) {
    int32_t* st = a.stats + (int64_t)j * 10;
    st[0] = len_h;
    st[1] = best_l;
    for (int o = 0; o < 4; ++o) {
      st[2 + o] = len_h - o > 0 ? len_h - o : 0;
      st[6 + o] = s_correct[o];
    }
  } else if (tid == 0) {
    double s = ((s_score[0] + s_score[1]) + s_score[2]) + s_score[3];
    s /= 4.0;
    s /= (double)(m > 0 ? m : 1);
    a.cider[j] = s * 10.0;
  }
}

}  // namespace icap

using namespace icap;

extern "C" size_t icap_caption_metrics_workspace_bytes(int64_t n_vocab, int64_t n_ref_words, int64_t n_hyp_words,
                                                       int64_t cap2, int64_t cap3, int64_t cap4) {
  const int64_t cap[3] = {cap2, cap3, cap4};
  for (int k = 0; k < 3; ++k)
    if (cap[k] < 1 || cap[k] > (1ll << 30)) return 0;
  if (n_vocab < 0 || n_ref_words < 0 || n_hyp_words < 0) return 0;
  return ws_layout(n_vocab, n_ref_words, n_hyp_words, cap).total;
}

extern "C" int icap_caption_metrics(const icap_caption_metrics_args* args, void* stream) {
  ICAP_REQUIRE(args, "icap_caption_metrics: null args");
  const icap_caption_metrics_args& g = *args;
  ICAP_REQUIRE(g.sel && g.img_ref_ptr && g.ref_ptr_a && g.ref_words_a && g.ref_ptr_b && g.ref_words_b &&
                   g.hyp_ptr_a && g.hyp_words_a && g.hyp_ptr_b && g.hyp_words_b && g.pair_ptr && g.workspace &&
                   g.stats && g.lcs && g.cider && g.flag,
               "icap_caption_metrics: null pointer");
  ICAP_REQUIRE(g.n_images >= 1 && g.n_images < (1 << 30), "icap_caption_metrics: n_images must be >= 1");
  ICAP_REQUIRE(g.n_vocab >= 1 && g.n_vocab < (1ll << 31) && g.n_ref_words >= 0 && g.n_ref_words < (1ll << 31) &&
                   g.n_hyp_words >= 0 && g.n_hyp_words < (1ll << 31),
               "icap_caption_metrics: bad word counts");
  ICAP_REQUIRE(g.stages >= 0 && g.stages <= ICAP_METRIC_STAGE_ALL, "icap_caption_metrics: bad stages");
  for (int k = 0; k < 3; ++k) {
    const int64_t c = g.capacity[k];
    ICAP_REQUIRE(c >= 1 && c <= (1ll << 30) && (c & (c - 1)) == 0,
                 "icap_caption_metrics: a table capacity must be a power of two, at most 2^30");
    ICAP_REQUIRE(g.positions[k] >= 0 && c > g.positions[k],
                 "icap_caption_metrics: a table capacity must be greater than the number of n-gram positions");
  }
  const metrics_ws wl = ws_layout(g.n_vocab, g.n_ref_words, g.n_hyp_words, g.capacity);
  ICAP_REQUIRE(g.workspace_bytes >= wl.total, "icap_caption_metrics: workspace too small");
  ICAP_REQUIRE((reinterpret_cast<uintptr_t>(g.workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(g.cider) & 7) == 0,
               "icap_caption_metrics: workspace must be 16-byte aligned, cider 8-byte aligned");

  metrics_dev a;
  a.n_images = g.n_images;
  a.sel = g.sel; a.img_ref_ptr = g.img_ref_ptr;
  a.ref_ptr_a = g.ref_ptr_a; a.ref_words_a = g.ref_words_a; a.ref_ptr_b = g.ref_ptr_b; a.ref_words_b = g.ref_words_b;
  a.hyp_ptr_a = g.hyp_ptr_a; a.hyp_words_a = g.hyp_words_a; a.hyp_ptr_b = g.hyp_ptr_b; a.hyp_words_b = g.hyp_words_b;
  a.pair_ptr = g.pair_ptr;
  a.n_vocab = g.n_vocab; a.n_ref_words = g.n_ref_words; a.n_hyp_words = g.n_hyp_words;
  char* ws = reinterpret_cast<char*>(g.workspace);
  for (int k = 0; k < 3; ++k) {
    a.cap[k] = g.capacity[k];
    a.table[k] = reinterpret_cast<unsigned long long*>(ws + wl.table[k]);
    a.df[k] = reinterpret_cast<int32_t*>(ws + wl.df[k]);
  }
  a.df1 = reinterpret_cast<int32_t*>(ws + wl.df1);
  a.ids_ref = reinterpret_cast<int32_t*>(ws + wl.ids_ref);
  a.ids_hyp = reinterpret_cast<int32_t*>(ws + wl.ids_hyp);
  a.stats = g.stats; a.lcs = g.lcs; a.flag = g.flag; a.cider = g.cider;

  const int stages = g.stages == 0 ? ICAP_METRIC_STAGE_ALL : g.stages;
  const unsigned I = (unsigned)g.n_images;
  if (stages & ICAP_METRIC_STAGE_BUILD) {
    int64_t big = g.n_vocab;
    for (int k = 0; k < 3; ++k) big = a.cap[k] > big ? a.cap[k] : big;
    const int64_t blocks = (big + 255) / 256;
    hipLaunchKernelGGL(metrics_clear_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, S_(stream),
                       a);
    int rc = check_launch("icap_caption_metrics(clear)");
    if (rc) return rc;
    hipLaunchKernelGGL(metrics_build_kernel, dim3(I), dim3(256), 0, S_(stream), a);
    rc = check_launch("icap_caption_metrics(build)");
    if (rc) return rc;
  }
  if (stages & ICAP_METRIC_STAGE_DF) {
    hipLaunchKernelGGL(metrics_df_kernel, dim3(I), dim3(256), 0, S_(stream), a);
    const int rc = check_launch("icap_caption_metrics(df)");
    if (rc) return rc;
  }
  if (stages & ICAP_METRIC_STAGE_SCORE) {
    hipLaunchKernelGGL(metrics_score_kernel, dim3(I), dim3(512), 0, S_(stream), a);
    const int rc = check_launch("icap_caption_metrics(score)");
    if (rc) return rc;
  }
  return ICAP_OK;
}
