// Baseline JPEG arithmetic shared by the host unit (jpeg_host.cpp) and the kernels (jpeg.hip): the bounded bit
// reader, Huffman symbol decode from the canonical tables of icap_jpeg_huff, one block's coefficient decode, the
// 8 x 8 "islow" integer IDCT, the "fancy" chroma upsampling and the fixed-point YCbCr -> RGB transform, restated
// from libjpeg's documented algorithms so that the output equals Pillow's decode byte for byte ("Device
// JPEG decode"). Plain inline functions, no HIP runtime call; every function is __host__ __device__ when the unit is
// compiled as HIP and a plain function otherwise.
//
// Defined arithmetic: a malformed stream may drive any value out of its range, so sums and products that a valid
// stream keeps inside 32 bits are formed in unsigned 32-bit (they wrap, identically on host and device) and read back
// as two's complement; shifts of signed values are arithmetic.
#pragma once

#include <stdint.h>

#include "icap.h"

#if defined(__HIP__)
#define ICAP_HD __host__ __device__ inline __attribute__((always_inline))
#define ICAP_UNROLL _Pragma("unroll")
#else
#define ICAP_HD static inline
#define ICAP_UNROLL
#endif

// zigzag position -> natural (row-major) position; the host unit and the kernels each hold one copy of this list
#define ICAP_JPEG_ZIGZAG                                                                                     \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,                   \
   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,                   \
   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

namespace icap {

// status word of one image (icap_jpeg_decode's status[i], icap_jpeg_decode_host's *status); the largest wins
enum { JPEG_OK = 0, JPEG_BAD_CODE = 1, JPEG_BAD_RUN = 2, JPEG_BAD_SEGMENT = 3 };

// ---- bit reader ------------------------------------------------------------------------------------------------
// Reads the `len` bytes at p, most significant bit first. A 0xFF 0x00 pair is the data byte 0xFF; 0xFF before
// anything else (a marker, or the last byte) ends the data. Past the end every bit is zero, so no read leaves
// [p, p + len). The device build fetches the stream through the aligned 16-byte chunk that holds the byte (the
// caller guarantees whole chunks are readable: icap_jpeg_decode's data is 16-byte aligned and padded).
struct JpegBits {
  const uint8_t* p;
  int64_t len, pos;
  uint32_t acc;  // the low n bits are the unread bits
  int32_t n;
#if defined(__HIP_DEVICE_COMPILE__)
  uint64_t w0, w1;
  uintptr_t chunk;
#endif
};

ICAP_HD void jpeg_bits_init(JpegBits& b, const uint8_t* p, int64_t len) {
  b.p = p;
  b.len = len < 0 ? 0 : len;
  b.pos = 0;
  b.acc = 0;
  b.n = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  b.w0 = b.w1 = 0;
  b.chunk = 0;
#endif
}

// byte at pos < len
ICAP_HD uint32_t jpeg_bits_byte(JpegBits& b, int64_t pos) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uintptr_t a = reinterpret_cast<uintptr_t>(b.p) + (uintptr_t)pos;
  const uintptr_t c = a & ~(uintptr_t)15;
  if (c != b.chunk) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // one 16-byte load
    const u32x4 v = *reinterpret_cast<const u32x4*>(c);
    b.w0 = (uint64_t)v[0] | ((uint64_t)v[1] << 32);
    b.w1 = (uint64_t)v[2] | ((uint64_t)v[3] << 32);
    b.chunk = c;
  }
  const uint32_t i = (uint32_t)(a & 15);
  const uint64_t hi = (uint64_t)0 - (uint64_t)(i >> 3);  // a mask, not a select: a select of two members is turned
  return (uint32_t)((((b.w0 & ~hi) | (b.w1 & hi)) >> ((i & 7) * 8)) & 0xff);  // into an indexed read of scratch
#else
  return b.p[pos];
#endif
}

// at least 25 unread bits
ICAP_HD void jpeg_bits_fill(JpegBits& b) {
  while (b.n <= 24) {
    uint32_t v = 0;
    if (b.pos < b.len) {
      v = jpeg_bits_byte(b, b.pos);
      ++b.pos;
      if (v == 0xff) {
        if (b.pos < b.len && jpeg_bits_byte(b, b.pos) == 0) {
          ++b.pos;
        } else {  // a marker or the end: nothing more to read
          b.pos = b.len;
          v = 0;
        }
      }
    }
    b.acc = (b.acc << 8) | v;
    b.n += 8;
  }
}

// the next k <= 16 bits, after jpeg_bits_fill
ICAP_HD uint32_t jpeg_bits_peek(const JpegBits& b, int k) { return (b.acc >> (b.n - k)) & ((1u << k) - 1u); }
ICAP_HD void jpeg_bits_skip(JpegBits& b, int k) { b.n -= k; }

// ---- Huffman ---------------------------------------------------------------------------------------------------
// One symbol, or -1 when the next 16 bits begin with no code of the table.
ICAP_HD int jpeg_huff_decode(JpegBits& b, const icap_jpeg_huff* h) {
  jpeg_bits_fill(b);
  const uint32_t look = jpeg_bits_peek(b, 16);
  const uint32_t e = h->look[look >> (16 - ICAP_JPEG_LOOK_BITS)];
  if (e) {
    jpeg_bits_skip(b, (int)(e >> 8));
    return (int)(e & 0xff);
  }
  for (int l = ICAP_JPEG_LOOK_BITS + 1; l <= 16; ++l) {
    const int32_t code = (int32_t)(look >> (16 - l));
    if (code <= h->maxcode[l]) {
      jpeg_bits_skip(b, l);
      return h->vals[(uint32_t)(h->valoff[l] + code) & 0xff];
    }
  }
  return -1;
}

// the next s <= 15 bits as a signed value (ITU T.81 F.2.2.1 EXTEND)
ICAP_HD int32_t jpeg_receive_extend(JpegBits& b, int s) {
  if (s == 0) return 0;
  jpeg_bits_fill(b);
  const int32_t v = (int32_t)jpeg_bits_peek(b, s);
  jpeg_bits_skip(b, s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block: out[64] = the quantised coefficients in natural order; pred is the component's DC predictor. zigzag
// is the caller's copy of ICAP_JPEG_ZIGZAG. At most 64 symbols are read. Returns a status (JPEG_OK or the error).
ICAP_HD int jpeg_decode_block(JpegBits& b, const icap_jpeg_huff* dc, const icap_jpeg_huff* ac, int32_t& pred,
                              const uint8_t* zigzag, int16_t* out) {
  for (int i = 0; i < 64; ++i) out[i] = 0;
  const int s = jpeg_huff_decode(b, dc);
  if (s < 0) return JPEG_BAD_CODE;
  if (s > 15) return JPEG_BAD_RUN;
  pred = (int32_t)(int16_t)(uint16_t)((uint32_t)pred + (uint32_t)jpeg_receive_extend(b, s));
  out[0] = (int16_t)pred;
  for (int k = 1; k < 64; ++k) {
    const int rs = jpeg_huff_decode(b, ac);
    if (rs < 0) return JPEG_BAD_CODE;
    const int r = rs >> 4, sz = rs & 15;
    if (sz == 0) {
      if (r != 15) break;  // end of block
      k += 15;             // sixteen zeros
      continue;
    }
    k += r;
    if (k > 63) return JPEG_BAD_RUN;
    out[zigzag[k]] = (int16_t)jpeg_receive_extend(b, sz);
  }
  return JPEG_OK;
}

// ---- IDCT (islow: CONST_BITS 13, PASS1_BITS 2) -----------------------------------------------------------------
ICAP_HD uint32_t jpeg_mul(uint32_t a, int32_t c) { return a * (uint32_t)c; }
ICAP_HD uint32_t jpeg_descale(uint32_t x, int n) { return (uint32_t)((int32_t)(x + (1u << (n - 1))) >> n); }

// eight values in, eight out (stride apart), descaled by `shift`
ICAP_HD void jpeg_idct_1d(const uint32_t in[8], uint32_t* out, int stride, int shift) {
  uint32_t z2 = in[2], z3 = in[6];
  uint32_t z1 = jpeg_mul(z2 + z3, 4433);
  uint32_t tmp2 = z1 + jpeg_mul(z3, -15137);
  uint32_t tmp3 = z1 + jpeg_mul(z2, 6270);
  uint32_t tmp0 = (in[0] + in[4]) << 13;
  uint32_t tmp1 = (in[0] - in[4]) << 13;
  const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  uint32_t z4 = tmp1 + tmp3;
  const uint32_t z5 = jpeg_mul(z3 + z4, 9633);
  tmp0 = jpeg_mul(tmp0, 2446);
  tmp1 = jpeg_mul(tmp1, 16819);
  tmp2 = jpeg_mul(tmp2, 25172);
  tmp3 = jpeg_mul(tmp3, 12299);
  z1 = jpeg_mul(z1, -7373);
  z2 = jpeg_mul(z2, -20995);
  z3 = jpeg_mul(z3, -16069) + z5;
  z4 = jpeg_mul(z4, -3196) + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  out[0 * stride] = jpeg_descale(tmp10 + tmp3, shift);
  out[7 * stride] = jpeg_descale(tmp10 - tmp3, shift);
  out[1 * stride] = jpeg_descale(tmp11 + tmp2, shift);
  out[6 * stride] = jpeg_descale(tmp11 - tmp2, shift);
  out[2 * stride] = jpeg_descale(tmp12 + tmp1, shift);
  out[5 * stride] = jpeg_descale(tmp12 - tmp1, shift);
  out[3 * stride] = jpeg_descale(tmp13 + tmp0, shift);
  out[4 * stride] = jpeg_descale(tmp13 - tmp0, shift);
}

ICAP_HD uint8_t jpeg_clamp8(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// coef[64] (quantised, natural order) x q[64] -> 8 rows of 8 samples at out, out_stride bytes apart
ICAP_HD void jpeg_idct_block(const int16_t* coef, const uint16_t* q, uint8_t* out, int64_t out_stride) {
  uint32_t ws[64];  // fully unrolled on the device, so it stays in registers
  ICAP_UNROLL
  for (int c = 0; c < 8; ++c) {  // columns: descale by CONST_BITS - PASS1_BITS
    uint32_t in[8];
    ICAP_UNROLL
    for (int r = 0; r < 8; ++r) in[r] = (uint32_t)((int32_t)coef[r * 8 + c] * (int32_t)q[r * 8 + c]);
    jpeg_idct_1d(in, ws + c, 8, 11);
  }
  ICAP_UNROLL
  for (int r = 0; r < 8; ++r) {  // rows: descale by CONST_BITS + PASS1_BITS + 3
    uint32_t o[8];
    jpeg_idct_1d(ws + r * 8, o, 1, 18);
    ICAP_UNROLL
    for (int c = 0; c < 8; ++c) out[r * out_stride + c] = jpeg_clamp8((int32_t)(o[c] + 128u));
  }
}

// ---- geometry --------------------------------------------------------------------------------------------------
// Component c of d: sampling (h, v), the padded plane (pw x ph samples, a whole number of MCUs) and its block grid.
struct JpegComp {
  int32_t h, v;      // sampling factors
  int32_t bw, bh;    // blocks per row / column of the padded plane
  int32_t block0;    // first block of the component in the image's coefficient array
  int64_t plane0;    // first byte of the component's plane in the image's plane area
};
ICAP_HD JpegComp jpeg_comp(const icap_jpeg_desc* d, int c) {
  JpegComp k;
  const int32_t yb = d->mcus_x * d->hs * d->mcus_y * d->vs, cb = d->mcus_x * d->mcus_y;
  k.h = c == 0 ? d->hs : 1;
  k.v = c == 0 ? d->vs : 1;
  k.bw = d->mcus_x * k.h;
  k.bh = d->mcus_y * k.v;
  k.block0 = c == 0 ? 0 : yb + (c - 1) * cb;
  k.plane0 = (int64_t)k.block0 * 64;
  return k;
}
ICAP_HD int32_t jpeg_blocks(const icap_jpeg_desc* d) {
  return d->mcus_x * d->mcus_y * (d->hs * d->vs + (d->ncomp == 3 ? 2 : 0));
}

// ---- upsampling and colour -------------------------------------------------------------------------------------
// The chroma sample of output pixel (y, x) from a plane of stride pw whose real (downsampled) size is cw x ch, for
// luma sampling hs x vs (1x1: the sample itself; 2x1: h2v1; 2x2: h2v2). Planes at most 2 samples wide are
// replicated, as libjpeg does; samples beyond cw x ch are never read.
ICAP_HD int32_t jpeg_chroma_at(const uint8_t* plane, int64_t pw, int32_t cw, int32_t ch, int hs, int vs, int32_t y,
                               int32_t x) {
  if (hs == 1) return plane[(int64_t)y * pw + x];
  const int32_t cx = x >> 1;
  if (vs == 1) {
    const uint8_t* row = plane + (int64_t)y * pw;
    const int32_t p = row[cx];
    if (cw <= 2) return p;
    if (x & 1) return cx == cw - 1 ? p : (3 * p + row[cx + 1] + 2) >> 2;
    return cx == 0 ? p : (3 * p + row[cx - 1] + 1) >> 2;
  }
  const int32_t cy = y >> 1;
  if (cw <= 2) return plane[(int64_t)cy * pw + cx];
  int32_t fy = (y & 1) ? cy + 1 : cy - 1;  // the far row; past an edge it is the edge row itself
  fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
  const uint8_t* nr = plane + (int64_t)cy * pw;
  const uint8_t* fr = plane + (int64_t)fy * pw;
  const int32_t c = 3 * nr[cx] + fr[cx];
  if (x & 1) return cx == cw - 1 ? (4 * c + 7) >> 4 : (3 * c + 3 * nr[cx + 1] + fr[cx + 1] + 7) >> 4;
  return cx == 0 ? (4 * c + 8) >> 4 : (3 * c + 3 * nr[cx - 1] + fr[cx - 1] + 8) >> 4;
}

ICAP_HD void jpeg_ycc_to_rgb(int32_t yy, int32_t cb, int32_t cr, uint8_t* rgb) {
  cb -= 128;
  cr -= 128;
  rgb[0] = jpeg_clamp8(yy + ((91881 * cr + 32768) >> 16));
  rgb[1] = jpeg_clamp8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = jpeg_clamp8(yy + ((116130 * cb + 32768) >> 16));
}

// RGB of pixel (y, x) of image d from its planes (the area jpeg_comp's plane0 indexes)
ICAP_HD void jpeg_pixel(const icap_jpeg_desc* d, const uint8_t* planes, int32_t y, int32_t x, uint8_t* rgb) {
  const JpegComp k0 = jpeg_comp(d, 0);
  const int32_t yy = planes[k0.plane0 + (int64_t)y * (k0.bw * 8) + x];
  if (d->ncomp == 1) {
    rgb[0] = rgb[1] = rgb[2] = (uint8_t)yy;
    return;
  }
  const JpegComp k1 = jpeg_comp(d, 1), k2 = jpeg_comp(d, 2);
  const int32_t cw = (d->width + d->hs - 1) / d->hs, ch = (d->height + d->vs - 1) / d->vs;
  const int32_t cb = jpeg_chroma_at(planes + k1.plane0, (int64_t)k1.bw * 8, cw, ch, d->hs, d->vs, y, x);
  const int32_t cr = jpeg_chroma_at(planes + k2.plane0, (int64_t)k2.bw * 8, cw, ch, d->hs, d->vs, y, x);
  jpeg_ycc_to_rgb(yy, cb, cr, rgb);
}

// The MCUs [first, first + count) of one entropy segment into coef (the image's [blocks][64] array). Returns the
// segment's status; decoding stops at the first error.
ICAP_HD int jpeg_decode_segment(const icap_jpeg_desc* d, const icap_jpeg_huff* huff, const uint8_t* zigzag,
                                const uint8_t* p, int64_t len, int32_t first, int32_t count, int16_t* coef) {
  const int32_t total = d->mcus_x * d->mcus_y;
  if (first < 0 || count < 0 || first > total || count > total - first) return JPEG_BAD_SEGMENT;
  JpegBits b;
  jpeg_bits_init(b, p, len);
  int32_t pred0 = 0, pred1 = 0, pred2 = 0;  // named, not an array: a component-indexed array would live in scratch
  for (int32_t m = first; m < first + count; ++m) {
    const int32_t my = m / d->mcus_x, mx = m - my * d->mcus_x;
    for (int c = 0; c < d->ncomp; ++c) {
      const JpegComp k = jpeg_comp(d, c);
      const icap_jpeg_huff* dc = huff + (d->dc_tab[c] & 1);
      const icap_jpeg_huff* ac = huff + 2 + (d->ac_tab[c] & 1);
      int32_t pred = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
      for (int v = 0; v < k.v; ++v)
        for (int h = 0; h < k.h; ++h) {
          const int32_t blk = k.block0 + (my * k.v + v) * k.bw + mx * k.h + h;
          const int rc = jpeg_decode_block(b, dc, ac, pred, zigzag, coef + (int64_t)blk * 64);
          if (rc != JPEG_OK) return rc;
        }
      if (c == 0) pred0 = pred;
      else if (c == 1) pred1 = pred;
      else pred2 = pred;
    }
  }
  return JPEG_OK;
}

}  // namespace icap
