// Host-only JPEG unit: the marker parser that decides which files the device path decodes (icap_jpeg_parse) and a
// host decoder built from jpeg_common.h's inline functions, for tests (icap_jpeg_decode_host). No kernel, no HIP
// header, no global state: it compiles with a plain host compiler, links into libicap_hip.so and is also built on
// its own as libicap_jpeg_host.so, which loader workers use so that they never load the HIP runtime.
#include <string.h>

#include <vector>

#include "jpeg_common.h"

namespace {

using namespace icap;

const uint8_t kZigzag[64] = ICAP_JPEG_ZIGZAG;

struct Reader {
  const uint8_t* d;
  int64_t size, pos;
  bool has(int64_t n) const { return pos + n <= size; }
  int u8() { return d[pos++]; }
  int u16() {
    const int v = (d[pos] << 8) | d[pos + 1];
    pos += 2;
    return v;
  }
};

// counts[1..16], vals[0, nvals) -> the canonical form; false unless they are a prefix code
bool build_huff(const uint8_t counts[17], const uint8_t* vals, int nvals, bool is_dc, icap_jpeg_huff* h) {
  memset(h, 0, sizeof(*h));
  for (int i = 0; i < nvals; ++i) {
    if (is_dc && vals[i] > 15) return false;
    h->vals[i] = vals[i];
  }
  int32_t code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    h->valoff[l] = k - code;
    for (int i = 0; i < counts[l]; ++i, ++k, ++code) {
      if (code >= (1 << l)) return false;
      if (l <= ICAP_JPEG_LOOK_BITS) {
        const int first = code << (ICAP_JPEG_LOOK_BITS - l), span = 1 << (ICAP_JPEG_LOOK_BITS - l);
        for (int j = 0; j < span; ++j) h->look[first + j] = (uint16_t)((l << 8) | vals[k]);
      }
    }
    h->maxcode[l] = counts[l] ? code - 1 : -1;
    code <<= 1;
  }
  h->maxcode[0] = h->maxcode[17] = -1;
  return true;
}

struct Frame {
  bool sof = false, jfif = false;
  int ids[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
  bool have_q[4] = {false, false, false, false}, have_h[4] = {false, false, false, false};
  uint16_t q[4][64];
};

bool parse_sof0(Reader& r, int64_t end, icap_jpeg_desc* d, Frame* f) {
  if (f->sof || end - r.pos < 6) return false;
  if (r.u8() != 8) return false;
  d->height = r.u16();
  d->width = r.u16();
  d->ncomp = r.u8();
  if (d->height < 1 || d->width < 1 || d->height > ICAP_JPEG_MAX_DIM || d->width > ICAP_JPEG_MAX_DIM) return false;
  if ((d->ncomp != 1 && d->ncomp != 3) || end - r.pos != 3 * d->ncomp) return false;
  for (int c = 0; c < d->ncomp; ++c) {
    f->ids[c] = r.u8();
    const int hv = r.u8(), h = hv >> 4, v = hv & 15;
    f->tq[c] = r.u8();
    if (f->tq[c] > 3) return false;
    if (c == 0) {
      if (!((h == 1 && v == 1) || (d->ncomp == 3 && h == 2 && (v == 1 || v == 2)))) return false;
      d->hs = h;
      d->vs = v;
    } else if (h != 1 || v != 1) {
      return false;
    }
  }
  d->mcus_x = (d->width + 8 * d->hs - 1) / (8 * d->hs);
  d->mcus_y = (d->height + 8 * d->vs - 1) / (8 * d->vs);
  d->blocks = jpeg_blocks(d);
  f->sof = true;
  return true;
}

bool parse_dqt(Reader& r, int64_t end, Frame* f) {
  while (r.pos < end) {
    const int pt = r.u8();
    if ((pt >> 4) != 0 || (pt & 15) > 3 || end - r.pos < 64) return false;  // 8-bit tables only
    for (int i = 0; i < 64; ++i) f->q[pt & 15][kZigzag[i]] = (uint16_t)r.u8();
    f->have_q[pt & 15] = true;
  }
  return true;
}

bool parse_dht(Reader& r, int64_t end, icap_jpeg_desc* d, Frame* f) {
  while (r.pos < end) {
    if (end - r.pos < 17) return false;
    const int tc = r.u8(), cls = tc >> 4, id = tc & 15;
    if (cls > 1 || id > 1) return false;  // baseline: two DC and two AC tables
    uint8_t counts[17] = {0};
    int n = 0;
    for (int l = 1; l <= 16; ++l) n += counts[l] = (uint8_t)r.u8();
    if (n > 256 || end - r.pos < n) return false;
    if (!build_huff(counts, r.d + r.pos, n, cls == 0, &d->huff[cls * 2 + id])) return false;
    r.pos += n;
    f->have_h[cls * 2 + id] = true;
  }
  return true;
}

bool parse_sos(Reader& r, int64_t end, icap_jpeg_desc* d, const Frame& f) {
  if (!f.sof || end - r.pos != 1 + 2 * d->ncomp + 3) return false;
  if (r.u8() != d->ncomp) return false;
  for (int c = 0; c < d->ncomp; ++c) {
    if (r.u8() != f.ids[c]) return false;  // the frame's components, in the frame's order
    const int t = r.u8();
    d->dc_tab[c] = t >> 4;
    d->ac_tab[c] = t & 15;
    if (d->dc_tab[c] > 1 || d->ac_tab[c] > 1 || !f.have_h[d->dc_tab[c]] || !f.have_h[2 + d->ac_tab[c]]) return false;
    if (!f.have_q[f.tq[c]]) return false;
    memcpy(d->quant[c], f.q[f.tq[c]], sizeof(d->quant[c]));
  }
  const int ss = r.u8(), se = r.u8(), ahal = r.u8();
  return ss == 0 && se == 63 && ahal == 0;
}

// The entropy data from r.pos: one segment per restart interval, RSTn in sequence between them, then EOI.
bool scan_segments(Reader& r, icap_jpeg_desc* d, icap_jpeg_segment* segs) {
  const int64_t total = (int64_t)d->mcus_x * d->mcus_y;
  const int64_t ri = d->restart_interval;
  d->nseg = (int32_t)(ri ? (total + ri - 1) / ri : 1);
  int64_t start = r.pos, i = r.pos;
  int32_t k = 0;
  while (i + 1 < r.size) {
    if (r.d[i] != 0xff || r.d[i + 1] == 0x00 || r.d[i + 1] == 0xff) {
      ++i;  // a data byte, a stuffed 0xFF (its 0x00 is passed next), or a fill byte before a marker
      continue;
    }
    const int m = r.d[i + 1];
    if (segs) {
      segs[k].offset = start;
      segs[k].length = i - start;
      segs[k].first_mcu = (int32_t)(ri ? k * ri : 0);
      segs[k].mcu_count = (int32_t)(ri ? (total - k * ri < ri ? total - k * ri : ri) : total);
    }
    if (m >= 0xd0 && m <= 0xd7) {
      if (ri == 0 || k + 1 >= d->nseg || m != 0xd0 + (k & 7)) return false;
      ++k;
      i += 2;
      start = i;
      continue;
    }
    return m == 0xd9 && k + 1 == d->nseg;  // EOI; another scan, DNL or anything else is not decoded here
  }
  return false;  // the data ends without EOI
}

int parse(const uint8_t* data, int64_t size, icap_jpeg_desc* d, icap_jpeg_segment* segs) {
  Reader r{data, size, 0};
  Frame f;
  memset(d, 0, sizeof(*d));
  if (size < 4 || data[0] != 0xff || data[1] != 0xd8) return ICAP_JPEG_UNSUPPORTED;
  r.pos = 2;
  for (;;) {
    if (!r.has(2) || r.u8() != 0xff) return ICAP_JPEG_UNSUPPORTED;
    int m = r.u8();
    while (m == 0xff && r.has(1)) m = r.u8();  // fill bytes
    const bool skip = (m >= 0xe0 && m <= 0xef) || m == 0xfe;
    if (!(m == 0xc0 || m == 0xc4 || m == 0xdb || m == 0xdd || m == 0xda || skip))
      return ICAP_JPEG_UNSUPPORTED;  // another SOF, DAC, DNL, RSTn, EOI before a scan, ...
    if (!r.has(2)) return ICAP_JPEG_UNSUPPORTED;
    const int len = r.u16();
    const int64_t end = r.pos - 2 + len;
    if (len < 2 || end > size) return ICAP_JPEG_UNSUPPORTED;
    bool ok = true;
    if (m == 0xc0) {
      ok = parse_sof0(r, end, d, &f);
    } else if (m == 0xc4) {
      ok = parse_dht(r, end, d, &f);
    } else if (m == 0xdb) {
      ok = parse_dqt(r, end, &f);
    } else if (m == 0xdd) {
      ok = len == 4;
      if (ok) d->restart_interval = r.u16();
    } else if (m == 0xe0) {
      if (len >= 16 && memcmp(data + r.pos, "JFIF\0", 5) == 0) f.jfif = true;
    } else if (m == 0xee) {
      if (len >= 7 && memcmp(data + r.pos, "Adobe", 5) == 0) ok = false;  // its transform flag picks the colours
    } else if (m == 0xda) {
      ok = parse_sos(r, end, d, f);
      if (ok && d->ncomp == 3 && !f.jfif && f.ids[0] == 'R' && f.ids[1] == 'G' && f.ids[2] == 'B') ok = false;
      if (!ok) return ICAP_JPEG_UNSUPPORTED;
      r.pos = end;
      return scan_segments(r, d, segs) ? ICAP_JPEG_OK : ICAP_JPEG_UNSUPPORTED;
    }
    if (!ok) return ICAP_JPEG_UNSUPPORTED;
    r.pos = end;
  }
}

}  // namespace

extern "C" int icap_jpeg_parse(const uint8_t* data, int64_t size, icap_jpeg_desc* desc, icap_jpeg_segment* segs,
                               int64_t max_segs) {
  if (!desc || size < 0 || (!data && size > 0)) return ICAP_ERR_ARG;
  icap_jpeg_desc d;
  int rc = parse(data, size, &d, nullptr);
  if (rc == ICAP_JPEG_OK && segs) {
    if (max_segs < d.nseg) return ICAP_ERR_ARG;
    rc = parse(data, size, &d, segs);
  }
  *desc = d;
  return rc;
}

extern "C" int icap_jpeg_decode_host(const uint8_t* data, int64_t size, const icap_jpeg_desc* desc,
                                     const icap_jpeg_segment* segs, uint8_t* out, int32_t* status) {
  if (!data || !desc || !segs || !out || !status || size < 0) return ICAP_ERR_ARG;
  const icap_jpeg_desc* d = desc;
  if ((d->ncomp != 1 && d->ncomp != 3) || d->hs < 1 || d->hs > 2 || d->vs < 1 || d->vs > d->hs || d->width < 1 ||
      d->height < 1 || d->width > ICAP_JPEG_MAX_DIM || d->height > ICAP_JPEG_MAX_DIM ||
      d->mcus_x != (d->width + 8 * d->hs - 1) / (8 * d->hs) || d->mcus_y != (d->height + 8 * d->vs - 1) / (8 * d->vs) ||
      d->blocks != jpeg_blocks(d) || d->nseg < 1)
    return ICAP_ERR_ARG;
  std::vector<int16_t> coef((size_t)d->blocks * 64, 0);
  std::vector<uint8_t> planes((size_t)d->blocks * 64, 0);
  int32_t st = JPEG_OK;
  for (int32_t s = 0; s < d->nseg; ++s) {
    const icap_jpeg_segment& g = segs[s];
    int rc = JPEG_BAD_SEGMENT;
    if (g.offset >= 0 && g.length >= 0 && g.offset <= size && g.length <= size - g.offset)
      rc = jpeg_decode_segment(d, d->huff, kZigzag, data + g.offset, g.length, g.first_mcu, g.mcu_count, coef.data());
    if (rc > st) st = rc;
  }
  *status = st;
  if (st != JPEG_OK) return ICAP_OK;
  for (int c = 0; c < d->ncomp; ++c) {
    const JpegComp k = jpeg_comp(d, c);
    for (int32_t b = 0; b < k.bw * k.bh; ++b) {
      const int32_t by = b / k.bw, bx = b - by * k.bw;
      jpeg_idct_block(coef.data() + (int64_t)(k.block0 + b) * 64, d->quant[c],
                      planes.data() + k.plane0 + ((int64_t)by * 8 * k.bw + bx) * 8, (int64_t)k.bw * 8);
    }
  }
  for (int32_t y = 0; y < d->height; ++y)
    for (int32_t x = 0; x < d->width; ++x) jpeg_pixel(d, planes.data(), y, x, out + ((int64_t)y * d->width + x) * 3);
  return ICAP_OK;
}
