// Stand-alone host check of jpeg_host.cpp (make jpeg_check; make SAN=1 jpeg_check for ASan + UBSan): no GPU, nothing
// loaded into Python. Given one JPEG file it decodes the file as it is, then every truncation of it and 200 copies
// with one bit of the entropy data flipped at seeded positions. Each of those must end in pixels or in an error
// (parser "unsupported" or a decoder status), never in a fault; every buffer is sized exactly, so under the
// sanitizers a read or write one byte outside fails the run.
//
//   jpeg_check FILE  ->  intact <fnv1a64 of the RGB bytes> <height> <width>
//                        truncations <count> pixels <n> errors <n>
//                        flips <count> pixels <n> errors <n>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "icap.h"

namespace {

// 0: pixels (into *rgb), 1: an error status or "unsupported"; -1: the unit misbehaved
int decode(const std::vector<uint8_t>& file, std::vector<uint8_t>* rgb, icap_jpeg_desc* desc,
           std::vector<icap_jpeg_segment>* segs) {
  // an exact-size copy, so that the sanitizers see the true end of the file
  std::vector<uint8_t> data(file.begin(), file.end());
  int rc = icap_jpeg_parse(data.data(), (int64_t)data.size(), desc, nullptr, 0);
  if (rc == ICAP_JPEG_UNSUPPORTED) return 1;
  if (rc != ICAP_JPEG_OK || desc->nseg < 1) return -1;
  segs->assign((size_t)desc->nseg, icap_jpeg_segment());
  rc = icap_jpeg_parse(data.data(), (int64_t)data.size(), desc, segs->data(), desc->nseg);
  if (rc != ICAP_JPEG_OK) return -1;
  rgb->assign((size_t)desc->height * desc->width * 3, 0);
  int32_t status = -1;
  rc = icap_jpeg_decode_host(data.data(), (int64_t)data.size(), desc, segs->data(), rgb->data(), &status);
  if (rc != ICAP_OK || status < 0) return -1;
  return status == 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: jpeg_check FILE\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    fprintf(stderr, "jpeg_check: cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<uint8_t> file;
  for (int c; (c = fgetc(f)) != EOF;) file.push_back((uint8_t)c);
  fclose(f);

  std::vector<uint8_t> rgb;
  std::vector<icap_jpeg_segment> segs;
  icap_jpeg_desc desc;
  if (decode(file, &rgb, &desc, &segs) != 0) {
    fprintf(stderr, "jpeg_check: the intact file did not decode\n");
    return 1;
  }
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint8_t v : rgb) h = (h ^ v) * 0x100000001b3ull;
  printf("intact %016llx %d %d\n", (unsigned long long)h, desc.height, desc.width);
  const int64_t e0 = segs.front().offset, e1 = segs.back().offset + segs.back().length;

  int pixels = 0, errors = 0;
  for (size_t n = 0; n < file.size(); ++n) {
    std::vector<uint8_t> cut(file.begin(), file.begin() + n), out;
    icap_jpeg_desc d;
    std::vector<icap_jpeg_segment> s;
    const int r = decode(cut, &out, &d, &s);
    if (r < 0) return 1;
    (r == 0 ? pixels : errors)++;
  }
  printf("truncations %zu pixels %d errors %d\n", file.size(), pixels, errors);

  pixels = errors = 0;
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  const int flips = 200;
  for (int i = 0; i < flips; ++i) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t bit = (rng >> 24) % (uint64_t)((e1 - e0) * 8);
    std::vector<uint8_t> bad(file), out;
    bad[(size_t)e0 + bit / 8] ^= (uint8_t)(1u << (bit % 8));
    icap_jpeg_desc d;
    std::vector<icap_jpeg_segment> s;
    const int r = decode(bad, &out, &d, &s);
    if (r < 0) return 1;
    (r == 0 ? pixels : errors)++;
  }
  printf("flips %d pixels %d errors %d\n", flips, pixels, errors);
  return 0;
}
