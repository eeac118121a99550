// Baseline JPEG decode on the device (DESIGN.md "Device JPEG decode"): entropy decode,
// dequantise + IDCT, chroma upsampling + YCbCr -> RGB, one launch each behind icap_jpeg_decode. All arithmetic is
// jpeg_common.h's, shared with the host decoder, so the RGB bytes are Pillow's.
//
// Entropy decode is serial within a segment (every code's position depends on the one before), so a segment is one
// lane's work and the launch's parallelism is images x segments: workgroup (chunk, image) is one wave whose lanes
// take segments chunk * 64 .. + 63 of that image. The image's four Huffman tables are staged in LDS once per
// workgroup (5.6 KiB: many workgroups per CU), so every lane of the wave reads the same tables while following its
// own stream. A file without restart markers is one active lane; the wave's other lanes would have diverged from it
// anyway (each stream takes its own branches), so what bounds throughput there is images per launch, not lane use.
//
// No read leaves its buffer on any input: stream bytes are fetched inside [segment start, + length) clipped to the
// image's data_len and to data_bytes, block indices come from the descriptor, whose fields are checked first, and
// every loop is bounded by blocks x 64 symbols. A stream that does not decode ends in status[image].
#include "common.h"
#include "jpeg_common.h"

namespace icap {

__constant__ uint8_t jpeg_zigzag[64] = ICAP_JPEG_ZIGZAG;
constexpr int JPEG_LAYOUT = 5;  // data_off, data_len, seg_off, work_off, out_off

// the descriptor fields the index arithmetic rests on
__device__ __forceinline__ bool jpeg_desc_ok(const icap_jpeg_desc* d) {
  return (d->ncomp == 1 || d->ncomp == 3) && d->hs >= 1 && d->hs <= 2 && d->vs >= 1 && d->vs <= d->hs &&
         d->width >= 1 && d->height >= 1 && d->width <= ICAP_JPEG_MAX_DIM && d->height <= ICAP_JPEG_MAX_DIM &&
         d->mcus_x == (d->width + 8 * d->hs - 1) / (8 * d->hs) && d->mcus_y == (d->height + 8 * d->vs - 1) / (8 * d->vs) &&
         d->blocks == jpeg_blocks(d) && d->nseg >= 1;
}

// status[i] = 0 before the segments' lanes raise it (a kernel like every other node of a captured decode)
__global__ __launch_bounds__(256) void jpeg_status_clear_kernel(int n, int32_t* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) status[i] = 0;
}

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(int n, const uint8_t* __restrict__ data, int64_t data_bytes,
                                                          const icap_jpeg_desc* __restrict__ descs,
                                                          const icap_jpeg_segment* __restrict__ segs,
                                                          int64_t total_segs, const int64_t* __restrict__ layout,
                                                          int16_t* __restrict__ coef, int32_t* __restrict__ status) {
  __shared__ icap_jpeg_huff huff[4];
  __shared__ uint8_t zigzag[64];
  const int img = blockIdx.y;
  if (img >= n) return;
  const icap_jpeg_desc* d = descs + img;
  const int64_t* lay = layout + (int64_t)img * JPEG_LAYOUT;
  {  // the tables: 4-byte words, one per lane and step
    const uint32_t* src = reinterpret_cast<const uint32_t*>(d->huff);
    uint32_t* dst = reinterpret_cast<uint32_t*>(huff);
    for (int i = threadIdx.x; i < (int)(sizeof(huff) / 4); i += 64) dst[i] = src[i];
    zigzag[threadIdx.x] = jpeg_zigzag[threadIdx.x];
  }
  __syncthreads();
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (!jpeg_desc_ok(d)) {
    if (s == 0) atomicMax(status + img, (int32_t)JPEG_BAD_SEGMENT);
    return;
  }
  if (s >= d->nseg) return;
  const int64_t data_off = lay[0], data_len = lay[1], seg_idx = lay[2] + s;
  int rc = JPEG_BAD_SEGMENT;
  if (data_off >= 0 && data_len >= 0 && data_off <= data_bytes && data_len <= data_bytes - data_off && seg_idx >= 0 &&
      seg_idx < total_segs) {
    const icap_jpeg_segment g = segs[seg_idx];
    if (g.offset >= 0 && g.length >= 0 && g.offset <= data_len && g.length <= data_len - g.offset)
      rc = jpeg_decode_segment(d, huff, zigzag, data + data_off + g.offset, g.length, g.first_mcu, g.mcu_count,
                               coef + lay[3] * 64);
  }
  if (rc != JPEG_OK) atomicMax(status + img, (int32_t)rc);
}

// dequantise + IDCT: one lane per 8 x 8 block of any component, into the component's padded plane
__global__ __launch_bounds__(256) void jpeg_idct_kernel(int n, const icap_jpeg_desc* __restrict__ descs,
                                                        const int64_t* __restrict__ layout,
                                                        const int16_t* __restrict__ coef, uint8_t* __restrict__ planes) {
  const int img = blockIdx.y;
  if (img >= n) return;
  const icap_jpeg_desc* d = descs + img;
  const int32_t b = blockIdx.x * 256 + threadIdx.x;
  if (!jpeg_desc_ok(d) || b >= d->blocks) return;
  const int64_t work = layout[(int64_t)img * JPEG_LAYOUT + 3] * 64;
  int c = 0;
  JpegComp k = jpeg_comp(d, 0);
  if (b >= k.block0 + k.bw * k.bh) {
    c = 1 + (b - k.bw * k.bh) / (d->mcus_x * d->mcus_y);
    k = jpeg_comp(d, c);
  }
  const int32_t r = b - k.block0, by = r / k.bw, bx = r - by * k.bw;
  jpeg_idct_block(coef + work + (int64_t)b * 64, d->quant[c], planes + work + k.plane0 + ((int64_t)by * 8 * k.bw + bx) * 8,
                  (int64_t)k.bw * 8);
}

// upsample + colour: one lane per output pixel
__global__ __launch_bounds__(256) void jpeg_color_kernel(int n, const icap_jpeg_desc* __restrict__ descs,
                                                         const int64_t* __restrict__ layout,
                                                         const uint8_t* __restrict__ planes, uint8_t* __restrict__ out) {
  const int img = blockIdx.z;
  if (img >= n) return;
  const icap_jpeg_desc* d = descs + img;
  const int32_t y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
  if (!jpeg_desc_ok(d) || y >= d->height || x >= d->width) return;
  const int64_t* lay = layout + (int64_t)img * JPEG_LAYOUT;
  uint8_t rgb[3];
  jpeg_pixel(d, planes + lay[3] * 64, y, x, rgb);
  uint8_t* o = out + lay[4] + ((int64_t)y * d->width + x) * 3;
  o[0] = rgb[0];
  o[1] = rgb[1];
  o[2] = rgb[2];
}

}  // namespace icap

using namespace icap;

extern "C" int icap_jpeg_decode(int32_t n, const uint8_t* data, int64_t data_bytes, const icap_jpeg_desc* descs,
                                const icap_jpeg_segment* segs, int64_t total_segs, const int64_t* layout,
                                int32_t max_segs, int32_t max_blocks, int32_t max_h, int32_t max_w, int16_t* coef,
                                uint8_t* planes, uint8_t* out, int32_t* status, int32_t stages, void* stream) {
  ICAP_REQUIRE(n >= 0 && n <= 65535, "icap_jpeg_decode: n must be in [0, 65535]");
  if (n == 0) return ICAP_OK;
  ICAP_REQUIRE(data && descs && segs && layout && coef && planes && out && status, "icap_jpeg_decode: null pointer");
  ICAP_REQUIRE((reinterpret_cast<uintptr_t>(data) & 15) == 0 && data_bytes >= 0 && (data_bytes & 15) == 0,
               "icap_jpeg_decode: data must be 16-byte aligned and data_bytes a multiple of 16");
  ICAP_REQUIRE((reinterpret_cast<uintptr_t>(descs) & 3) == 0 && (reinterpret_cast<uintptr_t>(segs) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(layout) & 7) == 0 && (reinterpret_cast<uintptr_t>(coef) & 1) == 0,
               "icap_jpeg_decode: misaligned table");
  ICAP_REQUIRE(total_segs >= 1 && max_segs >= 1 && max_blocks >= 1 && max_h >= 1 && max_w >= 1 &&
                   max_h <= ICAP_JPEG_MAX_DIM && max_w <= ICAP_JPEG_MAX_DIM,
               "icap_jpeg_decode: bad sizes");
  ICAP_REQUIRE(stages >= 1 && stages <= ICAP_JPEG_STAGE_ALL, "icap_jpeg_decode: stages must be a mask of ICAP_JPEG_STAGE_*");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int rc = ICAP_OK;
  if (stages & ICAP_JPEG_STAGE_ENTROPY) {
    hipLaunchKernelGGL(jpeg_status_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, status);
    rc = check_launch("icap_jpeg_decode(status)");
    if (rc != ICAP_OK) return rc;
    const dim3 ge((unsigned)((max_segs + 63) / 64), (unsigned)n);
    hipLaunchKernelGGL(jpeg_entropy_kernel, ge, dim3(64), 0, s, n, data, data_bytes, descs, segs, total_segs, layout,
                       coef, status);
    rc = check_launch("icap_jpeg_decode(entropy)");
    if (rc != ICAP_OK) return rc;
  }
  if (stages & ICAP_JPEG_STAGE_IDCT) {
    const dim3 gi((unsigned)((max_blocks + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(jpeg_idct_kernel, gi, dim3(256), 0, s, n, descs, layout, coef, planes);
    rc = check_launch("icap_jpeg_decode(idct)");
    if (rc != ICAP_OK) return rc;
  }
  if (stages & ICAP_JPEG_STAGE_COLOUR) {
    const dim3 gc((unsigned)((max_w + 255) / 256), (unsigned)max_h, (unsigned)n);
    hipLaunchKernelGGL(jpeg_color_kernel, gc, dim3(256), 0, s, n, descs, layout, planes, out);
    rc = check_launch("icap_jpeg_decode(colour)");
  }
  return rc;
}
