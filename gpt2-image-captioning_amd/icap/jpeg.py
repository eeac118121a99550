"""Baseline JPEG decode on the device (csrc/jpeg.hip): the parser decides, the kernels decode, Pillow takes the rest.

parse_jpeg runs on the host (csrc/jpeg_host.cpp through libicap_jpeg_host.so, which links no HIP library, so a
DataLoader worker that parses opens no device) and returns a descriptor for the files the kernels decode: SOF0, 8 bit,
grayscale or YCbCr at 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, with or without restart markers. Everything else
is None, and its caller decodes it with PIL as before. pack_batch lays a batch out as one host buffer (layout table,
descriptors, segments, file bytes), DeviceJpegDecoder.decode copies it in one piece and runs icap_jpeg_decode, which
writes the packed RGB uint8 HWC buffer ops.clip_preprocess_packed reads. The pixels equal
np.asarray(Image.open(f).convert("RGB")) byte for byte.
"""

from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

DESC_BYTES = C.sizeof(L.JpegDesc)
SEG_BYTES = C.sizeof(L.JpegSegment)
LAYOUT_COLS = 5  # data_off, data_len, seg_off, work_off, out_off (include/icap.h icap_jpeg_decode)
# toc entries of a JpegBatch
(TOC_N, TOC_LAYOUT, TOC_DESCS, TOC_SEGS, TOC_DATA, TOC_DATA_BYTES, TOC_TOTAL_SEGS, TOC_MAX_SEGS, TOC_MAX_BLOCKS,
 TOC_MAX_H, TOC_MAX_W, TOC_TOTAL_BLOCKS, TOC_OUT_BYTES, TOC_LEN) = range(14)


class JpegDescriptor:
    """What parse_jpeg found in one file: its size and the bytes of the icap_jpeg_desc and icap_jpeg_segment[nseg]
    the kernels read. Plain attributes, so a worker hands it over like any other sample."""

    __slots__ = ("height", "width", "ncomp", "hs", "vs", "restart_interval", "nseg", "blocks", "desc", "segs")

    def __init__(self, d: L.JpegDesc, segs: bytes) -> None:
        self.height, self.width, self.ncomp, self.hs, self.vs = d.height, d.width, d.ncomp, d.hs, d.vs
        self.restart_interval, self.nseg, self.blocks = d.restart_interval, d.nseg, d.blocks
        self.desc = bytes(d)
        self.segs = segs

    def __getstate__(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __setstate__(self, state) -> None:
        for k, v in zip(self.__slots__, state):
            setattr(self, k, v)


def parse_jpeg(data, lib=None) -> Optional[JpegDescriptor]:
    """The descriptor of a baseline JPEG the device path decodes, or None (decode it with PIL). Host only."""
    lib = lib or L.load_jpeg_host()
    data = bytes(data)
    d = L.JpegDesc()
    rc = lib.icap_jpeg_parse(data, len(data), C.addressof(d), None, 0)
    if rc == L.JPEG_UNSUPPORTED:
        return None
    if rc != L.JPEG_OK:
        raise L.IcapError(f"icap_jpeg_parse failed ({rc})")
    segs = (L.JpegSegment * d.nseg)()
    rc = lib.icap_jpeg_parse(data, len(data), C.addressof(d), C.addressof(segs), d.nseg)
    if rc != L.JPEG_OK:
        raise L.IcapError(f"icap_jpeg_parse failed ({rc})")
    return JpegDescriptor(d, bytes(segs))


def decode_jpeg_host(data, desc: Optional[JpegDescriptor] = None, lib=None) -> Tuple[Optional[np.ndarray], int]:
    """(RGB uint8 [H, W, 3] or None, status) from the host decoder, which is built from the kernels' own inline
    functions. For tests: the product decodes on the device or with PIL."""
    lib = lib or L.load_jpeg_host()
    data = bytes(data)
    desc = desc or parse_jpeg(data, lib)
    if desc is None:
        return None, L.JPEG_UNSUPPORTED
    out = np.empty((desc.height, desc.width, 3), dtype=np.uint8)
    st = C.c_int32(0)
    rc = lib.icap_jpeg_decode_host(data, len(data), desc.desc, desc.segs, out.ctypes.data, C.addressof(st))
    if rc != 0:
        raise L.IcapError(f"icap_jpeg_decode_host failed ({rc})")
    return (out if st.value == 0 else None), st.value


class JpegBatch(NamedTuple):
    """One batch for the device: `blob` (uint8, host) holds the layout table, the descriptors, the segments and the
    files' bytes back to back, each part 16-byte aligned, at the offsets `toc` (int64 [TOC_LEN]) names. The images
    decode to out_off of a packed RGB buffer of toc[TOC_OUT_BYTES] bytes, which also has room for the images of the
    batch that are not in the blob (pack_batch's `slots`)."""

    blob: torch.Tensor
    toc: torch.Tensor


def _align16(n: int) -> int:
    return (n + 15) & ~15


def pack_batch(items: Sequence[Tuple[bytes, JpegDescriptor]], out_offsets: Optional[Sequence[int]] = None,
               out_bytes: Optional[int] = None) -> JpegBatch:
    """Pack (file bytes, descriptor) pairs. out_offsets: each image's byte offset in the packed RGB buffer (default:
    back to back), out_bytes: that buffer's size (default: what the images need)."""
    n = len(items)
    layout = np.zeros((n, LAYOUT_COLS), dtype=np.int64)
    data_off = seg_off = work_off = out_off = 0
    for i, (data, d) in enumerate(items):
        layout[i] = (data_off, len(data), seg_off, work_off, out_off if out_offsets is None else out_offsets[i])
        data_off += _align16(len(data))
        seg_off += d.nseg
        work_off += d.blocks
        out_off += d.height * d.width * 3
    o_layout = 0
    o_descs = _align16(o_layout + layout.nbytes)
    o_segs = _align16(o_descs + n * DESC_BYTES)
    o_data = _align16(o_segs + seg_off * SEG_BYTES)
    blob = np.zeros(o_data + data_off, dtype=np.uint8)
    blob[o_layout:o_layout + layout.nbytes] = layout.reshape(-1).view(np.uint8)
    for i, (data, d) in enumerate(items):
        blob[o_descs + i * DESC_BYTES:o_descs + (i + 1) * DESC_BYTES] = np.frombuffer(d.desc, dtype=np.uint8)
        so = o_segs + int(layout[i, 2]) * SEG_BYTES
        blob[so:so + len(d.segs)] = np.frombuffer(d.segs, dtype=np.uint8)
        do = o_data + int(layout[i, 0])
        blob[do:do + len(data)] = np.frombuffer(data, dtype=np.uint8)
    toc = [0] * TOC_LEN
    toc[TOC_N], toc[TOC_LAYOUT], toc[TOC_DESCS], toc[TOC_SEGS], toc[TOC_DATA] = n, o_layout, o_descs, o_segs, o_data
    toc[TOC_DATA_BYTES], toc[TOC_TOTAL_SEGS], toc[TOC_TOTAL_BLOCKS] = data_off, seg_off, work_off
    toc[TOC_MAX_SEGS] = max((d.nseg for _, d in items), default=0)
    toc[TOC_MAX_BLOCKS] = max((d.blocks for _, d in items), default=0)
    toc[TOC_MAX_H] = max((d.height for _, d in items), default=0)
    toc[TOC_MAX_W] = max((d.width for _, d in items), default=0)
    toc[TOC_OUT_BYTES] = out_off if out_bytes is None else out_bytes
    return JpegBatch(torch.from_numpy(blob), torch.tensor(toc, dtype=torch.int64))


class DeviceJpegDecoder:
    """Decodes JpegBatches on `device`. decode() makes one host-to-device copy and one icap_jpeg_decode; nothing in
    it waits for the device, so the caller reads `status` where it synchronises anyway."""

    def __init__(self, device) -> None:
        self.device = torch.device(device)
        L.require_device(self.device)

    def upload(self, batch: JpegBatch) -> torch.Tensor:
        return batch.blob.to(self.device, non_blocking=True)

    def decode(self, batch: JpegBatch, blob_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               coef: Optional[torch.Tensor] = None, planes: Optional[torch.Tensor] = None,
               status: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(packed RGB uint8 [toc[TOC_OUT_BYTES]] on the device, status int32 [n]: 0, or why that image's entropy
        data did not decode — its pixels are then unspecified and the caller decodes the file with PIL). With every
        buffer given (blob_dev from upload(); coef int16 and planes uint8 of total blocks x 64) the call allocates
        nothing and can be captured into a graph."""
        from . import ops

        toc = [int(v) for v in batch.toc.tolist()]
        n, blocks = toc[TOC_N], toc[TOC_TOTAL_BLOCKS]
        dev = self.device
        blob_dev = self.upload(batch) if blob_dev is None else blob_dev
        out = torch.empty(toc[TOC_OUT_BYTES], dtype=torch.uint8, device=dev) if out is None else out
        coef = torch.empty(blocks * 64, dtype=torch.int16, device=dev) if coef is None else coef
        planes = torch.empty(blocks * 64, dtype=torch.uint8, device=dev) if planes is None else planes
        status = torch.empty(n, dtype=torch.int32, device=dev) if status is None else status
        if out.numel() < toc[TOC_OUT_BYTES] or coef.numel() < blocks * 64 or planes.numel() < blocks * 64:
            raise L.IcapError("DeviceJpegDecoder.decode: a buffer is smaller than the batch needs")
        ops.jpeg_decode(toc, blob_dev, coef, planes, out, status)
        return out, status

    def decode_files(self, files: Sequence[bytes]) -> Tuple[List[torch.Tensor], torch.Tensor]:
        """Each file's RGB uint8 [H, W, 3] (views of one device buffer) and the status words, from one call. Every
        file must be one parse_jpeg accepts."""
        items = []
        for f in files:
            d = parse_jpeg(f)
            if d is None:
                raise L.IcapError("decode_files: not a baseline JPEG the device path decodes (use PIL)")
            items.append((bytes(f), d))
        batch = pack_batch(items)
        out, status = self.decode(batch)
        images, off = [], 0
        for _, d in items:
            nb = d.height * d.width * 3
            images.append(out[off:off + nb].view(d.height, d.width, 3))
            off += nb
        return images, status


def decode_jpeg(data, device) -> torch.Tensor:
    """One baseline JPEG -> RGB uint8 [H, W, 3] on `device`, equal to Pillow's decode. Raises for a file the device
    path does not take or whose entropy data is malformed (there is no fallback here: the extraction loop, which
    has one, is icap.images.extract_directory(device_decode=True))."""
    images, status = DeviceJpegDecoder(device).decode_files([data])
    st = int(status[0].item())
    if st != 0:
        raise L.IcapError(f"decode_jpeg: malformed entropy data (status {st})")
    return images[0]
