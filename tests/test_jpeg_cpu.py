"""The host side of the device JPEG decode, without a GPU: the host decoder (built from the kernels' own inline
functions, csrc/jpeg_common.h) against Pillow over the whole grid, uint8 for uint8; what the parser accepts and what
it leaves to PIL; the stand-alone jpeg_check program over every truncation and 200 bit flips of one file; the
loader's decode="device" samples and collate."""

import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases as jc
from icap import _lib, jpeg
from icap.images import ImageDirectoryDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpt2-image-captioning_amd", "csrc")


def test_host_decoder_equals_pillow_over_the_grid():
    """All 288 files (12 sizes x 3 contents x 8 encodings): parsed, decoded, equal to Pillow's RGB bytes."""
    grid = jc.grid()
    assert len(grid) == 288
    wrong = []
    for name, data, ref in grid:
        desc = jpeg.parse_jpeg(data)
        assert desc is not None, name
        assert (desc.height, desc.width) == ref.shape[:2], name
        out, status = jpeg.decode_jpeg_host(data, desc)
        if status != 0 or not np.array_equal(out, ref):
            wrong.append((name, status))
    assert not wrong, wrong


def test_descriptor_fields():
    """Sampling, restart interval and segment count as the encodings imply (33 x 47: 3 x 3 MCUs at 4:2:0)."""
    arr = jc.content("noise", 33, 47)
    d = jpeg.parse_jpeg(jc.encode(arr, "q30-420"))
    assert (d.ncomp, d.hs, d.vs, d.restart_interval, d.nseg, d.blocks) == (3, 2, 2, 0, 1, 9 * 6)
    d = jpeg.parse_jpeg(jc.encode(arr, "q90-420-rst-blocks1"))
    assert (d.hs, d.vs, d.restart_interval, d.nseg) == (2, 2, 1, 9)
    d = jpeg.parse_jpeg(jc.encode(arr, "q85-422-rst-rows1"))  # 3 MCUs a row, 5 rows of 8 lines
    assert (d.hs, d.vs, d.restart_interval, d.nseg, d.blocks) == (2, 1, 3, 5, 15 * 4)
    d = jpeg.parse_jpeg(jc.encode(arr, "q100-444"))
    assert (d.hs, d.vs, d.blocks) == (1, 1, 6 * 5 * 3)
    d = jpeg.parse_jpeg(jc.encode(arr, "gray-q80"))
    assert (d.ncomp, d.hs, d.vs, d.blocks) == (1, 1, 1, 6 * 5)
    segs = (_lib.JpegSegment * d.nseg).from_buffer_copy(d.segs)
    assert segs[0].first_mcu == 0 and segs[0].mcu_count == 30 and segs[0].length > 0


def _save(im, **kw) -> bytes:
    buf = io.BytesIO()
    im.save(buf, **kw)
    return buf.getvalue()


def _baseline() -> bytes:
    return jc.encode(jc.content("noise", 13, 17), "q30-420")


def _edit_sampling(data: bytes) -> bytes:
    i = data.index(b"\xff\xc0")
    b = bytearray(data)
    assert b[i + 11] == 0x22  # marker 2, length 2, precision 1, height 2, width 2, ncomp 1, id 1 -> luma h << 4 | v
    b[i + 11] = 0x12
    return bytes(b)


def _edit_length(data: bytes) -> bytes:
    i = data.index(b"\xff\xdb")
    b = bytearray(data)
    b[i + 2:i + 4] = b"\xff\xff"
    return bytes(b)


REJECTS = {
    "progressive": lambda: _save(Image.fromarray(jc.content("noise", 13, 17)), format="JPEG", progressive=True),
    "cmyk": lambda: _save(Image.fromarray(jc.content("noise", 13, 17)).convert("CMYK"), format="JPEG"),
    "rgb-kept": lambda: _save(Image.fromarray(jc.content("noise", 13, 17)), format="JPEG", keep_rgb=True),
    "sampling-1x2": lambda: _edit_sampling(_baseline()),
    "length-past-the-end": lambda: _edit_length(_baseline()),
    "png": lambda: _save(Image.fromarray(jc.content("noise", 13, 17)), format="PNG"),
    "empty": lambda: b"",
    "no-eoi": lambda: _baseline()[:-2],
}


@pytest.mark.parametrize("case", list(REJECTS))
def test_parser_leaves_it_to_pil(case):
    data = REJECTS[case]()
    assert jpeg.parse_jpeg(data) is None
    assert jpeg.decode_jpeg_host(data) == (None, _lib.JPEG_UNSUPPORTED)


def test_rgb_kept_file_is_what_it_claims():
    """The "rgb-kept" case is the RGB file without a colour transform (Pillow keep_rgb: an Adobe APP14 marker, ids
    'R','G','B'), which Pillow reads back as stored; and the unedited baseline file is accepted."""
    data = REJECTS["rgb-kept"]()
    assert b"Adobe" in data and b"JFIF" not in data[:32]
    assert jpeg.parse_jpeg(_baseline()) is not None


def test_adobe_marker_alone_is_rejected():
    """An Adobe APP14 segment spliced into an accepted file: rejected for the marker itself."""
    data = _baseline()
    i = data.index(b"\xff\xdb")
    app14 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    assert jpeg.parse_jpeg(data[:i] + app14 + data[i:]) is None
    com = b"\xff\xfe\x00\x07hello"
    assert jpeg.parse_jpeg(data[:i] + com + data[i:]) is not None


def _fnv1a64(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for v in b:
        h = ((h ^ v) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("enc", ["q30-420", "q90-420-rst-blocks1"])
def test_jpeg_check_truncations_and_bit_flips(tmp_path, enc):
    """The stand-alone checker (host compiler, its own main, nothing loaded into Python; built here without sanitizer
    flags, `make SAN=1 jpeg_check` is the by-hand variant) on one 13 x 17 4:2:0 file: the intact file decodes to
    Pillow's pixels; each of the len(file) truncations and each of 200 single-bit flips of the entropy data ends in
    pixels or an error, and the program exits 0."""
    exe = str(tmp_path / "jpeg_check")
    subprocess.check_call(["make", "-s", "-C", CSRC, "jpeg_check", f"JPEG_CHECK={exe}"])
    data = jc.encode(jc.content("noise", 13, 17), enc)
    path = tmp_path / "in.jpg"
    path.write_bytes(data)
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[0] == f"intact {_fnv1a64(jc.reference(data).tobytes()):016x} 13 17", out
    t = out[1].split()
    assert t[0] == "truncations" and int(t[1]) == len(data) and int(t[3]) + int(t[5]) == len(data), out
    assert int(t[3]) == 0, out  # no truncation has an EOI: the parser leaves every one to PIL
    f = out[2].split()
    assert f[0] == "flips" and int(f[1]) == 200 and int(f[3]) + int(f[5]) == 200 and int(f[3]) > 0, out


def test_host_library_links_no_hip_runtime():
    """Loader workers parse through libicap_jpeg_host.so; it names no HIP library, so loading it opens no device."""
    blob = open(_lib.JPEG_HOST_LIB_PATH, "rb").read()
    assert b"libamdhip64" not in blob and b"libhsa-runtime64" not in blob
    assert b"libamdhip64" in open(_lib.LIB_PATH, "rb").read()
    lib = _lib.load_jpeg_host()
    assert all(hasattr(lib, n) for n in _lib.JPEG_HOST_FUNCTIONS) and not hasattr(lib, "icap_jpeg_decode")


@pytest.mark.parametrize("struct,cname", [(_lib.JpegHuff, "icap_jpeg_huff"), (_lib.JpegDesc, "icap_jpeg_desc"),
                                          (_lib.JpegSegment, "icap_jpeg_segment")])
def test_jpeg_struct_layout_matches_header(struct, cname, tmp_path):
    fields = [f[0] for f in struct._fields_]
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "icap.h"', "int main(void){",
            f'printf("%zu\\n", sizeof({cname}));']
    prog += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    prog += ["return 0;}"]
    (tmp_path / "t.c").write_text("\n".join(prog))
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", exe])
    vals = [int(x) for x in subprocess.check_output([exe]).split()]
    assert vals[0] == C.sizeof(struct)
    for f, off in zip(fields, vals[1:]):
        assert getattr(struct, f).offset == off, f


def test_device_decode_dataset_and_collate(tmp_path):
    """A directory of baseline JPEGs, one progressive JPEG and one PNG: decode="device" hands the baseline files over
    undecoded with their descriptors, and the other two as the pixels the host path gives; the collate packs one
    compressed buffer with its tables, whose files decode (host decoder) to the host path's pixels."""
    encs = ["q30-420", "q95-422", "q100-444", "q90-420-rst-blocks1", "gray-q80"]
    for k, enc in enumerate(encs):
        (tmp_path / f"b{k}.jpg").write_bytes(jc.encode(jc.content("noise", 33, 47, seed=k), enc))
    (tmp_path / "prog.jpg").write_bytes(REJECTS["progressive"]())
    (tmp_path / "pic.png").write_bytes(REJECTS["png"]())
    host = ImageDirectoryDataset(str(tmp_path))
    dev = ImageDirectoryDataset(str(tmp_path), decode="device")
    assert host.filenames == dev.filenames and len(dev) == 7
    samples = [dev[i] for i in range(len(dev))]
    names, sizes, blob, toc, fallback, fb_index = ImageDirectoryDataset.device_collate(samples)
    assert names == host.filenames
    want_fb = [i for i, n in enumerate(names) if n in ("prog.jpg", "pic.png")]
    assert fb_index.tolist() == want_fb
    pixels = [host[i][1] for i in range(len(host))]
    assert sizes.tolist() == [list(p.shape[:2]) for p in pixels]
    assert torch.equal(fallback, torch.cat([pixels[i].reshape(-1) for i in want_fb]))
    toc = toc.tolist()
    jp = [i for i in range(len(names)) if i not in want_fb]
    assert toc[jpeg.TOC_N] == len(jp) == 5 and blob.dtype == torch.uint8
    assert toc[jpeg.TOC_OUT_BYTES] == sum(p.numel() for p in pixels)
    raw = blob.numpy()
    lo = toc[jpeg.TOC_LAYOUT]
    layout = raw[lo:lo + len(jp) * jpeg.LAYOUT_COLS * 8].view(np.int64).reshape(-1, jpeg.LAYOUT_COLS)
    offs = np.concatenate([[0], np.cumsum([p.numel() for p in pixels])])
    for k, i in enumerate(jp):
        data_off, data_len, seg_off, work_off, out_off = layout[k].tolist()
        assert data_off % 16 == 0 and out_off == offs[i]
        data = raw[toc[jpeg.TOC_DATA] + data_off:toc[jpeg.TOC_DATA] + data_off + data_len].tobytes()
        assert data == (tmp_path / names[i]).read_bytes()
        d = _lib.JpegDesc.from_buffer_copy(raw[toc[jpeg.TOC_DESCS] + k * jpeg.DESC_BYTES:][:jpeg.DESC_BYTES].tobytes())
        assert (d.height, d.width) == tuple(pixels[i].shape[:2])
        out, status = jpeg.decode_jpeg_host(data)
        assert status == 0 and np.array_equal(out, pixels[i].numpy())
    assert toc[jpeg.TOC_TOTAL_SEGS] == 1 + 1 + 1 + 9 + 1 and toc[jpeg.TOC_MAX_SEGS] == 9
    with pytest.raises(ValueError):
        ImageDirectoryDataset(str(tmp_path), decode="gpu")
