"""Baseline JPEG decode on the device (csrc/jpeg.hip) against Pillow, uint8 for uint8: the whole grid file by file, 70
mixed files in one call, one image in many restart segments, a 480 x 640 file, the call replayed from a graph, and
extraction with device decode against host decode. Only valid files go to the GPU (malformed input: test_jpeg_cpu.py,
on the host build)."""

import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases as jc
from icap import jpeg, ops

pytestmark = pytest.mark.gpu


def test_grid_file_by_file(dev):
    """Every one of the 288 grid files through decode_jpeg equals Pillow's RGB bytes."""
    wrong = []
    for name, data, ref in jc.grid():
        out = jpeg.decode_jpeg(data, dev)
        assert out.dtype == torch.uint8 and tuple(out.shape) == ref.shape, name
        if not np.array_equal(out.cpu().numpy(), ref):
            wrong.append(name)
    assert not wrong, wrong


def test_seventy_mixed_files_in_one_call(dev):
    """More files than a wave has lanes, of different sizes, tables and samplings, in one icap_jpeg_decode: every
    image equals Pillow (and so its single-file result), every status is 0."""
    grid = jc.grid()
    picks = [grid[(i * 37) % len(grid)] for i in range(70)]  # 37 is coprime to 288: 70 different files
    assert len({p[0] for p in picks}) == 70 and len({p[0].split("-", 2)[2] for p in picks}) == len(jc.ENCODINGS)
    images, status = jpeg.DeviceJpegDecoder(dev).decode_files([p[1] for p in picks])
    assert status.cpu().tolist() == [0] * 70
    wrong = [p[0] for p, im in zip(picks, images) if not np.array_equal(im.cpu().numpy(), p[2])]
    assert not wrong, wrong
    one = jpeg.decode_jpeg(picks[5][1], dev)
    assert torch.equal(one, images[5])


def test_many_segments_in_one_image(dev):
    """96 x 80 at 4:2:0 with a restart marker after every MCU: 30 segments, 30 lanes for one image."""
    data = jc.big_file(96, 80, restart_marker_blocks=1)
    assert jpeg.parse_jpeg(data).nseg == 30
    assert np.array_equal(jpeg.decode_jpeg(data, dev).cpu().numpy(), jc.reference(data))


def test_480_by_640(dev):
    """The real block grid (7200 blocks) and the offsets that go with it; twice in one call, so that the second
    image's offsets are large too."""
    data = jc.big_file(480, 640)
    d = jpeg.parse_jpeg(data)
    assert (d.height, d.width, d.hs, d.vs, d.blocks) == (480, 640, 2, 2, 7200)
    ref = jc.reference(data)
    images, status = jpeg.DeviceJpegDecoder(dev).decode_files([data, data])
    assert status.cpu().tolist() == [0, 0]
    assert np.array_equal(images[0].cpu().numpy(), ref) and np.array_equal(images[1].cpu().numpy(), ref)


def test_graph_replay_equals_eager(dev):
    """icap_jpeg_decode allocates and synchronises nothing: captured once and replayed twice (the output cleared in
    between) it gives the eager bytes."""
    grid = jc.grid()
    files = [grid[i][1] for i in (2, 50, 100, 150, 200, 250)] + [jc.big_file(96, 80, restart_marker_blocks=1)]
    items = [(f, jpeg.parse_jpeg(f)) for f in files]
    batch = jpeg.pack_batch(items)
    dec = jpeg.DeviceJpegDecoder(dev)
    toc = batch.toc.tolist()
    blob = dec.upload(batch)
    blocks = toc[jpeg.TOC_TOTAL_BLOCKS]
    coef = torch.empty(blocks * 64, dtype=torch.int16, device=dev)
    planes = torch.empty(blocks * 64, dtype=torch.uint8, device=dev)
    out = torch.zeros(toc[jpeg.TOC_OUT_BYTES], dtype=torch.uint8, device=dev)
    status = torch.empty(len(files), dtype=torch.int32, device=dev)
    eager, st = dec.decode(batch)
    torch.cuda.synchronize(dev)
    assert st.cpu().tolist() == [0] * len(files)
    want = np.concatenate([jc.reference(f).reshape(-1) for f in files])
    assert np.array_equal(eager.cpu().numpy(), want)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.jpeg_decode(toc, blob, coef, planes, out, status)  # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        ops.jpeg_decode(toc, blob, coef, planes, out, status)
    for _ in range(2):
        out.zero_()
        status.fill_(7)
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, eager) and status.cpu().tolist() == [0] * len(files)


def test_extraction_with_device_decode_equals_host_decode(dev, tmp_path):
    """extract_directory over 12 small JPEGs, a progressive JPEG and a PNG with the B/32 CLIP tower: device_decode
    gives the host path's filenames, pixel_values and embeddings, bit for bit."""
    from icap.clip import CLIPVisionTower, DeviceCLIPProcessor
    from icap.images import extract_directory

    d = tmp_path / "images"
    d.mkdir()
    encs = list(jc.ENCODINGS)
    for k in range(12):
        h, w = [(33, 47), (48, 64), (40, 56), (64, 48)][k % 4]
        arr = jc.content(jc.CONTENTS[k % 3], h, w, seed=k)
        (d / f"img_{k:02d}.jpg").write_bytes(jc.encode(arr, encs[k % len(encs)]))
    buf = io.BytesIO()
    Image.fromarray(jc.content("noise", 40, 40, seed=99)).save(buf, format="JPEG", progressive=True)
    (d / "prog.jpg").write_bytes(buf.getvalue())
    Image.fromarray(jc.content("gradient", 36, 52)).save(d / "pic.png")
    tower = CLIPVisionTower.random_init(seed=0).to(dev)
    proc = DeviceCLIPProcessor(device=dev)
    got = {}
    for mode in (False, True):
        seen = []

        def embed(px, _seen=seen):
            _seen.append(px.clone())
            return tower.embed(px)

        out = tmp_path / f"clip_{int(mode)}.pt"
        n = extract_directory(str(d), str(out), embed, proc, tower.config.projection_dim, batch_size=5, num_workers=2,
                              device=dev, device_decode=mode)
        assert n == 14
        saved = torch.load(str(out), weights_only=True)
        got[mode] = (saved["filenames"], torch.cat(seen).cpu(), saved["embeddings"])
    assert got[True][0] == got[False][0] and len(got[True][0]) == 14
    assert torch.equal(got[True][1], got[False][1])
    assert torch.equal(got[True][2], got[False][2])
