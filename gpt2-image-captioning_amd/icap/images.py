"""Image-directory loading shared by the embedding extractors (src/utils.py:119-173 ImageDirectoryDataset and the
DataLoader loops of src/embeddings/clip.py:79-149 / vit.py:80-137).

The reference decodes JPEGs in `num_workers` DataLoader processes and preprocesses each batch on the host; here the
workers decode to RGB uint8 tensors (handed over through shared memory) and the batch goes to the tower's processor
(the device one runs resize / crop / normalise as HIP kernels). Filenames come in os.listdir order filtered by
extension, exactly as the reference lists them, so the saved .pt rows line up with the reference's.
"""

from __future__ import annotations

import os
from typing import Optional, Callable, List, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

IMAGE_EXTS = {".jpg", ".jpeg", ".png", ".webp"}  # src/utils.py:131


class ImageDirectoryDataset(Dataset):
    """src/utils.py:119-173: (filename, image) per file of a flat directory; images as RGB uint8 [H, W, 3]."""

    def __init__(self, directory: str, decode: str = "host") -> None:
        """decode="device": a baseline JPEG the device path takes (icap.jpeg.parse_jpeg) is handed over as its file
        bytes and descriptor, undecoded; every other file is decoded by PIL as with "host"."""
        if decode not in ("host", "device"):
            raise ValueError(f'decode must be "host" or "device", got {decode!r}')
        self.directory = directory
        self.decode = decode
        self.filenames = [f for f in os.listdir(directory) if os.path.splitext(f)[1].lower() in IMAGE_EXTS]

    def __len__(self) -> int:
        return len(self.filenames)

    def __getitem__(self, idx: int) -> Tuple[str, torch.Tensor]:
        """(filename, RGB uint8 [H, W, 3] tensor): a tensor, not a numpy array, so a DataLoader worker hands the
        decoded pixels over through shared memory instead of pickling ~1 MB per image through a pipe."""
        from PIL import Image

        name = self.filenames[idx]
        path = os.path.join(self.directory, name)
        if self.decode == "device":
            # parse only: libicap_jpeg_host.so links no HIP library, so the worker opens no device
            from .jpeg import parse_jpeg

            with open(path, "rb") as f:
                data = f.read()
            desc = parse_jpeg(data)
            if desc is not None:
                return name, (data, desc)
        with Image.open(path) as im:
            return name, torch.from_numpy(np.asarray(im.convert("RGB")).copy())

    @staticmethod
    def collate_fn(batch) -> Tuple[List[str], List[torch.Tensor]]:
        names, images = zip(*batch)
        return list(names), list(images)

    @staticmethod
    def packed_collate(batch) -> Tuple[List[str], torch.Tensor, torch.Tensor]:
        """(names, uint8 [sum H*W*3] with the images back to back, int64 [n, 2] (H, W)): the packing runs in the
        worker, so the main process receives one shared-memory buffer per batch (not one per image), which the
        DataLoader's pin-memory thread pins for an asynchronous host-to-device copy."""
        names, images = zip(*batch)
        sizes = torch.tensor([im.shape[:2] for im in images], dtype=torch.int64).reshape(-1, 2)
        packed = torch.cat([im.reshape(-1) for im in images]) if images else torch.empty(0, dtype=torch.uint8)
        return list(names), packed, sizes


    @staticmethod
    def device_collate(batch):
        """decode="device" samples -> (names, sizes int64 [n, 2], blob, toc, fallback, fb_index): `blob` / `toc` are
        icap.jpeg.pack_batch of the batch's undecoded JPEGs (one compressed buffer with its descriptor table),
        laid out so that image i decodes to its place in the packed RGB buffer of the whole batch; `fallback` holds
        the PIL-decoded pixels of the other images back to back and fb_index int64 [k] says which images they are."""
        from .jpeg import pack_batch

        names, samples = zip(*batch) if batch else ((), ())
        sizes, offs, off = [], [], 0
        for s in samples:
            h, w = (s[1].height, s[1].width) if isinstance(s, tuple) else s.shape[:2]
            sizes.append((h, w))
            offs.append(off)
            off += h * w * 3
        jp = [i for i, s in enumerate(samples) if isinstance(s, tuple)]
        fb = [i for i, s in enumerate(samples) if not isinstance(s, tuple)]
        jb = pack_batch([samples[i] for i in jp], [offs[i] for i in jp], off)
        fallback = torch.cat([samples[i].reshape(-1) for i in fb]) if fb else torch.empty(0, dtype=torch.uint8)
        return (list(names), torch.tensor(sizes, dtype=torch.int64).reshape(-1, 2), jb.blob, jb.toc, fallback,
                torch.tensor(fb, dtype=torch.int64))


def _decode_batch_on_device(decoder, batch):
    """One device_collate batch -> (packed RGB on the device, sizes, status, the batch positions of the images the
    device decoded): one host-to-device copy of the compressed batch, one icap_jpeg_decode, then the PIL-decoded
    images copied into their slots. Nothing here waits for the device; `status` is read at the end of the loop."""
    from .jpeg import JpegBatch

    names, sizes, blob, toc, fallback, fb_index = batch
    sizes = sizes.tolist()
    fb = fb_index.tolist()
    out, status = decoder.decode(JpegBatch(blob, toc))
    if fb:
        fb_dev = fallback.to(decoder.device, non_blocking=True)
        offs, off = [], 0
        for h, w in sizes:
            offs.append(off)
            off += h * w * 3
        src = 0
        for i in fb:
            nb = sizes[i][0] * sizes[i][1] * 3
            out[offs[i]:offs[i] + nb].copy_(fb_dev[src:src + nb])
            src += nb
    skip = set(fb)
    return out, sizes, status, [i for i in range(len(names)) if i not in skip]


def _worker_context(dev):
    """The DataLoader workers' start method: never fork them from a process that has initialised HIP. A forked
    worker shares the parent's pages copy-on-write, HIP runtime threads and locks included, and the parent then DMAs
    from pageable host memory that the child maps too (round-5 suite hang, DESIGN.md "Extraction loader"); the
    forkserver starts from a fresh interpreter (no HIP state) and forks the workers from there. Before any GPU call
    (CPU extraction, tests) plain fork is kept: it is the cheapest start."""
    if dev is not None and dev.type == "cuda" and torch.cuda.is_initialized():
        import multiprocessing as mp

        ctx = mp.get_context("forkserver")
        ctx.set_forkserver_preload(["torch", "PIL.Image", "numpy"])
        return ctx
    return None


@torch.no_grad()
def _worker_init(_):
    """DataLoader worker: one intra-op thread (PIL decodes single-threaded; torch's default of one thread per core
    in each of N workers oversubscribes the host N-fold)."""
    torch.set_num_threads(1)


def extract_directory(image_dir: str, output_path: str, embed: Callable, processor, out_dim: int,
                      batch_size: int = 32, num_workers: int = 4, device=None, feature: Optional[str] = None,
                      stats: Optional[dict] = None, device_decode: bool = False) -> int:
    """Every image of `image_dir` -> {"filenames": [...], "embeddings": fp32 [N, out_dim]} saved with torch.save
    (src/embeddings/clip.py:147-149 format). `embed(pixel_values)` returns L2-normalised features on the device.
    feature: an extra "feature" string naming what the embeddings are (readers that index "filenames" /
    "embeddings", src/dataset.py:127-137, ignore it). Returns the number of images.
    stats: filled with the main process's wall-time split (s): first_batch (worker start-up + first decode),
    wait (blocked on the loader after the first batch), issue (preprocess + embed launches), final (the one copy
    back + torch.save) — what bounds the loop (bench.py clip_extraction).
    device_decode (with a processor that has preprocess_packed, on a GPU): the workers hand over the compressed bytes
    of the baseline JPEGs icap.jpeg.parse_jpeg accepts and the device decodes them (csrc/jpeg.hip, Pillow's pixels
    byte for byte); every other file is decoded by PIL in the worker as before. The filename order and the saved
    file are those of the default path. An image whose entropy data does not decode (a status word, read once after
    the loop) is decoded again with PIL and its row replaced."""
    import time

    t_start = time.perf_counter()
    packed = hasattr(processor, "preprocess_packed")  # the device processor: one packed, pinned buffer per batch
    dev = torch.device(device) if device is not None else None
    pin = packed and dev is not None and dev.type == "cuda"
    device_decode = bool(device_decode) and pin
    ds = ImageDirectoryDataset(image_dir, decode="device" if device_decode else "host")
    decoder = None
    if device_decode:
        from .jpeg import DeviceJpegDecoder

        decoder = DeviceJpegDecoder(dev)
    collate = (ImageDirectoryDataset.device_collate if device_decode else
               ImageDirectoryDataset.packed_collate if packed else ImageDirectoryDataset.collate_fn)
    dl = DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=num_workers, pin_memory=pin,
                    collate_fn=collate,
                    persistent_workers=False, worker_init_fn=_worker_init if num_workers > 0 else None,
                    multiprocessing_context=_worker_context(dev) if num_workers > 0 else None)
    names: List[str] = []
    embs: List[torch.Tensor] = []
    decoded = []  # device decode: (status words, row of the batch's first image, batch positions they belong to)
    t_wait = t_issue = 0.0
    t_first = None
    it = iter(dl)
    while True:
        t0 = time.perf_counter()
        try:
            batch = next(it)
        except StopIteration:
            break
        t1 = time.perf_counter()
        if t_first is None:
            t_first = t1 - t_start
        else:
            t_wait += t1 - t0
        if device_decode:
            batch_names = batch[0]
            buf, sizes, status, positions = _decode_batch_on_device(decoder, batch)
            decoded.append((status, len(names), positions))
            px = processor.preprocess_packed(buf, sizes)
        elif packed:
            batch_names, buf, sizes = batch
            px = processor.preprocess_packed(buf, sizes.tolist())
        else:
            batch_names, batch_images = batch
            px = processor(images=batch_images).pixel_values
            if device is not None:
                # pageable host memory (the host processor's output): a plain copy. non_blocking from pageable memory
                # overlaps nothing — the runtime stages it through its own pinned buffer before returning — and it
                # was one of the two ingredients of the round-5 hang (DESIGN.md "Extraction loader"); the packed
                # path's buffer is pinned by the loader and copies asynchronously
                px = px.to(device)
        # the embeddings stay on the device until the end (one copy back, src/embeddings/clip.py:140 copies per
        # batch): no per-batch synchronisation, so the next batch's host work overlaps this batch's kernels
        embs.append(embed(px))
        names.extend(batch_names)
        t_issue += time.perf_counter() - t1
    t2 = time.perf_counter()
    final = torch.cat([e.float() for e in embs], 0).cpu() if embs else torch.empty((0, out_dim))
    for status, row0, positions in decoded:  # after the copy back: the device is idle, the status words are there
        for k in torch.nonzero(status.cpu()).flatten().tolist():
            row = row0 + positions[k]
            _, image = ImageDirectoryDataset(image_dir)[ds.filenames.index(names[row])]
            px = processor.preprocess_packed(image.reshape(-1), [tuple(image.shape[:2])])
            final[row] = embed(px).float().cpu()[0]
    out = {"filenames": names, "embeddings": final}
    if feature is not None:
        out["feature"] = feature
    torch.save(out, output_path)
    if stats is not None:
        stats.update(first_batch=round(t_first or 0.0, 3), wait=round(t_wait, 3), issue=round(t_issue, 3),
                     final=round(time.perf_counter() - t2, 3), total=round(time.perf_counter() - t_start, 3))
    return len(names)
