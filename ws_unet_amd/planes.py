"""Host planes: the Y planes of image files as (N,H,W) uint8 host tensors, and their way to the device.

A leaf module (torch, numpy, the native PNG reader): every table driver decodes and uploads through it.  It owns
  * the pinned rings (`_Ring`): `load_planes_u8` decodes into a reused pinned buffer; `upload_planes` / `mark_uploaded` record the upload's
    event on the buffer's ring slot, and a buffer is handed out again only after that upload has read it.  A caller that keeps a decode for
    later (the per-image rows ahead) asks `handout_of` / `still_holds` whether its buffer has been handed out again since;
  * the pre-decoded uint8 shards (`write_u8_shards` / `use_u8_shards`), which `load_planes_u8` serves instead of inflating a PNG;
  * the host's decode budget (`decode_budget`) and the thread pool for user-supplied readers (`decode_pool`).
"""
from __future__ import annotations

import json
import logging
import os
import pathlib
import threading
import time
import typing
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _io
from .imread import imread4_u8, png_shape, read_luma_batch


def file_stamp(path: str):
    try:
        st = os.stat(path)
        return (st.st_mtime_ns, st.st_size)
    except OSError:
        return None


_POOL = None


def decode_pool():
    """Thread pool for user-supplied `imread` callables (the default reader goes through libwsu_io instead)."""
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(max_workers=max(1, min(16, _io.usable_cores())))
    return _POOL


# ---- the pinned rings -----------------------------------------------------------------------------------------------------------------

_NBUF = 6                                                    # pinned buffers per chunk shape (decode of chunk k + 1 beside upload of chunk k ...)
_NBUF1 = _NBUF                                               # ... and per single-image shape (single_image_buffers: a caller that decodes rows ahead needs more)
_RINGS = {}                                                  # (N,H,W) -> _Ring
_RINGS_LOCK = threading.Lock()


class _Ring:
    """The pinned buffers of one (N,H,W) shape, handed out in turn: chunk k+1 is decoded while chunk k is uploaded and chunk k-1 may still wait
    in the stream (submit / collect pipelining)."""

    def __init__(self, shape, nbuf: int):
        pin = torch.cuda.is_available()
        self.bufs = [torch.empty(shape, dtype=torch.uint8, pin_memory=pin) for _ in range(nbuf)]
        self.slot_of = {id(b): i for i, b in enumerate(self.bufs)}          # (the buffers live as long as the ring: their ids are theirs)
        self.next = 0
        self.count = 0                                       # hand-outs so far
        self.handout = [0] * nbuf                            # per buffer: which hand-out it holds
        self.uploaded = [None] * nbuf                        # per buffer: the event of the upload that last read it (mark_uploaded)

    def hand_out(self) -> int:
        """the next buffer's index (under _RINGS_LOCK)"""
        i = self.next
        self.next = (i + 1) % len(self.bufs)
        self.count += 1
        self.handout[i] = self.count
        return i


def _slot(planes: torch.Tensor):
    """(ring, index) of a tensor that a live ring handed out, else None"""
    ring = _RINGS.get(tuple(planes.shape))
    i = ring.slot_of.get(id(planes)) if ring is not None else None
    return (ring, i) if i is not None and ring.bufs[i] is planes else None


def handout_of(planes: torch.Tensor):
    """Which hand-out of its pinned buffer `planes` holds right now (None: not a ring buffer)."""
    s = _slot(planes)
    return s[0].handout[s[1]] if s is not None else None


def still_holds(planes: torch.Tensor, handout) -> bool:
    """Whether the buffer still holds hand-out number `handout` (it has not been handed out again since)."""
    return handout_of(planes) == handout


def single_image_buffers(nbuf: int) -> None:
    """Pinned buffers per single-image shape from now on; a single-image ring that exists with fewer is replaced."""
    global _NBUF1
    with _RINGS_LOCK:
        _NBUF1 = nbuf
        for key in [k for k, r in _RINGS.items() if k[0] == 1 and len(r.bufs) < nbuf]:
            del _RINGS[key]


# ---- pre-decoded uint8 shards (round 4, SURVEY 8d ".npy covers"): a data set's Y planes decoded ONCE into (N, H, W) uint8 .npy shards; an
# evaluate pass then copies rows out of a memory-mapped shard (~0.03 ms per image) instead of inflating a PNG (~2 ms per image and thread) -- the
# host budget of a file-fed pass stops scaling with the GPU rate.  Same bytes as the decode (tests/test_host_logic.py), same result table.
_U8_SHARDS = {"index": {}, "maps": {}}


def write_u8_shards(files, shard_dir, images_per_shard: int = 1024) -> pathlib.Path:
    """Decode `files` (absolute paths of equally sized images) into <shard_dir>/planes_%04d.npy + index.json (path -> shard, row, source file
    stamp).  Returns shard_dir.  Run once per data set; `use_u8_shards(shard_dir)` then serves load_planes_u8 from it."""
    shard_dir = pathlib.Path(shard_dir)
    shard_dir.mkdir(parents=True, exist_ok=True)
    files = [str(pathlib.Path(f).resolve()) for f in files]
    index = {}
    for k in range(0, len(files), images_per_shard):
        part = files[k:k + images_per_shard]
        planes = read_luma_batch(part)
        name = f"planes_{k // images_per_shard:04d}.npy"
        np.save(shard_dir / name, planes)
        for r, f in enumerate(part):
            index[f] = [name, r, list(file_stamp(f) or (0, 0))]
    with open(shard_dir / "index.json", "w") as fh:
        json.dump({"format": "wsu-u8-shards-1", "files": index}, fh)
    return shard_dir


def use_u8_shards(shard_dir=None) -> int:
    """Serve load_planes_u8 from the shards under `shard_dir` (None: stop using shards).  Returns the number of indexed files."""
    _U8_SHARDS["index"], _U8_SHARDS["maps"] = {}, {}
    if shard_dir is None:
        return 0
    shard_dir = pathlib.Path(shard_dir)
    with open(shard_dir / "index.json") as fh:
        meta = json.load(fh)
    if meta.get("format") != "wsu-u8-shards-1":
        raise ValueError(f"{shard_dir}: not a wsu-u8-shards-1 index")
    _U8_SHARDS["index"] = {f: (str(shard_dir / name), row, tuple(stamp)) for f, (name, row, stamp) in meta["files"].items()}
    return len(_U8_SHARDS["index"])


def _planes_from_shards(fnames, out: np.ndarray) -> bool:
    """Fill out[i] with the pre-decoded plane of fnames[i]; False (out untouched or partly written: the caller decodes) unless EVERY file is
    indexed, unchanged on disk since it was decoded, and of the batch shape."""
    idx = _U8_SHARDS["index"]
    if not idx:
        return False
    ents = []
    for f in fnames:
        e = idx.get(f) or idx.get(str(pathlib.Path(f).resolve()))
        if e is None or e[2] != (file_stamp(f) or (0, 0)):
            return False
        ents.append(e)
    for i, (path, row, _) in enumerate(ents):
        mm = _U8_SHARDS["maps"].get(path)
        if mm is None:
            mm = _U8_SHARDS["maps"][path] = np.load(path, mmap_mode="r")
        if mm.shape[1:] != out.shape[1:]:
            return False
        out[i] = mm[row]
    return True


def decode_budget(files, gpu_images_per_s: float = None, sample: int = 16) -> dict:
    """What a file-fed evaluate pass costs the HOST: the PNG decode time per image on ONE thread (measured on `sample`
    of the files, warm page cache), the decode threads a rank needs to keep its GPU fed at `gpu_images_per_s`, and what this process may use
    (cores it may run on / ranks on this node).  Logs a warning when the budget is short -- the pass is then host-bound:
    pre-decode the data set once (write_u8_shards / use_u8_shards) or give the ranks more cores."""
    files = [str(f) for f in files[:sample]]
    res = {"decode_ms_per_image_per_thread": None, "threads_needed_per_rank": None, "usable_cores": _io.usable_cores(),
           "local_world_size": int(os.environ.get("LOCAL_WORLD_SIZE", "1")), "decode_threads_used": _io.default_threads()}
    if files:
        read_luma_batch(files[:2], threads=1)
        t0 = time.perf_counter()
        read_luma_batch(files, threads=1)
        res["decode_ms_per_image_per_thread"] = (time.perf_counter() - t0) / len(files) * 1e3
    if gpu_images_per_s and res["decode_ms_per_image_per_thread"]:
        res["threads_needed_per_rank"] = gpu_images_per_s * res["decode_ms_per_image_per_thread"] / 1e3
        have = res["usable_cores"] / max(1, res["local_world_size"])
        if have < res["threads_needed_per_rank"] and not _U8_SHARDS["index"]:
            logging.warning("ws_unet_amd.evaluate: this rank can decode on %.1f cores but needs %.1f decode threads to feed its GPU at %.0f images/s "
                            "(%.2f ms per PNG and thread): the pass is host-bound.  Pre-decode the data set (planes.write_u8_shards + use_u8_shards, "
                            "or --u8-shards) or run fewer ranks per host.", have, res["threads_needed_per_rank"], gpu_images_per_s, res["decode_ms_per_image_per_thread"])
    return res


def load_planes_u8(fnames, imread: typing.Callable = imread4_u8) -> typing.Optional[torch.Tensor]:
    """Y planes of a chunk of files as one (N,H,W) uint8 host tensor, or None when the files differ in shape.
    With the default reader the files are decoded by libwsu_io on C++ threads straight into a reused pinned buffer
    (PIL / cv2 style readers hold the GIL: Python threads do not scale them); any other `imread` is called per file."""
    fnames = [str(f) for f in fnames]
    if imread is imread4_u8:
        hw = png_shape(fnames[0]) or imread4_u8(fnames[0]).shape[:2]
        key = (len(fnames), hw[0], hw[1])
        with _RINGS_LOCK:                                     # (the per-image lookahead decodes on a helper thread beside the caller's own reads)
            ring = _RINGS.get(key)
            if ring is None:
                if len(_RINGS) > 8:
                    _RINGS.clear()
                ring = _RINGS[key] = _Ring(key, _NBUF1 if key[0] == 1 else _NBUF)
            i = ring.hand_out()
        if ring.uploaded[i] is not None:                     # the upload that last read this buffer (mark_uploaded)
            ring.uploaded[i].synchronize()
            ring.uploaded[i] = None
        buf = ring.bufs[i]
        if _planes_from_shards(fnames, buf.numpy()):         # pre-decoded (use_u8_shards): a row copy per image instead of an inflate
            return buf
        try:
            read_luma_batch(fnames, out=buf.numpy())
        except ValueError:                                   # ragged shapes
            return None
        return buf
    imgs = list(decode_pool().map(lambda f: np.ascontiguousarray(imread(f)[..., 3]), fnames))
    if len({im.shape for im in imgs}) != 1:
        return None
    return torch.from_numpy(np.stack(imgs))


def plane_groups(fnames, prefetched=None):
    """The Y planes of a chunk as [(host (n,H,W) uint8 tensor, fnames)]: the whole chunk, or image by image when it is ragged.  `prefetched`:
    the 1-tuple of a load_planes_u8 that already ran for this chunk."""
    planes = prefetched[0] if prefetched is not None else load_planes_u8(fnames)
    return [(planes, list(fnames))] if planes is not None else [(load_planes_u8([f]), [f]) for f in fnames]


def mark_uploaded(planes, event=None) -> None:
    """Record, for pinned buffer(s) handed out by load_planes_u8, the point in the current stream after which they may be overwritten
    (one event for all of them; `event`: an already recorded one)."""
    slots = [s for s in map(_slot, [planes] if isinstance(planes, torch.Tensor) else planes) if s is not None]
    if not slots or not torch.cuda.is_available():
        return
    if event is None:
        event = torch.cuda.Event()
        event.record()
    for ring, i in slots:
        ring.uploaded[i] = event


def upload_planes(planes, device):
    """Host planes (one tensor, or several behind one event) -> `device`, queued on the current stream; what load_planes_u8 handed out of its
    pinned ring is marked (mark_uploaded), so that no later decode overwrites a buffer this copy has not read yet."""
    one = isinstance(planes, torch.Tensor)
    dev = [p.to(device, non_blocking=True) for p in ([planes] if one else planes)]
    mark_uploaded(planes)
    return dev[0] if one else dev
