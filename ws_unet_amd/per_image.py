"""Rows ahead for the per-image evaluate API (`evaluate.predict_unet` under `predict_unet_cover` / `predict_unet_stego`).

While predict_unet works on row i (upload, forward, two scalars back: ~0.6 ms), helper threads decode the files of rows i + 1 .. i + AHEAD_DEPTH
into the pinned ring -- one decode (~1.5 ms) is longer than everything else of a row (reference: serial, evaluate.py:142-149) -- and the rows
already decoded when row i is asked for ride along in ITS launch (micro-batch), their results kept for their own calls: the per-image loop's
GPU work becomes a few batch-8..16 forwards instead of one batch-1 forward and one blocking read-back per image.
"""
from __future__ import annotations

import dataclasses
import os
import typing
from concurrent.futures import Future, ThreadPoolExecutor

import numpy as np
import torch

from . import _io, planes, unet_run
from .imread import png_shape

MICRO_BATCH = max(1, int(os.environ.get("WSU_PER_IMAGE_BATCH", "16")))      # at most this many images in one per-image-API launch: the row asked for + decoded rows ahead
QUEUE_DEPTH = 3                                              # launches in flight: the one a call waits for + two behind it (the GPU works while Python hands out rows)
AHEAD_DEPTH = QUEUE_DEPTH * MICRO_BATCH                      # rows announced ahead (fabrika's python iterator, fn.lookahead_depth): the rows of the NEXT launches
                                                             # are announced while the rows of this one return from the cache, and decode during this launch
planes.single_image_buffers(AHEAD_DEPTH + 2 * MICRO_BATCH)   # more than the rows decoded ahead + the rows being uploaded


class Decode(typing.NamedTuple):
    """A file announced ahead: its decode on a helper thread -> (pinned planes, their hand-out number) or None, and the file's stamp then."""
    future: Future
    stamp: typing.Any


@dataclasses.dataclass(eq=False)
class Launch:
    """Rows queued on the device as one launch: nothing has waited for it yet."""
    paths: list
    stamps: list
    x: torch.Tensor                                          # the device planes (a recompute reads them)
    host: torch.Tensor                                       # pinned: (beta_hat[n], l1[n], range flag) arrive here
    event: typing.Any                                        # recorded behind the copy into `host`
    n: int
    planar: bool
    model: typing.Any                                        # the model itself, not its id: an address is reused once its object is gone
    mode: typing.Any


class Result(typing.NamedTuple):
    """A row computed in an earlier row's launch, waiting for its own call."""
    beta: np.float32
    l1: np.float32
    stamp: typing.Any
    model: typing.Any
    mode: typing.Any


def _stale(rec, model, stamp=None, now=None):
    """THE validity rule of what was computed ahead (`rec`: a Result or a Launch): by this model (the object itself), from the file as it is
    now, in the model's present arithmetic.  -> None when all three hold, else the first that does not: 'model', 'stamp' or 'mode'."""
    if rec.model is not model:
        return "model"
    if stamp != now:
        return "stamp"
    return None if rec.mode == getattr(model, "mode", None) else "mode"


def _decode(path: str):
    """-> (planes, hand-out number of the pinned buffer) or None"""
    if png_shape(path) != (512, 512):
        return None
    pl = planes.load_planes_u8([path])
    return None if pl is None else (pl, planes.handout_of(pl))


def _ring_valid(res) -> bool:
    """the pinned buffer of a finished ahead-decode still holds that decode (it has not been handed out again since)"""
    return res is not None and planes.still_holds(*res)


class RowsAhead:
    """The rows that predict_unet's caller announced before asking for them: decoded ahead, computed in micro-batches, handed out row by row.

    What holds, whatever is announced:
      * rows, order and numbers are those of the one-image-per-launch loop, bit for bit (an image's statistics do not depend on what else
        is in its batch), and every image is computed once;
      * at most MICRO_BATCH images go into a launch; further launches are queued only while fewer than QUEUE_DEPTH are in flight and at
        least max(1, MICRO_BATCH // 2) rows are decoded (a launch of one or two rows costs the host what a full one does);
      * launches are collected in submission order up to the one that holds the row asked for; launches of another model are skipped;
      * a launch whose range flag tripped, or whose model has changed mode since, is recomputed in the present arithmetic;
      * a decode whose ring buffer was handed out again is dropped and its own row decodes again; the same holds for a file whose stamp
        changed, a file that is not 512x512 and an unreadable file (its own row raises the error, in order).  Nothing waits on a decode
        that is not finished;
      * a result or launch is served only to the model OBJECT that computed it, in the mode it was computed in, for the file as it is now
        (`_stale`); the records hold the model, so its address cannot pass to another model while they exist;
      * reset() -- start and end of a fabrika pass -- cancels the pending decodes and forgets results and launches, and with them the models;
      * the decode pool has max(4, min(AHEAD_DEPTH, usable cores)) threads."""

    def __init__(self):
        self.pool = None
        self.pending: typing.Dict[str, Decode] = {}          # announced, not yet asked for or taken along (oldest first)
        self.results: typing.Dict[str, Result] = {}
        self.inflight: typing.List[Launch] = []              # in submission order

    def announce(self, fname) -> None:
        """`fname` will be asked for soon: decode it on a helper thread."""
        if self.pool is None:
            self.pool = ThreadPoolExecutor(max_workers=max(4, min(AHEAD_DEPTH, _io.usable_cores())))
        pend = self.pending
        while len(pend) > AHEAD_DEPTH:                       # rows that were announced and never asked for
            pend.pop(next(iter(pend))).future.cancel()
        # a decode lives in one buffer of load_planes_u8's pinned ring, which is handed out again after the ring's size in further decodes:
        # a decode whose buffer was re-issued (_ring_valid), or of a file rewritten since, is dropped instead of uploaded
        pend[str(fname)] = Decode(self.pool.submit(_decode, str(fname)), planes.file_stamp(str(fname)))

    def reset(self) -> None:
        """Forget every announced-but-unconsumed decode and every computed-ahead result (start and end of a fabrika pass; a pass that raised
        midway leaves entries behind)."""
        pend = self.pending
        while pend:
            pend.pop(next(iter(pend))).future.cancel()
        self.results.clear()
        del self.inflight[:]                                 # (queued launches of an abandoned pass simply finish; nobody reads them)

    def predict(self, fname, model):
        """(beta_hat, l1) of `fname`, or None when it is not a 512x512 PNG that the native reader takes (the caller's slow paths define what
        happens then)."""
        path = str(fname)
        now = planes.file_stamp(path)                        # ONE stat per call: what is taken from the caches below must be of this file as it is now
        ent = self.results.pop(path, None)                   # computed in an earlier row's launch (the rows announced ahead ride along, below)
        if ent is not None and _stale(ent, model, ent.stamp, now) is None:
            return ent.beta, ent.l1
        # rows announced ahead whose files are already decoded join this row's launch (up to MICRO_BATCH images), and up to two further launches of
        # such rows are queued behind it before this call blocks on its own result: the reference's loop is one image per forward and one
        # blocking read-back per image (evaluate.py:48); the GPU sees launches it can fill and works on the next one while Python hands out this one's rows
        h = self._inflight_of(path, model, now)
        if h is None:
            pl = self._take_ahead(path, now)                 # decoded ahead by the iterator's lookahead, if still valid
            if pl is None:
                pl = planes.load_planes_u8([path]) if png_shape(path) == (512, 512) else None
            if pl is None:
                return None
            h = self._submit([(path, pl, now)] + self._take_ready(MICRO_BATCH - 1), model)
        while len(self.inflight) < QUEUE_DEPTH and self._ready() >= max(1, MICRO_BATCH // 2):
            more = self._take_ready(MICRO_BATCH)
            if not more:
                break
            self._submit(more, model)
        while True:                                          # collect in submission order up to this row's launch; the other rows' results wait for their calls
            g = self.inflight.pop(0)
            why = _stale(g, model)                           # (its rows carry their own stamps, compared when each is asked for)
            if why == "model":                               # queued for another model (a caller alternating models outside a fabrika pass): not ours
                continue
            beta, l1 = self._collect(g, model, recompute=why == "mode")
            for k, p in enumerate(g.paths):
                if g is h and p == path:
                    mine = (np.float32(beta[k]), np.float32(l1[k]))
                else:
                    self.results[p] = Result(np.float32(beta[k]), np.float32(l1[k]), g.stamps[k], model, getattr(model, "mode", None))
            if g is h:
                return mine

    def _ready(self) -> int:
        """how many announced rows, oldest first, have finished decoding"""
        k = 0
        for d in self.pending.values():
            if not d.future.done():
                break
            k += 1
        return k

    def _take_ready(self, limit: int):
        """Announced rows whose decode has FINISHED, oldest first, at most `limit`: [(path, planes, stamp)].  Stops at the first row still decoding
        (nothing waits here); rows whose ring slot may have been re-issued, whose file changed, or that are not 512x512 are dropped -- their own call
        decodes them again."""
        out = []
        pend = self.pending
        for path in list(pend):
            if len(out) >= limit:
                break
            fut, stamp = pend[path]
            if not fut.done():
                break
            pend.pop(path)
            if fut.cancelled():                              # (a file rewritten since it was announced is caught when its row takes the result: the
                continue                                     # result carries the announce-time stamp -- no stat per candidate here)
            try:
                res = fut.result()
            except Exception:                                # unreadable file: its own row raises the error, in order
                continue
            if _ring_valid(res):
                out.append((path, res[0], stamp))
        return out

    def _take_ahead(self, path: str, now):
        """the planes of `path` decoded ahead, if the file is still the one announced and the buffer still holds it (waits for that decode)"""
        ent = self.pending.pop(path, None)
        if ent is None:
            return None
        if ent.stamp != now:                                 # the file changed since it was announced: decode again
            ent.future.cancel()
            return None
        res = ent.future.result()
        return res[0] if _ring_valid(res) else None          # (a buffer handed out again since holds another file: decode again)

    def _submit(self, rows, model) -> Launch:
        """rows [(path, pinned planes (1,H,W), stamp)] -> upload, forward, statistics and the copy of (beta_hat[n], l1[n], range flag) into a pinned
        host buffer, all queued on the current stream, nothing waits.  The launch joins self.inflight."""
        dev = unet_run.model_device(model)
        n = len(rows)
        if n == 1:
            x_u8 = planes.upload_planes(rows[0][1], dev)
        else:
            x_u8 = torch.empty((n,) + tuple(rows[0][1].shape[1:]), dtype=torch.uint8, device=dev)
            for k, (_, pl, _) in enumerate(rows):
                x_u8[k].copy_(pl[0], non_blocking=True)
            planes.mark_uploaded([r[1] for r in rows])       # one event behind the n uploads
        dev_v, planar = unet_run._pack_stats(*unet_run.predict_u8_batch(x_u8, model), model)
        host = torch.empty(dev_v.shape, dtype=torch.float32, pin_memory=dev_v.is_cuda)
        host.copy_(dev_v, non_blocking=True)
        ev = None
        if dev_v.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
        h = Launch([r[0] for r in rows], [r[2] for r in rows], x_u8, host, ev, n, planar, model, getattr(model, "mode", None))
        self.inflight.append(h)
        return h

    def _collect(self, h: Launch, model, recompute: bool):
        """wait for ONE launch's results (its own event, not the stream): (beta_hat[n], l1[n]) as numpy.  A tripped range flag -- or `recompute`:
        the model left the arithmetic this launch was computed in since (an earlier launch tripped it) -- recomputes the launch's images in the
        present arithmetic."""
        if h.event is not None:
            h.event.synchronize()
        beta, l1, tripped = unet_run._unpack_stats(h.host.numpy().copy(), h.n, h.planar)
        if (tripped and unet_run.range_fallback(model)) or recompute:
            beta, l1, _ = unet_run.predict_u8_one_readback(h.x, model)
        return beta, l1

    def _inflight_of(self, path: str, model, now):
        """the queued launch that holds `path` (as the file is `now`) for this model, or None; one computed in another mode counts: it is
        recomputed when collected"""
        for h in self.inflight:
            if path in h.paths and _stale(h, model, h.stamps[h.paths.index(path)], now) in (None, "mode"):
                return h
        return None


rows_ahead = RowsAhead()
