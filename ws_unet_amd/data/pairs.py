"""Cover/stego pair loader for the UNet train step (`for inputs, (covers, alphas) in loader`).

The reference's training driver and dataset class for the UNet runs are not in the published tree, so the batch
composition is reconstructed from what IS there and from the run configs (models/unet/*/config.json):
  * rows come from `fabrika.cover_stego_spatial` over a split CSV (`tr_csv` / `va_csv`), one row per cover with its stego twin;
  * every pair contributes two samples, interleaved cover, stego as the detector's paired dataset does:
        (input = cover, target = cover, alpha = 0)   (input = stego, target = cover, alpha = row alpha)
    `covers_only=True` (the 'dropout' run) keeps only the first of the two;
  * the epoch order is a seeded permutation of the pairs (`reshuffle()` advances it); `shuffle=False` keeps fabrika's order.
That composition is this package's choice, not a pinned behaviour ("parity unpinned" for the sample order).

`simulate=True` needs no stego files: the rows are the covers alone (`fabrika.precovers`), one file is decoded per pair and the
stego sample is made on the device from the uploaded cover plane (ws_unet_amd.embed, 'HILLR' / 'LSBR' at `alpha`).  Composition,
order, alphas and the rank slices are those of the file route; 'HILLR' twins equal the files `embed.write_dataset` writes, 'LSBR'
twins are drawn afresh every epoch (`lsbr_stream()`), the same on every rank for the same file.

Three seeded draws per epoch, each over ALL pairs and indexed by pair id, so that every rank sees the same value for the same pair:
  * `default_rng([seed, epoch])`     the order of the pairs (`pair_order()`);
  * `default_rng([seed, epoch, 1])`  `post_flip` / `post_rotate` (the published configs' keys; data/__init__.py restates the reference's
    per-image transform): a horizontal flip, a vertical flip and a `rot90` count per pair -> one D4 code (`aug_ops()`, FLIP_ROT_OP).  The
    two samples and both targets of a pair share it -- the target stays aligned with its input; a simulated twin is made from the
    unrotated cover and transformed with it;
  * `default_rng([seed, epoch, 2])`  the payload, when `stego_method` and / or `alpha` is a list (`payload_plan()`): one
    (method, alpha) of the row-major (methods x alphas) combinations per pair; `alphas` of the batch is the drawn payload.

`parity_oracle` / `demosaic_oracle` (the published configs' keys; the reference's ParityOracle / DemosaicOracle, _defs/loader.py:73-103) append
side-information planes to every INPUT: the LSB plane, and the R, G, B site indicators of the RGGB grid.  The reference appends them before
its flips and rotation, so they are transformed with the image (`side_planes_u8`, then `apply_op`); targets and alphas are unchanged.  A
simulated twin's planes come from the twin's own pixels.

MI355X-side: files are decoded by libwsu_io on C++ threads into pinned buffers one batch ahead of the consumer, uploaded as
uint8 and assembled on the device by ONE kernel (wsu_pair_batch_f32: gather + D4 transform + x / 255, inputs and targets together)
-- 1 byte per pixel over PCIe instead of 4.  Data-parallel ranks take
disjoint, equally sized slices of every epoch (rank r gets pairs r, r+world, ...; the ragged tail is dropped so that all ranks
run the same number of steps and the per-step all-reduce never waits for a missing partner).
"""
from __future__ import annotations

import pathlib
import threading
import typing
from queue import Queue

import numpy as np
import torch

from .. import fabrika
from ..imread import read_luma_batch


@fabrika.cover_stego_spatial(iterator=None, convert_to=None, ignore_missing=True)
def _pair_rows(df, **kw):
    return df


@fabrika.precovers(iterator=None, convert_to=None, ignore_missing=True)
def _cover_rows(df, **kw):
    return df


def apply_op(x: np.ndarray, op: int) -> np.ndarray:
    """The D4 element `op` on the last two axes (the codes of wsu_pair_batch_f32): bit 0 mirrors the columns, bit 1 the rows, bit 2
    transposes last."""
    op = int(op)
    if not 0 <= op <= 7:
        raise ValueError(f"op {op} outside 0..7")
    if op & 1:
        x = x[..., :, ::-1]
    if op & 2:
        x = x[..., ::-1, :]
    if op & 4:
        x = np.swapaxes(x, -1, -2)
    return x


def side_planes_u8(plane: np.ndarray, parity: bool, demosaic: bool) -> np.ndarray:
    """(H,W) uint8 -> (P,H,W) uint8 of the UNtransformed image: the pixels, then 0/1 planes in the reference's transform order -- the LSB
    (parity), then the R (even row, even column), G (row + column odd) and B (odd row, odd column) sites (demosaic)."""
    out = [plane]
    if parity:
        out.append(plane & 1)
    if demosaic:
        r, c = np.indices(plane.shape)
        out += [((r | c) & 1) == 0, ((r ^ c) & 1) == 1, ((r & c) & 1) == 1]
    return np.stack([np.asarray(p, dtype=np.uint8) for p in out])


def _flip_rot_table() -> np.ndarray:
    ramp = np.arange(16).reshape(4, 4)
    images = [apply_op(ramp, o) for o in range(8)]
    table = []
    for k in range(4):
        for vflip in (0, 1):
            for hflip in (0, 1):
                y = ramp[:, ::-1] if hflip else ramp
                y = np.rot90(y[::-1] if vflip else y, k)
                table.append(next(o for o in range(8) if np.array_equal(images[o], y)))
    return np.array(table, dtype=np.uint8)


# op code of "horizontal flip, vertical flip, then np.rot90(., k)" at index hflip + 2 * vflip + 4 * k, found by comparing numpy's results
FLIP_ROT_OP = _flip_rot_table()


def _as_list(v) -> list:
    return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v]


class PairLoader:
    def __init__(self, dataset: typing.Union[str, pathlib.Path], split: typing.Optional[str],
                 stego_method: typing.Union[str, typing.Sequence[str], None], alpha: typing.Union[float, typing.Sequence[float], None],
                 batch_size: int = 16, *, covers_only: bool = False, shuffle: bool = True,
                 seed: int = 0, rank: int = 0, world: int = 1, device: typing.Optional[torch.device] = None,
                 take_num_images: typing.Optional[int] = None, threads: typing.Optional[int] = None, simulate: bool = False,
                 post_flip: bool = False, post_rotate: bool = False, parity_oracle: bool = False, demosaic_oracle: bool = False):
        per_pair = 1 if covers_only else 2
        if batch_size % per_pair:
            raise ValueError("batch_size must be even: every pair contributes a cover and a stego sample")
        self.dataset = pathlib.Path(dataset)
        if simulate and device is None:
            raise ValueError("simulate=True makes the stego samples on the device: it needs `device` (host-logic mode has no simulator)")
        self.simulate = bool(simulate) and not covers_only
        methods, alphas = _as_list(stego_method), _as_list(alpha)
        if not methods or not alphas:
            raise ValueError("an empty list of stego methods or alphas")
        self.combos = None                                              # [(method, alpha)] when a pair draws its payload (payload_plan)
        if len(methods) * len(alphas) == 1 or covers_only:
            stego_method, alpha = methods[0], alphas[0]                 # one combination: the scalar route
        else:
            self.combos = [(m, float(a)) for m in methods for a in alphas]
        self.method = None if covers_only or self.combos is not None else stego_method
        if self.simulate:
            self._simulated_rows(split, stego_method, alpha, take_num_images)
        elif self.combos is not None:
            self._combo_rows(split, take_num_images)
        else:
            df = _pair_rows(self.dataset, split=split, stego_method=stego_method, alpha=alpha, take_num_images=take_num_images)
            if not covers_only:
                df = df[~df["name_s"].isna()]
                if df.empty:
                    raise ValueError(f"no cover/stego pairs for stego_method={stego_method!r} alpha={alpha!r} under {self.dataset}")
            self.covers = [str(n) for n in df["name_c"]]
            self.stegos = [] if covers_only else [str(n) for n in df["name_s"]]
            self.alphas = [0.0] * len(df) if covers_only else [float(a) for a in df["alpha_s"]]
        self.batch_size, self.per_pair, self.covers_only = batch_size, per_pair, covers_only
        self.shuffle, self.seed, self.epoch = shuffle, seed, 0
        self.rank, self.world, self.device, self.threads = rank, world, device, threads
        self.post_flip, self.post_rotate = bool(post_flip), bool(post_rotate)
        self.parity_oracle, self.demosaic_oracle = bool(parity_oracle), bool(demosaic_oracle)
        self._pinned = {}
        self._uploaded = {}                                             # slot -> event recorded behind its last upload

    def _simulated_rows(self, split, stego_method, alpha, take_num_images) -> None:
        from .. import embed

        def training_method(m):                                         # the two methods a network is trained on
            name = embed.method_name(m)
            if name not in ("LSBR", "HILLR"):
                raise ValueError(f"PairLoader(simulate=True) makes 'LSBR' / 'HILLR' twins; {name!r} is not a "
                                 f"training method: write its twins with embed.write_dataset")
            return name

        if self.combos is not None:
            self.combos = [(training_method(m), a) for m, a in self.combos]
            bad = [a for _, a in self.combos if not 0.0 <= a <= 1.0]
            if bad:
                raise ValueError(f"alpha={bad[0]!r} outside [0, 1]")
            self.sim_method = self.sim_alpha = None
        else:
            if stego_method is None or alpha is None:
                raise ValueError("simulate=True needs a stego_method and an alpha")
            self.sim_method, self.sim_alpha = training_method(stego_method), float(alpha)
            if not 0.0 <= self.sim_alpha <= 1.0:
                raise ValueError(f"alpha={alpha!r} outside [0, 1]")
            self.method = self.sim_method
        df = _cover_rows(self.dataset, split=split, take_num_images=take_num_images)
        names = [pathlib.Path(n).relative_to(self.dataset).as_posix() for n in df["name"]]
        self.covers = sorted(names, key=lambda f: (pathlib.Path(f).stem, f))        # cover_stego_spatial's row order
        self.stegos = []
        self.alphas = None if self.combos is not None else [self.sim_alpha] * len(self.covers)

    def _combo_rows(self, split, take_num_images) -> None:
        """File route with several (method, alpha): one query per combination, joined on the cover's name; a cover that lacks the twin
        of any combination is dropped.  twins[k][p] = pair p's stego file under combination k."""
        found, order = [], None
        for m, a in self.combos:
            df = _pair_rows(self.dataset, split=split, stego_method=m, alpha=a, take_num_images=take_num_images)
            df = df[~df["name_s"].isna()]
            found.append({str(c): str(s) for c, s in zip(df["name_c"], df["name_s"])})
            if order is None:
                order = [str(c) for c in df["name_c"]]
        self.covers = [c for c in order if all(c in f for f in found)]
        if not self.covers:
            raise ValueError(f"no cover has a stego twin for every one of {self.combos} under {self.dataset}")
        self.twins = [[f[c] for c in self.covers] for f in found]
        self.stegos, self.alphas = [], None

    def lsbr_stream(self, epoch: typing.Optional[int] = None) -> int:
        """The `embed.image_seed` stream of the simulated 'LSBR' twins in `epoch` (default: the current one): a 32-bit function of
        the loader's seed and the epoch, so every epoch draws afresh and every rank makes the same twin of the same file."""
        e = self.epoch if epoch is None else int(epoch)
        return int(np.random.SeedSequence([self.seed, e]).generate_state(1)[0])

    # ---- epoch plan --------------------------------------------------------------------------------------
    def reshuffle(self) -> None:
        """Next epoch's permutation (the reference calls `tr_dataset.reshuffle()` before every epoch, detector/train.py:255)."""
        self.epoch += 1

    def pair_order(self) -> np.ndarray:
        n = len(self.covers)
        order = np.random.default_rng([self.seed, self.epoch]).permutation(n) if self.shuffle else np.arange(n)
        ppb = self.batch_size // self.per_pair                          # pairs per batch on one rank
        steps = n // (ppb * self.world)                                 # same on every rank; ragged tail dropped
        return order[:steps * ppb * self.world].reshape(steps, ppb, self.world)[:, :, self.rank]

    def aug_ops(self, epoch: typing.Optional[int] = None) -> np.ndarray:
        """The D4 code (apply_op) of every pair in `epoch` (default: the current one), indexed by pair id: "flip, then np.rot90(., k)" with
        the three draws of the module docstring.  All zero without `post_flip` / `post_rotate`."""
        n = len(self.covers)
        e = self.epoch if epoch is None else int(epoch)
        rng = np.random.default_rng([self.seed, e, 1])
        zero = np.zeros(n, dtype=np.int64)
        hflip = rng.integers(0, 2, n) if self.post_flip else zero
        vflip = rng.integers(0, 2, n) if self.post_flip else zero
        k = rng.integers(0, 4, n) if self.post_rotate else zero
        return FLIP_ROT_OP[hflip + 2 * vflip + 4 * k]

    def _combo_draw(self, epoch: typing.Optional[int] = None) -> np.ndarray:
        e = self.epoch if epoch is None else int(epoch)
        return np.random.default_rng([self.seed, e, 2]).integers(0, len(self.combos), len(self.covers))

    def payload_plan(self, epoch: typing.Optional[int] = None) -> typing.List[typing.Tuple[typing.Optional[str], float]]:
        """(stego method, alpha) of every pair's stego sample in `epoch` (default: the current one), indexed by pair id."""
        if self.combos is None:
            return [(self.method, float(a)) for a in self.alphas]
        return [self.combos[k] for k in self._combo_draw(epoch)]

    def __len__(self) -> int:
        return len(self.covers) // ((self.batch_size // self.per_pair) * self.world)

    # ---- one batch ---------------------------------------------------------------------------------------
    def _buffers(self, n, h, w, slot):
        key = (n, h, w, slot)
        if key not in self._pinned:
            pin = self.device is not None and torch.cuda.is_available()
            self._pinned[key] = torch.empty((n, h, w), dtype=torch.uint8, pin_memory=pin)
        return self._pinned[key]

    def _read(self, files, slot):
        """Decode `files` into the pinned buffer of `slot` (once the upload that last read it has finished)."""
        from ..imread import png_shape, imread4_u8
        hw = png_shape(files[0]) or imread4_u8(files[0]).shape[:2]
        if self.post_rotate and hw[0] != hw[1]:
            raise ValueError(f"post_rotate needs square images, {files[0]} is {hw[0]}x{hw[1]}")
        buf = self._buffers(len(files), hw[0], hw[1], slot)
        ev = self._uploaded.get(slot)
        if ev is not None:
            ev.synchronize()
        read_luma_batch(files, out=buf.numpy(), threads=self.threads)
        return buf

    def _decode(self, pairs: np.ndarray, slot: int, ops_all: np.ndarray, draw: typing.Optional[np.ndarray]):
        files_in, files_cov, alphas = [], [], []
        for p in pairs:
            c = str(self.dataset / self.covers[p])
            files_in.append(c); files_cov.append(c); alphas.append(0.0)
            if not self.covers_only:
                twin, a = (self.stegos[p], self.alphas[p]) if draw is None else (self.twins[draw[p]][p], self.combos[draw[p]][1])
                files_in.append(str(self.dataset / twin)); files_cov.append(c); alphas.append(a)     # only the drawn twin is decoded
        uniq = list(dict.fromkeys(files_in))                            # every cover is decoded once
        buf = self._read(uniq, slot)
        pos = {f: i for i, f in enumerate(uniq)}
        return {"buf": buf, "idx_in": np.array([pos[f] for f in files_in]), "idx_cov": np.array([pos[f] for f in files_cov]),
                "alphas": torch.tensor(alphas, dtype=torch.float32), "slot": slot, "op": np.repeat(ops_all[pairs], self.per_pair)}

    def _decode_simulated(self, pairs: np.ndarray, slot: int, ops_all: np.ndarray, draw: typing.Optional[np.ndarray]):
        """One decode per pair: plane i of the buffer is pair i's cover, plane len(pairs) + i will be its twin (_finish)."""
        from .. import embed
        files = [str(self.dataset / self.covers[p]) for p in pairs]
        buf = self._read(files, slot)
        m = len(files)
        payload = [(self.sim_method, self.sim_alpha) if draw is None else self.combos[draw[p]] for p in pairs]
        stream = self.lsbr_stream()
        sim = {}                                                        # method -> (planes, alphas, seeds) of its share of the batch
        for meth in dict.fromkeys(pm for pm, _ in payload):
            sel = [i for i in range(m) if payload[i][0] == meth]
            sim[meth] = (sel, [payload[i][1] for i in sel], [embed.image_seed(files[i], stream) for i in sel] if meth == "LSBR" else None)
        return {"buf": buf, "idx_in": np.array([j for i in range(m) for j in (i, m + i)]), "idx_cov": np.repeat(np.arange(m), 2),
                "alphas": torch.tensor([a for _, pa in payload for a in (0.0, pa)], dtype=torch.float32), "slot": slot,
                "op": np.repeat(ops_all[pairs], 2), "sim": sim}

    def _finish(self, staged):
        buf, idx_in, idx_cov, alphas, op = (staged[k] for k in ("buf", "idx_in", "idx_cov", "alphas", "op"))
        if self.device is None:                                         # host-logic mode: uint8 planes, no GPU involved
            planes = buf.numpy()
            if self.parity_oracle or self.demosaic_oracle:              # (n,P,H,W): plane 0 the transformed pixels, then the 0/1 side planes
                x = np.stack([apply_op(side_planes_u8(planes[i], self.parity_oracle, self.demosaic_oracle), o) for i, o in zip(idx_in, op)])
            else:
                x = np.stack([apply_op(planes[i], o) for i, o in zip(idx_in, op)])
            c = np.stack([apply_op(planes[i], o) for i, o in zip(idx_cov, op)])
            return torch.from_numpy(x), (torch.from_numpy(c), alphas)
        from .. import ops
        u8 = buf.to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()                                                     # the producer waits for it before it reuses the slot
        self._uploaded[staged["slot"]] = ev
        if self.simulate:                                               # the twins, made from the uploaded (untransformed) cover planes
            from .. import embed
            if self.combos is None:                                     # one method, one payload: the call this route always made
                twins = embed.simulate(u8, self.sim_method, self.sim_alpha, staged["sim"][self.sim_method][2])[0]
            else:
                twins = torch.empty_like(u8)
                for meth, (sel, a, seeds) in staged["sim"].items():     # one call per method present in the batch, per-image alphas
                    twins[sel] = embed.simulate(u8[sel], meth, a, seeds)[0]
            u8 = torch.cat([u8, twins])
        if self.parity_oracle or self.demosaic_oracle:                  # inputs (n,P,H,W): the side planes behind the image, same launch
            x, c = ops.pair_batch_planes(u8, idx_in, idx_cov, op, self.parity_oracle, self.demosaic_oracle)
        else:
            x, c = ops.pair_batch(u8, idx_in, idx_cov, op)              # (n,1,H,W) fp32 in [0,1], numpy's x / 255.
        return x, (c, alphas.to(self.device))

    def __iter__(self):
        plan = self.pair_order()
        ops_all = self.aug_ops()
        draw = None if self.combos is None else self._combo_draw()
        q: Queue = Queue(maxsize=1)

        def producer():
            try:
                for k, pairs in enumerate(plan):
                    q.put(("ok", (self._decode_simulated if self.simulate else self._decode)(pairs, k % 3, ops_all, draw)))    # 3 slots: decoded ahead, queued, in use
                q.put(("end", None))
            except BaseException as e:                                  # surfaced in the consumer
                q.put(("err", e))

        t = threading.Thread(target=producer, daemon=True)
        t.start()
        while True:
            kind, item = q.get()
            if kind == "err":
                raise item
            if kind == "end":
                break
            yield self._finish(item)
        t.join()
