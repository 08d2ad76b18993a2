"""Records what the UNet's host layer does: the sequence of C-ABI calls a forward (and a backward) makes, shared by
tests/test_gpu_unet_walk.py and tests/golden/make_unet_walk.py (which writes tests/golden/unet_walk.json).

The recorder puts a proxy in the place of the loaded library (``ws_unet_amd._lib._lib``).  The proxy calls every function through unchanged and
logs one short string per call of a symbol of ``_lib.SIGNATURES``:

    <ops._layer>|<symbol without 'wsu_'>|<arguments>

with every non-pointer argument's value and, per pointer argument, ``p`` (given) or ``-`` (null).  The stream (the last argument of every
launching function) and the ``*_bytes`` size queries are left out.
"""
import contextlib
import ctypes
import hashlib

import torch

MODES = ["f32", "bf16", "bf16x3", "bf16x3s", "f16f8", "f16f8p", "f16f8q", "f16f4p", "f16p"]
# every switch a configuration does not name is set to its default, so that the environment (WSU_*) cannot change a trace
DEFAULTS = dict(fuse_head=True, fuse_first=True, fuse_first_planar=False, fuse_up_planar=True, fuse_first_q=False,
                train_products="f16", train_fwd_mode="f16f8x", train_bwd_mode="f16f8x")


def configs():
    """name -> configuration.  kind 'infer': ``call`` is 'forward' (model(x)), 'keep' (forward_features(keep={})) or 'logit'
    (forward_features(want_logit=True)), under no_grad.  kind 'train': a forward under grad, then out.backward(dout)."""
    c = {}

    def infer(name, mode, ns, call="forward", cin=1, cout=1, **attrs):
        c[name] = dict(kind="infer", mode=mode, nsteps=ns, call=call, cin=cin, cout=cout, attrs=attrs)

    def train(name, mode, ns, cin=1, x_grad=False, freeze=None, **attrs):
        c[name] = dict(kind="train", mode=mode, nsteps=ns, cin=cin, cout=1, x_grad=x_grad, freeze=freeze, attrs=attrs)

    for ns in (0, 1, 2):
        for mode in MODES:
            infer(f"infer/{mode}/unet_{ns}", mode, ns)
    for mode in ("f32", "f16f8p", "f16f4p", "f16p"):
        infer(f"infer/{mode}/unet_4", mode, 4)
    infer("infer/bf16x3s/unet_2/fuse_head=0", "bf16x3s", 2, fuse_head=False)
    infer("infer/bf16x3s/unet_2/fuse_first=0", "bf16x3s", 2, fuse_first=False)
    infer("infer/f16f8p/unet_2/fuse_first_planar=1", "f16f8p", 2, fuse_first_planar=True)
    infer("infer/f16f4p/unet_2/fuse_up_planar=0", "f16f4p", 2, fuse_up_planar=False)
    infer("infer/f16f4p/unet_2/fuse_first_q=1", "f16f4p", 2, fuse_first_q=True)
    infer("infer/f16f4p/unet_2/fuse_first_q=1,fuse_up_planar=0", "f16f4p", 2, fuse_first_q=True, fuse_up_planar=False)
    infer("infer/f32/unet_2/keep", "f32", 2, call="keep")
    infer("infer/f16f4p/unet_2/keep", "f16f4p", 2, call="keep")                 # falls to 'bf16x3'
    infer("infer/bf16x3/unet_2/logit", "bf16x3", 2, call="logit")
    infer("infer/f16f4p/unet_2/logit", "f16f4p", 2, call="logit")
    infer("infer/f16f4p/unet_2/in=3", "f16f4p", 2, cin=3)
    infer("infer/bf16x3s/unet_2/in=3", "bf16x3s", 2, cin=3)
    infer("infer/f16f4p/unet_2/out=3", "f16f4p", 2, cout=3)
    infer("infer/f16f4p/unet_2/out=5", "f16f4p", 2, cout=5)                     # not planar-capable: the general path

    for ns in (0, 1, 2):
        train(f"train/f32/unet_{ns}", "f32", ns, train_mode="f32")
        train(f"train/bf16x3/unet_{ns}", "bf16x3", ns, train_mode="bf16x3")
        train(f"train/bf16x3-bf16x3/unet_{ns}", "bf16x3", ns, train_mode="bf16x3", train_fwd_mode="bf16x3", train_bwd_mode="bf16x3")
        train(f"train/f16f8p-f16/unet_{ns}", "f16f4p", ns, train_mode="f16f8p", train_products="f16")
        train(f"train/f16f8p-f16f8/unet_{ns}", "f16f4p", ns, train_mode="f16f8p", train_products="f16f8")
    train("train/bf16x3/unet_1/x_grad", "bf16x3", 1, x_grad=True, train_mode="bf16x3")
    train("train/f16f8p-f16/unet_1/x_grad", "f16f4p", 1, x_grad=True, train_mode="f16f8p")
    train("train/f16f8p-f16/unet_2/in=3", "f16f4p", 2, cin=3, train_mode="f16f8p")        # falls back to 'bf16x3'
    train("train/f16f8p-f16/unet_2/frozen_e21", "f16f4p", 2, freeze="e21", train_mode="f16f8p")
    return c


def build(cfg, seed=0, device="cuda"):
    """(model on the GPU, x, dout): the smallest legal input, N=1 and non-square (H = 2 * 2^nsteps, W = 4 * 2^nsteps), seeded uniform [0,1]
    pixels and default-initialised weights from a seeded CPU generator -- the range flag never trips."""
    from ws_unet_amd.model import get_model
    torch.manual_seed(1000 + seed)
    model = get_model(f"unet_{cfg['nsteps']}", in_channels=cfg["cin"], out_channels=cfg["cout"], channel=[0], drop_rate=None, mode=cfg["mode"])
    for k, v in {**DEFAULTS, **cfg["attrs"]}.items():
        setattr(model, k, v)
    if cfg.get("freeze"):
        getattr(model, cfg["freeze"]).weight.requires_grad_(False)
    g = torch.Generator().manual_seed(2000 + seed)
    h, w = 2 * 2 ** cfg["nsteps"], 4 * 2 ** cfg["nsteps"]
    x = torch.rand((1, cfg["cin"], h, w), generator=g)
    dout = torch.rand((1, cfg["cout"], h, w), generator=g) - 0.5
    return model.to(device), x.to(device), dout.to(device)


def step(cfg, model, x, dout):
    """One forward (and, kind 'train', backward) of the configuration; returns the output tensor(s) as a tuple."""
    if cfg["kind"] == "train":
        out = model(x)
        out.backward(dout)
        return (out,)
    with torch.no_grad():
        if cfg["call"] == "keep":
            keep = {}
            return (model.forward_features(x, keep=keep),) + tuple(keep[k] for k in sorted(keep))
        if cfg["call"] == "logit":
            return tuple(model.forward_features(x, want_logit=True))
        return (model(x),)


class _Proxy:
    def __init__(self, lib, log):
        self._wsu_lib, self._wsu_log = lib, log

    def __getattr__(self, name):
        from ws_unet_amd import _lib, ops
        fn = getattr(self._wsu_lib, name)
        sig = _lib.SIGNATURES.get(name)
        if sig is None or name.endswith("_bytes"):
            return fn
        types = sig[1][:-1] if sig[1] and sig[1][-1] is ctypes.c_void_p else sig[1]      # without the stream
        log, short = self._wsu_log, name[4:]

        def call(*args):
            vals = ",".join(("p" if a else "-") if t is ctypes.c_void_p else repr(a) for a, t in zip(args, types))
            log.append(f"{ops._layer}|{short}|{vals}")
            return fn(*args)
        self.__dict__[name] = call
        return call


@contextlib.contextmanager
def recording():
    """Yields the list that receives one entry per C-ABI call made while the block runs."""
    from ws_unet_amd import _lib
    real, log = _lib.load(), []
    _lib._lib = _Proxy(real, log)
    try:
        yield log
    finally:
        _lib._lib = real


def digest(tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def record(cfg, seed=0, device="cuda"):
    """{'trace': [two consecutive steps' calls, '--' between them], 'digest': sha256 of the first step's output(s)}."""
    from ws_unet_amd import ops
    model, x, dout = build(cfg, seed, device)
    if cfg.get("x_grad"):
        x.requires_grad_(True)
    ops.set_layer(None)
    ops._ws_cache.clear()               # the grow-only backward workspace: its size is an argument, and must not depend on what ran before
    with recording() as log:
        first = step(cfg, model, x, dout)
        log.append("--")
        step(cfg, model, x, dout)
    ops.set_layer(None)
    return {"trace": list(log), "digest": digest(first)}
