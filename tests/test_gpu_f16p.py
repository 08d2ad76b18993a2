"""Mode 'f16p' (include/wsu.h K1h): one product per tap, f16(w) * f16(x) with fp32 accumulation, activations stored as two f16 planes (planar H).
Layer kernels against a CPU emulation of the exact arithmetic and against the reference ops; the whole network against the oracle and against a CPU
emulation of the stored-operand rounding, on the 'he' formula weights and on trained-like weights (the 1e-4 gate); repeatability; the range flag
(only beyond +-65504); the evaluate API.  Bands: measured on an MI355X, written next to each bound with a >= 2x margin."""
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, gpu_model, images01, oracle_forward, planar_h_decode, planar_h_encode
from ws_unet_amd import evaluate, formula, ops, unet_run
from ws_unet_amd.model import get_model
from ws_unet_amd.model.unet import ENC, dec_names
from oracle import unet_ref

pytestmark = pytest.mark.gpu


def r16(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


def conv_emul(x, w, b):
    """the kernel's products in fp64: f16(w) * f16(x) (x is already what the tensor stores), reflect padding, + bias"""
    return F.conv2d(F.pad(r16(x).double(), (1, 1, 1, 1), mode="reflect"), r16(w).double(), b.double())


def _rand(shape, g, scale=1.0):
    return torch.relu(torch.randn(shape, generator=g)) * scale


# ---- 1. the 3x3 conv -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w,c1,c2,cout,kind", [
    (1, 16, 32, 64, 0, 64, "plain"),            # one tile
    (2, 40, 72, 32, 48, 128, "plain"),          # fused concat, two output blocks, partial tiles in both directions (half-block items: small grid)
    (3, 20, 34, 64, 0, 64, "pool"),             # non-square, ragged tiles, fused 2x2 max-pool
    (1, 64, 96, 128, 0, 256, "pool"),
    (2, 24, 48, 64, 0, 64, "head1"),            # fused 1x1 head + sigmoid, with y beside it
    (1, 18, 30, 64, 64, 64, "head4"),
    (1, 130, 260, 64, 0, 64, "plain"),          # more tiles than CUs: a persistent workgroup walks several
])
def test_conv3x3_h_against_emulation(n, h, w, c1, c2, cout, kind):
    g = torch.Generator().manual_seed(n * 1000 + h + w + c1 + cout)
    x1 = _rand((n, c1, h, w), g)
    x2 = _rand((n, c2, h, w), g) if c2 else None
    wt = torch.randn((cout, c1 + c2, 3, 3), generator=g) * (2.0 / (9 * (c1 + c2))) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    xs = r16(x1) if x2 is None else torch.cat([r16(x1), r16(x2)], 1)
    acc = conv_emul(xs, wt, b)                                          # fp64 sum of the exact f16 products
    act = torch.relu(acc)
    exact = torch.relu(F.conv2d(F.pad(xs, (1, 1, 1, 1), mode="reflect"), wt, b))        # fp32, weights not rounded
    wp = ops.pack_conv3x3_h(wt.to(DEV))
    kw = {}
    if kind.startswith("head"):
        hc = int(kind[4:])
        hw_ = torch.randn((hc, cout, 1, 1), generator=g) * 0.1
        hb = torch.randn(hc, generator=g) * 0.1
        kw = {"head_w": hw_.to(DEV), "head_b": hb.to(DEV), "want_logit": True}
    rf = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = ops.conv3x3_h(planar_h_encode(x1), None if x2 is None else planar_h_encode(x2), wp, b.to(DEV), cout, pool=kind == "pool", range_flag=rf, **kw)
    torch.cuda.synchronize()
    assert int(rf.item()) == 0
    if kind == "pool":
        y, yp = res
        ref_p = F.max_pool2d(act, 2)
        d = (planar_h_decode(yp).double() - r16(ref_p.float()).double()).abs()
        assert float(d.max()) <= float(ref_p.abs().max()) * 2 ** -10, float(d.max())     # at most one f16 rounding step apart
    elif kind.startswith("head"):
        out, logit, y = res
        z = torch.einsum("nchw,oc->nohw", act, hw_[:, :, 0, 0].double()) + hb.double()[None, :, None, None]
        dz = (logit.cpu().double() - z).abs().max().item()
        assert dz <= 2e-5, dz                                           # the head reads the fp32 accumulators (fp32 summation order)
        assert (out.cpu().double() - torch.sigmoid(z)).abs().max().item() <= 1e-5
    else:
        y = res
    got = planar_h_decode(y).double()
    ref = r16(act.float()).double()
    d = (got - ref).abs()
    # stored values: the f16 rounding of the fp32 sum -- equal to the rounding of the exact sum except where the summation order straddles a
    # rounding boundary (then one f16 step apart)
    assert float((d > 0).double().mean()) <= 2e-3, float((d > 0).double().mean())        # measured 3.4e-4 .. 6.4e-4
    assert float(d.max()) <= float(ref.abs().max()) * 2 ** -10, float(d.max())
    # against the fp32 conv of the unrounded weights: the f16 rounding of the weights and of the stored output, ~2^-11 relative
    rel = ((got - exact.double()).norm() / exact.double().norm()).item()
    assert rel <= 6e-4, rel                                             # measured 2.8e-4 .. 3.0e-4
    print(f"[f16p conv {kind} {n}x{c1}+{c2}x{h}x{w}->{cout}] differing stored values {float((d > 0).double().mean()):.2e}, rel L2 vs fp32 conv {rel:.2e}")


# ---- 2. the fused decoder entry --------------------------------------------------------------------------------------------------------------

def _up_emul(xl, xs, w3, wc, bias, cup, dt=torch.float64):
    """the kernel's arithmetic in fp64: 3x3 taps on the skip half (f16 weights), per parity class a 2x2-tap conv on the clamp-padded low tensor with
    the combined weights rounded to f16"""
    _, _, hl, wl = xl.shape
    y = F.conv2d(F.pad(xs.to(dt), (1, 1, 1, 1), mode="reflect"), r16(w3[:, cup:]).to(dt))
    xlp = F.pad(xl.to(dt), (1, 1, 1, 1), mode="replicate")
    for py in range(2):
        for px in range(2):
            t = F.conv2d(xlp, r16(wc[:, :, py, px]).to(dt))
            y[:, :, py::2, px::2] += t[:, :, py:py + hl, px:px + wl]
    return y + bias.to(dt)[None, :, None, None]


@pytest.mark.parametrize("n,hl,wl,cl,cup,c2,cout", [
    (1, 8, 16, 32, 16, 16, 64),
    (2, 16, 32, 128, 64, 64, 64),               # d41's channels
    (1, 24, 40, 64, 32, 32, 128),               # two output blocks, tiles past the image in both directions
    (3, 5, 7, 16, 16, 48, 64),                  # a single ragged tile
    (1, 64, 48, 32, 16, 32, 64),
])
def test_conv3x3_up_h(n, hl, wl, cl, cup, c2, cout):
    g = torch.Generator().manual_seed(hl * 100 + wl + cl + c2)
    xl = r16(_rand((n, cl, hl, wl), g))
    xs = r16(_rand((n, c2, 2 * hl, 2 * wl), g))
    wt = torch.randn((cl, cup, 2, 2), generator=g) * (1.0 / cl) ** 0.5
    bt = torch.randn(cup, generator=g) * 0.1
    w3 = torch.randn((cout, cup + c2, 3, 3), generator=g) * (2.0 / (9 * (cup + c2))) ** 0.5
    b3 = torch.randn(cout, generator=g) * 0.1
    wsk, wlo, bias, dense = ops.pack_conv3x3_up_h(w3.to(DEV), wt.to(DEV), bt.to(DEV), b3.to(DEV), want_dense=True)
    rf = torch.zeros(1, dtype=torch.int32, device=DEV)
    y = ops.conv3x3_up_h(planar_h_encode(xl), planar_h_encode(xs), wsk, wlo, bias, cout, range_flag=rf)
    got = planar_h_decode(y).double()
    assert int(rf.item()) == 0
    # (a) the exact composition of the reference's two ops on the same stored inputs, fp64
    xu = F.conv_transpose2d(xl.double(), wt.double(), bt.double(), stride=2)
    ref = torch.relu(F.conv2d(F.pad(torch.cat([xu, xs.double()], 1), (1, 1, 1, 1), mode="reflect"), w3.double(), b3.double()))
    rel = ((got - ref).norm() / ref.norm()).item()
    assert rel <= 6e-4, rel                                             # f16 weights and f16 output, ~2^-11 relative (measured 2.9e-4 .. 3.0e-4)
    # (b) its own arithmetic: combined weights (the packer's fp32 values) rounded to f16 once
    emu = r16(torch.relu(_up_emul(xl, xs, w3, dense.cpu(), bias.cpu(), cup)).float()).double()
    d = (got - emu).abs()
    assert float(d.max()) <= float(emu.abs().max()) * 2 ** -10, float(d.max())
    assert float((d > 0).double().mean()) <= 2e-3, float((d > 0).double().mean())        # measured 1.5e-4 .. 5.6e-4
    print(f"[f16p up {n}x{cl}/{c2}x{2 * hl}x{2 * wl}->{cout}] rel L2 vs reference ops {rel:.2e}, differing stored values {float((d > 0).double().mean()):.2e}")


# ---- 3. / 4. the whole network ---------------------------------------------------------------------------------------------------------------

def emulate_f16p(x, sd, nsteps):
    """CPU restatement of the mode's stored-operand rounding (fp32 sums): e11 in fp32 -> f16; every 3x3 conv multiplies f16 weights and f16
    activations; pool of stored values; every decoder block = the fused entry (combined weights from the device packer, rounded to f16); the last
    conv's fp32 accumulators feed the head."""
    t = {k: torch.as_tensor(v).float() for k, v in sd.items()}

    def conv(xin, name):
        return F.conv2d(F.pad(xin, (1, 1, 1, 1), mode="reflect"), r16(t[name + ".weight"]), t[name + ".bias"])

    cur = r16(torch.relu(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), t["e11.weight"], t["e11.bias"])))
    skips = []
    acc = None
    for lvl in range(nsteps + 1):
        a, b = ENC[lvl]
        if lvl >= 1:
            cur = r16(torch.relu(conv(cur, a)))
        acc = conv(cur, b)
        full = r16(torch.relu(acc))
        if lvl < nsteps:
            skips.append(full)
            cur = F.max_pool2d(full, 2)
        else:
            cur = full
    for depth in range(nsteps, 0, -1):
        up, c1, c2 = dec_names(depth)
        w3 = t[c1 + ".weight"]
        cup = t[up + ".weight"].shape[1]
        _, _, bias, dense = ops.pack_conv3x3_up_h(w3.to(DEV), t[up + ".weight"].to(DEV), t[up + ".bias"].to(DEV), t[c1 + ".bias"].to(DEV), want_dense=True)
        cur = r16(torch.relu(_up_emul(cur, skips[depth - 1], w3, dense.cpu(), bias.cpu(), cup, torch.float32)))
        acc = conv(cur, c2)
        cur = r16(torch.relu(acc))
    z = torch.einsum("nchw,oc->nohw", torch.relu(acc), t["outconv.weight"][:, :, 0, 0]) + t["outconv.bias"][None, :, None, None]
    return torch.sigmoid(z)


def _f16p_model(nsteps, variant="he"):
    m = gpu_model(nsteps, variant, "f16p")
    assert m.mode == "f16p"
    return m


@pytest.mark.parametrize("nsteps,n,h,w", [(0, 2, 32, 64), (1, 2, 48, 64), (2, 2, 64, 96), (3, 1, 64, 128), (4, 1, 128, 96),
                                          (2, 4, 512, 512), (2, 1, 2048, 1536)])
def test_network_he_weights(nsteps, n, h, w):
    _, x = images01(n, h, w, seed=nsteps * 7 + h)
    m = _f16p_model(nsteps)
    with torch.no_grad():
        y = m(x.to(DEV)).cpu()
    assert m.mode == "f16p"                                              # no range fallback on these weights
    sd = formula.formula_state_dict(nsteps, "he")
    emu = emulate_f16p(x, sd, nsteps)
    ref = oracle_forward(x, nsteps, "he")
    d_emu = (y.double() - emu.double()).abs()
    mae_emu, max_emu = float(d_emu.mean()), float(d_emu.max())
    mae = float((y.double() - ref.double()).abs().mean())
    print(f"[f16p unet_{nsteps} {n}x{h}x{w} he] MAE vs emulation {mae_emu:.2e} (max {max_emu:.2e}), MAE vs oracle {mae:.2e}")
    # The full-range 'he' weights amplify a one-step f16 rounding flip through the layers: the emulation itself moves by 2.8e-5 (unet_1) and
    # 7.3e-5 (unet_2) MAE when its sums are taken in fp64 instead of fp32, so the GPU cannot be held closer to it than that; the layer tests
    # above carry the tight check.  Measured GPU vs emulation: 7e-8 (unet_0), 2.9e-5 (unet_1), 7.3e-5 (unet_2, every size), 1.7e-4 (unet_3),
    # 1.4e-4 (unet_4); max 1.1e-3
    assert mae_emu <= 3.5e-4, mae_emu
    assert max_emu <= 2.5e-3, max_emu
    # the mode's own MAE on full-range weights, reported: measured 2.7e-5 (unet_0), 1.2e-4, 9.4e-5 (unet_2, every size), 2.5e-4, 1.7e-4 (unet_4)
    assert mae <= 5e-4, mae


@pytest.fixture(scope="module")
def trained_state():
    """unet_2 after 300 AdamW steps of this package's synthetic pretraining (as tests/test_gpu_round4.py)."""
    from ws_unet_amd.trainer import synthetic_pretrain
    m = gpu_model(2, "default", None)
    first = synthetic_pretrain(m, steps=1)
    last = synthetic_pretrain(m, steps=299)
    assert last < 0.5 * first, (first, last)
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def test_mae_gate_on_trained_weights(trained_state):
    """The gate the mode exists for: MAE <= 1e-4 of the [0,1] output against the fp32 CPU oracle on trained-like weights, images the training
    never saw, and no range fallback."""
    _, x = images01(4, 256, 256, seed=77)
    sd = {k: v.float() for k, v in trained_state.items()}
    with torch.no_grad():
        ref = unet_ref.unet_forward(x.clone(), sd, 2)
    assert float(ref.std()) > 0.05, float(ref.std())
    m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode="f16p")
    m.load_state_dict(trained_state)
    m = m.to(DEV)
    with torch.no_grad():
        y = m(x.to(DEV)).cpu()
    assert m.mode == "f16p"
    mae = float((y.double() - ref.double()).abs().mean())
    print(f"[f16p unet_2 trained] MAE vs oracle {mae:.2e}")
    assert mae <= 1e-4, mae                                             # the gate
    assert mae <= 4e-5, mae                                             # band: measured 1.6e-5


# ---- 5. repeatability --------------------------------------------------------------------------------------------------------------------------

def test_repeatable_and_default_mode_unaffected():
    _, x = images01(2, 256, 320, seed=5)
    xd = x.to(DEV)
    base = gpu_model(2, "he", "f16f4p")
    with torch.no_grad():
        y_q0 = base(xd).clone()
    m = _f16p_model(2)
    with torch.no_grad():
        a = m(xd).clone()
        b = m(xd).clone()
    assert torch.equal(a, b)
    with torch.no_grad():
        y_q1 = base(xd)
        y_q2 = gpu_model(2, "he", "f16f4p")(xd)
    assert torch.equal(y_q0, y_q1) and torch.equal(y_q0, y_q2)          # the default's bits do not depend on an f16p model having run
    assert not torch.equal(a, y_q0)                                     # (and the two modes are different arithmetics)


# ---- 6. range flag -----------------------------------------------------------------------------------------------------------------------------

def _scaled_state(s):
    """'he' weights with every activation multiplied by s exactly (ReLU is positively homogeneous): e11's weights and every conv bias times s,
    the head's weights over s -- the same [0,1] output in exact arithmetic"""
    sd = {k: torch.from_numpy(v).clone() for k, v in formula.formula_state_dict(2, "he").items()}
    for k in sd:
        if k == "e11.weight" or (k.endswith(".bias") and not k.startswith("outconv")):
            sd[k] *= s
    sd["outconv.weight"] /= s
    return sd


def _max_activation(x):
    inter = {}
    oracle_forward(x, 2, "he", intermediates=inter)
    return max(float(v.abs().max()) for k, v in inter.items() if torch.is_tensor(v) and k.startswith("x"))


def _run(sd, mode, x, caplog):
    m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode=mode)
    m.load_state_dict(sd)
    m = m.to(DEV)
    caplog.clear()
    with caplog.at_level(logging.WARNING), torch.no_grad():
        y = m(x.to(DEV)).cpu()
    return m, y, [r.getMessage() for r in caplog.records]


def test_range_flag_only_beyond_f16(caplog):
    _, x = images01(2, 64, 64, seed=9)
    amax = _max_activation(x)
    ref = oracle_forward(x, 2, "he")
    # activations up to ~4000: beyond the e4m3 modes' +-448, well inside f16
    sd = _scaled_state(4000.0 / amax)
    m, y, msgs = _run(sd, "f16p", x, caplog)
    assert m.mode == "f16p" and not any("65504" in s for s in msgs), msgs
    assert float((y - ref).abs().mean()) <= 1e-3
    mq, _, msgs_q = _run(sd, "f16f4p", x, caplog)
    assert mq.mode == "bf16x3s" and any("448" in s for s in msgs_q), msgs_q            # unlike the other planar modes
    # activations up to ~2e5: not a finite f16 -> loud fallback to fp32-range storage
    sd = _scaled_state(2e5 / amax)
    m, y, msgs = _run(sd, "f16p", x, caplog)
    assert m.mode == "bf16x3s" and any("65504" in s and "f16p" in s for s in msgs), msgs
    assert float((y - ref).abs().mean()) <= 1e-4                        # recomputed in 'bf16x3s'


# ---- 7. the evaluate API -----------------------------------------------------------------------------------------------------------------------

def test_evaluate_api(tmp_path):
    from PIL import Image
    n = 3
    cov = formula.synthetic_images(n, 512, 512, seed=2024)
    st = np.stack([formula.lsbr_embed(c, 0.4, seed=i) for i, c in enumerate(cov)])
    arr = np.concatenate([cov, st])
    exact = gpu_model(2, "he", "f32", drop_rate=0.)
    model = gpu_model(2, "he", "f16p", drop_rate=0.)
    b0, l0 = unet_run.predict_u8_batch(torch.from_numpy(arr).to(DEV), exact)
    b1, l1 = unet_run.predict_u8_batch(torch.from_numpy(arr).to(DEV), model)
    db, dl = (b1 - b0).abs().cpu(), (l1 - l0).abs().cpu()
    print(f"[f16p evaluate] |beta_hat - f32| max {float(db.max()):.2e} mean {float(db.mean()):.2e}; |l1 - f32| max {float(dl.max()):.2e} (l1 ~{float(l0.mean()):.1f})")
    assert float(db.max()) <= 3e-4, float(db.max())                    # measured 1.1e-4 (mean 4.8e-5)
    assert float(dl.max()) <= 6e-3, float(dl.max())                     # measured 2.8e-3 (l1 ~92, 0..255 units)
    # the per-image API on PNG files: the same numbers
    for i in (0, n):
        fname = tmp_path / f"{i}.png"
        Image.fromarray(arr[i]).save(fname)
        r = evaluate.predict_unet(str(fname), model)
        assert abs(r["beta_hat"] - float(b1[i])) <= 1e-6 and abs(r["l1"] - float(l1[i])) <= 1e-4, (r, float(b1[i]), float(l1[i]))
    assert model.mode == "f16p"
