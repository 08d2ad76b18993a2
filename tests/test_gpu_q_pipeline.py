"""The fragment pipeline of conv3x3_q / conv3x3_qu (csrc/conv3x3_q.hip: units_pipelined, load_unit, mma_unit; conv3x3_qu.hip: skip_units): in
every whole chunk step of the eight-wave form the fragment reads of unit u + 1 are issued before the matrix instructions of unit u, into the
other of two fragment sets, and row 1 of tap (dy, dx) is handed on by name to tap (dy + 1, dx) three taps later instead of being read again.
What can go wrong is a unit that multiplies the other set's fragments (its neighbour's weights, pixels or scale bytes), a handed-on row that
belongs to another tap, or a tile's first / steady / split last step that disagree about the order -- each puts a neighbouring tap's or
pixel's product into the sum.

Exact sums of several taps.  The operands are test_gpu_step_bases.py's (position-coded fp4-exact inputs, one input channel per output channel,
weights +-2^t), but SEVERAL taps are non-zero at once, with weights that differ from tap to tap, so a product formed from a neighbouring
unit's fragment changes the sum.  Every partial sum stays exact in an fp32 accumulator, in any order:
  * kind 'f16' (no residuals), all nine taps: products are multiples of 2^-4, nine of them sum to less than 2^8 -- 12 bits;
  * kind 'xres' (x carries a residual of fp4 code 0.5), all nine taps: the cross terms are multiples of 2^-15 -- 23 bits;
  * kind 'wres' (w = +-2^t (1 + 2^-14)), tap PAIRS: the cross terms are multiples of 2^-18, two products sum to at most 2^5 -- 23 bits.  The
    pairs are (t, t + 3) -- the handed-on row --, the two taps of one fp4 unit, and neighbours across two units.
So the accumulators hold the fp64 conv and the stored bytes are its encoding (torch.equal through the storage's own decoding); the restated
product families are confirmed against the fp64 conv on the CPU before a case is used, and that an fp32 number holds every expected value is
asserted per case."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, planar_q_parts, fp4_values
from test_gpu_step_bases import _assert_a, _assert_q, _bytes, _cmap, _launch_twice, _q_conv_terms, _x, _xq

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent

ALL = tuple(range(9))
# (kind, taps): the sums described above
TAPSETS = [("f16", ALL), ("xres", ALL), ("wres", (0, 3)), ("wres", (5, 8)), ("wres", (2, 3)), ("wres", (7, 8)), ("wres", (1, 2)), ("xres", (4, 7)), ("f16", (0, 8))]


def _wtap(cout, tap, wres):
    """+-2^t, t in {-2, -1, 0}, different from tap to tap for one output channel"""
    co = torch.arange(cout)
    v = torch.exp2(((co + tap) % 3 - 2).double()) * torch.where((co + 2 * tap) % 3 == 0, -1.0, 1.0).double()
    return v * (1.0 + 2.0 ** -14) if wres else v


def _weights(cin, cout, taps, wres):
    w = torch.zeros((cout, cin, 3, 3), dtype=torch.float64)
    for tap in taps:
        w[torch.arange(cout), torch.tensor(_cmap(cin, cout)), tap // 3, tap % 3] = _wtap(cout, tap, wres)
    return w


def _conv_exact(x64, cin, cout, taps, wres):
    """the fp64 conv of the weights above by gathering, reflect padding; asserts that an fp32 number holds every value"""
    xp = F.pad(x64, (1, 1, 1, 1), mode="reflect")
    h, w = x64.shape[2:]
    cm = torch.tensor(_cmap(cin, cout), device=x64.device)
    ref = torch.zeros((x64.shape[0], cout, h, w), dtype=torch.float64, device=x64.device)
    for tap in taps:
        dy, dx = tap // 3, tap % 3
        ref += xp[:, cm, dy:dy + h, dx:dx + w] * _wtap(cout, tap, wres).to(x64.device)[None, :, None, None]
    assert torch.equal(ref.float().double(), ref)
    return ref


@functools.lru_cache(maxsize=None)
def _confirmed(kind, taps):
    """on the CPU: the gather is the fp64 conv, the kernel's three product families sum to it, and its smallest term and largest sum fit 24 bits"""
    n, h, w, cin, cout = 2, 18, 35, 32, 64
    x = _x(n, h, w, cin, kind == "xres", "cpu")
    wgt = _weights(cin, cout, taps, kind == "wres")
    assert torch.equal(x.float().double(), x) and torch.equal(wgt.float().double(), wgt)
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect")
    conv = F.conv2d(xp, wgt)
    assert torch.equal(_conv_exact(x, cin, cout, taps, kind == "wres"), conv)
    assert torch.equal(_q_conv_terms(xp.float(), wgt.float()), conv)
    # every term is a multiple of `unit`, and the sum of the terms' magnitudes stays below 2^24 units: exact in any order
    unit = 2.0 ** {"f16": -4, "xres": -15, "wres": -18}[kind]
    assert torch.equal(torch.round(conv / unit) * unit, conv)
    assert float(F.conv2d(xp.abs(), wgt.abs()).max()) < unit * 2 ** 24
    _, _, cr, _ = planar_q_parts(x.float())
    assert bool((fp4_values(cr) != 0).any()) == (kind == "xres")
    return True


# (n, h, w, cin, cout, variant): 16 / 32 / 48 / 80 channels = the single (split last) step, first + last, and one / three steady steps between
# them; 16 x 32 = one tile, 34 x 66 = nine ragged tiles; Cout 64 / 128 on these grids run the half-block variant, 16 images whole blocks
_CONFIGS = [
    (1, 16, 32, 16, 64, "q"),
    (1, 16, 32, 32, 64, "norelu"),
    (1, 34, 66, 48, 128, "q"),
    (1, 34, 66, 80, 64, "pool"),
    (16, 34, 66, 16, 64, "pool"),
    (16, 34, 66, 32, 64, "q"),
    (16, 34, 66, 48, 64, "pool-norelu"),
    (16, 16, 32, 80, 64, "q"),
]
# format A (f16 + e4m3 residual) holds the sums of kind 'f16' exactly, not those with cross terms: its cases run with kind 'f16' alone
_CONFIGS_A = [(1, 34, 66, 80, 128, "a"), (16, 34, 66, 48, 64, "a"), (1, 16, 32, 16, 64, "a")]


def _conv(kind, taps, n, h, w, cin, cout, variant):
    """one launch pair of a configuration: (the outputs, the expected fp64 values, a label)"""
    from ws_unet_amd import ops
    wres, xres = kind == "wres", kind == "xres"
    x, xq = _x(n, h, w, cin, xres, DEV), _xq(n, h, w, cin, xres)
    wp = ops.pack_conv3x3_f4(_weights(cin, cout, taps, wres).float().to(DEV))
    relu, pool = "norelu" not in variant, "pool" in variant
    ref = _conv_exact(x, cin, cout, taps, wres)
    ref = torch.relu(ref) if relu else ref
    fmt = ops.PLANAR_A if variant == "a" else ops.PLANAR_Q
    out = _launch_twice(lambda: ops.conv3x3_q(xq, None, wp, None, cout, relu=relu, pool=pool, y_format=fmt))
    return out, ref, f"{kind} taps {taps} {n}x{cin}x{h}x{w}->{cout} {variant}"


def _check(out, ref, what, variant):
    pool = "pool" in variant
    (_assert_a if variant == "a" else _assert_q)(out[0] if pool else out, ref, what)
    if pool:
        _assert_q(out[1], F.max_pool2d(ref, 2), what + " y_pool")


@pytest.mark.parametrize("kind,taps", TAPSETS)
def test_sums_of_taps(kind, taps):
    assert _confirmed(kind, taps)
    for cfg in _CONFIGS + (_CONFIGS_A if kind == "f16" else []):
        out, ref, what = _conv(kind, taps, *cfg)
        _check(out, ref, what, cfg[5])


@pytest.mark.parametrize("cin", [16, 48])
@pytest.mark.parametrize("kind,taps", [("f16", ALL), ("xres", ALL), ("wres", (0, 3))])
def test_second_tile_of_a_workgroup(kind, taps, cin):
    """5 x 128 x 256: 320 tiles on at most 256 workgroups -- a workgroup walks a second tile, whose first step defines the accumulators again"""
    assert _confirmed(kind, taps)
    out, ref, what = _conv(kind, taps, 5, 128, 256, cin, 64, "q")
    _check(out, ref, what, "q")


@pytest.mark.parametrize("kind,taps", [("f16", ALL), ("xres", ALL), ("wres", (5, 8))])
def test_head_variant(kind, taps):
    """the head instantiation (its last step is a whole, pipelined step): the head's plane is an fp32 sum of 64 products (the bound of
    test_gpu_step_bases.test_head_variant); the y beside the head is format A, which holds the sums of kind 'f16' exactly (compared there)"""
    from ws_unet_amd import ops
    assert _confirmed(kind, taps)
    n, h, w, cin, cout = 3, 40, 72, 48, 64
    x = _x(n, h, w, cin, kind == "xres", DEV)
    ref = torch.relu(_conv_exact(x, cin, cout, taps, kind == "wres"))
    g = torch.Generator().manual_seed(62)
    hw_, hb = torch.randn((1, 64, 1, 1), generator=g) * 0.05, torch.randn(1, generator=g) * 0.1
    xq, wp = _xq(n, h, w, cin, kind == "xres"), ops.pack_conv3x3_f4(_weights(cin, cout, taps, kind == "wres").float().to(DEV))
    out, ya = _launch_twice(lambda: ops.conv3x3_q(xq, None, wp, None, cout, head_w=hw_.to(DEV), head_b=hb.to(DEV), want_y=True))
    if kind == "f16":
        _assert_a(ya, ref, f"head {kind} taps {taps} y")
    want = torch.sigmoid(F.conv2d(ref.cpu(), hw_.double(), hb.double()))
    err = float((out.cpu().double() - want).abs().max())
    print(f"[q pipeline head {kind} taps {taps}] max |sigmoid - fp64| = {err:.2e}")
    assert err < 2e-5, err


@pytest.mark.parametrize("c2", [32, 64])
@pytest.mark.parametrize("kind,taps", [("f16", ALL), ("xres", ALL), ("wres", (0, 3)), ("wres", (7, 8)), ("wres", (2, 3))])
def test_up_q_skip_half(kind, taps, c2):
    """the skip half of the fused decoder entry (two and four skip steps in front of the low step, nine ragged tiles): zero transposed-conv weights
    leave the skip half alone"""
    from ws_unet_amd import ops
    assert _confirmed(kind, taps)
    n, hl, wl, cl, cup, cout = 1, 17, 33, 16, 16, 64
    xs = _x(n, 2 * hl, 2 * wl, c2, kind == "xres", DEV)
    w3 = torch.zeros((cout, cup + c2, 3, 3), dtype=torch.float64)
    w3[:, cup:] = _weights(c2, cout, taps, kind == "wres")
    w_skip, w_low, bias = ops.pack_conv3x3_up(w3.float().to(DEV), torch.zeros((cl, cup, 2, 2), device=DEV), None, None)
    ql, qs = _xq(n, hl, wl, cl, False), _xq(n, 2 * hl, 2 * wl, c2, kind == "xres")
    y = _launch_twice(lambda: ops.conv3x3_up_q(ql, qs, w_skip, w_low, bias, cout))
    _assert_q(y, torch.relu(_conv_exact(xs, c2, cout, taps, kind == "wres")), f"up_q {kind} taps {taps} c2 {c2}")


# ---- WSU_Q_ROWS=4 (one matrix wave per SIMD, the pipeline's first form) stores the same bytes ------------------------------------------------

_ROWS_CASES = [("xres", ALL, (1, 34, 66, 48, 128, "q")), ("wres", (0, 3), (16, 34, 66, 32, 64, "pool")), ("f16", ALL, _CONFIGS_A[0])]


def _rows_bytes():
    """the stored bytes of _ROWS_CASES under the organisation the process's environment selects"""
    res = []
    for kind, taps, cfg in _ROWS_CASES:
        out, _, _ = _conv(kind, taps, *cfg)
        res += [_bytes(t).cpu() for t in (out if isinstance(out, tuple) else (out,))]
    return res


def test_four_matrix_waves_store_the_same_bytes():
    """the library reads WSU_Q_ROWS once per process: a child process runs the cases with four matrix waves"""
    path = str(HERE / ".qrows_pipeline.pt")
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_q_pipeline as t\n"
            "torch.save(t._rows_bytes(), sys.argv[1])\n") % (str(HERE.parent), str(HERE))
    r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, WSU_Q_ROWS="4"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    four = torch.load(path, weights_only=True)
    os.remove(path)
    assert os.environ.get("WSU_Q_ROWS", "2") != "4", "this process must run the default organisation"
    two = _rows_bytes()
    assert len(two) == len(four) and all(torch.equal(a, b) for a, b in zip(two, four))
