"""CPU-side check of the fragment pipeline in the chunk steps of conv3x3_q / conv3x3_qu (csrc/conv3x3_q.hip: units_pipelined; conv3x3_qu.hip:
skip_units): the fragment reads of unit u + 1 stand in front of the matrix instructions of unit u, so the wait in front of a unit's matrix
instructions leaves the younger unit's reads in flight -- `s_waitcnt lgkmcnt(n)` with n > 0 -- and a wave waits out a whole LDS latency
(`lgkmcnt(0)`) at most twice per step: for the step's first unit, which nothing precedes behind the barrier, and for its last, which nothing
follows.  `make -C ws_unet_amd/csrc isa` emits the gfx950 assembly (hipcc cross-compiles without a GPU); tools/step_isa.py keeps every
`s_waitcnt` with its operands.  The step's instruction bounds of tests/test_isa_step.py hold for the same blocks."""
import subprocess
import sys
from pathlib import Path

import pytest

from test_isa_step import Q_STEP_CNDMASK, Q_STEP_VALU, QU_SKIP_VALU, _steady

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

UNITS = 14                                      # units of a format-Q step: five fp4 units and nine f16 taps


@pytest.fixture(scope="module")
def listings():
    csrc = ROOT / "ws_unet_amd" / "csrc"
    r = subprocess.run(["make", "-C", str(csrc), "isa/conv3x3_q.s", "isa/conv3x3_qu.s", "-j2"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import step_isa
    return (step_isa.steps(csrc / "isa" / "conv3x3_q.s", waitcnt_operands=True), step_isa.steps(csrc / "isa" / "conv3x3_qu.s", waitcnt_operands=True))


def _check_block(name, i, block):
    """the block's fragment waits: at most two `lgkmcnt(0)`, inside the first and the last unit; returns a description of what is wrong"""
    import step_isa
    mfma = [k for k, op in enumerate(block) if step_isa.is_mfma(op)]
    per_unit = len(mfma) // UNITS
    assert per_unit * UNITS == len(mfma), (name, i, len(mfma))
    start = block.index("s_barrier") + 1
    zero = [k for k in range(start, mfma[-1]) if step_isa.lgkm_wait(block[k]) == 0]
    waits = step_isa.step_waits(block)
    print(f"{name} block {i}: {step_isa.stream(block)}")
    assert waits and any(n > 0 and before_mfma for n, before_mfma in waits), (name, i, "no wait leaves reads in flight")
    bad = []
    if len(zero) > 2:
        bad.append((name, i, f"{len(zero)} waits with lgkmcnt(0)"))
    for k in zero:
        before = sum(1 for m in mfma if m < k)
        if not (before < per_unit or len(mfma) - before <= per_unit):
            bad.append((name, i, f"lgkmcnt(0) behind {before} of {len(mfma)} matrix instructions"))
    return bad


def test_conv3x3_q_steps_wait_with_reads_in_flight(listings):
    q, _ = listings
    fmt_q = {k: v for k, v in q.items() if k.startswith("conv3x3_q_kernel<") and k.rstrip(">").endswith(", 1")}      # FMT = WSU_PLANAR_Q: every one is pipelined
    assert len(fmt_q) == 17, sorted(fmt_q)
    bad = []
    for name, rows in fmt_q.items():
        blocks = {i: b for i, _, b in rows}
        steady = _steady(rows)
        assert len(steady) >= 2, (name, [(i, c) for i, c, _ in rows])       # the tile's first step and the steps of its inner loop
        for i, c in steady:
            assert c["VALU"] <= Q_STEP_VALU and c["v_cndmask"] <= Q_STEP_CNDMASK, (name, i, c)
            bad += _check_block(name, i, blocks[i])
    assert not bad, bad


def test_conv3x3_qu_skip_steps_wait_with_reads_in_flight(listings):
    _, qu = listings
    rows = qu["conv3x3_qu_kernel<1>"]                                           # FMT = WSU_PLANAR_Q
    blocks = {i: b for i, _, b in rows}
    skip = _steady(rows)
    assert len(skip) == 2 and all(c["MFMA"] == 56 for _, c in skip), [(i, c) for i, c, _ in rows]
    bad = []
    for i, c in skip:
        assert c["VALU"] <= QU_SKIP_VALU and c["v_cndmask"] <= Q_STEP_CNDMASK, (i, c)
        bad += _check_block("conv3x3_qu_kernel<1>", i, blocks[i])
    assert not bad, bad


def test_wait_parser_on_an_excerpt():
    import step_isa
    block = (["v_add_u32_e32", "s_waitcnt lgkmcnt(0)", "s_barrier", "ds_read_b128", "ds_read_u8", "ds_read_b128", "s_waitcnt lgkmcnt(1)"] + ["v_mfma_f32_32x32x16_f16"] * 2
             + ["s_waitcnt vmcnt(0)", "s_waitcnt lgkmcnt(0)", "v_mfma_scale_f32_32x32x64_f8f6f4", "buffer_store_dwordx4", "s_waitcnt lgkmcnt(0)"])
    assert step_isa.step_waits(block) == [(1, True), (0, True)]                 # the waits in front of the barrier and behind the last matrix instruction do not count
    assert step_isa.stream(block) == "rsr[1]MM[]M"
    assert step_isa.lgkm_wait("s_waitcnt vmcnt(3)") is None and step_isa.lgkm_wait("s_waitcnt vmcnt(0) lgkmcnt(2)") == 2
    assert step_isa.count(block)["MFMA"] == 3 and step_isa.count(block)["ds"] == 3
