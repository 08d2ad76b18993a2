"""CPU-side bound on the chunk step of conv3x3_q / conv3x3_qu (csrc/conv3x3_q.hip: begin_step, q4_reads; conv3x3_qu.hip: sync_step,
skip_units): every lane base of a step's fragment reads is formed in front of the step's barrier and the reads carry immediates, so a step
issues about twenty vector instructions beside its matrix instructions, and the ninth tap's zero operands are READ from a zero block instead
of selected.  `make -C ws_unet_amd/csrc isa` emits the gfx950 assembly (hipcc cross-compiles without a GPU); tools/step_isa.py counts per
basic block.  The bounds are the format-H step plus what the step head needs for the fp4 units' bases, the slot wrap and the two address
selects (profiles/r25/README.md has the counts this tree reaches); the step cannot quietly grow back beyond them."""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

Q_STEP_VALU, Q_STEP_CNDMASK = 24, 4            # steady step of every format-Q conv3x3_q instantiation (was 58-85 / 18-30)
QU_SKIP_VALU = 30                               # skip step of the fused decoder entry (was 70 / 78): its class planes keep a few more


@pytest.fixture(scope="module")
def listings():
    csrc = ROOT / "ws_unet_amd" / "csrc"
    r = subprocess.run(["make", "-C", str(csrc), "isa/conv3x3_q.s", "isa/conv3x3_qu.s", "-j2"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import step_isa
    return step_isa.steps(csrc / "isa" / "conv3x3_q.s"), step_isa.steps(csrc / "isa" / "conv3x3_qu.s")


def _steady(rows):
    """the blocks of a kernel that are whole steps and nothing else: a barrier, no store, the kernel's largest matrix-instruction count -- and
    the step's fragment reads only (the block of a tile's LAST step goes on into the epilogue: it reads the bias from LDS as well)"""
    full = max(c["MFMA"] for _, c, _ in rows)
    cand = [(i, c) for i, c, _ in rows if c["stores"] == 0 and c["barriers"] == 1 and c["MFMA"] == full]
    reads = min(c["ds"] for _, c in cand)
    return [(i, c) for i, c in cand if c["ds"] == reads]


def test_conv3x3_q_steady_steps(listings):
    q, _ = listings
    fmt_q = {k: v for k, v in q.items() if k.startswith("conv3x3_q_kernel<") and k.rstrip(">").endswith(", 1")}      # FMT = WSU_PLANAR_Q
    assert len(fmt_q) == 17, sorted(fmt_q)
    bad = []
    for name, rows in fmt_q.items():
        steady = _steady(rows)
        assert len(steady) >= 2, (name, [(i, c) for i, c, _ in rows])       # the tile's first step and the steps of its inner loop
        for i, c in steady:
            print(f"{name} block {i}: {c}")
            if c["VALU"] > Q_STEP_VALU or c["v_cndmask"] > Q_STEP_CNDMASK:
                bad.append((name, i, c))
    assert not bad, bad


def test_conv3x3_qu_skip_step(listings):
    _, qu = listings
    rows = qu["conv3x3_qu_kernel<1>"]                                           # FMT = WSU_PLANAR_Q
    skip = _steady(rows)                                                        # 56 matrix instructions: the skip steps (a low step has 24)
    assert len(skip) == 2 and all(c["MFMA"] == 56 for _, c in skip), [(i, c) for i, c, _ in rows]
    for i, c in skip:
        print(f"conv3x3_qu_kernel<1> block {i}: {c}")
        assert c["VALU"] <= QU_SKIP_VALU and c["v_cndmask"] <= Q_STEP_CNDMASK, (i, c)


def test_the_fp4_reads_carry_immediates():
    """the largest immediate of a step's reads (the ninth tap's weight plane, 26 * 1024 + 512) fits the 16-bit offset field of a ds read"""
    assert ((8 * 3 + 2) * 64 + 32) * 16 < 1 << 16


def test_counter_on_an_excerpt():
    import step_isa
    block = ["s_barrier", "ds_read_b128", "v_add_u32_e32", "v_cndmask_b32_e32", "v_lshl_add_u32"] + ["v_mfma_f32_32x32x16_f16"] * 8 + ["buffer_store_dwordx4"]
    c = step_isa.count(block)
    assert c == {"MFMA": 8, "VALU": 3, "v_cndmask": 1, "adds": 2, "ds": 1, "stores": 1, "barriers": 1}
    assert [i for i, _, _ in step_isa.step_blocks([block[:6], block])] == [1]
