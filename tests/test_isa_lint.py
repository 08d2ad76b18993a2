"""CPU-side lint of the device assembly of every translation unit of libwsu (VERDICT r02 weak #1 / ADVICE r02): the packed-f32
read-after-write sites that made the fused head of conv3x3_pl return wrong logits on ~25 % of the launches must not come back with a
future schedule.  `make -C ws_unet_amd/csrc isa` emits the gfx950 assembly with each TU's own flags (hipcc cross-compiles without a GPU);
tools/pk_hazard.py defines the pattern.  Cause and hardware evidence: profiles/r03/pk_hazard.md."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def isa_files():
    csrc = ROOT / "ws_unet_amd" / "csrc"
    r = subprocess.run(["make", "-C", str(csrc), "isa", "-j8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted((csrc / "isa").glob("*.s"))
    assert len(files) >= 11, files
    return files


def test_no_packed_f32_producer_without_an_issue_cycle_before_its_consumer(isa_files):
    """Every TU: no packed-f32 VALU result is read by the NEXT vector instruction -- neither adjacent (the form that failed on hardware:
    `v_pk_add_f32 ... op_sel_hi:[0,1]` -> `v_max_f32`, which hipcc does not pad) nor separated only by an `s_waitcnt` (which hipcc counts
    as the wait state but which may retire without an issue cycle)."""
    import pk_hazard
    bad = []
    for f in isa_files:
        for kern, ln, prod, between, cons in pk_hazard.find_sites(f.read_text()):
            bad.append(f"{f.name}:{ln} {kern}: {prod} | {' ; '.join(between) or '(adjacent)'} | {cons}")
    assert not bad, "packed-f32 RAW pair without an issue cycle in between:\n" + "\n".join(bad)


def test_every_translation_unit_is_built_without_the_slp_vectorizer():
    mk = (ROOT / "ws_unet_amd" / "csrc" / "Makefile").read_text()
    flags = [ln for ln in mk.splitlines() if ln.startswith("CXXFLAGS")]
    assert len(flags) == 1 and "-fno-slp-vectorize" in flags[0]


def test_lint_recognises_the_round2_sites():
    """The scanner on a minimal excerpt of the SLP build of conv3x3_pl_kernel<1,...> (the failing schedule) and on its padded forms."""
    import pk_hazard
    site = """
kern_a:
	ds_read_b128 v[68:71], v153
	v_pk_fma_f32 v[88:89], v[74:75], v[64:65], 0 op_sel_hi:[1,0,0]
	s_waitcnt lgkmcnt(0)
	v_pk_fma_f32 v[88:89], v[72:73], v[68:69], v[88:89] op_sel_hi:[1,0,1]
"""
    found = pk_hazard.find_sites(site)
    assert len(found) == 1 and found[0][0] == "kern_a" and found[0][3] == ["s_waitcnt lgkmcnt(0)"]
    assert not pk_hazard.find_sites(site.replace("s_waitcnt lgkmcnt(0)", "s_nop 0\n\ts_waitcnt lgkmcnt(0)"))
    assert not pk_hazard.find_sites(site.replace("s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v90, v67"))
    assert not pk_hazard.find_sites(site.replace("v[88:89] op_sel_hi:[1,0,1]", "v[90:91] op_sel_hi:[1,0,1]"))       # no dependence
    patched, n = pk_hazard.patch(site)
    assert n == 1 and not pk_hazard.find_sites(patched) and patched.count("s_nop 0") == 1
    # the form that failed on hardware: an unpadded packed add, its low dword read by the next instruction
    adj = "kern_b:\n\tv_pk_add_f32 v[72:73], v[64:65], v[72:73] op_sel_hi:[0,1]\n\tv_max_f32_e32 v76, 0, v72\n"
    found = pk_hazard.find_sites(adj)
    assert len(found) == 1 and found[0][3] == [] and not pk_hazard.compiler_pads(found[0][2])
    assert pk_hazard.patch(adj, "waitcnt")[1] == 0 and pk_hazard.patch(adj, "adjacent")[1] == 1


# ---- float32 sequences of the metric kernels: no contraction (ws_unet_amd/csrc/wsu_metric.h) ------------------------------------------
# Kernels that restate numpy's float32 operation sequence.  The conv kernels that share pointwise.hip fuse on purpose and are not listed.
UNFUSED_KERNELS = {
    "pointwise.s": ["ws_stats_kernel", "ws_meter_kernel"],                                                    # K10, the WS meter
    "ws_attack.s": ["ws_attack_partial_kernel", "ws_attack_finish_kernel", "filter3x3_valid_kernel", "lsb_delta_unit_kernel"],   # K11
    "hill.s": ["hill_cost_kernel", "pred_err_partial_kernel", "pred_err_finish_kernel"],                      # K12, K14
    "correlation.s": ["pair_corr_mean_kernel", "pair_corr_centred_kernel", "pair_corr_finish_kernel"],        # K15
    "error_boxes.s": ["ae_values_kernel"],                                                                    # K16
}
# f32 FMAs of an expansion other than division, by kernel: (count, what they are).  ws_meter_kernel converts rintf(xi) to int64; the
# float -> int64 expansion is `v_trunc_f32; v_mul_f32 |t|, 2^-32; v_floor_f32; v_fma_f32 lo, hi, -2^32, |t|; v_cvt_u32_f32 x 2`, and
# inside the pixel loop the two literals sit in scalar registers (`s_mov_b32 sN, 0xcf800000` before the loop), so the FMA carries no
# literal of its own.
OTHER_EXPANSION_FMAS = {"ws_meter_kernel": (1, re.compile(r"v_fma_f32 v\d+, v\d+, (s\d+), \|v\d+\|"))}
_FMA = re.compile(r"\s*(v_fma_f32|v_fmac_f32|v_fmamk_f32|v_fmaak_f32|v_pk_fma_f32)(_e32|_e64|_dpp|_sdwa)?\s")
_POW32 = re.compile(r"0x[4c]f800000\b", re.I)                      # +-2^32: the 64-bit integer division's two FMAs per division


def kernel_bodies(text):
    """{kernel name as in the source: its instruction lines}, a body running from the kernel's label to its .amdhsa_kernel line"""
    lines, out = text.splitlines(), {}
    for end, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        start = next(i for i, l in enumerate(lines) if l.startswith(m.group(1) + ":"))
        short = re.search(r"(?:^_Z|_GLOBAL__N_1)(\d+)(?=\D)", m.group(1))          # the length-prefixed source name of the mangled symbol
        out[m.group(1)[short.end():short.end() + int(short.group(1))] if short else m.group(1)] = lines[start + 1:end]
    return out


def f32_fmas_and_divisions(body):
    fmas = [ln.strip() for ln in body if _FMA.match(ln) and not _POW32.search(ln)]
    return fmas, sum(1 for ln in body if re.match(r"\s*v_div_fixup_f32", ln))


def test_no_rn_intrinsic_in_the_sources():
    """`#pragma clang fp contract(off)` does not reach the round-to-nearest header intrinsics: they carry the default contraction and
    fuse with a neighbouring add.  Float32 sequences are written with plain operators (wsu_metric.h)."""
    csrc = ROOT / "ws_unet_amd" / "csrc"
    bad = [f"{f.name}:{i + 1}" for f in sorted(csrc.glob("*.hip")) + sorted(csrc.glob("*.h"))
           for i, ln in enumerate(f.read_text().splitlines()) if re.search(r"__f(add|sub|mul|div)_rn", ln)]
    assert not bad, bad


def test_the_library_reads_two_environment_variables_and_carries_no_timing_probe():
    """A variable in someone's shell must not change what the product computes: the library reads the two organisation switches the GPU
    suite pins (bitwise-equal results) and nothing else, and no timing-only switch, probe build or stamp buffer is left in its sources."""
    csrc = ROOT / "ws_unet_amd" / "csrc"
    sources = sorted(p for p in csrc.iterdir() if p.is_file() and (p.suffix in (".hip", ".h", ".cpp") or p.name == "Makefile"))
    assert len(sources) >= 20, sources
    names = {m for f in sources for m in re.findall(r'getenv\(\s*"?([^")]*)"?\s*\)', f.read_text())}
    assert names == {"WSU_Q_ROWS", "WSU_PL_MSPLIT"}, names
    bad = [f"{f.name}:{i + 1}" for f in sources for i, ln in enumerate(f.read_text().splitlines())
           if re.search(r"ablate|WSU_PROBE|_STAMPS", ln)]
    assert not bad, bad


def test_metric_kernels_have_no_fused_multiply_add_outside_a_division(isa_files):
    """In every listed kernel the f32 FMAs are exactly those of its IEEE divisions: #FMA == k * #v_div_fixup_f32, with k read from
    lsb_delta_unit_kernel of the same build (one division, nothing else that could fuse)."""
    by_name = {f.name: kernel_bodies(f.read_text()) for f in isa_files if f.name in UNFUSED_KERNELS}
    fmas, divs = f32_fmas_and_divisions(by_name["ws_attack.s"]["lsb_delta_unit_kernel"])
    assert divs == 1 and len(fmas) >= 1, (fmas, divs)
    k = len(fmas)
    bad = []
    for fname, kernels in UNFUSED_KERNELS.items():
        for kern in kernels:
            body = by_name[fname][kern]
            fmas, divs = f32_fmas_and_divisions(body)
            extra, form = OTHER_EXPANSION_FMAS.get(kern, (0, None))
            if form is not None:                                   # the named expansion: the FMA's scalar operand holds -2^32
                named = [m for m in map(form.fullmatch, fmas) if m and any(
                    re.match(rf"\s*s_mov_b32 {m.group(1)}, 0xcf800000\b", ln, re.I) for ln in body)]
                assert len(named) == extra, (kern, fmas)
            if len(fmas) != k * divs + extra:
                bad.append(f"{fname} {kern}: {len(fmas)} f32 FMAs, {divs} divisions x {k} + {extra}: " + " ; ".join(fmas[:6]))
    assert not bad, "\n".join(bad)
