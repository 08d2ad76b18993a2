"""CPU-side lint of the 5x5 predictor's kernels (K56, K57, ws_unet_amd/csrc/ols5.hip): like the metric kernels of tests/test_isa_lint.py
K57 restates a float32 operation sequence, so its only f32 FMAs are those of its IEEE division (the table of u / 255.f)."""
from test_isa_lint import ROOT, f32_fmas_and_divisions, isa_files, kernel_bodies  # noqa: F401  (isa_files: the module's fixture)


def test_the_makefile_builds_the_new_translation_unit():
    mk = (ROOT / "ws_unet_amd" / "csrc" / "Makefile").read_text()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")]
    assert len(srcs) == 1 and "ols5.hip" in srcs[0].split()


def test_prediction_kernel_has_no_fused_multiply_add_outside_a_division(isa_files):
    by_name = {f.name: kernel_bodies(f.read_text()) for f in isa_files if f.name in ("ws_attack.s", "ols5.s")}
    assert set(by_name) == {"ws_attack.s", "ols5.s"}, [f.name for f in isa_files]
    assert set(by_name["ols5.s"]) == {"ols_moments5_kernel", "predict5x5_kernel"}, sorted(by_name["ols5.s"])
    fmas, divs = f32_fmas_and_divisions(by_name["ws_attack.s"]["lsb_delta_unit_kernel"])      # one division, nothing else that could fuse
    assert divs == 1 and len(fmas) >= 1
    k = len(fmas)
    body = by_name["ols5.s"]["predict5x5_kernel"]
    fmas, divs = f32_fmas_and_divisions(body)
    assert divs == 1 and len(fmas) == k, f"{len(fmas)} f32 FMAs, {divs} divisions x {k}: " + " ; ".join(fmas[:6])
    # the 24 taps and the 9 of KB, each for the prediction and the bias plane, are multiplications of their own
    assert sum(1 for ln in body if ln.strip().startswith("v_mul_f32")) >= 24
    # the moment kernel is integer work: no f32 FMA at all
    assert f32_fmas_and_divisions(by_name["ols5.s"]["ols_moments5_kernel"]) == ([], 0)
