"""CPU-side lint of the cost-ordered changepoint kernels (K33, ws_unet_amd/csrc/ws_ordered.hip): like the metric kernels of
tests/test_isa_lint.py the term kernel restates numpy's float32 operation sequence, so its only f32 FMAs are those of the IEEE divisions;
the fold and finish kernels are integer code without any."""
from test_isa_lint import ROOT, f32_fmas_and_divisions, isa_files, kernel_bodies  # noqa: F401  (isa_files: the module's fixture)


def test_the_makefile_builds_the_new_translation_unit():
    mk = (ROOT / "ws_unet_amd" / "csrc" / "Makefile").read_text()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")]
    assert len(srcs) == 1 and "ws_ordered.hip" in srcs[0].split()


def test_ordered_kernels_have_no_fused_multiply_add_outside_a_division(isa_files):
    by_name = {f.name: kernel_bodies(f.read_text()) for f in isa_files if f.name in ("ws_attack.s", "ws_ordered.s")}
    assert set(by_name) == {"ws_attack.s", "ws_ordered.s"}, [f.name for f in isa_files]
    fmas, divs = f32_fmas_and_divisions(by_name["ws_attack.s"]["lsb_delta_unit_kernel"])      # one division, nothing else that could fuse
    assert divs == 1 and len(fmas) >= 1
    k = len(fmas)
    fmas, divs = f32_fmas_and_divisions(by_name["ws_ordered.s"]["ws_ordered_terms_kernel"])
    assert len(fmas) == k * divs, f"{len(fmas)} f32 FMAs, {divs} divisions x {k}: " + " ; ".join(fmas[:6])
    assert divs >= 2                                                                          # u / 255 and 1 / (5 + var)
    for kern in ("ws_ordered_fold_kernel", "ws_ordered_finish_kernel"):
        assert f32_fmas_and_divisions(by_name["ws_ordered.s"][kern]) == ([], 0), kern
