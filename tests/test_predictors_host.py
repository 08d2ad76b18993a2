"""CPU: the one table of model names the WS drivers share (ws_unet_amd/ws/predictors.py), the one resolution function above it
(ws.estimate.resolve_predictor) and the `device_arguments` method that replaces the class ladder of ws.estimate.predictor_arguments.  No GPU
call is made."""
import numpy as np
import pytest
import torch

from ws_unet_amd import filters, ols, ols5
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import estimate, jpeg, keysearch, locate, predictors, roc, structural

DRIVERS = ((estimate, [], "--filters", True), (roc, ["--data", "d", "--out-dir", "o"], "--filters", True),
           (locate, ["--data", "d", "--out-dir", "o", "--alpha", "0.5"], "--filters", False),
           (keysearch, ["--data", "d", "--out", "o", "--alpha", "0.5", "--first", "0", "--count", "4"], "--filter", False))


@pytest.fixture
def registered():
    """a 3x3 fit and a 5x5 kernel under names of their own, taken out again afterwards"""
    taps3, taps5 = np.arange(1., 9.) / 36., np.arange(1., 25.) / 300.
    filters.register_filter("fit3", taps3)
    ols5.register_kernel("fit5", taps5)
    yield taps3, taps5
    del filters.NAMED_FILTERS["fit3"], filters.NAMED_FILTERS_2D["fit3"], ols5.KERNELS["fit5"]


class Dummy:
    def __init__(self, name="dummy"):
        self.name = name
        self.plane = torch.zeros((1, 4, 4))

    def device_arguments(self, x_u8, correct_bias=False):
        return {"x_hat": self.plane, "hat_scale": 1.0}


def test_by_name_returns_what_the_drivers_made(registered):
    taps3, taps5 = registered
    classes = {"AVG": filters.FilterEstimator, "KB": filters.FilterEstimator, "fit3": filters.FilterEstimator,
               "OLSa": ols.AdaptiveOLSEstimator, "OLSa2": ols.AdaptiveOLSEstimator, "OLSa5x5": ols5.Predictor5x5, "OLSa5x5s": ols5.Predictor5x5,
               "fit5": ols5.Predictor5x5, "JPEG": jpeg.JPEGEstimator, "SPA": structural.StructuralEstimator, "RS": structural.StructuralEstimator}
    for name, cls in classes.items():
        a, b = predictors.by_name(name), predictors.by_name(name)
        assert type(a) is cls and type(b) is cls and a is not b, name
    for name in ("AVG", "KB", "fit3"):
        np.testing.assert_array_equal(predictors.by_name(name).kernel, filters.get_filter_estimator(filter_name=name, flatten=False).kernel)
    np.testing.assert_array_equal(predictors.by_name("fit3").kernel, filters.kernel_2d(taps3))
    assert [predictors.by_name(n).symmetric for n in ("OLSa", "OLSa2", "OLSa5x5", "OLSa5x5s")] == [False, True, False, True]
    assert predictors.by_name("OLSa5x5").adaptive and not predictors.by_name("fit5").adaptive
    np.testing.assert_array_equal(predictors.by_name("fit5").taps, taps5)
    assert predictors.by_name("JPEG").quality is None and predictors.by_name("JPEG").fallback == "KB"
    assert predictors.by_name("nothing") is None and predictors.by_name("OLS5x5") is None


def test_the_registered_names_are_gone_again():
    assert predictors.by_name("fit3") is None and predictors.by_name("fit5") is None
    assert "fit3" not in predictors.names() and "fit5" not in predictors.names()


def test_names_are_in_table_order(registered):
    assert predictors.names() == ["RS", "SPA", "OLSa", "OLSa2", "OLSa5x5", "OLSa5x5s", "fit5", "JPEG", "1", "AVG", "AVG9", "KB", "fit3"]
    assert predictors.names() == sorted(structural.NAMES) + sorted(ols.ADAPTIVE_NAMES) + ols5.names() + sorted(jpeg.NAMES) + sorted(filters.NAMED_FILTERS_2D)
    pixel = predictors.names(pixel_only=True)
    assert pixel == predictors.names()[2:] and "SPA" not in pixel and "RS" not in pixel
    for name in predictors.names():                                                # every listed name is answered
        assert predictors.by_name(name) is not None, name


def test_require_names_the_choices():
    assert isinstance(predictors.require("KB"), filters.FilterEstimator)
    with pytest.raises(ValueError, match="unknown filter 'JPG'") as e:
        predictors.require("JPG")
    assert "'JPEG'" in str(e.value) and str(predictors.names()) in str(e.value)
    with pytest.raises(ValueError, match="unknown filter") as e:
        roc.collect_ws_scores("nowhere", ["LSBR"], [1.0], ["KB", "JPG"])
    assert "'JPEG'" in str(e.value)


def test_one_table_serves_all_drivers(monkeypatch, tmp_path):
    made = []

    def make(name):
        made.append(name)
        return Dummy(name)

    assert predictors.by_name("dummy") is None
    monkeypatch.setattr(predictors, "TABLE", predictors.TABLE[:2] + [predictors.Entry(lambda: ["dummy"], make)] + predictors.TABLE[2:])
    est, name = estimate.resolve_predictor("dummy", None, (3,))
    assert isinstance(est, Dummy) and name == "dummy"
    est, name = locate.pixel_predictor("dummy", None, (3,))
    assert isinstance(est, Dummy) and name == "dummy"
    assert predictors.names()[:5] == ["RS", "SPA", "OLSa", "OLSa2", "dummy"] and "dummy" in predictors.names(pixel_only=True)
    # roc's name check accepts it: a data set without images gets as far as its empty table
    made.clear()
    with pytest.raises(ValueError, match="No objects to concatenate"):
        roc.collect_ws_scores(tmp_path / "nowhere", ["LSBR"], [1.0], ["KB", "dummy"])
    assert made == ["dummy"]
    for mod, argv, flag, _ in DRIVERS:
        assert "'dummy'" in _help(mod, flag)
    # the structural names stay refused where a pixel predictor is needed, with the message as it was
    with pytest.raises(ValueError, match="needs a pixel predictor; the structural"):
        locate.pixel_predictor("SPA", None, (3,))
    assert isinstance(estimate.resolve_predictor("RS", None, (3,))[0], structural.StructuralEstimator)


def test_device_arguments_is_the_whole_mapping():
    x = torch.zeros((1, 4, 4), dtype=torch.uint8)
    dummy = Dummy()
    got = estimate.predictor_arguments(x, dummy, None, False)
    assert list(got) == ["x_hat", "hat_scale"] and got["x_hat"] is dummy.plane and got["hat_scale"] == 1.0
    assert estimate._native_planes_ok((3,), dummy, imread4_u8, None)
    assert estimate._native_planes_ok((3,), structural.StructuralEstimator("SPA"), imread4_u8, None)

    def plain(xf):                                                                  # a host callable: the reference's call pattern
        return np.full((xf.shape[0] - 2, xf.shape[1] - 2, 1), 7., dtype=np.float32)

    assert not estimate._native_planes_ok((3,), plain, imread4_u8, None)
    with pytest.raises(ValueError, match="host_planes"):
        estimate.predictor_arguments(x, plain, None, False)
    host = estimate.predictor_arguments(x, plain, [np.zeros((4, 4, 1), dtype=np.float32)], True)
    assert list(host) == ["x_hat", "hat_scale", "x_bias"] and host["hat_scale"] == 1.0
    assert tuple(host["x_hat"].shape) == (1, 2, 2) == tuple(host["x_bias"].shape) and float(host["x_hat"][0, 0, 0]) == 7.
    # the built-in mappings that need no device: a filter's taps, and the JPEG predictor's refusal of bias correction
    kb = predictors.by_name("KB")
    got = estimate.predictor_arguments(x, kb, None, True)
    assert list(got) == ["pixel_filter"]
    np.testing.assert_array_equal(got["pixel_filter"], np.asarray(kb.kernel)[..., ::-1])
    with pytest.raises(ValueError, match="not defined for the JPEG predictor"):
        estimate.predictor_arguments(x, predictors.by_name("JPEG"), None, True)
    for name in predictors.names(pixel_only=True):
        assert hasattr(predictors.by_name(name), "device_arguments"), name
    assert hasattr(estimate.UNetEstimator, "device_arguments")


def _help(mod, flag) -> str:
    """the help text of one option of a driver's parser, on one line"""
    import contextlib
    import io
    import re
    out = io.StringIO()
    with contextlib.redirect_stdout(out), pytest.raises(SystemExit):
        mod.parse_args(["--help"])
    text = out.getvalue()
    start = re.search(rf"^  {flag} ", text, re.M).start()
    end = re.search(r"^  -", text[start + 4:], re.M)
    return " ".join(text[start:start + 4 + end.start() if end else len(text)].split())


def test_the_four_parsers_take_both_kernel_files_and_list_the_names(registered):
    for mod, argv, flag, with_structural in DRIVERS:
        a = mod.parse_args(argv + ["--kernels", "k.json", "--kernels5", "k5.json"])
        assert a.kernels == "k.json" and a.kernels5 == "k5.json", mod.__name__
        b = mod.parse_args(argv)
        assert b.kernels is None and b.kernels5 is None
        text = _help(mod, flag)
        for name in predictors.names(pixel_only=True):
            assert repr(name) in text, (mod.__name__, name)
        assert "'fit3'" in text and "'fit5'" in text                                # the registries are read when the parser is made
        for name in structural.NAMES:
            assert (repr(name) in text) == with_structural, (mod.__name__, name)
