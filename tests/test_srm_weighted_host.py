"""CPU: the restatement of the weighted SRM sums (srm_weighted_np) against srm_np and against a brute-force count; the condition on the
K51 inputs that lets the GPU test ask for equality; the selection channel's model files, refusals and argument checks of
ws_unet_amd.srm that need no GPU."""
import numpy as np
import pytest

import srm_np
import srm_weighted_np as swn
from ws_unet_amd import ops, srm


def _image(shape, seed=0):
    x = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    x[:, : shape[1] // 2, : shape[2] // 2] //= 64                           # a smooth corner: the centre bins among the others
    return x


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 4, 4), (2, 9, 21), (1, 12, 14)])
def test_constant_weights_scale_the_counts(shape):
    x = _image(shape)
    counts = srm_np.counts(x)
    np.testing.assert_array_equal(swn.sums(x, np.ones(shape, dtype=np.uint16)), counts)
    for v in (3, 65535):
        np.testing.assert_array_equal(swn.sums(x, np.full(shape, v, dtype=np.uint16)), v * counts)
    assert not swn.sums(x, np.zeros(shape, dtype=np.uint16)).any()


def _runs_through(h, w, taps, scan, at):
    """by brute force: the (row, column) of the first position of every counted run of a residual with these taps, scanned h or v on an
    h x w plane, that has the pixel `at` among its four positions"""
    out = []
    for r in range(h):
        for c in range(w):
            positions = [(r, c + k) if scan == "h" else (r + k, c) for k in range(4)]
            counted = all(0 <= pr + dr < h and 0 <= pc + dc < w for pr, pc in positions for dr, dc in taps)
            if counted and at in positions:
                out.append((r, c))
    return out


@pytest.mark.parametrize("at", [(0, 0), (5, 6), (3, 13), (11, 2), (11, 13)])
def test_one_weight_counts_the_runs_through_its_pixel(at):
    """a single non-zero weight: per table, that weight times the number of counted runs that have the pixel among their four positions"""
    shape = (1, 12, 14)
    x = _image(shape, 1)
    wt = np.zeros(shape, dtype=np.uint16)
    wt[0][at] = 40000
    got = swn.sums(x, wt)
    for t, (cls, q2, res, scan) in enumerate(srm_np.TABLES):
        taps = srm_np.CLASSES[cls][1][res]
        runs = _runs_through(12, 14, taps, scan, at)
        assert got[0, t].sum() == 40000 * len(runs), (cls, q2, res, scan)
        # ... each at the bin of its own four digits
        want = np.zeros(625, dtype=np.int64)
        for r, c in runs:
            digits = []
            for k in range(4):
                pr, pc = (r, c + k) if scan == "h" else (r + k, c)
                R = sum(wgt * int(x[0, pr + dr, pc + dc]) for (dr, dc), wgt in taps.items())
                digits.append(int(srm_np.digit(np.int64(R), q2)) + 2)
            want[sum(d * 5 ** (3 - k) for k, d in enumerate(digits))] += 40000
        np.testing.assert_array_equal(got[0, t], want)
    assert got.any() == (at != (11, 13))                                    # the last pixel is the position of no counted residual


def test_the_largest_of_four_weights_is_taken():
    """two weights inside one run: the run adds the larger once, not their sum"""
    # one row of five pixels: S1 h scanned h has exactly one run, positions 0..3
    x = np.array([[[10, 10, 10, 10, 10]]], dtype=np.uint8)
    wt = np.array([[[5, 9, 0, 7, 60000]]], dtype=np.uint16)                  # column 4 is no position of that run
    got = swn.sums(x, wt)
    assert got[0, 0, 312] == 9 and got[0, 4, 312] == 9 and got.sum() == 18   # S1 h scanned h at its two q; no other table has a run


# ---- K51's inputs ---------------------------------------------------------------------------------------------------------------------

def test_k51_inputs_have_no_pixel_near_a_boundary():
    """no pixel of the GPU comparisons has beta * 65536 within 1e-6 of a positive integer, so a last-bit difference of exp or of the
    division cannot move a floor there and the GPU test asks, in effect, for equality"""
    shapes, contents = set(), set()
    for case in swn.K51_CASES:
        x, rho, lam = swn.k51_case(*case)
        assert swn.near_boundary(x, rho, lam) == 0, case
        wt = swn.change_weights(x, rho, lam)
        assert wt.dtype == np.uint16 and wt.max() <= 43690
        assert (wt[~np.isfinite(rho)] == 0).all() and (np.isfinite(lam) or not wt.any())
        shapes.add(case[1]), contents.add(case[0])
    assert shapes == {(8, 8), (65, 130), (70, 90)} and contents == {"photo", "flat", "ends"}
    assert any(c[3] for c in swn.K51_CASES) and any(not np.isfinite(c[2]) for c in swn.K51_CASES)
    x, rho, lam = swn.k51_case("photo", (70, 90), 3.0, False)                # the weights are a real channel: neither empty nor flat
    wt = swn.change_weights(x, rho, lam)
    assert 0 < np.count_nonzero(wt) and len(np.unique(wt)) > 100


# ---- the model file and the refusals ----------------------------------------------------------------------------------------------------

def _fitted(**kw):
    rng = np.random.default_rng(0)
    m = srm.FLD(0.1, **kw).fit(rng.random((6, srm.DIM)), rng.random((6, srm.DIM)))
    m.stego_methods, m.alphas = ["HILL"], [0.4]
    return m


def test_model_round_trip_and_refusals(tmp_path):
    path, plain = tmp_path / "sc.npz", tmp_path / "plain.npz"
    m = _fitted(selection_channel="hill", sc_alpha=0.4, sc_params={"clamp": 1e9})
    assert m.sc == ("HILL", 0.4, '{"clamp": 1000000000.0}')
    m.save(path)
    with np.load(path) as z:
        assert str(z["features"]) == "srm-linear-sc" and str(z["sc_cost"]) == "HILL" and float(z["sc_alpha"]) == 0.4
        assert str(z["sc_params"]) == '{"clamp": 1000000000.0}'
    for kw in (dict(sc_alpha=0.4), dict(sc_alpha=None), dict(sc_alpha=0.4, submodels="linear")):
        back = srm.load(path, selection_channel="HILL", sc_params={"clamp": 1e9}, **kw)
        assert back.sc == m.sc and np.array_equal(back.w, m.w) and back.b == m.b and (back.stego_methods, back.alphas) == (["HILL"], [0.4])
    with pytest.raises(ValueError, match=r"'srm-linear-sc'.*'HILL'.*'srm-linear'"):          # tag: asked without a selection channel
        srm.load(path)
    with pytest.raises(ValueError, match=r"'HILL'.*'WOW'"):                                  # cost
        srm.load(path, selection_channel="WOW", sc_alpha=0.4, sc_params={"clamp": 1e9})
    with pytest.raises(ValueError, match=r"0\.4.*0\.2"):                                     # sc_alpha
        srm.load(path, selection_channel="HILL", sc_alpha=0.2, sc_params={"clamp": 1e9})
    with pytest.raises(ValueError, match="clamp"):                                           # the cost's parameters
        srm.load(path, selection_channel="HILL", sc_alpha=0.4)
    _fitted().save(plain)
    assert srm.load(plain).sc is None
    with pytest.raises(ValueError, match=r"'srm-linear-sc'.*'srm-linear'"):                  # tag: asked with one
        srm.load(plain, selection_channel="HILL", sc_alpha=0.4)
    with np.load(plain) as z:                                                                # without one the file has no new entry
        assert not [k for k in z.files if k.startswith("sc_")] and str(z["features"]) == "srm-linear"
    # score refuses before it reads any image
    for model, kw, both in ((m, dict(selection_channel="WOW", sc_alpha=0.4), r"'HILL'.*'WOW'"), (m, dict(selection_channel="HILL", sc_alpha=0.2), r"0\.4.*0\.2"),
                            (m, {}, r"'HILL'.*no selection channel"), (srm.load(plain), dict(selection_channel="HILL", sc_alpha=0.4), r"no selection channel.*'HILL'")):
        with pytest.raises(ValueError, match=both):
            srm.score(tmp_path, model, ["HILL"], [0.4], **kw)


def test_argument_checks(tmp_path):
    for submodels in ("minmax", "all"):
        with pytest.raises(ValueError, match="'linear' only"):
            srm.extract(tmp_path, "HILL", 0.4, selection_channel="HILL", submodels=submodels)
        with pytest.raises(ValueError, match="'linear' only"):
            srm.fit(tmp_path, ["HILL"], [0.4], selection_channel="HILL", submodels=submodels)
        with pytest.raises(ValueError, match="'linear' only"):
            srm.FLD(0.1, submodels, selection_channel="HILL", sc_alpha=0.4)
    with pytest.raises(ValueError, match="2 alphas are listed"):             # several alphas and no sc_alpha
        srm.fit(tmp_path, ["HILL"], [0.4, 0.2], selection_channel="HILL")
    with pytest.raises(ValueError, match="2 alphas are listed"):
        srm.main(["fit", "--data", str(tmp_path), "--stego-methods", "HILL", "--alphas", "0.4", "0.2", "--selection-channel", "HILL",
                  "--out", str(tmp_path / "m.npz")])
    with pytest.raises(ValueError, match="sc_alpha"):                        # the covers alone list no alpha
        srm.extract(tmp_path, selection_channel="HILL")
    with pytest.raises(ValueError, match="above 0"):
        srm.extract(tmp_path, selection_channel="HILL", sc_alpha=0.0)
    with pytest.raises(ValueError, match="need a selection_channel"):
        srm.extract(tmp_path, sc_alpha=0.4)
    with pytest.raises(ValueError, match="HILL / SUNIWARD / WOW"):
        srm.extract(tmp_path, selection_channel="MIPOD", sc_alpha=0.4)
    with pytest.raises(SystemExit):
        srm.parse_args(["fit", "--data", "d", "--alphas", "0.4", "--selection-channel", "MIPOD", "--out", "o"])
    a = srm.parse_args(["score", "--data", "d", "--alphas", "0.4", "--model", "m", "--selection-channel", "suniward", "--out", "o"])
    assert a.selection_channel == "SUNIWARD" and a.sc_alpha is None
    assert srm._check_sc(a.selection_channel, a.sc_alpha, a.alphas, a.submodels) == ("SUNIWARD", 0.4, "{}")
    a = srm.parse_args(["fit", "--data", "d", "--alphas", "0.4", "--out", "o"])                  # the defaults: no selection channel
    assert a.selection_channel is None and a.sc_alpha is None and srm._check_sc(None, None, a.alphas) is None
    # a block whose weights are all 0 is refused like a block without a run, and the message holds for both
    sums = np.zeros((1, len(ops.SRM_TABLES), ops.SRM_BINS), dtype=np.int64)
    with pytest.raises(ValueError, match="image 0 has no run of non-zero weight"):
        srm.features(sums)
