"""CPU: the host statistics of ws_unet_amd.histogram -- the chi-square p-value against scipy's incomplete gamma function and on hand cases,
the centres of mass against numpy.fft, the message length on hand curves -- the numpy restatement of the same (histogram_np), the command
line and the error messages.  Nothing here touches the GPU."""
import numpy as np
import pytest
import torch

import histogram_np
from ws_unet_amd import histogram, ops


def _random_histograms():
    rng = np.random.default_rng(58)
    hs = [rng.integers(0, 400, 256), rng.integers(0, 12, 256), rng.poisson(1000., 256), rng.poisson(3., 256)]
    flat = rng.poisson(1000., 128)                                      # nearly equalised pairs: a p-value well inside (0, 1)
    hs.append(np.stack([flat, flat + rng.integers(-40, 41, 128)], axis=1).reshape(-1))
    hs.append(np.stack([flat, flat + rng.integers(-70, 71, 128)], axis=1).reshape(-1))
    sparse = np.zeros(256, dtype=np.int64)
    sparse[40:80] = rng.integers(0, 5000, 40)                           # most pairs dropped
    hs.append(sparse)
    return np.stack(hs).astype(np.int64)


def test_chi2_against_scipy():
    """relative 1e-9 on p where p >= 1e-200, for the module and for the restatement, p itself and not its logarithm.  (The module has its
    own incomplete gamma function because torch.special.gammaincc misses this bound in the bulk: 1.5e-9 relative on histogram 1 below.)"""
    special = pytest.importorskip("scipy.special")
    hs = _random_histograms()
    stat, dof, p = histogram.chi2(hs)
    assert stat.dtype == np.float64 and dof.dtype == np.int64 and p.dtype == np.float64 and p.shape == (len(hs),)
    seen = 0
    for i, h in enumerate(hs):
        e, o = h[0::2].astype(np.float64), h[1::2].astype(np.float64)
        keep = e + o >= 10
        want_stat = float(((e[keep] - o[keep]) ** 2 / (2. * (e[keep] + o[keep]))).sum())
        want_dof = int(keep.sum()) - 1
        want_p = float(special.gammaincc(want_dof / 2., want_stat / 2.))
        s_np, d_np, p_np = histogram_np.chi2(h)
        print(f"histogram {i}: statistic {want_stat:.6g} dof {want_dof} p scipy {want_p:.17g} module {p[i]:.17g} restated {p_np:.17g}")
        assert dof[i] == want_dof == d_np
        assert abs(stat[i] - want_stat) <= 1e-12 * want_stat and abs(s_np - want_stat) <= 1e-12 * want_stat
        if want_p >= 1e-200:
            seen += 1
            assert abs(p[i] - want_p) <= 1e-9 * want_p and abs(p_np - want_p) <= 1e-9 * want_p
        else:
            assert p[i] < 1e-199 and p_np < 1e-199
    assert seen >= 4
    # the tail on its own: fixed (dof, statistic) from the bulk down to 1e-200 (96.1: Python floats must not pass through float32)
    for d, s in ((1, 0.5), (77, 96.1), (127, 100.), (127, 127.), (127, 300.), (127, 700.), (127, 1200.), (60, 900.), (3, 900.)):
        want = float(special.gammaincc(d / 2., s / 2.))
        h_p = float(histogram.gammaincc(d / 2., s / 2.))
        assert want >= 1e-200 and abs(h_p - want) <= 1e-9 * want and abs(histogram_np.gammaincc(d / 2., s / 2.) - want) <= 1e-9 * want, (d, s)


def test_chi2_hand_cases():
    equal = np.repeat(np.arange(5, 133), 2)                            # all pairs equal: statistic 0, p 1
    s, d, p = histogram.chi2(equal)
    assert (s, d, p) == (0., 127, 1.) and histogram_np.chi2(equal) == (0., 127, 1.)
    one = np.zeros(256, dtype=np.int64)
    one[6:8] = (30, 50)                                                # one pair kept: dof 0, p 0
    s, d, p = histogram.chi2(one)
    assert (s, d, p) == ((30 - 50) ** 2 / 160., 0, 0.) and histogram_np.chi2(one) == (2.5, 0, 0.)
    low = np.full(256, 4)                                              # every n_k = 8 < 10: nothing kept
    assert histogram.chi2(low)[1:] == (-1, 0.) and histogram_np.chi2(low)[1:] == (-1, 0.)
    assert histogram.chi2(low, min_pair=8)[1:] == (127, 1.)            # ... and kept at a lower bar
    half = np.zeros(256, dtype=np.int64)
    half[0::2] = 100                                                   # h[2k+1] = 0 throughout: each pair adds 100^2 / 200 = 50
    s, d, p = histogram.chi2(half)
    assert s == 128 * 50. and d == 127 and 0. <= p < 1e-300 and histogram_np.chi2(half)[:2] == (6400., 127)
    # a batch keeps its leading shape, and torch tensors are taken as numpy arrays are
    batch = np.stack([equal, one, low, half]).reshape(2, 2, 256)
    s, d, p = histogram.chi2(torch.from_numpy(batch))
    assert s.shape == d.shape == p.shape == (2, 2) and d.tolist() == [[127, 0], [-1, 127]] and p.tolist() == [[1., 0.], [0., float(p[1, 1])]]
    with pytest.raises(ValueError, match="256 bins"):
        histogram.chi2(np.zeros(255))


def test_com_and_com2_against_numpy_fft():
    """relative 1e-9: float64 FFTs of 256 / 65 536 integers err near 1e-14, an indexing mistake moves the value by more than 1e-3"""
    rng = np.random.default_rng(59)
    hs = np.stack([rng.integers(0, 3000, 256), rng.poisson(50., 256), np.bincount(rng.normal(120, 20, 100000).astype(int) % 256, minlength=256)])
    got = histogram.com(hs)
    assert got.shape == (3,) and got.dtype == np.float64
    for i, h in enumerate(hs):
        mag = np.abs(np.fft.fft(h.astype(np.float64)))
        want = sum(k * mag[k] for k in range(128)) / sum(mag[k] for k in range(128))
        assert abs(got[i] - want) <= 1e-9 * want and abs(histogram_np.com(h) - want) <= 1e-9 * want
        wrong = sum(k * mag[k] for k in range(1, 129)) / sum(mag[k] for k in range(1, 129))
        assert abs(wrong - want) > 1e-3 * want
    delta = np.zeros(256)
    delta[77] = 5.                                                     # |F| is flat: the mean of 0..127
    assert histogram.com(delta) == pytest.approx(63.5, rel=1e-12) and histogram_np.com(delta) == pytest.approx(63.5, rel=1e-12)
    A = rng.integers(0, 50, (2, 256, 256))
    A[1] = np.triu(A[1])                                               # not symmetric: a transposed index would show
    got2 = histogram.com2(torch.from_numpy(A))
    for i in range(2):
        mag = np.abs(np.fft.fft2(A[i].astype(np.float64)))
        want = sum((k + l) * mag[k, l] for k in range(128) for l in range(128)) / mag[:128, :128].sum()
        assert abs(got2[i] - want) <= 1e-9 * want and abs(histogram_np.com2(A[i]) - want) <= 1e-9 * want
    d2 = np.zeros((256, 256))
    d2[3, 200] = 1.
    assert histogram.com2(d2) == pytest.approx(127., rel=1e-12)        # flat |F2|: mean of k + l
    assert np.isnan(histogram.com(np.zeros(256)))
    with pytest.raises(ValueError, match="256 bins"):
        histogram.com(np.zeros(128))
    with pytest.raises(ValueError, match=r"\(256, 256\)"):
        histogram.com2(np.zeros((256, 128)))


def test_length_on_hand_curves():
    p = np.array([[1., .9, .5, .49, 1., 1., 1., 1., 1., 1.], [0.] * 10, [1.] * 10, [.4, 1., 1., 1., 1., 1., 1., 1., 1., 1.]])
    np.testing.assert_array_equal(histogram.length(p), [.3, 0., 1., 0.])
    np.testing.assert_array_equal(histogram_np.length(p), [.3, 0., 1., 0.])
    np.testing.assert_array_equal(histogram.length(p, threshold=.45), [1., 0., 1., 0.])
    assert histogram.length(p[0]) == .3 and histogram.length(np.zeros((0, 4))).shape == (0,)


def test_restated_counts_on_hand_planes():
    x = np.array([[0, 1, 2], [3, 4, 255]], dtype=np.uint8)
    t = histogram_np.seg_hist(x, 4)                                    # segments of t * 4 // 6: [0,1], [2], [3,4], [5]
    assert [np.flatnonzero(r).tolist() for r in t] == [[0, 1], [2], [3, 4], [255]] and t.sum() == 6
    assert [np.flatnonzero(r).tolist() for r in histogram_np.seg_hist(x, 4, "rows_up")] == [[3, 4], [255], [0, 1], [2]]
    np.testing.assert_array_equal(histogram_np.seg_lengths(2, 3, 4), [2, 1, 2, 1])
    np.testing.assert_array_equal(histogram_np.seg_lengths(2, 3, 8), [1, 1, 1, 0, 1, 1, 1, 0])
    np.testing.assert_array_equal(histogram_np.seg_hist(x, 8).sum(axis=1), histogram_np.seg_lengths(2, 3, 8))
    A = histogram_np.adjacency(x)
    assert A.sum() == 4 and A[0, 1] == A[1, 2] == A[3, 4] == A[4, 255] == 1
    np.testing.assert_array_equal(histogram_np.downsample(np.array([[255, 255, 9], [255, 254, 9], [1, 1, 1]], dtype=np.uint8)), [[254]])


def test_cli_parsing():
    a = histogram.parse_args(["score", "--data", "D", "--detector", "HCF2C", "--stego-methods", "LSBM", "HILL", "--alphas", "1", ".5", "--simulate",
                              "--out", "s.csv"])
    assert (a.command, a.detector, a.stego_methods, a.alphas, a.simulate, a.split, a.stream, a.batch_size) == (
        "score", "HCF2C", ["LSBM", "HILL"], [1., .5], True, None, 0, 32)
    a = histogram.parse_args(["curve", "--data", "D", "--out", "c.csv"])
    assert (a.command, a.stego_method, a.alpha, a.segments, a.order, a.min_pair, a.threshold) == ("curve", None, None, 100, "rows", 10, .5)
    a = histogram.parse_args(["curve", "--data", "D", "--stego-method", "LSBRS", "--alpha", ".3", "--segments", "50", "--order", "rows_up", "--out", "c.csv"])
    assert (a.stego_method, a.alpha, a.segments, a.order) == ("LSBRS", .3, 50, "rows_up")
    for bad in (["score", "--data", "D", "--detector", "SPAM", "--alphas", "1", "--out", "o"],
                ["score", "--data", "D", "--detector", "HCF", "--out", "o"],                                     # no --alphas
                ["curve", "--data", "D", "--stego-method", "LSBRS", "--out", "o"],                               # a method without its alpha
                ["curve", "--data", "D", "--segments", "0", "--out", "o"],
                ["curve", "--data", "D", "--order", "columns", "--out", "o"]):
        with pytest.raises(SystemExit):
            histogram.parse_args(bad)


def test_error_messages_before_any_gpu_work(tmp_path):
    assert histogram.DETECTORS == ("CHI2", "HCF", "HCFC", "HCF2", "HCF2C") and set(histogram.THRESHOLDS) == set(histogram.DETECTORS)
    with pytest.raises(ValueError, match="unknown detector 'SPAM'"):
        histogram.score(tmp_path, "SPAM", ["LSBR"], [.1])
    with pytest.raises(ValueError, match="unknown detector"):
        histogram.outputs(torch.zeros((1, 4, 4), dtype=torch.uint8), "hcf")
    with pytest.raises(ValueError, match="both stego_method and alpha"):
        histogram.extract(tmp_path, "HCF", "LSBR", None)
    with pytest.raises(ValueError, match="both stego_method and alpha"):
        histogram.curves(tmp_path, None, .1)
    with pytest.raises(ValueError, match="segments=0 outside 1..4096"):
        histogram.curves(tmp_path, segments=0)
    with pytest.raises(ValueError, match="unknown order 'columns'"):
        histogram.curves(tmp_path, order="columns")
    x = torch.zeros((1, 4, 4), dtype=torch.uint8)
    for bad in (0, 4097, 2.5, True):
        with pytest.raises(ValueError, match="outside 1..4096"):
            ops.hist_segments(x, bad)
    with pytest.raises(ValueError, match="unknown order"):
        ops.hist_segments(x, 4, "columns")
    with pytest.raises(Exception, match="CPU tensor"):                 # no CPU fall-back: a missing device is an error
        ops.hist_segments(x, 4)
    with pytest.raises(Exception, match="CPU tensor"):
        ops.adjacency_hist(x)
    with pytest.raises(Exception, match="CPU tensor"):
        ops.downsample2x2(x)


def test_argument_errors_of_the_entries_without_gpu():
    lib = ops._lib.load()
    assert lib.wsu_hist_segments(None, None, 1, 8, 8, 1, 0, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_hist_segments(1, 1, 1, 0, 8, 1, 0, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_hist_segments(1, 1, 1, 65536, 65536, 1, 0, None) == -1 and b"exceed" in lib.wsu_last_error()
    assert lib.wsu_hist_segments(1, 1, 1, 8, 8, 0, 0, None) == -1 and b"segments=0" in lib.wsu_last_error()
    assert lib.wsu_hist_segments(1, 1, 1, 8, 8, 4097, 0, None) == -1 and b"segments=4097" in lib.wsu_last_error()
    assert lib.wsu_hist_segments(1, 1, 1, 8, 8, 4, 2, None) == -1 and b"order=2" in lib.wsu_last_error()
    assert lib.wsu_adjacency_hist(None, None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_adjacency_hist(1, 1, 0, 8, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_adjacency_hist(1, 1, 1, 8, 0, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_downsample2x2(None, None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_downsample2x2(1, 1, 1, 1, 5, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_downsample2x2(1, 1, 1, 5, 1, None) == -1 and b"bad shape" in lib.wsu_last_error()
