"""CPU: the host half of the ae_boxes table (ws_unet_amd/error_boxes.py) -- subset draws, slice arithmetic from counts, the filter
exactness rule, quantile interpolation, the IQR clip, the output layout and the CLI arguments.  No GPU."""
import numpy as np
import pandas as pd
import pytest

import boxes_np
from ws_unet_amd import error_boxes, fabrika, filters


@pytest.mark.parametrize("shape", [(510, 510, 1), (20, 7, 1), (260100, 1), (13, 9)])
@pytest.mark.parametrize("size", [None, 0, 1, 1000])
def test_subset_residual_matches_the_reference_formula(shape, size):
    resid = np.random.default_rng(3).standard_normal(shape)
    fname = "../data/images/10.png"
    got = error_boxes.subset_residual(resid, fname, size)
    if size:
        rng = np.random.default_rng(fabrika.filename_to_image_seed(fname))
        selected = rng.integers(resid.size, size=size)
        selected = (selected // resid.shape[1], selected % resid.shape[1])
        want = resid[selected]
        # the flat interior indices the kernel reads give the same values, in draw order
        flat = resid.reshape(resid.shape[0], resid.shape[1], -1)[..., 0].reshape(-1)
        assert np.array_equal(flat[error_boxes.subset_indices(fname, resid.size, size)], want.reshape(-1))
    else:
        want = resid.flatten()
    assert np.array_equal(got, want)


def _ref_slices(a, edges):
    """The ranks the reference's slicing selects: argsort, argmin(... <= e) - 1, Python slices of the rank vector."""
    s = np.sort(a, kind="stable")
    cuts = [0] + [np.argmin(s <= e) - 1 for e in edges] + [len(a)]
    ranks = np.arange(len(a))
    return [ranks[cuts[j]:cuts[j + 1]] for j in range(len(cuts) - 1)]


@pytest.mark.parametrize("seed", range(40))
def test_slice_ranges_equal_argsort_slicing(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    kind = seed % 5
    if kind == 0:
        a = rng.integers(0, 40, n) / 4.0                      # KB-like quarters, ties, values at the edges
    elif kind == 1:
        a = rng.uniform(0.6, 30, n)                           # nothing <= 0.5: overlapping slices
    elif kind == 2:
        a = rng.uniform(0, 7.5, n)                            # everything <= 7.5: a one-element last slice
    elif kind == 3:
        a = np.full(n, 2.0)                                   # empty slices
    else:
        a = rng.choice([0.5, 1.5, 3.5, 7.5, 8.0], n)
    counts = [int((a <= e).sum()) for e in error_boxes.EDGE_VALUES]
    got = error_boxes.slice_ranges(counts, n)
    want = _ref_slices(a, error_boxes.EDGE_VALUES)
    assert [list(range(s, t)) for s, t in got] == [w.tolist() for w in want]


def test_slice_ranges_degenerate_cases():
    assert error_boxes.slice_ranges([0, 0, 5, 10], 10) == [(0, 9), (9, 9), (9, 4), (4, 9), (9, 10)]
    assert error_boxes.slice_ranges([10, 10, 10, 10], 10) == [(0, 9), (9, 9), (9, 9), (9, 9), (9, 10)]
    assert error_boxes.slice_ranges([3, 5, 7, 8], 10) == [(0, 2), (2, 4), (4, 6), (6, 7), (7, 10)]
    assert error_boxes.slice_ranges([1], 1) == [(0, 0), (0, 1)]


def test_filter_exactness_rule():
    for name in ("KB", "AVG"):
        t = error_boxes.filter_taps(filters.NAMED_FILTERS[name])
        assert t.shape == (9,) and t[4] == 0.0
        t2 = error_boxes.filter_taps(filters.NAMED_FILTERS_2D[name])
        assert np.array_equal(t, t2)
    with pytest.raises(ValueError, match="not exact"):
        error_boxes.filter_taps(filters.NAMED_FILTERS_2D["AVG9"])           # 1/9
    with pytest.raises(ValueError, match="not exact"):
        error_boxes.filter_taps(np.full((8, 1), 2.0))                       # 255 * 17 >= 2^12
    with pytest.raises(ValueError, match="not exact"):
        error_boxes.filter_taps(np.full((8, 1), 2.0 ** -13))
    error_boxes.filter_taps(np.full((8, 1), 2.0 ** -12))
    error_boxes.filter_taps(np.array([1.5, -1, 2, 0.25, 0, 0, 0, 0.125]))   # 255 * 5.875 < 2^12


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 10, 101, 1000])
def test_lerp_and_quantile_index_equal_numpy(n):
    from ws_unet_amd.hill import quantile_index
    v = np.sort(np.random.default_rng(n).uniform(0, 50, n).astype(np.float32).astype(np.float64))
    for q in error_boxes.QUANTILES:
        k, g = quantile_index(n, q)
        got = error_boxes.lerp(v[k], v[min(k + 1, n - 1)], g)
        assert got == np.quantile(v, q) == pd.Series(v).quantile(q)


def test_iqr_clip_equals_the_reference():
    for seed in range(20):
        s = pd.Series(np.random.default_rng(seed).exponential(3, 50).round(2))
        lo, hi = error_boxes.iqr_interval(s.quantile(.25), s.quantile(.75), s.min(), s.max())
        assert lo == boxes_np.iqr_interval(.25, sign=-1.5)(s)
        assert hi == boxes_np.iqr_interval(.75, sign=1.5)(s)
    assert error_boxes.iqr_interval(1.0, 3.0, 0.5, 10.0) == (0.5, 6.0)
    assert error_boxes.iqr_interval(1.0, 3.0, -5.0, 4.0) == (-2.0, 4.0)


def test_labels_columns_and_row_order():
    assert error_boxes.edge_labels() == ["0-0.5", "0.5-1.5", "1.5-3.5", "3.5-7.5", "7.5-inf"]
    assert error_boxes.edge_labels([1, 2.5]) == ["0-1", "1-2.5", "2.5-inf"]
    rows = {t: [{"Type": t, "edge_interval": lab, **{c: float(i) for i, c in enumerate(error_boxes.STATS)}}
                for lab in error_boxes.edge_labels()[::-1]] for t in ("UNet_l1ws", "KB", "AVG", "UNet_l1")}
    df = error_boxes._frame(rows)
    assert list(df.columns) == list(error_boxes.COLUMNS)
    assert list(zip(df["edge_interval"], df["Type"]))[:5] == [("0-0.5", "AVG"), ("0-0.5", "KB"), ("0-0.5", "UNet_l1"),
                                                             ("0-0.5", "UNet_l1ws"), ("0.5-1.5", "AVG")]
    assert df.to_csv(index=False).splitlines()[0] == "Type,edge_interval,min,q_25_iqr,q_25,q_50,q_75,q_75_iqr,max"
    # the restatement's layout is the same
    a = np.arange(40) / 4.0
    ref = boxes_np.table({"KB": a, "AVG": a[::-1]}, "KB")
    assert list(ref.columns) == list(error_boxes.COLUMNS)
    assert list(zip(ref["edge_interval"], ref["Type"])) == [(lab, t) for lab in error_boxes.edge_labels() for t in ("AVG", "KB")]


def test_cli_arguments():
    a = error_boxes.parse_args(["--data", "d", "--out", "o.csv"])
    assert (a.data, a.out, a.model_dir, a.num_pixels, a.take_num_images, a.mode, a.split) == ("d", "o.csv", None, None, None, None,
                                                                                            "split_te.csv")
    a = error_boxes.parse_args(["--data", "d", "--out", "o.csv", "--model-dir", "m", "--num-pixels", "1000", "--take-num-images", "3",
                                "--mode", "f32"])
    assert (a.model_dir, a.num_pixels, a.take_num_images, a.mode) == ("m", 1000, 3, "f32")
    with pytest.raises(SystemExit):
        error_boxes.parse_args(["--out", "o.csv"])
