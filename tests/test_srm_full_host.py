"""CPU: the host side of the SRM fan submodels and EDGE classes (K54, K55, ws_unet_amd/srm.py `features_fans`, `features_edge`, the
feature sets 'fans', 'edge' and 'full'): the table layouts and their totals, the restatements (srm_fans_np, srm_edge_np) at their edges,
the 8 125 / 9 828 / 34 671 layouts, the invariances that pin every h/v assignment, the singletons' tables, the model file's tag, the
selection channel's refusal, the C entries' argument errors (no GPU call is made) and the CLI parser."""
import itertools

import numpy as np
import pytest
import torch

import srm_edge_np as edge_np
import srm_fans_np as fans_np
import srm_minmax_np as mm_np
import srm_np
from ws_unet_amd import _lib, ops, srm

RESTATED = {"fans": (fans_np, ops.SRM_FAN_TABLES, ops.SRM_FAN_SETS), "edge": (edge_np, ops.SRM_EDGE_TABLES, ops.SRM_EDGE_SETS)}


def _plane(h=24, w=31, seed=7):
    x = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    x[3:14, 5:20] //= 32                                                    # a smooth patch: small residuals, ties of the rounding
    x[16:22, 2:12] = 201
    return x


@pytest.fixture(scope="module")
def restated_counts():
    """the restated counts of the 24 x 31 plane, once"""
    x = _plane()[None]
    out = {"fans": fans_np.counts(x), "edge": edge_np.counts(x)}
    for c in out.values():
        c.setflags(write=False)
    return out


# ---- the table layouts as data --------------------------------------------------------------------------------------------------------

def test_table_layouts_and_dimensions():
    assert len(ops.SRM_FAN_TABLES) == 200 == len(fans_np.TABLES) and len(ops.SRM_EDGE_TABLES) == 132 == len(edge_np.TABLES)
    for ref, tables, sets in RESTATED.values():
        assert [t[:4] for t in tables] == ref.TABLES
        assert [t[4:] for t in tables] == [ref.ab(cls, name, scan) for cls, _, name, scan in ref.TABLES]
        for cls in ref.CLASSES:                                             # the stated reaches are those of the members' taps
            assert list(ref.SETS) == list(sets[cls])
            for name in ref.SETS:
                assert ref.reach(cls, name) == ref.REACH[cls][name] == sets[cls][name], (cls, name)
    assert ops.SRM_FAN_Q2 == {"S1": (2, 4), "S3": (6, 9, 12)} and ops.SRM_EDGE_Q2 == {"E3": (8, 12, 16), "E5": (24, 36, 48)}
    assert ops.SRM_FAN_SET_NAMES == tuple(fans_np.SETS) and len(set(ops.SRM_FAN_SET_NAMES)) == 20
    assert ops.SRM_FAN_TABLES[0] == ("S1", 2, "E+N", "h", 1, 4) and ops.SRM_FAN_TABLES[1] == ("S1", 2, "E+N", "v", 4, 1)
    assert ops.SRM_FAN_TABLES[80] == ("S3", 6, "E+N", "h", 3, 6) and ops.SRM_FAN_TABLES[199] == ("S3", 12, "SW+S+SE+E+NE", "v", 7, 4)
    assert ops.SRM_EDGE_TABLES[0] == ("E3", 8, "U", "h", 1, 5) and ops.SRM_EDGE_TABLES[5] == ("E3", 8, "L", "v", 5, 1)
    assert ops.SRM_EDGE_TABLES[66] == ("E5", 24, "U", "h", 2, 7) and ops.SRM_EDGE_TABLES[131] == ("E5", 48, "UDLR", "v", 7, 4)
    # every fan is a run of adjacent directions on the circle, every pair is perpendicular, and the sets are closed under the image's
    # transposition and mirrors
    circle = list(fans_np.DIRECTIONS)
    for name, m in fans_np.SETS.items():
        if len(m) == 2:
            a, b = (fans_np.DIRECTIONS[k] for k in m)
            assert a[0] * b[0] + a[1] * b[1] == 0 and 0 in a and 0 in b
        else:
            k0 = circle.index(m[0])
            assert list(m) == [circle[(k0 + i) % 8] for i in range(len(m))], name
    for turn in (lambda d: (d[1], d[0]), lambda d: (d[0], -d[1]), lambda d: (-d[0], d[1])):
        turned = {k: next(j for j, e in fans_np.DIRECTIONS.items() if e == turn(d)) for k, d in fans_np.DIRECTIONS.items()}
        assert {frozenset(turned[k] for k in m) for m in fans_np.SETS.values()} == {frozenset(m) for m in fans_np.SETS.values()}
    # the dimensions
    assert (srm.FAN_DIM, srm.EDGE_DIM) == (8125, 9828) == (fans_np.DIM, edge_np.DIM) and len(srm.FAN_BLOCKS) == 25 and len(srm.EDGE_BLOCKS) == 36
    assert srm.FULL_DIMS == {"fans": 8125, "edge": 9828, "full": 34671} and 16718 + 8125 + 9828 == 34671
    assert srm.DIMS == {"linear": 3718, "minmax": 13000, "all": 16718}       # as it was
    assert srm.FAN_SUBMODELS == fans_np.SUBMODELS and srm.EDGE_SUBMODELS == edge_np.SUBMODELS
    assert [b[:3] for b in srm.FAN_BLOCKS[:6]] == [("S1", 2, "pair"), ("S1", 2, "fan3"), ("S1", 2, "fan4h"), ("S1", 2, "fan4v"), ("S1", 2, "fan5"),
                                                    ("S1", 4, "pair")]
    assert [(b[2], b[4]) for b in srm.EDGE_BLOCKS[:6]] == [("spam14h", 169), ("spam14v", 169), ("24", 325), ("22h", 325), ("22v", 325), ("41", 325)]
    assert srm.FAN_BLOCKS[0][3] == tuple(range(8)) and srm.FAN_BLOCKS[2][3] == (16, 18, 20, 22, 25, 27, 29, 31)
    assert srm.EDGE_BLOCKS[0][3] == (0, 2, 5, 7) and srm.EDGE_BLOCKS[3][3] == (16, 19)
    for blocks, n in ((srm.FAN_BLOCKS, 200), (srm.EDGE_BLOCKS, 132)):      # every table in exactly one submodel
        assert sorted(i for b in blocks for i in b[3]) == list(range(n))


@pytest.mark.parametrize("which", RESTATED)
def test_restatement_totals_and_small_images(which):
    ref, tables, _ = RESTATED[which]
    at = {t: i for i, t in enumerate(ref.TABLES)}
    for h, w in ((13, 17), (1, 1), (4, 7), (5, 8), (8, 5), (8, 8), (7, 8)):
        x = np.random.default_rng(h * w).integers(0, 256, (2, h, w), dtype=np.uint8)
        c = ref.counts(x)
        assert c.shape == (2, len(tables), 625) and c.dtype == np.int64
        assert c.sum(axis=2).tolist() == [ref.totals(h, w)] * 2
        assert ref.totals(h, w) == [2 * max(h - t[4], 0) * max(w - t[5], 0) for t in tables]
        # brute force: a run counts when every pixel its set reads at its four positions lies in the image
        for k, (cls, _, name, scan) in enumerate(ref.TABLES):
            taps = [t for member in ref.SETS[name] for t in ref.CLASSES[cls][1][member]]
            step = (0, 1) if scan == "h" else (1, 0)
            runs = sum(all(0 <= r + i * step[0] + dr < h and 0 <= cc + i * step[1] + dc < w for i in range(4) for dr, dc in taps)
                       for r in range(h) for cc in range(w))
            assert ref.totals(h, w)[k] == 2 * runs, (h, w, cls, name, scan)
    widest = ("S3", 6, "SE+E+NE+N+NW") if which == "fans" else ("E5", 24, "UDLR")
    for (h, w), want in (((5, 8), (2, 0)), ((8, 5), (0, 2)), ((8, 8), (8, 8)), ((7, 8), (6, 0)), ((8, 7), (0, 6))):
        assert (ref.totals(h, w)[at[(*widest, "h")]], ref.totals(h, w)[at[(*widest, "v")]]) == want
    assert not any(ref.totals(1, 1))
    # a constant plane: lo = hi = 0 everywhere, both updates in the centre bin
    c = ref.counts(np.full((1, 9, 11), 200, dtype=np.uint8))[0]
    assert c[:, 312].tolist() == ref.totals(9, 11) and c.sum() == sum(ref.totals(9, 11))


def test_restated_residuals_by_hand():
    """one bright pixel: the eight first-order residuals around it, and E3's U, D, L, R at it and beside it"""
    x = np.zeros((1, 7, 7), dtype=np.int64)
    x[0, 3, 3] = 5
    for k, (dr, dc) in fans_np.DIRECTIONS.items():
        R = srm_np.residual(x, fans_np.CLASSES["S1"][1][k])                  # over the centres 1 .. 5 (or 0 .. 6 on the axis it does not move on)
        full = np.zeros((7, 7), dtype=np.int64)
        u, l = max(-dr, 0), max(-dc, 0)
        full[u:u + R.shape[1], l:l + R.shape[2]] = R[0]
        assert full[3, 3] == -5 and full[3 - dr, 3 - dc] == 5 and np.count_nonzero(full) == 2, k
        R3 = srm_np.residual(x, fans_np.CLASSES["S3"][1][k])
        assert sorted(R3[R3 != 0].tolist()) == [-15, -5, 5, 15], k
    for name, at_pixel, above in (("U", -20, 0), ("D", -20, 10), ("L", -20, 10), ("R", -20, 10)):
        taps = edge_np.CLASSES["E3"][1][name]
        assert sum(taps.values()) == 0 and len(taps) == 6
        value = lambda r, c: sum(wt * x[0, r + dr, c + dc] for (dr, dc), wt in taps.items())
        assert value(3, 3) == at_pixel and value(2, 3) == above               # the row above the pixel sees it through a tap below only
    assert len(edge_np.CLASSES["E5"][1]["U"]) == 15 and edge_np.CLASSES["E5"][1]["U"][0, 0] == -12
    assert edge_np.CLASSES["E5"][1]["R"] == {(dc, -dr): wt for (dr, dc), wt in edge_np.CLASSES["E5"][1]["U"].items()}


# ---- features ---------------------------------------------------------------------------------------------------------------------------

def test_features_against_the_restatements(restated_counts):
    for which, features, dim in (("fans", srm.features_fans, 8125), ("edge", srm.features_edge, 9828)):
        ref, tables, _ = RESTATED[which]
        c = np.random.default_rng(2).integers(0, 1000, (3, len(tables), 625)).astype(np.int64)
        c[1, :, :300] = 0
        c[2] = 0
        c[2, :, 312] = 777
        want = ref.features(c)
        for got in (features(c), features(torch.from_numpy(c))):
            assert got.dtype == np.float64 and got.shape == (3, dim)
            np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(features(restated_counts[which]), ref.features(restated_counts[which]))
        for bad in (c[0], c[:, :-1], c[:, :, :624], np.zeros((1, 118, 625), dtype=np.int64)):
            with pytest.raises(ValueError, match="expected"):
                features(bad)
    blocks = srm.features_fans(np.ones((1, 200, 625), dtype=np.int64)).reshape(1, 25, 325)
    np.testing.assert_allclose(blocks.sum(axis=2), 1., rtol=0, atol=1e-12)


def test_features_are_invariant_under_d4_and_negation_of_the_image(restated_counts):
    """transposing the image, mirroring it either way and x -> 255 - x permute the sets, swap lo with hi and reverse the runs, all of
    which the tables' symmetrisation, the submodels' sums and the folds absorb: exactly equal features.  This pins every h/v assignment
    of FAN_SUBMODELS and EDGE_SUBMODELS: swapping the scans of any one table of a submodel breaks it."""
    x = _plane()
    for which, features in (("fans", srm.features_fans), ("edge", srm.features_edge)):
        ref = RESTATED[which][0]
        F = features(restated_counts[which])
        for name, y in (("transpose", x.T), ("left-right", x[:, ::-1]), ("top-bottom", x[::-1]), ("negation", 255 - x)):
            np.testing.assert_array_equal(features(ref.counts(np.ascontiguousarray(y)[None])), F, err_msg=f"{which} {name}")
        assert not np.array_equal(features(ref.counts(np.roll(x, 1, axis=1)[None])), F)
    # ... and a wrong assignment does break it: fan4h with its "horizontal" fans scanned h too is not invariant under transposition
    at = {t: i for i, t in enumerate(fans_np.TABLES)}
    wrong = [at["S1", 2, s, "h"] for s in fans_np.FAN4_VERTICAL + fans_np.FAN4_HORIZONTAL]
    c, ct = restated_counts["fans"], fans_np.counts(np.ascontiguousarray(x.T)[None])
    assert not np.array_equal(c[:, wrong].sum(axis=1) @ srm._MINMAX_FOLD, ct[:, wrong].sum(axis=1) @ srm._MINMAX_FOLD)


def test_singleton_blocks_are_the_plain_tables_folded(restated_counts):
    """an EDGE singleton's min/max table is T + T(negated) of its residual's plain (one update per run) table, so the spam14 blocks equal
    the blocks made from the plain tables, folded over sign and reversal the same way"""
    x = _plane()[None]
    plain = edge_np.counts(x, plain=True)
    two = restated_counts["edge"]
    at = {t: i for i, t in enumerate(edge_np.TABLES)}
    for cls, q2 in (("E3", 8), ("E5", 48)):
        for s in "UDLR":
            for scan in "hv":
                k = at[cls, q2, s, scan]
                np.testing.assert_array_equal(two[0, k], plain[0, k] + plain[0, k][::-1])        # bin 624 - b holds the negated digits
                R = srm_np.residual(x.astype(np.int64), edge_np.CLASSES[cls][1][s])
                np.testing.assert_array_equal(plain[0, k], srm_np.table(srm_np.digit(R, q2), scan)[0])
    F = srm.features_edge(two).reshape(-1)
    offset = 0
    for cls, q2, name, tabs, orbits in srm.EDGE_BLOCKS:
        if name.startswith("spam14"):
            block = srm_np.fold(plain[0, list(tabs)].sum(axis=0))
            np.testing.assert_array_equal(F[offset:offset + 169], (2 * block).astype(np.float64) / float(2 * block.sum()))
            np.testing.assert_array_equal(F[offset:offset + 169], block.astype(np.float64) / float(block.sum()))
        offset += orbits
    assert offset == 9828


def test_features_refuse_a_submodel_without_a_run():
    c = np.ones((2, 200, 625), dtype=np.int64)
    fan5 = next(b for b in srm.FAN_BLOCKS if b[:3] == ("S3", 6, "fan5"))
    c[1, list(fan5[3])] = 0
    with pytest.raises(ValueError, match="image 1.*S3.*q2=6.*fan5"):
        srm.features_fans(c)
    c[1, fan5[3][0]] = 1                                                     # one of the submodel's tables is enough
    assert srm.features_fans(c).shape == (2, 8125)
    c = np.ones((2, 132, 625), dtype=np.int64)
    c[0, [b for b in srm.EDGE_BLOCKS if b[:3] == ("E5", 36, "22v")][0][3]] = 0
    with pytest.raises(ValueError, match="image 0.*E5.*q2=36.*22v"):
        srm.features_edge(c)
    for ref, features in ((fans_np, srm.features_fans), (edge_np, srm.features_edge)):
        small = ref.counts(np.zeros((1, 4, 30), dtype=np.uint8))               # four rows: no vertical run of a wide set
        with pytest.raises(ValueError, match="image 0"):
            features(small)
        with pytest.raises(ValueError, match="without a run"):
            ref.features(small)


# ---- the drivers' logic ---------------------------------------------------------------------------------------------------------------

def test_feature_set_lookups():
    assert srm._COUNTS == {"linear": ("srm_counts",), "minmax": ("srm_minmax_counts",), "all": ("srm_counts", "srm_minmax_counts")}
    assert set(srm._FEATURES) == {"srm_counts", "srm_minmax_counts"} and set(srm.FEATURE_SETS) == {"linear", "minmax", "all"}
    assert srm._feature_set("linear") == ("srm-linear", 3718, ("srm_counts",)) and srm._feature_set("all")[1:] == (16718, srm._COUNTS["all"])
    assert srm._feature_set("fans") == ("srm-fans", 8125, ("srm_fan_counts",)) and srm._feature_set("edge") == ("srm-edge", 9828, ("srm_edge_counts",))
    assert srm._feature_set("full") == ("srm-full", 34671, ("srm_counts", "srm_minmax_counts", "srm_fan_counts", "srm_edge_counts"))
    assert srm._feature_set("full")[2][:2] == srm._COUNTS["all"]             # 'full' begins with 'all': the same entries in the same order
    assert srm._features_of("srm_counts") is srm.features and srm._features_of("srm_fan_counts") is srm.features_fans
    assert list(srm.TAGS) == ["linear", "minmax", "all", "fans", "edge", "full"] and len(set(srm.TAGS.values())) == 6
    for sub in ("fans", "edge", "full"):
        assert srm.FLD(0.1, sub).dual and srm.Ensemble(3, 5, submodels=sub).submodels == sub
    with pytest.raises(ValueError, match="unknown submodels"):
        srm.FLD(submodels="fan")
    with pytest.raises(ValueError, match="unknown submodels"):
        srm.extract("nowhere", submodels="everything")


def test_full_begins_with_all_byte_for_byte(monkeypatch, tmp_path):
    """`extract` on a data set of two small images with the count entries replaced by the restatements (no GPU): 'full' is 'all', then
    'fans', then 'edge', and only the entries a set needs run"""
    import pandas as pd
    from PIL import Image
    (tmp_path / "images").mkdir()
    rng = np.random.default_rng(21)
    planes = {}
    for k in (1, 2):
        planes[f"{k}.png"] = rng.integers(0, 256, (16, 24), dtype=np.uint8)
        Image.fromarray(planes[f"{k}.png"], mode="L").save(tmp_path / "images" / f"{k}.png")
    (tmp_path / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,16,24\n" for k in (1, 2)))
    ran = []
    restated = {"srm_counts": srm_np.counts, "srm_minmax_counts": mm_np.counts, "srm_fan_counts": fans_np.counts, "srm_edge_counts": edge_np.counts}
    for entry, fn in restated.items():
        monkeypatch.setattr(ops, entry, lambda x, entry=entry, fn=fn: (ran.append(entry), torch.from_numpy(fn(x.cpu().numpy())))[1])
    from ws_unet_amd import planes as planes_module
    monkeypatch.setattr(planes_module, "upload_planes", lambda p, device: p.clone())
    rows, full = srm.extract(tmp_path, submodels="full", batch_size=1)
    assert full.shape == (2, 34671) and sorted(set(ran)) == sorted(restated)
    del ran[:]
    _, every = srm.extract(tmp_path, submodels="all", batch_size=1)
    assert set(ran) == {"srm_counts", "srm_minmax_counts"}
    assert full[:, :16718].tobytes() == every.tobytes()
    del ran[:]
    _, fans = srm.extract(tmp_path, submodels="fans")
    assert set(ran) == {"srm_fan_counts"} and full[:, 16718:16718 + 8125].tobytes() == fans.tobytes()
    _, edge = srm.extract(tmp_path, submodels="edge")
    assert full[:, 16718 + 8125:].tobytes() == edge.tobytes()
    assert isinstance(rows, pd.DataFrame) and len(rows) == 2


def test_model_tag_round_trip_and_refusal(tmp_path):
    rng = np.random.default_rng(5)
    paths = {}
    for sub, tag, d in (("fans", "srm-fans", 8125), ("edge", "srm-edge", 9828), ("full", "srm-full", 34671), ("all", "srm-all", 16718)):
        m = srm.FLD(0.2, sub).fit(rng.random((5, d)), rng.random((4, d)) + 0.01)
        m.stego_methods, m.alphas = ["WOW"], [0.4]
        paths[sub] = tmp_path / f"{sub}.npz"
        m.save(paths[sub])
        with np.load(paths[sub], allow_pickle=False) as z:
            assert str(z["features"]) == tag and z["w"].shape == (d,)
        for r in (srm.load(paths[sub]), srm.load(paths[sub], sub), srm.load_model(paths[sub], sub)):
            assert r.submodels == sub and r.dual and (r.ridge, r.stego_methods, r.alphas) == (0.2, ["WOW"], [0.4])
            np.testing.assert_array_equal(r.w, m.w)
    for have, asked in itertools.permutations(paths, 2):
        with pytest.raises(ValueError, match=f"not a model on the 'srm-{asked}' features but on 'srm-{have}'"):
            srm.load(paths[have], asked)
    with pytest.raises(ValueError, match="'srm-fans' features, not on 'srm-full'"):           # before any file of the data set is read
        srm.score(tmp_path / "no_data", srm.load(paths["fans"]), ["LSBR"], [0.1], submodels="full")
    with pytest.raises(ValueError, match="'srm-full' features, not on 'srm-linear'"):
        srm.score(tmp_path / "no_data", srm.load(paths["full"]), ["LSBR"], [0.1])
    with pytest.raises(ValueError, match="34671"):
        srm.FLD(0.1, "full").fit(rng.random((3, 16718)), rng.random((3, 16718)))
    short = srm.load(paths["edge"])
    short.w = short.w[:3718]
    short.save(tmp_path / "short.npz")
    with pytest.raises(ValueError, match="3718 weights, expected 9828"):
        srm.load(tmp_path / "short.npz")
    # the ensemble carries the same tags
    X0, X1 = rng.random((12, 8125)), rng.random((12, 8125)) + 0.05
    with pytest.raises(ValueError, match=r"\(n, 8125\)"):
        srm.Ensemble(3, 5, submodels="fans").fit(X0[:, :100], X1[:, :100])


def test_selection_channel_is_refused():
    for sub in ("fans", "edge", "full"):
        with pytest.raises(ValueError, match=f"'linear' only, not '{sub}'"):
            srm.FLD(0.1, sub, selection_channel="HILL", sc_alpha=0.4)
        with pytest.raises(ValueError, match=f"'linear' only, not '{sub}'"):
            srm.extract("nowhere", submodels=sub, selection_channel="WOW", sc_alpha=0.2)
        with pytest.raises(ValueError, match=f"'linear' only, not '{sub}'"):
            srm.fit("nowhere", ["WOW"], [0.2], submodels=sub, selection_channel="WOW")
        with pytest.raises(ValueError, match=f"'linear' only, not '{sub}'"):
            srm.main(["fit", "--data", "nowhere", "--alphas", ".4", "--submodels", sub, "--selection-channel", "HILL", "--out", "m.npz"])


# ---- the C entries' argument errors: errno-style code + message before any HIP call ------------------------------------------------------

@pytest.mark.parametrize("entry", ["srm_fan_counts", "srm_edge_counts"])
def test_c_entry_rejects_bad_arguments_without_a_gpu(entry):
    assert _lib.SIGNATURES["wsu_" + entry] == _lib.SIGNATURES["wsu_srm_minmax_counts"]
    lib = _lib.load()
    err = lib.wsu_last_error

    def call(x=8, counts=8, n=1, h=8, w=8):
        return getattr(lib, "wsu_" + entry)(x, counts, n, h, w, None)
    assert call(x=None) == -1 and b"null" in err() and entry.encode() in err()
    assert call(counts=None) == -1 and b"null" in err()
    assert call(n=0) == -1 and b"bad shape" in err()
    assert call(n=65536) == -1 and b"bad shape" in err()
    assert call(h=0) == -1 and b"bad shape" in err()
    assert call(w=0) == -1 and b"bad shape" in err()
    assert call(h=2 ** 31 - 1, w=2 ** 31 - 1) == -1 and b"too many tiles" in err()
    with pytest.raises(_lib.WsuError, match="CPU tensor"):                   # a valid call gets as far as the device check
        getattr(ops, entry)(torch.zeros((1, 8, 8), dtype=torch.uint8))


def test_cli_parser_takes_the_new_sets():
    assert srm.parse_args(["fit", "--data", "d", "--alphas", ".4", "--out", "m.npz"]).submodels == "linear"
    for sub in ("fans", "edge", "full"):
        a = srm.parse_args(["fit", "--data", "d", "--alphas", ".4", "--submodels", sub, "--simulate", "--stego-methods", "WOW", "--out", "m.npz"])
        assert (a.submodels, a.simulate, a.stego_methods) == (sub, True, ["WOW"])
        for cmd in (["score", "--model", "m.npz"], ["features"]):
            assert srm.parse_args(cmd + ["--data", "d", "--alphas", ".1", "--submodels", sub, "--out", "o"]).submodels == sub
    a = srm.parse_args(["fit", "--data", "d", "--alphas", ".4", "--submodels", "full", "--classifier", "ensemble", "--d-sub", "300", "--out", "m.npz"])
    assert a.classifier_kw["classifier"] == "ensemble" and a.classifier_kw["d_sub"] == [300]
    with pytest.raises(SystemExit):
        srm.parse_args(["fit", "--data", "d", "--alphas", ".4", "--submodels", "fan", "--out", "m.npz"])
