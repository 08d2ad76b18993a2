"""CPU: the host half of the FLD ensemble (ws_unet_amd.ensemble) against the numpy restatement (ensemble_np): threshold search, out-of-bag
tally, votes, draws, files, loaders, the drivers' argument rules and the C entry's argument check."""
import numpy as np
import pytest

import ensemble_np as enp
from ws_unet_amd import _lib, ensemble, spam, srm


# ---- threshold ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(8))
def test_threshold_equals_the_brute_force(seed):
    """small weighted samples on a coarse grid (many tied projections, tied costs), rows of weight 0 whose projections are no candidates"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(4, 40))
    p = rng.integers(-4, 5, n).astype(np.float64) / 4.
    y = rng.integers(0, 2, n)
    y[:2] = (0, 1)
    wt = rng.integers(0, 4, n)
    wt[:2] = np.maximum(wt[:2], 1)
    p[1] = p[0] + 0.25                                                      # at least two distinct projections in the bag
    got, want = ensemble.threshold(p, y, wt), enp.threshold(p, y, wt)
    assert got == want
    assert got not in set(p[wt > 0].tolist())                                # a midpoint, never a projection of the bag


def test_threshold_ties_go_to_the_lowest_candidate_and_weights_count():
    p = np.array([0., 1., 2., 3.])
    y = np.array([0, 1, 0, 1])
    assert ensemble.threshold(p, y, np.ones(4, dtype=int)) == 0.5            # 0.5 and 2.5 both cost 1/4; 1.5 costs 1/2
    assert ensemble.threshold(p, y, np.array([1, 1, 5, 1])) == 2.5           # the cover at 2 now weighs more than the stego at 1
    assert ensemble.threshold(p, y, np.array([1, 0, 1, 1])) == 2.5           # the stego at 1 is out of the bag
    assert ensemble.threshold(np.array([7., 7.]), np.array([0, 1]), np.array([1, 1])) == 7.
    with pytest.raises(ValueError, match="no weight"):
        ensemble.threshold(p, y, np.array([1, 0, 1, 0]))


# ---- out-of-bag -----------------------------------------------------------------------------------------------------------------------

def test_oob_tally_on_a_hand_made_table():
    #            learner 0  1  2  3
    votes = np.array([[0, 0, 1, 1],     # cover, out of 0,1,2: 1 of 3 stego -> right
                      [1, 1, 0, 0],     # cover, out of 0,1  : 2 of 2 stego -> wrong
                      [1, 0, 1, 1],     # stego, out of 0,1  : tie          -> half
                      [0, 0, 0, 0],     # stego, in every bag: not judged
                      [0, 1, 1, 1]],    # stego, out of 3    : right
                     dtype=bool)
    in_bag = np.array([[0, 0, 0, 1], [0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 0]], dtype=bool)
    y = np.array([0, 0, 1, 1, 1])
    want = ((0 + 1) / 2 + (0.5 + 0) / 2) / 2
    assert ensemble.oob_error(votes, in_bag, y) == want == enp.oob_error(votes, in_bag, y)
    assert ensemble.oob_error(votes[:2], in_bag[:2], y[:2]) == (0.5 + 0.5) / 2      # no stego row at all: that class counts 1/2


@pytest.mark.parametrize("seed", range(3))
def test_oob_equals_the_restatement(seed):
    rng = np.random.default_rng(seed)
    votes, in_bag, y = rng.random((30, 6)) < 0.5, rng.random((30, 6)) < 0.6, rng.integers(0, 2, 30)
    assert ensemble.oob_error(votes, in_bag, y) == enp.oob_error(votes, in_bag, y)


# ---- votes and output -----------------------------------------------------------------------------------------------------------------

def _given_model(cls=ensemble.Ensemble, d=12, L=5, ds=4, **kw):
    rng = np.random.default_rng(5)
    m = cls(L, ds, 0.1, 3, **kw)
    m.idx = np.stack([np.sort(rng.permutation(d)[:ds]) for _ in range(L)]).astype(np.int32)
    m.w, m.b, m.mean = rng.standard_normal((L, ds)), rng.standard_normal(L) / 4., rng.standard_normal(d)
    m.d_sub_chosen, m.oob_error, m.oob_errors = ds, 0.125, [0.125]
    m.stego_methods, m.alphas = ["LSBM"], [0.4]
    return m


def test_votes_and_output_from_given_learners():
    m = _given_model()
    F = np.random.default_rng(6).standard_normal((40, 12))
    want = enp.votes(F, m.mean, m.idx, m.w, m.b)
    np.testing.assert_array_equal(m.votes(F), want)
    assert m.votes(F).dtype == np.int64 and len(set(want.tolist())) > 2
    np.testing.assert_array_equal(m.output(F), want / 5.)
    with pytest.raises(ValueError, match=r"\(N, 12\)"):
        m.votes(F[:, :11])
    with pytest.raises(ValueError, match="not fitted"):
        ensemble.Ensemble(5, 4).votes(F)
    assert not hasattr(m, "log_odds")


def test_constructor_rules():
    assert ensemble.Ensemble(d_sub=7).learners == 51 and ensemble.Ensemble(d_sub=7).ridge == 0.1 and ensemble.Ensemble(d_sub=[7, 9]).d_sub == [7, 9]
    for kw in (dict(), dict(d_sub=0), dict(d_sub=[3, -1]), dict(d_sub=[]), dict(d_sub=3, learners=0), dict(d_sub=3, ridge=-1.)):
        with pytest.raises(ValueError):
            ensemble.Ensemble(**kw)


# ---- draws ----------------------------------------------------------------------------------------------------------------------------

def test_draws_are_the_restatement_s_and_repeat():
    group, n_groups = ensemble.row_groups(6, 12)
    np.testing.assert_array_equal(group, np.tile(np.arange(6), 3))
    assert (group, n_groups)[1] == enp.groups(6, 12)[1] and np.array_equal(group, enp.groups(6, 12)[0])
    a = ensemble.draws(4, 30, [5, 9], 7, group, n_groups, 6)
    b = ensemble.draws(4, 30, [5, 9], 7, group, n_groups, 6)
    want = enp.draws(4, 30, [5, 9], 7, group, n_groups, 6)
    for (idx, c), (idx2, c2), (idx3, c3) in zip(a, b, want):
        np.testing.assert_array_equal(idx, idx2), np.testing.assert_array_equal(c, c2)
        np.testing.assert_array_equal(idx, idx3), np.testing.assert_array_equal(c, c3)
        assert (np.diff(idx, axis=1) > 0).all() and idx.min() >= 0 and idx.max() < 30          # sorted, distinct
        assert (c.sum(axis=1) == n_groups).all()
    assert a[0][0].shape == (7, 5) and a[1][0].shape == (7, 9) and a[0][1].shape == (7, 6)
    assert not np.array_equal(a[0][0], ensemble.draws(5, 30, [5, 9], 7, group, n_groups, 6)[0][0])


def test_groups_enter_a_bag_together():
    g0, g1 = np.array([10, 20, 30, 40]), np.array([40, 30, 20, 10, 10, 20, 30, 40])
    group, n_groups = ensemble.row_groups(4, 8, g0, g1)
    assert n_groups == 4 and group.tolist() == [0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3]
    for _, c in ensemble.draws(0, 9, [3], 20, group, n_groups, 4):
        wt = c[:, group]
        for g in range(4):
            assert (wt[:, group == g] == c[:, g:g + 1]).all()               # a cover and its twins carry their group's count
    # rows that cannot be paired by position: every row its own group
    group, n_groups = ensemble.row_groups(3, 4)
    assert n_groups == 7 and group.tolist() == list(range(7)) and enp.groups(3, 4)[0].tolist() == list(range(7))
    with pytest.raises(ValueError, match="neither"):
        ensemble.row_groups(3, 4, np.arange(3))
    with pytest.raises(ValueError, match="one integer per row"):
        ensemble.row_groups(3, 4, np.arange(3), np.arange(5))


def test_a_draw_with_an_empty_class_is_redrawn():
    """one cover group against many stego groups: most bootstrap samples miss the cover, and every kept draw has both classes"""
    group, n_groups = ensemble.row_groups(1, 7, np.array([0]), np.arange(1, 8))
    (idx, c), = ensemble.draws(11, 6, [2], 12, group, n_groups, 1)
    (idx_np, c_np), = enp.draws(11, 6, [2], 12, group, n_groups, 1)
    assert (c[:, 0] > 0).all() and (c[:, 1:].sum(axis=1) > 0).all()
    np.testing.assert_array_equal(idx, idx_np), np.testing.assert_array_equal(c, c_np)
    # the stream was used for the rejected draws too: the plain sequence without the rule differs
    rng = np.random.Generator(np.random.Philox(key=11))
    plain = [(np.sort(rng.permutation(6)[:2]), np.bincount(rng.integers(0, 8, 8), minlength=8)) for _ in range(12)]
    assert any(p[1][0] == 0 for p in plain) and not all(np.array_equal(p[1], cc) for p, cc in zip(plain, c))


# ---- files ----------------------------------------------------------------------------------------------------------------------------

def test_save_load_round_trip_is_byte_equal(tmp_path):
    m = _given_model()
    m.save(tmp_path / "a.npz")
    with np.load(tmp_path / "a.npz", allow_pickle=False) as z:
        assert str(z["classifier"]) == "ensemble"
        assert {"classifier", "idx", "w", "b", "mean", "d_sub", "oob_error", "oob_errors", "learners", "ridge", "seed"} <= set(z.files)
        assert all(z[k].dtype != object for k in z.files)
    r = ensemble.Ensemble.load(tmp_path / "a.npz")
    for k in ("idx", "w", "b", "mean"):
        got, want = getattr(r, k), getattr(m, k)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert (r.learners, r.d_sub, r.d_sub_chosen, r.ridge, r.seed, r.oob_error, r.oob_errors) == (5, [4], 4, 0.1, 3, 0.125, [0.125])
    assert (r.stego_methods, r.alphas) == (["LSBM"], [0.4])
    r.save(tmp_path / "b.npz")
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
    with pytest.raises(ValueError, match="not fitted"):
        ensemble.Ensemble(5, 4).save(tmp_path / "c.npz")


def _fld_files(tmp_path):
    f = spam.FLD()
    f.w, f.b = np.arange(686, dtype=np.float64), 0.25
    f.save(tmp_path / "spam_fld.npz")
    g = srm.FLD(submodels="linear")
    g.w, g.b = np.arange(srm.DIM, dtype=np.float64), 0.5
    g.save(tmp_path / "srm_fld.npz")
    return f, g


def test_fld_load_refuses_an_ensemble_file_and_load_model_dispatches(tmp_path):
    f, g = _fld_files(tmp_path)
    _given_model(spam.Ensemble, d=686).save(tmp_path / "spam_ens.npz")
    _given_model(srm.Ensemble, d=srm.DIM).save(tmp_path / "srm_ens.npz")
    for mod, name in ((spam, "spam_ens.npz"), (srm, "srm_ens.npz")):
        with pytest.raises(ValueError, match="ensemble.*load_model"):
            mod.FLD.load(tmp_path / name)
    with pytest.raises(ValueError, match="ensemble.*load_model"):
        srm.FLD.load(tmp_path / "srm_ens.npz", selection_channel="HILL", sc_alpha=0.4)
    # an FLD file: what it did
    r = spam.FLD.load(tmp_path / "spam_fld.npz")
    assert np.array_equal(r.w, f.w) and r.b == 0.25
    assert np.array_equal(srm.FLD.load(tmp_path / "srm_fld.npz").w, g.w)
    # load_model
    a, b = spam.load_model(tmp_path / "spam_fld.npz"), spam.load_model(tmp_path / "spam_ens.npz")
    assert type(a) is spam.FLD and type(b) is spam.Ensemble and (b.order, b.T, b.normalise) == (2, 3, "joint")
    c, e = srm.load_model(tmp_path / "srm_fld.npz"), srm.load_model(tmp_path / "srm_ens.npz", "linear")
    assert type(c) is srm.FLD and type(e) is srm.Ensemble and e.submodels == "linear" and e.sc is None
    with np.load(tmp_path / "srm_ens.npz") as z:
        assert str(z["features"]) == "srm-linear" and [int(v) for v in z["q2_S1"]] == [2, 4]
    with pytest.raises(ValueError, match="not an ensemble"):
        srm.Ensemble.load(tmp_path / "srm_fld.npz")
    with pytest.raises(ValueError, match="srm-minmax"):
        srm.load_model(tmp_path / "srm_ens.npz", "minmax")
    with pytest.raises(ValueError, match="selection channel"):
        srm.load_model(tmp_path / "srm_ens.npz", selection_channel="HILL", sc_alpha=0.4)


def test_an_ensemble_with_a_selection_channel_keeps_its_tag(tmp_path):
    m = _given_model(srm.Ensemble, d=srm.DIM, selection_channel="HILL", sc_alpha=0.4)
    m.save(tmp_path / "sc.npz")
    with np.load(tmp_path / "sc.npz") as z:
        assert str(z["features"]) == "srm-linear-sc" and str(z["sc_cost"]) == "HILL"
    r = srm.load_model(tmp_path / "sc.npz", "linear", "HILL", 0.4)
    assert r.sc == ("HILL", 0.4, "{}")
    assert srm.load_model(tmp_path / "sc.npz", selection_channel="HILL").sc == r.sc
    for kw in (dict(), dict(selection_channel="WOW", sc_alpha=0.4), dict(selection_channel="HILL", sc_alpha=0.2)):
        with pytest.raises(ValueError, match="HILL"):
            srm.load_model(tmp_path / "sc.npz", **kw)


def test_srm_score_refuses_an_ensemble_on_another_feature_set(tmp_path):
    """the checks come before any file is read or anything is launched"""
    m = _given_model(srm.Ensemble, d=srm.DIM)
    with pytest.raises(ValueError, match="'srm-linear' features, not on 'srm-all'"):
        srm.score(tmp_path, m, ["LSBM"], [0.4], submodels="all")
    with pytest.raises(ValueError, match="no selection channel"):
        srm.score(tmp_path, m, ["LSBM"], [0.4], selection_channel="HILL")
    with pytest.raises(ValueError, match=rf"\(n, {srm.DIMS['all']}\)"):
        srm.Ensemble(5, 4, submodels="all").fit(np.zeros((3, srm.DIM)), np.zeros((3, srm.DIM)))


# ---- the CLI's argument rules -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mod", [spam, srm])
def test_cli_argument_rules(mod, capsys):
    common = ["--data", "D", "--alphas", "0.4", "--out", "m.npz"]
    a = mod.parse_args(["fit", *common])
    assert (a.classifier, a.learners, a.d_sub, a.seed, a.ridge, a.classifier_kw) == ("fld", 51, None, 0, 0.1, {})
    a = mod.parse_args(["fit", *common, "--classifier", "ensemble", "--d-sub", "200", "400", "--learners", "11", "--seed", "3"])
    assert a.classifier_kw == dict(classifier="ensemble", learners=11, d_sub=[200, 400], seed=3)
    with pytest.raises(SystemExit):
        mod.parse_args(["fit", *common, "--classifier", "ensemble"])
    assert "--d-sub" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mod.parse_args(["fit", *common, "--classifier", "forest"])
    assert mod.parse_args(["score", *common, "--model", "m.npz"]).classifier_kw == {}
    with pytest.raises(ValueError, match="d_sub"):
        mod.fit("D", ["LSBM"], [0.4], classifier="ensemble")
    with pytest.raises(ValueError, match="unknown classifier"):
        mod.fit("D", ["LSBM"], [0.4], classifier="forest", d_sub=3)


def test_stem_groups():
    g0, g1 = ensemble.stem_groups(["images/b.png", "images/a.png"], ["stego_X/a.png", "stego_X/b.png", "stego_Y/a.png"])
    assert g0.tolist() == [1, 0] and g1.tolist() == [0, 1, 0]


# ---- the C entry ----------------------------------------------------------------------------------------------------------------------

def test_c_entry_checks_its_arguments_without_a_device():
    lib = _lib.load()
    assert _lib.SIGNATURES["wsu_subspace_gram_f64"][1][:4] == [_lib.c_void_p] * 4
    for args in ((None, 1, 1, 1), (1, None, 1, 1), (1, 1, None, 1), (1, 1, 1, None)):
        assert lib.wsu_subspace_gram_f64(*args, 4, 4, 2, 1, None) == -1 and b"null" in lib.wsu_last_error()
    for shape in ((0, 4, 2, 1), (4, 0, 2, 1), (4, 4, 0, 1), (4, 4, 2, 0), (-1, 4, 2, 1), (4, 4, 2, 65536)):
        assert lib.wsu_subspace_gram_f64(1, 1, 1, 1, *shape, None) == -1 and b"subspace_gram_f64" in lib.wsu_last_error()
    assert lib.wsu_mfma_f64_loop(None, 1, 1, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_mfma_f64_loop(1, 0, 1, None) == -1 and b"bad shape" in lib.wsu_last_error()
