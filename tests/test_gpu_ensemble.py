"""GPU: the float64 subspace Gram kernel (K53, ops.subspace_gram) exactly on integer data and within the rounding bound of a product sum
on real data, against the numpy restatement (ensemble_np); the base learners, the fit and the drivers of the FLD ensemble."""
import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

from conftest import GOLDEN
from gpu_util import DEV
import ensemble_np as enp
from ws_unet_amd import ensemble, ops, spam, srm
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import roc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TILE, KC, MFMA = ops.SUBSPACE_GRAM_TILE, ops.SUBSPACE_GRAM_KC, ops.SUBSPACE_GRAM_MFMA
# (n_rows, d, d_sub, L).  The last one comes from the kernel's constants: one MFMA row block and one column block past a workgroup's
# output tile (and one slot more, so that the last block is ragged too); n_rows is one staging chunk plus a ragged rest.
OWN = (KC + 7, TILE + 2 * MFMA, TILE + MFMA + 1, 2)
SHAPES = [(1, 1, 1, 1), (3, 5, 2, 1), (4, 16, 16, 1), (5, 17, 17, 2), (7, 40, 33, 3), (64, 70, 48, 2), (130, 100, 65, 2), OWN]
REAL_SHAPES = [(7, 40, 33, 3), (130, 100, 65, 2), OWN]


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _case(shape, real=False):
    """zt, idx, weights of one shape: rows of weight 0, one learner (the last) whose weights are all 0, unsorted idx, a repeated index"""
    n_rows, d, d_sub, L = shape
    rng = np.random.default_rng(n_rows * 1000 + d_sub)
    zt = rng.standard_normal((d, n_rows)) if real else rng.integers(-8, 9, (d, n_rows)).astype(np.float64)
    idx = np.stack([rng.permutation(d)[:d_sub] if d_sub <= d else rng.integers(0, d, d_sub) for _ in range(L + 1)]).astype(np.int32)
    if d_sub >= 2:
        idx[:, -1] = idx[:, 0]                                              # a repeated index
        if d_sub >= 3 and (np.diff(idx[0]) > 0).all():
            idx[0, :2] = idx[0, 1::-1]                                      # (a sorted permutation: unsort it)
    weights = rng.integers(0, 6, (L + 1, n_rows)).astype(np.int32)
    if n_rows >= 3:
        weights[:, rng.integers(0, n_rows, max(1, n_rows // 4))] = 0
    weights[-1] = 0
    return zt, idx, weights


def _gram(zt, idx, weights, **kw):
    return ops.subspace_gram(_dev(zt), _dev(idx), _dev(weights), **kw).cpu().numpy()


# ---- K53 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gram_is_exact_on_integer_data(shape):
    """zt in -8..8 and weights in 0..5: every partial sum is an integer far below 2^53, so any summation order gives the same double.  A
    kernel that reads the f64 accumulators with the f32 row map fails here: the data is not symmetric under that permutation."""
    zt, idx, weights = _case(shape)
    got = _gram(zt, idx, weights)
    assert got.dtype == np.float64 and got.shape == (shape[3] + 1, shape[2], shape[2])
    want = enp.gram(zt, idx, weights, np.int64)
    np.testing.assert_array_equal(got, want.astype(np.float64))
    assert not got[-1].any() and (shape[0] < 3 or got[:-1].any())
    if shape[2] >= 3:
        assert (weights[:-1] == 0).any() and (np.diff(idx[0].astype(np.int64)) < 0).any() and idx[0, -1] == idx[0, 0]


WORST = {}


@pytest.mark.parametrize("shape", REAL_SHAPES, ids=str)
def test_gram_on_real_values_stays_within_the_rounding_bound(shape):
    """|G - G_ref| <= (n_rows + 2) 2^-53 sum_i w_i |z_a z_b| per entry, G_ref in longdouble: a sum of n_rows products in any order, one
    rounding more for the weight"""
    zt, idx, weights = _case(shape, real=True)
    got = _gram(zt, idx, weights).astype(np.longdouble)
    ref, mag = enp.gram(zt, idx, weights, np.longdouble), enp.gram_abs(zt, idx, weights)
    bound = (shape[0] + 2) * U * mag
    ratio = float((np.abs(got - ref)[mag > 0] / bound[mag > 0]).max())
    print(f"{shape}: largest |G - G_ref| / bound = {ratio:.4f}")
    assert (np.abs(got - ref) <= bound).all()
    assert not got[-1].any()


def test_gram_is_symmetric_and_independent_of_the_batch_and_the_split():
    zt, idx, weights = _case((130, 100, 65, 4), real=True)
    z, i, w = _dev(zt), _dev(idx), _dev(weights)
    G = ops.subspace_gram(z, i, w)
    assert torch.equal(G, G.transpose(1, 2))                                 # bit for bit: torch.equal compares values, and none is NaN
    assert G.transpose(1, 2).contiguous().cpu().numpy().tobytes() == G.cpu().numpy().tobytes()
    for l in range(len(idx)):
        assert torch.equal(ops.subspace_gram(z, i[l:l + 1], w[l:l + 1])[0], G[l])
    per_learner = 8 * 65 * 65
    assert torch.equal(ops.subspace_gram(z, i, w, max_bytes=per_learner), G)        # one learner per launch
    assert torch.equal(ops.subspace_gram(z, i, w, max_bytes=1), G)                  # below one learner: still one per launch
    assert torch.equal(ops.subspace_gram(z, i, w, max_bytes=2 * per_learner + 5), G)
    out = torch.full((len(idx), 65, 65), np.nan, dtype=torch.float64, device=DEV)
    assert ops.subspace_gram(z, i, w, out=out) is out and torch.equal(out, G)


def test_gram_refuses_bad_arguments_before_launching():
    zt, idx, weights = _case((7, 40, 33, 3))
    z, i, w = _dev(zt), _dev(idx), _dev(weights)
    out = torch.full((4, 33, 33), 7., dtype=torch.float64, device=DEV)
    bad_hi, bad_lo = i.clone(), i.clone()
    bad_hi[2, 5], bad_lo[0, 0] = 40, -1
    cases = {
        "zt float32": (z.float(), i, w), "idx int64": (z, i.long(), w), "weights int64": (z, i, w.long()), "weights float": (z, i, w.double()),
        "zt 1-d": (z[0], i, w), "idx 1-d": (z, i[0], w), "weights of another n_rows": (z, i, w[:, :6].contiguous()),
        "weights of another L": (z, i, w[:2]), "zt on the host": (z.cpu(), i, w), "idx on the host": (z, i.cpu(), w),
        "weights on the host": (z, i, w.cpu()), "zt not contiguous": (_dev(zt.T.copy()).T, i, w), "idx not contiguous": (z, i[:, ::2], w),
        "idx of d": (z, bad_hi, w), "idx of -1": (z, bad_lo, w), "a negative weight": (z, i, w - 1), "no learner": (z, i[:0], w[:0]),
    }
    for what, args in cases.items():
        with pytest.raises(ValueError, match="subspace_gram"):
            ops.subspace_gram(*args, out=out)
        assert bool((out == 7.).all()), f"{what}: something was launched"
    for kw in (dict(out=out[:3]), dict(out=out.float()), dict(out=out.cpu()), dict(out=out.transpose(1, 2)), dict(max_bytes=0)):
        with pytest.raises(ValueError, match="subspace_gram"):
            ops.subspace_gram(z, i, w, **kw)
    lib = ops._lib.load()
    assert lib.wsu_subspace_gram_f64(z.data_ptr(), None, w.data_ptr(), out.data_ptr(), 7, 40, 33, 4, None) == -1 and b"null" in lib.wsu_last_error()


# ---- base learners --------------------------------------------------------------------------------------------------------------------

def _two_classes(n0, n1, d, shift, seed):
    rng = np.random.default_rng(seed)
    mix = np.eye(d) + 0.3 * rng.standard_normal((d, d)) / np.sqrt(d)         # correlated features of unequal scale
    X0 = rng.standard_normal((n0, d)) @ mix
    X1 = rng.standard_normal((n1, d)) @ mix + shift
    return X0, X1


def test_base_learners_and_projections_against_the_restatement():
    """Given the restatement's draws, w_l against numpy's float64 solve of the restated system, relative in the 2-norm, within
    c d_sub kappa 2^-53 with kappa <= 1 + d_sub / ridge (lambda = ridge trace / d_sub >= ridge ||S|| / d_sub) and
        c = 2 (3 d_sub + 1)  +  2 (n_rows + 8) g.
    First term: the textbook bound of a Cholesky solve (Higham, Accuracy and Stability, Thm 10.4 with ||  |R^T||R|  || <= d_sub ||A||):
    backward error d_sub gamma_(3 d_sub + 1) ||A||, hence forward error d_sub (3 d_sub + 1) kappa u; twice, since the restatement's LU
    solve is granted the same.  Second term: the matrix itself is formed with rounding on both sides, entry by entry a sum of n_rows
    products (K53's bound) less two outer products (8 more roundings granted): ||dM||_F <= (n_rows + 8) u trace(G) / (N - 2)
    <= (n_rows + 8) u d_sub g ||M||, where g = ||G|| / ((N - 2) ||M||) is how much larger than the regularised scatter the uncentred
    Gram is -- a property of the inputs, computed here from the restatement in longdouble.  Projections: |p - p_ref| <=
    ||z|| ||w_ref|| (that tolerance + (d_sub + 2) u)."""
    n0, n1, d, L, ds, ridge = 30, 60, 50, 6, 21, 0.1
    shift = np.zeros(d)
    shift[:8] = 0.5
    X0, X1 = _two_classes(n0, n1, d, shift, 3)
    X = np.concatenate([X0, X1])
    Z = X - X.mean(axis=0)
    y = np.concatenate([np.zeros(n0, dtype=int), np.ones(n1, dtype=int)])
    group, n_groups = enp.groups(n0, n1)
    (idx, c), = enp.draws(5, d, [ds], L, group, n_groups, n0)
    wt = c[:, group]
    m = ensemble.Ensemble(L, ds, ridge, 5)
    Zd = _dev(Z)
    got = m._solve(Zd, Zd.T.contiguous(), idx, wt, n0)
    kappa_bound = 1 + ds / ridge
    worst_w = worst_p = 0.
    for l in range(L):
        want, M = enp.base_learner(Z, y, idx[l], wt[l], ridge)
        _, M_ld = enp.base_learner(Z, y, idx[l], wt[l], ridge, np.longdouble)
        G = enp.gram(Z.T, idx[l:l + 1], wt[l:l + 1], np.longdouble)[0].astype(np.float64)
        g = np.linalg.norm(G, 2) / ((wt[l].sum() - 2) * np.linalg.norm(M_ld.astype(np.float64), 2))
        tol = (2 * (3 * ds + 1) + 2 * (len(Z) + 8) * g) * ds * kappa_bound * U
        err = np.linalg.norm(got[l] - want) / np.linalg.norm(want)
        assert np.linalg.cond(M) <= kappa_bound * (1 + 1e-9)
        p_got, p_want = Z[:, idx[l]] @ got[l], Z[:, idx[l]] @ want
        p_tol = np.linalg.norm(Z[:, idx[l]], axis=1) * np.linalg.norm(want) * (tol + (ds + 2) * U)
        print(f"learner {l}: |w - w_ref| / |w_ref| = {err:.3e} (tolerance {tol:.3e}, g = {g:.2f}); "
              f"largest projection error / its tolerance = {(np.abs(p_got - p_want) / p_tol).max():.3e}")
        worst_w, worst_p = max(worst_w, err / tol), max(worst_p, float((np.abs(p_got - p_want) / p_tol).max()))
        assert err <= tol
        assert (np.abs(p_got - p_want) <= p_tol).all()
    # the projection the fit makes on the device: the dense (d, L) matrix in one matmul
    P = (Zd @ _dev(ensemble.dense(idx, got, d))).cpu().numpy()
    for l in range(L):
        p_want = Z[:, idx[l]] @ got[l]
        assert (np.abs(P[:, l] - p_want) <= np.linalg.norm(Z[:, idx[l]], axis=1) * np.linalg.norm(got[l]) * (2 * ds + 4) * U).all()
    print(f"worst ratios to the tolerances: w {worst_w:.3e}, projections {worst_p:.3e}")


def test_a_failed_factorisation_names_the_learner():
    """every row of a class the same, the classes 1 apart: the centred rows are -1/2 and +1/2 everywhere, every product and sum is exact,
    the within-class scatter is exactly 0 and so is its ridge: nothing to factorise"""
    X0 = np.tile(np.arange(30, dtype=np.float64), (4, 1))
    with pytest.raises(ValueError, match=r"learner 0 .*ridge above 0"):
        ensemble.Ensemble(3, 20, 0., 0).fit(X0, X0 + 1.)
    with pytest.raises(ValueError, match="non-finite"):
        ensemble.Ensemble(3, 5, 0.1, 0).fit(np.full((3, 8), np.inf), np.zeros((3, 8)))
    with pytest.raises(ValueError, match="d_sub 9 above the 8"):
        ensemble.Ensemble(3, 9, 0.1, 0).fit(np.zeros((3, 8)), np.ones((3, 8)))


# ---- fit ------------------------------------------------------------------------------------------------------------------------------

def _fit_data(seed, rest=3.):
    """two Gaussian classes in 40 dimensions, unit variance, 60 groups of one cover and one stego row; the means differ by 8 standard
    deviations in five of the dimensions and by `rest` in the 35 others.

    Why the others differ at all: a base learner whose features all have equal class means sees the same distribution in both classes
    and votes by chance on the rows outside its bag.  With 5 of 40 features per learner that is C(35,5) / C(40,5) = 0.49 of the
    learners, and an out-of-bag error of 0 cannot be asked of such data (rest=0 below: 0.161).  So every dimension carries some signal.
    How much, fixed before the first run: the weakest learner (five features of shift `rest`) errs with probability Phi(-rest sqrt(5) / 2);
    a row is misjudged or tied only if at least half of its out-of-bag judges err, at most about twice that; over the 120 training
    rows the expected number of such rows is to stay below 0.1: 240 Phi(-rest sqrt(5) / 2) < 0.1 gives rest = 3 (Phi(-3.35) = 4e-4)."""
    rng = np.random.default_rng(seed)
    shift = np.full(40, float(rest))
    shift[[3, 11, 19, 27, 35]] = 8.
    return rng.standard_normal((60, 40)), rng.standard_normal((60, 40)) + shift


@pytest.fixture(scope="module")
def fitted():
    X0, X1 = _fit_data(0)
    return X0, X1, ensemble.Ensemble(11, [5, 12], 0.1, 0).fit(X0, X1), enp.fit(X0, X1, 11, [5, 12], 0.1, 0)


def test_fit_oob_error_is_zero_and_the_first_d_sub_is_chosen(fitted):
    """L = 11, d_sub = [5, 12], 60 groups: oob_error is 0 for both candidates and the tie goes to the first listed"""
    _, _, m, ref = fitted
    print(f"oob_errors {m.oob_errors} (restatement {ref['oob_errors']}), chosen d_sub {m.d_sub_chosen}")
    assert m.oob_error == 0.
    assert m.oob_errors == [0., 0.]
    assert m.d_sub_chosen == 5


def test_fit_with_uninformative_features_agrees_with_the_restatement():
    """the same classes with equal means in the 35 other dimensions: learners without an informative feature judge by chance, the
    out-of-bag error of d_sub = 5 is far from 0 and the SECOND candidate is chosen; product and restatement agree on all of it"""
    X0, X1 = _fit_data(0, rest=0.)
    m, ref = ensemble.Ensemble(11, [5, 12], 0.1, 0).fit(X0, X1), enp.fit(X0, X1, 11, [5, 12], 0.1, 0)
    print(f"oob_errors {m.oob_errors} (restatement {ref['oob_errors']}), chosen d_sub {m.d_sub_chosen}")
    assert m.oob_errors == ref["oob_errors"] and m.d_sub_chosen == ref["d_sub"] == 12
    assert m.oob_errors[0] > 0.05 and m.oob_error == m.oob_errors[1] == min(m.oob_errors)
    np.testing.assert_array_equal(m.idx, ref["idx"])
    H = np.concatenate(_fit_data(1, rest=0.))
    np.testing.assert_array_equal(m.votes(H), enp.votes(H, ref["mean"], ref["idx"], ref["w"], ref["b"]))


def test_fit_separates_two_gaussian_classes(fitted, tmp_path):
    """every held-out row is classified right; the model equals the restatement's in its draws, OOB errors, choice and votes; one seed
    gives byte-equal files, another seed other idx"""
    X0, X1, m, ref = fitted
    H0, H1 = _fit_data(1)
    print(f"oob_errors {m.oob_errors} (restatement {ref['oob_errors']}), chosen d_sub {m.d_sub_chosen}; held-out outputs: covers max "
          f"{m.output(H0).max():.3f}, stegos min {m.output(H1).min():.3f}")
    assert m.oob_errors == ref["oob_errors"] and m.d_sub_chosen == ref["d_sub"] and m.oob_error == min(m.oob_errors)
    np.testing.assert_array_equal(m.idx, ref["idx"])
    np.testing.assert_array_equal(m.votes(np.concatenate([H0, H1])), enp.votes(np.concatenate([H0, H1]), ref["mean"], ref["idx"], ref["w"], ref["b"]))
    assert (m.output(H0) < 0.5).all() and (m.output(H1) > 0.5).all()
    assert m.idx.shape == (11, m.d_sub_chosen) and m.idx.dtype == np.int32
    m.save(tmp_path / "a.npz")
    ensemble.Ensemble(11, [5, 12], 0.1, 0).fit(X0, X1).save(tmp_path / "b.npz")
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
    other = ensemble.Ensemble(11, [5, 12], 0.1, 1).fit(X0, X1)
    assert not np.array_equal(other.idx, m.idx)
    r = ensemble.Ensemble.load(tmp_path / "a.npz")
    np.testing.assert_array_equal(r.votes(H1), m.votes(H1))


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------

COVERS = (6, 7, 8, 9, 10)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """64 x 64 crops of the five golden covers (test_gpu_srm_weighted's crops, every eighth one: 8 per cover, 40 files) as a data set"""
    root = tmp_path_factory.mktemp("ensemble_data")
    (root / "images").mkdir()
    names = []
    for k in COVERS:
        p = np.ascontiguousarray(imread4_u8(GOLDEN / f"cover_{k}.png")[..., 3])
        crops = [p[r:r + 64, c:c + 64] for r in range(0, 512, 64) for c in range(0, 512, 64)]
        for j, crop in enumerate(crops[::8]):
            names.append(f"images/{k}_{j}.png")
            Image.fromarray(crop).save(root / names[-1])
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"{n},64,64\n" for n in names))
    return root


def _check_scores(csv, learners, n):
    df = pd.read_csv(csv, float_precision="round_trip")
    assert list(df.columns) == ["name", "height", "width", "output", "prediction", "stego_method", "alpha"] == list(pd.read_csv(GOLDEN / "b0.csv").columns)
    assert len(df) == 2 * n and df["stego_method"][:n].isna().all() and (df["stego_method"][n:] == "LSBM").all()
    steps = df["output"].to_numpy() * learners
    assert (steps == np.round(steps)).all() and df["output"].between(0., 1.).all() and (df["prediction"] == (df["output"] > 0.5)).all()
    return df


def test_srm_fit_score_and_the_roc_row(dataset, tmp_path):
    model_path, csv = tmp_path / "srm_ens.npz", tmp_path / "ens.csv"
    common = ["--data", str(dataset), "--stego-methods", "LSBM", "--alphas", "1.0", "--simulate"]
    srm.main(["fit", *common, "--classifier", "ensemble", "--learners", "7", "--d-sub", "40", "90", "--seed", "2", "--out", str(model_path)])
    model = srm.load_model(model_path, "linear")
    assert type(model) is srm.Ensemble and model.idx.shape == (7, model.d_sub_chosen) and model.d_sub == [40, 90] and len(model.oob_errors) == 2
    assert model.mean.shape == (3718,) and (model.stego_methods, model.alphas, model.seed) == (["LSBM"], [1.0], 2)
    # the groups came from the file stems: the same fit through the classes, given them, is the same file
    rows0, F0 = srm.extract(dataset)
    rows1, F1 = srm.extract(dataset, "LSBM", 1.0, simulate=True)
    assert rows1["name"].str.startswith("stego").all()
    direct = srm.Ensemble(7, [40, 90], 0.1, 2).fit(F0, F1, *ensemble.stem_groups(rows0["name"], rows1["name"]))
    direct.stego_methods, direct.alphas = ["LSBM"], [1.0]
    direct.save(tmp_path / "direct.npz")
    assert model_path.read_bytes() == (tmp_path / "direct.npz").read_bytes()
    srm.main(["score", *common, "--model", str(model_path), "--out", str(csv)])
    df = _check_scores(csv, 7, 40)
    np.testing.assert_array_equal(df["output"].to_numpy(), model.output(np.concatenate([F0, F1])))
    scores = roc.load_scores(csv, "B0_SRM_ENS", ["LSBM"], [1.0])
    assert len(scores) == 80
    scores["stego_method"] = scores["stego_method"].fillna("Cover")
    frame = roc.produce_roc(scores)                                         # what ws.roc's main makes of a --scores file
    auc = roc.auc_table(frame)
    # (the reference's rates are 0 / 0 = NaN where no score exceeds a threshold, as for the covers of a training set told apart completely)
    assert len(frame) == len(roc.TAUS) and auc["model_name"].tolist() == ["B0_SRM_ENS"] and auc["stego_method"].tolist() == ["LSBM"]
    assert (auc["auc"].isna() | auc["auc"].between(0., 1.)).all() and (auc["p_e"].isna() | auc["p_e"].between(0., 0.5)).all()
    print(f"B0_SRM_ENS on its own 40 training pairs: auc {float(auc['auc'].iloc[0])}, p_e {float(auc['p_e'].iloc[0])}; oob_errors {model.oob_errors}")
    with pytest.raises(ValueError, match="'srm-linear' features, asked for 'srm-minmax'"):        # load_model, before anything is read
        srm.main(["score", *common, "--model", str(model_path), "--submodels", "minmax", "--out", str(tmp_path / "no.csv")])
    with pytest.raises(ValueError, match="'srm-linear' features, not on 'srm-minmax'"):           # score's own check, as for an FLD
        srm.score(dataset, model, ["LSBM"], [1.0], simulate=True, submodels="minmax")
    with pytest.raises(ValueError, match="ensemble.*load_model"):
        srm.FLD.load(model_path)


def test_srm_fit_without_a_classifier_is_the_fld_file(dataset, tmp_path):
    common = ["--data", str(dataset), "--stego-methods", "LSBM", "--alphas", "1.0", "--simulate"]
    srm.main(["fit", *common, "--out", str(tmp_path / "cli.npz")])
    _, F0 = srm.extract(dataset)
    _, F1 = srm.extract(dataset, "LSBM", 1.0, simulate=True)
    model = srm.FLD(0.1, "linear").fit(F0, F1)
    model.stego_methods, model.alphas = ["LSBM"], [1.0]
    model.save(tmp_path / "direct.npz")
    assert (tmp_path / "cli.npz").read_bytes() == (tmp_path / "direct.npz").read_bytes()
    assert type(srm.load_model(tmp_path / "cli.npz")) is srm.FLD


def test_spam_fit_and_score(dataset, tmp_path):
    model_path, csv = tmp_path / "spam_ens.npz", tmp_path / "spam_ens.csv"
    common = ["--data", str(dataset), "--stego-methods", "LSBM", "--alphas", "1.0", "--simulate"]
    spam.main(["fit", *common, "--classifier", "ensemble", "--learners", "5", "--d-sub", "30", "--out", str(model_path)])
    model = spam.load_model(model_path)
    assert type(model) is spam.Ensemble and model.idx.shape == (5, 30) and (model.order, model.T, model.normalise) == (2, 3, "joint")
    spam.main(["score", *common, "--model", str(model_path), "--out", str(csv)])
    df = _check_scores(csv, 5, 40)
    assert len(roc.load_scores(csv, "B0_SPAM_ENS", ["LSBM"], [1.0])) == 80
    _, F0 = spam.extract(dataset)
    np.testing.assert_array_equal(df["output"].to_numpy()[:40], model.output(F0))
    with pytest.raises(ValueError, match="ensemble.*load_model"):
        spam.FLD.load(model_path)
