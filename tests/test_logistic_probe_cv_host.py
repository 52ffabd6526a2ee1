"""CPU: ``lla_softmax_grid_pass`` is declared, bound and refuses bad arguments before any device call; ``LogisticProbeCV`` on
the CPU (the float64 twin that the GPU tests use as their oracle) solves scikit-learn's LogisticRegression objective on
every fold's training rows, scores what it returns, and does not depend on how the classifiers or the rows are batched."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
from latents_util import write_dataset
from logistic_cv_util import unbalanced, within_strong_convexity
from lossyless_amd import _lib
from probe_cv_util import check_cv_scores, stratified_folds
from probe_util import make_data

TOL = 1e-4


def test_symbols_are_declared_bound_and_exported():
    import lossyless_amd
    with open(os.path.join(ROOT, "include", "lossyless_amd.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lla_softmax_grid_pass", "lla_softmax_grid_pass_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} not declared"
        assert name in _lib.EXPORTS and hasattr(raw, name), f"{name} not bound / exported"
    assert _lib.lib().lla_abi_version() == _lib.ABI_VERSION == 4          # additive: the ABI version stays
    assert "LogisticProbeCV" in lossyless_amd.__all__ and lossyless_amd.LogisticProbeCV is not None


def _call(C=40, K=3, G=4, B=16, ld_z=None, ld_w=None, null=(), z_dtype=None, V=False, shift=None):
    """lla_softmax_grid_pass on host buffers it must never read: every call here is refused by the argument checks."""
    L = _lib.lib()
    buf = np.zeros(1 << 16, dtype=np.float64)          # 16-byte aligned stand-in for every pointer
    p = ctypes.c_void_p(buf.ctypes.data + (-buf.ctypes.data) % 16)
    a = dict(z=p, y=p, fold=p, W=p, b=p, V=p if V else None, vb=p if V else None, held=p, cw=p, out_W=p, out_b=p, out_loss=p,
             ws=p)
    for k in null:
        a[k] = None
    if shift is not None:                              # a pointer off its alignment
        a[shift[0]] = ctypes.c_void_p(p.value + shift[1])
    return L.lla_softmax_grid_pass(a["z"], _lib.LLA_Z_F32 if z_dtype is None else z_dtype, C if ld_z is None else ld_z, a["y"],
                                   a["fold"], B, C, a["W"], a["b"], a["V"], a["vb"], K, G, C if ld_w is None else ld_w,
                                   a["held"], a["cw"], a["out_W"], a["out_b"], a["out_loss"], 0, a["ws"], None)


def test_bad_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    assert _call(C=12) == _lib.LLA_EINVAL                  # not a multiple of 8
    assert _call(C=1032) == _lib.LLA_EINVAL                # wider than 1024
    assert _call(C=0) == _lib.LLA_EINVAL
    assert _call(K=0) == _lib.LLA_EINVAL
    assert _call(K=33) == _lib.LLA_EINVAL                  # a group must fit one tile
    assert _call(K=33, G=1) == _lib.LLA_EINVAL
    assert _call(G=0) == _lib.LLA_EINVAL
    assert _call(G=-1) == _lib.LLA_EINVAL
    assert _call(K=1, G=65535 * 32 + 1) == _lib.LLA_EINVAL  # more tiles than a grid has
    assert _call(ld_z=32) == _lib.LLA_EINVAL               # ld_z < C
    assert _call(ld_z=42) == _lib.LLA_EINVAL               # pitch not a multiple of 4
    assert _call(ld_w=32) == _lib.LLA_EINVAL
    assert _call(ld_w=42) == _lib.LLA_EINVAL
    assert _call(B=-1) == _lib.LLA_EINVAL
    assert _call(z_dtype=7) == _lib.LLA_EINVAL
    for name in ("z", "y", "W", "b", "out_W", "out_b", "out_loss", "ws"):   # (out_loss: gradient mode needs it)
        assert _call(null=(name,)) == _lib.LLA_EINVAL, name
    assert _call(null=("held",)) == _lib.LLA_EINVAL        # folds, and nobody says which one a group holds out
    assert _call(V=True, null=("vb",)) == _lib.LLA_EINVAL
    assert _call(shift=("z", 8)) == _lib.LLA_EINVAL        # fp32 rows want 16 bytes
    assert _call(shift=("z", 4), z_dtype=_lib.LLA_Z_F16) == _lib.LLA_EINVAL
    assert _call(shift=("W", 8)) == _lib.LLA_EINVAL
    assert _call(V=True, shift=("V", 8)) == _lib.LLA_EINVAL
    assert _call(shift=("ws", 2)) == _lib.LLA_EINVAL
    for C, K, G in ((12, 3, 4), (1032, 3, 4), (40, 0, 4), (40, 33, 4), (40, 3, 0)):
        assert L.lla_softmax_grid_pass_workspace_bytes(C, K, G) == 0
    # ceil(G / (32 / K)) tiles of 32 slots, each with the walkers lla_svm_pass gives that many class tiles
    assert L.lla_softmax_grid_pass_workspace_bytes(512, 10, 3) == L.lla_svm_pass_workspace_bytes(512, 32)
    assert L.lla_softmax_grid_pass_workspace_bytes(512, 10, 40) == L.lla_svm_pass_workspace_bytes(512, 14 * 32)
    assert L.lla_softmax_grid_pass_workspace_bytes(512, 17, 3) == L.lla_svm_pass_workspace_bytes(512, 3 * 32)
    assert L.lla_softmax_grid_pass_workspace_bytes(512, 32, 2) == L.lla_svm_pass_workspace_bytes(512, 64)


def _sklearn_fit(lm, X, labels, Cw, class_weight):
    X1 = torch.cat([X.double(), torch.ones(X.shape[0], 1, dtype=torch.float64)], 1).numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = lm.LogisticRegression(C=Cw, fit_intercept=False, tol=1e-12, max_iter=20000,
                                    class_weight=class_weight).fit(X1, labels.numpy())
    return clf, X1


@pytest.mark.parametrize("class_weight", [None, "balanced", "dict"])
@pytest.mark.parametrize("N,C,K,cv", [(600, 40, 3, 3), (300, 40, 33, 2)])
def test_every_fold_against_scikit_learn(N, C, K, cv, class_weight):
    """(300, 40, 33): more classes than a tile of the device pass holds -- the twin has one route for every K."""
    lm = pytest.importorskip("sklearn.linear_model")
    from lossyless_amd import LogisticProbeCV
    X, y = unbalanced(N, C, K)
    labels = 2 * y + 1                                     # (labels are not class indexes)
    if class_weight == "dict":
        class_weight = {1: 2.5, 5: 0.3}                    # labels left out weigh 1
    candidates = [(1.0, class_weight), (0.05, class_weight)]
    search = LogisticProbeCV(candidates, cv=cv, tol=TOL).fit(X, labels)
    fold = stratified_folds(labels, cv)
    assert tuple(search.fold_coef_.shape) == (2, cv, K, C) and tuple(search.fold_intercept_.shape) == (2, cv, K)
    assert search.fold_coef_.dtype == torch.float32 and bool(search.converged_.all()) and search.folds_ == list(range(cv))
    assert tuple(search.converged_.shape) == (2, cv + 1)
    for c, (Cw, cw) in enumerate(candidates):
        for f in range(cv):
            train = fold != f
            clf, X1 = _sklearn_fit(lm, X[train], labels[train], Cw, cw)
            assert np.array_equal(search.classes_, clf.classes_)
            Wsk, bsk = torch.from_numpy(clf.coef_[:, :C]), torch.from_numpy(clf.coef_[:, C])
            within_strong_convexity(search.fold_coef_[c, f], search.fold_intercept_[c, f], Wsk, bsk, X[train], labels[train],
                                    search.classes_, Cw, cw, f"K {K} {cw} candidate {c} fold {f}")
            S = X[train].double() @ search.fold_coef_[c, f].double().T + search.fold_intercept_[c, f].double()
            assert np.array_equal(search.classes_[S.argmax(1).numpy()], clf.predict(X1))


@pytest.mark.parametrize("class_weight", [None, "balanced"])
def test_two_classes_are_the_binomial_problem(class_weight):
    lm = pytest.importorskip("sklearn.linear_model")
    from lossyless_amd import LogisticProbeCV
    N, C = 400, 40
    X, y = unbalanced(N, C, 2)
    labels = 2 * y + 1
    candidates = [(1.0, class_weight), (0.05, class_weight)]
    search = LogisticProbeCV(candidates, cv=3, tol=TOL).fit(X, labels)
    fold = stratified_folds(labels, 3)
    assert tuple(search.fold_coef_.shape) == (2, 3, 1, C) and tuple(search.fold_intercept_.shape) == (2, 3, 1)
    for c, (Cw, cw) in enumerate(candidates):
        for f in range(3):
            train = fold != f
            clf, X1 = _sklearn_fit(lm, X[train], labels[train], Cw, cw)
            wsk, bsk = torch.from_numpy(clf.coef_[:1, :C]), torch.from_numpy(clf.coef_[:1, C])
            within_strong_convexity(search.fold_coef_[c, f], search.fold_intercept_[c, f], wsk, bsk, X[train], labels[train],
                                    search.classes_, Cw, cw, f"two classes {cw} candidate {c} fold {f}")
            s = X[train].double() @ search.fold_coef_[c, f, 0].double() + float(search.fold_intercept_[c, f, 0])
            assert np.array_equal(search.classes_[(s > 0).long().numpy()], clf.predict(X1))
    assert check_cv_scores(search, X, labels, fold, cap=0.0) == 0.0
    best = search.best_estimator_
    assert tuple(best.coef_.shape) == (1, C) and tuple(best.predict_proba(X).shape) == (N, 2)


CANDIDATES = [(0.01, None), (1.0, "balanced"), (0.2, {1: 2.5, 5: 0.3}), (1.0, "balanced")]


@pytest.fixture(scope="module")
def searched():
    from lossyless_amd import LogisticProbeCV
    X, y = unbalanced(600, 40, 3)
    labels = 2 * y + 1
    return X, labels, LogisticProbeCV(CANDIDATES, cv=3, tol=TOL).fit(X, labels)


def test_scores_ranking_and_best_estimator(searched):
    from lossyless_amd import LogisticProbe
    X, labels, search = searched
    fold = stratified_folds(labels, 3)
    # cv_scores_ is the float64 accuracy of the returned coefficients on the held-out rows: no row is left out here
    assert check_cv_scores(search, X, labels, fold, cap=0.0) == 0.0
    assert tuple(search.cv_scores_.shape) == (4, 3) and search.cv_scores_.dtype == torch.float64
    assert torch.equal(search.mean_scores_, search.cv_scores_.mean(1))
    means = search.mean_scores_.numpy()
    assert search.best_index_ == int(np.argmax(means))     # numpy's argmax is the first maximum
    assert means[1] == means[3] and search.best_index_ != 3          # candidates 1 and 3 are the same: the first one ranks first
    Cw, cw = CANDIDATES[search.best_index_]
    assert search.best_params_ == dict(C=Cw, class_weight=cw)
    best = search.best_estimator_
    assert isinstance(best, LogisticProbe) and best.C == Cw and best.class_weight == cw and best.converged_
    alone = LogisticProbe(C=Cw, tol=TOL, class_weight=cw).fit(X, labels)
    within_strong_convexity(best.coef_, best.intercept_, alone.coef_, alone.intercept_, X, labels, search.classes_, Cw, cw,
                            "best_estimator_ against a standalone fit")
    assert torch.equal(best.predict(X), alone.predict(X))
    proba = best.predict_proba(X)
    assert tuple(proba.shape) == (600, 3) and float((proba.sum(1) - 1).abs().max()) < 1e-12
    assert search.n_passes_ > 0 and np.array_equal(search.classes_, np.array([1, 3, 5]))
    from lossyless_amd import LogisticProbeCV
    none = LogisticProbeCV(CANDIDATES[:2], cv=3, tol=TOL, refit=False).fit(X, labels)
    assert none.best_estimator_ is None and tuple(none.converged_.shape) == (2, 3)
    assert torch.equal(none.fold_coef_, search.fold_coef_[:2])


def test_fold_arrays_and_missing_classes(monkeypatch):
    from lossyless_amd import LogisticProbeCV
    X, y = unbalanced(600, 40, 3)
    g = torch.Generator().manual_seed(5)
    fold = torch.randint(-1, 2, (600,), generator=g)       # -1: always trains, never validates
    search = LogisticProbeCV(CANDIDATES[:2], cv=fold.numpy(), tol=TOL).fit(X, y)
    assert search.folds_ == [0, 1] and tuple(search.cv_scores_.shape) == (2, 2)
    assert check_cv_scores(search, X, y, fold, cap=0.0) == 0.0
    for f in (0, 1):                                       # the rows of fold -1 are in every training part
        train = fold != f
        Cw, cw = CANDIDATES[1]
        from lossyless_amd import LogisticProbe
        alone = LogisticProbe(C=Cw, tol=TOL, class_weight=cw).fit(X[train], y[train])
        within_strong_convexity(search.fold_coef_[1, f], search.fold_intercept_[1, f], alone.coef_, alone.intercept_, X[train],
                                y[train], search.classes_, Cw, cw, f"fold array, fold {f}")
    lacking = torch.where(y == 2, 0, 1)                    # fold 0 holds every row of class 2: its training part has none
    import lossyless_amd.probe as probe_module

    def no_walk(self):
        raise AssertionError("the rows were walked before the folds were checked")
    monkeypatch.setattr(probe_module._Rows, "groups", no_walk)
    probe = LogisticProbeCV(CANDIDATES[:1], cv=lacking.numpy())
    with pytest.raises(ValueError, match="lacks a class"):
        probe.fit(X, y)
    assert probe.cv_scores_ is None
    with pytest.raises(ValueError, match="no candidates"):
        LogisticProbeCV([])
    with pytest.raises(ValueError, match="class_weight"):
        LogisticProbeCV([(1.0, "heavy")])
    with pytest.raises(ValueError, match="at least 2"):
        LogisticProbeCV(CANDIDATES[:1], cv=1).fit(X, y)


def test_batches_and_groups_of_rows_give_the_same_bits(searched):
    from lossyless_amd import LogisticProbeCV
    X, labels, one = searched
    for kw, fit_kw in ((dict(max_problems=9), {}), (dict(max_problems=1), {}), ({}, dict(rows_per_pass=128)),
                       (dict(max_problems=12), dict(rows_per_pass=250))):
        again = LogisticProbeCV(CANDIDATES, cv=3, tol=TOL, **kw).fit(X, labels, **fit_kw)
        assert torch.equal(again.fold_coef_, one.fold_coef_) and torch.equal(again.fold_intercept_, one.fold_intercept_), kw
        assert torch.equal(again.cv_scores_, one.cv_scores_) and again.best_index_ == one.best_index_
        assert torch.equal(again.best_estimator_.coef_, one.best_estimator_.coef_)
        assert again.best_estimator_.objective_ == one.best_estimator_.objective_


def test_rows_beyond_one_block_of_the_twin():
    from lossyless_amd import LogisticProbeCV
    from lossyless_amd.probe import _HOST_BLOCK
    X, y = unbalanced(_HOST_BLOCK + 700, 24, 5)
    one = LogisticProbeCV([(0.1, "balanced")], cv=2, tol=TOL).fit(X, y)
    for rows_per_pass in (128, 1000):
        again = LogisticProbeCV([(0.1, "balanced")], cv=2, tol=TOL).fit(X, y, rows_per_pass=rows_per_pass)
        assert torch.equal(again.fold_coef_, one.fold_coef_) and torch.equal(again.cv_scores_, one.cv_scores_)


def test_compressed_latents_on_the_cpu(tmp_path):
    import hubconf
    from lossyless_amd import LogisticProbeCV
    comp, _ = hubconf.clip_compressor_b005(device="cpu", clip_weights="synthetic")
    N = 300
    file, _, _ = write_dataset(tmp_path, "5e-02", N, seed=17)
    ds = comp.open_dataset(file, device="cpu")
    labels = torch.arange(N) % 3
    rows = ds.all()

    # (sampled records carry escapes: rows of norm 1e5 on which two Newton steps are far from done -- what is under test
    # is that the streamed path and the array path are the same sums)
    def fit(data, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return LogisticProbeCV([(1e-6, None), (1e-7, "balanced")], cv=3, max_iter=2).fit(data, labels, **kw)
    a, b = fit(ds, rows_per_pass=128), fit(rows)
    assert torch.equal(a.fold_coef_, b.fold_coef_) and torch.equal(a.cv_scores_, b.cv_scores_) and a.n_passes_ == b.n_passes_
    assert bool(a.fold_coef_.abs().max() > 0) and bool(torch.isfinite(a.fold_coef_).all())
    assert torch.equal(fit(ds, rows_per_pass=128, keep_rows=True).fold_coef_, a.fold_coef_)
    assert torch.equal(a.best_estimator_.decision_function(ds), a.best_estimator_.decision_function(rows))


def test_logspace_and_sampled_candidates():
    from lossyless_amd import LinearProbeCV, LogisticProbeCV
    grid = LogisticProbeCV.logspace(5, 1e-3, 10.0)
    assert [cw for _, cw in grid] == [None] * 5 and grid[0][0] == 1e-3 and grid[-1][0] == 10.0
    ratios = [grid[i + 1][0] / grid[i][0] for i in range(4)]
    assert max(ratios) - min(ratios) < 1e-9 and abs(ratios[0] - 10.0) < 1e-9
    assert LogisticProbeCV.logspace(1, 0.5, 0.5, "balanced") == [(0.5, "balanced")]
    with pytest.raises(ValueError):
        LogisticProbeCV.logspace(3, 0.0, 1.0)
    with pytest.raises(ValueError):
        LogisticProbeCV.logspace(0, 1e-3, 1.0)
    X, y = make_data(200, 16, 3)
    search = LogisticProbeCV(LinearProbeCV.sample(3, seed=1), cv=2, tol=TOL).fit(X, y)
    assert tuple(search.cv_scores_.shape) == (3, 2) and search.best_params_["C"] == search.candidates[search.best_index_][0]


def test_max_iter_warns():
    from lossyless_amd import LogisticProbeCV
    X, y = make_data(200, 16, 3)
    with pytest.warns(RuntimeWarning, match="stopped short"):
        search = LogisticProbeCV([(1.0, None)], cv=2, tol=1e-12, max_iter=1).fit(X, y)
    assert not bool(search.converged_.all())
