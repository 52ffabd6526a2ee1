"""CPU: ``lla_svm_grid_pass`` is declared, bound and refuses bad arguments before any device call; ``class_weight`` of
``LinearProbe`` solves scikit-learn's class-weighted LinearSVC objective; ``LinearProbeCV`` on the CPU (the float64 twin,
the oracle of the GPU tests) returns, for every (candidate, fold), what a standalone fit on that fold's training rows
returns, and scores it as a float64 evaluation of the returned coefficients does."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
from latents_util import write_dataset
from lossyless_amd import _lib
from probe_cv_util import (accuracy64, check_cv_scores, ovr_weights, stratified_folds, weighted_grad_norms,
                           within_strong_convexity)
from probe_util import make_data

TOL = 1e-4
CANDIDATES = [(7e-3, None), (0.05, "balanced"), (0.3, None)]


def unbalanced(N, C, K, seed=1):
    """make_data with class k thinned to a share that falls with k: every class present, none as large as another."""
    X, y = make_data(2 * N, C, K, seed)
    g = torch.Generator().manual_seed(seed + 100)
    keep = torch.rand(2 * N, generator=g) < (1.0 / (1.0 + y.double()))
    at = torch.nonzero(keep)[:N, 0]
    return X[at], y[at]


def test_symbols_are_declared_bound_and_exported():
    import lossyless_amd
    with open(os.path.join(ROOT, "include", "lossyless_amd.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lla_svm_grid_pass", "lla_svm_grid_pass_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} not declared"
        assert name in _lib.EXPORTS and hasattr(raw, name), f"{name} not bound / exported"
    assert _lib.lib().lla_abi_version() == _lib.ABI_VERSION == 4          # additive: the ABI version stays
    assert "LinearProbeCV" in lossyless_amd.__all__ and lossyless_amd.LinearProbeCV is not None


def _call(C=40, J=3, B=16, ld_z=None, ld_w=None, null=(), z_dtype=None, V=False):
    """lla_svm_grid_pass on host buffers it must never read: every call here is refused by the argument checks."""
    L = _lib.lib()
    buf = np.zeros(1 << 16, dtype=np.float64)          # 16-byte aligned stand-in for every pointer
    p = ctypes.c_void_p(buf.ctypes.data + (-buf.ctypes.data) % 16)
    a = dict(z=p, y=p, fold=p, W=p, b=p, V=p if V else None, vb=p if V else None, col_class=p, col_held=p, col_cpos=p,
             col_cneg=p, out_W=p, out_b=p, out_loss=p, ws=p)
    for k in null:
        a[k] = None
    return L.lla_svm_grid_pass(a["z"], _lib.LLA_Z_F32 if z_dtype is None else z_dtype, C if ld_z is None else ld_z, a["y"],
                               a["fold"], B, C, a["W"], a["b"], a["V"], a["vb"], J, C if ld_w is None else ld_w,
                               a["col_class"], a["col_held"], a["col_cpos"], a["col_cneg"], a["out_W"], a["out_b"],
                               a["out_loss"], 0, a["ws"], None)


def test_bad_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    for name in ("col_class", "col_held", "col_cpos", "col_cneg"):
        assert _call(null=(name,)) == _lib.LLA_EINVAL, name
        assert _call(null=(name, "fold")) == _lib.LLA_EINVAL, name
    assert _call(C=12) == _lib.LLA_EINVAL                  # not a multiple of 8
    assert _call(C=1032) == _lib.LLA_EINVAL                # wider than 1024
    assert _call(C=0) == _lib.LLA_EINVAL
    assert _call(J=0) == _lib.LLA_EINVAL
    assert _call(ld_z=32) == _lib.LLA_EINVAL               # ld_z < C
    assert _call(ld_z=42) == _lib.LLA_EINVAL               # pitch not a multiple of 4
    assert _call(ld_w=32) == _lib.LLA_EINVAL
    assert _call(B=-1) == _lib.LLA_EINVAL
    assert _call(z_dtype=7) == _lib.LLA_EINVAL
    for name in ("z", "y", "W", "b", "out_W", "out_b", "out_loss", "ws"):
        assert _call(null=(name,)) == _lib.LLA_EINVAL, name
    assert _call(V=True, null=("vb",)) == _lib.LLA_EINVAL
    assert L.lla_svm_grid_pass_workspace_bytes(12, 3) == 0 and L.lla_svm_grid_pass_workspace_bytes(40, 0) == 0
    # [problem tiles][workgroups][32 problems][C + 2] floats, at most 512 workgroups: the grid of lla_svm_pass for K = J
    assert L.lla_svm_grid_pass_workspace_bytes(512, 10) == 512 * 32 * 514 * 4
    assert L.lla_svm_grid_pass_workspace_bytes(512, 400) == 13 * 39 * 32 * 514 * 4
    for C, J in ((40, 1), (512, 33), (1024, 4000)):
        assert L.lla_svm_grid_pass_workspace_bytes(C, J) == L.lla_svm_pass_workspace_bytes(C, J) > 0


@pytest.mark.parametrize("N,C,K", [(600, 40, 3), (400, 40, 2)])
def test_class_weight_against_scikit_learn(N, C, K):
    svm = pytest.importorskip("sklearn.svm")
    from lossyless_amd import LinearProbe
    X, y = unbalanced(N, C, K)
    labels = 2 * y + 1                                     # (labels are not class indexes)
    counts = torch.bincount(y)
    assert int(counts.min()) > 0 and int(counts.max()) >= 1.5 * int(counts.min())
    CW = 0.05
    for cw in ("balanced", {1: 2.5, 3: 0.4}):
        probe = LinearProbe(C=CW, tol=TOL, class_weight=cw).fit(X, labels)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            clf = svm.LinearSVC(C=CW, dual=False, tol=1e-12, max_iter=100000, class_weight=cw).fit(X.double().numpy(),
                                                                                                 labels.numpy())
        assert np.array_equal(probe.classes_, clf.classes_) and tuple(probe.coef_.shape) == clf.coef_.shape
        assert probe.converged_
        Y, c = ovr_weights(labels, probe.classes_, CW, cw)
        zero = torch.zeros_like(probe.coef_)
        g0, _ = weighted_grad_norms(zero, zero[:, 0], X, Y, c)
        ginf, _ = weighted_grad_norms(probe.coef_, probe.intercept_, X, Y, c)
        assert ginf <= TOL * g0
        within_strong_convexity(probe.coef_, probe.intercept_, torch.from_numpy(clf.coef_), torch.from_numpy(clf.intercept_),
                                X, Y, c, f"K {K} class_weight {cw}")
        assert np.array_equal(probe.predict(X).numpy(), clf.predict(X.double().numpy()))
        # the weights matter: the unweighted fit is another point
        plain = LinearProbe(C=CW, tol=TOL).fit(X, labels)
        assert float((plain.coef_ - probe.coef_).abs().max()) > 1e-3
    with pytest.raises(ValueError, match="class_weight"):
        LinearProbe(class_weight="even")
    with pytest.raises(ValueError, match="does not have"):
        LinearProbe(class_weight={4: 2.0}).fit(X, labels)


@pytest.fixture(scope="module")
def searched():
    from lossyless_amd import LinearProbeCV
    X, y = make_data(600, 40, 3)
    labels = 2 * y + 1
    cv = LinearProbeCV(CANDIDATES, cv=3, tol=TOL).fit(X, labels)
    return X, labels, cv


def _check_against_standalone_fits(cv, X, labels, fold, candidates):
    from lossyless_amd import LinearProbe
    K = cv.fold_coef_.shape[2]
    assert tuple(cv.fold_coef_.shape) == (len(candidates), len(cv.folds_), K, X.shape[1])
    assert tuple(cv.fold_intercept_.shape) == (len(candidates), len(cv.folds_), K)
    assert tuple(cv.cv_scores_.shape) == (len(candidates), len(cv.folds_)) and cv.cv_scores_.dtype == torch.float64
    assert bool(cv.converged_.all()) and cv.n_passes_ > 0
    for c, (CW, cw) in enumerate(candidates):
        for f, fid in enumerate(cv.folds_):
            train = fold != fid
            alone = LinearProbe(C=CW, tol=TOL, class_weight=cw).fit(X[train], labels[train])
            Y, wts = ovr_weights(labels[train], cv.classes_, CW, cw)
            within_strong_convexity(cv.fold_coef_[c, f], cv.fold_intercept_[c, f], alone.coef_, alone.intercept_, X[train], Y,
                                    wts, f"candidate {c} fold {fid}")
            # the score is the accuracy of the returned coefficients on the held-out rows, evaluated in float64: exact
            right, _, _ = accuracy64(cv.fold_coef_[c, f], cv.fold_intercept_[c, f], X[~train], labels[~train], cv.classes_)
            assert float(cv.cv_scores_[c, f]) == int(right.sum()) / int((~train).sum())
    assert torch.equal(cv.mean_scores_, cv.cv_scores_.mean(1))
    assert cv.best_index_ == int(np.argmax(cv.mean_scores_.numpy()))                   # numpy: the first maximum
    assert cv.best_params_ == dict(C=candidates[cv.best_index_][0], class_weight=candidates[cv.best_index_][1])


def test_search_on_cpu_tensors(searched):
    from lossyless_amd import LinearProbe
    X, labels, cv = searched
    fold = stratified_folds(labels, 3)
    assert np.array_equal(cv.classes_, [1, 3, 5]) and cv.folds_ == [0, 1, 2]
    _check_against_standalone_fits(cv, X, labels, fold, CANDIDATES)
    CW, cw = CANDIDATES[cv.best_index_]
    best, alone = cv.best_estimator_, LinearProbe(C=CW, tol=TOL, class_weight=cw).fit(X, labels)
    assert isinstance(best, LinearProbe) and best.converged_ and best.C == CW and best.class_weight == cw
    Y, wts = ovr_weights(labels, cv.classes_, CW, cw)
    within_strong_convexity(best.coef_, best.intercept_, alone.coef_, alone.intercept_, X, Y, wts, "best_estimator_")
    assert np.array_equal(best.predict(X).numpy(), alone.predict(X).numpy())
    assert tuple(cv.converged_.shape) == (3, 4)
    # class means 0.6 apart, unit noise: the float64 twin leaves next to no held-out row inside the fp32 score bound, so
    # the 1 % cap the device test allows for such rows is reachable on this generator
    assert check_cv_scores(cv, X, labels, fold) <= 0.01


def test_first_maximum_wins(searched):
    from lossyless_amd import LinearProbeCV
    X, labels, cv = searched
    twice = LinearProbeCV([CANDIDATES[1], CANDIDATES[0], CANDIDATES[1], CANDIDATES[0]], cv=3, tol=TOL, refit=False).fit(X, labels)
    assert torch.equal(twice.cv_scores_[0], twice.cv_scores_[2]) and torch.equal(twice.cv_scores_[1], twice.cv_scores_[3])
    assert twice.best_index_ in (0, 1) and twice.best_estimator_ is None and tuple(twice.converged_.shape) == (4, 3)
    assert torch.equal(twice.fold_coef_[0], twice.fold_coef_[2])


def test_folds_given_as_an_array_with_rows_that_always_train(searched):
    from lossyless_amd import LinearProbeCV
    X, labels, _ = searched
    g = torch.Generator().manual_seed(4)
    fold = torch.tensor([-1, 0, 5])[torch.randint(0, 3, (600,), generator=g)]        # (fold ids need not be 0 .. n-1)
    cands = CANDIDATES[:2]
    cv = LinearProbeCV(cands, cv=fold.numpy(), tol=TOL, refit=False).fit(X, labels)
    assert cv.folds_ == [0, 5] and int((fold == -1).sum()) > 100
    _check_against_standalone_fits(cv, X, labels, fold, cands)
    with pytest.raises(ValueError, match="fold ids"):
        LinearProbeCV(cands, cv=(fold - 1).numpy()).fit(X, labels)
    with pytest.raises(ValueError, match="fold ids"):
        LinearProbeCV(cands, cv=fold[:-1].numpy()).fit(X, labels)


def test_two_classes():
    from lossyless_amd import LinearProbeCV
    X, y = make_data(400, 40, 2)
    labels = 2 * y + 1
    cands = [(0.05, "balanced"), (7e-3, {1: 2.0})]
    cv = LinearProbeCV(cands, cv=4, tol=TOL).fit(X, labels)
    assert tuple(cv.fold_coef_.shape) == (2, 4, 1, 40)
    _check_against_standalone_fits(cv, X, labels, stratified_folds(labels, 4), cands)
    assert tuple(cv.best_estimator_.coef_.shape) == (1, 40)
    assert cv.best_estimator_.score(X, labels) > 0.9


def test_a_training_part_without_a_class_is_refused(searched, monkeypatch):
    from lossyless_amd import LinearProbeCV, probe
    X, labels, _ = searched

    def no_walk(self):
        raise AssertionError("the rows were walked before the folds were checked")
    monkeypatch.setattr(probe._Rows, "groups", no_walk)
    fold = torch.where(labels == 5, 1, 0)                                   # holding fold 1 out removes class 5
    with pytest.raises(ValueError, match="lacks a class"):
        LinearProbeCV(CANDIDATES, cv=fold.numpy()).fit(X, labels)
    with pytest.raises(ValueError, match="holds no row"):
        LinearProbeCV(CANDIDATES, cv=400).fit(X, labels)                    # more folds than rows of a class
    with pytest.raises(ValueError, match="at least 2"):
        LinearProbeCV(CANDIDATES, cv=1).fit(X, labels)
    with pytest.raises(ValueError, match="candidates"):
        LinearProbeCV([])


def test_batches_of_problems_give_the_same_coefficients(searched):
    from lossyless_amd import LinearProbeCV
    X, labels, cv = searched
    # 12 classifiers of 3 problems: 15 problems at a time is 5 classifiers, three batches.  Problems are independent and
    # a masked term is an exact zero, but a float64 matrix product of another width may group its sums differently
    # (the BLAS picks its blocking by shape), so equality to the bit is tried first and the bound holds in any case
    few = LinearProbeCV(CANDIDATES, cv=3, tol=TOL, max_problems=15).fit(X, labels)
    assert few.n_passes_ > cv.n_passes_
    assert torch.equal(few.cv_scores_, cv.cv_scores_) and few.best_index_ == cv.best_index_
    same = torch.equal(few.fold_coef_, cv.fold_coef_) and torch.equal(few.fold_intercept_, cv.fold_intercept_)
    print(f"batched coefficients equal to the bit: {same}; max difference {float((few.fold_coef_ - cv.fold_coef_).abs().max()):.3e}")
    fold = stratified_folds(labels, 3)
    for c, (CW, cw) in enumerate(CANDIDATES):
        for f in range(3):
            train = fold != f
            Y, wts = ovr_weights(labels[train], cv.classes_, CW, cw)
            within_strong_convexity(few.fold_coef_[c, f], few.fold_intercept_[c, f], cv.fold_coef_[c, f], cv.fold_intercept_[c, f],
                                    X[train], Y, wts, f"candidate {c} fold {f}")
    assert same


def test_sampler_is_seeded_and_in_range():
    from lossyless_amd import LinearProbeCV
    a, b = LinearProbeCV.sample(64, seed=3), LinearProbeCV.sample(64, seed=3)
    assert a == b and a != LinearProbeCV.sample(64, seed=4) and len(a) == 64
    assert all(1e-3 <= C <= 1.0 and cw in ("balanced", None) for C, cw in a)
    assert {cw for _, cw in a} == {"balanced", None}
    logs = np.log10([C for C, _ in a])
    assert logs.min() < -2.5 and logs.max() > -0.5 and abs(float(np.median(logs)) + 1.5) < 0.5      # log-uniform over three decades
    narrow = LinearProbeCV.sample(16, seed=0, low=0.01, high=0.02)
    assert all(0.01 <= C <= 0.02 for C, _ in narrow)
    LinearProbeCV(a)                                                        # (candidates as the constructor takes them)


def test_compressed_latents_on_the_cpu(tmp_path):
    import hubconf
    from lossyless_amd import LinearProbeCV
    comp, _ = hubconf.clip_compressor_b005(device="cpu", clip_weights="synthetic")
    N = 300
    file, _, _ = write_dataset(tmp_path, "5e-02", N, seed=17)
    ds = comp.open_dataset(file, device="cpu")
    labels = torch.arange(N) % 3
    rows = ds.all()
    # (sampled records carry escapes: the solve is far from done after two Newton steps -- what is under test here is
    # that the streamed path and the array path are the same search, as in test_probe_host.py)
    def fit(data, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return LinearProbeCV(CANDIDATES[:2], cv=3, max_iter=2).fit(data, labels, **kw)
    b = fit(rows, rows_per_pass=128)
    for kw in (dict(rows_per_pass=128), dict(rows_per_pass=128, keep_rows=True)):
        a = fit(ds, **kw)
        assert torch.equal(a.fold_coef_, b.fold_coef_) and torch.equal(a.fold_intercept_, b.fold_intercept_)
        assert torch.equal(a.cv_scores_, b.cv_scores_) and a.n_passes_ == b.n_passes_ and a.best_index_ == b.best_index_
        assert torch.equal(a.best_estimator_.coef_, b.best_estimator_.coef_) and bool(a.fold_coef_.abs().max() > 0)
    assert a.best_estimator_.score(ds, labels) == b.best_estimator_.score(rows, labels)
