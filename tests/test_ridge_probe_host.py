"""CPU: the Gram entry points are declared, bound, exported and built; ``lla_gram_pass`` / ``lla_segment_sums`` refuse what the
header says they refuse before any device call; ``RidgeProbe``'s float64 twin against scikit-learn's ``Ridge`` /
``RidgeClassifier``; ``path``; ``RidgeProbeCV`` against per-fold scikit-learn fits on the same folds; ties; the errors; and
latents opened on the CPU against their decompressed rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lossyless_amd
from conftest import ROOT
from latents_util import write_dataset
from lossyless_amd import RidgeProbe, RidgeProbeCV, _lib
from probe_util import P
from ridge_util import make_ridge_data

NEW = ("lla_gram_pass_workspace_bytes", "lla_gram_pass", "lla_segment_sums")
N, C, K, NT = 300, 24, 5, 3
ALPHAS = (1e-3, 1.0, 100.0)


def test_symbols_are_declared_bound_exported_and_built():
    with open(os.path.join(ROOT, "include", "lossyless_amd.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} not declared"
        assert name in _lib.EXPORTS and hasattr(raw, name), f"{name} not bound / exported"
    with open(os.path.join(ROOT, "lossyless_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert "gram.hip" in re.search(r"^SHARED\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert _lib.lib().lla_abi_version() == _lib.ABI_VERSION == 4
    for cls in (RidgeProbe, RidgeProbeCV):
        assert cls.__name__ in lossyless_amd.__all__ and getattr(lossyless_amd, cls.__name__) is cls


def test_gram_pass_refusals_come_before_any_device_call():
    """Host memory stands in for every pointer: a refused call never reads it, and no device is present."""
    L = _lib.lib()
    Cc, B, T = 16, 40, 3
    z, t = np.zeros((B, 24), dtype=np.float32), np.zeros((B, 4), dtype=np.float32)
    gram, s, cross = np.full((Cc, Cc), 7.0), np.full(Cc, 7.0), np.full((T, Cc), 7.0)
    tsum, tsq = np.full(4, 7.0), np.full(4, 7.0)
    ws = np.zeros(1 << 16, dtype=np.uint8)
    for a in (z, t, gram, s, cross, tsum, tsq, ws):
        assert a.ctypes.data % 16 == 0
    off = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)                                       # noqa: E731

    def run(**kw):
        v = dict(z=P(z), dt=_lib.LLA_Z_F32, ld_z=24, B=B, C=Cc, t=P(t), ld_t=4, T=T, gram=P(gram), sum=P(s), cross=P(cross),
                 tsum=P(tsum), tsq=P(tsq), acc=0, ws=P(ws))
        v.update(kw)
        return L.lla_gram_pass(v["z"], v["dt"], v["ld_z"], v["B"], v["C"], v["t"], v["ld_t"], v["T"], v["gram"], v["sum"],
                               v["cross"], v["tsum"], v["tsq"], v["acc"], v["ws"], None)

    bad = [dict(C=12), dict(C=0), dict(C=-8), dict(C=1032, ld_z=1032), dict(B=-1), dict(ld_z=8), dict(ld_z=18), dict(dt=0),
           dict(dt=3), dict(z=off(z, 4)), dict(z=off(z, 8)), dict(z=off(z, 4), dt=_lib.LLA_Z_F16), dict(z=None),
           dict(T=0), dict(T=-1), dict(T=4097, ld_t=4097), dict(ld_t=2), dict(t=off(t, 2)), dict(t=None), dict(t=None, T=0, ld_t=0, B=-1),
           dict(gram=None), dict(sum=None), dict(cross=None), dict(tsum=None), dict(tsq=None), dict(ws=None),
           dict(gram=off(gram, 8)), dict(sum=off(s, 8)), dict(cross=off(cross, 8)), dict(tsum=off(tsum, 8)),
           dict(tsq=off(tsq, 8)), dict(ws=off(ws, 8))]
    for kw in bad:
        assert run(**kw) == _lib.LLA_EINVAL, kw
    # B == 0 with accumulate: LLA_OK, nothing launched or touched (fp16 rows need 8 bytes only; no targets: their outputs may be NULL)
    assert run(B=0, acc=1) == _lib.LLA_OK and run(z=off(z, 8), dt=_lib.LLA_Z_F16, B=0, acc=1) == _lib.LLA_OK
    assert run(B=0, acc=1, t=None, T=0, ld_t=0, cross=None, tsum=None, tsq=None) == _lib.LLA_OK
    assert all(bool((a == 7).all()) for a in (gram, s, cross, tsum, tsq))
    for C_, T_ in ((12, 0), (0, 0), (1032, 0), (-8, 0), (8, -1), (8, 4097)):
        assert int(L.lla_gram_pass_workspace_bytes(C_, T_)) == 0, (C_, T_)
    for C_, T_ in ((8, 0), (512, 0), (512, 3), (1024, 0), (1024, 4096), (136, 33)):
        assert int(L.lla_gram_pass_workspace_bytes(C_, T_)) > 0, (C_, T_)


def test_segment_sums_refusals_come_before_any_device_call():
    L = _lib.lib()
    Cc, B = 16, 40
    z, out = np.zeros((B, 24), dtype=np.float32), np.full((3, Cc), 7.0)
    good = np.array([0, 10, 10, 40], dtype=np.int32)
    off = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)                                       # noqa: E731

    def run(**kw):
        v = dict(z=P(z), dt=_lib.LLA_Z_F32, ld_z=24, B=B, C=Cc, seg=good, S=3, out=P(out), acc=0)
        v.update(kw)
        seg = v["seg"]
        return L.lla_segment_sums(v["z"], v["dt"], v["ld_z"], v["B"], v["C"], None if seg is None else P(seg), v["S"],
                                  v["out"], v["acc"], None)

    i32 = lambda *a: np.array(a, dtype=np.int32)                                                # noqa: E731
    bad = [dict(C=12), dict(C=1032, ld_z=1032), dict(B=-1), dict(ld_z=8), dict(ld_z=18), dict(dt=0), dict(z=off(z, 4)),
           dict(z=None), dict(seg=None), dict(S=0), dict(S=-1), dict(out=None), dict(out=off(out, 8)),
           dict(seg=i32(1, 10, 10, 40)), dict(seg=i32(0, 10, 10, 39)), dict(seg=i32(0, 10, 10, 41)), dict(seg=i32(0, 20, 10, 40)),
           dict(seg=i32(0, 41, 41, 40)), dict(seg=i32(0, -1, 10, 40))]
    for kw in bad:
        assert run(**kw) == _lib.LLA_EINVAL, {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    assert run(B=0, acc=1, seg=i32(0, 0, 0, 0)) == _lib.LLA_OK and bool((out == 7).all())


@pytest.fixture(scope="module")
def data():
    X, y, T = make_ridge_data(N, C, K, NT, seed=5)
    return X, y, T, X.double().numpy(), y.numpy(), T.double().numpy()


def _close(probe, want, what):
    """The issue's tolerance: relative coefficient and absolute intercept difference <= 1e-9."""
    coef, icpt = np.atleast_2d(want.coef_), np.atleast_1d(want.intercept_)
    assert probe.coef_.dtype == torch.float64 and tuple(probe.coef_.shape) == coef.shape, what
    rel = np.abs(probe.coef_.numpy() - coef).max() / np.abs(coef).max()
    gap = np.abs(probe.intercept_.numpy() - icpt).max()
    assert rel <= 1e-9 and gap <= 1e-9, f"{what}: coefficients {rel:.3g}, intercept {gap:.3g}"


def test_twin_against_scikit_learn(data):
    lm = pytest.importorskip("sklearn.linear_model")
    X, y, T, X64, y64, T64 = data
    yb = np.where(y64 > 1, 7, -2)
    for alpha in ALPHAS:
        for kw in (dict(), dict(rows_per_pass=77)):
            p = RidgeProbe(alpha).fit(X, T, **kw)
            want = lm.Ridge(alpha=alpha, solver="cholesky").fit(X64, T64)
            _close(p, want, f"Ridge alpha {alpha}")
            assert abs(p.score(X, T) - want.score(X64, T64)) <= 1e-12
            assert np.abs(p.predict(X, rows_per_pass=50).numpy() - want.predict(X64)).max() <= 1e-9
            p = RidgeProbe(alpha).fit(X, y, **kw)
            want = lm.RidgeClassifier(alpha=alpha, solver="cholesky").fit(X64, y64)
            _close(p, want, f"RidgeClassifier alpha {alpha}")
            assert np.array_equal(p.classes_, want.classes_) and np.array_equal(p.predict(X).numpy(), want.predict(X64))
            assert p.score(X, y) == want.score(X64, y64) and p.n_passes_ == 1
            p = RidgeProbe(alpha).fit(X, yb, **kw)
            want = lm.RidgeClassifier(alpha=alpha, solver="cholesky").fit(X64, yb)
            _close(p, want, f"binary RidgeClassifier alpha {alpha}")
            assert tuple(p.decision_function(X).shape) == (N,) and np.array_equal(p.predict(X).numpy(), want.predict(X64))
    # one target given as [N]: predictions come back as [N]; no intercept
    p = RidgeProbe(1.0).fit(X, T[:, 0])
    _close(p, lm.Ridge(alpha=1.0, solver="cholesky").fit(X64, T64[:, :1]), "one target")
    assert tuple(p.predict(X).shape) == (N,)
    p = RidgeProbe(1.0, fit_intercept=False).fit(X, T)
    _close(p, lm.Ridge(alpha=1.0, solver="cholesky", fit_intercept=False).fit(X64, T64), "no intercept")
    assert bool((p.intercept_ == 0).all())
    p = RidgeProbe(1.0, fit_intercept=False).fit(X, y)
    _close(p, lm.RidgeClassifier(alpha=1.0, solver="cholesky", fit_intercept=False).fit(X64, y64), "classifier, no intercept")


def test_path_equals_separate_fits(data):
    X, y, T = data[:3]
    for target in (y, T):
        base = RidgeProbe(3.0).fit(X, target)
        for probe, alpha in zip(base.path(ALPHAS), ALPHAS):
            own = RidgeProbe(alpha).fit(X, target)
            assert probe.alpha == alpha and probe.moments_ is base.moments_
            assert float((probe.coef_ - own.coef_).abs().max()) <= 1e-12 * float(own.coef_.abs().max())
            assert float((probe.intercept_ - own.intercept_).abs().max()) <= 1e-12
            assert torch.equal(probe.predict(X), own.predict(X))
    with pytest.raises(RuntimeError, match="fit first"):
        RidgeProbe().path([1.0])


def test_cv_against_per_fold_scikit_learn(data):
    lm = pytest.importorskip("sklearn.linear_model")
    X, y, T, X64, y64, T64 = data
    fold = torch.from_numpy(np.random.default_rng(3).integers(0, 4, N))
    fold[:7] = -1                                               # rows that always train
    f64 = fold.numpy()
    for kw in (dict(), dict(rows_per_pass=64), dict(rows_per_pass=64, keep_rows=True)):
        cv = RidgeProbeCV(ALPHAS, cv=fold).fit(X, y, **kw)
        assert cv.n_passes_ == 2 and cv.folds_ == [0, 1, 2, 3] and tuple(cv.cv_scores_.shape) == (3, 4)
        reg = RidgeProbeCV(ALPHAS, cv=fold).fit(X, T, **kw)
        assert reg.n_passes_ == 1
        for a, alpha in enumerate(ALPHAS):
            for f in range(4):
                tr, te = f64 != f, f64 == f
                want = lm.RidgeClassifier(alpha=alpha, solver="cholesky").fit(X64[tr], y64[tr])
                right = int((want.predict(X64[te]) == y64[te]).sum())
                assert round(float(cv.cv_scores_[a, f]) * int(te.sum())) == right, (alpha, f)
                want = lm.Ridge(alpha=alpha, solver="cholesky").fit(X64[tr], T64[tr])
                mse = float(((want.predict(X64[te]) - T64[te]) ** 2).mean())
                assert abs(-float(reg.cv_scores_[a, f]) - mse) <= 1e-9 * mse, (alpha, f)
                assert np.abs(reg.fold_coef_[a, f].numpy() - want.coef_).max() <= 1e-9 * np.abs(want.coef_).max()
    # integer cv: the stratified folds of the other CV classes / scikit-learn's unshuffled KFold
    ms = pytest.importorskip("sklearn.model_selection")
    reg = RidgeProbeCV(ALPHAS, cv=5).fit(X, T, rows_per_pass=100)
    for a, alpha in enumerate(ALPHAS):
        want = ms.cross_val_score(lm.Ridge(alpha=alpha, solver="cholesky"), X64, T64, cv=ms.KFold(5), scoring="neg_mean_squared_error")
        assert np.abs(reg.cv_scores_[a].numpy() - want).max() <= 1e-9 * np.abs(want).max()
    from lossyless_amd.probe import _folds_of
    cls = torch.searchsorted(torch.unique(y), y)
    strat = _folds_of(5, cls, K)[0]
    a, b = RidgeProbeCV(ALPHAS, cv=5).fit(X, y), RidgeProbeCV(ALPHAS, cv=strat).fit(X, y)
    assert torch.equal(a.cv_scores_, b.cv_scores_)


def test_ties_pick_the_lowest_alpha_and_best_estimator_is_the_full_fit(data):
    X, y, T = data[:3]
    Xs = X.clone()
    Xs[:, 0] = (y.float() - 2) * 50                             # separable: every small alpha scores 1.0 on every fold
    cv = RidgeProbeCV([10.0, 1e-3, 1.0, 1e-3], cv=3).fit(Xs, y)
    assert bool((cv.cv_scores_[:3] == 1.0).all()) and cv.best_params_ == {"alpha": 1e-3} and cv.best_index_ == 1
    for target, fit_intercept in ((y, True), (T, True), (T, False)):
        cv = RidgeProbeCV(ALPHAS, cv=4, fit_intercept=fit_intercept).fit(X, target, rows_per_pass=90)
        own = RidgeProbe(cv.best_params_["alpha"], fit_intercept).fit(X, target)
        assert cv.best_index_ == int(cv.mean_scores_.argmax())
        assert float((cv.best_estimator_.coef_ - own.coef_).abs().max()) <= 1e-11 * float(own.coef_.abs().max())
        assert float((cv.best_estimator_.intercept_ - own.intercept_).abs().max()) <= 1e-11
        assert torch.equal(cv.best_estimator_.predict(X), own.predict(X)) if target is y else True
    assert RidgeProbeCV.logspace(3, 1e-2, 1.0) == pytest.approx([1e-2, 1e-1, 1.0])


def test_errors(data):
    X, y, T = data[:3]
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            RidgeProbe(alpha=bad)
        with pytest.raises(ValueError):
            RidgeProbeCV([1.0, bad])
    with pytest.raises(ValueError):
        RidgeProbeCV([])
    with pytest.raises(ValueError):
        RidgeProbeCV.logspace(3, 0.0, 1.0)
    for target in (T[:-1], T[:, :, None], y[:-1], torch.zeros(N, 0)):
        with pytest.raises(ValueError):
            RidgeProbe().fit(X, target)
    with pytest.raises(ValueError):
        RidgeProbe().fit(X)                                     # no labels anywhere
    with pytest.raises(ValueError):
        RidgeProbe().fit(X, torch.zeros(N, dtype=torch.int64))  # one class
    nan = X.clone()
    nan[17, 3] = float("nan")
    for target in (y, T):
        with pytest.raises(ValueError):
            RidgeProbe().fit(nan, target)
        with pytest.raises(ValueError):
            RidgeProbeCV([1.0], cv=3).fit(nan, target, rows_per_pass=64)
    bad_t = T.clone()
    bad_t[3, 1] = float("inf")
    with pytest.raises(ValueError):
        RidgeProbe().fit(X, bad_t)
    for cv in (1, N + 1, torch.zeros(N, dtype=torch.int64), torch.zeros(N - 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            RidgeProbeCV([1.0], cv=cv).fit(X, T)
    with pytest.raises(RuntimeError, match="fit first"):
        RidgeProbe().predict(X)
    probe = RidgeProbe().fit(X, T)
    with pytest.raises(ValueError):
        probe.predict(X[:, :8])
    with pytest.raises(ValueError):
        probe.score(X, T[:, :2])
    with pytest.raises(ValueError):
        probe.score(X, y)


def test_compressed_latents_on_the_cpu(tmp_path):
    import hubconf
    comp, _ = hubconf.clip_compressor_b005(device="cpu", clip_weights="synthetic")
    n = 200
    file, _, _ = write_dataset(tmp_path, "5e-02", n, seed=23)
    y = np.arange(n) % 4
    np.save(tmp_path / "labels.npy", y)
    ds = comp.open_dataset(file, device="cpu", label_file=str(tmp_path / "labels.npy"))
    rows = ds.all()
    t = torch.from_numpy(np.random.default_rng(1).normal(size=(n, 2)))
    for target in (None, t):
        a = RidgeProbe(2.0).fit(ds, target, rows_per_pass=64)
        b = RidgeProbe(2.0).fit(rows, torch.from_numpy(y) if target is None else target, rows_per_pass=64)
        c = RidgeProbe(2.0).fit(ds, target, rows_per_pass=64, keep_rows=True)
        assert torch.equal(a.coef_, b.coef_) and torch.equal(a.coef_, c.coef_) and torch.equal(a.intercept_, b.intercept_)
        assert all(torch.equal(a.moments_[k], b.moments_[k]) for k in ("gram", "sum", "cross", "tsum", "tsq"))
        cva = RidgeProbeCV([0.1, 10.0], cv=3).fit(ds, target, rows_per_pass=64)
        cvb = RidgeProbeCV([0.1, 10.0], cv=3).fit(rows, torch.from_numpy(y) if target is None else target, rows_per_pass=64)
        assert torch.equal(cva.cv_scores_, cvb.cv_scores_) and torch.equal(cva.best_estimator_.coef_, cvb.best_estimator_.coef_)
    assert a.predict(ds, rows_per_pass=77).shape == (n, 2)
