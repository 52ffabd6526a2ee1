"""CPU: ``lla_softmax_pass`` is declared, bound and refuses bad arguments before any device call; ``LogisticProbe`` on the
CPU (the float64 evaluation that the GPU tests use as their oracle) solves scikit-learn's LogisticRegression objective."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
from latents_util import write_dataset
from logistic_util import binomial_objective64, row_weights, softmax_objective64
from lossyless_amd import _lib
from probe_util import make_data

CW, TOL = 1.0, 1e-4


def test_symbols_are_declared_bound_and_exported():
    import lossyless_amd
    with open(os.path.join(ROOT, "include", "lossyless_amd.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lla_softmax_pass", "lla_softmax_pass_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} not declared"
        assert name in _lib.EXPORTS and hasattr(raw, name), f"{name} not bound / exported"
    assert _lib.lib().lla_abi_version() == _lib.ABI_VERSION == 4          # additive: the ABI version stays
    assert "LogisticProbe" in lossyless_amd.__all__ and lossyless_amd.LogisticProbe is not None


def _call(C=40, K=3, B=16, ld_z=None, ld_w=None, null=(), z_dtype=None, V=False, shift=None):
    """lla_softmax_pass on host buffers it must never read: every call here is refused by the argument checks."""
    L = _lib.lib()
    buf = np.zeros(1 << 16, dtype=np.float64)          # 16-byte aligned stand-in for every pointer
    p = ctypes.c_void_p(buf.ctypes.data + (-buf.ctypes.data) % 16)
    a = dict(z=p, y=p, W=p, b=p, V=p if V else None, vb=p if V else None, cw=p, out_W=p, out_b=p, out_loss=p, ws=p)
    for k in null:
        a[k] = None
    if shift is not None:                              # a pointer off its alignment
        a[shift[0]] = ctypes.c_void_p(p.value + shift[1])
    return L.lla_softmax_pass(a["z"], _lib.LLA_Z_F32 if z_dtype is None else z_dtype, C if ld_z is None else ld_z, a["y"], B,
                              C, a["W"], a["b"], a["V"], a["vb"], K, C if ld_w is None else ld_w, a["cw"], a["out_W"],
                              a["out_b"], a["out_loss"], 0, a["ws"], None)


def test_bad_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    assert _call(C=12) == _lib.LLA_EINVAL                  # not a multiple of 8
    assert _call(C=1032) == _lib.LLA_EINVAL                # wider than 1024
    assert _call(C=0) == _lib.LLA_EINVAL
    assert _call(K=0) == _lib.LLA_EINVAL
    assert _call(ld_z=32) == _lib.LLA_EINVAL               # ld_z < C
    assert _call(ld_z=42) == _lib.LLA_EINVAL               # pitch not a multiple of 4
    assert _call(ld_w=32) == _lib.LLA_EINVAL
    assert _call(ld_w=42) == _lib.LLA_EINVAL
    assert _call(B=-1) == _lib.LLA_EINVAL
    assert _call(z_dtype=7) == _lib.LLA_EINVAL
    for name in ("z", "y", "W", "b", "out_W", "out_b", "out_loss", "ws"):   # (out_loss: gradient mode needs it)
        assert _call(null=(name,)) == _lib.LLA_EINVAL, name
    assert _call(V=True, null=("vb",)) == _lib.LLA_EINVAL
    assert _call(shift=("z", 8)) == _lib.LLA_EINVAL        # fp32 rows want 16 bytes
    assert _call(shift=("z", 4), z_dtype=_lib.LLA_Z_F16) == _lib.LLA_EINVAL
    assert _call(shift=("W", 8)) == _lib.LLA_EINVAL
    assert _call(V=True, shift=("V", 8)) == _lib.LLA_EINVAL
    assert _call(shift=("ws", 2)) == _lib.LLA_EINVAL
    for C, K, B in ((12, 3, 16), (1032, 3, 16), (40, 0, 16), (40, 3, -1)):
        assert L.lla_softmax_pass_workspace_bytes(C, K, B) == 0
    # the partial sums of lla_svm_pass; lse [B] and a [B] behind them once the classes span more than one tile
    assert L.lla_softmax_pass_workspace_bytes(512, 10, 4096) == L.lla_svm_pass_workspace_bytes(512, 10)
    assert L.lla_softmax_pass_workspace_bytes(512, 32, 4096) == L.lla_svm_pass_workspace_bytes(512, 32)
    assert L.lla_softmax_pass_workspace_bytes(512, 33, 4096) == L.lla_svm_pass_workspace_bytes(512, 33) + 2 * 4096 * 4


def _unbalanced(N, C, K):
    """make_data with class k given about (k + 1) shares of the rows (every class present)."""
    X, _ = make_data(N, C, K)
    g = torch.Generator().manual_seed(N + K)
    shares = torch.arange(1, K + 1, dtype=torch.float64)
    y = torch.multinomial(shares / shares.sum(), N, replacement=True, generator=g)
    y[:K] = torch.arange(K)
    mu = torch.randn(K, C, generator=g) * 0.6
    return (X + mu[y]).float(), y


def _stacked(W, b):
    return torch.cat([W.double(), b.double()[:, None]], 1)


@pytest.mark.parametrize("class_weight", [None, "balanced", "dict"])
@pytest.mark.parametrize("N,C,K", [(600, 40, 3), (300, 40, 33), (900, 64, 37)])
def test_cpu_solver_against_scikit_learn(N, C, K, class_weight):
    lm = pytest.importorskip("sklearn.linear_model")
    from lossyless_amd import LogisticProbe
    X, y = _unbalanced(N, C, K)
    labels = 2 * y + 1                                     # (labels are not class indexes)
    if class_weight == "dict":
        class_weight = {1: 2.5, 5: 0.3}                    # labels left out weigh 1
    probe = LogisticProbe(C=CW, tol=TOL, class_weight=class_weight).fit(X, labels)
    X1 = torch.cat([X.double(), torch.ones(N, 1, dtype=torch.float64)], 1).numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = lm.LogisticRegression(C=CW, fit_intercept=False, tol=1e-12, max_iter=20000,
                                    class_weight=class_weight).fit(X1, labels.numpy())
    assert np.array_equal(probe.classes_, clf.classes_)
    assert tuple(probe.coef_.shape) == (K, C) and tuple(probe.intercept_.shape) == (K,)
    assert probe.coef_.dtype == torch.float32 and probe.converged_ and probe.n_passes_ > 0
    idx, w = row_weights(probe, labels, class_weight)
    Wsk, bsk = torch.from_numpy(clf.coef_[:, :C]), torch.from_numpy(clf.coef_[:, C])
    zero = torch.zeros(K, C, dtype=torch.float64)
    _, g0W, g0b = softmax_objective64(zero, zero[:, 0], X, idx, w, CW)
    f, gW, gb = softmax_objective64(probe.coef_, probe.intercept_, X, idx, w, CW)
    _, gWsk, gbsk = softmax_objective64(Wsk, bsk, X, idx, w, CW)
    g2, g2_sk = float(_stacked(gW, gb).norm()), float(_stacked(gWsk, gbsk).norm())
    dist = float((_stacked(probe.coef_, probe.intercept_) - _stacked(Wsk, bsk)).norm())
    ginf, g0 = float(_stacked(gW, gb).abs().max()), float(_stacked(g0W, g0b).abs().max())     # (printed, not asserted)
    print(f"N {N} C {C} K {K} {class_weight}: passes {probe.n_passes_}, |g|inf {ginf:.3e} (tol |g0|inf {TOL * g0:.3e}), "
          f"|W - W_sk| {dist:.3e} (|g| {g2:.3e} + |g_sk| {g2_sk:.3e})")
    assert dist <= g2 + g2_sk                              # f is 1-strongly convex: |W - W*| <= |grad f(W)|
    assert abs(probe.objective_ - float(f)) <= 1e-6 * float(f)
    assert np.array_equal(probe.predict(X).numpy(), clf.predict(X1))
    assert probe.score(X, labels) == float((probe.predict(X) == labels).double().mean())
    proba = probe.predict_proba(X)
    assert tuple(proba.shape) == (N, K) and float((proba.sum(1) - 1).abs().max()) < 1e-12
    assert float((proba - torch.from_numpy(clf.predict_proba(X1))).abs().max()) <= 2 * dist * float(X.double().norm(dim=1).max() + 1)


@pytest.mark.parametrize("class_weight", [None, "balanced"])
def test_two_classes_are_the_binomial_problem(class_weight):
    lm = pytest.importorskip("sklearn.linear_model")
    from lossyless_amd import LogisticProbe
    N, C = 400, 40
    X, y = _unbalanced(N, C, 2)
    labels = 2 * y + 1
    probe = LogisticProbe(C=CW, tol=TOL, class_weight=class_weight).fit(X, labels)
    X1 = torch.cat([X.double(), torch.ones(N, 1, dtype=torch.float64)], 1).numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = lm.LogisticRegression(C=CW, fit_intercept=False, tol=1e-12, max_iter=20000,
                                    class_weight=class_weight).fit(X1, labels.numpy())
    assert tuple(probe.coef_.shape) == (1, C) and tuple(probe.intercept_.shape) == (1,) and probe.converged_
    idx, w = row_weights(probe, labels, class_weight)
    sign = 2.0 * idx.double() - 1.0                        # classes_[1] is the positive class
    wsk, bsk = torch.from_numpy(clf.coef_[0, :C]), float(clf.coef_[0, C])
    f, gw, gb = binomial_objective64(probe.coef_[0], probe.intercept_[0], X, sign, w, CW)
    _, gwsk, gbsk = binomial_objective64(wsk, bsk, X, sign, w, CW)
    g2, g2_sk = float(torch.cat([gw, gb[None]]).norm()), float(torch.cat([gwsk, gbsk[None]]).norm())
    dist = float(torch.cat([probe.coef_[0].double() - wsk, (probe.intercept_.double() - bsk)]).norm())
    print(f"two classes {class_weight}: passes {probe.n_passes_}, |w - w_sk| {dist:.3e} (|g| {g2:.3e} + |g_sk| {g2_sk:.3e})")
    assert dist <= g2 + g2_sk
    assert abs(probe.objective_ - float(f)) <= 1e-6 * float(f)
    s = probe.decision_function(X)
    assert s.dim() == 1 and tuple(s.shape) == (N,)
    proba = probe.predict_proba(X)
    assert tuple(proba.shape) == (N, 2) and float((proba.sum(1) - 1).abs().max()) < 1e-12
    assert torch.equal(proba[:, 1], torch.sigmoid(s))
    assert np.array_equal(probe.predict(X).numpy(), clf.predict(X1))


def test_groups_give_the_bits_of_one_group():
    from lossyless_amd import LogisticProbe
    from lossyless_amd.probe import _HOST_BLOCK
    for N, K in ((600, 3), (_HOST_BLOCK + 700, 5)):        # less than one block of the twin, and more
        X, y = _unbalanced(N, 24, K)
        one = LogisticProbe(C=CW, tol=TOL, class_weight="balanced").fit(X, y)
        for rows_per_pass in (128, 1000):
            g = LogisticProbe(C=CW, tol=TOL, class_weight="balanced").fit(X, y, rows_per_pass=rows_per_pass)
            assert torch.equal(g.coef_, one.coef_) and torch.equal(g.intercept_, one.intercept_)
            assert g.objective_ == one.objective_ and g.n_passes_ == one.n_passes_
            assert torch.equal(g.decision_function(X, rows_per_pass=rows_per_pass), one.decision_function(X))


def test_compressed_latents_on_the_cpu(tmp_path):
    import hubconf
    from lossyless_amd import LogisticProbe
    comp, _ = hubconf.clip_compressor_b005(device="cpu", clip_weights="synthetic")
    N = 300
    file, lf, _ = write_dataset(tmp_path, "5e-02", N, seed=17)
    ds = comp.open_dataset(file, device="cpu")
    labels = torch.arange(N) % 3
    rows = ds.all()
    # (sampled records carry escapes of up to 2^20 quantisation steps: rows of norm 1e5 on which the solve is far from done
    # after two Newton steps -- what is under test here is that the streamed path and the array path are the same sums)
    def fit(data, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return LogisticProbe(C=1e-6, max_iter=2).fit(data, labels, **kw)
    a = fit(ds, rows_per_pass=128)
    b = fit(rows)
    assert torch.equal(a.coef_, b.coef_) and torch.equal(a.intercept_, b.intercept_) and a.n_passes_ == b.n_passes_
    assert a.objective_ == b.objective_ and bool(a.coef_.abs().max() > 0) and bool(torch.isfinite(a.coef_).all())
    assert torch.equal(fit(ds, rows_per_pass=128, keep_rows=True).coef_, a.coef_)
    assert torch.equal(a.decision_function(ds), a.decision_function(rows)) and tuple(a.decision_function(ds).shape) == (N, 3)
    assert a.score(ds, labels) == float((a.predict(ds) == labels).double().mean())
    assert float((a.predict_proba(ds).sum(1) - 1).abs().max()) < 1e-12
    # the object's own labels are used when none are given
    with_labels = comp.open_dataset(file, label_file=lf, device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        own = LogisticProbe(C=1e-6, max_iter=1).fit(with_labels, rows_per_pass=128)
    assert np.array_equal(own.classes_, np.arange(N)) and tuple(own.coef_.shape) == (N, 512)


def test_errors():
    from lossyless_amd import LogisticProbe
    X, y = make_data(60, 16, 3)
    with pytest.raises(TypeError, match="integers"):
        LogisticProbe().fit(X, y.float())
    with pytest.raises(ValueError, match="labels for"):
        LogisticProbe().fit(X, y[:-1])
    with pytest.raises(ValueError, match="labels"):
        LogisticProbe().fit(X)
    with pytest.raises(ValueError, match="two classes"):
        LogisticProbe().fit(X, torch.zeros(60, dtype=torch.int64))
    with pytest.raises(ValueError, match="class_weight"):
        LogisticProbe(class_weight="heavy")
    with pytest.raises(ValueError, match="does not have"):
        LogisticProbe(class_weight={7: 2.0}).fit(X, y)
    with pytest.raises(ValueError, match="positive"):
        LogisticProbe(class_weight={1: 0.0}).fit(X, y)
    with pytest.raises(ValueError):
        LogisticProbe(C=0.0)
    for call in ("decision_function", "predict", "predict_proba"):
        with pytest.raises(RuntimeError, match="fit first"):
            getattr(LogisticProbe(), call)(X)
    with pytest.raises(RuntimeError, match="fit first"):
        LogisticProbe().score(X, y)


def test_max_iter_warns():
    from lossyless_amd import LogisticProbe
    X, y = make_data(200, 16, 3)
    with pytest.warns(RuntimeWarning, match="stopped short"):
        p = LogisticProbe(tol=1e-12, max_iter=1).fit(X, y)
    assert p.converged_ is False
