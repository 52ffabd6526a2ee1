"""CPU: ``lla_svm_pass`` is declared, bound and refuses bad arguments before any device call; ``LinearProbe`` on the CPU
(the float64 evaluation that the GPU tests use as their oracle) solves scikit-learn's LinearSVC objective."""
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
from probe_util import grad_norms, make_data, probe_signs

CW, TOL = 7e-3, 1e-4


def test_symbols_are_declared_bound_and_exported():
    import lossyless_amd
    with open(os.path.join(ROOT, "include", "lossyless_amd.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lla_svm_pass", "lla_svm_pass_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} not declared"
        assert name in _lib.EXPORTS and hasattr(raw, name), f"{name} not bound / exported"
    assert _lib.lib().lla_abi_version() == _lib.ABI_VERSION == 4          # additive: the ABI version stays
    assert "LinearProbe" in lossyless_amd.__all__ and lossyless_amd.LinearProbe is not None
    mk = open(os.path.join(ROOT, "lossyless_amd", "csrc", "Makefile")).read()
    assert "probe.hip" in re.search(r"^SHARED\s*=\s*(.*)$", mk, re.M).group(1).split()


def _call(C=40, K=3, B=16, ld_z=None, ld_w=None, null=(), z_dtype=None, V=False):
    """lla_svm_pass on host buffers it must never read: every call here is refused by the argument checks."""
    L = _lib.lib()
    buf = np.zeros(1 << 16, dtype=np.float64)          # 16-byte aligned stand-in for every pointer
    p = ctypes.c_void_p(buf.ctypes.data + (-buf.ctypes.data) % 16)
    a = dict(z=p, y=p, W=p, b=p, V=p if V else None, vb=p if V else None, out_W=p, out_b=p, out_loss=p, ws=p)
    for k in null:
        a[k] = None
    return L.lla_svm_pass(a["z"], _lib.LLA_Z_F32 if z_dtype is None else z_dtype, C if ld_z is None else ld_z, a["y"], B, C,
                          a["W"], a["b"], a["V"], a["vb"], K, C if ld_w is None else ld_w, a["out_W"], a["out_b"],
                          a["out_loss"], 0, a["ws"], None)


def test_bad_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    assert _call(C=12) == _lib.LLA_EINVAL                  # not a multiple of 8
    assert _call(C=1032) == _lib.LLA_EINVAL                # wider than 1024
    assert _call(C=0) == _lib.LLA_EINVAL
    assert _call(K=0) == _lib.LLA_EINVAL
    assert _call(ld_z=32) == _lib.LLA_EINVAL               # ld_z < C
    assert _call(ld_z=42) == _lib.LLA_EINVAL               # pitch not a multiple of 4
    assert _call(ld_w=32) == _lib.LLA_EINVAL
    assert _call(B=-1) == _lib.LLA_EINVAL
    assert _call(z_dtype=7) == _lib.LLA_EINVAL
    for name in ("z", "y", "W", "b", "out_W", "out_b", "out_loss", "ws"):
        assert _call(null=(name,)) == _lib.LLA_EINVAL, name
    assert _call(V=True, null=("vb",)) == _lib.LLA_EINVAL
    assert L.lla_svm_pass_workspace_bytes(12, 3) == 0 and L.lla_svm_pass_workspace_bytes(40, 0) == 0
    # [class tiles][workgroups][32 classes][C + 2] floats, at most 512 workgroups
    assert L.lla_svm_pass_workspace_bytes(512, 10) == 512 * 32 * 514 * 4
    assert L.lla_svm_pass_workspace_bytes(512, 1000) == 32 * 16 * 32 * 514 * 4


@pytest.mark.parametrize("N,C,K", [(600, 40, 3), (400, 40, 2), (900, 64, 37)])
def test_cpu_solver_against_scikit_learn(N, C, K):
    svm = pytest.importorskip("sklearn.svm")
    from lossyless_amd import LinearProbe
    X, y = make_data(N, C, K)
    labels = 2 * y + 1                                     # (labels are not class indexes)
    probe = LinearProbe(C=CW, tol=TOL).fit(X, labels)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = svm.LinearSVC(C=CW, dual=False, tol=1e-12, max_iter=100000).fit(X.double().numpy(), labels.numpy())
    assert np.array_equal(probe.classes_, clf.classes_)
    assert tuple(probe.coef_.shape) == clf.coef_.shape and tuple(probe.intercept_.shape) == clf.intercept_.shape
    assert probe.coef_.dtype == torch.float32 and probe.converged_ and probe.n_passes_ > 0
    Y = probe_signs(probe, labels)
    zero = torch.zeros_like(probe.coef_)
    g0, _ = grad_norms(zero, zero[:, 0], X, Y, CW)
    ginf, g2 = grad_norms(probe.coef_, probe.intercept_, X, Y, CW)
    Wsk, bsk = torch.from_numpy(clf.coef_), torch.from_numpy(clf.intercept_)
    _, g2_sk = grad_norms(Wsk, bsk, X, Y, CW)
    dist = float(torch.cat([probe.coef_.double() - Wsk, (probe.intercept_.double() - bsk)[:, None]], 1).norm())
    print(f"N {N} C {C} K {K}: passes {probe.n_passes_}, |g|inf {ginf:.3e} (tol |g0|inf {TOL * g0:.3e}), "
          f"|W - W_sk| {dist:.3e} (|g| {g2:.3e} + |g_sk| {g2_sk:.3e})")
    assert ginf <= TOL * g0
    assert dist <= g2 + g2_sk                              # f is 1-strongly convex: |W - W*| <= |grad f(W)|
    assert np.array_equal(probe.predict(X).numpy(), clf.predict(X.double().numpy()))
    assert probe.score(X, labels) == float((probe.predict(X) == labels).double().mean())


def test_compressed_latents_on_the_cpu(tmp_path):
    import hubconf
    from lossyless_amd import LinearProbe
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
            return LinearProbe(max_iter=2).fit(data, labels, **kw)
    for rows_per_pass in (128, 65536):
        a = fit(ds, rows_per_pass=rows_per_pass)
        b = fit(rows, rows_per_pass=rows_per_pass)
        assert torch.equal(a.coef_, b.coef_) and torch.equal(a.intercept_, b.intercept_) and a.n_passes_ == b.n_passes_
        assert a.objective_ == b.objective_ and bool(a.coef_.abs().max() > 0)
        kept = fit(ds, rows_per_pass=rows_per_pass, keep_rows=True)
        assert torch.equal(kept.coef_, a.coef_)
    assert torch.equal(a.decision_function(ds), a.decision_function(rows)) and tuple(a.decision_function(ds).shape) == (N, 3)
    assert a.score(ds, labels) == float((a.predict(ds) == labels).double().mean())
    # the object's own labels (arange(N): one class per row) are used when none are given
    with_labels = comp.open_dataset(file, label_file=lf, device="cpu")
    own = LinearProbe(max_iter=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        own.fit(with_labels, rows_per_pass=128)
    assert np.array_equal(own.classes_, np.arange(N)) and tuple(own.coef_.shape) == (N, 512)


def test_fit_refuses_what_it_cannot_fit(tmp_path):
    import hubconf
    from lossyless_amd import LinearProbe
    X, y = make_data(60, 16, 3)
    with pytest.raises(ValueError, match="labels"):
        LinearProbe().fit(X)
    comp, _ = hubconf.clip_compressor_b005(device="cpu", clip_weights="synthetic")
    file, _, _ = write_dataset(tmp_path, "5e-02", 8, seed=3)
    with pytest.raises(ValueError, match="labels"):
        LinearProbe().fit(comp.open_dataset(file, device="cpu"))
    with pytest.raises(ValueError, match="two classes"):
        LinearProbe().fit(X, torch.zeros(60, dtype=torch.int64))
    for bad in (float("nan"), float("inf")):
        Xb = X.clone()
        Xb[41, 3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            LinearProbe().fit(Xb, y, rows_per_pass=32)
    with pytest.raises(ValueError, match="labels for"):
        LinearProbe().fit(X, y[:-1])


def test_max_iter_warns():
    from lossyless_amd import LinearProbe
    X, y = make_data(200, 16, 3)
    with pytest.warns(RuntimeWarning, match="stopped short"):
        p = LinearProbe(tol=1e-12, max_iter=1).fit(X, y)
    assert p.converged_ is False
