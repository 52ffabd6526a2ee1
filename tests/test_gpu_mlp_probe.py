"""GPU: ``MLPProbe`` trained in the kernels of csrc/mlp.hip from containers that stay compressed on the device -- bit
reproducibility, the device against the float64 twin over a short horizon (held to a multiple of what fp32 arithmetic on the
CPU does to the same steps), a problem a linear probe cannot learn, and ``HyperpriorLatents``."""
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from conftest import load_tables
from mlp_probe_util import SHORT, XOR, largest_difference, replay, short_data, xor_data
from oracle import cbind, container

pytestmark = pytest.mark.gpu

# max |parameter difference| between the 6 steps of SHORT in torch-CPU float32 (nn.Sequential + autograd + AdamW) and in the
# float64 twin, as mlp_probe_util.replay computes it: 1.4523e-07 on the x86-64 host this was written on (torch 2.x CPU, any
# thread count); rounded up.  The test recomputes it and asserts that this constant is not below it.
D32 = 1.5e-7
# the same yardstick for the XOR problem's held-out probabilities after its 192 steps: 2.1354e-06 there; rounded up
D32_XOR_PROBA = 2.2e-6
FACTOR = 4      # the MFMA chain and the CPU's blocked sums order the same fp32 additions differently


def _params(probe):
    return probe.coefs_ + probe.intercepts_


def _same(a, b):
    return all(p.dtype == q.dtype and torch.equal(p, q) for p, q in zip(_params(a), _params(b))) and a.loss_curve_ == b.loss_curve_


def _class_symbols(tab, n, n_classes, seed):
    """Symbols inside every channel's coding window (rows of ordinary size) whose mean depends on row % n_classes."""
    rng = np.random.default_rng(seed)
    C = tab["cdf"].shape[0]
    width = (tab["cdf_len"].astype(np.int64) - 2)[None, :]
    means = rng.normal(size=(n_classes, C)) * 1.5
    v = np.rint(width / 2 + means[np.arange(n) % n_classes] + rng.normal(size=(n, C)) * 1.5)
    return (tab["offset"][None, :] + np.clip(v, 0, width - 1)).astype(np.int32)


def test_bit_reproducibility_from_compressed_latents(tmp_path):
    import hubconf
    from lossyless_amd import MLPProbe
    N = 300                                  # batch 64: four full batches and one of 44; decode groups of 128: three of them
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    tab = load_tables("5e-02")
    sym = _class_symbols(tab, N, 3, seed=5)
    file = tmp_path / "z.bin"
    container.write_container(str(file), [cbind.rans_encode(s, tab["cdf"], tab["cdf_len"], tab["offset"]) for s in sym])
    ds = comp.open_dataset(file)
    assert ds.device.type == "cuda" and len(ds) == N
    labels = torch.arange(N) % 3
    kw = dict(hid_dim=32, n_hid_layers=2, epochs=2, batch_size=64, seed=4)
    a = MLPProbe(**kw).fit(ds, labels, decode_group=128)
    b = MLPProbe(**kw).fit(ds, labels, decode_group=128)
    assert a.coefs_[0].is_cuda and a.coefs_[0].dtype == torch.float32 and tuple(a.coefs_[-1].shape) == (3, 32)
    assert all(bool(torch.isfinite(p).all()) for p in _params(a)) and a.n_steps_ == 10
    assert _same(a, b)
    assert _same(a, MLPProbe(**kw).fit(ds, labels))                       # one decode group
    rows = ds.all()
    assert rows.is_cuda
    assert _same(a, MLPProbe(**kw).fit(rows, labels))                     # a CUDA tensor, indexed by the same permutation
    assert _same(a, MLPProbe(**kw).fit(rows, labels, decode_group=128))
    assert not _same(a, MLPProbe(**dict(kw, seed=5)).fit(ds, labels))
    assert a.loss_curve_[1] < a.loss_curve_[0]
    s = a.decision_function(ds, rows_per_pass=128)
    assert tuple(s.shape) == (N, 3) and torch.equal(s, a.decision_function(rows))
    assert a.score(ds, labels) == float((a.predict(rows).cpu() == labels).double().mean())


def test_device_against_twin_over_a_short_horizon():
    """Figures measured on the MI355X are printed; the bar is FACTOR x D32."""
    from lossyless_amd import MLPProbe
    X, y = short_data()
    twin, closest = replay(SHORT, X, y, torch.float64)
    assert closest >= 1e-5, f"a hidden pre-activation of the twin comes within {closest:.3e} of zero: choose another data seed"
    cpu32, _ = replay(SHORT, X, y, torch.float32)
    d32 = largest_difference(cpu32, twin)
    assert D32 >= d32, f"the fp32 yardstick recomputed here is {d32:.4e}, above the constant {D32:.4e}"
    fitted = MLPProbe(**SHORT).fit(X, y)                                    # the CPU path IS the twin
    assert largest_difference(_params(fitted), twin) == 0.0
    dev = MLPProbe(**SHORT).fit(X.cuda(), y)
    assert dev.n_steps_ == 6 and dev.coefs_[0].is_cuda
    got = largest_difference(_params(dev), twin)
    print(f"device against twin {got:.4e}; torch-CPU fp32 against twin {d32:.4e} (constant {D32:.4e}); bar {FACTOR * D32:.4e}")
    assert got <= FACTOR * D32
    assert abs(dev.loss_curve_[-1] - fitted.loss_curve_[-1]) <= 1e-5 * fitted.loss_curve_[-1]
    assert dev.accuracy_curve_ == fitted.accuracy_curve_


def test_it_learns_what_a_linear_probe_cannot():
    """The XOR of two signs.  The float64 twin alone reaches held-out accuracy 1.0 with every margin >= 0.5 (asserted of the
    twin); the device fit must then score 1.0.  Its probabilities are held to the bar of the short-horizon test computed for
    THIS problem: FACTOR x what torch-CPU fp32 training does to the held-out probabilities (D32_XOR_PROBA)."""
    import warnings
    from lossyless_amd import LogisticProbe, MLPProbe
    Xtr, ytr = xor_data(2048, 1)
    Xte, yte = xor_data(512, 2)
    twin = MLPProbe(**XOR).fit(Xtr, ytr)
    s = twin.decision_function(Xte)
    margin = torch.where(yte == 1, s[:, 1] - s[:, 0], s[:, 0] - s[:, 1])
    assert twin.score(Xte, yte) == 1.0 and float(margin.min()) >= 0.5, f"the twin's smallest margin is {float(margin.min()):.3f}"
    dev = MLPProbe(**XOR).fit(Xtr.cuda(), ytr)
    assert dev.score(Xte.cuda(), yte) == 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        linear = LogisticProbe().fit(Xtr.cuda(), ytr)
    assert linear.score(Xte.cuda(), yte) < 0.75
    proba = dev.predict_proba(Xte.cuda())
    assert tuple(proba.shape) == (512, 2) and float((proba.double().sum(1) - 1).abs().max()) <= 1e-6
    cpu32, _ = replay(XOR, Xtr, ytr, torch.float32)
    shadow = MLPProbe(**XOR)
    n = len(cpu32) // 2
    shadow.coefs_, shadow.intercepts_, shadow.classes_ = [p.double() for p in cpu32[:n]], [p.double() for p in cpu32[n:]], twin.classes_
    want = twin.predict_proba(Xte)
    d32 = float((shadow.predict_proba(Xte) - want).abs().max())
    assert D32_XOR_PROBA >= d32, f"the fp32 yardstick recomputed here is {d32:.4e}, above the constant {D32_XOR_PROBA:.4e}"
    got = float((proba.double().cpu() - want).abs().max())
    print(f"device against twin, probabilities {got:.4e}; torch-CPU fp32 against twin {d32:.4e}; bar {FACTOR * D32_XOR_PROBA:.4e}")
    assert got <= FACTOR * D32_XOR_PROBA


def test_fit_from_hyperprior_latents():
    from hyperprior_latents_util import hyper_model
    from lossyless_amd import HyperpriorLatents, MLPProbe
    model = hyper_model()
    N = 96
    g = torch.Generator().manual_seed(3)
    labels = torch.arange(N) % 3
    z = (torch.randn(3, 512, generator=g)[labels] * 0.5 + torch.randn(N, 512, generator=g) * 0.7).cuda()
    z_strings, side_strings = model.compress(z)
    with tempfile.TemporaryDirectory() as d:
        file = os.path.join(d, "z.bin")
        container.write_container(file, [s for pair in zip(z_strings, side_strings) for s in pair])
        ds = HyperpriorLatents(file, types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()),
                                                           hyperprior=model))
    kw = dict(hid_dim=32, n_hid_layers=1, epochs=2, batch_size=40, seed=1)   # 96 = 40 + 40 + 16
    a = MLPProbe(**kw).fit(ds, labels, decode_group=80)
    b = MLPProbe(**kw).fit(ds, labels, decode_group=80)
    assert _same(a, b) and _same(a, MLPProbe(**kw).fit(ds.all(), labels))
    assert all(bool(torch.isfinite(p).all()) for p in _params(a)) and a.n_steps_ == 6
    assert a.loss_curve_[1] < a.loss_curve_[0]
    assert tuple(a.decision_function(ds).shape) == (N, 3)
