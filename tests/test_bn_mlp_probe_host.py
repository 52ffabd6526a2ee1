"""CPU: the kernels of csrc/batchnorm.hip are declared, bound and exported; the CPU Philox4x32-10 and the keep pattern drawn
from it; ``BatchNormMLPProbe``'s float64 twin (hand-written forward, backward, running statistics and AdamW: the CPU path,
and the oracle of the GPU tests) against autograd and ``torch.optim.AdamW``; the layout of ``state_dict()``; the learning-rate
schedules against ``torch.optim.lr_scheduler``; reproducibility; refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from bn_mlp_probe_util import forward_with_masks, masks_of, reference_module
from conftest import GOLDEN, ROOT
from lossyless_amd import _lib
from probe_util import make_data

SYMBOLS = ("lla_bn_relu_dropout_fwd", "lla_bn_bwd")


def _close(got, want, what, rel=1e-12):
    err, ref = float((got - want).abs().max()), float(want.abs().max())
    assert err <= rel * ref, f"{what}: {err:.3e} against {ref:.3e}"


def test_symbols_are_declared_bound_and_exported():
    import lossyless_amd
    from lossyless_amd import MLPProbe
    with open(os.path.join(ROOT, "include", "lossyless_amd.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} not declared"
        assert name in _lib.EXPORTS and hasattr(raw, name), f"{name} not bound / exported"
    assert _lib.lib().lla_abi_version() == _lib.ABI_VERSION == 4          # additive: the ABI version stays
    assert "BatchNormMLPProbe" in lossyless_amd.__all__ and lossyless_amd.BatchNormMLPProbe is not None
    mk = open(os.path.join(ROOT, "lossyless_amd", "csrc", "Makefile")).read()
    assert "batchnorm.hip" in mk
    with pytest.raises(ValueError, match="norm_layer"):                   # MLPProbe stays the class-default network
        MLPProbe(norm_layer="batchnorm")
    with pytest.raises(ValueError, match="dropout"):
        MLPProbe(dropout_p=0.2)


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    from lossyless_amd import philox4x32_10
    got = philox4x32_10(np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert got.dtype == np.uint32 and " ".join(f"{int(w):08x}" for w in got) == want
    both = philox4x32_10(np.array([counter, (0, 0, 0, 0)], dtype=np.uint32), np.array(key, dtype=np.uint32))   # vectorised
    assert np.array_equal(both[0], got)


def test_keep_rate_and_pattern_definition():
    from lossyless_amd import dropout_keep, philox4x32_10
    keep = dropout_keep(seed=0x0123456789abcdef, step=3, layer=1, rows=1024, cols=1024, p=0.2)
    assert keep.dtype == torch.bool and tuple(keep.shape) == (1024, 1024)
    sigma = (0.16 / 2 ** 20) ** 0.5
    assert abs(float(keep.double().mean()) - 0.8) <= 4 * sigma
    # element (i, j) is word j % 4 of the block with counter ((i N + j) / 4, 0, step, layer) and key (seed_lo, seed_hi)
    i, j, N = 517, 642, 1024
    w = philox4x32_10(np.array([(i * N + j) // 4, 0, 3, 1]), np.array([0x89abcdef, 0x01234567]))[j % 4]
    assert bool(keep[i, j]) == (np.float32(int(w) >> 8) * np.float32(2.0 ** -24) >= np.float32(0.2))
    assert not torch.equal(keep, dropout_keep(0x0123456789abcdef, 4, 1, 1024, 1024, 0.2))
    assert not torch.equal(keep, dropout_keep(0x0123456789abcdef, 3, 0, 1024, 1024, 0.2))
    assert torch.equal(keep[:8], dropout_keep(0x0123456789abcdef, 3, 1, 8, 1024, 0.2))


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_twin_against_autograd(weight_decay, p):
    """Gradients of every parameter, the parameters after each of 5 AdamW steps and the running statistics against float64
    autograd + torch.optim.AdamW on the reference's layout with the twin's own masks: max |difference| <= 1e-12
    max |reference| per tensor."""
    from lossyless_amd.probe import _Adam, _TwinBNMLP, _mlp_init
    IN, HID, K, B, SEED = 8, 16, 3, 7, 0xfeedfacecafebeef
    g = torch.Generator().manual_seed(5)
    Ws, bs = _mlp_init([IN, HID, HID, K], g)
    twin = _TwinBNMLP(Ws, bs[-1] + 0.1 * torch.randn(K, generator=g), _Adam(1e-3, weight_decay, (0.9, 0.999), 1e-8), p, SEED, 0.1, 1e-5)
    for ga, be in zip(twin.gammas, twin.betas):                           # (gamma = 1, beta = 0 would hide a wrong dgamma / da)
        ga.add_(0.3 * torch.randn(HID, generator=g, dtype=torch.float64))
        be.add_(0.3 * torch.randn(HID, generator=g, dtype=torch.float64))
    net = reference_module(IN, HID, 2, K, p, torch.float64)
    lins = [m for m in net if isinstance(m, torch.nn.Linear)]
    bns = [m for m in net if isinstance(m, torch.nn.BatchNorm1d)]
    with torch.no_grad():
        for m, W in zip(lins, twin.Ws):
            m.weight.copy_(W)
        lins[-1].bias.copy_(twin.b)
        for m, ga, be in zip(bns, twin.gammas, twin.betas):
            m.weight.copy_(ga), m.bias.copy_(be)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=weight_decay, betas=(0.9, 0.999), eps=1e-8)
    params = lambda: [m.weight for m in lins] + [m.weight for m in bns] + [m.bias for m in bns] + [lins[-1].bias]   # noqa: E731
    for step in range(5):
        x = torch.randn(B, IN, generator=g, dtype=torch.float64)
        y = torch.randint(0, K, (B,), generator=g)
        loss, right, grads = twin.gradients(x, y)
        opt.zero_grad()
        logits = forward_with_masks(net, x, masks_of(SEED, step, 2, B, HID, p, torch.float64))
        want = torch.nn.functional.cross_entropy(logits, y)
        want.backward()
        assert abs(loss / B - float(want.detach())) <= 1e-12 * float(want.detach())
        assert right == int((logits.argmax(1) == y).sum())
        for i, (got, q) in enumerate(zip(grads, params())):
            assert float(q.grad.abs().max()) > 0
            _close(got, q.grad, f"step {step} gradient {i}")
        twin.step(x, y)
        opt.step()
        for i, (got, q) in enumerate(zip(twin._params(), params())):
            _close(got, q.detach(), f"step {step} parameter {i}")
        for l, m in enumerate(bns):
            _close(twin.rms[l], m.running_mean, f"step {step} running_mean {l}")
            _close(twin.rvs[l], m.running_var, f"step {step} running_var {l}")
            assert int(m.num_batches_tracked) == twin.t == step + 1


def test_state_dict_loads_into_the_reference_layout():
    from lossyless_amd import BatchNormMLPProbe
    X, y = make_data(120, 16, 3)
    probe = BatchNormMLPProbe(hid_dim=24, n_hid_layers=2, epochs=2, batch_size=32, seed=1, lr=1e-2).fit(X, 2 * y + 1)
    sd = probe.state_dict()
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    assert list(sd) == (["module.0.weight"] + [f"module.1.{k}" for k in bn] + ["module.4.weight"] + [f"module.5.{k}" for k in bn]
                        + ["module.8.weight", "module.8.bias"])

    class Wrapper(torch.nn.Module):                                       # the reference's MLP keeps the Sequential as .module
        def __init__(self):
            super().__init__()
            self.module = reference_module(16, 24, 2, 3)

    net = Wrapper()
    net.load_state_dict(sd, strict=True)
    net.eval()
    assert int(net.module[1].num_batches_tracked) == probe.n_steps_ == probe.num_batches_tracked_ == 2 * 4
    s = probe.decision_function(X)
    assert s.dtype == torch.float64 and tuple(s.shape) == (120, 3)
    with torch.no_grad():
        got = net.module(X)
    assert float((got.double() - s).abs().max()) <= 1e-4 * float(s.abs().max())      # (the module runs in fp32)
    net64 = Wrapper().double().eval()
    with torch.no_grad():
        lins = [m for m in net64.module if isinstance(m, torch.nn.Linear)]
        bns = [m for m in net64.module if isinstance(m, torch.nn.BatchNorm1d)]
        for m, W in zip(lins, probe.coefs_):
            m.weight.copy_(W)
        lins[-1].bias.copy_(probe.intercepts_[0])
        for m, ga, be, rm, rv in zip(bns, probe.bn_weights_, probe.bn_biases_, probe.running_means_, probe.running_vars_):
            m.weight.copy_(ga), m.bias.copy_(be), m.running_mean.copy_(rm), m.running_var.copy_(rv)
        assert float((net64.module(X.double()) - s).abs().max()) <= 1e-12 * float(s.abs().max())
    assert np.array_equal(probe.classes_, np.array([1, 3, 5]))
    assert set(probe.predict(X).tolist()) <= {1, 3, 5}
    proba = probe.predict_proba(X)
    assert tuple(proba.shape) == (120, 3) and float((proba.sum(1) - 1).abs().max()) < 1e-12
    assert probe.score(X, 2 * y + 1) == float((probe.predict(X) == 2 * y + 1).double().mean())
    assert len(probe.loss_curve_) == 2 and probe.loss_curve_[1] < probe.loss_curve_[0]
    assert len(probe.coefs_) == 3 and tuple(probe.coefs_[2].shape) == (3, 24) and len(probe.intercepts_) == 1
    assert all(tuple(t.shape) == (24,) for group in (probe.bn_weights_, probe.bn_biases_, probe.running_means_, probe.running_vars_)
               for t in group)


@pytest.mark.parametrize("epochs", [4, 10, 200])
def test_schedules_are_torchs(epochs):
    """``lr_curve_`` against MultiStepLR / ExponentialLR built by the formulas of lossyless/helpers.py:536-545 on a dummy
    optimiser, stepped once per epoch: 1e-15 relative."""
    from lossyless_amd import BatchNormMLPProbe
    X, y = make_data(16, 8, 2)
    decay_factor, k_steps = 100, 3

    def torch_curve(make):
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=3e-4)
        sched, out = make(opt), []
        for _ in range(epochs):
            out.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
        return out

    delta = epochs // (k_steps + 1)
    want = {"unifmultistep": torch_curve(lambda o: torch.optim.lr_scheduler.MultiStepLR(
                o, milestones=[delta * i for i in range(1, k_steps + 1)], gamma=(1 / decay_factor) ** (1 / k_steps))),
            "expdecay": torch_curve(lambda o: torch.optim.lr_scheduler.ExponentialLR(o, gamma=(1 / decay_factor) ** (1 / epochs))),
            None: [3e-4] * epochs}
    for name, curve in want.items():
        probe = BatchNormMLPProbe(hid_dim=8, n_hid_layers=1, epochs=epochs, batch_size=16, scheduler=name).fit(X, y)
        assert len(probe.lr_curve_) == epochs
        assert all(abs(a - b) <= 1e-15 * b for a, b in zip(probe.lr_curve_, curve)), name
    assert want["unifmultistep"][-1] < 1.01 * 3e-4 / decay_factor and want["unifmultistep"][0] == 3e-4


def _tensors(probe):
    from bn_mlp_probe_util import fitted_tensors
    return fitted_tensors(probe)


def test_seeds():
    from lossyless_amd import BatchNormMLPProbe, dropout_keep
    X, y = make_data(100, 16, 4)
    kw = dict(hid_dim=16, n_hid_layers=2, epochs=2, batch_size=32, dropout_p=0.5)
    a, b, c = (BatchNormMLPProbe(seed=s, **kw).fit(X, y) for s in (3, 3, 4))
    for Wa, Wb, Wc in zip(_tensors(a), _tensors(b), _tensors(c)):
        assert torch.equal(Wa, Wb) and not torch.equal(Wa, Wc)
    assert a.loss_curve_ == b.loss_curve_ and a.loss_curve_ != c.loss_curve_
    assert a.dropout_seed_ == b.dropout_seed_ != c.dropout_seed_ and 0 <= a.dropout_seed_ < 2 ** 64
    assert not torch.equal(dropout_keep(a.dropout_seed_, 0, 0, 32, 16, 0.5), dropout_keep(c.dropout_seed_, 0, 0, 32, 16, 0.5))
    # a float64 array is the float32 tensor's values; the decode group does not change the batches or the masks
    d = BatchNormMLPProbe(seed=3, **kw).fit(X.double().numpy(), y.numpy(), decode_group=32)
    assert all(torch.equal(p, q) for p, q in zip(_tensors(a), _tensors(d)))
    # dropout changes the fit, and p = 0 draws nothing
    e = BatchNormMLPProbe(seed=3, **dict(kw, dropout_p=0)).fit(X, y)
    assert torch.equal(e.coefs_[0], BatchNormMLPProbe(seed=3, **dict(kw, dropout_p=0)).fit(X, y).coefs_[0])
    assert not torch.equal(a.coefs_[0], e.coefs_[0])


def test_compressed_latents_on_the_cpu_equal_their_rows():
    import hubconf
    from lossyless_amd import BatchNormMLPProbe
    comp, _ = hubconf.clip_compressor_b005(device="cpu", clip_weights="synthetic")
    file = os.path.join(GOLDEN, "golden_5e-02.bin")
    ds = comp.open_dataset(file, device="cpu")
    rows = torch.from_numpy(np.ascontiguousarray(comp.decompress_dataset(file, is_info=False, is_cpu=True)))
    N = len(ds)
    assert N == 64 and tuple(rows.shape) == (64, 512)
    labels = (torch.arange(N) * 7) % 3
    kw = dict(hid_dim=16, n_hid_layers=2, epochs=2, batch_size=24, seed=2)     # 64 = 24 + 24 + 16: a ragged last batch
    a = BatchNormMLPProbe(**kw).fit(ds, labels, decode_group=48)               # ... and two decode groups per epoch
    b = BatchNormMLPProbe(**kw).fit(rows, labels)
    for p, q in zip(_tensors(a), _tensors(b)):
        assert p.dtype == torch.float64 and torch.equal(p, q) and bool(torch.isfinite(p).all())
    assert a.loss_curve_ == b.loss_curve_ and a.n_steps_ == b.n_steps_ == 6
    assert torch.equal(a.decision_function(ds), a.decision_function(rows))


def test_refusals():
    from lossyless_amd import BatchNormMLPProbe
    X, y = make_data(65, 16, 3)
    with pytest.raises(ValueError, match="MLPProbe"):
        BatchNormMLPProbe(norm_layer="identity")
    with pytest.raises(ValueError, match="activation"):
        BatchNormMLPProbe(activation="GELU")
    with pytest.raises(ValueError, match="dropout_p"):
        BatchNormMLPProbe(dropout_p=1.0)
    with pytest.raises(ValueError, match="scheduler"):
        BatchNormMLPProbe(scheduler="cosine")
    with pytest.raises(ValueError, match="hid_dim"):
        BatchNormMLPProbe(hid_dim=20)
    with pytest.raises(ValueError, match=r"N = 65.*batch_size = 32"):     # a last minibatch of one row
        BatchNormMLPProbe(hid_dim=16, batch_size=32).fit(X, y)
    assert BatchNormMLPProbe(hid_dim=16, norm_layer="batch", epochs=1, batch_size=32).fit(X[:64], y[:64]).n_steps_ == 2
    with pytest.raises(ValueError, match="in_dim"):
        BatchNormMLPProbe(hid_dim=16).fit(X[:, :12], y)
    with pytest.raises(TypeError, match="integers"):                      # regression targets
        BatchNormMLPProbe(hid_dim=16).fit(X, y.float())
    for call in ("decision_function", "predict", "predict_proba", "state_dict"):
        with pytest.raises(RuntimeError, match="fit first"):
            getattr(BatchNormMLPProbe(), call)(*(() if call == "state_dict" else (X,)))
