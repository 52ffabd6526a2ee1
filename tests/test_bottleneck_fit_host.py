"""CPU: BottleneckFit's float64 twin against torch autograd, the noise stream, the schedules, a small fit.  No device.

Gradient criterion: the twin writes its backward by hand in the kernel's order of operations, the reference is autograd over
compressai's formulation; both are float64, so they differ by rounding only.  An element is held to 1e-9 of its own size plus
1e-9 of the largest element of ITS OWN ROW (one of the 60 parameters, over the channels; dist and rate apart): a sum over
the rows of a batch can cancel to nothing in one channel while rounding does not.  The entries the distortion does not
depend on are compared apart: exact zeros in the twin, rounding noise under autograd."""
import math
import os
import re

import numpy as np
import pytest
import torch

import eb_reference as R
import lossyless_amd
from conftest import ROOT
from lossyless_amd import BottleneckFit, _lib, bottleneck_noise, lr_schedule, philox4x32_10
from lossyless_amd.bottleneck_fit import beta_schedule, twin_aux, twin_pass

SYMBOLS = ("lla_eb_train_pass", "lla_eb_train_pass_workspace_bytes", "lla_eb_aux_grad")
CASES = [("plain", 1, 4), ("plain", 3, 4), ("plain", 33, 4), ("plain", 1, 68), ("plain", 3, 68), ("plain", 33, 68),
         ("bound", 33, 68), ("signs", 33, 68), ("matrix30", 33, 68), ("factor5", 33, 68)]


def test_symbols_sources_and_exports():
    raw = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(raw, name), f"{name} not bound / exported"
    with open(os.path.join(ROOT, "lossyless_amd", "csrc", "Makefile")) as f:
        assert "eb_train.hip" in re.search(r"^SHARED\s*=\s*(.*)$", f.read(), re.M).group(1).split()
    for name in ("BottleneckFit", "bottleneck_noise"):
        assert name in lossyless_amd.__all__ and getattr(lossyless_amd, name) is not None


@pytest.mark.parametrize("name,B,C", CASES)
def test_twin_gradients_equal_autograd(name, B, C):
    z, main, q, target = R.stress_case(name, B, C)
    u = bottleneck_noise(5, 3, B, C)
    got, dist, rate = twin_pass(z, main, u)
    ref, rdist, rrate = R.reference_pass(z, main, u)
    if name == "bound":      # the case is what it says: most likelihoods sit on the bound
        assert float(rrate) > 0.9 * B * C * -math.log(1e-9)
    if name == "signs":
        lower = R.logits(main[2:], ((z.double() + main[1]) * torch.exp(main[0]) + u.double()).t()[:, None, :] - 0.5)
        assert bool((lower < -1).any()) and bool((lower > 1).any())
    # the distortion depends on scaling alone: the twin's closed form gives exact zeros elsewhere, autograd gives 0 for the
    # network and rounding noise of (1 / e^s) e^s - 1 per row for biasing
    assert not bool(got[0, 1:].any()) and not bool(ref[0, 2:].any()) and float(ref[0, 1].abs().max()) <= 4 * B * 2.0 ** -53
    for name_q, g, r in (("dist", got[0, :1], ref[0, :1]), ("rate", got[1], ref[1])):
        rows = r.abs().amax(1, keepdim=True)                 # one of the 60 parameter rows over its C channels
        bad = (g - r).abs() > 1e-9 * r.abs() + 1e-9 * rows
        assert not bool(bad.any()), f"{name_q}: rows {sorted(set(bad.nonzero()[:, 0].tolist()))}"
    assert abs(float(dist - rdist)) <= 1e-9 * abs(float(rdist)) and abs(float(rate - rrate)) <= 1e-9 * abs(float(rrate))
    gq, aux = twin_aux(main[2:], q, target)
    rq, raux = R.reference_aux(main[2:], q, target)
    torch.testing.assert_close(gq, rq, rtol=1e-9, atol=1e-9 * float(rq.abs().max()))
    assert abs(float(aux - raux)) <= 1e-9 * float(raux)


def test_noise_is_the_documented_philox_stream():
    seed, step, rows, cols = 0x0123456789ABCDEF, 7, 5, 12
    u = bottleneck_noise(seed, step, rows, cols)
    assert u.dtype == torch.float32 and tuple(u.shape) == (rows, cols)
    for i, c in ((0, 0), (0, 3), (2, 5), (4, 11)):
        e = (i * cols + c) // 4
        w = philox4x32_10(np.array([e & 0xFFFFFFFF, e >> 32, step, 0x6E6F6973]), np.array([0x89ABCDEF, 0x01234567]))[c % 4]
        assert float(u[i, c]) == float(np.float32(int(w) >> 8) * np.float32(2.0 ** -24) - np.float32(0.5))
    assert not torch.equal(u, bottleneck_noise(seed, step + 1, rows, cols))
    assert not torch.equal(u, bottleneck_noise(seed + 1, step, rows, cols))
    with pytest.raises(ValueError):
        bottleneck_noise(0, 0, 4, 6)
    n = 1 << 16
    big = bottleneck_noise(3, 1, 256, 256).double()
    assert float(big.min()) >= -0.5 and float(big.max()) < 0.5
    # uniform on [-1/2, 1/2): mean 0, variance 1/12, fourth central moment 1/80 -> standard errors of the two estimates
    assert abs(float(big.mean())) < 5 * math.sqrt(1 / 12 / n)
    assert abs(float((big ** 2).mean()) - 1 / 12) < 5 * math.sqrt((1 / 80 - 1 / 144) / n)


def _gaussian_features(N, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, C, generator=g) * torch.linspace(0.05, 2, C) + torch.linspace(-1, 1, C)


def test_twin_fit_learns_and_saves_the_shipped_key_set():
    C, N = 8, 512
    fit = BottleneckFit(0.05, epochs=3, batch_size=64, scheduler=None, seed=1).fit(_gaussian_features(N, C))
    assert fit.engine_ == "twin"
    assert fit.loss_curve_[-1] < fit.loss_curve_[0]
    assert fit.aux_curve_[2] < fit.aux_curve_[1] < fit.aux_curve_[0]
    assert len(fit.rate_curve_) == len(fit.distortion_curve_) == 3 and all(r > 0 for r in fit.rate_curve_)
    eb = fit.rate_estimator_.entropy_bottleneck
    assert fit.rate_estimator_.is_coder_updated
    for c in range(C):
        row = eb._quantized_cdf[c, :int(eb._cdf_length[c])]
        assert bool((row[1:] > row[:-1]).all()), f"CDF row {c} is not strictly increasing"
    sd = fit.state_dict()
    shipped = torch.load(os.path.join(ROOT, "lossyless_amd", "assets", "beta5e-02_factorized_rate.pt"), map_location="cpu",
                         weights_only=True)
    assert set(sd) == set(shipped)
    for k, v in shipped.items():
        if k.endswith("_quantized_cdf"):
            assert sd[k].shape[0] == C and sd[k].dtype == v.dtype
        else:
            assert tuple(sd[k].shape) == tuple(C if d == 512 else d for d in v.shape) and sd[k].dtype == v.dtype, k
    # the same seed gives the same fit
    again = BottleneckFit(0.05, epochs=3, batch_size=64, scheduler=None, seed=1).fit(_gaussian_features(N, C))
    assert all(torch.equal(sd[k], v) for k, v in again.state_dict().items())


def test_schedules_equal_the_reference_formulas():
    N, bs, epochs, beta = 100, 16, 8, 0.1
    fit = BottleneckFit(beta, epochs=epochs, batch_size=bs, lr=1e-3, lr_coder=3e-4, seed=0).fit(_gaussian_features(N, 4))
    steps_per_epoch = math.ceil(N / bs)                       # the last short batch is kept
    total = epochs * steps_per_epoch

    def annealer(t):                                          # lossyless/helpers.py Annealer, mode "linear", start_step 0
        initial, final, n = beta * 1e-5, beta, math.ceil(1 / 10 * total)
        return initial + (final - initial) / n * t if t < n else final

    assert beta_schedule(beta, total, "linear") == [annealer(t) for t in range(total)]
    assert fit.beta_curve_ == [annealer((e + 1) * steps_per_epoch - 1) for e in range(epochs)]
    assert beta_schedule(beta, total, "constant") == [beta] * total
    assert fit.lr_curve_ == lr_schedule("unifmultistep", 1e-3, epochs, decay_factor=1000)
    gamma = (1 / 1000) ** (1 / 3)                             # MultiStepLR, milestones 2, 4, 6
    want = [1e-3 * gamma ** sum(e >= m for m in (2, 4, 6)) for e in range(epochs)]
    assert np.allclose(fit.lr_curve_, want, rtol=1e-12)


def test_refusals():
    with pytest.raises(ValueError):
        BottleneckFit(0.05, filters=(3, 3))
    with pytest.raises(ValueError):
        BottleneckFit(0.05, beta_anneal="geometric")
    with pytest.raises(ValueError):
        BottleneckFit(0.05, scheduler="cosine")
    with pytest.raises(ValueError):
        BottleneckFit(0.05).fit(torch.zeros(0, 8))
