"""CPU: HyperpriorFit's float64 twin against torch autograd, the noise stream, a small fit.  No device.

Gradient criterion, that of test_bottleneck_fit_host.py: the twin writes its backward by hand in the kernels' order, the
reference (hyperprior_reference.py) is autograd over compressai's formulation; both are float64 and differ by rounding only.
An element is held to 1e-9 of its own size plus 1e-9 of the largest element of its group."""
import math
import os
import re

import numpy as np
import pytest
import torch

import hyperprior_reference as H
import lossyless_amd
from conftest import ROOT
from lossyless_amd import HyperpriorFit, _lib, bottleneck_noise, hyperprior_noise, philox4x32_10
from lossyless_amd.bottleneck_fit import twin_aux
from lossyless_amd.hyperprior_fit import (SIDE_TAG, twin_affine_grad, twin_gaussian_pass, twin_side_pass, twin_step_gradients)
from lossyless_amd.rates import HRateHyperprior, synthetic_hyperprior_state_dict

SYMBOLS = ("lla_eb_side_pass", "lla_eb_side_pass_workspace_bytes", "lla_eb_aux_grad_any", "lla_gaussian_train_pass",
           "lla_gaussian_train_pass_workspace_bytes", "lla_affine_grad", "lla_affine_grad_workspace_bytes")


def test_symbols_sources_and_exports():
    raw = _lib.lib()
    with open(os.path.join(ROOT, "include", "lossyless_amd.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(raw, name), f"{name} not bound / exported"
        assert re.search(rf"\b{name}\(", header), f"{name} is not declared in the header"
    with open(os.path.join(ROOT, "lossyless_amd", "csrc", "Makefile")) as f:
        assert "hyperprior_train.hip" in re.search(r"^SHARED\s*=\s*(.*)$", f.read(), re.M).group(1).split()
    for name in ("HyperpriorFit", "hyperprior_noise"):
        assert name in lossyless_amd.__all__ and getattr(lossyless_amd, name) is not None


def test_noise_generalises_the_bottleneck_stream():
    for rows, cols in ((5, 12), (33, 68), (1, 4096)):
        assert torch.equal(hyperprior_noise(0x0123456789ABCDEF, 7, rows, cols), bottleneck_noise(0x0123456789ABCDEF, 7, rows, cols))
    seed, step = 0x0123456789ABCDEF, 7
    for rows, cols in ((5, 10), (3, 102)):
        for tag in (0x6E6F6973, SIDE_TAG):
            u = hyperprior_noise(seed, step, rows, cols, tag)
            assert u.dtype == torch.float32 and tuple(u.shape) == (rows, cols)
            for i, c in ((0, 0), (0, cols - 1), (1, 0), (rows - 1, cols - 1), (2, 5)):
                f = i * cols + c
                w = philox4x32_10(np.array([f // 4 & 0xFFFFFFFF, f // 4 >> 32, step, tag]), np.array([0x89ABCDEF, 0x01234567]))[f % 4]
                assert float(u[i, c]) == float(np.float32(int(w) >> 8) * np.float32(2.0 ** -24) - np.float32(0.5))
        assert not torch.equal(hyperprior_noise(seed, step, rows, cols), hyperprior_noise(seed, step, rows, cols, SIDE_TAG))
    big = hyperprior_noise(3, 1, 642, 102, SIDE_TAG).double()
    assert float(big.min()) >= -0.5 and float(big.max()) < 0.5
    assert abs(float(big.mean())) < 5 * math.sqrt(1 / 12 / big.numel())


@pytest.mark.parametrize("B,S", [(1, 10), (33, 10), (3, 102), (33, 130)])
def test_twin_side_pass_equals_autograd(B, S):
    x, net, q, target = H.side_case(B, S)
    u = hyperprior_noise(5, 3, B, S, SIDE_TAG)
    s_hat, dx, grads, rate = twin_side_pass(x, net, u)
    ref = H.reference_side(x, net, u)
    assert torch.equal(s_hat, ref["s_hat"]) and H.close(dx, ref["dx"])
    for k, sl in (("matrix", slice(0, 33)), ("bias", slice(33, 46)), ("factor", slice(46, 58))):
        rows = ref["grads"][sl].abs().amax(1, keepdim=True)
        assert bool(((grads[sl] - ref["grads"][sl]).abs() <= 1e-9 * ref["grads"][sl].abs() + 1e-9 * rows).all()), k
    assert abs(float(rate - ref["rate"])) <= 1e-9 * abs(float(ref["rate"]))
    # `scale` multiplies the gradients and nothing else
    s2, dx2, g2, r2 = twin_side_pass(x, net, u, 0.25)
    assert torch.equal(dx2, 0.25 * dx) and torch.equal(g2, 0.25 * grads) and torch.equal(s2, s_hat) and r2 == rate
    gq, aux = twin_aux(net, q, target)                # the aux of the side bottleneck: any S
    rq, raux = H.R.reference_aux(net, q, target)
    torch.testing.assert_close(gq, rq, rtol=1e-9, atol=1e-9 * float(rq.abs().max()))
    assert abs(float(aux - raux)) <= 1e-9 * float(raux)


@pytest.mark.parametrize("name,B,C", [("plain", 1, 4), ("plain", 33, 68), ("plain", 3, 10)] + [(n, 33, 68) for n in H.GAUSS_CASES[1:]])
def test_twin_gaussian_pass_equals_autograd(name, B, C):
    u = hyperprior_noise(5, 3, B, C)
    z, scaling, biasing, gp = H.gaussian_case(name, B, C, u)
    y, dgp, dy, g_dist, dist, rate = twin_gaussian_pass(z, scaling, biasing, gp, u, H.BOUND)
    ref = H.reference_gaussian(z, scaling, biasing, gp, u)
    sraw, g_sc = gp[:, :C], ref["dgp"][:, :C]
    if name == "lowscale":      # below the bound a gradient passes only where it is negative: both kinds are in the case
        assert bool((sraw < H.BOUND).all()) and bool((g_sc < 0).any()) and bool((g_sc == 0).sum() > B * C // 4)
        assert bool((dgp[:, :C] <= 0).all())
    if name == "negative":
        assert bool((sraw < 0).all()) and bool((g_sc < 0).any())
    if name == "likbound":
        assert float(ref["rate"]) > 0.9 * B * C * -math.log(1e-9)
    if name == "tie":
        v = (z.double() + biasing) * torch.exp(scaling) + u.double()
        tied = v == gp[:, C:].double()
        assert int(tied.sum()) == ((B + 1) // 2) * C
        assert not bool(dy[tied].any()) and not bool(dgp[:, C:][tied].any()) and bool(dgp[:, :C][tied].any())
    assert torch.equal(y, ref["y"])
    for k, got, want in (("scales", dgp[:, :C], ref["dgp"][:, :C]), ("means", dgp[:, C:], ref["dgp"][:, C:]), ("dy", dy, ref["dy"]),
                         ("g_dist", g_dist, ref["g_dist"])):
        assert H.close(got, want), k
    assert abs(float(dist - ref["dist"])) <= 1e-9 * float(ref["dist"]) and abs(float(rate - ref["rate"])) <= 1e-9 * abs(float(ref["rate"]))
    # the affine's gradient: d rate / d (scaling, biasing) through y, by autograd on the whole expression
    s = scaling.clone().requires_grad_(True)
    b = biasing.clone().requires_grad_(True)
    full = H.gaussian_rate((z.double() + b) * torch.exp(s), gp.double(), u)
    rs, rb = torch.autograd.grad(full, (s, b))
    gs, gb = twin_affine_grad(dy, y, scaling)
    assert H.close(gs, rs) and H.close(gb, rb)


@pytest.mark.parametrize("B,C,S", [(33, 16, None), (8, 20, 7)])
def test_twin_step_equals_autograd(B, C, S):
    P, q, target = H.initial_parameters(C, seed=2, side_z_dim=S)
    Sd = P["net"].shape[1]
    g = torch.Generator().manual_seed(4)
    z = torch.randn(B, C, generator=g) * torch.exp(0.7 * torch.randn(B, 1, generator=g))
    u_s, u_z = hyperprior_noise(9, 2, B, Sd, SIDE_TAG), hyperprior_noise(9, 2, B, C)
    G, sums = twin_step_gradients(P, z, u_s, u_z, H.BOUND, 0.03)
    Rg, rsums = H.reference_step(P, z, u_s, u_z, 0.03)
    got, want = H.flat_groups(G), H.flat_groups(Rg)
    assert set(got) == set(want) == {"scaling", "biasing", "net", "side_W", "side_b", "z_W", "z_b"}
    for k in want:
        assert float(want[k].abs().max()) > 0 and H.close(got[k], want[k]), k
    for a, b in zip(sums, rsums):
        assert abs(float(a - b)) <= 1e-9 * abs(float(b))


def _rows(N, C, seed=0):
    """Rows whose scale varies from row to row: z_i = a_i g_i, a_i log-normal."""
    g = torch.Generator().manual_seed(seed)
    return torch.exp(0.7 * torch.randn(N, 1, generator=g)) * torch.randn(N, C, generator=g)


def test_twin_fit_lowers_the_held_out_rate_and_saves_the_key_set():
    C, N = 16, 512
    Z = _rows(N + 256, C)
    kw = dict(epochs=3, batch_size=64, scheduler=None, seed=1)
    fit = HyperpriorFit(0.05, **kw).fit(Z[:N])
    assert fit.engine_ == "twin" and fit.rate_estimator_.side_z_dim == 10 and fit.rate_estimator_.side_encoder.module[0].out_features == 256
    fresh = HyperpriorFit(0.05, **kw).initial_estimator(C).eval()
    fresh.update(force=True)
    bits = []
    for m in (fresh, fit.rate_estimator_):
        assert not m.training and m.is_coder_updated
        m.make_pickable_()                   # (no coder: forward_help skips the real rate, which needs the device)
        with torch.no_grad():
            bits.append(float(m.forward_help(Z[N:], None)[2]["H_q_Z"]))
        m.undo_pickable_()
    print(f"held-out H_q_Z: untrained {bits[0]:.1f} bits, trained {bits[1]:.1f} bits; rate curve {fit.rate_curve_}")
    assert bits[1] < bits[0]
    for name in ("rate", "side_rate", "distortion", "loss", "aux", "beta"):
        assert len(getattr(fit, f"{name}_curve_")) == 3
    assert fit.aux_curve_[2] < fit.aux_curve_[1] < fit.aux_curve_[0] and all(0 < s < r for s, r in zip(fit.side_rate_curve_, fit.rate_curve_))
    sd = fit.state_dict()
    assert set(sd) == set(synthetic_hyperprior_state_dict(0, C))
    HRateHyperprior(C).load_state_dict(sd, strict=True)
    again = HyperpriorFit(0.05, **kw).fit(Z[:N]).state_dict()
    assert all(torch.equal(sd[k], again[k]) for k in sd), "the same seed gave another state dict"
    other = HyperpriorFit(0.05, **dict(kw, seed=2)).initial_estimator(C)
    assert not torch.equal(other.z_encoder.module[0].weight, fresh.z_encoder.module[0].weight)
    w = fresh.side_encoder.module[0].weight.detach()                     # weights_init: uniform in +-sqrt(6 / fan_in), zero biases
    assert float(w.abs().max()) <= math.sqrt(6 / C) and float(w.abs().max()) > 0.95 * math.sqrt(6 / C)
    assert not bool(fresh.z_encoder.module[4].bias.any())


def test_refusals():
    with pytest.raises(ValueError, match="not built"):
        HyperpriorFit(0.05, is_pred_mean=False)
    with pytest.raises(ValueError):
        HyperpriorFit(0.05, filters=(3, 3))
    with pytest.raises(ValueError):
        HyperpriorFit(0.05, beta_anneal="geometric")
    with pytest.raises(ValueError):
        HyperpriorFit(0.05, scheduler="cosine")
    with pytest.raises(ValueError):
        HyperpriorFit(0.05, factor_dim=0)
    with pytest.raises(ValueError):
        HyperpriorFit(0.05, side_z_dim=0)
    with pytest.raises(ValueError):
        HyperpriorFit(-1.0)
    with pytest.raises(ValueError):
        HyperpriorFit(0.05).fit(torch.zeros(0, 8))
    with pytest.raises(ValueError):
        HyperpriorFit(0.05).fit(torch.zeros(8))
