"""GPU: ``lla_bn_relu_dropout_fwd`` and ``lla_bn_bwd`` (csrc/batchnorm.hip) through the C ABI, against float64 -- held to a
multiple of what torch's own fp32 batch norm on the CPU does to the same inputs -- the dropout pattern against the CPU
Philox4x32-10, bit reproducibility, untouched padding and refusals."""
import ctypes

import pytest
import torch

from lossyless_amd import _lib, dropout_keep

pytestmark = pytest.mark.gpu

FACTOR = 4               # a different but fixed summation order (the margin of test_gpu_mlp_probe.py)
FLOOR = 2.0 ** -24       # of the tensor's maximum: one rounding to fp32
EPS, MOMENTUM, POISON = 1e-5, 0.1, 7.0
BS, NS = (2, 3, 33, 257), (8, 40, 2048)      # the minimum, odd, one past a 32-row step, one past 256 threads; the minimum
#                                              width, a ragged 32-column strip, the workload's width


def _pitched(t, pad=4):
    """[B, N] -> the [B, N + pad] poison-filled buffer holding it in its first N columns (on the device)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), POISON, dtype=torch.float32, device="cuda")
    buf[:, :t.shape[1]] = t
    return buf


def _fwd(a, ld, B, N, gamma, beta, out, ldo, mean, rstd, rm, rv, p=0.0, seed=0, step=0, layer=0):
    P = _lib.ptr
    rc = _lib.lib().lla_bn_relu_dropout_fwd(P(a), ld, P(gamma), P(beta), P(out), ldo, P(mean), P(rstd), P(rm), P(rv), B, N, EPS,
                                            MOMENTUM, p, seed, step, layer, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _bwd(g, ldg, a, lda, gamma, mean, rstd, p, dgamma, dbeta, da, ldda, B, N):
    P = _lib.ptr
    rc = _lib.lib().lla_bn_bwd(P(g), ldg, P(a), lda, P(gamma), P(mean), P(rstd), p, P(dgamma), P(dbeta), P(da), ldda, B, N,
                               _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _inputs(B, N, kind, seed=0):
    g = torch.Generator().manual_seed(1000 * B + N + seed)
    a = torch.randn(B, N, generator=g)
    if kind == "cancel":
        a = 1000.0 + a                        # E[a^2] - mean^2 would lose everything in fp32
    gamma, beta = 1.0 + 0.3 * torch.randn(N, generator=g), 0.3 * torch.randn(N, generator=g)
    rm, rv = 0.5 * torch.randn(N, generator=g), 0.5 + torch.rand(N, generator=g)
    return a, gamma, beta, rm, rv, torch.randn(B, N, generator=g)


def _forward64(a, gamma, beta, rm, rv):
    a, gamma, beta, B = a.double(), gamma.double(), beta.double(), a.shape[0]
    mean = a.sum(0) / B
    var = ((a - mean) ** 2).sum(0) / B
    rstd = 1.0 / torch.sqrt(var + EPS)
    h = (gamma * ((a - mean) * rstd) + beta).clamp_min(0.0)
    return dict(out=h, mean=mean, rstd=rstd, running_mean=(1 - MOMENTUM) * rm.double() + MOMENTUM * mean,
                running_var=(1 - MOMENTUM) * rv.double() + MOMENTUM * var * B / (B - 1))


def _forward32(a, gamma, beta, rm, rv):
    """torch's fp32 batch norm on the CPU (training mode), then ReLU."""
    rm, rv = rm.clone(), rv.clone()
    y, mean, rstd = torch.native_batch_norm(a, gamma, beta, rm, rv, True, MOMENTUM, EPS)
    return dict(out=torch.relu(y), mean=mean, rstd=rstd, running_mean=rm, running_var=rv)


def _hold(got, want, yardstick, what):
    """Per tensor: max |got - float64| <= max(FACTOR x max |torch fp32 - float64|, 2^-24 max |float64|); figures printed."""
    for k, w in want.items():
        err = float((got[k].double().cpu() - w).abs().max())
        e32 = float((yardstick[k].double() - w).abs().max())
        bar = max(FACTOR * e32, FLOOR * float(w.abs().max()))
        print(f"{what} {k}: device {err:.3e}, torch-CPU fp32 {e32:.3e}, ratio {err / e32 if e32 else float('nan'):.3f}, bar {bar:.3e}")
        assert err <= bar, f"{what} {k}: {err:.3e} above {bar:.3e}"


def _run_forward(a, gamma, beta, rm, rv, p=0.0, seed=0, step=0, layer=0, pad=4):
    B, N = a.shape
    ab, out = _pitched(a, pad), torch.full((B, N + pad), POISON, device="cuda")
    dev = dict(mean=torch.full((N,), POISON, device="cuda"), rstd=torch.full((N,), POISON, device="cuda"),
               running_mean=rm.cuda(), running_var=rv.cuda())
    rc = _fwd(ab, N + pad, B, N, gamma.cuda(), beta.cuda(), out, N + pad, dev["mean"], dev["rstd"], dev["running_mean"],
              dev["running_var"], p, seed, step, layer)
    assert rc == _lib.LLA_OK
    assert bool((out[:, N:] == POISON).all()) and bool((ab[:, N:] == POISON).all()) and torch.equal(ab[:, :N].cpu(), a)
    dev["out"] = out[:, :N].clone()
    return dev, ab


@pytest.mark.parametrize("kind", ["normal", "cancel"])
@pytest.mark.parametrize("B", BS)
def test_forward_against_float64(B, kind):
    for N in NS:
        a, gamma, beta, rm, rv, _ = _inputs(B, N, kind)
        dev, _ = _run_forward(a, gamma, beta, rm, rv)
        _hold(dev, _forward64(a, gamma, beta, rm, rv), _forward32(a, gamma, beta, rm, rv), f"fwd B={B} N={N} {kind}")
        again, _ = _run_forward(a, gamma, beta, rm, rv, p=0.0, seed=0x1234567890abcdef, step=9, layer=3)
        assert all(torch.equal(dev[k], again[k]) for k in dev)          # the same bits; p = 0 draws nothing, whatever the seed


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_dropout_pattern_is_the_cpu_philox(p):
    B, N = 33, 40
    a, gamma, beta, rm, rv, _ = _inputs(B, N, "normal")
    h = _run_forward(a, gamma, beta, rm, rv)[0]["out"].cpu()
    s = torch.tensor(1.0 / (1.0 - p), dtype=torch.float64).float()
    assert int((h > 0).sum()) > B * N // 4
    seen = []
    for seed, step, layer in ((0, 0, 0), (0xfedcba9876543210, 0, 1), (0xfedcba9876543210, 1, 0), (5, 4000000000, 7)):
        out = _run_forward(a, gamma, beta, rm, rv, p, seed, step, layer)[0]["out"].cpu()
        keep = dropout_keep(seed, step, layer, B, N, p)
        assert torch.equal((out != 0)[h > 0], keep[h > 0])
        assert torch.equal(out, torch.where(keep, h * s, torch.zeros(())))           # kept values are h s bit for bit
        assert torch.equal(out, _run_forward(a, gamma, beta, rm, rv, p, seed, step, layer, pad=0)[0]["out"].cpu())   # any pitch
        assert all(not torch.equal(keep, k) for k in seen)
        seen.append(keep)


def _backward_reference(a, gamma, beta, mask_s, dout, dtype):
    a = a.to(dtype).requires_grad_()
    gamma, beta = gamma.to(dtype).requires_grad_(), beta.to(dtype).requires_grad_()
    y = torch.nn.functional.batch_norm(a, None, None, gamma, beta, True, MOMENTUM, EPS)
    ((torch.relu(y) * mask_s.to(dtype)) * dout.to(dtype)).sum().backward()
    return dict(dgamma=gamma.grad, dbeta=beta.grad, da=a.grad)


@pytest.mark.parametrize("kind, p", [("normal", 0.0), ("normal", 0.5), ("cancel", 0.5)])
@pytest.mark.parametrize("B", BS)
def test_backward_against_float64_autograd(B, kind, p):
    seed, step, layer = 0x0badc0de0badc0de, 2, 1
    for N in NS:
        a, gamma, beta, rm, rv, dout = _inputs(B, N, kind, seed=7)
        dev, ab = _run_forward(a, gamma, beta, rm, rv, p, seed, step, layer)
        s = float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float64).float())
        mask_s = dropout_keep(seed, step, layer, B, N, p).double() * s if p else torch.ones(B, N, dtype=torch.float64)
        g = _pitched(torch.where(dev["out"] > 0, dout.cuda(), torch.zeros((), device="cuda")))    # what lla_gemm_f32_nn delivers
        da = torch.full((B, N + 4), POISON, device="cuda")
        got = dict(dgamma=torch.full((N,), POISON, device="cuda"), dbeta=torch.full((N,), POISON, device="cuda"))
        args = (ab, N + 4, gamma.cuda(), dev["mean"], dev["rstd"], p)
        assert _bwd(g, N + 4, *args, got["dgamma"], got["dbeta"], da, N + 4, B, N) == _lib.LLA_OK
        assert bool((da[:, N:] == POISON).all()) and bool((g[:, N:] == POISON).all())
        got["da"] = da[:, :N].clone()
        _hold(got, _backward_reference(a, gamma, beta, mask_s, dout, torch.float64),
              _backward_reference(a, gamma, beta, mask_s, dout, torch.float32), f"bwd B={B} N={N} {kind} p={p}")
        # in place, and again: the same bits
        dg2, db2 = torch.empty_like(got["dgamma"]), torch.empty_like(got["dbeta"])
        assert _bwd(g, N + 4, *args, dg2, db2, g, N + 4, B, N) == _lib.LLA_OK
        assert torch.equal(g[:, :N], got["da"]) and bool((g[:, N:] == POISON).all())
        assert torch.equal(dg2, got["dgamma"]) and torch.equal(db2, got["dbeta"])


def test_refusals_launch_nothing():
    B, N = 4, 8
    a, gamma, beta, rm, rv, dout = _inputs(B, N, "normal")
    ab, gamma, beta = _pitched(a), gamma.cuda(), beta.cuda()
    fresh = lambda *shape: torch.full(shape, POISON, device="cuda")                     # noqa: E731
    out, mean, rstd, rmd, rvd, g, dg, db = fresh(B, N + 4), fresh(N), fresh(N), fresh(N), fresh(N), fresh(B, N + 4), fresh(N), fresh(N)
    ld = N + 4

    def fwd(a_=ab, lda=ld, B_=B, N_=N, ldo=ld, p=0.2, out_=out):
        return _fwd(a_, lda, B_, N_, gamma, beta, out_, ldo, mean, rstd, rmd, rvd, p, 1, 0, 0)

    def bwd(g_=g, ldg=ld, B_=B, N_=N, ldda=ld, p=0.2, da_=g):
        return _bwd(g_, ldg, ab, ld, gamma, mean, rstd, p, dg, db, da_, ldda, B_, N_)

    off = ctypes.c_void_p(ab.data_ptr() + 4)                                           # 4-byte aligned only

    class Raw:
        def data_ptr(self):
            return off.value

    for rc in (fwd(B_=1), fwd(N_=6), fwd(lda=N - 4), fwd(ldo=N - 4), fwd(lda=N + 2), fwd(p=1.0), fwd(p=-0.1), fwd(a_=Raw()),
               fwd(out_=Raw()), fwd(B_=-1), fwd(N_=0), fwd(out_=ab),
               bwd(B_=1), bwd(N_=6), bwd(ldg=N - 4), bwd(ldda=N - 4), bwd(ldda=N + 2), bwd(p=1.0), bwd(g_=Raw()), bwd(da_=Raw()),
               bwd(da_=ab)):
        assert rc == _lib.LLA_EINVAL
    assert fwd(B_=0) == _lib.LLA_OK and bwd(B_=0) == _lib.LLA_OK
    for t in (out, mean, rstd, rmd, rvd, g, dg, db):
        assert bool((t == POISON).all())                                               # nothing was launched
    assert fwd() == _lib.LLA_OK and bool((out[:, :N] != POISON).any())
