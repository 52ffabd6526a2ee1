"""GPU: ``lla_svm_pass`` against a float64 evaluation of the same sums, held to the rounding bound derived in
probe_util.reference_and_bound (a wrong row, class or tail shows at O(1) of the absolute sums the bound is ~1e-4 of), its
repeatability, and ``LinearProbe`` fitted from containers that stay compressed on the device against the CPU solver."""
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from conftest import load_tables
from oracle import cbind, container
from probe_util import gamma, grad_norms, probe_signs, reference_and_bound, signs, svm_pass

pytestmark = pytest.mark.gpu

BS, KS = (1, 63, 64, 65, 257), (1, 3, 32, 33, 37)
CW, TOL = 7e-3, 1e-4


def _case(B, C, K, dtype, seed, pad=8):
    """Rows with pitch C + pad (the padding poisoned), labels drawn from [-1, K] (both ends are no class), W, b, V, vb."""
    g = torch.Generator().manual_seed(seed)
    ld = C + pad
    flat = torch.full((B, ld), float("nan"))
    flat[:, :C] = torch.randn(B, C, generator=g)
    flat = flat.to(dtype).cuda()
    y = torch.randint(-1, K + 1, (B,), generator=g).to(torch.int32).cuda()
    W = (torch.randn(K, C, generator=g) * (0.7 / C ** 0.5)).cuda()
    b = (torch.randn(K, generator=g) * 0.3).cuda()
    V = torch.randn(K, C, generator=g).cuda()
    vb = torch.randn(K, generator=g).cuda()
    return flat, ld, y, W, b, V, vb


def _check(got, val, bound, what):
    for key, g in zip(("W", "b", "loss"), got):
        if val[key] is None:
            continue
        err, lim = (g.double() - val[key]).abs(), bound[key]
        worst = float((err / lim.clamp_min(1e-300)).max())
        assert bool((err <= lim).all()), f"{what} out_{key}: error / bound = {worst:.3g}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("C", [40, 512, 1024])
def test_kernel_against_float64_in_both_modes(C, dtype):
    seed = 0
    for B in BS:
        for K in KS:
            seed += 1
            flat, ld, y, W, b, V, vb = _case(B, C, K, dtype, seed)
            Z = flat[:, :C]
            for Vm, vbm in ((None, None), (V, vb)):
                val, bound = reference_and_bound(Z, y, W, b, Vm, vbm)
                got = svm_pass(flat, ld, y, B, C, W, b, Vm, vbm, K)
                _check(got, val, bound, f"B {B} C {C} K {K} {'hv' if Vm is not None else 'grad'}")
                if Vm is not None:
                    assert bool((got[2] == 7.0).all())            # out_loss is not touched in Hessian-vector mode


def test_every_margin_active_and_none_active():
    B, C, K = 257, 40, 37
    flat, ld, y, W, b, V, vb = _case(B, C, K, torch.float32, 99)
    zero, zb = torch.zeros_like(W), torch.zeros_like(b)
    for Vm, vbm in ((None, None), (V, vb)):                        # W = 0: m = 1 everywhere
        val, bound = reference_and_bound(flat[:, :C], y, zero, zb, Vm, vbm)
        _check(svm_pass(flat, ld, y, B, C, zero, zb, Vm, vbm, K), val, bound, "W = 0")
    assert float(val["b"].abs().max()) > 0
    # no margin active: rows = 10 e_class + small noise, W = 2 I, b = -6 -> y s >= 14 - 0.8, or 6 - 0.8
    g = torch.Generator().manual_seed(5)
    yv = torch.randint(0, K, (B,), generator=g)
    Z = 0.1 * torch.randn(B, C, generator=g)
    Z[torch.arange(B), yv] += 10.0
    Z, yv = Z.cuda().contiguous(), yv.to(torch.int32).cuda()
    Wi = torch.zeros(K, C)
    Wi[torch.arange(K), torch.arange(K)] = 2.0
    Wi, bi = Wi.cuda(), torch.full((K,), -6.0).cuda()
    margin = 1.0 - signs(yv.long(), K) * (Z.double() @ Wi.double().T + bi.double())
    assert float(margin.max()) < -1.0
    for Vm, vbm in ((None, None), (V, vb)):
        oW, ob, ol = svm_pass(Z, C, yv, B, C, Wi, bi, Vm, vbm, K)
        assert bool((oW == 0).all()) and bool((ob == 0).all()) and (Vm is not None or bool((ol == 0).all()))


def test_accumulate_over_two_calls_equals_the_union():
    B, C, K = 257, 512, 37
    flat, ld, y, W, b, V, vb = _case(B, C, K, torch.float32, 7)
    cut = 100
    for Vm, vbm in ((None, None), (V, vb)):
        out = svm_pass(flat[:cut], ld, y[:cut], cut, C, W, b, Vm, vbm, K)
        out = svm_pass(flat[cut:], ld, y[cut:], B - cut, C, W, b, Vm, vbm, K, out=out, accumulate=1)
        val, bound = reference_and_bound(flat[:, :C], y, W, b, Vm, vbm)
        # (two partial totals and one more addition: within the bound of the whole, which allows B + 8 additions)
        _check(out, val, bound, "accumulate")
        keep = [t.clone() for t in out]
        svm_pass(flat, ld, y, 0, C, W, b, Vm, vbm, K, out=out, accumulate=1)       # B = 0: nothing is touched
        assert all(torch.equal(a, c) for a, c in zip(out, keep))


def test_two_calls_give_the_same_bits():
    B, C, K = 257, 512, 37
    flat, ld, y, W, b, V, vb = _case(B, C, K, torch.float32, 11)
    for Vm, vbm in ((None, None), (V, vb)):
        a = svm_pass(flat, ld, y, B, C, W, b, Vm, vbm, K)
        c = svm_pass(flat, ld, y, B, C, W, b, Vm, vbm, K)
        assert all(torch.equal(p, q) for p, q in zip(a, c))


# ------------------------------------------------------------------ end to end
N = 600


def _class_symbols(tab, n, n_classes, seed):
    """Symbols inside every channel's coding window (no escapes: rows of ordinary size) whose mean depends on row % n_classes."""
    rng = np.random.default_rng(seed)
    C = tab["cdf"].shape[0]
    width = (tab["cdf_len"].astype(np.int64) - 2)[None, :]                 # symbols offset .. offset + width - 1
    means = rng.normal(size=(n_classes, C)) * 1.5
    v = np.rint(width / 2 + means[np.arange(n) % n_classes] + rng.normal(size=(n, C)) * 1.5)
    return (tab["offset"][None, :] + np.clip(v, 0, width - 1)).astype(np.int32)


@pytest.fixture(scope="module")
def factorized(tmp_path_factory):
    """A container of N in-window records on the device, its rows, and the CPU solver's fits for labels % 3 and % 2."""
    import hubconf
    from lossyless_amd import LinearProbe
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    tab = load_tables("5e-02")
    sym = _class_symbols(tab, N, 6, seed=31)
    file = tmp_path_factory.mktemp("probe") / "z.bin"
    container.write_container(str(file), [cbind.rans_encode(s, tab["cdf"], tab["cdf_len"], tab["offset"]) for s in sym])
    ds = comp.open_dataset(file)
    rows = ds.all().cpu()
    cpu = {k: LinearProbe(C=CW, tol=TOL).fit(rows, torch.arange(N) % k) for k in (3, 2)}
    return dict(ds=ds, rows=rows, cpu=cpu)


def _kernel_bound_at(rows, Y_idx, K, W, b):
    """sup over the gradient's entries of the kernel's rounding bound at (W, b), scaled as the objective scales it."""
    _, bound = reference_and_bound(rows, Y_idx, W, b)
    return CW * max(float(bound["W"].max()), float(bound["b"].max()))


def _check_fit(gpu, cpu, rows, labels):
    assert np.array_equal(gpu.classes_, cpu.classes_) and gpu.coef_.is_cuda and gpu.coef_.dtype == torch.float32
    assert tuple(gpu.coef_.shape) == tuple(cpu.coef_.shape) and gpu.converged_
    Y = probe_signs(cpu, labels)
    K = Y.shape[1]
    Wg, bg = gpu.coef_.cpu(), gpu.intercept_.cpu()
    zero = torch.zeros_like(Wg)
    g0, _ = grad_norms(zero, zero[:, 0], rows, Y, CW)
    ginf, g2 = grad_norms(Wg, bg, rows, Y, CW)
    _, g2_cpu = grad_norms(cpu.coef_, cpu.intercept_, rows, Y, CW)
    idx = torch.where(Y[:, 0] > 0, 0, 1) if K == 1 else Y.argmax(1)
    kb = _kernel_bound_at(rows, idx, K, Wg, bg)
    dist = float(torch.cat([(Wg - cpu.coef_).double(), (bg - cpu.intercept_).double()[:, None]], 1).norm())
    print(f"K {K}: passes {gpu.n_passes_} (cpu {cpu.n_passes_}), |g|inf {ginf:.3e} <= {2 * TOL * g0:.3e} + {kb:.3e}; "
          f"|W_gpu - W_cpu| {dist:.3e} <= {g2:.3e} + {g2_cpu:.3e}")
    assert ginf <= 2 * TOL * g0 + kb
    assert dist <= g2 + g2_cpu
    return dist


@pytest.mark.parametrize("n_classes", [3, 2])
def test_fit_from_compressed_latents_on_the_device(factorized, n_classes):
    from lossyless_amd import LinearProbe
    ds, rows, cpu = factorized["ds"], factorized["rows"], factorized["cpu"][n_classes]
    labels = torch.arange(N) % n_classes
    for kw in (dict(), dict(rows_per_pass=128), dict(keep_rows=True)):
        gpu = LinearProbe(C=CW, tol=TOL).fit(ds, labels, **kw)
        dist = _check_fit(gpu, cpu, rows, labels)
    s_gpu, s_cpu = gpu.decision_function(ds).cpu().double(), cpu.decision_function(rows)
    assert tuple(s_gpu.shape) == ((N,) if n_classes == 2 else (N, 3)) and s_gpu.shape == s_cpu.shape
    Es = gamma(512 + 2) * (rows.double().abs() @ gpu.coef_.cpu().double().abs().T + gpu.intercept_.cpu().double().abs())
    lim = dist * (rows.double().norm(dim=1, keepdim=True) + 1.0) + Es
    assert bool(((s_gpu - s_cpu).abs().reshape(N, -1) <= lim).all())
    assert gpu.score(ds, labels) == float((gpu.predict(ds).cpu() == labels).double().mean())
    assert gpu.score(ds, labels) > 0.9


def test_fit_from_hyperprior_latents():
    from hyperprior_latents_util import hyper_model
    from lossyless_amd import HyperpriorLatents, LinearProbe
    model = hyper_model()
    g = torch.Generator().manual_seed(3)
    n = 300
    labels = torch.arange(n) % 3
    z = (torch.randn(3, 512, generator=g)[labels] * 0.5 + torch.randn(n, 512, generator=g) * 0.7).cuda()
    z_strings, side_strings = model.compress(z)
    with tempfile.TemporaryDirectory() as d:
        file = os.path.join(d, "z.bin")
        container.write_container(file, [s for pair in zip(z_strings, side_strings) for s in pair])
        ds = HyperpriorLatents(file, types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()),
                                                           hyperprior=model))
    rows = ds.all().cpu()
    cpu = LinearProbe(C=CW, tol=TOL).fit(rows, labels)
    gpu = LinearProbe(C=CW, tol=TOL).fit(ds, labels, rows_per_pass=128)
    _check_fit(gpu, cpu, rows, labels)
