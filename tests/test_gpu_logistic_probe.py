"""GPU: ``lla_softmax_pass`` against a float64 evaluation of the same sums, held to the rounding bound derived in
logistic_util.softmax_reference_and_bound, on both of its paths (K <= 32: the row statistics inside the pass; K > 32: the
row-statistics kernel first); its edge cases and repeatability; ``lla_svm_pass`` unchanged beside it; and ``LogisticProbe``
fitted from containers that stay compressed on the device against the CPU solver."""
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from conftest import load_tables
from logistic_util import binomial_objective64, row_weights, softmax_objective64, softmax_pass, softmax_reference_and_bound
from oracle import cbind, container
from probe_util import U, gamma, reference_and_bound, svm_pass

pytestmark = pytest.mark.gpu

BS, KS = (1, 31, 33, 65, 257), (1, 2, 3, 32, 33, 70)      # 32: a full fused tile; 33: two kernels, one class in the last tile
CW, TOL = 1.0, 1e-4


def _case(B, C, K, dtype, seed, pad=8, weights=True):
    """Rows with pitch C + pad (the padding poisoned), labels drawn from [-1, K] (both ends are no class), W, b, V, vb and
    class weights from [1e-3, 1]."""
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
    cw = (1e-3 + (1.0 - 1e-3) * torch.rand(K, generator=g)).cuda() if weights else None
    return flat, ld, y, W, b, V, vb, cw


def _check(got, val, bound, what):
    worst = {}
    for key, g in zip(("W", "b", "loss"), got):
        if val[key] is None:
            continue
        assert bool(torch.isfinite(g).all()), f"{what} out_{key} is not finite"
        err, lim = (g.double() - val[key]).abs(), bound[key]
        worst[key] = float((err / lim.clamp_min(1e-300)).max())
        assert bool((err <= lim).all()), f"{what} out_{key}: error / bound = {worst[key]:.3g}"
    return worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("C", [40, 512, 1024])
def test_kernel_against_float64_in_both_modes(C, dtype):
    seed, worst = 0, 0.0
    for B in BS:
        for K in KS:
            seed += 1
            flat, ld, y, W, b, V, vb, cw = _case(B, C, K, dtype, seed, weights=seed % 2 == 1)
            Z = flat[:, :C]
            for Vm, vbm in ((None, None), (V, vb)):
                val, bound = softmax_reference_and_bound(Z, y, W, b, Vm, vbm, cw)
                got = softmax_pass(flat, ld, y, B, C, W, b, Vm, vbm, K, cw)
                w = _check(got, val, bound, f"B {B} C {C} K {K} {'hv' if Vm is not None else 'grad'}")
                worst = max(worst, *w.values())
                if Vm is not None:
                    assert bool((got[2] == 7.0).all())            # out_loss is not touched in Hessian-vector mode
    print(f"C {C} {dtype}: largest error / bound = {worst:.3g}")


@pytest.mark.parametrize("K", [10, 70])
def test_scores_of_magnitude_200(K):
    B, C = 65, 512
    flat, ld, y, W, b, V, vb, cw = _case(B, C, K, torch.float32, 40 + K)
    Z = flat[:, :C]
    W = W * float(200.0 / (Z.double() @ W.double().T).abs().max())
    assert 150.0 < float((Z.double() @ W.double().T + b.double()).abs().max()) < 250.0
    for Vm, vbm in ((None, None), (V, vb)):
        val, bound = softmax_reference_and_bound(Z, y, W, b, Vm, vbm, cw)
        _check(softmax_pass(flat, ld, y, B, C, W, b, Vm, vbm, K, cw), val, bound, f"|s| ~ 200, K {K}")
    # one class dominates: p = 1 to fp32 for it and 0 for the rest, so the residual of a row labelled with it is within u of 0
    z1 = torch.randn(1, C, generator=torch.Generator().manual_seed(K)).cuda()
    bd = b.clone()
    bd[K - 1] += 1000.0
    y1 = torch.tensor([K - 1], dtype=torch.int32).cuda()
    oW, ob, ol = softmax_pass(z1, C, y1, 1, C, W, bd, None, None, K)
    assert bool(torch.isfinite(oW).all()) and float(ob.abs().max()) <= U       # B = 1: out_b[k] is the residual r_0k
    assert float(ol.abs().max()) <= U * 1200.0                                 # lse - s_y = 0 up to the rounding of lse
    oW, ob, _ = softmax_pass(z1, C, y1, 1, C, W, bd, V, vb, K)                 # a = t of that class, p (t - a) = 0
    val, bound = softmax_reference_and_bound(z1, y1, W, bd, V, vb)
    _check((oW, ob, None), val, bound, "dominant class, hv")


def test_one_class_gives_exact_zeros():
    B, C, K = 65, 40, 1
    flat, ld, y, W, b, V, vb, cw = _case(B, C, K, torch.float32, 3)
    assert bool((y == 0).any()) and bool((y != 0).any())
    for Vm, vbm in ((None, None), (V, vb)):
        for weights in (None, cw):
            oW, ob, ol = softmax_pass(flat, ld, y, B, C, W, b, Vm, vbm, K, weights)
            assert bool((oW == 0).all()) and bool((ob == 0).all()) and (Vm is not None or bool((ol == 0).all()))


@pytest.mark.parametrize("K", [10, 70])
def test_rows_without_a_class_contribute_exactly_nothing(K):
    B, C = 65, 40
    flat, ld, y, W, b, V, vb, cw = _case(B, C, K, torch.float32, 4)
    y = torch.where(torch.arange(B) % 2 == 0, -1, K + torch.arange(B) % 3).to(torch.int32).cuda()
    for Vm, vbm in ((None, None), (V, vb)):
        oW, ob, ol = softmax_pass(flat, ld, y, B, C, W, b, Vm, vbm, K, cw)
        assert bool((oW == 0).all()) and bool((ob == 0).all()) and (Vm is not None or bool((ol == 0).all()))


@pytest.mark.parametrize("K", [10, 37])
def test_accumulate_over_two_calls_equals_the_union(K):
    B, C = 257, 512
    flat, ld, y, W, b, V, vb, cw = _case(B, C, K, torch.float32, 7)
    cut = 100
    for Vm, vbm in ((None, None), (V, vb)):
        out = softmax_pass(flat[:cut], ld, y[:cut], cut, C, W, b, Vm, vbm, K, cw)
        out = softmax_pass(flat[cut:], ld, y[cut:], B - cut, C, W, b, Vm, vbm, K, cw, out=out, accumulate=1)
        val, bound = softmax_reference_and_bound(flat[:, :C], y, W, b, Vm, vbm, cw)
        # (two partial totals and one more addition: within the bound of the whole, which allows B + 8 additions)
        _check(out, val, bound, "accumulate")
        keep = [t.clone() for t in out]
        softmax_pass(flat, ld, y, 0, C, W, b, Vm, vbm, K, cw, out=out, accumulate=1)   # B = 0: nothing is touched
        assert all(torch.equal(a, c) for a, c in zip(out, keep))
        zeroed = softmax_pass(flat, ld, y, 0, C, W, b, Vm, vbm, K, cw)                 # B = 0 without it: zeros
        assert bool((zeroed[0] == 0).all()) and bool((zeroed[1] == 0).all())


@pytest.mark.parametrize("K", [10, 70])
def test_two_calls_give_the_same_bits(K):
    B, C = 257, 512
    flat, ld, y, W, b, V, vb, cw = _case(B, C, K, torch.float32, 11)
    for Vm, vbm in ((None, None), (V, vb)):
        a = softmax_pass(flat, ld, y, B, C, W, b, Vm, vbm, K, cw)
        c = softmax_pass(flat, ld, y, B, C, W, b, Vm, vbm, K, cw)
        assert all(torch.equal(p, q) for p, q in zip(a, c))


def test_the_hinge_pass_is_what_it_was():
    """``lla_svm_pass`` shares its walk with the softmax pass: the same float64 bound, and the same bits from two calls."""
    B, C, K = 257, 512, 37
    g = torch.Generator().manual_seed(11)
    flat = torch.full((B, C + 8), float("nan"))
    flat[:, :C] = torch.randn(B, C, generator=g)
    flat = flat.cuda()
    y = torch.randint(-1, K + 1, (B,), generator=g).to(torch.int32).cuda()
    W, b = (torch.randn(K, C, generator=g) * (0.7 / C ** 0.5)).cuda(), (torch.randn(K, generator=g) * 0.3).cuda()
    V, vb = torch.randn(K, C, generator=g).cuda(), torch.randn(K, generator=g).cuda()
    for Vm, vbm in ((None, None), (V, vb)):
        val, bound = reference_and_bound(flat[:, :C], y, W, b, Vm, vbm)
        a = svm_pass(flat, C + 8, y, B, C, W, b, Vm, vbm, K)
        c = svm_pass(flat, C + 8, y, B, C, W, b, Vm, vbm, K)
        for key, got in zip(("W", "b", "loss"), a):
            if val[key] is not None:
                assert bool(((got.double() - val[key]).abs() <= bound[key]).all()), key
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
    """Containers of N in-window records on the device (means by row % 6 for the labels % 3 and % 2, by row % 37 for the
    labels % 37), their rows, and the CPU solver's fits."""
    import hubconf
    from lossyless_amd import LogisticProbe
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    tab = load_tables("5e-02")
    out = {}
    for n_means, ks in ((6, (3, 2)), (37, (37,))):
        sym = _class_symbols(tab, N, n_means, seed=31)
        file = tmp_path_factory.mktemp("logistic") / f"z{n_means}.bin"
        container.write_container(str(file), [cbind.rans_encode(s, tab["cdf"], tab["cdf_len"], tab["offset"]) for s in sym])
        ds = comp.open_dataset(file)
        rows = ds.all().cpu()
        for k in ks:
            out[k] = dict(ds=ds, rows=rows, cpu=LogisticProbe(C=CW, tol=TOL).fit(rows, torch.arange(N) % k))
    return out


def _stacked(W, b):
    return torch.cat([W.double(), b.double()[:, None]], 1)


def _check_fit(gpu, cpu, rows, labels):
    """The issue's four inequalities at the fitted weights -> |theta_gpu - theta_cpu|_2."""
    assert np.array_equal(gpu.classes_, cpu.classes_) and gpu.coef_.is_cuda and gpu.coef_.dtype == torch.float32
    assert tuple(gpu.coef_.shape) == tuple(cpu.coef_.shape) and gpu.converged_ and cpu.converged_
    idx, w = row_weights(cpu, labels, None)
    Wg, bg = gpu.coef_.cpu(), gpu.intercept_.cpu()
    K = len(cpu.classes_)
    if K == 2:                           # the binomial objective; the passes saw the K = 2 softmax at (-w / 2, w / 2) with C / 2
        sign = 2.0 * idx.double() - 1.0
        grad = lambda W, b: torch.cat([t.reshape(-1) for t in binomial_objective64(W[0], b[0], rows, sign, w, CW)[1:]])  # noqa: E731
        Ws, bs = torch.cat([-Wg, Wg]) / 2, torch.cat([-bg, bg]) / 2
        _, bound = softmax_reference_and_bound(rows, idx, Ws, bs)
        kb = 2.0 * (CW / 2) * max(float(bound["W"].max()), float(bound["b"].max()))
    else:
        grad = lambda W, b: _stacked(*softmax_objective64(W, b, rows, idx, w, CW)[1:]).reshape(-1)    # noqa: E731
        _, bound = softmax_reference_and_bound(rows, idx, Wg, bg)
        kb = CW * max(float(bound["W"].max()), float(bound["b"].max()))
    g0 = float(grad(torch.zeros_like(Wg), torch.zeros_like(bg)).abs().max())
    g_gpu, g_cpu = grad(Wg, bg), grad(cpu.coef_, cpu.intercept_)
    dist = float((_stacked(Wg, bg) - _stacked(cpu.coef_, cpu.intercept_)).norm())
    print(f"K {K}: passes {gpu.n_passes_} (cpu {cpu.n_passes_}), |g|inf {float(g_gpu.abs().max()):.3e} <= {2 * TOL * g0:.3e} + "
          f"{kb:.3e}; |theta_gpu - theta_cpu| {dist:.3e} <= {float(g_gpu.norm()):.3e} + {float(g_cpu.norm()):.3e}")
    assert float(g_gpu.abs().max()) <= 2 * TOL * g0 + kb
    assert dist <= float(g_gpu.norm()) + float(g_cpu.norm())
    return dist


def _check_predictions(gpu, cpu, ds, rows, labels, dist):
    n, K = rows.shape[0], len(cpu.classes_)
    s_gpu, s_cpu = gpu.decision_function(ds).cpu().double(), cpu.decision_function(rows)
    assert tuple(s_gpu.shape) == ((n,) if K == 2 else (n, K)) and s_gpu.shape == s_cpu.shape
    Es = gamma(512 + 2) * (rows.double().abs() @ gpu.coef_.cpu().double().abs().T + gpu.intercept_.cpu().double().abs())
    lim = dist * (rows.double().norm(dim=1, keepdim=True) + 1.0) + Es
    assert bool(((s_gpu - s_cpu).abs().reshape(n, -1) <= lim).all())
    proba = gpu.predict_proba(ds)
    assert tuple(proba.shape) == (n, K) and float((proba.double().sum(1) - 1).abs().max()) <= 1e-6
    assert gpu.score(ds, labels) == float((gpu.predict(ds).cpu() == labels).double().mean())
    assert gpu.score(ds, labels) > 0.9


@pytest.mark.parametrize("n_classes", [3, 2, 37])
def test_fit_from_compressed_latents_on_the_device(factorized, n_classes):
    from lossyless_amd import LogisticProbe
    ds, rows, cpu = (factorized[n_classes][k] for k in ("ds", "rows", "cpu"))
    labels = torch.arange(N) % n_classes
    for kw in (dict(), dict(rows_per_pass=128), dict(keep_rows=True)):
        gpu = LogisticProbe(C=CW, tol=TOL).fit(ds, labels, **kw)
        dist = _check_fit(gpu, cpu, rows, labels)
    _check_predictions(gpu, cpu, ds, rows, labels, dist)


@pytest.mark.parametrize("n_classes,kw", [(3, dict(rows_per_pass=128)), (2, dict(keep_rows=True)), (37, dict())],
                         ids=["3-groups", "2-kept", "37-default"])
def test_fit_from_hyperprior_latents(n_classes, kw):
    from hyperprior_latents_util import hyper_model
    from lossyless_amd import HyperpriorLatents, LogisticProbe
    model = hyper_model()
    g = torch.Generator().manual_seed(3)
    labels = torch.arange(N) % n_classes
    z = (torch.randn(n_classes, 512, generator=g)[labels] * 0.5 + torch.randn(N, 512, generator=g) * 0.7).cuda()
    z_strings, side_strings = model.compress(z)
    with tempfile.TemporaryDirectory() as d:
        file = os.path.join(d, "z.bin")
        container.write_container(file, [s for pair in zip(z_strings, side_strings) for s in pair])
        ds = HyperpriorLatents(file, types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()),
                                                           hyperprior=model))
    rows = ds.all().cpu()
    cpu = LogisticProbe(C=CW, tol=TOL).fit(rows, labels)
    gpu = LogisticProbe(C=CW, tol=TOL).fit(ds, labels, **kw)
    dist = _check_fit(gpu, cpu, rows, labels)
    _check_predictions(gpu, cpu, ds, rows, labels, dist)
