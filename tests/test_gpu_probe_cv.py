"""GPU: ``lla_svm_grid_pass`` against a float64 evaluation of the same weighted, masked sums, held to the rounding bound
derived in probe_cv_util.grid_reference_and_bound; its exact cases (a problem whose held-out fold is every row, no fold
array, the shipped ``lla_svm_pass`` at unit weights); and ``LinearProbeCV`` fitted from containers that stay compressed
on the device against its CPU twin."""
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from conftest import load_tables
from oracle import cbind, container
from probe_cv_util import (check_cv_scores, class_symbols, grid_pass, grid_reference_and_bound, ovr_weights, stratified_folds,
                           within_strong_convexity)
from probe_util import make_data, svm_pass

pytestmark = pytest.mark.gpu

BS, JS = (1, 63, 65, 257), (1, 33, 70)
TOL = 1e-4
CANDIDATES = [(7e-3, None), (0.05, "balanced"), (0.3, None)]


def _case(B, C, J, dtype, seed, pad=8, n_labels=5):
    """Rows with pitch C + pad (the padding poisoned); labels from [-1, n_labels + 1] while the columns' classes are drawn
    from [0, n_labels) with repeats, in no order (so -1 and the two largest labels match no column); three folds and
    held-out folds from {-1, 0, 1, 2}; two weights per column from [1e-3, 1]."""
    g = torch.Generator().manual_seed(seed)
    ld = C + pad
    flat = torch.full((B, ld), float("nan"))
    flat[:, :C] = torch.randn(B, C, generator=g)
    flat = flat.to(dtype).cuda()
    y = torch.randint(-1, n_labels + 2, (B,), generator=g).to(torch.int32).cuda()
    fold = torch.randint(0, 3, (B,), generator=g).to(torch.int32).cuda()
    cols = (torch.randint(0, n_labels, (J,), generator=g).to(torch.int32).cuda(),
            torch.randint(-1, 3, (J,), generator=g).to(torch.int32).cuda(),
            (1e-3 + (1.0 - 1e-3) * torch.rand(J, generator=g)).cuda(), (1e-3 + (1.0 - 1e-3) * torch.rand(J, generator=g)).cuda())
    W = (torch.randn(J, C, generator=g) * (0.7 / C ** 0.5)).cuda()
    b = (torch.randn(J, generator=g) * 0.3).cuda()
    V = torch.randn(J, C, generator=g).cuda()
    vb = torch.randn(J, generator=g).cuda()
    return flat, ld, y, fold, cols, W, b, V, vb


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
        for J in JS:
            seed += 1
            flat, ld, y, fold, cols, W, b, V, vb = _case(B, C, J, dtype, seed)
            Z = flat[:, :C]
            for Vm, vbm in ((None, None), (V, vb)):
                val, bound = grid_reference_and_bound(Z, y, fold, W, b, cols, Vm, vbm)
                got = grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, cols)
                _check(got, val, bound, f"B {B} C {C} J {J} {'hv' if Vm is not None else 'grad'}")
                if Vm is not None:
                    assert bool((got[2] == 7.0).all())            # out_loss is not touched in Hessian-vector mode
    assert float(val["W"].abs().max()) > 0


def test_a_wrong_weight_or_fold_would_show():
    """The bound is ~1e-4 of what swapping the two weights or ignoring the fold moves."""
    B, C, J = 257, 40, 33
    flat, ld, y, fold, cols, W, b, V, vb = _case(B, C, J, torch.float32, 3)
    val, bound = grid_reference_and_bound(flat[:, :C], y, fold, W, b, cols)
    swapped, _ = grid_reference_and_bound(flat[:, :C], y, fold, W, b, (cols[0], cols[1], cols[3], cols[2]))
    unfolded, _ = grid_reference_and_bound(flat[:, :C], y, None, W, b, cols)
    for other in (swapped, unfolded):
        assert float(((other["W"] - val["W"]).abs() / bound["W"].clamp_min(1e-300)).max()) > 100


def test_exact_cases():
    B, C, J = 257, 40, 33
    flat, ld, y, fold, cols, W, b, V, vb = _case(B, C, J, torch.float32, 21)
    one = torch.ones_like(fold)
    out_of = cols[1] == 1
    assert 0 < int(out_of.sum()) < J
    for Vm, vbm in ((None, None), (V, vb)):
        # every row is in fold 1: the problems that hold fold 1 out see no row at all
        oW, ob, ol = grid_pass(flat, ld, y, one, B, C, W, b, Vm, vbm, cols)
        assert bool((oW[out_of] == 0).all()) and bool((ob[out_of] == 0).all()) and bool((oW[~out_of] != 0).any())
        assert Vm is not None or (bool((ol[out_of] == 0).all()) and bool((ol[~out_of] > 0).all()))
        # no fold array = a fold array no problem holds out
        a = grid_pass(flat, ld, y, None, B, C, W, b, Vm, vbm, cols)
        c = grid_pass(flat, ld, y, torch.full_like(fold, 7), B, C, W, b, Vm, vbm, cols)
        assert all(torch.equal(p, q) for p, q in zip(a, c))


@pytest.mark.parametrize("B,C,K", [(257, 512, 37), (65, 40, 3)])
def test_unit_weights_and_no_fold_give_the_bits_of_svm_pass(B, C, K):
    flat, ld, _, _, _, W, b, V, vb = _case(B, C, K, torch.float32, 13)
    y = torch.randint(-1, K + 1, (B,), generator=torch.Generator().manual_seed(2)).to(torch.int32).cuda()
    cols = (torch.arange(K, dtype=torch.int32).cuda(), torch.full((K,), -1, dtype=torch.int32).cuda(),
            torch.ones(K).cuda(), torch.ones(K).cuda())
    for Vm, vbm in ((None, None), (V, vb)):
        a = svm_pass(flat, ld, y, B, C, W, b, Vm, vbm, K)
        c = grid_pass(flat, ld, y, None, B, C, W, b, Vm, vbm, cols)
        assert all(torch.equal(p, q) for p, q in zip(a, c))
        assert float(a[0].abs().max()) > 0


def test_accumulate_over_two_calls_equals_the_union():
    B, C, J = 257, 512, 70
    flat, ld, y, fold, cols, W, b, V, vb = _case(B, C, J, torch.float32, 7)
    cut = 100
    for Vm, vbm in ((None, None), (V, vb)):
        out = grid_pass(flat[:cut], ld, y[:cut], fold[:cut], cut, C, W, b, Vm, vbm, cols)
        out = grid_pass(flat[cut:], ld, y[cut:], fold[cut:], B - cut, C, W, b, Vm, vbm, cols, out=out, accumulate=1)
        val, bound = grid_reference_and_bound(flat[:, :C], y, fold, W, b, cols, Vm, vbm)
        # (two partial totals and one more addition: within the bound of the whole, which allows B + 8 additions)
        _check(out, val, bound, "accumulate")
        keep = [t.clone() for t in out]
        grid_pass(flat, ld, y, fold, 0, C, W, b, Vm, vbm, cols, out=out, accumulate=1)      # B = 0: nothing is touched
        assert all(torch.equal(a, c) for a, c in zip(out, keep))


def test_two_calls_give_the_same_bits():
    B, C, J = 257, 512, 70
    flat, ld, y, fold, cols, W, b, V, vb = _case(B, C, J, torch.float32, 11)
    for Vm, vbm in ((None, None), (V, vb)):
        a = grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, cols)
        c = grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, cols)
        assert all(torch.equal(p, q) for p, q in zip(a, c))


# ------------------------------------------------------------------ end to end
def _check_search(gpu, cpu, rows, labels, n_folds=3):
    """The device search against its CPU twin on the decoded rows: every classifier converged, every coefficient set
    within the strong-convexity bound of the twin's, the scores those of a float64 evaluation of the returned
    coefficients (rows inside the fp32 score bound left out, at most 1 % of a fold)."""
    fold = stratified_folds(labels, n_folds)
    nc = len(CANDIDATES)
    assert gpu.fold_coef_.is_cuda and gpu.fold_coef_.dtype == torch.float32
    assert tuple(gpu.fold_coef_.shape) == tuple(cpu.fold_coef_.shape) == (nc, n_folds, 3, rows.shape[1])
    assert bool(gpu.converged_.all()) and tuple(gpu.converged_.shape) == (nc, n_folds + 1)
    assert np.array_equal(gpu.classes_, cpu.classes_) and gpu.folds_ == cpu.folds_
    for c, (CW, cw) in enumerate(CANDIDATES):
        for f in range(n_folds):
            train = fold != f
            Y, wts = ovr_weights(labels[train], gpu.classes_, CW, cw)
            within_strong_convexity(gpu.fold_coef_[c, f], gpu.fold_intercept_[c, f], cpu.fold_coef_[c, f],
                                    cpu.fold_intercept_[c, f], rows[train], Y, wts, f"candidate {c} fold {f}")
    worst = check_cv_scores(gpu, rows, labels, fold)
    print(f"largest share of held-out rows inside the fp32 score bound: {worst:.4f}")
    assert gpu.best_index_ == int(np.argmax(gpu.mean_scores_.numpy()))
    CW, cw = CANDIDATES[gpu.best_index_]
    Y, wts = ovr_weights(labels, gpu.classes_, CW, cw)
    best, twin = gpu.best_estimator_, cpu.best_estimator_
    if gpu.best_index_ == cpu.best_index_:
        within_strong_convexity(best.coef_, best.intercept_, twin.coef_, twin.intercept_, rows, Y, wts, "best_estimator_")
    assert best.converged_ and best.coef_.is_cuda and best.C == CW and best.class_weight == cw


def test_search_from_device_rows_of_the_cpu_tests_generator():
    """(600, 40, 3), class means 0.6 apart and unit noise: the generator on which test_probe_cv_host.py shows that the
    1 % cap on rows inside the score bound is reachable."""
    from lossyless_amd import LinearProbeCV
    X, y = make_data(600, 40, 3)
    labels = 2 * y + 1
    cpu = LinearProbeCV(CANDIDATES, cv=3, tol=TOL).fit(X, labels)
    gpu = LinearProbeCV(CANDIDATES, cv=3, tol=TOL).fit(X.cuda(), labels, rows_per_pass=256)
    _check_search(gpu, cpu, X, labels)
    few = LinearProbeCV(CANDIDATES, cv=3, tol=TOL, max_problems=15).fit(X.cuda(), labels, rows_per_pass=256)
    _check_search(few, cpu, X, labels)


def test_search_from_compressed_latents_on_the_device(tmp_path):
    import hubconf
    from lossyless_amd import LinearProbeCV
    N = 600
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    tab = load_tables("5e-02")
    sym = class_symbols(tab, N, 6, seed=31)
    file = tmp_path / "z.bin"
    container.write_container(str(file), [cbind.rans_encode(s, tab["cdf"], tab["cdf_len"], tab["offset"]) for s in sym])
    ds = comp.open_dataset(file)
    rows = ds.all().cpu()
    labels = torch.arange(N) % 3
    cpu = LinearProbeCV(CANDIDATES, cv=3, tol=TOL).fit(rows, labels)
    for kw in (dict(rows_per_pass=128), dict(keep_rows=True)):
        gpu = LinearProbeCV(CANDIDATES, cv=3, tol=TOL).fit(ds, labels, **kw)
        _check_search(gpu, cpu, rows, labels)
    assert float(gpu.cv_scores_.min()) > 0.8
    assert gpu.best_estimator_.score(ds, labels) > 0.9


def test_search_from_hyperprior_latents():
    from hyperprior_latents_util import hyper_model
    from lossyless_amd import HyperpriorLatents, LinearProbeCV
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
    cpu = LinearProbeCV(CANDIDATES, cv=3, tol=TOL).fit(rows, labels)
    gpu = LinearProbeCV(CANDIDATES, cv=3, tol=TOL).fit(ds, labels, rows_per_pass=128)
    _check_search(gpu, cpu, rows, labels)
