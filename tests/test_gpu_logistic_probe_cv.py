"""GPU: ``lla_softmax_grid_pass`` against a float64 evaluation of every group, held to the bound derived for
``lla_softmax_pass`` (logistic_util.softmax_reference_and_bound, applied per group to that group's labels and weights), over
every way K classes pack into a 32-column tile; bit-equality with ``lla_softmax_pass`` where the grids agree; isolation of
the groups inside a tile; and ``LogisticProbeCV`` fitted from containers that stay compressed against its CPU twin."""
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from conftest import load_tables
from logistic_cv_util import grid_reference_and_bound, group_labels, softmax_grid_pass, within_strong_convexity
from logistic_util import softmax_pass
from oracle import cbind, container
from probe_cv_util import check_cv_scores, class_symbols, stratified_folds

pytestmark = pytest.mark.gpu

BS, CS = (1, 31, 33, 65, 257), (40, 512, 1024)
# (K, G): one tile with two dead columns; a second tile with one group; three tiles; ...; no dead columns, then a spill;
# 15 dead columns per tile; full tiles of one group; one class (exact zeros)
KGS = ((10, 3), (10, 4), (10, 7), (3, 10), (3, 11), (2, 16), (2, 17), (16, 2), (16, 3), (17, 1), (17, 3), (32, 2), (1, 5))
TOL = 1e-4


def _case(B, C, K, G, dtype, seed, pad=8, weights=True, folds=True):
    """Rows with pitch C + pad (the padding poisoned), labels from [-1, K] (both ends are no class), three folds, groups
    that hold out fold 0, 1, 2 or none (-1), W, b, V, vb for G K columns and class weights from [1e-3, 1]."""
    g = torch.Generator().manual_seed(seed)
    ld = C + pad
    flat = torch.full((B, ld), float("nan"))
    flat[:, :C] = torch.randn(B, C, generator=g)
    flat = flat.to(dtype).cuda()
    y = torch.randint(-1, K + 1, (B,), generator=g).to(torch.int32).cuda()
    fold = torch.randint(0, 3, (B,), generator=g).to(torch.int32).cuda() if folds else None
    held = torch.tensor([(j % 4) - 1 for j in range(1, G + 1)], dtype=torch.int32).cuda()      # 0, 1, 2, -1, 0, ...
    W = (torch.randn(G * K, C, generator=g) * (0.7 / C ** 0.5)).cuda()
    b = (torch.randn(G * K, generator=g) * 0.3).cuda()
    V = torch.randn(G * K, C, generator=g).cuda()
    vb = torch.randn(G * K, generator=g).cuda()
    cw = (1e-3 + (1.0 - 1e-3) * torch.rand(G, K, generator=g)).cuda() if weights else None
    return flat, ld, y, fold, held, W, b, V, vb, cw


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
def test_kernel_against_float64_in_both_modes(dtype):
    """A sparse grid: every (K, G), every B and every C, each in both modes; weights and the fold array alternate with NULL."""
    worst = 0.0
    for i, (K, G) in enumerate(KGS):
        for B, C in {(BS[i % 5], CS[i % 3]), (BS[(i + 2) % 5], CS[(i + 1) % 3])}:
            flat, ld, y, fold, held, W, b, V, vb, cw = _case(B, C, K, G, dtype, 100 + i, weights=i % 2 == 0, folds=i % 3 != 2)
            Z = flat[:, :C]
            for Vm, vbm in ((None, None), (V, vb)):
                val, bound = grid_reference_and_bound(Z, y, fold, W, b, K, G, held, cw, Vm, vbm)
                got = softmax_grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, K, G, held, cw)
                w = _check(got, val, bound, f"B {B} C {C} K {K} G {G} {'hv' if Vm is not None else 'grad'}")
                worst = max(worst, *w.values())
                if Vm is not None:
                    assert bool((got[2] == 7.0).all())            # out_loss is not touched in Hessian-vector mode
                if K == 1:
                    assert all(bool((t == 0).all()) for t in got[:2 if Vm is not None else 3])     # one class: exact zeros
    print(f"{dtype}: largest error / bound = {worst:.3g}")


def test_a_group_that_holds_every_row_out_gives_exact_zeros():
    B, C, K, G = 65, 40, 10, 4
    flat, ld, y, fold, held, W, b, V, vb, cw = _case(B, C, K, G, torch.float32, 3)
    fold = torch.full_like(fold, 2)
    held = torch.tensor([0, 2, -1, 2], dtype=torch.int32).cuda()
    for Vm, vbm in ((None, None), (V, vb)):
        oW, ob, ol = softmax_grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, K, G, held, cw)
        for g in (1, 3):
            sl = slice(g * K, (g + 1) * K)
            assert bool((oW[sl] == 0).all()) and bool((ob[sl] == 0).all()) and (Vm is not None or bool((ol[sl] == 0).all()))
        assert bool((oW[:K] != 0).any()) and bool((oW[2 * K:3 * K] != 0).any())


@pytest.mark.parametrize("B,C,K,G", [(257, 512, 10, 3), (65, 40, 3, 10), (257, 512, 32, 1)])
def test_one_tile_gives_the_bits_of_the_softmax_pass(B, C, K, G):
    """One tile: the grid is that of ``lla_softmax_pass`` for these K classes, and every group's slice is bitwise what it
    returns for (W_g, b_g, the labels with the group's held-out rows relabelled -1, the group's class weights)."""
    flat, ld, y, fold, held, W, b, V, vb, cw = _case(B, C, K, G, torch.float32, 21)
    for Vm, vbm in ((None, None), (V, vb)):
        oW, ob, ol = softmax_grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, K, G, held, cw)
        for g in range(G):
            sl = slice(g * K, (g + 1) * K)
            yg = group_labels(y, fold, held, g).contiguous()
            rW, rb, rl = softmax_pass(flat, ld, yg, B, C, W[sl].contiguous(), b[sl].contiguous(),
                                      None if Vm is None else Vm[sl].contiguous(), None if vbm is None else vbm[sl].contiguous(),
                                      K, cw[g].contiguous())
            assert torch.equal(oW[sl], rW) and torch.equal(ob[sl], rb), f"group {g}"
            assert Vm is not None or torch.equal(ol[sl], rl), f"group {g} loss"


def test_groups_inside_a_tile_do_not_see_each_other():
    """One group's W of magnitude 1e30: the other two groups of the tile keep their bits (a statistics loop that ran over a
    neighbour's columns would not)."""
    B, C, K, G = 65, 512, 10, 3
    flat, ld, y, fold, held, W, b, V, vb, cw = _case(B, C, K, G, torch.float32, 5)
    W2 = W.clone()
    W2[K:2 * K] = torch.where(W[K:2 * K] > 0, 1e30, -1e30)
    for Vm, vbm in ((None, None), (V, vb)):
        a = softmax_grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, K, G, held, cw)
        c = softmax_grid_pass(flat, ld, y, fold, B, C, W2, b, Vm, vbm, K, G, held, cw)
        for sl in (slice(0, K), slice(2 * K, 3 * K)):
            assert all(torch.equal(p[sl], q[sl]) for p, q in zip(a, c))


def test_scores_of_magnitude_200_and_a_dominating_class():
    B, C, K, G = 65, 512, 10, 4
    flat, ld, y, fold, held, W, b, V, vb, cw = _case(B, C, K, G, torch.float32, 50)
    Z = flat[:, :C]
    W = W * float(200.0 / (Z.double() @ W.double().T).abs().max())
    assert 150.0 < float((Z.double() @ W.double().T + b.double()).abs().max()) < 250.0
    for Vm, vbm in ((None, None), (V, vb)):
        val, bound = grid_reference_and_bound(Z, y, fold, W, b, K, G, held, cw, Vm, vbm)
        _check(softmax_grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, K, G, held, cw), val, bound, "|s| ~ 200")
    # one class dominates in every group: p = 1 to fp32 for it, so the residual of a row labelled with it is within u of 0
    bd = b.clone()
    bd[K - 1::K] += 1000.0
    z1 = torch.randn(1, C, generator=torch.Generator().manual_seed(K)).cuda()
    y1 = torch.tensor([K - 1], dtype=torch.int32).cuda()
    U = 2.0 ** -24
    oW, ob, ol = softmax_grid_pass(z1, C, y1, None, 1, C, W, bd, None, None, K, G, held)
    assert bool(torch.isfinite(oW).all()) and float(ob.abs().max()) <= U and float(ol.abs().max()) <= U * 1200.0
    val, bound = grid_reference_and_bound(z1, y1, None, W, bd, K, G, held, None, V, vb)
    _check(softmax_grid_pass(z1, C, y1, None, 1, C, W, bd, V, vb, K, G, held)[:2] + (None,), val, bound, "dominant class, hv")


def test_accumulate_over_two_calls_equals_the_union():
    B, C, K, G = 257, 512, 10, 4
    flat, ld, y, fold, held, W, b, V, vb, cw = _case(B, C, K, G, torch.float32, 7)
    cut = 100
    for Vm, vbm in ((None, None), (V, vb)):
        out = softmax_grid_pass(flat[:cut], ld, y[:cut], fold[:cut], cut, C, W, b, Vm, vbm, K, G, held, cw)
        out = softmax_grid_pass(flat[cut:], ld, y[cut:], fold[cut:], B - cut, C, W, b, Vm, vbm, K, G, held, cw, out=out,
                                accumulate=1)
        val, bound = grid_reference_and_bound(flat[:, :C], y, fold, W, b, K, G, held, cw, Vm, vbm)
        # (two partial totals and one more addition: within the bound of the whole, which allows B + 8 additions)
        _check(out, val, bound, "accumulate")
        keep = [t.clone() for t in out]
        softmax_grid_pass(flat, ld, y, fold, 0, C, W, b, Vm, vbm, K, G, held, cw, out=out, accumulate=1)   # B = 0: untouched
        assert all(torch.equal(a, c) for a, c in zip(out, keep))
        zeroed = softmax_grid_pass(flat, ld, y, fold, 0, C, W, b, Vm, vbm, K, G, held, cw)                 # B = 0 without it
        assert bool((zeroed[0] == 0).all()) and bool((zeroed[1] == 0).all())


def test_two_calls_give_the_same_bits():
    B, C, K, G = 257, 512, 10, 7
    flat, ld, y, fold, held, W, b, V, vb, cw = _case(B, C, K, G, torch.float32, 11)
    for Vm, vbm in ((None, None), (V, vb)):
        a = softmax_grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, K, G, held, cw)
        c = softmax_grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, K, G, held, cw)
        assert all(torch.equal(p, q) for p, q in zip(a, c))


# ------------------------------------------------------------------ end to end
N = 600
CANDIDATES = [(0.01, None), (1.0, "balanced"), (0.1, {0: 1.5})]     # (on the CPU the twin leaves no held-out row undecided)


def _check_search(gpu, cpu, rows, labels, n_folds=3):
    """The device search against its CPU twin on the decoded rows: every classifier converged, every coefficient set within
    the strong-convexity bound of the twin's, the scores those of a float64 evaluation of the returned coefficients (rows
    inside the fp32 score bound left out, at most 1 % of a fold; the twin alone leaves out none)."""
    fold = stratified_folds(labels, n_folds)
    nc, K = len(CANDIDATES), len(cpu.classes_)
    Kp = 1 if K == 2 else K
    assert gpu.fold_coef_.is_cuda and gpu.fold_coef_.dtype == torch.float32
    assert tuple(gpu.fold_coef_.shape) == tuple(cpu.fold_coef_.shape) == (nc, n_folds, Kp, rows.shape[1])
    assert bool(gpu.converged_.all()) and tuple(gpu.converged_.shape) == (nc, n_folds + 1)
    assert np.array_equal(gpu.classes_, cpu.classes_) and gpu.folds_ == cpu.folds_
    for c, (Cw, cw) in enumerate(CANDIDATES):
        for f in range(n_folds):
            train = fold != f
            within_strong_convexity(gpu.fold_coef_[c, f], gpu.fold_intercept_[c, f], cpu.fold_coef_[c, f],
                                    cpu.fold_intercept_[c, f], rows[train], labels[train], cpu.classes_, Cw, cw,
                                    f"K {K} candidate {c} fold {f}")
    assert check_cv_scores(cpu, rows, labels, fold, cap=0.0) == 0.0
    worst = check_cv_scores(gpu, rows, labels, fold)
    print(f"largest share of held-out rows inside the fp32 score bound: {worst:.4f}")
    assert gpu.best_index_ == int(np.argmax(gpu.mean_scores_.numpy()))
    Cw, cw = CANDIDATES[gpu.best_index_]
    best, twin = gpu.best_estimator_, cpu.best_estimator_
    if gpu.best_index_ == cpu.best_index_:
        within_strong_convexity(best.coef_, best.intercept_, twin.coef_, twin.intercept_, rows, labels, cpu.classes_, Cw, cw,
                                "best_estimator_")
    assert best.converged_ and best.coef_.is_cuda and best.C == Cw and best.class_weight == cw


@pytest.fixture(scope="module")
def factorized(tmp_path_factory):
    """Containers of N in-window records on the device (means by row % 6 for the labels % 3 and % 2, by row % 37 for the
    labels % 37) and their decoded rows."""
    import hubconf
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    tab = load_tables("5e-02")
    out = {}
    for n_means, ks in ((6, (3, 2)), (37, (37,))):
        sym = class_symbols(tab, N, n_means, seed=31)
        file = tmp_path_factory.mktemp("logistic_cv") / f"z{n_means}.bin"
        container.write_container(str(file), [cbind.rans_encode(s, tab["cdf"], tab["cdf_len"], tab["offset"]) for s in sym])
        ds = comp.open_dataset(file)
        rows = ds.all().cpu()
        for k in ks:
            out[k] = dict(ds=ds, rows=rows)
    return out


@pytest.mark.parametrize("n_classes", [3, 2])
def test_search_from_compressed_latents_on_the_device(factorized, n_classes):
    from lossyless_amd import LogisticProbeCV
    ds, rows = factorized[n_classes]["ds"], factorized[n_classes]["rows"]
    labels = torch.arange(N) % n_classes
    cpu = LogisticProbeCV(CANDIDATES, cv=3, tol=TOL).fit(rows, labels)
    for kw in (dict(), dict(rows_per_pass=128), dict(keep_rows=True)):
        gpu = LogisticProbeCV(CANDIDATES, cv=3, tol=TOL).fit(ds, labels, **kw)
        _check_search(gpu, cpu, rows, labels)
    # (labels % 2 over means by row % 6: every stratified fold holds out a cluster its training part never saw)
    assert n_classes == 2 or float(gpu.cv_scores_.min()) > 0.8
    assert gpu.best_estimator_.score(ds, labels) > 0.9
    proba = gpu.best_estimator_.predict_proba(ds)
    assert tuple(proba.shape) == (N, n_classes) and float((proba.double().sum(1) - 1).abs().max()) <= 1e-6


def test_more_than_32_classes_take_the_softmax_pass_per_classifier(factorized):
    """K = 37: ``lla_softmax_grid_pass`` refuses it, so the passes are ``lla_softmax_pass`` per classifier on the shared rows."""
    from lossyless_amd import LogisticProbeCV
    ds, rows = factorized[37]["ds"], factorized[37]["rows"]
    labels = torch.arange(N) % 37
    cpu = LogisticProbeCV(CANDIDATES, cv=3, tol=TOL).fit(rows, labels)
    gpu = LogisticProbeCV(CANDIDATES, cv=3, tol=TOL).fit(ds, labels, rows_per_pass=256)
    _check_search(gpu, cpu, rows, labels)


@pytest.mark.parametrize("n_classes,kw", [(3, dict(rows_per_pass=128)), (2, dict(keep_rows=True))], ids=["3-groups", "2-kept"])
def test_search_from_hyperprior_latents(n_classes, kw):
    from hyperprior_latents_util import hyper_model
    from lossyless_amd import HyperpriorLatents, LogisticProbeCV
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
    cpu = LogisticProbeCV(CANDIDATES, cv=3, tol=TOL).fit(rows, labels)
    gpu = LogisticProbeCV(CANDIDATES, cv=3, tol=TOL).fit(ds, labels, **kw)
    _check_search(gpu, cpu, rows, labels)
