"""GPU: ``lla_kmeans_pass`` against float64 scores, held to the rounding bounds derived in kmeans_util -- assignment, tie order,
sums from the device's own assignment, exact counts, statistics, accumulation over groups, repeatability, predict-only and
B = 0 -- on both of its paths (K <= 32: one kernel; K > 32: assign kernel + sums walk); and ``KMeansProbe`` from containers
that stay compressed on the device against its float64 twin on the decompressed rows."""
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from conftest import load_tables
from kmeans_util import (centre_bound, check_assignment, check_totals, dist_and_bound, kmeans_pass, margin_inside,
                         scores_and_bound, twin_margins)
from oracle import cbind, container, eb
from probe_cv_util import class_symbols
from probe_util import U, gamma

pytestmark = pytest.mark.gpu

KS, BS = (1, 2, 10, 32, 33, 70), (1, 31, 33, 1000)


def _case(B, C, K, dtype, metric, seed, pad_z=8, pad_w=4):
    """Rows with pitch C + pad_z around K centroids and centroids with pitch C + pad_w (the padding poisoned); metric 0:
    b = -1/2 |c|^2 rounded once, metric 1: unit centroids and, for odd seeds, a small b (the kernel takes any)."""
    g = torch.Generator().manual_seed(seed)
    ld_z, ld_w = C + pad_z, C + pad_w
    c = torch.randn(K, C, generator=g)
    if metric == 1:
        c = c / c.norm(dim=1, keepdim=True)
    W = torch.full((K, ld_w), float("nan"))
    W[:, :C] = c
    z = torch.full((B, ld_z), float("nan"))
    z[:, :C] = c[torch.randint(0, K, (B,), generator=g)] * (1.0 if metric == 0 else 3.0) + 0.7 * torch.randn(B, C, generator=g)
    if B > 2:
        z[2, :C] = 0.0                                                  # a row of zeros: r = 0, every score is b
    if metric == 0:
        b = (-0.5 * (c.double() ** 2).sum(1)).float()
    else:
        b = 0.01 * torch.randn(K, generator=g) if seed % 2 else torch.zeros(K)
    return z.to(dtype).cuda(), ld_z, W.cuda(), ld_w, b.cuda()


def _check_call(z, ld_z, B, C, W, ld_w, b, K, metric, what):
    out = kmeans_pass(z, ld_z, B, C, W, b, K, ld_w, metric)
    Z, Wc = z[:, :C], W[:, :C]
    ref = scores_and_bound(Z, Wc, b, metric)
    a = out[0].to(torch.int64)
    inside = check_assignment(ref, a, what)
    d64, Ed = dist_and_bound(ref, a, metric)
    err = (out[1].double() - d64).abs()
    assert bool((err <= Ed).all()), f"{what}: dist error / bound = {float((err / Ed.clamp_min(1e-300)).max()):.3g}"
    assert bool((out[1] >= 0).all()) or metric == 1
    worst = check_totals(Z, ref, out, K, C, metric, what)
    assert bool((out[2][:, C:] == 7.0).all()), f"{what}: the padding of out_sum was written"
    return out, ref, inside, worst


@pytest.mark.parametrize("metric", [0, 1], ids=["euclidean", "cosine"])
@pytest.mark.parametrize("C", [8, 512, 1024])
def test_kernels_against_float64(C, metric):
    seed, worst, inside, rows = 0, 0.0, 0, 0
    for K in KS:
        for B in BS:
            seed += 1
            dtype = torch.float16 if seed % 3 == 0 else torch.float32
            z, ld_z, W, ld_w, b = _case(B, C, K, dtype, metric, 1000 * C + seed)
            what = f"C {C} K {K} B {B} {dtype}"
            out, ref, n_in, w = _check_call(z, ld_z, B, C, W, ld_w, b, K, metric, what)
            worst, inside, rows = max(worst, w), inside + n_in, rows + B
            # a second call: the same bits
            again = kmeans_pass(z, ld_z, B, C, W, b, K, ld_w, metric)
            assert all(torch.equal(p, q) for p, q in zip(out, again)), f"{what}: two calls differ"
            # predict only: the same rows' outputs, the accumulators untouched
            pred = kmeans_pass(z, ld_z, B, C, W, b, K, ld_w, metric, sums=False)
            assert torch.equal(pred[0], out[0]) and torch.equal(pred[1], out[1]), f"{what}: predict-only differs"
            assert bool((pred[2] == 7.0).all()) and bool((pred[3] == 7.0).all()) and bool((pred[4] == 7.0).all())
            # accumulated over groups: identical rows' outputs, totals within the same bounds
            if B > 33:
                acc = None
                for g0 in range(0, B, 257):
                    g = min(257, B - g0)
                    part = kmeans_pass(z[g0:g0 + g], ld_z, g, C, W, b, K, ld_w, metric, accumulate=int(g0 > 0),
                                       out=None if acc is None else (acc[0][g0:], acc[1][g0:], acc[2], acc[3], acc[4]))
                    if acc is None:
                        acc = (torch.cat([part[0], torch.full((B - g,), -7, dtype=torch.int32, device="cuda")]),
                               torch.cat([part[1], torch.full((B - g,), 7.0, device="cuda")]), part[2], part[3], part[4])
                assert torch.equal(acc[0], out[0]) and torch.equal(acc[1], out[1]), f"{what}: groups change a row's outputs"
                check_totals(z[:, :C], ref, acc, K, C, metric, what + " accumulated")
    print(f"C {C} metric {metric}: worst sums error / bound {worst:.3g}; {inside} of {rows} rows inside the score margin")


@pytest.mark.parametrize("metric", [0, 1], ids=["euclidean", "cosine"])
def test_walkers_own_several_row_tiles(metric):
    B, C = 16384 + 32 * 512 + 45, 8                  # more than two row tiles per walker, and a ragged last one
    for K in (10, 70):
        z, ld_z, W, ld_w, b = _case(B, C, K, torch.float32, metric, 5 + K)
        _check_call(z, ld_z, B, C, W, ld_w, b, K, metric, f"B {B} K {K}")


@pytest.mark.parametrize("metric", [0, 1], ids=["euclidean", "cosine"])
def test_ties_go_to_the_lowest_index_on_both_paths(metric):
    for C, B, dtype in ((8, 1000, torch.float32), (512, 333, torch.float16)):
        z, ld_z, W, ld_w, b = _case(B, C, 10, dtype, metric, 90 + C)
        one = kmeans_pass(z, ld_z, B, C, W, b, 10, ld_w, metric)
        # K = 10 padded to 40 with copies: the two-kernel path must answer with the bits of the one-kernel path
        W40, b40 = W.repeat(4, 1).contiguous(), b.repeat(4).contiguous()
        two = kmeans_pass(z, ld_z, B, C, W40, b40, 40, ld_w, metric)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
        assert torch.equal(two[2][:10], one[2]) and bool((two[2][10:, :C] == 0).all())
        assert torch.equal(two[3][:10], one[3]) and bool((two[3][10:] == 0).all()) and torch.equal(one[4], two[4])
        # duplicates inside one tile, and K = 70 whose second half copies the first
        W20, b20 = W.repeat(2, 1).contiguous(), b.repeat(2).contiguous()
        dup = kmeans_pass(z, ld_z, B, C, W20, b20, 20, ld_w, metric)
        assert torch.equal(dup[0], one[0]) and torch.equal(dup[1], one[1])
        z7, _, W35, _, b35 = _case(B, C, 35, dtype, metric, 91 + C)
        half = kmeans_pass(z7, ld_z, B, C, W35, b35, 35, ld_w, metric)
        full = kmeans_pass(z7, ld_z, B, C, W35.repeat(2, 1).contiguous(), b35.repeat(2).contiguous(), 70, ld_w, metric)
        assert int(full[0].max()) < 35 and torch.equal(full[0], half[0]) and torch.equal(full[1], half[1])


def test_no_rows():
    C, K = 16, 5
    _, ld_z, W, ld_w, b = _case(4, C, K, torch.float32, 0, 3)
    z = torch.zeros((1, ld_z), device="cuda")
    out = kmeans_pass(z, ld_z, 0, C, W, b, K, ld_w, 0)                  # zeroed
    assert bool((out[2][:, :C] == 0).all()) and bool((out[3] == 0).all()) and bool((out[4] == 0).all())
    assert int(out[0][0]) == -7 and float(out[1][0]) == 7.0
    kept = kmeans_pass(z, ld_z, 0, C, W, b, K, ld_w, 0, accumulate=1)   # untouched
    assert bool((kept[2] == 7.0).all()) and bool((kept[3] == 7.0).all()) and bool((kept[4] == 7.0).all())
    for K2 in (5, 40):
        _, _, W2, _, b2 = _case(4, C, K2, torch.float32, 0, 4)
        none = kmeans_pass(z, ld_z, 0, C, W2, b2, K2, ld_w, 0, sums=False)
        assert bool((none[2] == 7.0).all()) and bool((none[3] == 7.0).all()) and bool((none[4] == 7.0).all())


# ------------------------------------------------------------------ end to end
N_E2E, N_CLASSES = 1500, 6
# (K, seed) of the comparison with the twin: chosen on the CPU, with the twin alone (kmeans_util.twin_margins), so that at
# most 1 % of the rows lie inside the margin bound at any of the twin's iterations and no cluster runs empty -- seed 4 at
# K = 6: no row at all; seed 0 at K = 40: one row of 1500.  test_against_the_twin asserts the condition again.
TWIN_CASES = ((6, 4), (40, 0))


@pytest.fixture(scope="module")
def dataset():
    import hubconf
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    tab = load_tables("5e-02")
    sym = class_symbols(tab, N_E2E, N_CLASSES, seed=41)
    with tempfile.TemporaryDirectory() as d:
        file = os.path.join(d, "z.bin")
        container.write_container(file, [cbind.rans_encode(s, tab["cdf"], tab["cdf_len"], tab["offset"]) for s in sym])
        ds = comp.open_dataset(file)
    rows = torch.from_numpy(eb.dequantise(sym, tab))
    assert np.array_equal(ds.all().cpu().numpy(), rows.numpy())
    return ds, rows, torch.arange(N_E2E) % N_CLASSES


def _fixed_point(probe, rows, metric):
    """The fitted state against float64 on the decompressed rows: labels, inertia and (converged at tol = 0) the centres."""
    m = 1 if metric == "cosine" else 0
    c = probe.cluster_centers_.cpu()
    b = torch.zeros(len(c)) if m else (-0.5 * (c.double() ** 2).sum(1)).float()
    ref = scores_and_bound(rows, c, b, m)
    a = probe.labels_.cpu()
    inside = check_assignment(ref, a, "labels_")
    assert inside <= 0.01 * len(rows)
    d64, Ed = dist_and_bound(ref, a, m)
    assert abs(probe.inertia_ - float(d64.sum())) <= float(Ed.sum()) + 1e-12 * float(d64.sum())
    if probe.converged_ and m == 0:
        mean = torch.zeros_like(c, dtype=torch.float64).index_add_(0, a, rows.double())
        cnt = torch.bincount(a, minlength=len(c)).double()
        assert bool((cnt > 0).all())
        err = (c.double() - mean / cnt[:, None]).abs()
        assert bool((err <= centre_bound(rows, a, c)).all()), "a centre is not the mean of its members"


@pytest.mark.parametrize("K,seed", TWIN_CASES)
def test_against_the_twin(dataset, K, seed):
    from lossyless_amd import KMeansProbe
    from lossyless_amd.probe import _Rows, _kmeans_init
    ds, rows, y = dataset
    init = _kmeans_init(_Rows(rows, 1 << 30, False), K, False, "k-means++", seed, None)
    labels, n_iter, worst, emptied = twin_margins(rows, init)
    assert worst <= 0.01 and not emptied, f"the chosen seed no longer satisfies the margin condition: {worst}, {emptied}"
    twin = KMeansProbe(K, seed=seed, tol=0).fit(rows)
    assert torch.equal(twin.labels_, labels) and twin.n_iter_ == n_iter
    gpu = KMeansProbe(K, seed=seed, tol=0).fit(ds)
    assert gpu.cluster_centers_.is_cuda and gpu.cluster_centers_.dtype == torch.float32 and gpu.labels_.dtype == torch.int64
    assert torch.equal(gpu.labels_.cpu(), twin.labels_) and gpu.n_iter_ == twin.n_iter_ and gpu.converged_
    assert gpu.cluster_scores(y)["purity"] == twin.cluster_scores(y)["purity"]
    assert gpu.n_passes_ == gpu.n_iter_ + 1 and len(gpu.inertia_curve_) == gpu.n_iter_
    _fixed_point(gpu, rows, "euclidean")
    assert torch.equal(gpu.predict(ds, rows_per_pass=400).cpu(), twin.labels_)


@pytest.mark.parametrize("K,seed", TWIN_CASES)
def test_streamed_resident_kept_and_repeated(dataset, K, seed):
    from lossyless_amd import KMeansProbe
    ds, rows, _ = dataset
    base = KMeansProbe(K, seed=seed, tol=0).fit(ds, rows_per_pass=400)
    kept = KMeansProbe(K, seed=seed, tol=0).fit(ds, rows_per_pass=400, keep_rows=True)
    again = KMeansProbe(K, seed=seed, tol=0).fit(ds, rows_per_pass=400)
    resident = KMeansProbe(K, seed=seed, tol=0).fit(ds)
    tensor = KMeansProbe(K, seed=seed, tol=0).fit(rows.cuda(), rows_per_pass=400)
    for other in (kept, again, tensor):
        assert torch.equal(other.cluster_centers_, base.cluster_centers_) and torch.equal(other.labels_, base.labels_)
        assert other.inertia_ == base.inertia_ and other.n_iter_ == base.n_iter_
    assert torch.equal(resident.labels_, base.labels_) and resident.n_iter_ == base.n_iter_
    half = KMeansProbe(K, seed=seed, tol=0).fit(rows.half().cuda(), rows_per_pass=400)      # fp16 rows: other data, same walk
    _fixed_point(half, rows.half().float(), "euclidean")


def test_from_hyperprior_latents():
    from hyperprior_latents_util import hyper_model
    from lossyless_amd import HyperpriorLatents, KMeansProbe
    model = hyper_model()
    n = 600
    g = torch.Generator().manual_seed(3)
    means = torch.randn(N_CLASSES, 512, generator=g) * 0.5
    z = (means[torch.arange(n) % N_CLASSES] + torch.randn(n, 512, generator=g) * 0.7).cuda()
    z_strings, side_strings = model.compress(z)
    owner = types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()), hyperprior=model)
    with tempfile.TemporaryDirectory() as d:
        file = os.path.join(d, "z.bin")
        container.write_container(file, [s for pair in zip(z_strings, side_strings) for s in pair])
        ds = HyperpriorLatents(file, owner)
    rows = ds.all()
    a = KMeansProbe(N_CLASSES, seed=1).fit(ds, rows_per_pass=256)
    b = KMeansProbe(N_CLASSES, seed=1).fit(rows, rows_per_pass=256)
    assert torch.equal(a.cluster_centers_, b.cluster_centers_) and torch.equal(a.labels_, b.labels_) and a.inertia_ == b.inertia_
    _fixed_point(a, rows.cpu(), "euclidean")


def test_cosine_metric(dataset):
    from lossyless_amd import KMeansProbe
    ds, rows, y = dataset
    probe = KMeansProbe(N_CLASSES, metric="cosine", seed=4, tol=0).fit(ds, rows_per_pass=512)
    # every centre is a float64 unit vector rounded to fp32: its norm is within u of 1 (and the float64 norm's own rounding)
    norms = probe.cluster_centers_.double().norm(dim=1)
    assert float((norms - 1).abs().max()) <= 1.01 * U
    _fixed_point(probe, rows, "cosine")
    assert probe.cluster_scores(y)["purity"] > 0.5
    # rows scaled by positive constants keep their labels wherever the margin exceeds the bound (powers of two: everywhere)
    g = torch.Generator().manual_seed(2)
    for scale in (2.0 ** torch.randint(-3, 4, (N_E2E, 1), generator=g).float(), torch.rand(N_E2E, 1, generator=g) * 4 + 0.25):
        scaled = rows * scale
        pred = probe.predict(scaled.cuda()).cpu()
        c = probe.cluster_centers_.cpu()
        ref = scores_and_bound(scaled, c, torch.zeros(len(c)), 1)
        inside = margin_inside(ref["s"], 2 * ref["Es"].amax(1))
        assert int(inside.sum()) <= 0.01 * N_E2E and torch.equal(pred[~inside], probe.labels_.cpu()[~inside])
    assert torch.equal(probe.predict(rows.cuda() * 4.0), probe.labels_)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_transform(dataset, metric):
    """Against float64, within the bound of its fp32 evaluation: s^ from lla_gemm_f32 (Es of scores_and_bound with the dot's
    gamma_{C+2}; metric 1: b = 0 and the scale applied by torch, the same two roundings), n2 a sum of rounded squares in some
    order (En), then   euclidean: fl(n2^ - 2 s^) clamped, as dist_and_bound; its root: |sqrt(x^) - sqrt(x)| <= sqrt(|x^ - x|),
    + SQRT_U u of rounding;   cosine: fl(1 - t^)."""
    from knn_util import SQRT_U
    from lossyless_amd import KMeansProbe
    ds, rows, _ = dataset
    K = 40
    probe = KMeansProbe(K, metric=metric, seed=0, max_iter=3, tol=0, init="random")
    with pytest.warns(RuntimeWarning):
        probe.fit(ds)
    got = probe.transform(ds, rows_per_pass=700)
    assert tuple(got.shape) == (N_E2E, K) and got.dtype == torch.float32 and got.is_cuda
    m = 1 if metric == "cosine" else 0
    c = probe.cluster_centers_.cpu()
    b = torch.zeros(K) if m else (-0.5 * (c.double() ** 2).sum(1)).float()
    ref = scores_and_bound(rows, c, b, m)
    s, Es = ref["s"], ref["Es"]
    if not m:                                    # (wherever the GEMM adds its bias: probe_util.reference_and_bound)
        Es = gamma(rows.shape[1] + 2) * (rows.double().abs() @ c.double().abs().T + b.double().abs())
    if m:
        want, lim = 1.0 - s, Es + U * (1 + s.abs() + Es)
    else:
        x = (ref["n2"][:, None] - 2 * s).clamp_min(0.0)
        Ex = ref["En"][:, None] + 2 * Es + U * (ref["n2"][:, None] + ref["En"][:, None] + 2 * s.abs() + 2 * Es)
        want = torch.sqrt(x)
        lim = torch.sqrt(Ex) + SQRT_U * U * (want + torch.sqrt(Ex))
    err = (got.double().cpu() - want).abs()
    assert bool((err <= lim).all()), f"transform error / bound = {float((err / lim).max()):.3g}"
