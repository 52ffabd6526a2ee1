"""GPU: ``lla_gram_pass`` and ``lla_segment_sums`` against float64 moments of the same values, held to the bounds derived in
ridge_util -- symmetry and repeatability bit for bit, fp16 rows against their widened copy, accumulation, B = 0 -- and
``RidgeProbe`` / ``RidgeProbeCV`` from device rows and from containers that stay compressed against the float64 twin."""
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from conftest import load_tables
from oracle import cbind, container, eb
from probe_cv_util import class_symbols
from ridge_util import (U64, check_moments, f32_moments_coefficient_error, f32_moments_cv_mse_error, gram_pass, make_ridge_data,
                        moments_and_bounds, segment_sums)

pytestmark = pytest.mark.gpu

BS = (1, 31, 33, 200)


def _rows(B, C, dtype, seed, pad=8, T=0, pad_t=1):
    """Rows with pitch C + pad and targets with pitch T + pad_t (the padding poisoned), asymmetric in the columns."""
    g = torch.Generator().manual_seed(seed)
    z = torch.full((B, C + pad), float("nan"))
    z[:, :C] = torch.randn(B, C, generator=g) * (1.0 + torch.arange(C) % 5) + 0.25
    t = None
    if T:
        t = torch.full((B, T + pad_t), float("nan"))
        t[:, :T] = torch.randn(B, T, generator=g) * 2.0 - 0.5
        t = t.cuda()
    return z.to(dtype).cuda(), t


@pytest.mark.parametrize("C", [8, 24, 136, 520, 1024])
def test_gram_pass_against_float64(C):
    seed, worst = 0, 0.0
    for B in BS:
        for T, dtype in ((0, torch.float32), (0, torch.float16), (3, torch.float32), (3, torch.float16), (35, torch.float32),
                         (35, torch.float16)):
            seed += 1
            z, t = _rows(B, C, dtype, 100 * C + seed, T=T)
            ld_z, ld_t = C + 8, T + 1
            what = f"C {C} B {B} T {T} {dtype}"
            out = gram_pass(z, ld_z, B, C, t, ld_t, T)
            ref = moments_and_bounds(z[:, :C], t[:, :T] if T else None)
            worst = max(worst, check_moments(out, ref, C, T, what))
            assert torch.equal(out[0], out[0].T), f"{what}: out_gram is not symmetric bit for bit"
            if not T:
                assert all(bool((o == 7.0).all()) for o in out[2:]), f"{what}: target outputs touched without targets"
            again = gram_pass(z, ld_z, B, C, t, ld_t, T)
            assert all(torch.equal(p, q) for p, q in zip(out, again)), f"{what}: two calls differ"
            if dtype == torch.float16:                       # the widened copy, another pitch: the same bits
                wide = torch.full((B, C + 4), float("nan"), device="cuda")
                wide[:, :C] = z[:, :C].float()
                same = gram_pass(wide, C + 4, B, C, t, ld_t, T)
                assert all(torch.equal(p, q) for p, q in zip(out, same)), f"{what}: fp16 rows differ from their fp32 copy"
            if B > 33:                                       # two calls accumulated: within the sum of both bounds
                cut = 77
                acc = gram_pass(z[:cut], ld_z, cut, C, t[:cut] if T else None, ld_t, T)
                acc = gram_pass(z[cut:], ld_z, B - cut, C, t[cut:] if T else None, ld_t, T, out=acc, accumulate=1)
                lo = moments_and_bounds(z[:cut, :C], t[:cut, :T] if T else None)
                hi = moments_and_bounds(z[cut:, :C], t[cut:, :T] if T else None)
                both = {k: (lo[k][0] + hi[k][0], lo[k][1] + hi[k][1]) for k in lo}
                check_moments(acc, both, C, T, what + " accumulated")
                assert torch.equal(acc[0], acc[0].T)
    print(f"C {C}: worst Gram error / bound {worst:.3g}")


def test_walkers_own_several_chunks():
    """C = 8 is one tile and 512 walkers (T = 3: two tiles, 256): more than two chunks each and a ragged last chunk."""
    B, C = 2 * 512 * 32 + 45, 8
    for T in (0, 3):
        z, t = _rows(B, C, torch.float32, 7 + T, T=T)
        out = gram_pass(z, C + 8, B, C, t, T + 1, T)
        check_moments(out, moments_and_bounds(z[:, :C], t[:, :T] if T else None), C, T, f"B {B} T {T}")
        assert torch.equal(out[0], out[0].T)


def test_no_rows():
    C, T = 24, 3
    z, t = _rows(4, C, torch.float32, 3, T=T)
    out = gram_pass(z, C + 8, 0, C, t, T + 1, T)                       # zeroed
    assert all(bool((o[:T] == 0).all()) for o in out[2:]) and bool((out[0] == 0).all()) and bool((out[1] == 0).all())
    kept = gram_pass(z, C + 8, 0, C, t, T + 1, T, accumulate=1)        # untouched
    assert all(bool((o == 7.0).all()) for o in kept)
    none = gram_pass(z, C + 8, 0, C)
    assert bool((none[0] == 0).all()) and bool((none[1] == 0).all()) and all(bool((o == 7.0).all()) for o in none[2:])
    seg = segment_sums(z, C + 8, 0, C, [0, 0, 0])
    assert bool((seg == 0).all()) and bool((segment_sums(z, C + 8, 0, C, [0, 0, 0], accumulate=1) == 7.0).all())


@pytest.mark.parametrize("C", [8, 136, 1024])
def test_segment_sums_against_float64(C):
    """Empty, one-row and ragged segments; more than 256 segments (two launches); fp16 rows; accumulation."""
    B = 700
    for dtype, offsets in ((torch.float32, [0, 0, 1, 1, 9, 300, 300, 683, B]), (torch.float16, [0, B]),
                           (torch.float32, sorted(np.random.default_rng(C).integers(0, B + 1, 299).tolist() + [0, B]))):
        z, _ = _rows(B, C, dtype, C + len(offsets))
        out = segment_sums(z, C + 8, B, C, offsets)
        Z = z[:, :C].double()
        for s, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
            want, mass = Z[a:b].sum(0), Z[a:b].abs().sum(0)
            assert bool(((out[s] - want).abs() <= (b - a + 2) * U64 * mass).all()), f"C {C} segment {s} [{a}, {b})"
        assert torch.equal(out, segment_sums(z, C + 8, B, C, offsets))
        twice = segment_sums(z, C + 8, B, C, offsets, out=out.clone(), accumulate=1)
        assert torch.equal(twice, out + out)


# ------------------------------------------------------------------ end to end
N_E2E, N_CLASSES, N_TARGETS = 1500, 6, 3
ALPHAS = (1e-2, 1.0, 100.0)


@pytest.fixture(scope="module")
def dataset():
    import hubconf
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    tab = load_tables("5e-02")
    sym = class_symbols(tab, N_E2E, N_CLASSES, seed=41)
    y = np.arange(N_E2E) % N_CLASSES
    with tempfile.TemporaryDirectory() as d:
        file, lf = os.path.join(d, "z.bin"), os.path.join(d, "y.npy")
        container.write_container(file, [cbind.rans_encode(s, tab["cdf"], tab["cdf_len"], tab["offset"]) for s in sym])
        np.save(lf, y)
        ds = comp.open_dataset(file, label_file=lf)
    rows = torch.from_numpy(eb.dequantise(sym, tab))
    assert np.array_equal(ds.all().cpu().numpy(), rows.numpy())
    g = torch.Generator().manual_seed(9)
    A = torch.randn(rows.shape[1], N_TARGETS, generator=g, dtype=torch.float64) / rows.shape[1] ** 0.5
    t = (rows.double() @ A + 0.3 * torch.randn(N_E2E, N_TARGETS, generator=g, dtype=torch.float64)).float()
    return ds, rows, torch.from_numpy(y), t


@pytest.fixture(scope="module")
def tolerance(dataset):
    """4 x the coefficient error that fp32 accumulation of the moments causes in the twin's solver, measured on the CPU
    (ridge_util.f32_moments_coefficient_error) -> {kind: absolute coefficient tolerance}."""
    _, rows, y, t = dataset
    measured = {"classify": f32_moments_coefficient_error(rows, y, ALPHAS, True),
                "regress": f32_moments_coefficient_error(rows, t, ALPHAS, False)}
    print(f"measured fp32-moments coefficient error: {measured}")
    return {k: 4.0 * v for k, v in measured.items()}


def _inside(scores, rows, tol):
    """Rows whose float64 top-two score gap does not exceed the tolerance times the row's L1 norm."""
    top = scores.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) <= tol * rows.double().abs().sum(1)


def test_solver_is_the_twins(dataset):
    """The device's moments through the twin's solver: isolates the solver from the kernel (1e-12; ``RidgeProbe`` runs that
    very solver, so this pins the wiring).  What carries the weight is ``moments_`` against float64: a chain is never longer
    than the 400 rows of a group, groups are joined in double, class sums and the other sums are double throughout, and the
    class counts are exact."""
    from lossyless_amd import RidgeProbe
    from lossyless_amd.probe import _ridge_solve, _signed_targets
    _, rows, y, t = dataset
    Z, A = rows.double(), rows.double().abs()
    g32, g64 = (400 + 2) * 2.0 ** -24, (N_E2E + 2) * U64
    for target in (y, t):
        p = RidgeProbe(0.5).fit(rows.cuda(), target, rows_per_pass=400)
        m = p.moments_
        assert m["gram"].dtype == torch.float64 and not m["gram"].is_cuda and torch.equal(m["gram"], m["gram"].T)
        R, ts = _signed_targets(m["n"], m["sum"], m["cross"], m["tsum"]) if target is y else (m["cross"], m["tsum"])
        W, b = _ridge_solve(m["n"], m["gram"], m["sum"], R, ts, [0.5])
        assert float((p.coef_ - W[0]).abs().max()) <= 1e-12 * float(W.abs().max())
        assert float((p.intercept_ - b[0]).abs().max()) <= 1e-12
        assert m["n"] == N_E2E and bool(((m["gram"] - Z.T @ Z).abs() <= g32 * (A.T @ A)).all())
        assert bool(((m["sum"] - Z.sum(0)).abs() <= g64 * A.sum(0)).all())
        if target is y:
            onehot = torch.nn.functional.one_hot(y, N_CLASSES).double()
            assert bool(((m["cross"] - onehot.T @ Z).abs() <= g64 * (onehot.T @ A)).all())
            assert torch.equal(m["tsum"], onehot.sum(0)) and bool((m["tsq"] == N_E2E).all())
        else:
            T64 = t.double()
            assert bool(((m["cross"] - T64.T @ Z).abs() <= g32 * (T64.abs().T @ A)).all())
            assert bool(((m["tsum"] - T64.sum(0)).abs() <= g64 * T64.abs().sum(0)).all())
            assert bool(((m["tsq"] - (T64 * T64).sum(0)).abs() <= g64 * (T64 * T64).sum(0)).all())


def test_end_to_end_against_the_twin(dataset, tolerance):
    """Device fit against the float64 twin on the same fp32 rows.  Tolerance: 4 x the measured effect of fp32-accumulated
    moments on the twin's coefficients (max |W32 - W64| over alphas 1e-2, 1, 100 on these 1500 x 512 rows; measured on the
    CPU: 6.8e-05 for the classifier's +-1 targets, 4.6e-05 for the three regression targets, against coefficients of up to
    5.8e-02 and 1.8e-01: 1500 rows for 512 columns leave the centred Gram matrix ill-conditioned at the small alphas).  Predictions agree wherever the twin's top-two gap exceeds the tolerance times the row's L1 norm."""
    from lossyless_amd import RidgeProbe
    ds, rows, y, t = dataset
    mu1 = float(rows.double().mean(0).abs().sum())
    for alpha in ALPHAS:
        twin, gpu = RidgeProbe(alpha).fit(rows, y), RidgeProbe(alpha).fit(ds, rows_per_pass=400)
        tol = tolerance["classify"]
        err = float((gpu.coef_ - twin.coef_).abs().max())
        print(f"alpha {alpha}: classifier coefficient error {err:.3g} (tolerance {tol:.3g})")
        assert err <= tol and float((gpu.intercept_ - twin.intercept_).abs().max()) <= tol * (mu1 + 1)
        inside = _inside(twin.decision_function(rows), rows, tol)
        assert int(inside.sum()) <= 0.01 * N_E2E
        pred = gpu.predict(ds, rows_per_pass=700).cpu()
        assert torch.equal(pred[~inside], twin.predict(rows)[~inside]) and np.array_equal(gpu.classes_, twin.classes_)
        twin, gpu = RidgeProbe(alpha).fit(rows, t), RidgeProbe(alpha).fit(ds, t, rows_per_pass=400)
        tol = tolerance["regress"]
        err = float((gpu.coef_ - twin.coef_).abs().max())
        print(f"alpha {alpha}: regression coefficient error {err:.3g} (tolerance {tol:.3g})")
        assert err <= tol and float((gpu.intercept_ - twin.intercept_).abs().max()) <= tol * (mu1 + 1)
        assert abs(gpu.score(ds, t) - twin.score(rows, t)) <= 1e-5            # (fp32 predictions)


def test_containers_resident_kept_and_repeated(dataset):
    from lossyless_amd import RidgeProbe, RidgeProbeCV
    ds, rows, y, t = dataset
    for target in (None, t):
        base = RidgeProbe(1.0).fit(ds, target, rows_per_pass=400)
        others = [RidgeProbe(1.0).fit(ds, target, rows_per_pass=400, keep_rows=True), RidgeProbe(1.0).fit(ds, target, rows_per_pass=400),
                  RidgeProbe(1.0).fit(ds.all(), y if target is None else t, rows_per_pass=400)]
        for other in others:
            assert all(torch.equal(other.moments_[k], base.moments_[k]) for k in ("gram", "sum", "cross", "tsum", "tsq"))
            assert torch.equal(other.coef_, base.coef_) and torch.equal(other.intercept_, base.intercept_)
        cv = [RidgeProbeCV(ALPHAS, cv=3).fit(ds, target, rows_per_pass=400, keep_rows=k) for k in (False, True)]
        cv.append(RidgeProbeCV(ALPHAS, cv=3).fit(ds.all(), y if target is None else t, rows_per_pass=400))
        for other in cv[1:]:
            assert torch.equal(other.cv_scores_, cv[0].cv_scores_) and torch.equal(other.best_estimator_.coef_, cv[0].best_estimator_.coef_)
    half = RidgeProbe(1.0).fit(rows.half().cuda(), y, rows_per_pass=400)     # fp16 rows: other data, the same walk
    wide = RidgeProbe(1.0).fit(rows.half().float().cuda(), y, rows_per_pass=400)
    assert torch.equal(half.coef_, wide.coef_)


def test_from_hyperprior_latents():
    from hyperprior_latents_util import hyper_model
    from lossyless_amd import HyperpriorLatents, RidgeProbe
    model = hyper_model()
    n = 600
    g = torch.Generator().manual_seed(3)
    means = torch.randn(N_CLASSES, 512, generator=g) * 0.5
    y = torch.arange(n) % N_CLASSES
    z = (means[y] + torch.randn(n, 512, generator=g) * 0.7).cuda()
    z_strings, side_strings = model.compress(z)
    owner = types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()), hyperprior=model)
    with tempfile.TemporaryDirectory() as d:
        file = os.path.join(d, "z.bin")
        container.write_container(file, [s for pair in zip(z_strings, side_strings) for s in pair])
        ds = HyperpriorLatents(file, owner)
    a = RidgeProbe(1.0).fit(ds, y, rows_per_pass=256)
    b = RidgeProbe(1.0).fit(ds.all(), y, rows_per_pass=256)
    c = RidgeProbe(1.0).fit(ds, y, rows_per_pass=256, keep_rows=True)
    assert torch.equal(a.coef_, b.coef_) and torch.equal(a.coef_, c.coef_) and torch.equal(a.intercept_, b.intercept_)
    assert a.score(ds, y) > 0.9


def test_cv_on_the_device(dataset, tolerance, monkeypatch):
    from lossyless_amd import RidgeProbeCV
    from lossyless_amd.probe import _Rows
    ds, rows, y, t = dataset
    walks = []
    groups = _Rows.groups

    def counted(self):
        walks.append(1)
        return groups(self)

    monkeypatch.setattr(_Rows, "groups", counted)
    fold = torch.from_numpy(np.random.default_rng(8).integers(0, 4, N_E2E))
    gpu = RidgeProbeCV(ALPHAS, cv=fold).fit(ds, rows_per_pass=400)
    assert len(walks) == 2 and gpu.n_passes_ == 2
    del walks[:]
    reg = RidgeProbeCV(ALPHAS, cv=fold).fit(ds, t, rows_per_pass=400)
    assert len(walks) == 1 and reg.n_passes_ == 1
    monkeypatch.undo()
    twin, twin_reg = RidgeProbeCV(ALPHAS, cv=fold).fit(rows, y), RidgeProbeCV(ALPHAS, cv=fold).fit(rows, t)
    # accuracy counts: equal to the twin's up to the rows of the fold inside the margin; at most 1 % of the rows are
    tol, excluded = tolerance["classify"], 0
    for a in range(len(ALPHAS)):
        for f in range(4):
            held = fold == f
            s = rows[held].double() @ twin.fold_coef_[a, f].T + twin.fold_intercept_[a, f]
            inside = int(_inside(s, rows[held], tol).sum())
            excluded = max(excluded, inside)
            n = int(held.sum())
            assert abs(round(float(gpu.cv_scores_[a, f]) * n) - round(float(twin.cv_scores_[a, f]) * n)) <= inside, (a, f)
    assert excluded <= 0.01 * N_E2E
    assert gpu.best_params_ == twin.best_params_
    # negative MSE: within 4 x what numpy-fp32 per-fold moments do to the twin's closed form (measured on the CPU on this
    # fixture: 1.4e-06 absolute on held-out MSEs of 0.12 .. 0.18; the centred 512 x 512 matrix of 1100 rows is ill-conditioned)
    tol_mse = 4.0 * f32_moments_cv_mse_error(rows, t, fold, ALPHAS)
    err = float((reg.cv_scores_ - twin_reg.cv_scores_).abs().max())
    print(f"container: held-out MSE error {err:.3g} (tolerance {tol_mse:.3g})")
    assert err <= tol_mse
    assert reg.best_params_ == twin_reg.best_params_
    assert float((reg.best_estimator_.coef_ - twin_reg.best_estimator_.coef_).abs().max()) <= tolerance["regress"]


# ------------------------------------------------------------------ overlapping classes: what the scoring walk gets wrong shows
N_OV, C_OV, K_OV = 1500, 72, 5
ALPHAS_OV = (1e-2, 30.0, 1e3)
# seed and class separation chosen on the CPU, with the twin alone: held-out accuracies of 0.65 .. 0.74 that differ across
# alphas and folds, and at most 1 row of any fold inside the margin (the tests assert the 1 % condition again)
OV_SEED, OV_SEP = 1, 0.2


@pytest.fixture(scope="module")
def overlap():
    X, y, T = make_ridge_data(N_OV, C_OV, K_OV, N_TARGETS, OV_SEED, sep=OV_SEP)
    fold = torch.from_numpy(np.random.default_rng(8).integers(0, 4, N_OV))
    fold[:40] = -1                                              # rows that always train and are never scored
    tol = 4.0 * f32_moments_coefficient_error(X, y, ALPHAS_OV, True)
    return X, y * 3 - 4, T, fold, tol                           # (labels that are not their own class index)


def test_predictions_on_overlapping_classes(overlap):
    """Device predictions against the twin's where the classes overlap (training accuracy about 0.76): equal on every row whose
    float64 top-two gap exceeds the tolerance (4 x the measured fp32-moments coefficient error, 1.2e-07 on this 1500 x 72
    fixture) times the row's L1 norm; at most 1 % of the rows are excluded."""
    from lossyless_amd import RidgeProbe
    X, y, _, _, tol = overlap
    for alpha in ALPHAS_OV:
        twin, gpu = RidgeProbe(alpha).fit(X, y), RidgeProbe(alpha).fit(X.cuda(), y, rows_per_pass=400)
        assert float((gpu.coef_ - twin.coef_).abs().max()) <= tol
        inside = _inside(twin.decision_function(X), X, tol)
        assert int(inside.sum()) <= 0.01 * N_OV
        want = twin.predict(X)
        assert 0.5 < float((want == y).double().mean()) < 0.9, "the fixture no longer overlaps"
        assert torch.equal(gpu.predict(X.cuda(), rows_per_pass=700).cpu()[~inside], want[~inside])


def test_cv_scoring_walk_on_overlapping_classes(overlap, monkeypatch):
    """The scoring walk against the twin where a wrong fold, alpha or column would change the counts: held-out accuracies of
    0.65 .. 0.74 that differ across alphas and folds, rows with fold id -1, 15 columns padded to 16, and scores taken in
    pieces of 64 rows (``_SCORE_ELEMS`` lowered: a run of a 400-row group is scored in two or more pieces)."""
    import lossyless_amd.probe as probe
    from lossyless_amd import RidgeProbeCV
    X, y, _, fold, tol = overlap
    twin = RidgeProbeCV(ALPHAS_OV, cv=fold).fit(X, y)
    assert len({round(float(v), 6) for v in twin.cv_scores_.reshape(-1)}) >= 8 and float(twin.cv_scores_.max()) < 0.9
    monkeypatch.setattr(probe, "_SCORE_ELEMS", 64 * 16)
    for kw in (dict(rows_per_pass=400), dict()):
        gpu = RidgeProbeCV(ALPHAS_OV, cv=fold).fit(X.cuda(), y, **kw)
        excluded = 0
        for a in range(len(ALPHAS_OV)):
            for f in range(4):
                held = fold == f
                s = X[held].double() @ twin.fold_coef_[a, f].T + twin.fold_intercept_[a, f]
                inside = int(_inside(s, X[held], tol).sum())
                excluded = max(excluded, inside)
                n = int(held.sum())
                got, want = round(float(gpu.cv_scores_[a, f]) * n), round(float(twin.cv_scores_[a, f]) * n)
                assert abs(got - want) <= inside, (a, f, got, want)
        assert excluded <= 0.01 * N_OV and gpu.best_params_ == twin.best_params_ and gpu.folds_ == [0, 1, 2, 3]
        assert np.array_equal(gpu.classes_, twin.classes_)


def test_cv_closed_form_mse_on_the_device(overlap):
    """The one-walk regression search.  (a) ``cv_scores_`` against the twin's within 4 x what numpy-fp32 per-fold moments do
    to the twin's closed form (ridge_util.f32_moments_cv_mse_error; measured on the CPU: 2.9e-07 absolute on MSEs of 0.09 ..
    0.34).  (b) the device's own fold coefficients applied to the held-out rows in float64 give, computed directly, the MSE its
    closed form reports, within the same tolerance: a wrong term or a moment in the wrong bucket moves it by far more."""
    from lossyless_amd import RidgeProbeCV
    X, _, T, fold, _ = overlap
    tol = 4.0 * f32_moments_cv_mse_error(X, T, fold, ALPHAS_OV)
    twin = RidgeProbeCV(ALPHAS_OV, cv=fold).fit(X, T)
    for kw in (dict(rows_per_pass=400), dict()):
        gpu = RidgeProbeCV(ALPHAS_OV, cv=fold).fit(X.cuda(), T, **kw)
        err = float((gpu.cv_scores_ - twin.cv_scores_).abs().max())
        worst = 0.0
        for a in range(len(ALPHAS_OV)):
            for f in range(4):
                held = fold == f
                pred = X[held].double() @ gpu.fold_coef_[a, f].T + gpu.fold_intercept_[a, f]
                worst = max(worst, abs(float(((pred - T[held].double()) ** 2).mean()) + float(gpu.cv_scores_[a, f])))
        print(f"{kw}: held-out MSE against the twin {err:.3g}, against the direct computation {worst:.3g} (tolerance {tol:.3g})")
        assert err <= tol and worst <= tol
        assert gpu.n_passes_ == 1 and gpu.best_params_ == twin.best_params_
        assert [m["n"] for m in gpu.fold_moments_] == [float((fold == f).sum()) for f in range(4)]
