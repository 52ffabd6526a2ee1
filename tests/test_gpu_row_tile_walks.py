"""GPU: the walk of csrc/row_tile.h where a persistent workgroup (a "walker") owns SEVERAL row tiles, and the width classes no
other test launches -- ``lla_svm_pass``, ``lla_svm_grid_pass``, ``lla_softmax_pass`` (with ``softmax_rows_kernel``),
``lla_softmax_grid_pass``, ``lla_knn_pass`` + ``lla_knn_finish`` and ``lla_kmeans_pass`` against float64, every comparison
held to the bound the ``*_util.py`` helpers derive (no tolerance of this module's own).

The launch arithmetic (row_tile.h, probe.hip, knn.hip; ``_walk`` below repeats it and every case asserts what it claims):
a pass over B rows and K columns has ceil(B / 32) row tiles and ceil(K / 32) column tiles; tile_walkers = max(512 / column
tiles, 1) walkers per column tile (kResident = 512), for kNN at most kWalkersMax = 64; walker p takes the row tiles p, p + P,
...  softmax_rows_kernel has min(row tiles, 512) workgroups whatever K is.

  K = 513, B = 1957      17 column tiles -> 30 walkers; 62 row tiles = 2 * 30 + 2: walkers 0 and 1 run the loop three times,
                         the rest twice; the last tile has 1957 - 61 * 32 = 5 rows
  K = 10, B = 32813      one column tile -> 512 walkers; 1026 row tiles = 2 * 512 + 2: three and two; 13 rows in the last
  K = 70, B = 32813      three column tiles -> 170 walkers of six or seven tiles; softmax_rows_kernel's 512 workgroups own
                         two or three
  K = 16416, B = 70      513 column tiles -> 512 / 513 = 0 walkers, clamped to ONE, which owns all three row tiles
  softmax grid           K = 3, G = 170: ten groups a tile -> 17 tiles -> 30 walkers (B = 1957: as the first line), two dead
                         columns in every tile; K = 10, G = 3: one tile -> 512 walkers (B = 32813: as the second line)
  kNN Q = 33, n = 4141   two query tiles -> 256 walkers, capped to 64; 130 row tiles = 2 * 64 + 2; 13 rows in the last
  kNN Q = 2049, n = 493  65 query tiles -> 7 walkers; 16 row tiles = 2 * 7 + 2; 13 rows in the last

The widths: C <= 128 runs NT = 1 / NG = 4 (C = 128 is its top, C = 8 its bottom: one column group, so waves 1 to 3 add
empty score tiles to the ordered merge), 128 < C <= 256 runs NT = 2 / NG = 8 (C = 136: clamped columns in the second
32-column tile of a wave; C = 256: none)."""
import numpy as np
import pytest
import torch

import kmeans_util
from knn_util import check_lists, knn_search, scores_and_bound, votes64
from logistic_cv_util import grid_reference_and_bound as softmax_grid_reference_and_bound, softmax_grid_pass
from logistic_util import softmax_pass, softmax_reference_and_bound
from probe_cv_util import grid_pass, grid_reference_and_bound, signs_and_weights
from probe_util import reference_and_bound, signs, svm_pass

pytestmark = pytest.mark.gpu

NCLS = 7                             # classes of the kNN votes
F32, F16 = torch.float32, torch.float16


def _walk(rows, columns, per_tile=32, cap=None, resident=False):
    """The launchers' arithmetic -> (walkers, row tiles, the most tiles a walker owns, rows of the last tile).
    ``per_tile``: live columns of a column tile; ``cap``: kWalkersMax; ``resident``: a grid of min(row tiles, 512)."""
    ntiles = -(-rows // 32)
    walkers = 512 if resident else max(512 // -(-columns // per_tile), 1)
    walkers = min(walkers, cap or walkers, ntiles)
    return walkers, ntiles, -(-ntiles // walkers), rows - 32 * (ntiles - 1)


def test_the_shapes_reach_what_the_docstring_says():
    assert _walk(1957, 513) == (30, 62, 3, 5) and 62 - 2 * 30 == 2
    assert _walk(32813, 10) == (512, 1026, 3, 13) and 1026 - 2 * 512 == 2
    assert _walk(32813, 70) == (170, 1026, 7, 13) and _walk(32813, 70, resident=True) == (512, 1026, 3, 13)
    assert 512 // 513 == 0 and _walk(70, 16416) == (1, 3, 3, 6)
    assert _walk(1957, 3 * 170, per_tile=30) == (30, 62, 3, 5) and _walk(32813, 10 * 3, per_tile=30) == (512, 1026, 3, 13)
    assert _walk(4141, 33, cap=64) == (64, 130, 3, 13) and _walk(493, 2049, cap=64) == (7, 16, 3, 13)
    assert _walk(257, 37)[2] == 1 and _walk(1000, 65, cap=64)[2] == 1          # (the other modules' largest: one tile each)


# ------------------------------------------------------------------ cases (as the other modules' _case helpers draw them)
def _rows(B, C, dtype, g, pad=8, values=None):
    """Rows with pitch C + pad, the padding poisoned -> (flat storage on the device, pitch)."""
    flat = torch.full((B, C + pad), float("nan"))
    flat[:, :C] = torch.randn(B, C, generator=g) if values is None else values
    return flat.to(dtype).cuda(), C + pad


def _linear(K, C, g):
    """W, b, V, vb for K columns."""
    return ((torch.randn(K, C, generator=g) * (0.7 / C ** 0.5)).cuda(), (torch.randn(K, generator=g) * 0.3).cuda(),
            torch.randn(K, C, generator=g).cuda(), torch.randn(K, generator=g).cuda())


def _weights(g, *shape):
    return (1e-3 + (1.0 - 1e-3) * torch.rand(*shape, generator=g)).cuda()


def _labels(B, K, g):
    """Labels drawn from [-1, K]: both ends are no class."""
    return torch.randint(-1, K + 1, (B,), generator=g).to(torch.int32).cuda()


def _hinge(B, C, K, dtype, seed):
    """-> (run(V, vb, lo, hi, out, accumulate), ref(V, vb), V, vb) of ``lla_svm_pass`` on one seeded case."""
    g = torch.Generator().manual_seed(seed)
    flat, ld = _rows(B, C, dtype, g)
    y = _labels(B, K, g)
    W, b, V, vb = _linear(K, C, g)

    def run(Vm, vbm, lo=0, hi=B, out=None, accumulate=0):
        return svm_pass(flat[lo:hi], ld, y[lo:hi], hi - lo, C, W, b, Vm, vbm, K, out=out, accumulate=accumulate)
    return run, lambda Vm, vbm: reference_and_bound(flat[:, :C], y, W, b, Vm, vbm), V, vb


def _softmax(B, C, K, dtype, seed, weights=True):
    g = torch.Generator().manual_seed(seed)
    flat, ld = _rows(B, C, dtype, g)
    y = _labels(B, K, g)
    W, b, V, vb = _linear(K, C, g)
    cw = _weights(g, K) if weights else None

    def run(Vm, vbm, lo=0, hi=B, out=None, accumulate=0):
        return softmax_pass(flat[lo:hi], ld, y[lo:hi], hi - lo, C, W, b, Vm, vbm, K, cw, out=out, accumulate=accumulate)
    return run, lambda Vm, vbm: softmax_reference_and_bound(flat[:, :C], y, W, b, Vm, vbm, cw), V, vb


def _hinge_grid(B, C, J, dtype, seed, n_labels=5):
    """Labels from [-1, n_labels + 1], the columns' classes from [0, n_labels) with repeats, three folds, held-out folds
    from {-1, 0, 1, 2}, two weights per column from [1e-3, 1] (test_gpu_probe_cv.py)."""
    g = torch.Generator().manual_seed(seed)
    flat, ld = _rows(B, C, dtype, g)
    y = torch.randint(-1, n_labels + 2, (B,), generator=g).to(torch.int32).cuda()
    fold = torch.randint(0, 3, (B,), generator=g).to(torch.int32).cuda()
    cols = (torch.randint(0, n_labels, (J,), generator=g).to(torch.int32).cuda(),
            torch.randint(-1, 3, (J,), generator=g).to(torch.int32).cuda(), _weights(g, J), _weights(g, J))
    W, b, V, vb = _linear(J, C, g)

    def run(Vm, vbm, lo=0, hi=B, out=None, accumulate=0):
        return grid_pass(flat[lo:hi], ld, y[lo:hi], fold[lo:hi], hi - lo, C, W, b, Vm, vbm, cols, out=out, accumulate=accumulate)
    return run, lambda Vm, vbm: grid_reference_and_bound(flat[:, :C], y, fold, W, b, cols, Vm, vbm), V, vb


def _softmax_grid(B, C, K, G, dtype, seed):
    """Three folds, groups that hold out fold 0, 1, 2 or none, class weights from [1e-3, 1] (test_gpu_logistic_probe_cv.py)."""
    g = torch.Generator().manual_seed(seed)
    flat, ld = _rows(B, C, dtype, g)
    y = _labels(B, K, g)
    fold = torch.randint(0, 3, (B,), generator=g).to(torch.int32).cuda()
    held = torch.tensor([(j % 4) - 1 for j in range(1, G + 1)], dtype=torch.int32).cuda()
    W, b, V, vb = _linear(G * K, C, g)
    cw = _weights(g, G, K)

    def run(Vm, vbm, lo=0, hi=B, out=None, accumulate=0):
        return softmax_grid_pass(flat[lo:hi], ld, y[lo:hi], fold[lo:hi], hi - lo, C, W, b, Vm, vbm, K, G, held, cw, out=out,
                                 accumulate=accumulate)
    return run, lambda Vm, vbm: softmax_grid_reference_and_bound(flat[:, :C], y, fold, W, b, K, G, held, cw, Vm, vbm), V, vb


def _check(got, val, bound, what):
    """-> the largest error / bound over the outputs (out_loss is not looked at in Hessian-vector mode)."""
    worst = 0.0
    for key, g in zip(("W", "b", "loss"), got):
        if val[key] is None:
            continue
        assert bool(torch.isfinite(g).all()), f"{what} out_{key} is not finite"
        err, lim = (g.double() - val[key]).abs(), bound[key]
        ratio = float((err / lim.clamp_min(1e-300)).max())
        assert bool((err <= lim).all()), f"{what} out_{key}: error / bound = {ratio:.3g}"
        worst = max(worst, ratio)
    return worst


def _three_properties(case, B, cut, what):
    """Both modes: within the bound of float64; a second call gives the same bits; two accumulated calls split at row ``cut``
    stay within the bound of the whole (two partial totals and one more addition: the bound allows B + 8).
    -> the largest error / bound."""
    run, ref, V, vb = case
    assert 0 < cut < B and cut % 32
    worst = 0.0
    for Vm, vbm in ((None, None), (V, vb)):
        mode = f"{what} {'hv' if Vm is not None else 'grad'}"
        val, bound = ref(Vm, vbm)
        got = run(Vm, vbm)
        worst = max(worst, _check(got, val, bound, mode))
        assert float(val["W"].abs().max()) > 0
        if Vm is not None:
            assert bool((got[2] == 7.0).all())                    # out_loss is not touched in Hessian-vector mode
        again = run(Vm, vbm)
        assert all(torch.equal(p, q) for p, q in zip(got, again)), f"{mode}: two calls differ"
        out = run(Vm, vbm, 0, cut)
        out = run(Vm, vbm, cut, B, out=out, accumulate=1)
        worst = max(worst, _check(out, val, bound, mode + f" accumulated over rows [0, {cut}) and [{cut}, {B})"))
    return worst


# ------------------------------------------------------------------ 1. several row tiles per walker
# (K, B, C, dtype, the row the accumulated calls are split at: the second call still gives some walker two tiles)
WALKS = [(513, 1957, 40, F32, 37), (513, 1957, 136, F16, 37), (10, 32813, 8, F32, 45), (16416, 70, 8, F32, 5)]
WALK_IDS = ["K513-B1957-C40-f32", "K513-B1957-C136-f16", "K10-B32813-C8-f32", "K16416-B70-C8-f32"]


@pytest.mark.parametrize("K,B,C,dtype,cut", WALKS, ids=WALK_IDS)
def test_hinge_pass_over_several_row_tiles(K, B, C, dtype, cut):
    assert _walk(B, K)[2] == 3 and _walk(B - cut, K)[2] >= 2
    worst = _three_properties(_hinge(B, C, K, dtype, 1000 + K), B, cut, f"hinge K {K} B {B} C {C}")
    print(f"lla_svm_pass K {K} B {B} C {C} {dtype}: largest error / bound = {worst:.3g}")


@pytest.mark.parametrize("K,B,C,dtype,cut", WALKS + [(70, 32813, 8, F32, 45)], ids=WALK_IDS + ["K70-B32813-C8-f32"])
def test_softmax_pass_over_several_row_tiles(K, B, C, dtype, cut):
    assert _walk(B, K)[2] >= 3 and _walk(B - cut, K)[2] >= 2
    if K == 70:
        assert _walk(B, K, resident=True)[2] == 3 and _walk(B - cut, K, resident=True)[2] == 2      # softmax_rows_kernel
    worst = _three_properties(_softmax(B, C, K, dtype, 2000 + K), B, cut, f"softmax K {K} B {B} C {C}")
    print(f"lla_softmax_pass K {K} B {B} C {C} {dtype}: largest error / bound = {worst:.3g}")


def test_hinge_grid_pass_over_several_row_tiles():
    J, B, C, cut = 513, 1957, 40, 37
    assert _walk(B, J)[2] == 3 and _walk(B - cut, J)[2] == 2
    worst = _three_properties(_hinge_grid(B, C, J, F32, 3000), B, cut, f"hinge grid J {J} B {B} C {C}")
    print(f"lla_svm_grid_pass J {J} B {B} C {C}: largest error / bound = {worst:.3g}")


@pytest.mark.parametrize("K,G,B,C,cut", [(3, 170, 1957, 40, 37), (10, 3, 32813, 8, 45)],
                         ids=["K3-G170-B1957-C40", "K10-G3-B32813-C8"])
def test_softmax_grid_pass_over_several_row_tiles(K, G, B, C, cut):
    live = (32 // K) * K
    assert live < 32 and _walk(B, G * K, per_tile=live)[2] == 3 and _walk(B - cut, G * K, per_tile=live)[2] == 2
    worst = _three_properties(_softmax_grid(B, C, K, G, F32, 4000 + K), B, cut, f"softmax grid K {K} G {G} B {B} C {C}")
    print(f"lla_softmax_grid_pass K {K} G {G} B {B} C {C}: largest error / bound = {worst:.3g}")


def _knn_case(Q, n, C, dtype, metric, seed, pad=8):
    """Rows with pitch C + pad and queries with pitch C + 4 (the padding poisoned), labels from [-1, NCLS], and for odd seeds
    one train index per query to skip (-1: none) (test_gpu_knn_probe.py)."""
    g = torch.Generator().manual_seed(seed)
    z, ld_z = _rows(n, C, dtype, g, pad)
    qv = torch.randn(Q, C, generator=g)
    q, ld_q = _rows(Q, C, F32, g, 4, values=qv / qv.norm(dim=1, keepdim=True) if metric == 1 else qv)
    y = _labels(n, NCLS, g)
    q_self = torch.randint(-1, n, (Q,), generator=g).to(torch.int32).cuda() if seed % 2 else None
    inv_T = float(np.float32(1 / 0.07 if metric == 1 else 1 / C ** 0.5))
    return z, ld_z, q, ld_q, y, q_self, inv_T


def _knn_properties(Q, n, C, dtype, metric, ks, seed, splits):
    """Every k: the list properties and the votes against float64; a second call and every split of the rows in ``splits``
    give the bits of the single call.  -> the largest (score, votes) error / bound."""
    z, ld_z, q, ld_q, y, q_self, inv_T = _knn_case(Q, n, C, dtype, metric, seed)
    s, E = scores_and_bound(q[:, :C], z[:, :C], metric)
    worst, worst_v = 0.0, 0.0
    for k in ks:
        what = f"Q {Q} n {n} C {C} k {k}"
        args = (q, ld_q, Q, z, ld_z, n, C, k, metric)
        one = knn_search(*args, q_self=q_self, labels=y, K=NCLS, inv_T=inv_T)
        worst = max(worst, check_lists(one[0], one[1], s, E, k, n, q_self, what))
        want, lim = votes64(one[0], one[1], y, NCLS, inv_T)
        err = (one[2].double().cpu() - want).abs()
        ratio = float((err / lim.clamp_min(1e-300)).max())
        assert bool((err <= lim).all()), f"{what}: votes error / bound = {ratio:.3g}"
        worst_v = max(worst_v, ratio)
        for groups in (None,) + tuple(splits):
            other = knn_search(*args, q_self=q_self, groups=groups, labels=y, K=NCLS, inv_T=inv_T)
            assert all(torch.equal(a, b) for a, b in zip(one, other)), f"{what}: groups of {groups} differ"
    return worst, worst_v


@pytest.mark.parametrize("metric", [0, 1], ids=["dot", "cosine"])
@pytest.mark.parametrize("Q,n", [(33, 4141), (2049, 493)], ids=["Q33-n4141", "Q2049-n493"])
def test_knn_lists_carried_over_several_row_tiles(Q, n, metric):
    """Walkers 0 and 1 carry their lists over three tiles; groups of 64 rows leave most walkers with nothing to add to the
    lists of the call before (the early return), groups of 2049 cut the rows of the first shape off a tile's edge."""
    assert _walk(n, Q, cap=64)[2] == 3 and 2049 % 32 and _walk(64, Q, cap=64)[0] == 2
    worst, worst_v = _knn_properties(Q, n, 40, F32, metric, (5, 200), 5000 + Q + metric, (64, 2049))
    print(f"lla_knn_pass Q {Q} n {n} C 40 metric {metric}: largest score error / bound {worst:.3g}, votes {worst_v:.3g}")


# ------------------------------------------------------------------ 2. an exact case
def _dyadic(B, C, K, seed):
    """Inputs whose every score, margin, residual, partial sum and loss is a small multiple of a power of two: integer rows
    in [-2, 2], W in {-1/4, 0, 1/4}, V in {-1/2 .. 1/2} and b, vb in {-1 .. 1} in steps of 1/4, weights in {1/4, 1/2, 1, 2}."""
    g = torch.Generator().manual_seed(seed)
    quarter = lambda lo, hi, *shape: (torch.randint(lo, hi + 1, shape, generator=g).float() / 4).cuda()      # noqa: E731
    flat, ld = _rows(B, C, F32, g, values=torch.randint(-2, 3, (B, C), generator=g).float())
    y = _labels(B, K, g)
    W, b, V, vb = quarter(-1, 1, K, C), quarter(-4, 4, K), quarter(-2, 2, K, C), quarter(-4, 4, K)
    fold = torch.randint(0, 3, (B,), generator=g).to(torch.int32).cuda()
    power = lambda: (2.0 ** torch.randint(-2, 2, (K,), generator=g).float()).cuda()                         # noqa: E731
    cols = (torch.randint(0, K, (K,), generator=g).to(torch.int32).cuda(),
            torch.randint(-1, 3, (K,), generator=g).to(torch.int32).cuda(), power(), power())
    return flat, ld, y, fold, cols, W, b, V, vb


def _assert_exact_in_fp32(Z, Y, c, W, b, V, vb):
    """The precondition, from the float64 side: every term of every sum is an integer multiple of its unit (a power of two)
    and sum |term| / unit < 2^24 -- so every partial sum, in any order, is an integer below 2^24 times the unit: an fp32
    number.  c [B, K] are the weights (ones for ``lla_svm_pass``), cmin their smallest."""
    whole = lambda t, unit: bool((t / unit == (t / unit).round()).all())       # noqa: E731
    Z, W, b, V, vb = Z.double(), W.double(), b.double(), V.double(), vb.double()
    cmin = float(c[c > 0].min())
    assert whole(Z, 1.0) and whole(W, 0.25) and whole(b, 0.25) and whole(V, 0.25) and whole(vb, 0.25)
    assert whole(torch.log2(c[c > 0]), 1.0) and cmin == 2.0 ** round(np.log2(cmin))
    limit = 2.0 ** 24
    assert float((Z.abs() @ W.abs().T + b.abs()).max()) / 0.25 < limit          # scores
    assert float((Z.abs() @ V.abs().T + vb.abs()).max()) / 0.25 < limit         # tangents
    s, t = Z @ W.T + b, Z @ V.T + vb
    m = (1.0 - Y * s).clamp_min(0.0)
    assert whole(m, 0.25)
    for R, unit in ((c * (-2.0 * Y * m), 0.5 * cmin), (c * 2.0 * torch.where(m > 0, t, torch.zeros_like(t)), 0.5 * cmin)):
        assert whole(R, unit)
        assert float((R.abs().T @ Z.abs()).max()) / unit < limit and float(R.abs().sum(0).max()) / unit < limit
    assert whole(c * m * m, cmin / 16) and float((c * m * m).sum(0).max()) / (cmin / 16) < limit
    assert float(m.max()) ** 2 * 16 < limit                                     # m * m itself, before the weight


def _assert_equal(got, val, what):
    for key, g in zip(("W", "b", "loss"), got):
        if val[key] is not None:
            assert float(val[key].abs().max()) > 0
            wrong = int((g.double() != val[key]).sum())
            assert torch.equal(g.double(), val[key]), f"{what} out_{key}: {wrong} of {g.numel()} entries differ from float64"


def test_dyadic_inputs_give_exactly_the_float64_sums():
    """A bound grows with B; here nothing is rounded, so a tile that is dropped, doubled or summed into the wrong walker's
    slice changes the result and fails ``torch.equal``: K = 513, B = 1957, C = 40, walkers of three and of two tiles."""
    K, B, C = 513, 1957, 40
    assert _walk(B, K) == (30, 62, 3, 5)
    flat, ld, y, fold, cols, W, b, V, vb = _dyadic(B, C, K, 77)
    Z = flat[:, :C]
    ones = torch.ones((B, K), dtype=torch.float64, device="cuda")
    _assert_exact_in_fp32(Z, signs(y.to(torch.int64), K), ones, W, b, V, vb)
    Yg, cg = signs_and_weights(y, fold, cols)
    assert 0 < int((cg == 0).sum()) < cg.numel()
    _assert_exact_in_fp32(Z, Yg, cg, W, b, V, vb)
    for Vm, vbm in ((None, None), (V, vb)):
        mode = "hv" if Vm is not None else "grad"
        val, _ = reference_and_bound(Z, y, W, b, Vm, vbm)
        _assert_equal(svm_pass(flat, ld, y, B, C, W, b, Vm, vbm, K), val, f"lla_svm_pass {mode}")
        val, _ = grid_reference_and_bound(Z, y, fold, W, b, cols, Vm, vbm)
        _assert_equal(grid_pass(flat, ld, y, fold, B, C, W, b, Vm, vbm, cols), val, f"lla_svm_grid_pass {mode}")


# ------------------------------------------------------------------ 3. the width classes
WIDTHS = [136, 256, 128, 8]          # NT = 2 / NG = 8 with and without clamped columns; the top of NT = 1; one column group
DTYPES = pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])


def _grid_of(make, what, dtype, C, columns):
    """B in {33, 257} x ``columns``, both modes (``_three_properties`` with the cut at row 13) -> prints the worst."""
    worst, seed = 0.0, 0
    for B in (33, 257):
        for cols in columns:
            seed += 1
            args = cols if isinstance(cols, tuple) else (cols,)
            worst = max(worst, _three_properties(make(B, C, *args, dtype, 100 * C + seed), B, 13, f"{what} B {B} C {C} {args}"))
    print(f"{what} C {C} {dtype}: largest error / bound = {worst:.3g}")


@DTYPES
@pytest.mark.parametrize("C", WIDTHS)
def test_hinge_pass_at_the_other_widths(C, dtype):
    _grid_of(_hinge, "lla_svm_pass", dtype, C, (3, 37))


@DTYPES
@pytest.mark.parametrize("C", WIDTHS)
def test_softmax_pass_at_the_other_widths(C, dtype):
    _grid_of(_softmax, "lla_softmax_pass", dtype, C, (3, 37))


@DTYPES
@pytest.mark.parametrize("C", WIDTHS)
def test_hinge_grid_pass_at_the_other_widths(C, dtype):
    _grid_of(_hinge_grid, "lla_svm_grid_pass", dtype, C, (3, 37))


@DTYPES
@pytest.mark.parametrize("C", WIDTHS)
def test_softmax_grid_pass_at_the_other_widths(C, dtype):
    """A group has at most 32 classes, so the 3 and 37 of the other passes are the classes of a group and the number of
    groups: (K, G) = (3, 3), one tile with 23 dead columns, and (3, 37), four tiles of ten groups, the last with seven."""
    _grid_of(_softmax_grid, "lla_softmax_grid_pass", dtype, C, ((3, 3), (3, 37)))


@pytest.mark.parametrize("metric", [0, 1], ids=["dot", "cosine"])
@DTYPES
@pytest.mark.parametrize("C", WIDTHS)
def test_knn_at_the_other_widths(C, dtype, metric):
    worst, worst_v, seed = 0.0, 0.0, 0
    for Q in (1, 33):
        for n in (31, 257):
            seed += 1
            w, v = _knn_properties(Q, n, C, dtype, metric, (5, 32), 100 * C + 10 * metric + seed, (64,))
            worst, worst_v = max(worst, w), max(worst_v, v)
    print(f"lla_knn_pass C {C} {dtype} metric {metric}: largest score error / bound {worst:.3g}, votes {worst_v:.3g}")


def _kmeans_case(B, C, K, dtype, metric, seed, pad_z=8, pad_w=4):
    """Rows around K centroids and centroids with pitch C + pad_w (the padding poisoned), a row of zeros; metric 0:
    b = -1/2 |c|^2 rounded once, metric 1: unit centroids and, for odd seeds, a small b (test_gpu_kmeans_probe.py)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(K, C, generator=g)
    if metric == 1:
        c = c / c.norm(dim=1, keepdim=True)
    W, ld_w = _rows(K, C, F32, g, pad_w, values=c)
    zv = c[torch.randint(0, K, (B,), generator=g)] * (1.0 if metric == 0 else 3.0) + 0.7 * torch.randn(B, C, generator=g)
    zv[2] = 0.0
    z, ld_z = _rows(B, C, dtype, g, pad_z, values=zv)
    if metric == 0:
        b = (-0.5 * (c.double() ** 2).sum(1)).float()
    else:
        b = 0.01 * torch.randn(K, generator=g) if seed % 2 else torch.zeros(K)
    return z, ld_z, W, ld_w, b.cuda()


@pytest.mark.parametrize("metric", [0, 1], ids=["euclidean", "cosine"])
@DTYPES
@pytest.mark.parametrize("C", [136, 256, 128])
def test_kmeans_at_the_other_widths(C, dtype, metric):
    """Both paths (K = 10: one kernel; K = 33: the assign kernel and the sums walk): assignment, distances, sums at the device's
    own assignment, counts and statistics against float64; a second call the same bits; predict-only the same rows' outputs."""
    worst, seed = 0.0, 0
    for K in (10, 33):
        for B in (33, 1000):
            seed += 1
            what = f"C {C} K {K} B {B}"
            z, ld_z, W, ld_w, b = _kmeans_case(B, C, K, dtype, metric, 100 * C + 10 * metric + seed)
            out = kmeans_util.kmeans_pass(z, ld_z, B, C, W, b, K, ld_w, metric)
            ref = kmeans_util.scores_and_bound(z[:, :C], W[:, :C], b, metric)
            a = out[0].to(torch.int64)
            kmeans_util.check_assignment(ref, a, what)
            d64, Ed = kmeans_util.dist_and_bound(ref, a, metric)
            err = (out[1].double() - d64).abs()
            assert bool((err <= Ed).all()), f"{what}: dist error / bound = {float((err / Ed.clamp_min(1e-300)).max()):.3g}"
            worst = max(worst, kmeans_util.check_totals(z[:, :C], ref, out, K, C, metric, what))
            assert bool((out[2][:, C:] == 7.0).all()), f"{what}: the padding of out_sum was written"
            again = kmeans_util.kmeans_pass(z, ld_z, B, C, W, b, K, ld_w, metric)
            assert all(torch.equal(p, q) for p, q in zip(out, again)), f"{what}: two calls differ"
            pred = kmeans_util.kmeans_pass(z, ld_z, B, C, W, b, K, ld_w, metric, sums=False)
            assert torch.equal(pred[0], out[0]) and torch.equal(pred[1], out[1]), f"{what}: predict-only differs"
    print(f"lla_kmeans_pass C {C} {dtype} metric {metric}: largest sums error / bound = {worst:.3g}")
