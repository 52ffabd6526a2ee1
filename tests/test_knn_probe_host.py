"""CPU: the k-NN entry points are declared, bound and exported; ``KNNProbe``'s float64 twin against a brute-force search, a
case whose neighbours, ties and votes are known on paper, ``score_grid`` against ``score``, the errors, and latents opened
on the CPU against their decompressed rows."""
import ctypes

import numpy as np
import pytest
import torch

import lossyless_amd
from knn_util import brute_force, scores_and_bound
from latents_util import write_dataset
from lossyless_amd import KNNProbe, _lib
from probe_util import make_data

NEW = ("lla_knn_pass_workspace_bytes", "lla_knn_pass", "lla_knn_finish")


def test_symbols_are_bound_and_exported():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert _lib.lib().lla_abi_version() == _lib.ABI_VERSION == 4
    assert "KNNProbe" in lossyless_amd.__all__ and lossyless_amd.KNNProbe is KNNProbe


def test_workspace_is_bounded_by_lists_not_by_rows():
    L = _lib.lib()
    for Q, k in ((1, 1), (33, 20), (8192, 200), (8192, 256)):
        nbytes = int(L.lla_knn_pass_workspace_bytes(Q, k))
        tiles = -(-Q // 32)
        assert 0 < nbytes <= max(tiles, 64) * 32 * k * 8 * 2 + 8, (Q, k, nbytes)
    assert all(int(L.lla_knn_pass_workspace_bytes(Q, k)) == 0 for Q, k in ((0, 5), (8, 0), (8, 257), (-1, 5)))


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_twin_against_brute_force(metric):
    N, C, K, k = 300, 40, 7, 9
    X, y = make_data(N, C, K, seed=5)
    Xq, _ = make_data(70, C, K, seed=6)
    probe = KNNProbe(k=k, metric=metric).fit(X, y)
    qn = Xq.double() / Xq.double().norm(dim=1, keepdim=True) if metric == "cosine" else Xq.double()
    s, _ = scores_and_bound(qn, X, 1 if metric == "cosine" else 0)
    want = brute_force(s, k)
    own, _ = scores_and_bound(X.double() / X.double().norm(dim=1, keepdim=True) if metric == "cosine" else X.double(), X,
                              1 if metric == "cosine" else 0)
    want_loo = brute_force(own, k, skip=np.arange(N))
    for rows_per_pass in (17, 64, 300):
        for queries_per_pass in (5, 300):
            kw = dict(rows_per_pass=rows_per_pass, queries_per_pass=queries_per_pass)
            sim, idx = probe.kneighbors(Xq, **kw)
            assert sim.dtype == torch.float64 and idx.dtype == torch.int64 and tuple(idx.shape) == (70, k)
            assert torch.equal(idx, want), kw
            assert float((sim - torch.gather(s, 1, want)).abs().max()) < 1e-13
            assert bool((sim[:, 1:] <= sim[:, :-1]).all())
            assert torch.equal(probe.kneighbors(None, exclude_self=True, **kw)[1], want_loo), kw
            if metric == "cosine":             # a row's best neighbour is itself
                assert torch.equal(probe.kneighbors(X, k=3, **kw)[1][:, 0], torch.arange(N))


def _one_hot(at, C=8):
    return torch.eye(C)[torch.as_tensor(at)]


def test_hand_made_neighbours_ties_and_votes():
    # rows 0, 1: e0 (class 5); rows 2, 3: e1 (class 2); row 4: e2 (class 9); row 5: e0 + e1 (class 9)
    X = torch.cat([_one_hot([0, 0, 1, 1, 2]), (_one_hot([0]) + _one_hot([1]))])
    y = torch.tensor([5, 5, 2, 2, 9, 9])
    probe = KNNProbe(k=4, T=0.5, metric="dot").fit(X, y)
    assert list(probe.classes_) == [2, 5, 9]
    q = torch.cat([_one_hot([0]), 2 * _one_hot([1]), _one_hot([0]) + _one_hot([2])])
    sim, idx = probe.kneighbors(q)
    # query e0: rows 0, 1, 5 score 1 (lowest index first), then the zeros from the lowest index on
    assert idx.tolist() == [[0, 1, 5, 2], [2, 3, 5, 0], [0, 1, 4, 5]]
    assert sim.tolist() == [[1, 1, 1, 0], [2, 2, 2, 0], [1, 1, 1, 1]]
    # votes of query e0 at T = 0.5: class 5: 1 + 1, class 9: 1, class 2: exp(-2)
    votes = probe.predict_proba(q) * torch.tensor([[3 + np.exp(-2.0)], [3 + np.exp(-4.0)], [4.0]])
    want = torch.tensor([[np.exp(-2.0), 2, 1], [2, np.exp(-4.0), 1], [0, 2, 2]], dtype=torch.float64)
    assert float((votes - want).abs().max()) < 1e-15
    assert probe.predict(q).tolist() == [5, 2, 5]                  # the tie of query 2 goes to the lower class index
    # uniform weights count: query e0 -> {5: 2, 9: 1, 2: 1}; cosine sees 2 e1 as e1 and row 5 at 1 / sqrt(2)
    uni = KNNProbe(k=4, metric="cosine", weights="uniform").fit(X, y)
    assert (uni.predict_proba(q) * 4).tolist() == [[1, 2, 1], [2, 1, 1], [0, 2, 2]]
    sim, idx = uni.kneighbors(q[1:2])
    assert idx.tolist() == [[2, 3, 5, 0]] and sim[0, :2].tolist() == [1, 1] and abs(float(sim[0, 2]) - 0.5 ** 0.5) < 1e-15
    # leave one out: row 0's neighbours start at its duplicate, row 4 (alone on e2) sees only zeros, lowest index first
    sim, idx = probe.kneighbors(None, k=3, exclude_self=True)
    assert idx[0].tolist() == [1, 5, 2] and idx[1].tolist() == [0, 5, 2] and idx[4].tolist() == [0, 1, 2]
    assert probe.predict(None, k=1, exclude_self=True).tolist() == [5, 5, 2, 2, 5, 5]
    assert probe.score(None, k=1, exclude_self=True) == 4 / 6 and probe.score(None, k=1) == 1.0
    assert probe.score(X, y, k=1) == 1.0


def test_score_grid_is_one_search_for_every_k_and_T():
    X, y = make_data(240, 24, 5, seed=3, sep=0.4)
    Xq, yq = make_data(90, 24, 5, seed=4, sep=0.4)
    probe = KNNProbe().fit(X, y)
    ks, Ts = (1, 3, 10, 40), (0.03, 0.07, 1.0)
    grid = probe.score_grid(Xq, ks, Ts, labels=yq, rows_per_pass=50)
    loo = probe.score_grid(None, ks, Ts, exclude_self=True, queries_per_pass=64)
    assert sorted(grid) == sorted((k, T) for k in ks for T in Ts) == sorted(loo)
    for (k, T), acc in grid.items():
        assert acc == KNNProbe(k=k, T=T).fit(X, y).score(Xq, yq) == probe.score(Xq, yq, k=k, T=T)
        assert loo[(k, T)] == probe.score(None, k=k, T=T, exclude_self=True)
    assert len(set(grid.values())) > 1


def test_errors():
    X, y = make_data(30, 16, 3, seed=1)
    with pytest.raises(RuntimeError, match="fit first"):
        KNNProbe().kneighbors(X)
    probe = KNNProbe(k=5).fit(X, y)
    with pytest.raises(ValueError):
        probe.kneighbors(X, k=31)
    with pytest.raises(ValueError):
        probe.kneighbors(None, k=30, exclude_self=True)          # 29 usable rows
    assert tuple(probe.kneighbors(None, k=29, exclude_self=True)[1].shape) == (30, 29)
    with pytest.raises(ValueError):
        probe.kneighbors(X[:, :8])
    with pytest.raises(ValueError):
        probe.kneighbors(X.clone(), exclude_self=True)           # not the fitted object
    with pytest.raises(TypeError):
        KNNProbe().fit(X, y.double())
    with pytest.raises(ValueError):
        KNNProbe().fit(X, y[:-1])
    with pytest.raises(ValueError):
        KNNProbe().fit(X).predict(X)                             # no labels: neighbours only
    assert tuple(KNNProbe(k=2).fit(X).kneighbors(X)[1].shape) == (30, 2)
    for bad in (dict(k=0), dict(T=0.0), dict(metric="l2"), dict(weights="rank")):
        with pytest.raises(ValueError):
            KNNProbe(**bad)


def test_compressed_latents_on_the_cpu(tmp_path):
    import hubconf
    comp, _ = hubconf.clip_compressor_b005(device="cpu", clip_weights="synthetic")
    N = 300
    file, lf, _ = write_dataset(tmp_path, "5e-02", N, seed=17)
    ds = comp.open_dataset(file, device="cpu")
    labels = torch.arange(N) % 3
    rows = ds.all()
    a, b = KNNProbe(k=7).fit(ds, labels), KNNProbe(k=7).fit(rows, labels)
    sim_a, idx_a = a.kneighbors(ds, rows_per_pass=128, queries_per_pass=50)
    sim_b, idx_b = b.kneighbors(rows)
    assert torch.equal(idx_a, idx_b) and float((sim_a - sim_b).abs().max()) < 1e-13
    assert torch.equal(idx_a[:, 0], torch.arange(N))
    assert torch.equal(a.kneighbors(None, exclude_self=True, rows_per_pass=77)[1], b.kneighbors(None, exclude_self=True)[1])
    assert a.score(None, exclude_self=True) == b.score(None, exclude_self=True)
    # the object's own labels are used when none are given
    own = KNNProbe(k=1).fit(comp.open_dataset(file, label_file=lf, device="cpu"))
    assert np.array_equal(own.classes_, np.arange(N)) and own.score() == 1.0
