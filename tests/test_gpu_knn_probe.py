"""GPU: ``lla_knn_pass`` + ``lla_knn_finish`` against float64 scores, held to the rounding bound derived in
knn_util.scores_and_bound -- range, uniqueness, order, completeness, votes -- their invariance under any split of the rows,
repeatability, tie order and refusals; and ``KNNProbe`` from containers that stay compressed on the device against its
float64 twin on the decompressed rows."""
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from conftest import load_tables
from knn_util import check_lists as _check_lists, knn_search, scores_and_bound, votes64
from oracle import cbind, container, eb
from probe_util import U

pytestmark = pytest.mark.gpu

QS, NS, KS = (1, 33, 65), (1, 31, 257, 1000), (1, 5, 32, 200, 256)
NCLS = 7


def _case(Q, n, C, dtype, metric, seed, pad=8):
    """Rows with pitch C + pad and queries with pitch C + 4 (the padding poisoned), labels drawn from [-1, NCLS] (both ends
    are no class) and, for odd seeds, one train index per query to skip (-1: none)."""
    g = torch.Generator().manual_seed(seed)
    ld_z, ld_q = C + pad, C + 4
    z = torch.full((n, ld_z), float("nan"))
    z[:, :C] = torch.randn(n, C, generator=g)
    z = z.to(dtype).cuda()
    q = torch.full((Q, ld_q), float("nan"))
    qv = torch.randn(Q, C, generator=g)
    q[:, :C] = qv / qv.norm(dim=1, keepdim=True) if metric == 1 else qv
    q = q.cuda()
    y = torch.randint(-1, NCLS + 1, (n,), generator=g).to(torch.int32).cuda()
    q_self = torch.randint(-1, n, (Q,), generator=g).to(torch.int32).cuda() if seed % 2 else None
    inv_T = float(np.float32(1 / 0.07 if metric == 1 else 1 / C ** 0.5))
    return z, ld_z, q, ld_q, y, q_self, inv_T


@pytest.mark.parametrize("metric", [0, 1], ids=["dot", "cosine"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("C", [40, 512, 1024])
def test_kernels_against_float64(C, dtype, metric):
    seed, worst, worst_v = 0, 0.0, 0.0
    for Q in QS:
        for n in NS:
            s = E = None
            for k in KS:
                seed += 1
                z, ld_z, q, ld_q, y, q_self, inv_T = _case(Q, n, C, dtype, metric, 1000 * C + seed)
                what = f"Q {Q} n {n} k {k}"
                s, E = scores_and_bound(q[:, :C], z[:, :C], metric)
                args = (q, ld_q, Q, z, ld_z, n, C, k, metric)
                one = knn_search(*args, q_self=q_self, labels=y, K=NCLS, inv_T=inv_T)
                worst = max(worst, _check_lists(one[0], one[1], s, E, k, n, q_self, what))
                # votes: float64 on the returned lists
                want, lim = votes64(one[0], one[1], y, NCLS, inv_T)
                err = (one[2].double().cpu() - want).abs()
                assert bool((err <= lim).all()), f"{what}: votes error / bound = {float((err / lim.clamp_min(1e-300)).max()):.3g}"
                worst_v = max(worst_v, float((err / lim.clamp_min(1e-300)).max()))
                # any split of the rows, and a second call: the same bits
                for groups in (None, 64, 257):
                    other = knn_search(*args, q_self=q_self, groups=groups, labels=y, K=NCLS, inv_T=inv_T)
                    assert all(torch.equal(a, b) for a, b in zip(one, other)), f"{what}: groups of {groups} differ"
                # the head of the lists is the search at a smaller k
                if k == 32:
                    head = knn_search(*args, q_self=q_self, k_out=5, labels=y, K=NCLS, inv_T=inv_T)
                    five = knn_search(q, ld_q, Q, z, ld_z, n, C, 5, metric, q_self=q_self, labels=y, K=NCLS, inv_T=inv_T)
                    assert all(torch.equal(a, b) for a, b in zip(head, five)), f"{what}: the head is not the top 5"
    print(f"C {C}: worst score error / bound {worst:.3g}, worst votes error / bound {worst_v:.3g}")


@pytest.mark.parametrize("metric", [0, 1], ids=["dot", "cosine"])
def test_duplicate_rows_come_out_lowest_index_first(metric):
    for C, n, Q, k, dtype in ((40, 130, 33, 32, torch.float32), (512, 500, 65, 200, torch.float16), (1024, 66, 5, 256, torch.float32)):
        z, ld_z, q, ld_q, _, _, _ = _case(Q, n, C, dtype, metric, 77 + C)
        z = z.repeat_interleave(2, dim=0).contiguous()                   # rows 2 i and 2 i + 1 are equal
        for groups in (None, 31):                                        # (31: the pairs straddle calls and tiles)
            val, idx, _ = knn_search(q, ld_q, Q, z, ld_z, 2 * n, C, k, metric, groups=groups)
            used = min(k, 2 * n) // 2 * 2
            lo, hi = idx[:, 0:used:2], idx[:, 1:used:2]
            assert bool((lo % 2 == 0).all()) and torch.equal(hi, lo + 1)
            assert torch.equal(val[:, 0:used:2], val[:, 1:used:2])


def test_base_offsets_the_indexes():
    Q, n, C, k = 33, 257, 40, 5
    z, ld_z, q, ld_q, _, _, _ = _case(Q, n, C, torch.float32, 1, 5)
    val, idx, _ = knn_search(q, ld_q, Q, z, ld_z, n, C, k, 1)
    val2, idx2, _ = knn_search(q, ld_q, Q, z, ld_z, n, C, k, 1, row_base=2 ** 31 - 1 - n, groups=100)
    assert torch.equal(val, val2) and torch.equal(idx.to(torch.int64) + (2 ** 31 - 1 - n), idx2.to(torch.int64))


def test_unsupported_arguments_are_refused_before_any_launch():
    from lossyless_amd import _lib
    L = _lib.lib()
    Q, n, k = 8, 40, 5
    ws = torch.full((int(L.lla_knn_pass_workspace_bytes(Q, 256)),), 0x5A, dtype=torch.uint8, device="cuda")
    z = torch.randn(n, 1040, device="cuda")
    q = torch.randn(Q, 1040, device="cuda")
    val = torch.full((Q, 256), 7.0, device="cuda")
    idx = torch.full((Q, 256), 7, dtype=torch.int32, device="cuda")
    votes = torch.full((Q, NCLS), 7.0, device="cuda")
    y = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = _lib.stream_ptr()

    def run_pass(C=40, k=k, metric=1, n=n, ld=1040, Q=Q):
        return L.lla_knn_pass(_lib.ptr(q), ld, Q, _lib.ptr(z), _lib.LLA_Z_F32, ld, n, C, 0, k, metric, None, 0, _lib.ptr(ws), st)

    for bad in (dict(C=12), dict(C=1032), dict(C=0), dict(k=0), dict(k=257), dict(metric=2), dict(metric=-1), dict(n=-1),
                dict(ld=32), dict(ld=1042), dict(Q=0)):
        assert run_pass(**bad) == _lib.LLA_EINVAL, bad
    assert run_pass(n=0) == 0                                            # no rows: no launch
    for kk, k_out in ((0, 1), (257, 5), (5, 0), (5, 6)):
        assert L.lla_knn_finish(Q, kk, k_out, _lib.ptr(y), NCLS, 1.0, _lib.ptr(val), _lib.ptr(idx), _lib.ptr(votes),
                                _lib.ptr(ws), st) == _lib.LLA_EINVAL, (kk, k_out)
    assert L.lla_knn_finish(Q, k, k, _lib.ptr(y), 0, 1.0, _lib.ptr(val), _lib.ptr(idx), _lib.ptr(votes), _lib.ptr(ws), st) \
        == _lib.LLA_EINVAL
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and bool((val == 7.0).all()) and bool((idx == 7).all()) and bool((votes == 7.0).all())


# ------------------------------------------------------------------ end to end
N_TRAIN, N_TEST, N_DRAWN, K_E2E = 400, 64, 256, 5


def _class_symbols(tab, n, n_classes, seed):
    """Symbols inside every channel's coding window whose mean depends on row % n_classes (test_gpu_logistic_probe.py)."""
    rng = np.random.default_rng(seed)
    C = tab["cdf"].shape[0]
    width = (tab["cdf_len"].astype(np.int64) - 2)[None, :]
    means = rng.normal(size=(n_classes, C)) * 1.5
    v = np.rint(width / 2 + means[np.arange(n) % n_classes] + rng.normal(size=(n, C)) * 1.5)
    return (tab["offset"][None, :] + np.clip(v, 0, width - 1)).astype(np.int32)


def _well_separated(train, drawn, labels):
    """The first N_TEST drawn rows whose k-NN lists the fp32 kernel cannot order differently from float64: every gap between
    consecutive scores of the float64 top K_E2E + 1 exceeds twice the bound (the queries' own rounding to fp32, u |q| . |z| / |z|,
    added to it), and the two leading classes' votes differ by more than 4e-3 of their sum: two scores off by at most 6.2e-5
    each (the bound's ceiling at C = 512, |cos| <= 1) move a weight exp((s - s0) / 0.07) by at most 1.8e-3 of itself, so the
    difference of two classes' votes by at most 1.8e-3 of the sum; twice that is asked for.  -> (their positions, the float64 twin fitted on the train rows)."""
    from lossyless_amd import KNNProbe
    twin = KNNProbe(k=K_E2E).fit(train, labels)
    qn = drawn.double() / drawn.double().norm(dim=1, keepdim=True)
    s, E = scores_and_bound(qn, train, 1)
    E = E + U * (qn.abs() @ train.double().abs().T) / train.double().norm(dim=1)[None, :]
    top, at = torch.sort(s, dim=1, descending=True, stable=True)
    gap = top[:, :K_E2E] - top[:, 1:K_E2E + 1]
    need = 2 * torch.gather(E, 1, at[:, :K_E2E + 1]).amax(1, keepdim=True)
    votes = twin._votes(drawn, None, None, 65536, 8192, False)
    lead = torch.sort(votes, dim=1, descending=True)[0]
    ok = (gap > need).all(1) & ((lead[:, 0] - lead[:, 1]) > 4e-3 * votes.sum(1))
    keep = torch.nonzero(ok)[:N_TEST, 0]
    assert keep.numel() == N_TEST, f"only {keep.numel()} of {N_DRAWN} drawn rows are well separated"
    # the property itself, for all the queries that are used
    assert bool((gap[keep] > need[keep]).all())
    return keep, twin


def _check_end_to_end(train_ds, test_ds, train_rows, test_rows, labels, test_labels, twin):
    from lossyless_amd import KNNProbe
    gpu = KNNProbe(k=K_E2E).fit(train_ds, labels)
    sim, idx = gpu.kneighbors(test_ds)
    want_sim, want_idx = twin.kneighbors(test_rows)
    assert sim.is_cuda and sim.dtype == torch.float32 and idx.dtype == torch.int64
    assert torch.equal(idx.cpu(), want_idx)
    assert float((sim.cpu().double() - want_sim).abs().max()) < 1e-4
    assert torch.equal(gpu.predict(test_ds).cpu(), twin.predict(test_rows))
    assert gpu.score(test_ds, test_labels) == twin.score(test_rows, test_labels)
    # one search for the grid, leave-one-out on the fitted rows
    ks, Ts = (1, 5, 20), (0.07, 0.5)
    grid = gpu.score_grid(None, ks, Ts, exclude_self=True)
    for (k, T), acc in grid.items():
        assert acc == gpu.score(None, k=k, T=T, exclude_self=True), (k, T)
    assert min(grid.values()) > 0.3                     # (six classes)
    # any blocking: the same bits
    base = gpu.kneighbors(test_ds, k=20)
    proba = gpu.predict_proba(test_ds, k=20)
    loo = gpu.kneighbors(None, k=20, exclude_self=True)
    assert not bool((loo[1] == torch.arange(N_TRAIN, device=loo[1].device)[:, None]).any())
    for rows_per_pass in (64, 257, N_TRAIN):
        for queries_per_pass in (32, 8192):
            kw = dict(rows_per_pass=rows_per_pass, queries_per_pass=queries_per_pass)
            assert all(torch.equal(a, b) for a, b in zip(base, gpu.kneighbors(test_ds, k=20, **kw))), kw
            assert torch.equal(proba, gpu.predict_proba(test_ds, k=20, **kw)), kw
            assert all(torch.equal(a, b) for a, b in zip(loo, gpu.kneighbors(None, k=20, exclude_self=True, **kw))), kw


def test_from_compressed_latents_on_the_device(tmp_path):
    import hubconf
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    tab = load_tables("5e-02")
    n_classes = 6
    sym = _class_symbols(tab, N_TRAIN, n_classes, seed=31)
    drawn = _class_symbols(tab, N_DRAWN, n_classes, seed=32)
    labels, drawn_labels = torch.arange(N_TRAIN) % n_classes, torch.arange(N_DRAWN) % n_classes
    keep, twin = _well_separated(torch.from_numpy(eb.dequantise(sym, tab)), torch.from_numpy(eb.dequantise(drawn, tab)), labels)
    files = []
    for name, rows in (("train", sym), ("test", drawn[keep.numpy()])):
        files.append(tmp_path / f"{name}.bin")
        container.write_container(str(files[-1]), [cbind.rans_encode(s, tab["cdf"], tab["cdf_len"], tab["offset"]) for s in rows])
    train_ds, test_ds = comp.open_dataset(files[0]), comp.open_dataset(files[1])
    train_rows, test_rows = train_ds.all().cpu(), test_ds.all().cpu()
    assert np.array_equal(train_rows.numpy(), eb.dequantise(sym, tab))
    _check_end_to_end(train_ds, test_ds, train_rows, test_rows, labels, drawn_labels[keep], twin)


def test_from_hyperprior_latents():
    from hyperprior_latents_util import hyper_model
    from lossyless_amd import HyperpriorLatents
    model = hyper_model()
    n_classes = 6
    g = torch.Generator().manual_seed(3)
    labels, drawn_labels = torch.arange(N_TRAIN) % n_classes, torch.arange(N_DRAWN) % n_classes
    means = torch.randn(n_classes, 512, generator=g) * 0.5
    z = (means[torch.cat([labels, drawn_labels])] + torch.randn(N_TRAIN + N_DRAWN, 512, generator=g) * 0.7).cuda()
    z_strings, side_strings = model.compress(z)
    pairs = list(zip(z_strings, side_strings))
    owner = types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()), hyperprior=model)

    def opened(chosen):
        with tempfile.TemporaryDirectory() as d:
            file = os.path.join(d, "z.bin")
            container.write_container(file, [s for pair in chosen for s in pair])
            return HyperpriorLatents(file, owner)

    train_ds = opened(pairs[:N_TRAIN])
    train_rows = train_ds.all().cpu()
    drawn_rows = opened(pairs[N_TRAIN:]).all().cpu()
    keep, twin = _well_separated(train_rows, drawn_rows, labels)
    test_ds = opened([pairs[N_TRAIN + int(i)] for i in keep])
    test_rows = test_ds.all().cpu()
    assert torch.equal(test_rows, drawn_rows[keep])
    _check_end_to_end(train_ds, test_ds, train_rows, test_rows, labels, drawn_labels[keep], twin)
