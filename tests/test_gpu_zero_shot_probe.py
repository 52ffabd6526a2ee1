"""ZeroShotProbe on the device: class embeddings from tower A (K = 7, 3 templates, E = 64), 600 planted rows as a tensor, as
a ``CompressedLatents`` and as its kept rows; predictions against the float64 twin outside the propagated bound."""
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from conftest import load_tables
from latents_util import sub_tables
from oracle import cbind, container, eb
from text_tower_util import CASE_A, direct_logits, logit_bound, make_tokens, planted_rows, tower_case

pytestmark = pytest.mark.gpu

K, TEMPLATES, E, N, NOISE, MAX_EXCLUDED = 7, 3, 64, 600, 0.02, 0.02


class _Owner:
    """What ``CompressedLatents`` reads of a compressor: the device, the width and the tables (the first 64 channels of
    the shipped beta = 5e-2 rate point)."""

    def __init__(self, tab):
        self.device, self.z_dim, self.tab = torch.device("cuda"), E, tab

    def _tables(self):
        t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in self.tab.items()}
        t["W"] = int(self.tab["cdf"].shape[1])
        return t


@pytest.fixture(scope="module")
def case():
    from lossyless_amd import CompressedLatents, ZeroShotProbe
    from lossyless_amd.clip_text import TextTransformer
    tok = make_tokens(K * TEMPLATES, 77, CASE_A["vocab"], seed=6).reshape(K, TEMPLATES, 77)
    probe = ZeroShotProbe.from_tokens(TextTransformer(tower_case("A")[0]).to("cuda"), tok)
    assert tuple(probe.coef_.shape) == (K, E) and abs(probe.logit_scale - 1 / 0.07) < 1e-4
    tab = sub_tables(load_tables("5e-02"), E)
    planted, y = planted_rows(probe.coef_, N, NOISE, seed=2)
    # through the coder: the rows are what the container decodes to (the shipped rate point's grid, steps of ~0.19)
    sym = eb.symbols_of(planted.numpy(), tab)
    rows = torch.from_numpy(eb.dequantise(sym, tab))
    with tempfile.TemporaryDirectory() as d:
        file, lf = os.path.join(d, "z.bin"), os.path.join(d, "y.npy")
        container.write_container(file, [cbind.rans_encode(s, tab["cdf"], tab["cdf_len"], tab["offset"]) for s in sym])
        np.save(lf, y.numpy())
        ds = CompressedLatents(file, _Owner(tab), label_file=lf)
    assert np.array_equal(ds.all().cpu().numpy(), rows.numpy())
    want = direct_logits(rows, probe.coef_, probe.logit_scale)
    bound = logit_bound(E, probe.logit_scale, probe.coef_)
    return probe, ds, rows, y, want, bound


def test_the_twin_alone_decides_nearly_every_row(case):
    """Checked on the CPU arm before anything runs on the device: the rows whose float64 top-2 margin lies inside twice
    the bound (either logit may move by the bound) are the only ones excused, and they are at most 2 %."""
    probe, ds, rows, y, want, bound = case
    top = want.topk(2, dim=1).values
    excluded = float(((top[:, 0] - top[:, 1]) <= 2 * bound).double().mean())
    print(f"logit bound {bound:.3g}; rows inside the margin: {excluded:.4f}; twin accuracy "
          f"{float((want.argmax(1) == y).double().mean()):.3f}")
    assert excluded <= MAX_EXCLUDED
    twin = probe.decision_function(rows)                     # CPU rows: the float64 twin
    assert twin.dtype == torch.float64 and float((twin - want).abs().max()) <= 1e-9


def test_predictions_and_probabilities(case):
    probe, ds, rows, y, want, bound = case
    s = probe.decision_function(ds, rows_per_pass=256)
    assert s.is_cuda and s.dtype == torch.float32 and tuple(s.shape) == (N, K)
    err = float((s.double().cpu() - want).abs().max())
    print(f"logits: error {err:.3g} bound {bound:.3g}")
    assert err <= bound
    top = want.topk(2, dim=1).values
    decided = (top[:, 0] - top[:, 1]) > 2 * bound
    assert float((~decided).double().mean()) <= MAX_EXCLUDED
    pred = probe.predict(ds, rows_per_pass=256).cpu()
    assert torch.equal(pred[decided], want.argmax(1)[decided])
    # softmax: |dp_k| <= p_k (|ds_k| + sum_j p_j |ds_j|) <= 2 bound, plus the fp32 softmax's own roundings (K + 8 of 2^-24)
    p = probe.predict_proba(ds, rows_per_pass=256)
    perr = float((p.double().cpu() - torch.softmax(want, 1)).abs().max())
    pbound = 2 * bound + (K + 8) * 2.0 ** -24
    print(f"probabilities: error {perr:.3g} bound {pbound:.3g}")
    assert perr <= pbound
    mixed = torch.cat([torch.zeros(2, E), rows[:3]]).cuda()            # a row of zeros: zero logits
    assert torch.equal(probe.decision_function(mixed)[:2], torch.zeros(2, K, device="cuda"))


def test_scores_are_those_of_the_devices_logits(case):
    probe, ds, rows, y, want, bound = case
    s = probe.decision_function(ds).cpu()
    own = s[torch.arange(N), y][:, None]
    rank = ((s > own) | ((s == own) & (torch.arange(K)[None, :] < y[:, None]))).sum(1)
    for k in (1, 3, K):
        assert probe.top_k_score(ds, k) == float((rank < k).double().mean())
        assert probe.top_k_score(rows.cuda(), k, y) == probe.top_k_score(ds, k)
    assert probe.score(ds) == probe.top_k_score(ds, 1) == float((probe.predict(ds).cpu() == y).double().mean())
    assert probe.score(ds) > 0.9


def test_container_kept_rows_and_tensor_give_the_same_bits(case):
    from lossyless_amd.probe import _Rows
    probe, ds, rows, y, want, bound = case
    base = probe.decision_function(ds, rows_per_pass=256)
    kept = _Rows(ds, 256, True)
    kept_rows = torch.cat([z for _, z in kept.groups()])
    assert torch.equal(kept_rows.cpu(), rows)
    for other in (probe.decision_function(kept_rows, rows_per_pass=256), probe.decision_function(ds.all()),
                  probe.decision_function(rows.cuda(), rows_per_pass=100), probe.decision_function(ds, rows_per_pass=7)):
        assert torch.equal(other, base)
    assert torch.equal(probe.decision_function(rows[17:18].cuda())[0], base[17])
    half = probe.decision_function(rows.half().cuda())
    assert torch.equal(half, probe.decision_function(rows.half().float().cuda()))


def test_from_hyperprior_latents():
    """600 rows of 512 through a synthetic scale hyperprior (made in about a second): the container, its decoded rows and
    its kept rows give the same logits."""
    from hyperprior_latents_util import hyper_model
    from lossyless_amd import HyperpriorLatents, ZeroShotProbe
    model = hyper_model()
    g = torch.Generator().manual_seed(3)
    W = torch.randn(K, 512, generator=g)
    W = W / W.norm(dim=1, keepdim=True)
    y = torch.arange(N) % K
    z = (W[y] * 8 + torch.randn(N, 512, generator=g) * 0.3).cuda()
    z_strings, side_strings = model.compress(z)
    owner = types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()), hyperprior=model)
    with tempfile.TemporaryDirectory() as d:
        file = os.path.join(d, "z.bin")
        container.write_container(file, [s for pair in zip(z_strings, side_strings) for s in pair])
        ds = HyperpriorLatents(file, owner)
    probe = ZeroShotProbe(W)
    a, b = probe.decision_function(ds, rows_per_pass=256), probe.decision_function(ds.all(), rows_per_pass=64)
    assert probe.logit_scale == 100.0 and torch.equal(a, b) and probe.score(ds, y) > 0.9
    want = direct_logits(ds.all().cpu(), probe.coef_, 100.0)
    assert float((a.double().cpu() - want).abs().max()) <= logit_bound(512, 100.0, probe.coef_)
