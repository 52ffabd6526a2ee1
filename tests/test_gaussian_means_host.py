"""CPU: ``HRateHyperprior(coded_means=)`` -- the opt-in coder that subtracts the predicted means (lossyless/rates.py:647-650)
instead of the scales the reference puts in their place (rates.py:689-696).  Construction, the switch in
``get_indexes_means_hat``, the state dict, and the oracle coder composed with the means the twin hands out.  No device."""
import numpy as np
import pytest
import torch

from lossyless_amd.rates import HRateHyperprior
from oracle import gc

C, S, B = 24, 10, 9


@pytest.fixture(scope="module")
def tables():
    return gc.derive_tables(gc.get_scale_table())


def _twin(mode=None, seed=3):
    """A CPU twin whose z_encoder predicts scales over (and past) the table and means that are NOT the scales."""
    torch.manual_seed(seed)
    m = HRateHyperprior(C, side_z_dim=S) if mode is None else HRateHyperprior(C, side_z_dim=S, coded_means=mode)
    m.eval()
    with torch.no_grad():
        m.scaling.fill_(0.4)
        m.biasing.normal_(0, 0.1)
        last = m.z_encoder.module[-1]
        last.weight.mul_(6)
        last.bias[:C] = torch.exp(torch.linspace(np.log(0.05), np.log(300.0), C))
        last.bias[C:] = torch.linspace(-40.0, 40.0, C)
    m.update(force=True)          # (the 64-level scale table and the coding tables: host code)
    return m


def _side_hat(m, z):
    """What ``EntropyBottleneck.decompress`` gives for the side strings of z (the strings themselves are coded on the GPU
    only): round(side - median) + median."""
    with torch.no_grad():
        med = m.entropy_bottleneck._medians()
        return torch.round(m.side_encoder(m.process_z_in(z)) - med) + med


def test_constructs_on_the_cpu_and_refuses_bad_values():
    assert HRateHyperprior(C).coded_means == "scales"
    assert HRateHyperprior(C, coded_means="scales").coded_means == "scales"
    m = HRateHyperprior(C, coded_means="predicted")
    assert m.coded_means == "predicted" and m.scaling.device.type == "cpu"
    for bad in ("means", "Predicted", "", None, 1):
        with pytest.raises(ValueError):
            HRateHyperprior(C, coded_means=bad)
    with pytest.raises(ValueError):
        HRateHyperprior(C, is_pred_mean=False, coded_means="predicted")
    assert HRateHyperprior(C, is_pred_mean=False).coded_means == "scales"


def test_state_dict_does_not_carry_the_mode():
    a, b = _twin("scales"), _twin("predicted")
    assert list(a.state_dict()) == list(b.state_dict())
    assert not any("coded_means" in k for k in a.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    a.load_state_dict(b.state_dict(), strict=True)
    assert b.coded_means == "predicted" and a.coded_means == "scales"


def test_get_indexes_means_hat_returns_the_second_chunk_only_in_the_new_mode(tables):
    z = torch.randn(B, C, generator=torch.Generator().manual_seed(1)) * 3
    got = {}
    for mode in (None, "scales", "predicted"):
        m = _twin(mode)
        side_hat = _side_hat(m, z)
        m._side_strings_to_rows = lambda strings, s=side_hat: s          # (the side strings are decoded on the GPU only)
        with torch.no_grad():
            idx, means_hat = m.get_indexes_means_hat([b""] * B)
            scales, means = m.z_encoder(side_hat).chunk(2, -1)
        assert not torch.equal(scales, means)
        assert tuple(idx.shape) == tuple(means_hat.shape) == (B, C, 1, 1)
        assert np.array_equal(idx.reshape(B, C).numpy(), gc.build_indexes(scales.numpy(), tables["scale_table"]))
        want = means if mode == "predicted" else scales
        assert torch.equal(means_hat.reshape(B, C), want), mode
        got[mode] = idx
    assert torch.equal(got[None], got["scales"]) and torch.equal(got["scales"], got["predicted"])   # the row never depends on the mean


def test_oracle_coder_with_the_twins_means_reproduces_the_twins_cpu_values(tables):
    """symbols_of(z_in, means) -> compress -> decompress -> + means, with the rows and means ``get_indexes_means_hat`` hands
    out, is what the twin's CPU path (``forward_help``'s conditional model: the trained likelihood's own quantisation) returns -- in the new
    mode.  In the default mode the coder's values are centred at the scales and differ from it."""
    z = torch.randn(B, C, generator=torch.Generator().manual_seed(2)) * 4
    coded = {}
    for mode in ("scales", "predicted"):
        m = _twin(mode)
        side_hat = _side_hat(m, z)
        m._side_strings_to_rows = lambda strings, s=side_hat: s
        with torch.no_grad():
            idx, means_hat = m.get_indexes_means_hat([b""] * B)
            z_in = m.process_z_in(z)
            scales, means = m.chunk_params(m.z_encoder(side_hat))
            # (forward_help's own lines, rates.py:647-650; the whole method also codes on the GPU for its real-rate log)
            z_hat_twin = m.process_z_out(m.gaussian_conditional(z_in, scales, means=means)[0])
        assert float((means - scales).abs().min()) > 0           # nowhere equal: a mix-up cannot pass by accident
        mh = means_hat.reshape(B, C).numpy()
        sym = gc.symbols_of(z_in.numpy(), mh)
        assert np.array_equal(sym, np.rint(z_in.numpy() - mh).astype(np.int32))
        rows = idx.reshape(B, C).numpy()
        strings = gc.compress(sym, rows, tables)
        back = gc.decompress(strings, rows, tables)
        assert np.array_equal(back, sym)
        coded[mode] = m.process_z_out(torch.from_numpy(back.astype(np.float32) + mh))
        if mode == "predicted":
            assert torch.equal(coded[mode], z_hat_twin)
        else:
            assert not torch.equal(coded[mode], z_hat_twin)
    assert not torch.equal(coded["scales"], coded["predicted"])
