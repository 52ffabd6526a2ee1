"""CPU: ``FeatureCompressor`` on ``device="cpu"`` (the library's host coder) at three widths against the oracle, against
``ClipCompressor``'s host path at 512 dimensions, and the plumbing of the windowed coder's symbols."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import container, eb, pyrans
from wide_coder_util import gaussian_features, widen_state_dict

WIDE_SYMBOLS = ("lla_rans_table_fits", "lla_rans_wide_window", "lla_quantise_encode_wide", "lla_rans_decode_batch_wide",
                "lla_rans_decode_gather_wide")


def _shipped(tag="5e-02"):
    return torch.load(os.path.join(ROOT, "lossyless_amd", "assets", f"beta{tag}_factorized_rate.pt"), map_location="cpu",
                      weights_only=True)


@functools.lru_cache(maxsize=None)
def rate_point(C):
    """A factorized rate point at C dimensions: the shipped one at 512 (tables pushed 3 bins outwards), an untrained
    module with seeded affine elsewhere."""
    if C == 512:
        return widen_state_dict(_shipped(), push=3)
    from lossyless_amd.rates import HRateFactorizedPrior
    torch.manual_seed(C)
    m = HRateFactorizedPrior(C, kwargs_ent_bottleneck=dict(init_scale=6, filters=[3, 3, 3, 3]))
    with torch.no_grad():
        m.scaling.copy_(torch.randn(C) * 0.2)
        m.biasing.copy_(torch.randn(C) * 0.1)
    m.entropy_bottleneck.update()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _comp(C):
    import hubconf
    return hubconf.feature_compressor(rate_point(C), device="cpu")


@pytest.mark.parametrize("C", [24, 512, 1024])
def test_round_trip_and_oracle(C, tmp_path):
    comp = _comp(C)
    assert comp.z_dim == C
    Z = gaussian_features(40, C, seed=C) * 4
    z_hat = comp(Z)
    strings = comp.compress(Z)
    assert len(strings) == 40 and torch.equal(comp.decompress(strings), z_hat)
    assert comp.get_rate(Z) == 8 * sum(map(len, strings)) / 40
    file = tmp_path / "z.bin"
    comp.compress_dataset(Z, file, is_info=False)
    assert np.array_equal(comp.decompress_dataset(file, is_info=False), z_hat.numpy())
    assert torch.equal(comp.open_dataset(file).take([39, 0, 39]), z_hat[[39, 0, 39]])
    # the container parses with the oracle's reader and its records decode with the pure-Python coder to the same values
    records = container.read_container(str(file))
    assert [bytes(r) for r in records] == strings
    t = comp._tables()
    tab = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in t.items()}
    sym = eb.symbols_of(Z.numpy(), tab)
    for i in (0, 17, 39):
        got = pyrans.decode(bytes(records[i]), C, tab["cdf"], tab["cdf_len"], tab["offset"])
        assert list(got) == sym[i].tolist()
        assert bytes(records[i]) == pyrans.encode(sym[i], tab["cdf"], tab["cdf_len"], tab["offset"])
    assert np.array_equal(eb.dequantise(sym, tab).astype(np.float32), z_hat.numpy())


def test_same_bytes_as_clip_compressor_host_path(tmp_path):
    """At 512 dimensions the records are what ClipCompressor's coder gives for the same embeddings: the strings decode
    through ClipCompressor's host path to ClipCompressor's values, and a container of them is the FeatureCompressor's file."""
    from lossyless_amd import ClipCompressor
    sd = rate_point(512)
    comp = _comp(512)
    clip = ClipCompressor(sd, device="cpu", clip_weights="synthetic")
    Z = (gaussian_features(33, 512, seed=5) * 0.4).half()           # embeddings are fp16
    strings = comp.compress(Z)
    assert torch.equal(clip.decompress(strings), comp(Z))
    file, file2 = tmp_path / "z.bin", tmp_path / "z2.bin"
    comp.compress_dataset(Z, file, is_info=False)
    body, off = clip._records_of(strings)                           # ClipCompressor's own record framing
    clip._write_container(file2, body, len(strings), None, None, 0.0, False)
    assert file.read_bytes() == file2.read_bytes()
    assert np.array_equal(clip.decompress_dataset(file, is_info=False), comp(Z).numpy())
    assert torch.equal(clip.open_dataset(file, device="cpu").take([1, 32]), comp.open_dataset(file).take([1, 32]))


def test_z_dim_from_a_dict_and_from_a_path(tmp_path):
    import hubconf
    from lossyless_amd import FeatureCompressor
    for C in (24, 1024):
        sd = rate_point(C)
        path = tmp_path / f"rate{C}.pt"
        torch.save(sd, path)
        a, b = FeatureCompressor(sd, device="cpu"), hubconf.feature_compressor(str(path), device="cpu")
        assert a.z_dim == b.z_dim == C and a.entropy_bottleneck.channels == C
        Z = gaussian_features(5, C, seed=1)
        assert a.compress(Z) == b.compress(Z)
    assert set(FeatureCompressor(_shipped(), device="cpu").state_dict()) == set(_shipped())


def test_wrong_width_names_both_widths():
    comp = _comp(24)
    for bad in (torch.zeros(3, 25), torch.zeros(3, 512), torch.zeros(24)):
        with pytest.raises(ValueError, match=r"width 24 .*(25|512|24)"):
            comp(bad)
    with pytest.raises(ValueError, match="width 24 .* width 25"):
        comp.compress_dataset([torch.zeros(3, 24), torch.zeros(3, 25)], os.devnull, is_info=False)


def test_batches_equal_one_tensor_and_labels_round_trip(tmp_path):
    comp = _comp(24)
    Z = gaussian_features(2500, 24, seed=2) * 3
    y = np.arange(2500) % 7
    one, many, lf, lf2 = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "a.npy", tmp_path / "b.npy"
    comp.compress_dataset(Z, one, lf, labels=y, is_info=False, entropy_group=1)
    cuts = [0, 1, 700, 701, 1900, 2500]
    comp.compress_dataset((Z[a:b] for a, b in zip(cuts, cuts[1:])), many, lf2, labels=torch.from_numpy(y), is_info=False)
    assert one.read_bytes() == many.read_bytes()
    half = tmp_path / "h.bin"
    comp.compress_dataset([Z[:10].half(), Z[10:20].half().float()], half, is_info=False)      # mixed dtypes, same values
    assert half.read_bytes() == (lambda f: (comp.compress_dataset(Z[:20].half(), f, is_info=False), f.read_bytes())[1])(tmp_path / "h2.bin")
    dec, labels = comp.decompress_dataset(one, lf, is_info=False)
    assert np.array_equal(labels, y) and np.array_equal(np.load(lf2), np.load(lf)) and dec.shape == (2500, 24)
    ds = comp.open_dataset(one, lf)
    assert torch.equal(ds.labels([6, 8]), torch.tensor([6, 1]))
    with pytest.raises(ValueError):
        comp.compress_dataset(Z, one, lf, is_info=False)            # a label file without labels
    with pytest.raises(ValueError):
        comp.compress_dataset(Z, one, lf, labels=y[:5], is_info=False)


def test_hub_factories_are_unchanged():
    import inspect
    import hubconf
    for name in ("clip_compressor_b005", "clip_compressor_b001", "clip_compressor_b01", "clip_compressor"):
        f = getattr(hubconf, name)
        params = list(inspect.signature(f).parameters)
        assert params == (["state_dict", "device", "kwargs"] if name == "clip_compressor" else ["device", "kwargs"])
    comp, transform = hubconf.clip_compressor_b005(device="cpu", clip_weights="synthetic")
    assert comp.z_dim == 512 and transform is comp.preprocess and int(comp.entropy_bottleneck._quantized_cdf.shape[1]) == 32
    comp2, _ = hubconf.clip_compressor(_shipped(), device="cpu", clip_weights="synthetic")
    assert all(torch.equal(v, comp2.state_dict()[k]) for k, v in comp.state_dict().items() if k.startswith(("scaling", "biasing", "entropy")))
    assert list(inspect.signature(hubconf.feature_compressor).parameters) == ["state_dict", "device"]


def test_wide_symbols_in_header_and_binding():
    from lossyless_amd import _lib
    header = open(os.path.join(ROOT, "include", "lossyless_amd.h")).read()
    raw = _lib.lib()
    for name in WIDE_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(raw, name), f"{name} not bound / exported"
        assert re.search(rf"\b{name}\(", header), f"{name} not declared"
    for macro, value in (("LLA_CODER_ENCODE", _lib.CODER_ENCODE), ("LLA_CODER_DECODE", _lib.CODER_DECODE),
                         ("LLA_CODER_GATHER", _lib.CODER_GATHER), ("LLA_Z_SYMBOLS", _lib.LLA_Z_SYMBOLS)):
        assert re.search(rf"#define {macro} {value}\b", header)


def test_the_query_matches_the_documented_limits():
    """What the issue's motivation states: at 512 channels the encoder refuses from W = 49, the gathered decoder a little
    earlier; at 1024 channels the shipped width is refused; the shipped shape at 512 fits all three."""
    from lossyless_amd import _lib
    fits = _lib.lib().lla_rans_table_fits
    assert [fits(512, 32, k) for k in range(3)] == [1, 1, 1] and [fits(512, 33, k) for k in range(3)] == [1, 1, 1]
    assert fits(512, 48, 0) == 1 and fits(512, 49, 0) == 0
    assert fits(512, 40, 2) == 0 or fits(512, 41, 2) == 0           # the gather refuses before the encoder does
    # 1024 channels: 2 KiB of table per entry of W and 8 KiB of (length, offset) pairs: the decoder takes W <= 28
    assert fits(1024, 28, 1) == 1 and fits(1024, 29, 1) == 0 and [fits(1024, 32, k) for k in range(3)] == [0, 0, 0]
    assert fits(0, 33, 0) == 0 and fits(512, 2, 0) == 0 and fits(512, 33, 3) == 0
    window = _lib.lib().lla_rans_wide_window
    for C, W in ((512, 33), (1024, 33), (2048, 33), (512, 129), (37, 9)):
        for kind in range(3):
            wc = window(C, W, kind, 0, None)
            assert wc > 0 and wc % 4 == 0 and window(C, W, kind, wc, None) == wc
