"""CPU: the pieces of the hyperprior dataset path that need no GPU -- the new C entry points are declared, bound and
exported; the two-records-per-image container is the reference's framing (``lla_container_index`` and the reference's
field readers walk it); ``HyperpriorClipCompressor`` builds on the CPU and refuses to compute there."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from lossyless_amd import _lib

NEW_SYMBOLS = ("lla_gaussian_quantise_encode", "lla_gaussian_decode_dequantise", "lla_rans_compact_pairs",
               "lla_rans_compact_pairs_workspace_bytes", "lla_rans_decode_batch_strided")


def _strings(n, seed):
    """n (z, side) pairs of rANS-shaped strings: whole 4-byte words, zero-length ones included."""
    rng = np.random.default_rng(seed)
    z = [rng.integers(0, 256, size=4 * int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 40, size=n)]
    s = [rng.integers(0, 256, size=4 * int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 9, size=n)]
    if n > 2:
        z[1], s[2], s[n - 1] = b"", b"", b""
    return z, s


def test_new_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "lossyless_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared"
        assert name in _lib.EXPORTS and hasattr(L, name), f"{name} not bound / exported"
    # each replaces reference lines, and says which
    for name in ("lla_gaussian_quantise_encode", "lla_gaussian_decode_dequantise"):
        doc = header[:header.index("int " + name)].rsplit("/*", 1)[1]
        assert "rates.py:694-729" in doc or "rates.py:715-724" in doc, name
    assert _lib.lib().lla_abi_version() == _lib.ABI_VERSION
    # argument checks run on the host, before any launch: B = 0 is a no-op, null pointers are refused
    Lb = _lib.lib()
    assert Lb.lla_gaussian_quantise_encode(None, 2, 0, 512, None, None, None, 512, None, 0.11, None, 64, 8, None, None,
                                           None, 0, None, None, None, None) == 0
    assert Lb.lla_gaussian_quantise_encode(None, 2, 4, 512, None, None, None, 512, None, 0.11, None, 64, 8, None, None,
                                           None, 0, None, None, None, None) == -1
    assert Lb.lla_gaussian_decode_dequantise(None, None, 1, 0, 2, 4, 512, None, None, None, 512, None, 0.11, None, 64, 8,
                                             None, None, None, None, None) == -1
    assert Lb.lla_rans_compact_pairs(None, 0, None, None, 0, None, 3, None, 0, None, None, 0, None) == -1
    assert Lb.lla_rans_compact_pairs_workspace_bytes(1000) >= 2000 * 4 + _lib.lib().lla_rans_compact_workspace_bytes(2000)


@pytest.mark.parametrize("n", [0, 1, 5, 300])
def test_pair_container_is_the_reference_framing_with_two_records_per_image(n, tmp_path):
    from lossyless_amd.compressor import read_bytes, read_uints
    from lossyless_amd.hyperprior_compressor import read_pair_container, write_pair_container
    z, s = _strings(n, seed=n)
    path = tmp_path / "pairs.bin"
    write_pair_container(path, z, s)
    blob = path.read_bytes()
    # the bytes, spelled out
    want = (2 * n).to_bytes(4, "big") + b"".join(len(x).to_bytes(4, "big") + x for pair in zip(z, s) for x in pair)
    assert blob == want
    # lla_container_index: 2N records, in order
    arr = np.frombuffer(blob, dtype=np.uint8)
    cnt = ctypes.c_uint32(0)
    off = np.zeros(2 * n + 1, dtype=np.uint64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert _lib.lib().lla_container_index(P(arr), arr.size, P(off), off.size, ctypes.byref(cnt)) == 0
    assert cnt.value == 2 * n and int(off[-1]) == len(blob) - 4
    body = blob[4:]
    for i in range(n):
        assert body[int(off[2 * i]) + 4:int(off[2 * i + 1])] == z[i]
        assert body[int(off[2 * i + 1]) + 4:int(off[2 * i + 2])] == s[i]
    # the reference's reader loop (hub/compressor.py:233-237) walks it unchanged
    with path.open("rb") as f:
        (n_rec,) = read_uints(f, 1)
        recs = [read_bytes(f, read_uints(f, 1)[0]) for _ in range(n_rec)]
        assert f.read() == b""
    assert n_rec == 2 * n and recs[0::2] == z and recs[1::2] == s
    # reader / writer of the package round-trip (file objects too)
    assert read_pair_container(path) == [z, s]
    buf = io.BytesIO()
    write_pair_container(buf, z, s)
    assert buf.getvalue() == blob and read_pair_container(io.BytesIO(blob)) == [z, s]


def test_pair_container_reader_refuses_damaged_files():
    from lossyless_amd.hyperprior_compressor import read_pair_container, write_pair_container
    z, s = _strings(6, seed=1)
    buf = io.BytesIO()
    write_pair_container(buf, z, s)
    blob = buf.getvalue()
    for cut in (0, 3, 4, 7, len(blob) - 1):
        with pytest.raises(ValueError):
            read_pair_container(io.BytesIO(blob[:cut]))
    with pytest.raises(ValueError):      # odd count
        read_pair_container(io.BytesIO((11).to_bytes(4, "big") + blob[4:]))
    with pytest.raises(ValueError):
        write_pair_container(io.BytesIO(), z, s[:-1])


def test_synthetic_hyperprior_weights_are_seeded_and_spread_over_the_scale_table():
    """What the GPU tests rely on, checked where it is cheap: the predicted scales use at least half of the 64 rows, fall
    below ``scale_bound`` (mean = scale < bound there: the row is bounded, the mean is not) and above the last entry."""
    from lossyless_amd.rates import HRateHyperprior, synthetic_hyperprior_state_dict
    sd, sd2 = synthetic_hyperprior_state_dict(3), synthetic_hyperprior_state_dict(3)
    assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert not torch.equal(sd["z_encoder.module.8.bias"], synthetic_hyperprior_state_dict(4)["z_encoder.module.8.bias"])
    m = HRateHyperprior(512).eval()
    m.load_state_dict(sd)
    assert m.is_coder_updated and tuple(m.gaussian_conditional._quantized_cdf.shape)[0] == 64
    z = torch.randn(256, 512, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        z_in = m.process_z_in(z)
        med = m.entropy_bottleneck._medians()
        s_hat = torch.round(m.side_encoder(z_in) - med) + med
        scales = m.z_encoder(s_hat)[:, :512]
        idx = m.gaussian_conditional.build_indexes(scales)
    bound = float(m.gaussian_conditional.scale_bound)
    assert idx.unique().numel() >= 32
    assert bool((scales < bound).any()) and bool((scales > float(m.gaussian_conditional.scale_table[-1])).any())


def test_hyperprior_compressor_builds_on_the_cpu_and_refuses_to_compute_there(tmp_path):
    import hubconf
    from lossyless_amd import ClipCompressor, HyperpriorClipCompressor
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    sd = synthetic_hyperprior_state_dict(0)
    path = tmp_path / "hyperprior.pt"
    torch.save(sd, path)
    c, transform = hubconf.clip_hyperprior_compressor(str(path), device="cpu", clip_weights="synthetic")
    assert isinstance(c, HyperpriorClipCompressor) and isinstance(c, ClipCompressor) and transform is c.preprocess
    assert c.z_dim == 512 and c.side_z_dim == 102 and c.records_per_image == 2 and ClipCompressor.records_per_image == 1
    for k, v in sd.items():              # loaded by HRateHyperprior._load_from_state_dict, tables included
        assert torch.equal(c.hyperprior.state_dict()[k], v), k
    x = torch.zeros(2, 3, 224, 224)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c.compress(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c.decompress([[b""], [b""]])
    with pytest.raises(ValueError):
        c.compress_dataset(x, tmp_path / "x.bin")
    with pytest.raises(NotImplementedError, match="not bit-equal"):
        c.decompress_dataset(tmp_path / "x.bin", is_cpu=True)
    import inspect
    assert inspect.signature(c.decompress_dataset).parameters["is_cpu"].default is False
    # what ClipCompressor keeps for its factorized model says so here instead of failing on a missing attribute
    for call in (c._tables, lambda: c._records_of([b""]), lambda: c._decode_records_host(None, None, 0)):
        with pytest.raises(NotImplementedError, match="HyperpriorClipCompressor"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c.encode_batch_records(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c._decode_strings([[b""], [b""]])
    with pytest.raises(KeyError):        # a factorized state dict is not a hyperprior one
        HyperpriorClipCompressor({k: v for k, v in sd.items() if not k.startswith("z_encoder")}, device="cpu",
                                 clip_weights="synthetic")


def test_compact_pairs_counts_two_records_per_image_without_overflow():
    """2B records are counted in an int: B = 2^30 is refused before anything is launched, and the workspace size of the
    largest B accepted is computed in size_t."""
    import ctypes
    from lossyless_amd import _lib
    L = _lib.lib()
    big = (1 << 30) - 1
    nblk = (2 * big + 1023) // 1024
    assert int(L.lla_rans_compact_pairs_workspace_bytes(big)) == 2 * big * 4 + (nblk + 1) * 8
    assert int(L.lla_rans_compact_pairs_workspace_bytes(0)) == int(L.lla_rans_compact_pairs_workspace_bytes(1)) == 8 + 16
    buf = (ctypes.c_uint64 * 4)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    for B in (1 << 30, (1 << 31) - 1, -1):
        assert L.lla_rans_compact_pairs(P, 8, P, P, 8, P, B, P, 32, P, P, 1 << 40, None) == _lib.LLA_EINVAL
