"""CPU: the entry points behind ``HyperpriorLatents`` -- declared, bound, exported, their argument checks (nothing is
launched: every call here is refused, or has B = 0) -- and ``HyperpriorClipCompressor.open_dataset`` on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from lossyless_amd import _lib

NEW_SYMBOLS = ("lla_rans_decode_gather_strided", "lla_gaussian_decode_gather")


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "lossyless_amd.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared"
        assert name in _lib.EXPORTS and hasattr(raw, name), f"{name} not bound / exported"
        doc = header[:header.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "lossyless/rates.py:715-724" in " ".join(doc.split())      # says which reference lines it replaces
    doc = header[:header.index("int lla_rans_decode_gather_strided(")].rsplit("/*", 1)[1]
    assert "float(sym) + median" in doc                                   # the equality HyperpriorLatents depends on
    assert _lib.lib().lla_abi_version() == _lib.ABI_VERSION == 4          # additive: the ABI version stays


def test_strided_gather_checks_its_arguments():
    L = _lib.lib()
    buf = np.zeros(4096, np.uint8)                    # stands for every pointer: no call below gets as far as a launch

    def call(**over):
        a = dict(payload=P(buf), off=P(buf), first=1, step=2, N=8, index=P(buf), B=4, C=102, cdf=P(buf), W=23,
                 cdf_len=P(buf), offset=P(buf), bias=P(buf), es=P(buf), med=P(buf), out=P(buf), dtype=_lib.LLA_Z_F32,
                 ld=104, status=P(buf))
        a.update(over)
        return L.lla_rans_decode_gather_strided(
            a["payload"], a["off"], 1, a["first"], a["step"], a["N"], a["index"], a["B"], a["C"], a["cdf"], a["W"],
            a["cdf_len"], a["offset"], a["bias"], a["es"], a["med"], a["out"], a["dtype"], a["ld"], a["status"], None)

    for k in ("payload", "off", "index", "cdf", "cdf_len", "offset", "bias", "es", "med", "out", "status"):
        assert call(**{k: None}) == _lib.LLA_EINVAL, k
    assert call(first=-1) == _lib.LLA_EINVAL and call(step=0) == _lib.LLA_EINVAL and call(step=-2) == _lib.LLA_EINVAL
    assert call(ld=101) == _lib.LLA_EINVAL and call(N=-1) == _lib.LLA_EINVAL
    for bad in (0, 3, -1):
        assert call(dtype=bad) == _lib.LLA_EINVAL
    assert call(B=0) == _lib.LLA_OK
    assert call(B=0, first=-1) == _lib.LLA_EINVAL     # a bad stride is refused whatever B is


def test_gaussian_gather_checks_its_arguments():
    L = _lib.lib()
    buf = np.zeros(4096, np.uint8)

    def call(**over):
        a = dict(payload=P(buf), off=P(buf), first=0, step=2, N=8, index=P(buf), B=4, C=512, bias=P(buf), es=P(buf),
                 scales=P(buf), lds=1024, table=P(buf), cdf=P(buf), T=64, W=3133, cdf_len=P(buf), offset=P(buf),
                 out=P(buf), dtype=_lib.LLA_Z_F32, ld=512, status_in=None, status=P(buf))
        a.update(over)
        return L.lla_gaussian_decode_gather(
            a["payload"], a["off"], 1, a["first"], a["step"], a["N"], a["index"], a["B"], a["C"], a["bias"], a["es"],
            a["scales"], a["lds"], a["table"], 0.11, a["cdf"], a["T"], a["W"], a["cdf_len"], a["offset"], a["out"],
            a["dtype"], a["ld"], a["status_in"], a["status"], None)

    for k in ("payload", "off", "index", "bias", "es", "scales", "table", "cdf", "cdf_len", "offset", "out", "status"):
        assert call(**{k: None}) == _lib.LLA_EINVAL, k
    assert call(first=-1) == _lib.LLA_EINVAL and call(step=0) == _lib.LLA_EINVAL
    assert call(ld=511) == _lib.LLA_EINVAL and call(lds=511) == _lib.LLA_EINVAL
    assert call(N=-1) == _lib.LLA_EINVAL and call(T=0) == _lib.LLA_EINVAL and call(W=2) == _lib.LLA_EINVAL
    assert call(B=-1) == _lib.LLA_EINVAL and call(C=0) == _lib.LLA_EINVAL
    for bad in (0, 3, -1):
        assert call(dtype=bad) == _lib.LLA_EINVAL
    assert call(B=0) == _lib.LLA_OK and call(B=0, status_in=P(buf)) == _lib.LLA_OK
    assert call(B=0, step=0) == _lib.LLA_EINVAL
    # the LDS query refuses what the entry point refuses, before it asks the device anything
    assert "lla_gaussian_decode_gather_lds_bytes" in _lib.EXPORTS
    front = ctypes.c_size_t(7)
    for bad in (dict(C=0), dict(T=0), dict(W=2), dict(dtype=0), dict(C=8192)):
        a = dict(C=512, T=64, W=3133, dtype=_lib.LLA_Z_F32)
        a.update(bad)
        assert L.lla_gaussian_decode_gather_lds_bytes(a["C"], a["T"], a["W"], a["dtype"], ctypes.byref(front)) == 0
        assert front.value == 0


def test_open_dataset_on_the_cpu_is_refused_before_the_file_is_touched(tmp_path):
    import hubconf
    from lossyless_amd.hyperprior_compressor import _WHY_NO_CPU
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    c, _ = hubconf.clip_hyperprior_compressor(synthetic_hyperprior_state_dict(0), device="cpu", clip_weights="synthetic")
    missing = tmp_path / "no_such_file.bin"
    for kw in (dict(device="cpu"), dict(), dict(device="cuda")):        # (a compressor on the CPU serves nothing)
        with pytest.raises(NotImplementedError, match="two records per image") as e:
            c.open_dataset(missing, **kw)
        assert _WHY_NO_CPU in str(e.value)
    assert not missing.exists()


def test_mlp_forward_padded_validates_its_input():
    from lossyless_amd.rates import MLP
    m = MLP(102, 1024, n_hid_layers=2, hid_dim=512)
    with pytest.raises(ValueError):
        m.forward_padded(torch.zeros(4, 102))
