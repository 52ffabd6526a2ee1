"""Shared by test_latents_host.py and test_gpu_latents.py: fixtures for ``lla_rans_decode_gather`` and its host twin
(no test in here)."""
import ctypes
import functools
import os

import numpy as np

from conftest import GOLDEN, load_tables, sample_symbols
from oracle import cbind, container, eb

TABLE_KEYS = ("cdf", "cdf_len", "offset", "bias", "exp_scale", "median")
GOLDEN_TAIL = [63, 0, 0, 63, 31]


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def golden_index():
    """A fixed-seed permutation of the 64 golden records, then repeats and the two ends."""
    return np.concatenate([np.random.default_rng(2024).permutation(64), GOLDEN_TAIL]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def golden_case(tag):
    """-> (tables, padded body uint8, offsets uint64 [65], want fp32 [64,512]) of tests/golden/golden_{tag}.bin."""
    from lossyless_amd import _lib
    tab = load_tables(tag)
    blob = np.fromfile(os.path.join(GOLDEN, f"golden_{tag}.bin"), dtype=np.uint8)
    n = ctypes.c_uint32(0)
    off = np.zeros(65, dtype=np.uint64)
    assert _lib.lib().lla_container_index(P(blob), blob.size, P(off), off.size, ctypes.byref(n)) == 0 and n.value == 64
    body = np.concatenate([blob[4:], np.zeros(4, np.uint8)])
    want = eb.dequantise(np.load(os.path.join(GOLDEN, f"symbols_{tag}.npy")), tab)
    return tab, body, off, want


def sub_tables(tab, C):
    """The first C channels of a table set, contiguous."""
    return {k: np.ascontiguousarray(tab[k][:C]) for k in TABLE_KEYS}


@functools.lru_cache(maxsize=None)
def coded_case(tag, B, seed, C=None, escape_boost=0.02):
    """B records of symbols drawn from the model (conftest.sample_symbols), coded by the oracle WITHOUT length prefixes
    -> (tables, symbols int32 [B,C], padded payload uint8, offsets uint64 [B+1], want fp32 [B,C])."""
    full = load_tables(tag)
    sym = sample_symbols(full, B, seed, escape_boost=escape_boost)
    tab = full if C is None else sub_tables(full, C)
    sym = np.ascontiguousarray(sym[:, :tab["cdf"].shape[0]])
    pay, off = cbind.rans_encode_batch(sym, tab["cdf"], tab["cdf_len"], tab["offset"])
    pay = np.concatenate([pay, np.zeros(4, np.uint8)])
    return tab, sym, pay, off.astype(np.uint64), eb.dequantise(sym, tab)


def code_rows(sym, tab):
    """int32 [B,C] -> (padded payload, offsets, want) as coded_case."""
    sym = np.ascontiguousarray(sym, dtype=np.int32)
    pay, off = cbind.rans_encode_batch(sym, tab["cdf"], tab["cdf_len"], tab["offset"])
    return np.concatenate([pay, np.zeros(4, np.uint8)]), off.astype(np.uint64), eb.dequantise(sym, tab)


def edge_rows(tab):
    """The rows of test_gpu_entropy.test_encode_edge_symbols."""
    C = tab["cdf"].shape[0]
    return np.stack([np.full(C, -2 ** 29, np.int32),                 # all escaped, 8-digit payloads
                     np.full(C, 2 ** 29, np.int32),
                     tab["offset"].astype(np.int32),
                     (tab["offset"] + tab["cdf_len"] - 2).astype(np.int32),   # exactly the escape index
                     (tab["offset"] + tab["cdf_len"] - 3).astype(np.int32),
                     (tab["offset"] - 1).astype(np.int32)])


def host_gather(pay, off, prefix, index, tab, dtype=np.float32, ld=None, fill=None):
    """lla_rans_decode_gather_host -> (rc, out [B, ld], status)."""
    from lossyless_amd import _lib
    t = {k: np.ascontiguousarray(tab[k]) for k in TABLE_KEYS}
    C, W = t["cdf"].shape
    index = np.ascontiguousarray(index, dtype=np.int64)
    B = index.shape[0]
    ld = C if ld is None else ld
    out = np.full((B, ld), np.nan if fill is None else fill, dtype=dtype)
    status = np.full(B, -7, np.int32)
    rc = _lib.lib().lla_rans_decode_gather_host(
        P(pay), P(off), prefix, off.shape[0] - 1, P(index), B, C, P(t["cdf"]), W, P(t["cdf_len"]), P(t["offset"]),
        P(t["bias"]), P(t["exp_scale"]), P(t["median"]), P(out), _lib.LLA_Z_F32 if dtype == np.float32 else _lib.LLA_Z_F16,
        ld, P(status))
    return rc, out, status


def write_dataset(tmp_path, tag, N, seed):
    """A container of N sampled records + a label file holding arange(N) -> (file, label file, symbols)."""
    tab = load_tables(tag)
    sym = sample_symbols(tab, N, seed, escape_boost=0.02)
    strings = [cbind.rans_encode(s, tab["cdf"], tab["cdf_len"], tab["offset"]) for s in sym]
    file, lf = tmp_path / "z.bin", tmp_path / "y.npy"
    container.write_container(str(file), strings)
    np.save(lf, np.arange(N))
    return file, lf, sym
