"""Shared by test_gpu_wide_coder.py, test_gpu_feature_compressor.py and test_feature_compressor_host.py: coding tables
of any shape built directly, the host coder as the reference, and thin callers of the ``lla_*_wide`` entry points (no
test in here)."""
import ctypes
import functools

import numpy as np

TABLE_KEYS = ("cdf", "cdf_len", "offset", "bias", "exp_scale", "median")


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def make_tables(C, W, seed=0):
    """Random per-channel pmfs through ``pmf_to_quantized_cdf``: a different ``cdf_len`` per channel, every fifth channel
    the minimum of 3 entries (one symbol + escape), channel 1 the full W; plus a per-channel affine and medians."""
    from lossyless_amd.entropy import pmf_to_quantized_cdf
    rng = np.random.default_rng(seed)
    cdf = np.zeros((C, W), np.int32)
    cdf_len = rng.integers(3, W + 1, size=C).astype(np.int32)
    cdf_len[::5] = 3
    cdf_len[1 % C] = W
    offset = np.zeros(C, np.int32)
    for c in range(C):
        n = int(cdf_len[c])
        pmf = rng.random(n - 1) + 0.02          # n - 2 symbols and the tail mass (the escape symbol)
        pmf[-1] *= 0.2
        cdf[c, :n] = pmf_to_quantized_cdf(pmf / pmf.sum()).astype(np.int64).astype(np.int32)
        offset[c] = -int(rng.integers(0, n))
    return dict(cdf=cdf, cdf_len=cdf_len, offset=offset,
                bias=rng.normal(0, 0.2, C).astype(np.float32),
                exp_scale=np.exp(rng.normal(0, 0.3, C)).astype(np.float32),
                median=rng.uniform(-0.5, 0.5, C).astype(np.float32))


def in_table_symbols(tab, B, seed):
    """Symbols inside every channel's table, uniform over its regular slots."""
    rng = np.random.default_rng(seed)
    n_reg = np.maximum(tab["cdf_len"].astype(np.int64) - 2, 1)
    return (tab["offset"][None, :] + (rng.random((B, n_reg.shape[0])) * n_reg[None, :]).astype(np.int64)).astype(np.int32)


def plant_escapes(sym, tab, channels, magnitude=1500, seed=1):
    """Symbols outside the table (escape coding), both sides, on ``channels`` in about a third of the rows each."""
    rng = np.random.default_rng(seed)
    out = sym.copy()
    B = sym.shape[0]
    for c in channels:
        rows = rng.random(B) < 0.35
        rows[c % B] = True
        mag = rng.integers(1, magnitude, size=B)
        below = tab["offset"][c] - mag
        above = tab["offset"][c] + tab["cdf_len"][c] - 2 + mag - 1       # the first one IS the escape index
        out[:, c] = np.where(rows, np.where(rng.random(B) < 0.5, below, above), out[:, c])
    return out.astype(np.int32)


def z_for(sym, tab):
    """fp32 rows whose quantisation lands on (or next to) ``sym``: the dequantised values."""
    return ((sym.astype(np.float32) + tab["median"][None, :]) / tab["exp_scale"][None, :] - tab["bias"][None, :]).astype(np.float32)


# ------------------------------------------------------------------ the reference: the library's host coder
def host_encode(sym, tab, prefix=0):
    """lla_rans_encode_batch_host -> (payload uint8, offsets uint64 [B + 1])."""
    from lossyless_amd import _lib
    sym = np.ascontiguousarray(sym, dtype=np.int32)
    B, C = sym.shape
    t = {k: np.ascontiguousarray(tab[k]) for k in TABLE_KEYS}
    off = np.zeros(B + 1, np.uint64)
    L = _lib.lib()
    args = (P(sym), B, C, P(t["cdf"]), t["cdf"].shape[1], P(t["cdf_len"]), P(t["offset"]), prefix)
    assert L.lla_rans_encode_batch_host(*args, None, 0, P(off)) in (_lib.LLA_OK, _lib.LLA_ECAP)
    out = np.empty(int(off[-1]), np.uint8)
    _lib.check(L.lla_rans_encode_batch_host(*args, P(out), out.size, P(off)), "lla_rans_encode_batch_host")
    return out, off


def host_dequantise(sym, tab):
    from lossyless_amd import _lib
    sym = np.ascontiguousarray(sym, dtype=np.int32)
    out = np.empty(sym.shape, np.float32)
    _lib.check(_lib.lib().lla_dequantise_host(P(sym), sym.shape[0], sym.shape[1], P(np.ascontiguousarray(tab["bias"])),
                                              P(np.ascontiguousarray(tab["exp_scale"])),
                                              P(np.ascontiguousarray(tab["median"])), P(out)), "lla_dequantise_host")
    return out


def padded(payload):
    return np.concatenate([payload, np.zeros((-len(payload)) % 4 + 4, np.uint8)])


# ------------------------------------------------------------------ device callers
def dev_tables(tab):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(tab[k])).cuda() for k in TABLE_KEYS}


def _streams(scratch, stride, lengths):
    """end-aligned scratch -> (streams back to back, lengths)."""
    sc, ln = scratch.cpu().numpy(), lengths.cpu().numpy().astype(np.int64)
    parts = [sc[(b + 1) * stride - int(n):(b + 1) * stride] for b, n in enumerate(ln)]
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), ln


def device_encode(x, d, W, window=None, want_symbols=False):
    """x: int32 symbols or fp16 / fp32 z (numpy).  window None: the RESIDENT entry point (lla_rans_encode_batch /
    lla_quantise_encode); else lla_quantise_encode_wide with that window.  -> (rc, streams, lengths, symbols_out)."""
    import torch
    from lossyless_amd import _lib
    L = _lib.lib()
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    B, C = xt.shape
    zt = {torch.int32: _lib.LLA_Z_SYMBOLS, torch.float16: _lib.LLA_Z_F16, torch.float32: _lib.LLA_Z_F32}[xt.dtype]
    stride = int(L.lla_rans_max_encoded_bytes(C))
    scratch = torch.zeros(B * stride, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros(B, dtype=torch.int32, device="cuda")
    symbols = torch.full((B, C), -12345, dtype=torch.int32, device="cuda") if want_symbols else None
    tabs = (_lib.ptr(d["cdf"]), W, _lib.ptr(d["cdf_len"]), _lib.ptr(d["offset"]), _lib.ptr(scratch), stride, _lib.ptr(lengths))
    aff = (_lib.ptr(d["bias"]), _lib.ptr(d["exp_scale"]), _lib.ptr(d["median"]))
    if window is not None:
        rc = L.lla_quantise_encode_wide(_lib.ptr(xt), zt, B, C, *aff, *tabs, _lib.ptr(symbols), window, _lib.stream_ptr())
    elif zt == _lib.LLA_Z_SYMBOLS:
        rc = L.lla_rans_encode_batch(_lib.ptr(xt), B, C, *tabs, _lib.stream_ptr())
    else:
        rc = L.lla_quantise_encode(_lib.ptr(xt), zt, B, C, *aff, *tabs, _lib.ptr(symbols), _lib.stream_ptr())
    if rc != 0:
        return rc, None, None, None
    torch.cuda.synchronize()
    s, ln = _streams(scratch, stride, lengths)
    return rc, s, ln, (symbols.cpu().numpy() if want_symbols else None)


def device_decode_wide(payload, off, prefix, B, d, C, W, window, off_first=0, off_step=1):
    """lla_rans_decode_batch_wide -> (rc, symbols, status)."""
    import torch
    from lossyless_amd import _lib
    pay = torch.from_numpy(padded(payload)).cuda()
    offs = torch.from_numpy(np.ascontiguousarray(off).astype(np.int64)).cuda()
    sym = torch.full((B, C), -12345, dtype=torch.int32, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().lla_rans_decode_batch_wide(_lib.ptr(pay), _lib.ptr(offs), prefix, off_first, off_step, B, C,
                                               _lib.ptr(d["cdf"]), W, _lib.ptr(d["cdf_len"]), _lib.ptr(d["offset"]),
                                               _lib.ptr(sym), _lib.ptr(status), window, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, sym.cpu().numpy(), status.cpu().numpy()


def device_gather_wide(payload, off, prefix, N, index, d, C, W, window, dtype="float32", ld=None, off_first=0, off_step=1,
                       fill=-777.0):
    """lla_rans_decode_gather_wide -> (rc, out [B, ld] prefilled with ``fill``, status)."""
    import torch
    from lossyless_amd import _lib
    pay = torch.from_numpy(padded(payload)).cuda()
    offs = torch.from_numpy(np.ascontiguousarray(off).astype(np.int64)).cuda()
    idx = torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).cuda()
    B = idx.numel()
    ld = C if ld is None else ld
    tdt = getattr(torch, dtype)
    out = torch.full((B, ld), fill, dtype=tdt, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().lla_rans_decode_gather_wide(
        _lib.ptr(pay), _lib.ptr(offs), prefix, off_first, off_step, N, _lib.ptr(idx), B, C, _lib.ptr(d["cdf"]), W,
        _lib.ptr(d["cdf_len"]), _lib.ptr(d["offset"]), _lib.ptr(d["bias"]), _lib.ptr(d["exp_scale"]), _lib.ptr(d["median"]),
        _lib.ptr(out), _lib.LLA_Z_F32 if tdt == torch.float32 else _lib.LLA_Z_F16, ld, _lib.ptr(status), window,
        _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu(), status.cpu().numpy()


# ------------------------------------------------------------------ rate points with wide tables
def widen_state_dict(sd, push):
    """A factorized rate point whose outer quantiles are pushed ``push`` bins outwards and whose tables are rebuilt from
    them (``EntropyBottleneck.update``): the same model, W larger by 2 * push."""
    import torch
    from lossyless_amd.entropy import EntropyBottleneck
    C = int(sd["scaling"].numel())
    eb = EntropyBottleneck(C, init_scale=10, filters=[3, 3, 3, 3])
    pre = "entropy_bottleneck."
    own = {k[len(pre):]: v.clone() for k, v in sd.items() if k.startswith(pre) and not k.rsplit(".", 1)[-1].startswith(("_offset", "_quantized_cdf", "_cdf_length"))}
    eb.load_state_dict(own, strict=False)
    with torch.no_grad():
        eb.quantiles[:, 0, 0] -= push
        eb.quantiles[:, 0, 2] += push
    eb.update(force=True)
    out = {k: v.clone() for k, v in sd.items() if not k.startswith(pre)}
    out.update({pre + k: v.detach().clone() for k, v in eb.state_dict().items()})
    return out


def gaussian_features(N, C, seed):
    """Seeded Gaussian rows with per-channel scales."""
    import torch
    g = torch.Generator().manual_seed(seed)
    scale = 0.2 + torch.rand(C, generator=g)
    return torch.randn(N, C, generator=g) * scale
