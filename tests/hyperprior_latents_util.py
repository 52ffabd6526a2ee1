"""Shared by test_gpu_hyperprior_latents.py: callers of the two gathered decoders and of the calls they must equal
(no test in here)."""
import numpy as np
import torch

SENTINEL = -123.25


def hyper_model():
    from lossyless_amd.rates import HRateHyperprior, synthetic_hyperprior_state_dict
    m = HRateHyperprior(512).eval()
    m.load_state_dict(synthetic_hyperprior_state_dict(0))
    return m.cuda()


def _idx(index):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(index, dtype=np.int64))).cuda()


def side_symbols(model, payload, offsets, N):
    """lla_rans_decode_batch_strided over the side records (1, 2) -> int32 [N, S], status."""
    from lossyless_amd import _lib
    ebt, S = model.entropy_bottleneck.device_tables(), model.side_z_dim
    sym = torch.empty((N, S), dtype=torch.int32, device="cuda")
    st = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().lla_rans_decode_batch_strided(
        _lib.ptr(payload), _lib.ptr(offsets), 1, 1, 2, N, S, _lib.ptr(ebt["cdf"]), ebt["W"], _lib.ptr(ebt["cdf_len"]),
        _lib.ptr(ebt["offset"]), _lib.ptr(sym), _lib.ptr(st), _lib.stream_ptr())
    _lib.check(rc, "lla_rans_decode_batch_strided")
    return sym, st


def side_gather(model, payload, offsets, N, index, ld, dtype=torch.float32):
    """lla_rans_decode_gather_strided on the side records as HyperpriorLatents calls it (zero bias, unit scale, the
    medians) -> (out [B, ld] prefilled with SENTINEL, status)."""
    from lossyless_amd import _lib
    ebt, p, S = model.entropy_bottleneck.device_tables(), model._device_params(), model.side_z_dim
    idx = _idx(index)
    B = idx.numel()
    out = torch.full((B, ld), SENTINEL, dtype=dtype, device="cuda")
    st = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().lla_rans_decode_gather_strided(
        _lib.ptr(payload), _lib.ptr(offsets), 1, 1, 2, N, _lib.ptr(idx), B, S, _lib.ptr(ebt["cdf"]), ebt["W"],
        _lib.ptr(ebt["cdf_len"]), _lib.ptr(ebt["offset"]), _lib.ptr(p["side_bias"]), _lib.ptr(p["side_scale"]),
        _lib.ptr(ebt["median"]), _lib.ptr(out), _lib.LLA_Z_F32 if dtype == torch.float32 else _lib.LLA_Z_F16, ld,
        _lib.ptr(st), _lib.stream_ptr())
    _lib.check(rc, "lla_rans_decode_gather_strided")
    torch.cuda.synchronize()
    return out, st


def decode_all(model, payload, offsets, prefix, first, step, B, bias, es, scales_mat, C):
    """lla_gaussian_decode_dequantise over B consecutive images -> (z_hat fp32 [B, C], status): the yardstick."""
    from lossyless_amd import _lib
    gct, p = model.gaussian_conditional.device_tables(), model._device_params()
    z_hat = torch.full((B, C), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().lla_gaussian_decode_dequantise(
        _lib.ptr(payload), _lib.ptr(offsets), prefix, first, step, B, C, _lib.ptr(bias), _lib.ptr(es),
        _lib.ptr(scales_mat), scales_mat.stride(0), _lib.ptr(p["scale_table"]), p["scale_bound"], _lib.ptr(gct["cdf"]),
        gct["T"], gct["W"], _lib.ptr(gct["cdf_len"]), _lib.ptr(gct["offset"]), _lib.ptr(z_hat), _lib.ptr(st),
        _lib.stream_ptr())
    _lib.check(rc, "lla_gaussian_decode_dequantise")
    torch.cuda.synchronize()
    return z_hat, st


def cond_gather(model, payload, offsets, prefix, first, step, N, index, bias, es, scales_mat, C, dtype=torch.float32,
                ld=None, shift=0, status_in=None):
    """lla_gaussian_decode_gather -> (out [B, ld] prefilled with SENTINEL, status).  ``scales_mat`` holds one row per
    OUTPUT row; ``shift`` moves the output's base address by that many elements."""
    from lossyless_amd import _lib
    gct, p = model.gaussian_conditional.device_tables(), model._device_params()
    idx = _idx(index)
    B = idx.numel()
    ld = C if ld is None else ld
    flat = torch.full((B * ld + shift,), SENTINEL, dtype=dtype, device="cuda")
    out = flat[shift:].view(B, ld)
    st = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().lla_gaussian_decode_gather(
        _lib.ptr(payload), _lib.ptr(offsets), prefix, first, step, N, _lib.ptr(idx), B, C, _lib.ptr(bias), _lib.ptr(es),
        _lib.ptr(scales_mat), scales_mat.stride(0), _lib.ptr(p["scale_table"]), p["scale_bound"], _lib.ptr(gct["cdf"]),
        gct["T"], gct["W"], _lib.ptr(gct["cdf_len"]), _lib.ptr(gct["offset"]), _lib.ptr(out),
        _lib.LLA_Z_F32 if dtype == torch.float32 else _lib.LLA_Z_F16, ld, _lib.ptr(status_in), _lib.ptr(st),
        _lib.stream_ptr())
    _lib.check(rc, "lla_gaussian_decode_gather")
    torch.cuda.synchronize()
    assert shift == 0 or float(flat[0]) == SENTINEL
    return out, st


def hand_built(model, B, C, seed):
    """z, affine and a scales matrix with a leading dimension of 2C + 8 whose leading C columns hold ties on table
    entries, values at / below the bound, values above the table and one-ulp neighbours, then log-normal scales; some
    z far outside every window (escapes).  C >= 24."""
    g = torch.Generator().manual_seed(seed)
    gc = model.gaussian_conditional
    table = gc.scale_table.detach().float().cpu()
    bound = float(gc.scale_bound)
    special = torch.tensor([bound, bound / 2, 0.0, -3.0, 1e-30, -0.0, float(table[-1]) * 1.0001, 300.0, 1e4, 2e5,
                            float(torch.nextafter(table[5], torch.tensor(0.0))),
                            float(torch.nextafter(table[40], torch.tensor(0.0)))])
    n_ties = min(len(table), C - len(special) - 4)
    ties = table[torch.linspace(0, len(table) - 1, n_ties).round().long()]
    scales = torch.exp(torch.randn(B, C, generator=g) * 2.5)
    scales[:, :n_ties] = ties[None, :]
    scales[:, n_ties:n_ties + len(special)] = special[None, :]
    mat = torch.randn(B, 2 * C + 8, generator=g)
    mat[:, :C] = scales
    z = torch.randn(B, C, generator=g) * 3
    z[:, C - 1], z[:, C - 2], z[:, n_ties] = 5000.0, -60000.0, 40.0
    bias = (torch.randn(C, generator=g) * 0.1).cuda()
    es = torch.exp(torch.randn(C, generator=g).double() * 0.2).float().cuda()
    return z.cuda().contiguous(), bias, es, mat.cuda()


def encode_rows(model, z, bias, es, scales_mat, C):
    """lla_gaussian_quantise_encode + compaction WITHOUT length prefixes -> (padded payload, int64 offsets [B+1])."""
    from lossyless_amd import _lib
    from lossyless_amd.entropy import EntropyBottleneck
    L = _lib.lib()
    gct, p = model.gaussian_conditional.device_tables(), model._device_params()
    B = z.shape[0]
    stride = int(L.lla_rans_max_encoded_bytes(C))
    scratch = torch.empty(B * stride, dtype=torch.uint8, device="cuda")
    lengths = torch.empty(B, dtype=torch.int32, device="cuda")
    rc = L.lla_gaussian_quantise_encode(
        _lib.ptr(z), _lib.LLA_Z_F32, B, C, _lib.ptr(bias), _lib.ptr(es), _lib.ptr(scales_mat), scales_mat.stride(0),
        _lib.ptr(p["scale_table"]), p["scale_bound"], _lib.ptr(gct["cdf"]), gct["T"], gct["W"], _lib.ptr(gct["cdf_len"]),
        _lib.ptr(gct["offset"]), _lib.ptr(scratch), stride, _lib.ptr(lengths), None, None, _lib.stream_ptr())
    _lib.check(rc, "lla_gaussian_quantise_encode")
    payload, offsets = EntropyBottleneck.compact_device(scratch, stride, lengths, B)
    total = int(offsets[-1])
    return torch.cat([payload[:total], torch.zeros(8, dtype=torch.uint8, device="cuda")]), offsets.to(torch.int64)
