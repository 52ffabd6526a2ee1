"""GPU: the three conditional entry points with the predicted means (lla_gaussian_quantise_encode_means,
lla_gaussian_decode_dequantise_means, lla_gaussian_decode_gather_means) against the CPU oracle, bit for bit, their tie to
the entry points without means, and ``coded_means="predicted"`` through the compressor, the container and a fit."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gc

pytestmark = pytest.mark.gpu

SENTINEL = -123.25
BOUND = 0.11
F32 = np.float32


@pytest.fixture(scope="module")
def tables():
    return gc.derive_tables(gc.get_scale_table())


@pytest.fixture(scope="module")
def dev_tables(tables):
    d = {k: torch.from_numpy(np.ascontiguousarray(tables[k])).cuda() for k in ("cdf", "cdf_len", "offset", "scale_table")}
    d["T"], d["W"] = tables["cdf"].shape
    return d


# ------------------------------------------------------------------------------------------------------------ the cases
def _case(B, C, half, seed):
    """z, affine, scales and means (numpy, fp32 but z) with every case the kernels must get right: scales below the bound and
    past the table (columns 2, 3), negative means, means that push z_in - mean out of the window on either side (escapes), and exact ties
    z_in - mean = k + 0.5 for even and odd k (columns 2, 3: zero bias, unit scale, values exact in fp16)."""
    rng = np.random.default_rng(seed)
    bias = (rng.normal(size=C) * 0.1).astype(F32)
    es = np.exp(rng.normal(size=C) * 0.2).astype(F32)
    scales = np.exp(rng.normal(size=(B, C)) * 2.5).astype(F32)
    means = (rng.normal(size=(B, C)) * 30).astype(F32)
    z = (rng.normal(size=(B, C)) * 3).astype(np.float16 if half else F32)
    scales[:, 0:2] = 0.2
    means[:, 0], means[:, 1] = 3000.0, -70000.0                   # z_in - mean far below / above the narrow window
    bias[2:4], es[2:4] = 0.0, 1.0
    scales[:, 2], scales[:, 3] = 0.01, 1e4                        # ... coded with the first row (below the bound) and the last
    means[:, 2:4] = -7.25
    z[:, 2], z[:, 3] = -4.75, -3.75                               # z_in - mean = 2.5 (-> 2) and 3.5 (-> 4)
    if B > 1:
        z[1, 2], z[1, 3] = -9.75, -10.75                          # -2.5 (-> -2) and -3.5 (-> -4)
    return z, bias, es, scales, means


def _layout(scales, means, packed):
    """-> (scales tensor, means address, ld_scales, ld_means, keep-alive): ``packed`` is the caller's layout, one [B, 2C] matrix
    with means = scales + C and ld = 2C; otherwise two dense [B, C] arrays."""
    B, C = scales.shape
    if packed:
        mat = torch.from_numpy(np.concatenate([scales, means], axis=1)).cuda()
        return mat, ctypes.c_void_p(mat.data_ptr() + 4 * C), 2 * C, 2 * C, mat
    s, m = torch.from_numpy(scales.copy()).cuda(), torch.from_numpy(means.copy()).cuda()
    return s, ctypes.c_void_p(m.data_ptr()), C, C, m


def _reference(z, bias, es, scales, means, tables):
    z_in = (z.astype(F32) + bias) * es                            # one fp32 rounding per operation
    idx = gc.build_indexes(scales, tables["scale_table"], BOUND)
    sym = gc.symbols_of(z_in, means)
    strings = gc.compress(sym, idx, tables)
    z_hat = (sym.astype(F32) + means) / es - bias
    return z_in, idx, sym, strings, z_hat


# ------------------------------------------------------------------------------------------------------------ the callers
def _records(payload, offsets):
    off = offsets.cpu().numpy()
    blob = payload[: int(off[-1])].cpu().numpy().tobytes()
    return [blob[int(off[r]):int(off[r + 1])] for r in range(len(off) - 1)]


def _upload(strings):
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    blob = np.frombuffer(b"".join(strings) + b"\0" * 8, dtype=np.uint8).copy()
    return torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda()


def _encode(t, z, bias, es, sc, ld_s, mean_args):
    """``mean_args``: () for lla_gaussian_quantise_encode, (means address, ld_means) for the _means entry point.
    -> (rc, strings, symbols, indexes)."""
    from lossyless_amd import _lib
    from lossyless_amd.entropy import EntropyBottleneck
    L = _lib.lib()
    B, C = z.shape
    stride = int(L.lla_rans_max_encoded_bytes(C))
    scratch = torch.zeros(B * stride, dtype=torch.uint8, device="cuda")
    lengths = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    sym = torch.full((B, C), -7, dtype=torch.int32, device="cuda")
    idx = torch.full((B, C), -7, dtype=torch.int32, device="cuda")
    fn = L.lla_gaussian_quantise_encode_means if mean_args else L.lla_gaussian_quantise_encode
    rc = fn(_lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, B, C, _lib.ptr(bias), _lib.ptr(es),
            _lib.ptr(sc), ld_s, *mean_args, _lib.ptr(t["scale_table"]), BOUND, _lib.ptr(t["cdf"]), t["T"], t["W"],
            _lib.ptr(t["cdf_len"]), _lib.ptr(t["offset"]), _lib.ptr(scratch), stride, _lib.ptr(lengths), _lib.ptr(sym),
            _lib.ptr(idx), _lib.stream_ptr())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, lengths, sym, idx
    return rc, _records(*EntropyBottleneck.compact_device(scratch, stride, lengths, B)), sym, idx


def _decode(t, payload, offsets, B, C, bias, es, sc, ld_s, mean_args):
    from lossyless_amd import _lib
    L = _lib.lib()
    z_hat = torch.full((B, C), SENTINEL, dtype=torch.float32, device="cuda")
    st = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    fn = L.lla_gaussian_decode_dequantise_means if mean_args else L.lla_gaussian_decode_dequantise
    rc = fn(_lib.ptr(payload), _lib.ptr(offsets), 0, 0, 1, B, C, _lib.ptr(bias), _lib.ptr(es), _lib.ptr(sc), ld_s, *mean_args,
            _lib.ptr(t["scale_table"]), BOUND, _lib.ptr(t["cdf"]), t["T"], t["W"], _lib.ptr(t["cdf_len"]), _lib.ptr(t["offset"]),
            _lib.ptr(z_hat), _lib.ptr(st), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, z_hat, st


def _gather(t, payload, offsets, N, index, C, bias, es, sc, ld_s, mean_args, dtype, ld_out, status_in=None):
    from lossyless_amd import _lib
    L = _lib.lib()
    B = index.numel()
    out = torch.full((B, ld_out), SENTINEL, dtype=dtype, device="cuda")
    st = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    fn = L.lla_gaussian_decode_gather_means if mean_args else L.lla_gaussian_decode_gather
    rc = fn(_lib.ptr(payload), _lib.ptr(offsets), 0, 0, 1, N, _lib.ptr(index), B, C, _lib.ptr(bias), _lib.ptr(es), _lib.ptr(sc),
            ld_s, *mean_args, _lib.ptr(t["scale_table"]), BOUND, _lib.ptr(t["cdf"]), t["T"], t["W"], _lib.ptr(t["cdf_len"]),
            _lib.ptr(t["offset"]), _lib.ptr(out), _lib.LLA_Z_F32 if dtype == torch.float32 else _lib.LLA_Z_F16, ld_out,
            _lib.ptr(status_in), _lib.ptr(st), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out, st


# ------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("packed", [True, False], ids=["means=scales+C", "separate"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("C", [5, 68, 130])
@pytest.mark.parametrize("B", [1, 33, 257])
def test_means_entry_points_against_the_oracle(tables, dev_tables, B, C, half, packed):
    t = dev_tables
    z, bias, es, scales, means = _case(B, C, half, seed=1000 * B + 10 * C + half)
    z_in, idx, sym, strings, z_hat = _reference(z, bias, es, scales, means, tables)
    # the case holds what it is meant to hold
    lo, n = tables["offset"][idx], tables["cdf_len"][idx] - 2
    assert (sym[:, 0] < lo[:, 0]).all() and (sym[:, 1] - lo[:, 1] >= n[:, 1]).all() and (means < 0).any()
    assert sym[0, 2] == 2 and sym[0, 3] == 4 and (B == 1 or (sym[1, 2] == -2 and sym[1, 3] == -4))
    assert (z_in[:, 2:4] - means[:, 2:4] - np.floor(z_in[:, 2:4] - means[:, 2:4]) == 0.5).all()
    assert idx.min() == 0 and idx.max() == 63
    zd, bd, ed = torch.from_numpy(z).cuda(), torch.from_numpy(bias).cuda(), torch.from_numpy(es).cuda()
    sc, mp, ld_s, ld_m, _keep = _layout(scales, means, packed)
    if packed and C % 4:
        assert sc.data_ptr() % 16 == 0 and mp.value % 16 != 0      # the two row pointers are aligned differently

    # 1. encode
    rc, got, gsym, gidx = _encode(t, zd, bd, ed, sc, ld_s, (mp, ld_m))
    assert rc == 0
    assert np.array_equal(gidx.cpu().numpy(), idx) and np.array_equal(gsym.cpu().numpy(), sym)
    assert got == strings

    # 2. decode
    payload, offsets = _upload(strings)
    rc, back, st = _decode(t, payload, offsets, B, C, bd, ed, sc, ld_s, (mp, ld_m))
    assert rc == 0 and int(st.abs().max()) == 0
    assert np.array_equal(back.cpu().numpy().view(np.uint32), z_hat.view(np.uint32))

    # 3. gather: shuffled with repeats, one row out of range on either side, one row with status_in set
    rng = np.random.default_rng(B + C)
    index = np.concatenate([rng.permutation(B), rng.integers(0, B, size=5)]).astype(np.int64)
    Bo = index.size
    bad_lo, bad_hi, dead = 1, Bo - 2, Bo - 1
    rows = index.copy()
    index[bad_lo], index[bad_hi] = -1, B
    status_in = torch.zeros(Bo, dtype=torch.int32, device="cuda")
    status_in[dead] = 7
    gsc, gmp, gld_s, gld_m, _keep2 = _layout(scales[rows], means[rows], packed)
    idx_d = torch.from_numpy(index).cuda()
    ok = np.ones(Bo, dtype=bool)
    ok[[bad_lo, bad_hi, dead]] = False
    want_st = np.zeros(Bo, dtype=np.int32)
    want_st[[bad_lo, bad_hi]], want_st[dead] = 2, 7
    want = np.where(ok[:, None], z_hat[rows], F32(0))
    for dtype, cast in ((torch.float32, F32), (torch.float16, np.float16)):
        rc, out, st = _gather(t, payload, offsets, B, idx_d, C, bd, ed, gsc, gld_s, (gmp, gld_m), dtype, C + 3, status_in)
        assert rc == 0 and np.array_equal(st.cpu().numpy(), want_st)
        o = out.cpu().numpy()
        assert (o[:, C:] == cast(SENTINEL)).all()                                      # pad columns untouched
        w = want.astype(cast)                                                          # (numpy rounds to nearest even)
        bits = np.uint32 if cast is F32 else np.uint16
        assert np.array_equal(o[:, :C].view(bits), w.view(bits))

    # 4. means == scales, ld_means == ld_scales: the bytes and values of the entry points without means
    sp = ctypes.c_void_p(sc.data_ptr())
    rc0, s0, sym0, idx0 = _encode(t, zd, bd, ed, sc, ld_s, ())
    rc1, s1, sym1, idx1 = _encode(t, zd, bd, ed, sc, ld_s, (sp, ld_s))
    assert rc0 == rc1 == 0 and s0 == s1 and torch.equal(sym0, sym1) and torch.equal(idx0, idx1)
    assert s0 != strings                                                               # (and the means do matter)
    p0, o0 = _upload(s0)
    rc0, d0, st0 = _decode(t, p0, o0, B, C, bd, ed, sc, ld_s, ())
    rc1, d1, st1 = _decode(t, p0, o0, B, C, bd, ed, sc, ld_s, (sp, ld_s))
    assert rc0 == rc1 == 0 and torch.equal(st0, st1) and int(st0.abs().max()) == 0
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32))
    gsp = ctypes.c_void_p(gsc.data_ptr())
    live = torch.from_numpy(rows).cuda()
    for dtype in (torch.float32, torch.float16):
        rc0, g0, gs0 = _gather(t, p0, o0, B, live, C, bd, ed, gsc, gld_s, (), dtype, C + 3)
        rc1, g1, gs1 = _gather(t, p0, o0, B, live, C, bd, ed, gsc, gld_s, (gsp, gld_s), dtype, C + 3)
        assert rc0 == rc1 == 0 and torch.equal(gs0, gs1) and int(gs0.abs().max()) == 0
        assert torch.equal(g0.view(torch.int16), g1.view(torch.int16))
        if dtype == torch.float32:
            assert torch.equal(g0[:, :C], d0[live])


def test_means_argument_checks_launch_nothing(tables, dev_tables):
    t, B, C = dev_tables, 9, 12
    z, bias, es, scales, means = _case(B, C, False, seed=5)
    _, _, _, strings, _ = _reference(z, bias, es, scales, means, tables)
    zd, bd, ed = torch.from_numpy(z).cuda(), torch.from_numpy(bias).cuda(), torch.from_numpy(es).cuda()
    sc, mp, ld_s, ld_m, _keep = _layout(scales, means, False)
    payload, offsets = _upload(strings)
    index = torch.arange(B, dtype=torch.int64, device="cuda")
    for bad in ((None, ld_m), (mp, C - 1), (mp, 0)):
        rc, lengths, sym, idx = _encode(t, zd, bd, ed, sc, ld_s, bad)
        assert rc == -1 and bool((lengths == -1).all()) and bool((sym == -7).all()) and bool((idx == -7).all())
        rc, z_hat, st = _decode(t, payload, offsets, B, C, bd, ed, sc, ld_s, bad)
        assert rc == -1 and bool((z_hat == SENTINEL).all()) and bool((st == -7).all())
        rc, out, st = _gather(t, payload, offsets, B, index, C, bd, ed, sc, ld_s, bad, torch.float32, C)
        assert rc == -1 and bool((out == SENTINEL).all()) and bool((st == -7).all())
    assert _encode(t, zd, bd, ed, sc, ld_s, (mp, ld_m))[0] == 0        # (the same calls with good arguments go through)


def test_gather_means_lds_query_is_a_sibling(dev_tables):
    """The query of the entry point without means answers what it answered; the sibling reports the two mean buffers
    (2 x 256 rows x 16 channels x 4 bytes) in front of the packed rows."""
    from lossyless_amd import _lib
    L, t = _lib.lib(), dev_tables
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for C in (5, 68, 512):
        for dt in (_lib.LLA_Z_F32, _lib.LLA_Z_F16):
            g0 = L.lla_gaussian_decode_gather_lds_bytes(C, t["T"], t["W"], dt, ctypes.byref(a))
            g1 = L.lla_gaussian_decode_gather_means_lds_bytes(C, t["T"], t["W"], dt, ctypes.byref(b))
            head = (8 * C + 4 * t["T"] + 7) // 8 * 8
            assert a.value == (head + 15) // 16 * 16 + 16 + 3 * 16384 and b.value == a.value + 2 * 16384
            assert g0 >= a.value and g1 >= b.value
    assert L.lla_gaussian_decode_gather_means_lds_bytes(0, t["T"], t["W"], _lib.LLA_Z_F32, None) == 0


# ------------------------------------------------------------------------------------------------------------ the dataset
def test_dataset_round_trip_and_random_access_in_the_new_mode(tmp_path):
    import hubconf
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    sd = synthetic_hyperprior_state_dict(0)
    comp, _ = hubconf.clip_hyperprior_compressor(sd, device="cuda", clip_weights="synthetic", coded_means="predicted")
    ref, _ = hubconf.clip_hyperprior_compressor(sd, device="cuda", clip_weights="synthetic")
    assert comp.hyperprior.coded_means == "predicted" and ref.hyperprior.coded_means == "scales"
    with pytest.raises(ValueError):
        hubconf.clip_hyperprior_compressor(sd, device="cuda", clip_weights="synthetic", coded_means="means")
    images = torch.randn(64, 3, 224, 224, generator=torch.Generator().manual_seed(0))
    f, f0 = tmp_path / "predicted.bin", tmp_path / "scales.bin"
    comp.compress_dataset(images, str(f), is_info=False)
    ref.compress_dataset(images, str(f0), is_info=False)
    assert f.read_bytes() != f0.read_bytes()
    Z = comp.decompress_dataset(str(f), is_info=False)
    with torch.no_grad():
        want = comp(images.cuda())
    assert tuple(Z.shape) == (64, 512) and np.array_equal(Z.view(np.uint32), want.float().cpu().numpy().view(np.uint32))
    # the string entry points and the rate agree with each other and with forward
    x9 = images[:9].cuda()
    strings = comp.compress(x9)
    with torch.no_grad():
        assert torch.equal(comp.decompress(strings), comp(x9))
    assert comp.get_rate(x9) == 8 * sum(len(s) for pair in strings for s in pair) / 9
    # random access
    ds = comp.open_dataset(str(f))
    idx = torch.randperm(64, generator=torch.Generator().manual_seed(1))[:40]
    idx[3] = idx[7]
    got = ds.take(idx)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), Z[idx.numpy()].view(np.uint32))
    assert torch.equal(ds.take(idx, dtype=torch.float16), torch.from_numpy(Z[idx.numpy()]).cuda().half())
    assert torch.equal(ds.all(), torch.from_numpy(Z).cuda())
    assert ds.lds_report()["front"] == ref.open_dataset(str(f0)).lds_report()["front"] + 2 * 16384
    # the file does not say which mode wrote it: the other mode decodes other values (or finds a record malformed)
    try:
        assert not np.array_equal(ref.decompress_dataset(str(f), is_info=False), Z)
    except ValueError:
        pass


# ------------------------------------------------------------------------------------------------------------ the rate
def test_coding_with_the_predicted_means_takes_fewer_bits_after_a_fit():
    """The end-to-end fit of DESIGN.md 5.20 (C = 64, 8192 rows, 5 epochs of 32 steps, beta = 1e-1, seed 0), its 2048 held-out
    rows coded in both modes with the same state dict."""
    from lossyless_amd import HyperpriorFit
    from lossyless_amd.rates import HRateHyperprior
    g = torch.Generator().manual_seed(0)
    Z = (torch.exp(0.7 * torch.randn(8192 + 2048, 1, generator=g)) * torch.randn(8192 + 2048, 64, generator=g)).cuda()
    fit = HyperpriorFit(1e-1, epochs=5, batch_size=256, scheduler=None, seed=0).fit(Z[:8192])
    held, sd, m = Z[8192:], fit.state_dict(), fit.rate_estimator_

    def coder(mode):
        c = HRateHyperprior(64, side_z_dim=m.side_z_dim, coded_means=mode, kwargs_ent_bottleneck=m.kwargs_ent_bottleneck)
        c.load_state_dict(sd, strict=False)
        c.update()
        return c.cuda().eval()

    def bits(c):
        payload, offsets = c.encode_device(held)
        assert torch.equal(c.decode_device(payload, offsets, held.shape[0]), c.represent_device(held))
        return 8.0 * float(offsets[-1]) / held.shape[0]

    bits_fit = 8.0 * float(m.encode_device(held)[1][-1]) / held.shape[0]
    bits_scales, bits_predicted = bits(coder("scales")), bits(coder("predicted"))
    print(f"bits per row (records with their length prefixes): coded_means=scales {bits_scales:.1f}, predicted "
          f"{bits_predicted:.1f}; training-rate estimate of the last epoch {fit.rate_curve_[-1]:.1f} "
          f"(side {fit.side_rate_curve_[-1]:.1f})")
    assert bits_scales == bits_fit                    # the default mode is the fitted module's own coder
    assert bits_predicted < bits_scales
