"""GPU: the hyperprior dataset path.  The yardstick throughout is the unchanged host-round-trip path --
``GaussianConditional.compress / decompress``, ``HRateHyperprior.compress / decompress`` -- which tests/test_gpu_gaussian.py
ties to the CPU oracle; everything here must give the same bytes and the same values, bit for bit."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from lossyless_amd.rates import HRateHyperprior, synthetic_hyperprior_state_dict
    m = HRateHyperprior(512).eval()
    m.load_state_dict(synthetic_hyperprior_state_dict(0))
    return m.cuda()


@pytest.fixture(scope="module")
def comp():
    import hubconf
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    c, _ = hubconf.clip_hyperprior_compressor(synthetic_hyperprior_state_dict(0), device="cuda", clip_weights="synthetic")
    return c


def _records(payload, offsets, prefix):
    off = offsets.cpu().numpy()
    blob = payload[: int(off[-1])].cpu().numpy().tobytes()
    return [blob[int(off[r]) + prefix:int(off[r + 1])] for r in range(len(off) - 1)]


def _upload(strings):
    lens = np.fromiter((len(s) for s in strings), dtype=np.int64, count=len(strings))
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    blob = np.frombuffer(b"".join(strings) + b"\0\0\0\0", dtype=np.uint8).copy()
    return torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda()


def _gaussian_encode(model, z, bias, es, scales_mat, C, want_out=True):
    from lossyless_amd import _lib
    from lossyless_amd.entropy import EntropyBottleneck
    L = _lib.lib()
    gct, p = model.gaussian_conditional.device_tables(), model._device_params()
    B = z.shape[0]
    stride = int(L.lla_rans_max_encoded_bytes(C))
    scratch = torch.empty(B * stride, dtype=torch.uint8, device="cuda")
    lengths = torch.empty(B, dtype=torch.int32, device="cuda")
    sym = torch.full((B, C), -7, dtype=torch.int32, device="cuda") if want_out else None
    idx = torch.full((B, C), -7, dtype=torch.int32, device="cuda") if want_out else None
    rc = L.lla_gaussian_quantise_encode(
        _lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, B, C, _lib.ptr(bias), _lib.ptr(es),
        _lib.ptr(scales_mat), scales_mat.stride(0), _lib.ptr(p["scale_table"]), p["scale_bound"], _lib.ptr(gct["cdf"]),
        gct["T"], gct["W"], _lib.ptr(gct["cdf_len"]), _lib.ptr(gct["offset"]), _lib.ptr(scratch), stride,
        _lib.ptr(lengths), _lib.ptr(sym), _lib.ptr(idx), _lib.stream_ptr())
    _lib.check(rc, "lla_gaussian_quantise_encode")
    payload, offsets = EntropyBottleneck.compact_device(scratch, stride, lengths, B)
    return _records(payload, offsets, 0), sym, idx


def _gaussian_decode(model, payload, offsets, prefix, first, step, B, bias, es, scales_mat, C):
    from lossyless_amd import _lib
    gct, p = model.gaussian_conditional.device_tables(), model._device_params()
    z_hat = torch.full((B, C), float("nan"), dtype=torch.float32, device="cuda")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    rc = _lib.lib().lla_gaussian_decode_dequantise(
        _lib.ptr(payload), _lib.ptr(offsets), prefix, first, step, B, C, _lib.ptr(bias), _lib.ptr(es),
        _lib.ptr(scales_mat), scales_mat.stride(0), _lib.ptr(p["scale_table"]), p["scale_bound"], _lib.ptr(gct["cdf"]),
        gct["T"], gct["W"], _lib.ptr(gct["cdf_len"]), _lib.ptr(gct["offset"]), _lib.ptr(z_hat), _lib.ptr(status),
        _lib.stream_ptr())
    _lib.check(rc, "lla_gaussian_decode_dequantise")
    return z_hat, status


def _kernel_inputs(model, B, C, dtype, seed):
    """z, affine and a scales matrix with a leading dimension, holding every boundary case of the issue."""
    g = torch.Generator().manual_seed(seed)
    gc = model.gaussian_conditional
    table = gc.scale_table.detach().float().cpu()
    bound = float(gc.scale_bound)
    bias = (torch.randn(C, generator=g) * 0.1).cuda()
    es = torch.exp(torch.randn(C, generator=g).double() * 0.2).float().cuda()
    mat = torch.randn(B, 2 * C + 8, generator=g)                 # (scales are its leading C columns: ld = 2C + 8)
    scales = torch.exp(torch.randn(B, C, generator=g) * 2.5)
    scales[:, 0:64] = table[None, :]                             # exactly on the table values: the `<=` tie
    scales[:, 64:70] = torch.tensor([bound, bound / 2, 0.0, -3.0, 1e-30, -0.0])       # at / below the bound (mean < bound)
    scales[:, 70:74] = torch.tensor([float(table[-1]) * 1.0001, 300.0, 1e4, 2e5])  # above the last entry
    scales[:, 74:76] = torch.nextafter(table[[5, 40]], torch.tensor(0.0))             # one ulp under a table value
    mat[:, :C] = scales
    z = torch.randn(B, C, generator=g) * 3
    z[:, 100] = 5000.0                                           # |z_in - mean| far outside every window: escapes
    z[:, 101] = -60000.0
    z[:, 64] = 40.0                                              # ... and outside the narrowest row (scale = bound)
    mat[:, 100], mat[:, 101] = 0.2, 1.0
    return z.to(dtype).cuda().contiguous(), bias, es, mat.cuda()


@pytest.mark.parametrize("B,C,dtype", [(1, 512, torch.float32), (257, 512, torch.float32), (1024, 512, torch.float32),
                                       (1, 512, torch.float16), (257, 512, torch.float16), (1024, 512, torch.float16),
                                       (257, 509, torch.float16), (67, 510, torch.float32)])
def test_fused_gaussian_kernels_equal_the_gaussian_conditional_path(model, B, C, dtype):
    gc = model.gaussian_conditional
    z, bias, es, mat = _kernel_inputs(model, B, C, dtype, seed=B + C)
    scales = mat[:, :C]
    z_in = (z.float() + bias) * es                               # process_z_in (rates.py:434-435)
    idx_ref = gc.build_indexes(scales)
    sym_ref = torch.round(z_in - scales).to(torch.int32)
    want = gc.compress(z_in, idx_ref, means=scales)
    assert idx_ref.unique().numel() >= 32 and bool((scales < float(gc.scale_bound)).any())
    esc = (sym_ref < gc._offset[idx_ref.long()]) | (sym_ref - gc._offset[idx_ref.long()] >= gc._cdf_length[idx_ref.long()] - 2)
    assert bool(esc.any()) and bool((~esc).any())

    got, sym, idx = _gaussian_encode(model, z, bias, es, mat, C)
    assert torch.equal(idx, idx_ref) and torch.equal(sym, sym_ref)
    assert got == want
    assert _gaussian_encode(model, z, bias, es, mat, C, want_out=False)[0] == want      # outputs are optional

    payload, offsets = _upload(want)
    z_hat, status = _gaussian_decode(model, payload, offsets, 0, 0, 1, B, bias, es, mat, C)
    assert int(status.abs().max()) == 0
    back = gc.decompress(want, idx_ref, means=scales)
    assert torch.equal(z_hat, (back / es) - bias)                # process_z_out (rates.py:437-438)


def test_compact_pairs_interleaves_and_reports_the_needed_size(model):
    from lossyless_amd import _lib
    L = _lib.lib()
    B = 1500
    g = torch.Generator().manual_seed(1)
    stride_a, stride_b = 64, 32
    la = (torch.randint(0, 17, (B,), generator=g) * 4).to(torch.int32)
    lb = (torch.randint(0, 9, (B,), generator=g) * 4).to(torch.int32)
    la[3], lb[3], lb[7] = 0, 0, 0
    sa = torch.randint(0, 256, (B * stride_a,), generator=g, dtype=torch.uint8)
    sb = torch.randint(0, 256, (B * stride_b,), generator=g, dtype=torch.uint8)
    want, offs = b"", [0]
    for i in range(B):
        for s, st, ln in ((sa, stride_a, int(la[i])), (sb, stride_b, int(lb[i]))):
            want += ln.to_bytes(4, "big") + s[(i + 1) * st - ln:(i + 1) * st].numpy().tobytes()
            offs.append(len(want))
    wsb = int(L.lla_rans_compact_pairs_workspace_bytes(B))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    dev = [t.cuda() for t in (sa, la, sb, lb)]      # (named: they must outlive the launches)

    def run(cap):
        out = torch.full((len(want) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        off = torch.empty(2 * B + 1, dtype=torch.int64, device="cuda")
        rc = L.lla_rans_compact_pairs(_lib.ptr(dev[0]), stride_a, _lib.ptr(dev[1]), _lib.ptr(dev[2]), stride_b,
                                      _lib.ptr(dev[3]), B, _lib.ptr(out), cap, _lib.ptr(off), _lib.ptr(ws), wsb,
                                      _lib.stream_ptr())
        _lib.check(rc, "lla_rans_compact_pairs")
        return out.cpu().numpy().tobytes(), off.cpu().numpy().tolist()

    out, off = run(len(want) + 64)
    assert off == offs and out[:len(want)] == want and set(out[len(want):]) == {0xEE}
    cap = offs[2001] + 2                       # record 2001 does not fit: nothing at or beyond it is written
    out, off = run(cap)
    assert off == offs and out[:offs[2001]] == want[:offs[2001]] and set(out[offs[2001]:]) == {0xEE}
    assert L.lla_rans_compact_pairs(None, 0, None, None, 0, None, B, None, 0, None, _lib.ptr(ws), 8, None) == -1


@pytest.mark.parametrize("B,dtype", [(1, torch.float32), (300, torch.float16), (1024, torch.float32)])
def test_encode_device_records_are_the_strings_of_compress(model, B, dtype):
    z = (torch.randn(B, 512, generator=torch.Generator().manual_seed(B)) * 0.7).to(dtype).cuda()
    z_strings, side_strings = model.compress(z)
    payload, offsets, sym = model.encode_device(z, want_symbols=True)
    assert payload.is_cuda and offsets.is_cuda and offsets.shape == (2 * B + 1,)
    rec = _records(payload, offsets, 4)
    assert rec[0::2] == z_strings and rec[1::2] == side_strings
    off = offsets.cpu().numpy()                                   # the prefixes are the big-endian lengths
    blob = payload[: int(off[-1])].cpu().numpy().tobytes()
    assert all(int.from_bytes(blob[int(off[r]):int(off[r]) + 4], "big") == len(rec[r]) for r in range(2 * B))
    p2, o2 = model.encode_device(z)
    assert torch.equal(o2, offsets) and torch.equal(p2[: int(off[-1])], payload[: int(off[-1])])
    # the side strings hold nothing beyond the symbols the encoder already had: decoding them gives sym + median
    med = model.entropy_bottleneck._medians().detach()
    s_hat = model.entropy_bottleneck.decompress(side_strings).reshape(B, -1)
    assert torch.equal(s_hat, sym["side_symbols"].float() + med[None, :])
    idx, means = model.get_indexes_means_hat(side_strings)
    assert torch.equal(idx.reshape(B, -1), sym["z_indexes"])
    assert torch.equal(torch.round(model.process_z_in(z) - means.reshape(B, -1)).int(), sym["z_symbols"])
    assert sym["z_indexes"].unique().numel() >= 32
    assert bool((means < float(model.gaussian_conditional.scale_bound)).any())
    # ... and decode_device / represent_device give what decompress gives
    want = model.decompress([z_strings, side_strings])
    padded = torch.cat([payload[: int(off[-1])], torch.zeros(4, dtype=torch.uint8, device="cuda")])
    assert torch.equal(model.decode_device(padded, offsets, B), want)
    assert torch.equal(model.represent_device(z), want)


def test_encode_device_reads_a_strided_view_as_its_values_and_checks_the_shape(model):
    wide = (torch.randn(33, 1024, generator=torch.Generator().manual_seed(5)) * 0.7).cuda()
    view = wide[:, 256:768]                                       # a column slice: row stride 1024, not dense
    assert not view.is_contiguous()
    p_ref, o_ref = model.encode_device(view.clone())
    p, o = model.encode_device(view)
    assert torch.equal(o, o_ref) and torch.equal(p[: int(o[-1])], p_ref[: int(o[-1])])
    for bad in (wide, wide[:, :511], wide[0, :512], wide[:, :512].reshape(33, 2, 256)):
        with pytest.raises(ValueError):
            model.encode_device(bad)
    with pytest.raises(ValueError):
        model.decode_device(p.int(), o, 33)


class _DS(torch.utils.data.Dataset):
    def __init__(self, x, y):
        self.x, self.y = x, y

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.y[i]


N_IMAGES = 1300


@pytest.fixture(scope="module")
def dataset(comp, tmp_path_factory):
    """1300 synthetic images + labels, their file, and the strings of the unchanged ``HRateHyperprior.compress``."""
    from lossyless_amd.compressor import SyntheticImages
    x = SyntheticImages(N_IMAGES, seed=11).device_batch(0, N_IMAGES, "cuda")
    y = (torch.arange(N_IMAGES) * 7) % 1000
    z = torch.cat([comp.clip(x[i:i + 500]) for i in range(0, N_IMAGES, 500)])
    z_strings, side_strings = comp.hyperprior.compress(z)
    d = tmp_path_factory.mktemp("hyperprior")
    f, lf = d / "Z.bin", d / "Y.npy"
    comp.compress_dataset(_DS(x.cpu(), y), f, label_file=lf, kwargs_dataloader=dict(batch_size=96, num_workers=0),
                          is_info=False)
    return dict(x=x, y=y, z=z, z_strings=z_strings, side_strings=side_strings, file=f, label_file=lf, dir=d)


def test_compress_dataset_file_equals_the_python_assembly_for_two_batch_sizes(comp, dataset, capsys):
    from lossyless_amd.hyperprior_compressor import read_pair_container, write_pair_container
    buf = io.BytesIO()
    write_pair_container(buf, dataset["z_strings"], dataset["side_strings"])
    blob = dataset["file"].read_bytes()                 # batches of 96, ragged last one (1300 = 13 * 96 + 52)
    assert blob == buf.getvalue()
    assert int.from_bytes(blob[:4], "big") == 2 * N_IMAGES
    assert read_pair_container(dataset["file"]) == [dataset["z_strings"], dataset["side_strings"]]
    # other batches, the tower once per batch, two coding groups (1200 + 100 images): the same file
    f2 = dataset["dir"] / "Z2.bin"
    comp.compress_dataset(dataset["x"], f2, kwargs_dataloader=dict(batch_size=300), entropy_group=1, coalesce=0)
    out = capsys.readouterr().out
    assert f2.read_bytes() == blob
    assert f"Rate: {8 * len(blob) / N_IMAGES:.2f} bits/img | Encoding:" in out


def test_decompress_dataset_equals_forward_and_the_string_paths(comp, dataset):
    Z, Y = comp.decompress_dataset(dataset["file"], label_file=dataset["label_file"], is_info=False)
    assert Z.shape == (N_IMAGES, 512) and Z.dtype == np.float32 and Y.dtype == np.int64
    assert np.array_equal(Y, dataset["y"].numpy())
    assert np.array_equal(comp.decompress_dataset(dataset["file"], is_info=False, batch_size=500), Z)
    x = dataset["x"]
    fwd = torch.cat([comp(x[i:i + 500]) for i in range(0, N_IMAGES, 500)])
    assert fwd.dtype == torch.float32 and torch.equal(torch.from_numpy(Z).cuda(), fwd)
    strings = comp.compress(x[:200])
    assert strings == [dataset["z_strings"][:200], dataset["side_strings"][:200]]
    assert torch.equal(comp.decompress(strings), fwd[:200])
    assert torch.equal(comp.hyperprior.decompress([dataset["z_strings"], dataset["side_strings"]]), fwd)
    bits = 8 * (sum(map(len, strings[0])) + sum(map(len, strings[1]))) / 200
    assert comp.get_rate(x[:200]) == bits
    with pytest.raises(NotImplementedError):
        comp.decompress_dataset(dataset["file"], is_cpu=True)


def test_damaged_files_raise_and_do_not_fault(comp, dataset):
    from lossyless_amd.hyperprior_compressor import write_pair_container
    blob = dataset["file"].read_bytes()
    d = dataset["dir"]
    for k, cut in enumerate((2, 4, 4 + 2, len(blob) // 2 + 1, len(blob) - 4)):
        f = d / f"cut{k}.bin"
        f.write_bytes(blob[:cut])
        with pytest.raises(ValueError):
            comp.decompress_dataset(f, is_info=False)
    f = d / "odd.bin"                                    # an odd number of records is not a pair file
    f.write_bytes((2 * N_IMAGES - 1).to_bytes(4, "big") + blob[4:len(blob) - 4 - len(dataset["side_strings"][-1])])
    with pytest.raises(ValueError):
        comp.decompress_dataset(f, is_info=False)

    z, s = list(dataset["z_strings"][:300]), list(dataset["side_strings"][:300])
    good = comp.decompress([z, s])
    # a z record cut short: its image's status is set, decompress raises
    bad_z = list(z)
    bad_z[5] = bad_z[5][:8]
    body = b"".join(len(r).to_bytes(4, "big") + r for pair in zip(bad_z, s) for r in pair)
    off = np.zeros(601, dtype=np.int64)
    off[1:] = np.cumsum([4 + len(r) for pair in zip(bad_z, s) for r in pair])
    payload = torch.from_numpy(np.frombuffer(body + b"\0" * 4, dtype=np.uint8).copy()).cuda()
    m = comp.hyperprior
    params, _ = m._scales_of(m.encode_device(dataset["z"][:300], want_symbols=True)[2]["side_symbols"])
    p = m._device_params()
    z_hat, status = _gaussian_decode(m, payload, torch.from_numpy(off).cuda(), 1, 0, 2, 300, p["bias"], p["exp_scale"],
                                     params, 512)
    st = status.cpu().numpy()
    assert st[5] == 1 and st.sum() == 1
    keep = [i for i in range(300) if i != 5]
    assert torch.equal(z_hat[keep], good[keep])
    with pytest.raises(ValueError, match="malformed"):
        comp.decompress([bad_z, s])
    f = d / "short_record.bin"
    write_pair_container(f, bad_z, s)
    with pytest.raises(ValueError, match="malformed"):
        comp.decompress_dataset(f, is_info=False)
    # a record whose length is not whole words cannot be opened: status, not a misaligned read
    bad_z[5] = z[5][:-1]
    with pytest.raises(ValueError, match="malformed"):
        comp.decompress([bad_z, s])
    # flipped bytes inside z and side records: every read stays inside the record and the tables, so this either raises
    # or returns other values -- what it must not do is fault
    rng = np.random.default_rng(0)
    for which in (0, 1):
        pair = [list(z), list(s)]
        for i in rng.integers(0, 300, size=40):
            r = bytearray(pair[which][i])
            for j in rng.integers(0, len(r), size=6):
                r[j] ^= 0xFF
            pair[which][i] = bytes(r)
        try:
            out = comp.decompress(pair)
            assert out.shape == (300, 512)
        except ValueError:
            pass
    torch.cuda.synchronize()
    assert torch.equal(comp.decompress([z, s]), good)       # the device is fine afterwards
