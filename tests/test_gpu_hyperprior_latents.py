"""GPU: random access into hyperprior containers.  ``lla_rans_decode_gather_strided`` against
``lla_rans_decode_batch_strided`` + ``float() + median``, ``lla_gaussian_decode_gather`` against
``lla_gaussian_decode_dequantise`` over all records then ``[index]``, and ``HyperpriorLatents`` against
``decompress_dataset``.  Integer decode, the same separately rounded fp32 operations, the same GEMM calls => bit-exact."""
import numpy as np
import pytest
import torch

from hyperprior_latents_util import (SENTINEL, cond_gather, decode_all, encode_rows, hand_built, hyper_model, side_gather,
                                     side_symbols)

pytestmark = pytest.mark.gpu

N = 300


@pytest.fixture(scope="module")
def model():
    return hyper_model()


@pytest.fixture(scope="module")
def coded(model):
    """N seeded random embeddings through ``encode_device``; the side symbols, the scales of every image and the rows
    ``lla_gaussian_decode_dequantise`` gives for all N records -- computed once, left unchanged."""
    z = (torch.randn(N, 512, generator=torch.Generator().manual_seed(41)) * 0.7).cuda()
    payload, offsets = model.encode_device(z)
    total = int(offsets[-1])
    payload = torch.cat([payload[:total], torch.zeros(8, dtype=torch.uint8, device="cuda")])
    sym, st = side_symbols(model, payload, offsets, N)
    assert int(st.abs().max()) == 0
    params, ld = model._scales_of(sym)
    params = params.contiguous()
    p = model._device_params()
    rows, st = decode_all(model, payload, offsets, 1, 0, 2, N, p["bias"], p["exp_scale"], params, 512)
    assert int(st.abs().max()) == 0
    idx = model.gaussian_conditional.build_indexes(params[:, :512])
    assert idx.unique().numel() >= 32 and bool((params[:, :512] < float(model.gaussian_conditional.scale_bound)).any())
    med = model.entropy_bottleneck.device_tables()["median"]
    return dict(payload=payload, offsets=offsets, side_sym=sym, s_hat=sym.float() + med[None, :], params=params,
                rows=rows, bias=p["bias"], es=p["exp_scale"])


def _gather(model, coded, index, **kw):
    """lla_gaussian_decode_gather on the z records (0, 2) with the gathered rows of the scales matrix."""
    index = np.asarray(index, dtype=np.int64)
    safe = torch.from_numpy(np.clip(index, 0, N - 1)).cuda()
    scales = kw.pop("scales", None)
    if scales is None:
        scales = coded["params"][safe].contiguous()
    return cond_gather(model, kw.pop("payload", coded["payload"]), kw.pop("offsets", coded["offsets"]), 1, 0, 2, N, index,
                       coded["bias"], coded["es"], scales, 512, **kw)


# ------------------------------------------------------------------ strided gather of the side records
# The pitch: a row holds S = 102 side channels (max(10, 512 // 5)) and the entry point requires ld_out >= C, so a pitch of
# 40 cannot be used with this model.  Tested instead: 104, the padded K of z_encoder's first GEMM (what HyperpriorLatents
# passes: vector stores, two fill columns), and 142 = S + 40 (forty fill columns, no multiple of 4: scalar stores).
@pytest.mark.parametrize("ld", [104, 142])
def test_strided_gather_writes_s_hat_into_a_padded_matrix(model, coded, ld):
    S = model.side_z_dim
    assert S == 102 and ld >= S
    rng = np.random.default_rng(7)
    index = np.concatenate([rng.permutation(N), [0, 0, N - 1, N - 1, 17, 17, 17], [N - 1, 0]])
    out, st = side_gather(model, coded["payload"], coded["offsets"], N, index, ld)
    assert not st.any()
    want = coded["s_hat"][torch.from_numpy(index).cuda()]
    assert torch.equal(out[:, :S].view(torch.int32), want.view(torch.int32))
    assert (out[:, S:] == SENTINEL).all()


def test_strided_gather_flags_indices_out_of_range(model, coded):
    S = model.side_z_dim
    index = [5, -1, N, 2 ** 31, 7, 299]
    out, st = side_gather(model, coded["payload"], coded["offsets"], N, index, 104)
    assert st.tolist() == [0, 2, 2, 2, 0, 0]
    assert not out[1:4, :S].any() and (out[:, S:] == SENTINEL).all()
    assert torch.equal(out[[0, 4, 5], :S], coded["s_hat"][[5, 7, 299]])


# ------------------------------------------------------------------ gathered conditional decode
@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 700])
def test_conditional_gather_equals_decode_of_all_records_then_index(model, coded, B):
    index = np.random.default_rng(B).integers(0, N, size=B)        # with repeats
    want = coded["rows"][torch.from_numpy(index).cuda()]
    out, st = _gather(model, coded, index)
    assert not st.any() and torch.equal(out.view(torch.int32), want.view(torch.int32))
    out16, st = _gather(model, coded, index, dtype=torch.float16)
    assert not st.any() and torch.equal(out16.view(torch.int16), want.half().view(torch.int16))


@pytest.mark.parametrize("name", ["one record 256 times", "reversed"])
def test_conditional_gather_of_repeated_and_reversed_indices(model, coded, name):
    index = np.full(256, 123) if name.startswith("one") else np.arange(N - 1, -1, -1)
    out, st = _gather(model, coded, index)
    assert not st.any() and torch.equal(out, coded["rows"][torch.from_numpy(index).cuda()])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_conditional_gather_leaves_the_row_padding_alone(model, coded, dtype):
    index = np.random.default_rng(5).permutation(N)[:70]
    want = coded["rows"][torch.from_numpy(index).cuda()].to(dtype)
    out, st = _gather(model, coded, index, dtype=dtype, ld=520)
    assert not st.any() and torch.equal(out[:, :512], want) and (out[:, 512:] == SENTINEL).all()
    # a pitch and a base address that rule out vector stores take the scalar write-out: same values
    out, st = _gather(model, coded, index, dtype=dtype, ld=513, shift=1)
    assert not st.any() and torch.equal(out[:, :512], want) and (out[:, 512:] == SENTINEL).all()


@pytest.mark.parametrize("C,B", [(40, 70), (512, 257)])
def test_conditional_gather_with_hand_built_scales(model, C, B):
    """Ties on table entries, sub-bound values, values above the table, escapes; C = 40 is no multiple of the 16-channel
    group (the last group holds 8 channels) and its scales matrix has a pitch of 88."""
    z, bias, es, mat = hand_built(model, B, C, seed=B + C)
    gc = model.gaussian_conditional
    rows = gc.build_indexes(mat[:, :C])
    assert rows.unique().numel() >= 16 and int(rows.min()) == 0 and int(rows.max()) == len(gc.scale_table) - 1
    payload, offsets = encode_rows(model, z, bias, es, mat, C)
    want, st = decode_all(model, payload, offsets, 0, 0, 1, B, bias, es, mat, C)
    assert int(st.abs().max()) == 0
    index = np.random.default_rng(C).permutation(B)
    pick = torch.from_numpy(index).cuda()
    scales = mat[pick].contiguous()
    for ld, shift in ((C, 0), (C + 3, 0), (C + 8, 1)):
        out, st = cond_gather(model, payload, offsets, 0, 0, 1, B, index, bias, es, scales, C, ld=ld, shift=shift)
        assert not st.any() and torch.equal(out[:, :C].view(torch.int32), want[pick].view(torch.int32))
        assert (out[:, C:] == SENTINEL).all()
    # scales read through an unaligned base (the scalar loads)
    odd = torch.empty(scales.numel() + 1, device="cuda")[1:].view_as(scales).copy_(scales)
    out, st = cond_gather(model, payload, offsets, 0, 0, 1, B, index, bias, es, odd, C)
    assert not st.any() and torch.equal(out.view(torch.int32), want[pick].view(torch.int32))


# ------------------------------------------------------------------ statuses
def test_conditional_gather_flags_indices_out_of_range(model, coded):
    index = [5, -1, N, 2 ** 31, 7, 299]
    out, st = _gather(model, coded, index)
    assert st.tolist() == [0, 2, 2, 2, 0, 0] and not out[1:4].any()
    assert torch.equal(out[[0, 4, 5]], coded["rows"][[5, 7, 299]])


def test_conditional_gather_flags_a_truncated_z_record_and_keeps_its_neighbours(model, coded):
    rows = coded["rows"]
    body = coded["payload"].clone()                              # private copies: the shared fixture stays as it is
    for keep_words, what in ((1, "cannot be opened"), (2, "opens, then overruns")):
        cut = coded["offsets"].clone()
        cut[20] = cut[21] - 4 - 4 * keep_words                  # image 10's z record: a length prefix and 1 or 2 words
        index = [9, 10, 11, 10, 12]
        out, st = _gather(model, coded, index, payload=body, offsets=cut)
        assert st.tolist() == [0, 1, 0, 1, 0], what
        assert not out[1].any() and not out[3].any(), what
        assert torch.equal(out[[0, 2, 4]], rows[[9, 11, 12]]), what
    # a whole workgroup around the damaged record
    index = np.arange(N)
    out, st = _gather(model, coded, index, payload=body, offsets=cut)
    keep = [i for i in range(N) if i != 10]
    assert st[10] == 1 and int(st.sum()) == 1 and not out[10].any() and torch.equal(out[keep], rows[keep])


def test_status_in_is_copied_through_and_the_row_is_zeroed_without_a_read(model, coded):
    index = np.array([4, 2 ** 40, 6, 7, -9, 9], dtype=np.int64)  # rows 1 and 4 name no record at all ...
    status_in = torch.tensor([0, 1, 0, 7, 1, 0], dtype=torch.int32, device="cuda")
    out, st = _gather(model, coded, index, status_in=status_in)
    assert st.tolist() == [0, 1, 0, 7, 1, 0]                     # ... and get the side pass's status, not a 2
    assert not out[[1, 3, 4]].any() and torch.equal(out[[0, 2, 5]], coded["rows"][[4, 6, 9]])


# ------------------------------------------------------------------ HyperpriorLatents
class _DS(torch.utils.data.Dataset):
    def __init__(self, x, y):
        self.x, self.y = x, y

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.y[i]


@pytest.fixture(scope="module")
def comp():
    import hubconf
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    c, _ = hubconf.clip_hyperprior_compressor(synthetic_hyperprior_state_dict(0), device="cuda", clip_weights="synthetic")
    return c


@pytest.fixture(scope="module")
def dataset(comp, tmp_path_factory):
    from lossyless_amd.compressor import SyntheticImages
    x = SyntheticImages(N, seed=13).device_batch(0, N, "cuda")
    y = (torch.arange(N) * 7) % 1000
    d = tmp_path_factory.mktemp("hyperprior_latents")
    f, lf = d / "Z.bin", d / "Y.npy"
    comp.compress_dataset(_DS(x.cpu(), y), f, label_file=lf, kwargs_dataloader=dict(batch_size=96, num_workers=0),
                          is_info=False)
    ds = comp.open_dataset(f, label_file=lf)
    Z = torch.from_numpy(comp.decompress_dataset(f, is_info=False)).cuda()
    return dict(file=f, label_file=lf, dir=d, y=y, ds=ds, Z=Z)


def test_hyperprior_latents_equal_decompress_dataset(comp, dataset):
    from lossyless_amd import HyperpriorLatents
    ds, Z = dataset["ds"], dataset["Z"]
    assert isinstance(ds, HyperpriorLatents) and len(ds) == N and ds.device.type == "cuda"
    assert 0 < ds.nbytes < N * 512 * 4 / 2
    everything = ds.all()
    assert everything.is_cuda and everything.dtype == torch.float32 and torch.equal(everything, Z)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(2))
    assert torch.equal(ds.take(perm), Z[perm.cuda()])
    assert torch.equal(ds.take(perm, dtype=torch.float16), Z[perm.cuda()].half())
    assert torch.equal(ds.all(dtype=torch.float16), Z.half())
    a = ds.take([3, 4])
    assert a.data_ptr() != ds.take([5, 6]).data_ptr() and torch.equal(a, Z[3:5])      # not a cached buffer
    wide = torch.full((3, 520), SENTINEL, device="cuda")
    assert ds.take(np.array([0, 5, 2]), out=wide[:, :512]).data_ptr() == wide.data_ptr()
    assert torch.equal(wide[:, :512], Z[[0, 5, 2]]) and (wide[:, 512:] == SENTINEL).all()
    assert torch.equal(ds[11], Z[11]) and torch.equal(ds[5:290:7], Z[5:290:7]) and tuple(ds.take([]).shape) == (0, 512)
    assert torch.equal(ds.labels([4, 2, 299]).cpu(), dataset["y"][[4, 2, 299]])
    assert comp.open_dataset(dataset["file"], device="cuda").nbytes == ds.nbytes


def test_packed_rows_of_the_shipped_table_stay_in_lds(dataset):
    """The fallback to global-memory rows gives the same values, so only this shows it: the launch is granted enough
    dynamic LDS for the staging AND the packed rows of the 64-level table."""
    for dtype in (torch.float32, torch.float16):
        r = dataset["ds"].lds_report(dtype)
        assert r["front"] == 4352 + 16 + 3 * 16384 and r["packed_rows"] == 264 + 512 + 2 * 27256, r
        assert r["rows_in_lds"] and r["front"] + r["packed_rows"] <= r["granted"] <= 160 * 1024, r


def test_working_buffers_are_released(dataset):
    ds, Z = dataset["ds"], dataset["Z"]
    ds.take(torch.arange(10))
    assert ds.workspace_nbytes == 10 * (104 + 512 + 512 + 1024 + 2) * 4
    ds.release()
    assert ds.workspace_nbytes == 0 and torch.equal(ds.take([7, 8]), Z[7:9])
    for _ in ds.batches(128):
        assert ds.workspace_nbytes > 0
    assert ds.workspace_nbytes == 0                              # batches() frees them when the epoch ends


def test_hyperprior_latents_batches(dataset):
    ds, Z, y = dataset["ds"], dataset["Z"], dataset["y"]

    def run(**kw):
        return list(ds.batches(64, shuffle=True, generator=torch.Generator().manual_seed(3), **kw))

    small, large = run(decode_group=128), run()
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3))
    assert [tuple(z.shape) for z, _ in large] == [(64, 512)] * 4 + [(44, 512)] and len(small) == 5
    for k, ((za, ya), (zb, yb)) in enumerate(zip(small, large)):
        rows = perm[64 * k:64 * k + 64]
        assert torch.equal(za, zb) and torch.equal(ya, yb) and torch.equal(ya.cpu(), y[rows])
        assert torch.equal(zb, Z[rows.cuda()])
    assert len(run(drop_last=True)) == 4


def test_hyperprior_latents_statuses(comp, dataset):
    from lossyless_amd.hyperprior_compressor import read_pair_container, write_pair_container
    ds, Z, d = dataset["ds"], dataset["Z"], dataset["dir"]
    for bad in ([N], [-1], [0, 2 ** 40]):
        with pytest.raises(IndexError):
            ds.take(bad)
    out = ds.take([-1, 8, N], check=False)
    assert not out[0].any() and not out[2].any() and torch.equal(out[1], Z[8])
    z, s = read_pair_container(dataset["file"])
    z[5] = z[5][:8]                                              # a z record cut short
    s[7] = s[7][:4]                                              # a side record that cannot be opened
    f = d / "damaged.bin"
    write_pair_container(f, z, s)
    bad = comp.open_dataset(f)
    for rows in ([4, 5, 6], [7], [6, 7, 8]):
        with pytest.raises(ValueError, match="malformed"):
            bad.take(rows)
    out = bad.take([4, 5, 6, 7, 8], check=False)
    assert not out[1].any() and not out[3].any() and torch.equal(out[[0, 2, 4]], Z[[4, 6, 8]])
    assert torch.equal(bad.take([4, 6, 8, 299]), Z[[4, 6, 8, 299]])
    blob = dataset["file"].read_bytes()
    z, s = read_pair_container(dataset["file"])
    odd = d / "odd.bin"                                          # an odd number of records is not a pair file
    odd.write_bytes((2 * N - 1).to_bytes(4, "big") + blob[4:len(blob) - 4 - len(s[-1])])
    with pytest.raises(ValueError, match="two per image"):
        comp.open_dataset(odd)


@pytest.mark.parametrize("n_other", [1, 255, 300])
def test_take_does_not_depend_on_batch_size_or_row_position(dataset, n_other):
    ds = dataset["ds"]
    g = torch.Generator().manual_seed(n_other)
    idx = torch.randint(0, N, (77,), generator=g)
    other = torch.randint(0, N, (n_other,), generator=g)
    alone = ds.take(idx)
    assert torch.equal(ds.take(torch.cat([other, idx]))[-len(idx):], alone)
