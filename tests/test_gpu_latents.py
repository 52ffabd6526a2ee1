"""GPU: ``lla_rans_decode_gather`` (gather + rANS decode + dequantise in one kernel) against the oracle, against the
two-kernel path it fuses (``lla_rans_decode_batch`` + ``lla_dequantise``) and against its host twin; ``CompressedLatents``
on the device.  Integer decode and separately rounded fp32 operations => bit-exact."""
import numpy as np
import pytest
import torch

from conftest import BETAS
from latents_util import (TABLE_KEYS, code_rows, coded_case, edge_rows, golden_case, golden_index, host_gather,
                          write_dataset)

pytestmark = pytest.mark.gpu

SENTINEL = -123.25


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_gather(pay, off, prefix, index, tab, dtype=torch.float32, ld=None):
    """lla_rans_decode_gather -> (out [B, ld] prefilled with SENTINEL, status), both on the host."""
    from lossyless_amd import _lib
    t = {k: _dev(tab[k]) for k in TABLE_KEYS}
    C, W = tab["cdf"].shape
    payload, offsets = _dev(pay), _dev(off.astype(np.int64))
    idx = _dev(np.asarray(index, dtype=np.int64))
    B = idx.numel()
    ld = C if ld is None else ld
    out = torch.full((B, ld), SENTINEL, dtype=dtype, device="cuda")
    status = torch.full((max(B, 1),), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().lla_rans_decode_gather(
        _lib.ptr(payload), _lib.ptr(offsets), prefix, off.shape[0] - 1, _lib.ptr(idx), B, C, _lib.ptr(t["cdf"]), W,
        _lib.ptr(t["cdf_len"]), _lib.ptr(t["offset"]), _lib.ptr(t["bias"]), _lib.ptr(t["exp_scale"]), _lib.ptr(t["median"]),
        _lib.ptr(out), _lib.LLA_Z_F32 if dtype == torch.float32 else _lib.LLA_Z_F16, ld, _lib.ptr(status),
        _lib.stream_ptr())
    _lib.check(rc, "lla_rans_decode_gather")
    torch.cuda.synchronize()
    return out.cpu(), status[:B].cpu()


@pytest.fixture(scope="module")
def two_kernel_rows():
    """The 300 sampled records through the path the gather kernel fuses: lla_rans_decode_batch, then lla_dequantise."""
    from lossyless_amd import _lib
    tab, sym, pay, off, want = coded_case("5e-02", 300, 9)
    t = {k: _dev(tab[k]) for k in TABLE_KEYS}
    payload, offsets = _dev(pay), _dev(off.astype(np.int64))
    s = torch.empty((300, 512), dtype=torch.int32, device="cuda")
    st = torch.zeros(300, dtype=torch.int32, device="cuda")
    z = torch.empty((300, 512), dtype=torch.float32, device="cuda")
    L = _lib.lib()
    _lib.check(L.lla_rans_decode_batch(_lib.ptr(payload), _lib.ptr(offsets), 0, 300, 512, _lib.ptr(t["cdf"]), 32,
                                       _lib.ptr(t["cdf_len"]), _lib.ptr(t["offset"]), _lib.ptr(s), _lib.ptr(st),
                                       _lib.stream_ptr()), "lla_rans_decode_batch")
    _lib.check(L.lla_dequantise(_lib.ptr(s), 300, 512, _lib.ptr(t["bias"]), _lib.ptr(t["exp_scale"]), _lib.ptr(t["median"]),
                                _lib.ptr(z), _lib.stream_ptr()), "lla_dequantise")
    torch.cuda.synchronize()
    assert int(st.max()) == 0 and np.array_equal(s.cpu().numpy(), sym)
    return z.cpu()


@pytest.mark.parametrize("tag", BETAS)
def test_gather_of_golden_records_is_bit_exact(tag):
    tab, body, off, want = golden_case(tag)
    idx = golden_index()
    out, st = device_gather(body, off, 1, idx, tab)
    assert st.tolist() == [0] * len(idx)
    assert np.array_equal(out.numpy().view(np.uint32), want[idx].view(np.uint32))
    out16, st = device_gather(body, off, 1, idx, tab, dtype=torch.float16)
    assert st.tolist() == [0] * len(idx)
    with np.errstate(over="ignore"):
        want16 = want[idx].astype(np.float16)
    assert np.array_equal(out16.numpy().view(np.uint16), want16.view(np.uint16))


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1024])
def test_gather_equals_decode_then_dequantise(B, two_kernel_rows):
    tab, _, pay, off, _ = coded_case("5e-02", 300, 9)
    idx = np.random.default_rng(B).integers(0, 300, size=B)        # with repeats
    out, st = device_gather(pay, off, 0, idx, tab)
    assert not st.any() and torch.equal(out, two_kernel_rows[torch.from_numpy(idx)])


@pytest.mark.parametrize("name", ["one record 256 times", "reversed"])
def test_gather_of_repeated_and_reversed_indices(name, two_kernel_rows):
    tab, _, pay, off, _ = coded_case("5e-02", 300, 9)
    idx = np.full(256, 123) if name.startswith("one") else np.arange(299, -1, -1)
    out, st = device_gather(pay, off, 0, idx, tab)
    assert not st.any() and torch.equal(out, two_kernel_rows[torch.from_numpy(idx)])


def test_gather_flags_indices_out_of_range():
    tab, body, off, want = golden_case("5e-02")
    out, st = device_gather(body, off, 1, [5, -1, 64, 2 ** 40, 7], tab)
    assert st.tolist() == [0, 2, 2, 2, 0]
    assert not out[1:4].any()
    assert np.array_equal(out[0].numpy(), want[5]) and np.array_equal(out[4].numpy(), want[7])


def test_gather_flags_a_record_too_short_to_open():
    tab, body, off, want = golden_case("5e-02")
    cut = off.copy()
    cut[10] = cut[11] - 4 - 4                             # record 10: a length prefix and ONE word (record 9 only ends later)
    out, st = device_gather(body, cut, 1, [9, 10, 11, 10], tab)
    assert st.tolist() == [0, 1, 0, 1]
    assert not out[1].any() and not out[3].any()
    assert np.array_equal(out[0].numpy(), want[9]) and np.array_equal(out[2].numpy(), want[11])
    # a stream that opens but ends early is an overrun: same status, and its row is zeroed after the fact
    cut = off.copy()
    cut[10] = cut[11] - 4 - 8
    out, st = device_gather(body, cut, 1, [9, 10, 11], tab)
    assert st.tolist() == [0, 1, 0] and not out[1].any()
    assert np.array_equal(out[0].numpy(), want[9]) and np.array_equal(out[2].numpy(), want[11])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_gather_leaves_the_row_padding_alone(dtype):
    tab, body, off, want = golden_case("5e-02")
    idx = golden_index()[:9]
    out, st = device_gather(body, off, 1, idx, tab, dtype=dtype, ld=520)
    with np.errstate(over="ignore"):
        w = torch.from_numpy(want[idx].astype(np.float16 if dtype == torch.float16 else np.float32))
    assert not st.any() and torch.equal(out[:, :512], w) and (out[:, 512:] == SENTINEL).all()
    # a pitch that rules out 16-byte stores takes the scalar write-out: same values
    out, st = device_gather(body, off, 1, idx, tab, dtype=dtype, ld=513)
    assert not st.any() and torch.equal(out[:, :512], w) and (out[:, 512:] == SENTINEL).all()


def test_gather_with_forty_channels():
    """C = 40 is no multiple of the 16-channel staging group: the last group holds 8 channels."""
    tab, _, pay, off, want = coded_case("5e-02", 70, 11, C=40)
    idx = np.random.default_rng(3).permutation(70)
    out, st = device_gather(pay, off, 0, idx, tab)
    assert not st.any() and np.array_equal(out.numpy(), want[idx])
    out, st = device_gather(pay, off, 0, idx, tab, ld=43)           # ... and through the scalar write-out
    assert not st.any() and np.array_equal(out[:, :40].numpy(), want[idx]) and (out[:, 40:] == SENTINEL).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_gather_with_six_channels_through_the_ragged_scalar_write_out(dtype):
    """C = 6 is no multiple of 4 (the second 16-byte chunk of a staged line holds two channels) and a pitch of 7 rules out
    16-byte stores: bit-equal to lla_rans_decode_batch + lla_dequantise, the padding column untouched."""
    from lossyless_amd import _lib
    B, C = 70, 6
    tab, sym, pay, off, _ = coded_case("5e-02", B, 17, C=C)
    t = {k: _dev(tab[k]) for k in TABLE_KEYS}
    payload, offsets = _dev(pay), _dev(off.astype(np.int64))
    s = torch.empty((B, C), dtype=torch.int32, device="cuda")
    st2 = torch.zeros(B, dtype=torch.int32, device="cuda")
    z = torch.empty((B, C), dtype=torch.float32, device="cuda")
    L = _lib.lib()
    _lib.check(L.lla_rans_decode_batch(_lib.ptr(payload), _lib.ptr(offsets), 0, B, C, _lib.ptr(t["cdf"]), tab["cdf"].shape[1],
                                       _lib.ptr(t["cdf_len"]), _lib.ptr(t["offset"]), _lib.ptr(s), _lib.ptr(st2),
                                       _lib.stream_ptr()), "lla_rans_decode_batch")
    _lib.check(L.lla_dequantise(_lib.ptr(s), B, C, _lib.ptr(t["bias"]), _lib.ptr(t["exp_scale"]), _lib.ptr(t["median"]),
                                _lib.ptr(z), _lib.stream_ptr()), "lla_dequantise")
    torch.cuda.synchronize()
    assert int(st2.max()) == 0 and np.array_equal(s.cpu().numpy(), sym)
    idx = np.random.default_rng(5).permutation(B)
    out, st = device_gather(pay, off, 0, idx, tab, dtype=dtype, ld=7)
    want = z.cpu()[torch.from_numpy(idx)].to(dtype)
    assert not st.any() and torch.equal(out[:, :C], want) and (out[:, C:] == SENTINEL).all()


def test_gather_zeroes_an_overrun_row_and_keeps_its_neighbours():
    """Record 100 starts 8 bytes late: it still opens and then runs past its end (the host twin says so first).  Its row is
    zeroed after the workgroup has written it; every other row of both workgroups is untouched."""
    B, r = 257, 100
    tab, _, pay, off, _ = coded_case("5e-02", B, 21, C=40)
    cut = off.copy()
    cut[r] = off[r] + 8
    idx = np.arange(B)
    rc, _, hst = host_gather(pay, cut, 0, idx, tab)
    assert rc == 0 and hst[r] == 1 and int(hst.sum()) == 1
    whole, st0 = device_gather(pay, off, 0, idx, tab)
    out, st = device_gather(pay, cut, 0, idx, tab)
    keep = [i for i in range(B) if i != r]
    assert not st0.any() and np.array_equal(st.numpy(), hst)
    assert not out[r].any() and torch.equal(out[keep], whole[keep])
    assert torch.equal(out[[r - 1, r + 1, 256]], whole[[r - 1, r + 1, 256]])     # (named: same workgroup, and the second one)


def test_gather_of_edge_rows(tables):
    rows = edge_rows(tables)
    pay, off, want = code_rows(rows, tables)
    idx = [5, 0, 3, 1, 2, 4, 0]
    out, st = device_gather(pay, off, 0, idx, tables)
    assert not st.any() and np.array_equal(out.numpy().view(np.uint32), want[idx].view(np.uint32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_host_twin_equals_the_device(dtype):
    tab, _, pay, off, _ = coded_case("5e-02", 300, 9)
    cut = off.copy()
    cut[200] = cut[201] - 4                                # record 200 cannot be opened (one word, no prefix here)
    idx = np.concatenate([np.random.default_rng(1).integers(0, 300, size=400), [200, -5, 300, 299, 0]])
    out, st = device_gather(pay, cut, 0, idx, tab, dtype=dtype)
    rc, hout, hst = host_gather(pay, cut, 0, idx, tab, dtype=np.float32 if dtype == torch.float32 else np.float16)
    assert rc == 0 and np.array_equal(st.numpy(), hst) and set(hst.tolist()) == {0, 1, 2}
    assert np.array_equal(out.numpy().view(np.uint8), hout.view(np.uint8))


def test_compressed_latents_on_the_device(tmp_path):
    import hubconf
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    N = 1500                                               # no multiple of the 256 records of a workgroup
    file, lf, _ = write_dataset(tmp_path, "5e-02", N, seed=23)
    ds = comp.open_dataset(file, label_file=lf)
    host = comp.open_dataset(file, label_file=lf, device="cpu")
    assert len(ds) == N and ds.device.type == "cuda" and ds.nbytes == host.nbytes
    Z = comp.decompress_dataset(file, is_info=False, is_cpu=False)
    everything = ds.all()
    assert everything.is_cuda and np.array_equal(everything.cpu().numpy(), Z)
    assert torch.equal(ds.all(dtype=torch.float16), everything.half())

    def run(d, **kw):
        return list(d.batches(200, shuffle=True, generator=torch.Generator().manual_seed(3), **kw))

    small, large, cpu = run(ds, decode_group=512), run(ds, decode_group=65536), run(host)
    assert len(small) == len(large) == len(cpu) == 8
    for (za, ya), (zb, yb), (zc, yc) in zip(small, large, cpu):
        assert za.is_cuda and ya.is_cuda and torch.equal(za, zb) and torch.equal(ya, yb)
        assert torch.equal(ya.cpu(), yc) and torch.equal(za.cpu(), zc)      # same order, same values on the host
        assert torch.equal(za, everything[ya])
    assert len(run(ds, drop_last=True)) == 7

    buf = torch.zeros(3, 512, device="cuda")
    assert ds.take(torch.tensor([7, 7, 1499]), out=buf) is buf and torch.equal(buf, everything[[7, 7, 1499]])
    wide = torch.full((3, 520), SENTINEL, device="cuda")
    ds.take(np.array([0, 5, 2]), out=wide[:, :512])        # rows with a pitch: the padding stays
    assert torch.equal(wide[:, :512], everything[[0, 5, 2]]) and (wide[:, 512:] == SENTINEL).all()
    assert torch.equal(ds[11], everything[11]) and torch.equal(ds[5:900:7], everything[5:900:7])
    for bad in ([N], [-1]):
        with pytest.raises(IndexError):
            ds.take(bad)
