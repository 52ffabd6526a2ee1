"""GPU: the ordered hyperprior mode.  ``lla_gemm_f32_ordered`` against its host twin (which tests/test_ordered_mlp_host.py
ties to an exact restatement of the chain), bit for bit over every tile edge; ``HRateHyperprior(mlp_precision="ordered")``
on the device against the host path; a dataset written on the device and read on the host; the committed container; and the
default mode, untouched."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from ordered_util import F32, bits, golden_state_dict, host_gemm, mixed_rows, ordered_inputs, ordered_model

pytestmark = pytest.mark.gpu

SENTINEL = -123.25
# the kernel's tile is 64 x 64 (4 x 4 per thread), its K stage 32: one row, one short of a tile, one over, several tiles and
# a tail; N below a thread's quad row, over one tile, many tiles; K one group, three stages and a quarter, sixteen stages
MS, NS, KS = (1, 63, 65, 257), (4, 68, 1024), (8, 104, 512)


def device_gemm(A, W, bias, relu, pad=(8, 4, 12)):
    """``lla_gemm_f32_ordered`` on operands sliced out of wider device buffers -> the whole C buffer [M, N + pad] (numpy),
    pre-filled with SENTINEL."""
    from lossyless_amd import _lib
    M, K = A.shape
    N = W.shape[0]
    pa, pw, pc = pad
    Ad = torch.full((M, K + 2 * pa), 7.0, device="cuda")
    Wd = torch.full((N, K + 2 * pw), 7.0, device="cuda")
    Ad[:, pa:pa + K] = torch.from_numpy(A).cuda()
    Wd[:, pw:pw + K] = torch.from_numpy(W).cuda()
    Cd = torch.full((M, N + pc), SENTINEL, device="cuda")
    bd = None if bias is None else torch.from_numpy(bias).cuda()
    rc = _lib.lib().lla_gemm_f32_ordered(_lib.ptr(Ad[:, pa:]), Ad.stride(0), _lib.ptr(Wd[:, pw:]), Wd.stride(0),
                                         _lib.ptr(bd), _lib.ptr(Cd), Cd.stride(0), M, N, K, int(relu),
                                         _lib.stream_ptr())
    _lib.check(rc, "lla_gemm_f32_ordered")
    return Cd.cpu().numpy()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_device_gemm_equals_the_host_chain(M, N, K):
    A, W, bias = ordered_inputs(M, N, K, seed=100 + M + N + K)
    for with_bias in (False, True):
        for relu in (False, True):
            b = bias if with_bias else None
            want = host_gemm(A, W, b, relu)
            got = device_gemm(A, W, b, relu)
            assert torch.equal(bits(got[:, :N]), bits(want)), (with_bias, relu)
            assert (got[:, N:] == F32(SENTINEL)).all()            # columns beyond N are not written
    if M > 1:      # the chain of underflowing products: -0 without ReLU, +0 with it, on both sides
        assert np.signbit(host_gemm(A, W, None, False)[M - 1, N - 2])
        assert not np.signbit(device_gemm(A, W, None, True)[M - 1, N - 2])


def test_device_gemm_does_not_depend_on_the_call():
    A, W, bias = ordered_inputs(257, 68, 104, seed=5)
    whole = device_gemm(A, W, bias, True)[:, :68]
    lo = 0
    for rows in (1, 63, 193):
        part = device_gemm(A[lo:lo + rows], W, bias, True)[:, :68]
        assert torch.equal(bits(part), bits(whole[lo:lo + rows])), rows
        lo += rows
    assert lo == 257


def test_device_gemm_refuses_misaligned_operands():
    from lossyless_amd import _lib
    a, w, c = torch.zeros(2, 20, device="cuda"), torch.zeros(4, 16, device="cuda"), torch.zeros(2, 4, device="cuda")
    call = lambda A, lda: _lib.lib().lla_gemm_f32_ordered(_lib.ptr(A), lda, _lib.ptr(w), 16, None, _lib.ptr(c), 4, 2, 4,
                                                          16, 0, _lib.stream_ptr())
    assert call(a, 20) == _lib.LLA_OK
    assert call(a[:, 1:], 20) == _lib.LLA_EINVAL          # 4 bytes off a 16-byte boundary


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def z300():
    return mixed_rows(300, 512, seed=4)


@pytest.mark.parametrize("coded_means", ["scales", "predicted"])
@pytest.mark.parametrize("half", [False, True])
def test_model_device_equals_host(z300, coded_means, half):
    dev, host = ordered_model(coded_means, device="cuda"), ordered_model(coded_means)
    z = z300.half() if half else z300
    payload, offsets, sym = dev.encode_device(z.cuda(), want_symbols=True)
    assert sym["z_indexes"].unique().numel() >= 32 and sym["side_symbols"].unique().numel() > 1
    hp, ho, hsym = host.encode_host(z, want_symbols=True)
    for k in sym:
        assert torch.equal(sym[k].cpu(), hsym[k]), k
    used = int(ho[-1])
    assert torch.equal(offsets.cpu(), ho) and torch.equal(payload[:used].cpu(), hp[:used])
    z_hat = dev.decode_device(payload, offsets, 300)
    assert torch.equal(bits(host.decode_host(payload[:used + 4].cpu(), offsets.cpu(), 300)), bits(z_hat.cpu()))
    assert torch.equal(bits(dev.represent_device(z.cuda()).cpu()), bits(z_hat.cpu()))
    # the module on the GPU decodes on the host too (CPU copies of its tables and weights)
    assert torch.equal(bits(dev.decode_host(hp, ho, 300)), bits(z_hat.cpu()))
    # one image per call gives the records of the one call of 300
    blob = payload[:used].cpu().numpy().tobytes()
    off = ho.numpy()
    for i in (0, 63, 64, 299):
        p1, o1 = dev.encode_device(z[i:i + 1].cuda())
        assert p1[:int(o1[-1])].cpu().numpy().tobytes() == blob[off[2 * i]:off[2 * i + 2]], i


# ---------------------------------------------------------------------------------------------------------- the dataset
N_IMAGES = 600


@pytest.fixture(scope="module")
def comp():
    import hubconf
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    c, _ = hubconf.clip_hyperprior_compressor(synthetic_hyperprior_state_dict(0), device="cuda", clip_weights="synthetic",
                                              mlp_precision="ordered")
    return c


def test_dataset_written_on_the_device_is_read_on_the_host(comp, tmp_path):
    import hubconf
    from lossyless_amd.compressor import SyntheticImages
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    x = SyntheticImages(N_IMAGES, seed=12).device_batch(0, N_IMAGES, "cuda")
    f = tmp_path / "Z.bin"
    comp.compress_dataset(x, f, kwargs_dataloader=dict(batch_size=300), is_info=False)
    Z = comp.decompress_dataset(f, is_info=False)
    assert Z.shape == (N_IMAGES, 512) and Z.dtype == np.float32
    assert torch.equal(bits(comp.decompress_dataset(f, is_cpu=True, is_info=False)), bits(Z))
    cpu, _ = hubconf.clip_hyperprior_compressor(synthetic_hyperprior_state_dict(0), device="cpu", clip_weights="synthetic",
                                                mlp_precision="ordered")
    assert torch.equal(bits(cpu.decompress_dataset(f, is_cpu=True, is_info=False, batch_size=250)), bits(Z))
    idx = torch.randperm(N_IMAGES, generator=torch.Generator().manual_seed(0))
    latents = comp.open_dataset(f)
    assert torch.equal(bits(latents.take(idx).cpu()), bits(Z[idx.numpy()]))
    seen = torch.cat([z.cpu() for z in latents.batches(256)])
    assert torch.equal(bits(seen), bits(Z))
    with pytest.raises(NotImplementedError):
        comp.open_dataset(f, device="cpu")


def test_golden_device_container_decodes_on_the_device():
    """The committed container an MI355X wrote (tools/make_ordered_golden.py): this device, this build, the same bits."""
    import hubconf
    c, _ = hubconf.clip_hyperprior_compressor(golden_state_dict(), device="cuda", clip_weights="synthetic",
                                              mlp_precision="ordered")
    want = np.load(os.path.join(GOLDEN, "ordered_hyperprior_z_hat.npy"))
    got = c.decompress_dataset(os.path.join(GOLDEN, "ordered_hyperprior.bin"), is_info=False)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(c.decompress_dataset(os.path.join(GOLDEN, "ordered_hyperprior.bin"), is_cpu=True, is_info=False)),
                       bits(want))


def test_default_mode_is_untouched(z300, tmp_path):
    import hubconf
    from lossyless_amd.rates import HRateHyperprior, synthetic_hyperprior_state_dict
    sd = synthetic_hyperprior_state_dict(0)
    plain = HRateHyperprior(512).eval()
    plain.load_state_dict(sd)
    named = ordered_model(precision="fp32", device="cuda")
    assert plain.mlp_precision == "fp32"
    z = z300.cuda()
    (p0, o0), (p1, o1) = plain.cuda().encode_device(z), named.encode_device(z)
    assert torch.equal(o0, o1) and torch.equal(p0[:int(o0[-1])], p1[:int(o1[-1])])
    c, _ = hubconf.clip_hyperprior_compressor(sd, device="cuda", clip_weights="synthetic", mlp_precision="fp32")
    with pytest.raises(NotImplementedError, match="lla_gemm_f32"):
        c.decompress_dataset(tmp_path / "none.bin", is_cpu=True)
