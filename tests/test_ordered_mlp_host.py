"""No GPU: the ordered hyperprior mode on the host -- ``lla_gemm_f32_ordered_host`` against an exact restatement of the
chain, ``HRateHyperprior(mlp_precision="ordered")``'s host round trip, the refusals of the other modes, the new entry
points' argument checks, a CPU ``HyperpriorClipCompressor`` reading a container, and the committed container that an
MI355X wrote (tests/golden/ordered_hyperprior.*: host = device across machines and versions)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from ordered_util import (F32, MIN_NORMAL, P, bits, chain_reference, golden_state_dict, host_gemm, mixed_rows,
                          mul_then_add_reference, ordered_inputs, ordered_model)

SHAPES = [(1, 4, 8), (3, 12, 40), (5, 68, 104)]


@pytest.fixture(scope="module")
def cases():
    """Inputs and the exact chain (without bias / ReLU: the variants are one more exact step each), once per shape."""
    out = {}
    for i, (M, N, K) in enumerate(SHAPES):
        A, W, bias = ordered_inputs(M, N, K, seed=10 + i)
        ref, tiniest = chain_reference(A, W)
        out[(M, N, K)] = (A, W, bias, ref, tiniest)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_host_gemm_is_the_exact_chain(cases, shape):
    A, W, bias, ref, tiniest = cases[shape]
    # the inputs can tell the chain from a multiply-then-add, and walk through denormals
    assert not torch.equal(bits(ref), bits(mul_then_add_reference(A, W)))
    assert ref[0, 0] == F32(2.0 ** -11 + 2.0 ** -24) and mul_then_add_reference(A, W)[0, 0] == F32(2.0 ** -11)
    assert 0 < tiniest < MIN_NORMAL
    for with_bias in (False, True):
        for relu in (False, True):
            want, _ = chain_reference(A, W, bias if with_bias else None, relu)
            got = host_gemm(A, W, bias if with_bias else None, relu)
            assert torch.equal(bits(got), bits(want)), (shape, with_bias, relu)
    if shape[0] > 1:      # the chain of underflowing negative products ends at -0, which ReLU turns into +0
        M, N = shape[0], shape[1]
        assert np.signbit(ref[M - 1, N - 2]) and ref[M - 1, N - 2] == 0
        assert not np.signbit(host_gemm(A, W, None, True)[M - 1, N - 2])


def test_host_gemm_first_two_steps_are_fused():
    """The crafted pair alone (K = 8, the other k zero): 2^-11 + 2^-24 fused, 2^-11 if the product were rounded."""
    A, W = np.zeros((1, 8), F32), np.zeros((4, 8), F32)
    A[0, :2] = [1.0, 1.0 + 2.0 ** -12]
    W[0, :2] = [-1.0, 1.0 + 2.0 ** -12]
    assert host_gemm(A, W, None, False)[0, 0] == F32(2.0 ** -11 + 2.0 ** -24)
    assert mul_then_add_reference(A, W)[0, 0] == F32(2.0 ** -11)


def test_host_gemm_chain_is_per_element(cases):
    A, W, bias, _, _ = cases[(5, 68, 104)]
    whole = host_gemm(A, W, bias, True)
    for m in range(5):
        assert torch.equal(bits(host_gemm(A[m:m + 1], W, bias, True)), bits(whole[m:m + 1]))
    # ... and does not depend on the pitches: operands sliced out of wider buffers, C into a wider one
    Aw, Ww = np.full((5, 120), 7.0, F32), np.full((68, 112), 7.0, F32)
    Aw[:, 8:112], Ww[:, 4:108] = A, W
    got = host_gemm(Aw[:, 8:112], Ww[:, 4:108], bias, True, ldc=72, sentinel=-123.25)
    assert torch.equal(bits(got[:, :68]), bits(whole)) and (got[:, 68:] == F32(-123.25)).all()


def test_new_entry_points_exported_and_argument_checks():
    from lossyless_amd import _lib
    L = _lib.lib()
    new = ("lla_gemm_f32_ordered", "lla_gemm_f32_ordered_host", "lla_gaussian_quantise_encode_host",
           "lla_gaussian_decode_dequantise_host")
    assert set(new) <= set(_lib.EXPORTS)
    A, W, b, C = np.zeros((2, 16), F32), np.zeros((4, 16), F32), np.zeros(4, F32), np.zeros((2, 4), F32)
    ok = dict(A=P(A), lda=16, W=P(W), ldw=16, bias=P(b), C=P(C), ldc=4, M=2, N=4, K=16, relu=0)
    call = lambda **kw: L.lla_gemm_f32_ordered_host(*{**ok, **kw}.values())
    assert call() == _lib.LLA_OK and call(bias=None) == _lib.LLA_OK and call(M=0, A=None) == _lib.LLA_OK
    for bad in (dict(A=None), dict(W=None), dict(C=None), dict(K=12), dict(K=0), dict(N=3), dict(lda=8), dict(ldw=8),
                dict(ldc=0), dict(M=-1)):
        assert call(**bad) == _lib.LLA_EINVAL, bad
    # the device entry point refuses the same before any device call (no GPU is touched: the pointers are never used)
    dev = lambda **kw: L.lla_gemm_f32_ordered(*{**ok, **kw}.values(), None)
    for bad in (dict(K=12), dict(lda=8), dict(ldw=8), dict(N=3), dict(A=None), dict(W=None), dict(C=None)):
        assert dev(**bad) == _lib.LLA_EINVAL, bad

    # the conditional host coders
    m = ordered_model()
    h = m._host_params()
    gc = h["gc"]
    B, Cz = 2, 512
    z = np.zeros((B, Cz), F32)
    scales = np.ones((B, Cz), F32)
    off = np.zeros(B + 1, np.uint64)
    enc = dict(z=P(z), zt=_lib.LLA_Z_F32, B=B, C=Cz, bias=P(h["bias"]), es=P(h["exp_scale"]), scales=P(scales), ld=Cz,
               means=None, ldm=0, stab=P(h["scale_table"]), bound=h["scale_bound"], cdf=P(gc["cdf"]), T=gc["T"], W=gc["W"],
               cdf_len=P(gc["cdf_len"]), offset=P(gc["offset"]), prefix=1, out=None, cap=0, out_off=P(off), sym=None,
               idx=None)
    ecall = lambda **kw: L.lla_gaussian_quantise_encode_host(*{**enc, **kw}.values())
    assert ecall() == _lib.LLA_ECAP and off[-1] > 0          # sizing call
    for bad in (dict(z=None), dict(zt=7), dict(bias=None), dict(es=None), dict(scales=None), dict(ld=Cz - 1),
                dict(means=P(scales), ldm=Cz - 1), dict(stab=None), dict(cdf=None), dict(cdf_len=None), dict(offset=None),
                dict(out_off=None), dict(W=2), dict(C=0)):
        assert ecall(**bad) == _lib.LLA_EINVAL, bad
    out = np.zeros(int(off[-1]), np.uint8)
    assert ecall(out=P(out), cap=out.size) == _lib.LLA_OK
    zh, st = np.zeros((B, Cz), F32), np.zeros(B, np.int32)
    dec = dict(payload=P(out), off=P(off), prefix=1, first=0, step=1, B=B, C=Cz, bias=P(h["bias"]), es=P(h["exp_scale"]),
               scales=P(scales), ld=Cz, means=None, ldm=0, stab=P(h["scale_table"]), bound=h["scale_bound"],
               cdf=P(gc["cdf"]), T=gc["T"], W=gc["W"], cdf_len=P(gc["cdf_len"]), offset=P(gc["offset"]), z_hat=P(zh),
               status=P(st))
    dcall = lambda **kw: L.lla_gaussian_decode_dequantise_host(*{**dec, **kw}.values())
    assert dcall() == _lib.LLA_OK and not st.any()
    for bad in (dict(payload=None), dict(off=None), dict(first=-1), dict(step=0), dict(bias=None), dict(scales=None),
                dict(ld=Cz - 1), dict(means=P(scales), ldm=1), dict(stab=None), dict(cdf=None), dict(z_hat=None),
                dict(status=None), dict(C=0)):
        assert dcall(**bad) == _lib.LLA_EINVAL, bad


# ------------------------------------------------------------------------------------------------ the model on the host
@pytest.fixture(scope="module")
def z64():
    return mixed_rows(64, 512, seed=1)


@pytest.mark.parametrize("coded_means", ["scales", "predicted"])
@pytest.mark.parametrize("half", [False, True])
def test_host_round_trip_of_the_model(z64, coded_means, half):
    m = ordered_model(coded_means)
    z = z64.half() if half else z64
    payload, offsets, sym = m.encode_host(z, want_symbols=True)
    # the test exercises row selection: many table rows, side symbols that differ
    assert sym["z_indexes"].unique().numel() >= 32 and sym["side_symbols"].unique().numel() > 1
    z_hat = m.decode_host(payload, offsets, 64)
    assert z_hat.dtype == torch.float32 and z_hat.shape == (64, 512)
    assert torch.equal(bits(z_hat), bits(m.represent_host(z)))
    z_strings, side_strings = m.compress(z)
    off, blob = offsets.numpy(), payload.numpy().tobytes()
    for i in range(64):
        assert blob[off[2 * i]:off[2 * i + 1]] == len(z_strings[i]).to_bytes(4, "big") + z_strings[i]
        assert blob[off[2 * i + 1]:off[2 * i + 2]] == len(side_strings[i]).to_bytes(4, "big") + side_strings[i]
    assert torch.equal(bits(m.decompress([z_strings, side_strings])), bits(z_hat))
    # one image per call gives the records of the batch (the chain does not depend on M)
    p1, o1 = m.encode_host(z[5:6])
    assert p1.numpy().tobytes()[:int(o1[-1])] == blob[off[10]:off[12]]
    # a record cut short is refused
    cut = offsets.clone()
    cut[1:] -= 4
    with pytest.raises(ValueError, match="malformed"):
        m.decode_host(payload, cut, 64)


def test_modes_differ_and_other_precisions_refuse(z64):
    for precision in ("fp32", "fp16"):
        m = ordered_model(precision=precision)
        for call in (lambda: m.encode_host(z64), lambda: m.represent_host(z64),
                     lambda: m.decode_host(torch.zeros(8, dtype=torch.uint8), torch.zeros(3, dtype=torch.int64), 1)):
            with pytest.raises(NotImplementedError, match='mlp_precision="ordered"'):
                call()
    from lossyless_amd.rates import MLP
    with pytest.raises(ValueError, match="ordered"):
        MLP(4, 4, precision="exact")
    # the mode is no part of the state dict
    assert set(ordered_model().state_dict()) == set(ordered_model(precision="fp32").state_dict())
    # on the CPU the ordered MLP is the chain on the padded operands, not torch's Linear
    m = ordered_model()
    x = z64[:3, :m.side_z_dim].contiguous()
    got = m.z_encoder(x)
    a = np.zeros((3, 104), F32)
    a[:, :m.side_z_dim] = x.numpy()
    lin = [l for l in m.z_encoder.module if isinstance(l, torch.nn.Linear)]
    for i, l in enumerate(lin):
        n, k = l.weight.shape
        w = np.zeros((-(-n // 8) * 8, a.shape[1]), F32)
        w[:n, :k] = l.weight.detach().numpy()
        b = np.zeros(w.shape[0], F32)
        b[:n] = l.bias.detach().numpy()
        a = host_gemm(a, w, b, i < len(lin) - 1)
    assert torch.equal(bits(got), bits(a[:, :1024]))


# ------------------------------------------------------------------------------------------- the compressor on the host
@pytest.fixture(scope="module")
def cpu_compressor():
    from lossyless_amd import HyperpriorClipCompressor
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    return HyperpriorClipCompressor(synthetic_hyperprior_state_dict(0), device="cpu", clip_weights="synthetic",
                                    mlp_precision="ordered")


def _container_of(m, z, path):
    from lossyless_amd.hyperprior_compressor import write_pair_container
    z_strings, side_strings = m.compress(z)
    write_pair_container(path, z_strings, side_strings)
    return z_strings, side_strings


def test_cpu_compressor_decodes_a_container(cpu_compressor, z64, tmp_path):
    c = cpu_compressor
    path = tmp_path / "z.bin"
    strings = _container_of(c.hyperprior, z64, path)
    want = c.hyperprior.represent_host(z64).numpy()
    got = c.decompress_dataset(path, is_cpu=True, is_info=False)
    assert got.dtype == np.float32 and torch.equal(bits(got), bits(want))
    assert torch.equal(bits(c.decompress_dataset(path, is_cpu=True, is_info=False, batch_size=7)), bits(want))
    assert torch.equal(bits(c.decompress(list(strings))), bits(want))
    # what needs the tower, the GPU decoder or HyperpriorLatents still raises on a CPU compressor
    with pytest.raises(RuntimeError, match="MI355X"):
        c.decompress_dataset(path, is_cpu=False, is_info=False)
    with pytest.raises(RuntimeError, match="MI355X"):
        c.compress(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError, match="MI355X"):
        c(torch.zeros(1, 3, 224, 224))
    with pytest.raises(NotImplementedError):
        c.open_dataset(path)

    blob = path.read_bytes()
    bad = tmp_path / "bad.bin"
    bad.write_bytes(blob[:-3])                                           # truncated
    with pytest.raises(ValueError):
        c.decompress_dataset(bad, is_cpu=True, is_info=False)
    bad.write_bytes((127).to_bytes(4, "big") + blob[4:-(4 + len(strings[1][-1]))])     # odd record count
    with pytest.raises(ValueError, match="two per image"):
        c.decompress_dataset(bad, is_cpu=True, is_info=False)
    first = 4 + 4 + len(strings[0][0])                                   # image 0's side record: 8 bytes long, say
    bad.write_bytes(blob[:first] + (8).to_bytes(4, "big") + blob[first + 4:])
    with pytest.raises(ValueError):
        c.decompress_dataset(bad, is_cpu=True, is_info=False)
    hurt = bytearray(blob)
    hurt[8:16] = b"\xff" * 8                                             # image 0's z record: its state words
    hurt[16:len(strings[0][0]) + 8] = b"\xff" * (len(strings[0][0]) - 8)
    bad.write_bytes(bytes(hurt))
    try:      # (a damaged stream either overruns -- ValueError -- or decodes to other values: never the written ones)
        other = c.decompress_dataset(bad, is_cpu=True, is_info=False)
        assert not np.array_equal(other[0], want[0])
    except ValueError:
        pass


def test_default_mode_keeps_refusing_on_the_cpu(z64, tmp_path):
    from lossyless_amd import HyperpriorClipCompressor
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    c = HyperpriorClipCompressor(synthetic_hyperprior_state_dict(0), device="cpu", clip_weights="synthetic")
    assert c.hyperprior.mlp_precision == "fp32"
    with pytest.raises(NotImplementedError, match="lla_gemm_f32"):
        c.decompress_dataset(tmp_path / "none.bin", is_cpu=True)
    with pytest.raises(NotImplementedError, match="lla_gemm_f32"):
        c._decode_records_host(np.zeros(8, np.uint8), np.zeros(3, np.uint64), 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        c.decompress([[b"12345678"], [b"12345678"]])


# --------------------------------------------------------------------------------------- the container an MI355X wrote
def test_golden_device_container_decodes_on_the_host():
    """tests/golden/ordered_hyperprior.bin was written by ``encode_device`` on an MI355X (tools/make_ordered_golden.py)
    and ordered_hyperprior_z_hat.npy is what ``decode_device`` gave there: the host decodes the same bits."""
    from lossyless_amd import HyperpriorClipCompressor
    c = HyperpriorClipCompressor(golden_state_dict(), device="cpu", clip_weights="synthetic", mlp_precision="ordered")
    want = np.load(os.path.join(GOLDEN, "ordered_hyperprior_z_hat.npy"))
    got = c.decompress_dataset(os.path.join(GOLDEN, "ordered_hyperprior.bin"), is_cpu=True, is_info=False)
    assert want.dtype == np.float32 and want.shape == (32, 512)
    assert torch.equal(bits(got), bits(want))
