"""GPU: the Python coder on tables the resident kernels refuse (``HRateFactorizedPrior`` at 1024 dimensions, a
``ClipCompressor`` with W > 64) and ``FeatureCompressor`` end to end at 1024 dimensions, against the same objects on the
CPU (the library's host coder).  Everything is exact."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
from wide_coder_util import gaussian_features, widen_state_dict

pytestmark = pytest.mark.gpu

ENCODE, DECODE, GATHER = 0, 1, 2


def _fits(C, W):
    from lossyless_amd import _lib
    return [_lib.lib().lla_rans_table_fits(C, W, k) for k in (ENCODE, DECODE, GATHER)]


def _shipped():
    return torch.load(os.path.join(ROOT, "lossyless_amd", "assets", "beta5e-02_factorized_rate.pt"), map_location="cpu",
                      weights_only=True)


def test_factorized_prior_at_1024_dimensions():
    from lossyless_amd.rates import HRateFactorizedPrior
    torch.manual_seed(0)
    m = HRateFactorizedPrior(1024, kwargs_ent_bottleneck=dict(init_scale=16, filters=[3, 3, 3, 3]))
    m.entropy_bottleneck.update()
    W = int(m.entropy_bottleneck._quantized_cdf.shape[1])
    assert W >= 33 and _fits(1024, W) == [0, 0, 0]
    m.eval()
    z = gaussian_features(300, 1024, seed=1) * 6
    want = m.compress(z)                                   # the module on the CPU: the host coder
    z_hat = m.decompress(want)
    g = HRateFactorizedPrior(1024, kwargs_ent_bottleneck=dict(init_scale=16, filters=[3, 3, 3, 3]))
    g.load_state_dict(m.state_dict())
    g = g.cuda().eval()
    got = g.compress(z.cuda())
    assert got == want
    assert torch.equal(g.decompress(got).cpu(), z_hat)
    assert g.compress(z.half().cuda()) == m.compress(z.half())


def test_clip_compressor_with_a_table_wider_than_64(tmp_path):
    from lossyless_amd import ClipCompressor
    sd = widen_state_dict(_shipped(), push=20)
    W = int(sd["entropy_bottleneck._quantized_cdf"].shape[1])
    assert W > 64 and _fits(512, W) == [0, 0, 0]
    comp = ClipCompressor(sd, device="cuda", clip_weights="synthetic")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 3, 224, 224, generator=g).half().cuda()
    strings = comp.compress(x)
    assert torch.equal(comp.decompress(strings), comp(x))
    file = tmp_path / "z.bin"
    comp.compress_dataset(x, file, is_info=False)
    on_gpu = comp.decompress_dataset(file, is_info=False, is_cpu=False)
    assert np.array_equal(on_gpu, comp.decompress_dataset(file, is_info=False, is_cpu=True))
    assert np.array_equal(on_gpu, comp(x).cpu().numpy())
    assert torch.equal(comp.open_dataset(file).take([5, 0, 5]).cpu(), torch.from_numpy(on_gpu[[5, 0, 5]]))


N, C = 1536, 1024


@functools.lru_cache(maxsize=None)
def fitted():
    """1536 rows of seeded Gaussian features with per-channel scales, one epoch of BottleneckFit on them."""
    from lossyless_amd import BottleneckFit
    Z = gaussian_features(N, C, seed=7)
    fit = BottleneckFit(0.05, epochs=1, batch_size=256, seed=1).fit(Z.cuda())
    return Z, fit.state_dict()


def test_feature_compressor_end_to_end_at_1024_dimensions(tmp_path):
    import hubconf
    from lossyless_amd import LinearProbe
    Z, sd = fitted()
    W = int(sd["entropy_bottleneck._quantized_cdf"].shape[1])
    assert _fits(C, W)[GATHER] == 0                                   # the resident gather refuses 1024 x W whatever W is
    comp = hubconf.feature_compressor(sd, device="cuda")
    host = hubconf.feature_compressor(sd, device="cpu")
    assert comp.z_dim == host.z_dim == C
    y = (torch.arange(N) % 5).numpy()
    file, lf, file_h = tmp_path / "z.bin", tmp_path / "y.npy", tmp_path / "zh.bin"
    comp.compress_dataset(Z.cuda(), file, lf, labels=y, is_info=False)
    host.compress_dataset(Z, file_h, is_info=False)
    assert file.read_bytes() == file_h.read_bytes()
    z_hat = comp(Z)
    assert torch.equal(z_hat.cpu(), host(Z))
    dec, labels = comp.decompress_dataset(file, lf, is_info=False, is_cpu=False)
    assert np.array_equal(dec, comp.decompress_dataset(file, is_info=False, is_cpu=True))
    assert np.array_equal(dec, z_hat.cpu().numpy()) and np.array_equal(labels, y)

    ds = comp.open_dataset(file, lf)
    gen = torch.Generator().manual_seed(2)
    idx = torch.cat([torch.randperm(N, generator=gen), torch.tensor([3, 3, N - 1])])
    assert torch.equal(ds.take(idx), z_hat[idx.cuda()])
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(9))
    got = torch.cat([zb for zb, _ in ds.batches(200, shuffle=True, generator=torch.Generator().manual_seed(9),
                                                decode_group=600)])
    assert torch.equal(got, ds.take(perm))

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)               # (three Newton steps stop short of tol, by design)
        a = LinearProbe(max_iter=3).fit(ds)
        b = LinearProbe(max_iter=3).fit(z_hat, torch.from_numpy(y).cuda())
    bits = lambda t: torch.as_tensor(t).detach().cpu().contiguous().view(torch.int32)
    assert torch.equal(bits(a.coef_), bits(b.coef_)) and a.n_passes_ == b.n_passes_
