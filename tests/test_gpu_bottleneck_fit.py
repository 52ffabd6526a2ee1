"""MI355X: ``lla_eb_train_pass`` / ``lla_eb_aux_grad`` against torch autograd in float64, the noise stream, the refusals, 20
steps of the device engine against the float64 twin, and BottleneckFit end to end.

Bounds.  Nothing here is fixed by hand: the restatement of the loss in eb_reference.py is evaluated by torch on the CPU in
fp32 and in float64 on the SAME fp32-representable parameters, rows and noise; the worst fp32-against-float64 error of a
parameter group, times 4, bounds the kernel's error in that group (the kernel's fp32 sums run in another order than torch's,
which is what the factor covers -- the margin of the ridge probes' tests).  The two scalar sums have one number each, whose fp32
error can vanish by chance: their bound is 4 x max(that error, 2^-24 |sum|) -- half an ulp of the sum is what ONE rounding of
the result costs any fp32 evaluation.  Each test prints error / bound per group before it asserts."""
import ctypes
import math

import numpy as np
import pytest
import torch

import eb_reference as R
from lossyless_amd import BottleneckFit, _lib, bottleneck_noise
from lossyless_amd.bottleneck_fit import _DeviceEngine, _TwinEngine, beta_schedule
from lossyless_amd.probe import _Adam, _adamw

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 1234.5
SEED, STEP = 0x1234567855AA, 9


def _guarded(n, dtype=torch.float32, fill=SENTINEL):
    """A device buffer of n elements with 4 guard elements on either side -> (whole, view): the view is 16-byte aligned."""
    whole = torch.full((n + 8,), fill, dtype=dtype, device=DEV)
    return whole, whole[4:4 + n]


def _guards_intact(whole, n, fill=SENTINEL):
    return bool((whole[:4] == fill).all()) and bool((whole[4 + n:] == fill).all())


def _device_pass(z, main32, ldz=None, seed=SEED, step=STEP):
    """Run the pass on z (CPU tensor, fp16 or fp32) and main32 [60, C] fp32 -> (grads [2, 60, C], sums [2], guards ok)."""
    L = _lib.lib()
    B, C = z.shape
    ldz = C if ldz is None else ldz
    zd = torch.full((B, ldz), float("nan"), dtype=z.dtype, device=DEV)       # columns beyond C: NaN, never to be read
    zd[:, :C] = z.to(DEV)
    md = main32.to(DEV).contiguous()
    gw, g = _guarded(2 * 60 * C)
    nws = int(L.lla_eb_train_pass_workspace_bytes(B, C))
    assert nws > 0 and nws % 4 == 0
    ww, ws = _guarded(nws // 4)
    sums = torch.full((4,), SENTINEL, dtype=torch.float64, device=DEV)
    rc = L.lla_eb_train_pass(_lib.ptr(zd), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, ldz, B, C,
                             _lib.ptr(md[2:]), _lib.ptr(md[0]), _lib.ptr(md[1]), seed, step, _lib.ptr(g), _lib.ptr(sums[1:]),
                             _lib.ptr(ws), _lib.stream_ptr(torch.device(DEV)))
    _lib.check(rc, "lla_eb_train_pass")
    torch.cuda.synchronize()
    ok = (_guards_intact(gw, 2 * 60 * C) and _guards_intact(ww, nws // 4) and float(sums[0]) == SENTINEL
          and float(sums[3]) == SENTINEL and bool(torch.isnan(zd[:, C:]).all()) and torch.equal(md.cpu(), main32))
    return g.cpu().reshape(2, 60, C).clone(), sums[1:3].cpu().clone(), ok


_REF = {}


def _reference(name, B, C, half):
    """(z as the kernel reads it, main32, u, float64 grads, float64 sums, bounds) of a case, computed once."""
    key = (name, B, C, half)
    if key not in _REF:
        z, main, q, target = R.stress_case(name, B, C)
        z = z.half() if half else z.float()
        main32 = main.float()
        u = bottleneck_noise(SEED, STEP, B, C)
        ref, dist, rate = R.reference_pass(z.float(), main32.double(), u)
        r32, d32, t32 = R.reference_pass(z.float(), main32, u)
        bound = {k: 4 * v for k, v in R.group_errors(r32, ref).items()}
        sums = torch.stack([dist, rate])
        s32 = torch.stack([d32, t32]).double()
        sbound = 4 * torch.maximum((s32 - sums).abs(), sums.abs() * 2.0 ** -24)
        _REF[key] = (z, main32, u, ref, sums, bound, sbound)
    return _REF[key]


SHAPES = [(C, B, False) for C in (64, 68, 512) for B in (1, 63, 64, 65, 1000)] + [(64, 65, True), (68, 1000, True), (512, 63, True), (68, 1, True), (512, 64, True)]
CASES = [("plain", B, C, half) for C, B, half in SHAPES] + [(n, 33, 68, False) for n in ("bound", "signs", "matrix30", "factor5")]


@pytest.mark.parametrize("name,B,C,half", CASES)
def test_pass_against_float64_per_gradient_element(name, B, C, half):
    z, main32, u, ref, sums, bound, sbound = _reference(name, B, C, half)
    got, gsums, ok = _device_pass(z, main32)
    assert ok, "a guard word, a guard column or an input was written"
    err = R.group_errors(got, ref)
    print(f"{name} B={B} C={C} {'fp16' if half else 'fp32'}: " + "  ".join(f"{k} {err[k]:.2e}/{bound[k]:.2e}" for k in err)
          + f"  sums {[f'{float(e):.2e}/{float(b):.2e}' for e, b in zip((gsums - sums).abs(), sbound)]}")
    assert bool(torch.isfinite(got).all())
    for k in err:
        assert err[k] <= bound[k], f"{k}: error {err[k]:.3e} beyond 4 x the fp32 restatement's {bound[k] / 4:.3e}"
    assert bool(((gsums - sums).abs() <= sbound).all())
    again, asums, _ = _device_pass(z, main32)
    assert torch.equal(again, got) and torch.equal(asums, gsums), "a second call gave other bits"


@pytest.mark.parametrize("half", [False, True])
def test_pass_reads_rows_by_their_pitch(half):
    z, main32, u, ref, sums, bound, sbound = _reference("plain", 65, 68, half)
    dense, dsums, _ = _device_pass(z, main32)
    padded, psums, ok = _device_pass(z, main32, ldz=80)
    assert ok and torch.equal(dense, padded) and torch.equal(dsums, psums)


@pytest.mark.parametrize("name,C", [("plain", 64), ("plain", 68), ("plain", 512), ("plain", 1028), ("matrix30", 68), ("factor5", 68)])
def test_aux_against_float64(name, C):
    _, main, q, target = R.stress_case(name, 1, C)
    net32, q32 = main[2:].float().contiguous(), q.float().contiguous()
    ref, aux = R.reference_aux(net32.double(), q32.double(), target)
    r32, a32 = R.reference_aux(net32, q32, target)
    bound = 4 * float((r32.double() - ref).abs().max())
    abound = 4 * max(abs(float(a32) - float(aux)), 2.0 ** -24 * float(aux))
    gw, g = _guarded(3 * C)
    out = torch.full((3,), SENTINEL, dtype=torch.float64, device=DEV)
    nd, qd, td = net32.to(DEV), q32.to(DEV), target.float().to(DEV)
    for _ in range(2):
        rc = _lib.lib().lla_eb_aux_grad(_lib.ptr(nd), _lib.ptr(qd), _lib.ptr(td), C, _lib.ptr(g), _lib.ptr(out[1:]),
                                        _lib.stream_ptr(torch.device(DEV)))
        _lib.check(rc, "lla_eb_aux_grad")
        torch.cuda.synchronize()
        got, gaux = g.cpu().reshape(C, 3).clone(), float(out[1])
        err = float((got.double() - ref).abs().max())
        print(f"aux {name} C={C}: grad {err:.2e}/{bound:.2e}  loss {abs(gaux - float(aux)):.2e}/{abound:.2e}")
        assert err <= bound and abs(gaux - float(aux)) <= abound
        assert _guards_intact(gw, 3 * C) and float(out[0]) == SENTINEL and float(out[2]) == SENTINEL
        first = (got, gaux) if _ == 0 else first
    assert torch.equal(first[0], got) and first[1] == gaux


def test_kernel_noise_is_bottleneck_noise():
    """B = 1 makes e = c / 4, so one row of C = 4096 channels walks the first 1024 counters.  At scaling = 0 the distortion's
    gradient for scaling is -sign(u + 1e-6) u exactly (exp(0) = 1, one row, no sum): |u| to the bit.  The sign of u comes from
    the rate's gradient for biasing on a density that is symmetric about 0 (zero biases and factors, z = 0): it has the sign of
    v = u, read where |u| > 2^-10 (nearer to the mode the fp32 rounding of the two evaluations decides)."""
    C = 4096
    main, _, _ = R.initial_main(C)
    main[0:2] = 0.0
    main[2 + R.N_MAT:] = 0.0
    main[2:2 + R.N_MAT] = main[2:3].mean()          # one matrix value everywhere: L is odd
    for seed, step in ((0, 0), (SEED, STEP), (2 ** 63 + 5, 2 ** 32 - 1)):
        got, sums, ok = _device_pass(torch.zeros(1, C), main.float(), seed=seed, step=step)
        u = bottleneck_noise(seed, step, 1, C)[0].numpy()
        want = -np.sign(u + np.float32(1e-6)) * u
        assert ok and np.array_equal(got[0, 0].numpy(), want.astype(np.float32))
        far = np.abs(u) > 2.0 ** -10
        assert np.array_equal(np.sign(got[1, 1].numpy())[far], np.sign(u)[far])
        assert abs(float(sums[0]) - float(np.abs(u.astype(np.float64) + np.float64(np.float32(1e-6))).sum())) < 1e-3
    # rows beyond the first: e = (i C + c) / 4 -- the distortion sum of a tall batch, to the bound of the pass test
    z, main32, u, ref, rsums, bound, sbound = _reference("plain", 1000, 68, False)
    _, gsums, _ = _device_pass(z, main32)
    assert abs(float(gsums[0] - rsums[0])) <= float(sbound[0])


def test_refusals_launch_nothing():
    L = _lib.lib()
    C, B = 64, 8
    main = R.initial_main(C)[0].float().to(DEV).contiguous()
    z = torch.zeros(B, C, device=DEV)
    gw, g = _guarded(2 * 60 * C)
    ws = torch.zeros(int(L.lla_eb_train_pass_workspace_bytes(B, C)), dtype=torch.uint8, device=DEV)
    sums = torch.full((2,), SENTINEL, dtype=torch.float64, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)

    def call(zp=None, dt=_lib.LLA_Z_F32, ldz=C, b=B, c=C, params=None, s=None, bz=None, grads=None, wsp=None, out=None):
        return L.lla_eb_train_pass(zp or _lib.ptr(z), dt, ldz, b, c, params or _lib.ptr(main[2:]), s or _lib.ptr(main[0]),
                                   bz or _lib.ptr(main[1]), 1, 1, grads or _lib.ptr(g), out or _lib.ptr(sums), wsp or _lib.ptr(ws), st)

    assert L.lla_eb_train_pass_workspace_bytes(B, 66) == 0 and L.lla_eb_train_pass_workspace_bytes(-1, C) == 0
    for rc in (call(c=66), call(c=0), call(b=-1), call(ldz=C - 4), call(dt=7), call(dt=0), call(zp=off(z, 2)),
               call(params=off(main, 8 * C + 4)), call(s=off(main, 4)), call(bz=off(main, 4 * C + 8)), call(grads=off(gw, 4)),
               call(wsp=off(ws, 4)), call(out=off(sums, 4))):
        assert rc == _lib.LLA_EINVAL
    assert call(b=0) == _lib.LLA_OK
    q = torch.zeros(C, 3, device=DEV)
    t = torch.zeros(3, device=DEV)
    aux = lambda **k: L.lla_eb_aux_grad(k.get("p", _lib.ptr(main[2:])), k.get("q", _lib.ptr(q)), _lib.ptr(t), k.get("c", C),
                                        _lib.ptr(g), k.get("o", _lib.ptr(sums)), st)
    for rc in (aux(c=66), aux(c=0), aux(p=off(main, 8 * C + 4)), aux(q=off(q, 4)), aux(o=off(sums, 4))):
        assert rc == _lib.LLA_EINVAL
    torch.cuda.synchronize()
    assert bool((gw == SENTINEL).all()) and bool((sums == SENTINEL).all())


def _engine_args(C, seed=3):
    main, q, target = R.initial_main(C, seed)
    return main.float().double(), q.float().double(), target


def test_trajectory_of_20_steps_against_the_twin():
    C, B, steps, beta = 64, 256, 20, 0.1
    main, q, target = _engine_args(C)
    g = torch.Generator().manual_seed(11)
    batches = [(torch.randn(B, C, generator=g) * torch.linspace(0.05, 2, C) + torch.linspace(-1, 1, C)) for _ in range(steps)]
    betas = beta_schedule(beta, steps, "linear")
    adams = lambda: (_Adam(1e-3, 3e-8, (0.9, 0.999), 1e-8), _Adam(3e-4, 1e-6, (0.9, 0.999), 1e-8))
    twin = _TwinEngine(main, q, target, *adams(), seed=SEED)
    dev = _DeviceEngine(main, q, target, *adams(), seed=SEED, device=DEV, max_batch=B, steps_per_epoch=steps)
    # the fp32 restatement: autograd in fp32 on the CPU, the same AdamW formulas on fp32 tensors
    a32, c32 = adams()
    m32, q32 = main.float(), q.float()
    mom, momq = [(torch.zeros_like(m32), torch.zeros_like(m32))], [(torch.zeros_like(q32), torch.zeros_like(q32))]
    for t, zb in enumerate(batches):
        twin.step(zb, t, betas[t])
        dev.step(zb.to(DEV), t, betas[t])
        gr, _, _ = R.reference_pass(zb, m32, bottleneck_noise(SEED, t, B, C))
        _adamw([m32], [(gr[0] + betas[t] * gr[1]) / B], mom, a32, t + 1)
        gq, _ = R.reference_aux(m32[2:], q32, target)
        _adamw([q32], [gq], momq, c32, t + 1)
    tm, tq = twin.state()
    dm, dq = dev.state()
    drift, err = R.group_errors(m32, tm), R.group_errors(dm, tm)
    qdrift, qerr = float((q32.double() - tq).abs().max()), float((dq.double() - tq).abs().max())
    print("trajectory: " + "  ".join(f"{k} {err[k]:.2e}/{4 * drift[k]:.2e}" for k in err) + f"  quantiles {qerr:.2e}/{4 * qdrift:.2e}")
    for k in err:
        assert err[k] <= 4 * drift[k], k
    assert qerr <= 4 * qdrift
    tl, dl = twin.epoch_log(), dev.epoch_log()
    assert tl.shape == dl.shape == (steps, 3) and np.allclose(tl, dl, rtol=1e-4)


def _features(N, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, C, generator=g) * torch.linspace(0.05, 2, C) + torch.linspace(-1, 1, C)


def _bits_per_row(m, z):
    strings = m.compress(z)[0]
    return 8.0 * sum(len(s) for s in strings) / len(strings)


_FITS = {}


def _fit(beta):
    if beta not in _FITS:
        Z = _features(8192 + 2048, 64).to(DEV)
        _FITS[beta] = (BottleneckFit(beta, epochs=5, batch_size=256, scheduler=None, seed=0).fit(Z[:8192]), Z[8192:])
    return _FITS[beta]


def test_end_to_end_fit_codes_fewer_bits_than_the_untrained_module():
    fit, held = _fit(1e-1)
    assert fit.engine_ == "device" and fit.rate_estimator_.scaling.is_cuda
    fresh = BottleneckFit(1e-1, seed=0).initial_estimator(64).eval()
    fresh.update(force=True)
    fresh = fresh.to(DEV)
    trained, untrained = _bits_per_row(fit.rate_estimator_, held), _bits_per_row(fresh, held)
    print(f"bits per row: trained {trained:.1f}, untrained {untrained:.1f}; rate curve {fit.rate_curve_}")
    assert trained < untrained
    assert fit.loss_curve_[-1] < fit.loss_curve_[0] and fit.aux_curve_[-1] < fit.aux_curve_[0]
    m = fit.rate_estimator_
    z_hat = m(held, None)[0]
    assert torch.equal(m.decompress(m.compress(held)), z_hat)
    again = BottleneckFit(1e-1, epochs=5, batch_size=256, scheduler=None, seed=0).fit(_features(8192 + 2048, 64).to(DEV)[:8192])
    a, b = fit.state_dict(), again.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a), "the same seed gave another state dict"


def test_higher_beta_gives_fewer_bits():
    (hi, held), (lo, _) = _fit(1e-1), _fit(1e-2)
    b_hi, b_lo = _bits_per_row(hi.rate_estimator_, held), _bits_per_row(lo.rate_estimator_, held)
    print(f"bits per row: beta 1e-1 {b_hi:.1f}, beta 1e-2 {b_lo:.1f}")
    assert b_hi < b_lo


def test_state_dict_loads_into_clip_compressor_and_round_trips_a_dataset(tmp_path):
    import hubconf
    Z = _features(2048, 512, seed=2).to(DEV)
    fit = BottleneckFit(5e-2, epochs=2, batch_size=256, scheduler=None, seed=0).fit(Z)
    comp, _ = hubconf.clip_compressor(fit.state_dict(), device=DEV, clip_weights="synthetic")
    g = torch.Generator().manual_seed(0)
    images = torch.randn(64, 3, 224, 224, generator=g)
    file = tmp_path / "z.bin"
    comp.compress_dataset(images, str(file), is_info=False)
    z = comp.decompress_dataset(str(file), is_info=False, is_cpu=False)
    assert tuple(z.shape) == (64, 512) and np.array_equal(z, comp.decompress_dataset(str(file), is_info=False))
    with torch.no_grad():
        want = comp(images.to(DEV))
    assert np.array_equal(z, want.float().cpu().numpy())


def test_fit_from_compressed_latents_equals_fit_from_its_rows(tmp_path):
    import hubconf
    from oracle import container
    import os
    from conftest import ROOT
    from lossyless_amd.rates import HRateFactorizedPrior
    comp, _ = hubconf.clip_compressor_b005(device=DEV, clip_weights="synthetic")
    sd = torch.load(os.path.join(ROOT, "lossyless_amd", "assets", "beta5e-02_factorized_rate.pt"), map_location="cpu",
                    weights_only=True)
    m = HRateFactorizedPrior(512)
    m.load_state_dict(sd)
    strings = m.to(DEV).eval().compress(_features(600, 512, seed=4).to(DEV))[0]       # a container of the shipped rate point
    file = tmp_path / "z.bin"
    container.write_container(str(file), strings)
    ds = comp.open_dataset(file)
    kw = dict(epochs=2, batch_size=128, scheduler=None, seed=5)          # four full batches and one of 88 per epoch
    a = BottleneckFit(5e-2, **kw).fit(ds).state_dict()
    b = BottleneckFit(5e-2, **kw).fit(ds.all()).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
