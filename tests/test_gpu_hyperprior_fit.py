"""MI355X: ``lla_eb_side_pass`` / ``lla_eb_aux_grad_any`` / ``lla_gaussian_train_pass`` / ``lla_affine_grad`` against the float64
twin of hyperprior_fit.py per gradient group, the noise streams, the refusals, 20 steps of the device engine against the twin,
and HyperpriorFit end to end.

Bounds, by the method of test_gpu_bottleneck_fit.py.  Nothing is fixed by hand: the SAME formulas (the twin's) are evaluated by
torch on the CPU in fp32 and in float64 on the same fp32-representable inputs and noise; the worst fp32-against-float64 error of
a group, times 4, bounds the kernel's error in that group (the kernel's libm and the order of its fp32 sums differ from
torch's: that is what the factor covers).  A scalar sum has one number, whose fp32 error can vanish by chance: its bound is
4 x max(that error, 2^-24 |sum|), one rounding of the result.  Each test prints error / bound per group before it asserts."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import hyperprior_reference as H
from lossyless_amd import BottleneckFit, HyperpriorFit, _lib, hyperprior_noise
from lossyless_amd.bottleneck_fit import beta_schedule, twin_aux
from lossyless_amd.hyperprior_fit import (SIDE_TAG, _DeviceEngine, _flatten, _TwinEngine, twin_affine_grad, twin_gaussian_pass,
                                          twin_side_pass)
from lossyless_amd.probe import _Adam, _adamw

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 1234.5
SEED, STEP = 0x1234567855AA, 9
SCALE = 0.05 / 33


def _guarded(n, dtype=torch.float32, fill=SENTINEL):
    """A device buffer of n elements with 4 guard elements on either side -> (whole, view): the view is 16-byte aligned."""
    whole = torch.full((n + 8,), fill, dtype=dtype, device=DEV)
    return whole, whole[4:4 + n]


def _intact(whole, n, fill=SENTINEL):
    return bool((whole[:4] == fill).all()) and bool((whole[4 + n:] == fill).all())


def _pitched(t, ld, fill=float("nan")):
    """CPU [B, W] -> device [B, ld] with the columns beyond W filled (NaN: never to be read)."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=DEV)
    out[:, :t.shape[1]] = t.to(DEV)
    return out


def _st():
    return _lib.stream_ptr(torch.device(DEV))


def _errors(got, ref):
    return {k: float((got[k].double() - ref[k].double()).abs().max()) for k in ref}


def _check(tag, got, ref, ref32, sums=()):
    """Print error / bound of every group, then assert.  ``sums``: the groups that are one number (floor 2^-24 |sum|)."""
    err, base = _errors(got, ref), _errors(ref32, ref)
    bound = {k: 4 * (max(base[k], 2.0 ** -24 * abs(float(ref[k]))) if k in sums else base[k]) for k in ref}
    print(f"{tag}: " + "  ".join(f"{k} {err[k]:.2e}/{bound[k]:.2e}" for k in ref))
    for k in ref:
        assert bool(torch.isfinite(got[k]).all()), k
        assert err[k] <= bound[k], f"{tag} {k}: error {err[k]:.3e} beyond 4 x the fp32 evaluation's {bound[k] / 4:.3e}"


# ------------------------------------------------------------------------------------------------------------- side pass
def _side_groups(s_hat, dx, grads, rate):
    return dict(s_hat=s_hat, dx=dx, matrix=grads[:33], bias=grads[33:46], factor=grads[46:], rate=torch.as_tensor(rate).reshape(1))


def _device_side(x, net32, scale=SCALE, seed=SEED, step=STEP, pad=True):
    L = _lib.lib()
    B, S = x.shape
    ldx, lds, ldd = (S + 3, -(-S // 8) * 8 + 8, -(-S // 8) * 8) if pad else (S, S, S)
    xd, nd = _pitched(x, ldx), net32.to(DEV).contiguous()
    sw, s_hat = _guarded(B * lds)
    dw, dx = _guarded(B * ldd)
    gw, g = _guarded(58 * S)
    nws = int(L.lla_eb_side_pass_workspace_bytes(B, S))
    assert nws > 0 and nws % 4 == 0
    ww, ws = _guarded(nws // 4)
    out = torch.full((3,), SENTINEL, dtype=torch.float64, device=DEV)
    rc = L.lla_eb_side_pass(_lib.ptr(xd), ldx, B, S, _lib.ptr(nd), seed, step, scale, _lib.ptr(s_hat), lds, _lib.ptr(dx), ldd,
                            _lib.ptr(g), _lib.ptr(out[1:]), _lib.ptr(ws), _st())
    _lib.check(rc, "lla_eb_side_pass")
    torch.cuda.synchronize()
    s_hat, dx = s_hat.view(B, lds), dx.view(B, ldd)
    ok = (_intact(sw, B * lds) and _intact(dw, B * ldd) and _intact(gw, 58 * S) and _intact(ww, nws // 4)
          and float(out[0]) == SENTINEL and float(out[2]) == SENTINEL and torch.equal(nd.cpu(), net32)
          and not bool(s_hat[:, S:].any()) and not bool(dx[:, S:].any()))           # pad columns: exactly zero
    return _side_groups(s_hat[:, :S].cpu().clone(), dx[:, :S].cpu().clone(), g.view(58, S).cpu().clone(), out[1:2].cpu().clone()), ok


@pytest.mark.parametrize("S", [10, 102, 130])
@pytest.mark.parametrize("B", [1, 33, 1000])
def test_side_pass_against_the_twin(B, S):
    x, net, q, target = H.side_case(B, S)
    net32 = net.float()
    u = hyperprior_noise(SEED, STEP, B, S, SIDE_TAG)
    scale = float(np.float32(SCALE))
    ref = _side_groups(*twin_side_pass(x, net32.double(), u, scale))
    ref32 = _side_groups(*twin_side_pass(x, net32, u, scale))
    got, ok = _device_side(x, net32)
    assert ok, "a guard word, an input or a pad column was written"
    _check(f"side B={B} S={S}", got, ref, ref32, sums=("rate",))
    again, _ = _device_side(x, net32)
    assert all(torch.equal(got[k], again[k]) for k in got), "a second call gave other bits"
    dense, _ = _device_side(x, net32, pad=False)
    assert all(torch.equal(got[k], dense[k]) for k in got), "the pitches changed the values"


@pytest.mark.parametrize("S", [10, 102, 130])
def test_aux_any_against_the_twin(S):
    _, net, q, target = H.side_case(1, S)
    net32, q32 = net.float().contiguous(), q.float().contiguous()
    rg, raux = twin_aux(net32.double(), q32.double(), target)
    g32, a32 = twin_aux(net32, q32, target)
    gw, g = _guarded(3 * S)
    out = torch.full((3,), SENTINEL, dtype=torch.float64, device=DEV)
    nd, qd, td = net32.to(DEV), q32.to(DEV), target.float().to(DEV)
    rc = _lib.lib().lla_eb_aux_grad_any(_lib.ptr(nd), _lib.ptr(qd), _lib.ptr(td), S, _lib.ptr(g), _lib.ptr(out[1:]), _st())
    _lib.check(rc, "lla_eb_aux_grad_any")
    torch.cuda.synchronize()
    assert _intact(gw, 3 * S) and float(out[0]) == SENTINEL and float(out[2]) == SENTINEL
    _check(f"aux S={S}", dict(grad=g.cpu().view(S, 3), aux=out[1:2].cpu()), dict(grad=rg, aux=raux.reshape(1)),
           dict(grad=g32, aux=a32.reshape(1)), sums=("aux",))


# --------------------------------------------------------------------------------------------------------- Gaussian pass
def _gauss_groups(C, y, dgp, dy, g_dist, dist, rate):
    one = lambda v: torch.as_tensor(v).reshape(1)
    return dict(y=y, scales=dgp[:, :C], means=dgp[:, C:2 * C], dy=dy, g_dist=g_dist, dist=one(dist), rate=one(rate))


def _device_gauss(z, s32, b32, gp32, scale=SCALE, seed=SEED, step=STEP, pad=True, prologue=False):
    L = _lib.lib()
    B, C = z.shape
    ldz, ldg, ldy = (C + 4, -(-2 * C // 8) * 8 + 8, -(-C // 8) * 8 + 8) if pad else (C, 2 * C, C)
    zd, gd = _pitched(z, ldz), _pitched(gp32, ldg)
    sd, bd = s32.to(DEV).contiguous(), b32.to(DEV).contiguous()
    bufs = {k: _guarded(n) for k, n in (("dgp", B * ldg), ("y", B * ldy), ("dy", B * ldy), ("g_dist", C))}
    nws = int(L.lla_gaussian_train_pass_workspace_bytes(B, C))
    assert nws > 0 and nws % 4 == 0
    ww, ws = _guarded(nws // 4)
    out = torch.full((4,), SENTINEL, dtype=torch.float64, device=DEV)
    P = _lib.ptr
    rc = L.lla_gaussian_train_pass(P(zd), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, ldz, B, C, P(sd), P(bd),
                                   None if prologue else P(gd), ldg, H.BOUND, seed, step, scale, P(bufs["dgp"][1]), P(bufs["y"][1]),
                                   ldy, P(bufs["dy"][1]), P(bufs["g_dist"][1]), P(out[1:]), P(ws), _st())
    _lib.check(rc, "lla_gaussian_train_pass")
    torch.cuda.synchronize()
    dgp, y, dy = bufs["dgp"][1].view(B, ldg), bufs["y"][1].view(B, ldy), bufs["dy"][1].view(B, ldy)
    ok = (all(_intact(w, v.numel()) for w, v in bufs.values()) and _intact(ww, nws // 4) and float(out[0]) == SENTINEL
          and float(out[3]) == SENTINEL and bool(torch.isnan(zd[:, C:]).all()) and bool(torch.isnan(gd[:, 2 * C:]).all())
          and torch.equal(sd.cpu(), s32) and not bool(y[:, C:].any()))
    if prologue:                     # y alone: nothing else is touched
        ok = ok and all(bool((bufs[k][1] == SENTINEL).all()) for k in ("dgp", "dy", "g_dist")) and bool((out == SENTINEL).all())
        return y[:, :C].cpu().clone(), ok
    ok = ok and not bool(dgp[:, 2 * C:].any()) and not bool(dy[:, C:].any())
    return _gauss_groups(C, y[:, :C].cpu().clone(), dgp[:, :2 * C].cpu().clone(), dy[:, :C].cpu().clone(),
                         bufs["g_dist"][1].cpu().clone(), out[1:2].cpu().clone(), out[2:3].cpu().clone()), ok


GAUSS = [("plain", B, C, half) for B, C in ((33, 68), (65, 512), (1000, 68)) for half in (False, True)] + \
        [(n, 33, 68, False) for n in H.GAUSS_CASES[1:]]


@pytest.mark.parametrize("name,B,C,half", GAUSS)
def test_gaussian_pass_against_the_twin(name, B, C, half):
    u = hyperprior_noise(SEED, STEP, B, C)
    z, scaling, biasing, gp = H.gaussian_case(name, B, C, u)
    z = z.half() if half else z.float()
    s32, b32, gp32 = scaling.float(), biasing.float(), gp.float()
    scale = float(np.float32(SCALE))
    ref = _gauss_groups(C, *twin_gaussian_pass(z.float(), s32.double(), b32.double(), gp32, u, H.BOUND, scale))
    ref32 = _gauss_groups(C, *twin_gaussian_pass(z.float(), s32, b32, gp32, u, H.BOUND, scale))
    got, ok = _device_gauss(z, s32, b32, gp32)
    assert ok, "a guard word, an input or a pad column was written"
    if name == "lowscale":
        assert bool((got["scales"] < 0).any()) and bool((got["scales"] == 0).any()) and not bool((got["scales"] > 0).any())
    if name == "tie":
        assert not bool(got["dy"][::2].any()) and not bool(got["means"][::2].any()) and bool(got["scales"][::2].any())
    if name == "likbound":
        assert float(got["rate"]) > 0.9 * B * C * -math.log(1e-9)
    _check(f"gauss {name} B={B} C={C} {'fp16' if half else 'fp32'}", got, ref, ref32, sums=("dist", "rate"))
    again, _ = _device_gauss(z, s32, b32, gp32)
    assert all(torch.equal(got[k], again[k]) for k in got), "a second call gave other bits"
    dense, _ = _device_gauss(z, s32, b32, gp32, pad=False)
    assert all(torch.equal(got[k], dense[k]) for k in got), "the pitches changed the values"
    y, ok = _device_gauss(z, s32, b32, gp32, prologue=True)
    assert ok and torch.equal(y, got["y"]), "the prologue's y differs from the pass's"


@pytest.mark.parametrize("B,C", [(33, 68), (65, 512), (1000, 68), (7, 10)])
def test_affine_grad_against_the_twin(B, C):
    g = torch.Generator().manual_seed(B + C)
    dy, y = torch.randn(B, C, generator=g) * 1e-3, torch.randn(B, C, generator=g) * 3
    s32, add = 1 + 0.3 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    inv = float(np.float32(1.0 / B))
    ref = dict(zip(("scaling", "biasing"), twin_affine_grad(dy.double(), y.double(), s32.double(), add.double(), inv)))
    ref32 = dict(zip(("scaling", "biasing"), twin_affine_grad(dy, y, s32, add, inv)))
    L, P = _lib.lib(), _lib.ptr
    ld, ldy = C + 5, C + 9
    dyd, yd, sd, ad = _pitched(dy, ld), _pitched(y, ldy), s32.to(DEV), add.to(DEV)
    (gsw, gs), (gbw, gb) = _guarded(C), _guarded(C)
    nws = int(L.lla_affine_grad_workspace_bytes(B, C))
    ww, ws = _guarded(nws // 4)
    for _ in range(2):
        rc = L.lla_affine_grad(P(dyd), ld, P(yd), ldy, P(sd), B, C, P(ad), 1.0 / B, P(gs), P(gb), P(ws), _st())
        _lib.check(rc, "lla_affine_grad")
        torch.cuda.synchronize()
        got = dict(scaling=gs.cpu().clone(), biasing=gb.cpu().clone())
        first = got if _ == 0 else first
    assert _intact(gsw, C) and _intact(gbw, C) and _intact(ww, nws // 4)
    assert all(torch.equal(first[k], got[k]) for k in got)
    _check(f"affine B={B} C={C}", got, ref, ref32)


def test_kernel_noise_is_hyperprior_noise():
    """Side stream: x = 0 makes s_hat = u, every element, to the bit -- at a width that is no multiple of 4, over many rows.
    z stream: one row at scaling = biasing = 0, z = 0 gives y = 0, v = u: the distortion's gradient for scaling is
    -sign(u + 1e-6) u exactly (one row: no sum), and with means 0 and scales 1 the sign of dy is the sign of u wherever
    |u| > 2^-10 (the likelihood is symmetric about the mean)."""
    for (B, S), (seed, step) in zip(((33, 102), (1000, 10), (5, 130)), ((0, 0), (SEED, STEP), (2 ** 63 + 5, 2 ** 32 - 1))):
        _, net, _, _ = H.side_case(1, S)
        got, ok = _device_side(torch.zeros(B, S), net.float(), seed=seed, step=step)
        assert ok and torch.equal(got["s_hat"], hyperprior_noise(seed, step, B, S, SIDE_TAG))
    for C, (seed, step) in zip((4095, 4096, 102), ((0, 0), (SEED, STEP), (2 ** 63 + 5, 2 ** 32 - 1))):
        gp = torch.cat([torch.ones(1, C), torch.zeros(1, C)], 1)
        got, ok = _device_gauss(torch.zeros(1, C), torch.zeros(C), torch.zeros(C), gp, scale=1.0, seed=seed, step=step)
        u = hyperprior_noise(seed, step, 1, C)[0].numpy()
        assert ok and np.array_equal(got["g_dist"].numpy(), (-np.sign(u + np.float32(1e-6)) * u).astype(np.float32))
        far = np.abs(u) > 2.0 ** -10
        assert np.array_equal(np.sign(got["dy"][0].numpy())[far], np.sign(u)[far])


def test_refusals_launch_nothing():
    L, P = _lib.lib(), _lib.ptr
    B, S, C = 8, 10, 12
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    x, net = torch.zeros(B, 16, device=DEV), torch.zeros(58 * S + 8, device=DEV)
    ow, o = _guarded(4096)
    sums = torch.full((4,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    assert L.lla_eb_side_pass_workspace_bytes(B, 0) == 0 and L.lla_eb_side_pass_workspace_bytes(-1, S) == 0
    assert L.lla_gaussian_train_pass_workspace_bytes(B, 0) == 0 and L.lla_affine_grad_workspace_bytes(-1, C) == 0

    def side(b=B, s=S, ldx=16, lds=16, ldd=16, xp=None, pp=None, sp=None, gp=None, op=None, wp=None):
        return L.lla_eb_side_pass(xp or P(x), ldx, b, s, pp or P(net), 1, 1, 1.0, sp or P(o), lds, P(o[1024:]), ldd,
                                  gp or P(o[2048:]), op or P(sums), wp or P(ws), _st())

    for rc in (side(s=0), side(b=-1), side(ldx=S - 1), side(lds=S - 1), side(ldd=S - 1), side(xp=off(x, 2)), side(pp=off(net, 4)),
               side(gp=off(o, 4)), side(op=off(sums, 4)), side(wp=off(ws, 4)), side(sp=off(o, 2))):
        assert rc == _lib.LLA_EINVAL
    assert side(b=0) == _lib.LLA_OK
    z, vec, gpb = torch.zeros(B, 16, device=DEV), torch.zeros(64, device=DEV), torch.ones(B, 32, device=DEV)

    def gauss(b=B, c=C, dt=_lib.LLA_Z_F32, ldz=16, ldg=32, ldy=16, bound=0.11, zp=None, sp=None, gpp=P(gpb), dgp=P(o), op=None, wp=None):
        return L.lla_gaussian_train_pass(zp or P(z), dt, ldz, b, c, sp or P(vec), P(vec[16:]), gpp, ldg, bound, 1, 1, 1.0, dgp,
                                         P(o[1024:]), ldy, P(o[2048:]), P(o[3072:]), op or P(sums), wp or P(ws), _st())

    for rc in (gauss(c=0), gauss(b=-1), gauss(dt=0), gauss(dt=7), gauss(ldz=C - 1), gauss(ldg=2 * C - 1), gauss(ldy=C - 1),
               gauss(bound=0.0), gauss(zp=off(z, 2)), gauss(sp=off(vec, 4)), gauss(dgp=None), gauss(op=off(sums, 4)),
               gauss(wp=off(ws, 4))):
        assert rc == _lib.LLA_EINVAL
    assert gauss(b=0) == _lib.LLA_OK

    def affine(b=B, c=C, ld=16, ldy=16, sp=None, gs=None, wp=None, dyp=None):
        return L.lla_affine_grad(dyp or P(z), ld, P(x), ldy, sp or P(vec), b, c, None, 0.0, gs or P(o), P(o[1024:]), wp or P(ws), _st())

    for rc in (affine(c=0), affine(b=-1), affine(ld=C - 1), affine(ldy=C - 1), affine(sp=off(vec, 4)), affine(gs=off(o, 4)),
               affine(wp=off(ws, 4)), affine(dyp=off(z, 2))):
        assert rc == _lib.LLA_EINVAL
    assert affine(b=0) == _lib.LLA_OK
    q, t = torch.zeros(S, 3, device=DEV), torch.zeros(3, device=DEV)
    aux = lambda **k: L.lla_eb_aux_grad_any(k.get("p", P(net)), k.get("q", P(q)), P(t), k.get("s", S), P(o), k.get("o", P(sums)), _st())
    for rc in (aux(s=0), aux(s=-4), aux(p=off(net, 4)), aux(q=off(q, 4)), aux(o=off(sums, 4))):
        assert rc == _lib.LLA_EINVAL
    torch.cuda.synchronize()
    assert bool((ow == SENTINEL).all()) and bool((sums == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------ the engine
def _rows(N, C, seed=0):
    """Rows whose scale varies from row to row: z_i = a_i g_i, a_i log-normal."""
    g = torch.Generator().manual_seed(seed)
    return torch.exp(0.7 * torch.randn(N, 1, generator=g)) * torch.randn(N, C, generator=g)


@pytest.mark.parametrize("C,B,steps,S,hidden", [(64, 256, 20, 12, 256), (300, 64, 4, 60, 300)])
def test_trajectory_against_the_twin(C, B, steps, S, hidden):
    """20 steps at the issue's shape; 4 at C = 300, where the hidden width 300 and C itself are padded to 304 in the engine's
    buffers (the other shapes of this file have hidden widths that are multiples of 8)."""
    beta = 0.1
    P, q, target = H.initial_parameters(C, seed=3)
    f32 = lambda v: [t.float() for t in v] if isinstance(v, list) else v.float()
    P32 = {k: f32(v) for k, v in P.items()}
    P, q32 = {k: [t.double() for t in v] if isinstance(v, list) else v.double() for k, v in P32.items()}, q.float()
    assert P["net"].shape[1] == S and P["side_W"][0].shape == (hidden, C)
    batches = [_rows(B, C, seed=20 + t) for t in range(steps)]
    betas = beta_schedule(beta, steps, "linear")
    adams = lambda: (_Adam(1e-3, 3e-8, (0.9, 0.999), 1e-8), _Adam(3e-4, 1e-6, (0.9, 0.999), 1e-8))
    twin = _TwinEngine(P, q32.double(), target, H.BOUND, *adams(), seed=SEED)
    devs = [_DeviceEngine(P, q32.double(), target, H.BOUND, *adams(), seed=SEED, device=DEV, max_batch=B, steps_per_epoch=steps)
            for _ in range(2)]
    # the fp32 evaluation: autograd in fp32 on the CPU over compressai's formulation, the same AdamW formulas on fp32 tensors
    a32, c32 = adams()
    mom = [(torch.zeros_like(p), torch.zeros_like(p)) for p in _flatten(P32)]
    momq, log32 = [(torch.zeros_like(q32), torch.zeros_like(q32))], []
    for t, zb in enumerate(batches):
        twin.step(zb, t, betas[t])
        for dev in devs:
            dev.step(zb.to(DEV), t, betas[t])
        G, sums = H.reference_step(P32, zb, hyperprior_noise(SEED, t, B, S, SIDE_TAG), hyperprior_noise(SEED, t, B, C), betas[t])
        _adamw(_flatten(P32), _flatten(G), mom, a32, t + 1)
        gq, aux = H.R.reference_aux(P32["net"], q32, target)
        _adamw([q32], [gq], momq, c32, t + 1)
        log32.append([float(v) for v in sums] + [float(aux)])
    (tp, tq), (dp, dq), (ep, eq) = twin.state(), devs[0].state(), devs[1].state()
    assert torch.equal(devs[0].flat[0], devs[1].flat[0]) and torch.equal(dq, eq), "two runs gave other bits"
    got, ref, ref32 = H.flat_groups(dp), H.flat_groups(tp), H.flat_groups(P32)
    got["quantiles"], ref["quantiles"], ref32["quantiles"] = dq.reshape(-1), tq.reshape(-1), q32.reshape(-1)
    assert all(a.shape == b.shape for a, b in zip(_flatten(dp), _flatten(tp))), "state() returned padded shapes"
    _check(f"trajectory C={C}", got, ref, ref32)
    tl, dl = twin.epoch_log(), devs[0].epoch_log()
    assert tl.shape == dl.shape == (steps, 4)
    # The sums of step 0 (dist, rate_z, rate_s, aux), where all three evaluations hold the same parameters, are bounded like a
    # kernel's sums.  Later steps' sums follow the drifting parameters; a sum over channels adds the drifts up, which the groups'
    # MAXIMA above do not measure: their worst departure is printed, not asserted (DESIGN.md 5.20 has the figures).
    names = ("dist", "rate_z", "rate_s", "aux")
    l32 = np.asarray(log32)
    print("trajectory sums, worst relative departure from the twin over the steps: "
          + "  ".join(f"{k} device {np.abs(dl[:, j] / tl[:, j] - 1).max():.2e} fp32 {np.abs(l32[:, j] / tl[:, j] - 1).max():.2e}"
                      for j, k in enumerate(names)))
    _check("trajectory sums of step 0", {k: torch.tensor([dl[0, j]]) for j, k in enumerate(names)},
           {k: torch.tensor([tl[0, j]]) for j, k in enumerate(names)}, {k: torch.tensor([l32[0, j]]) for j, k in enumerate(names)},
           sums=names)
    # pads of the flat buffer stay zero under AdamW: the padded side width (12 -> 16, 60 -> 64), hidden width and C (300 -> 304)
    p = devs[0].p
    assert not bool(p["side_W"][2][S:].any()) and not bool(p["z_W"][0][:, S:].any())
    assert not bool(p["side_W"][0][hidden:].any()) and not bool(p["side_W"][0][:, C:].any()) and not bool(p["side_b"][0][hidden:].any())
    assert not bool(p["side_W"][1][:, hidden:].any()) and not bool(p["z_W"][2][2 * C:].any()) and not bool(p["z_W"][2][:, hidden:].any())


def _payload_bits(m, z):
    payload, offsets = m.encode_device(z)
    return 8.0 * float(offsets[-1]) / z.shape[0], (payload, offsets)


_FIT = {}


def _fit():
    if not _FIT:
        Z = _rows(8192 + 2048, 64).to(DEV)
        _FIT["fit"] = HyperpriorFit(1e-1, epochs=5, batch_size=256, scheduler=None, seed=0).fit(Z[:8192])
        _FIT["Z"] = Z
    return _FIT["fit"], _FIT["Z"][:8192], _FIT["Z"][8192:]


def test_end_to_end_fit_codes_fewer_bits_than_the_untrained_module():
    fit, train, held = _fit()
    assert fit.engine_ == "device" and fit.rate_estimator_.scaling.is_cuda
    fresh = HyperpriorFit(1e-1, seed=0).initial_estimator(64).eval()
    fresh.update(force=True)
    fresh = fresh.to(DEV)
    m = fit.rate_estimator_
    trained, (payload, offsets) = _payload_bits(m, held)
    untrained, _ = _payload_bits(fresh, held)
    fac = BottleneckFit(1e-1, epochs=5, batch_size=256, scheduler=None, seed=0).fit(train).rate_estimator_
    fac_bits = 8.0 * sum(len(s) + 4 for s in fac.compress(held)[0]) / held.shape[0]       # (+ the 4-byte length prefix of a record)
    print(f"bits per row (records with their length prefixes): hyperprior trained {trained:.1f}, untrained {untrained:.1f}; "
          f"BottleneckFit at the same beta {fac_bits:.1f}; rate curve {fit.rate_curve_} side {fit.side_rate_curve_}")
    assert trained < untrained
    assert fit.loss_curve_[-1] < fit.loss_curve_[0] and fit.aux_curve_[-1] < fit.aux_curve_[0]
    assert torch.equal(m.decode_device(payload, offsets, held.shape[0]), m.represent_device(held))


def test_state_dict_loads_into_the_hub_entry_and_round_trips_a_dataset(tmp_path):
    import hubconf
    Z = _rows(2048, 512, seed=2).to(DEV)
    fit = HyperpriorFit(5e-2, epochs=2, batch_size=256, scheduler=None, seed=0).fit(Z)
    assert fit.rate_estimator_.side_z_dim == 102
    comp, _ = hubconf.clip_hyperprior_compressor(fit.state_dict(), device=DEV, clip_weights="synthetic")
    g = torch.Generator().manual_seed(0)
    images = torch.randn(64, 3, 224, 224, generator=g)
    file = tmp_path / "z.bin"
    comp.compress_dataset(images, str(file), is_info=False)
    z = comp.decompress_dataset(str(file), is_info=False)
    assert tuple(z.shape) == (64, 512)
    with torch.no_grad():
        want = comp(images.to(DEV))
    assert np.array_equal(z, want.float().cpu().numpy())


def test_fit_from_compressed_latents_equals_fit_from_its_rows(tmp_path):
    import hubconf
    from conftest import ROOT
    from lossyless_amd.rates import HRateFactorizedPrior
    from oracle import container
    comp, _ = hubconf.clip_compressor_b005(device=DEV, clip_weights="synthetic")
    sd = torch.load(os.path.join(ROOT, "lossyless_amd", "assets", "beta5e-02_factorized_rate.pt"), map_location="cpu",
                    weights_only=True)
    m = HRateFactorizedPrior(512)
    m.load_state_dict(sd)
    strings = m.to(DEV).eval().compress((_rows(600, 512, seed=4) * 0.5).to(DEV))[0]
    file = tmp_path / "z.bin"
    container.write_container(str(file), strings)
    ds = comp.open_dataset(file)
    kw = dict(epochs=2, batch_size=128, scheduler=None, seed=5)          # four full batches and one of 88 per epoch
    a = HyperpriorFit(5e-2, **kw).fit(ds).state_dict()
    b = HyperpriorFit(5e-2, **kw).fit(ds.all()).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
