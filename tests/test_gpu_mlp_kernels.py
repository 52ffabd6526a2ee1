"""GPU: the kernels of csrc/mlp.hip through the C ABI against float64 torch, element by element.

The two GEMMs are held to the standard forward bound of an fp32 fma chain of length L, |got - want| <= 2 L 2^-24 (|A| |B|)
(derived, not measured); ``lla_softmax_xent`` and ``lla_adamw_step`` to the bounds their tests state.  Every shape is called
twice (the same bits) into buffers whose pitch is larger than their width (the bytes between stay a sentinel)."""
import ctypes

import pytest
import torch

from lossyless_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = -123.25


def _padded(t, pad, fill=SENTINEL):
    """[R, C] -> (flat [R, C + pad] on the device with the padding set to ``fill``, pitch)."""
    R, C = t.shape
    flat = torch.full((R, C + pad), fill, dtype=t.dtype)
    flat[:, :C] = t
    return flat.cuda(), C + pad


def _gemm_nn(dY, ldy, W, ldw, H, ldh, M, N, K, pad=8):
    out = torch.full((max(M, 1), K + pad), SENTINEL, dtype=torch.float32, device="cuda")
    rc = _lib.lib().lla_gemm_f32_nn(_lib.ptr(dY), ldy, _lib.ptr(W), ldw, _lib.ptr(H), ldh, _lib.ptr(out), K + pad, M, N, K,
                                    _lib.stream_ptr())
    _lib.check(rc, "lla_gemm_f32_nn")
    torch.cuda.synchronize()
    return out


def _gemm_tn(dY, ldy, X, ldx, M, N, K, with_db, pad=8):
    dW = torch.full((N, K + pad), SENTINEL, dtype=torch.float32, device="cuda")
    db = torch.full((N + pad,), SENTINEL, dtype=torch.float32, device="cuda")
    rc = _lib.lib().lla_gemm_f32_tn(_lib.ptr(dY), ldy, _lib.ptr(X), ldx, _lib.ptr(dW), K + pad, _lib.ptr(db) if with_db else None,
                                    M, N, K, _lib.stream_ptr())
    _lib.check(rc, "lla_gemm_f32_tn")
    torch.cuda.synchronize()
    return dW, db


@pytest.mark.parametrize("mask", [False, True], ids=["plain", "relu-mask"])
def test_gemm_nn_against_float64(mask):
    g = torch.Generator().manual_seed(11)
    worst = 0.0
    for M in (1, 31, 33, 100):
        for N in (4, 36, 64):
            for K in (8, 40, 520):
                dY, ldy = _padded(torch.randn(M, N, generator=g), 4, float("nan"))
                W, ldw = _padded(torch.randn(N, K, generator=g), 4, float("nan"))
                H = ldh = None
                if mask:                     # a forward ReLU output: positive values, exact zeros and negative zeros
                    h = torch.randn(M, K, generator=g).clamp_min(0.0)
                    h[torch.rand(M, K, generator=g) < 0.2] = -0.0
                    assert bool((h == 0).any()) and bool(torch.signbit(h).any()) and bool((h > 0).any())
                    H, ldh = _padded(h, 8, 1.0)
                got = _gemm_nn(dY, ldy, W, ldw, H, ldh or 0, M, N, K)
                a, b = dY[:, :N].double(), W[:, :K].double()
                want, bound = a @ b, 2 * N * U * (a.abs() @ b.abs())
                if mask:
                    keep = H[:, :K] > 0
                    want, bound = torch.where(keep, want, 0.0), torch.where(keep, bound, 0.0)
                    assert bool((got[:, :K][~keep] == 0).all())
                err = (got[:, :K].double() - want).abs()
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
                assert bool((err <= bound).all()), f"M {M} N {N} K {K}: error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3g}"
                assert bool((got[:, K:] == SENTINEL).all()), f"M {M} N {N} K {K}: wrote beyond the width"
                assert torch.equal(_gemm_nn(dY, ldy, W, ldw, H, ldh or 0, M, N, K), got)
    print(f"lla_gemm_f32_nn ({'mask' if mask else 'plain'}): worst error / bound {worst:.3g}")


@pytest.mark.parametrize("with_db", [False, True], ids=["dW", "dW+db"])
def test_gemm_tn_against_float64(with_db):
    g = torch.Generator().manual_seed(12)
    worst = 0.0
    for M in (1, 2, 31, 33, 257):
        for N in (4, 36):
            for K in (8, 520):
                dY, ldy = _padded(torch.randn(M, N, generator=g), 4, float("nan"))
                X, ldx = _padded(torch.randn(M, K, generator=g), 8, float("nan"))
                dW, db = _gemm_tn(dY, ldy, X, ldx, M, N, K, with_db)
                a, b = dY[:, :N].double(), X[:, :K].double()
                want, bound = a.T @ b, 2 * M * U * (a.abs().T @ b.abs())
                err = (dW[:, :K].double() - want).abs()
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
                assert bool((err <= bound).all()), f"M {M} N {N} K {K}: error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3g}"
                assert bool((dW[:, K:] == SENTINEL).all()) and bool((db[N:] == SENTINEL).all())
                if with_db:
                    err_b = (db[:N].double() - a.sum(0)).abs()
                    assert bool((err_b <= 2 * M * U * a.abs().sum(0)).all()), f"M {M} N {N} K {K}: db"
                else:
                    assert bool((db == SENTINEL).all())
                dW2, db2 = _gemm_tn(dY, ldy, X, ldx, M, N, K, with_db)
                assert torch.equal(dW2, dW) and torch.equal(db2, db)
    print(f"lla_gemm_f32_tn: worst error / bound {worst:.3g}")


def _xent(logits, ld, y, B, K, kpad, scale, pad=8):
    L = _lib.lib()
    d = torch.full((max(B, 1), kpad + pad), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    right = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.lla_softmax_xent_workspace_bytes(B)), dtype=torch.uint8, device="cuda")
    rc = L.lla_softmax_xent(_lib.ptr(logits), ld, _lib.ptr(y), B, K, kpad, scale, _lib.ptr(d), kpad + pad, _lib.ptr(loss),
                            _lib.ptr(right), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "lla_softmax_xent")
    torch.cuda.synchronize()
    return d, loss, right


@pytest.mark.parametrize("K", [1, 2, 10, 33, 1000])
def test_softmax_xent_against_float64(K):
    g = torch.Generator().manual_seed(100 + K)
    kpad = -(-K // 8) * 8
    for B in (1, 33, 257):
        s = torch.randn(B, K, generator=g) * 3
        s[0] = 80.0 * torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0) + torch.randn(K, generator=g)   # magnitude 80
        if K > 1:                            # a gap of at least 1e-3 between the top two of every row
            top = s.topk(2, 1)
            close = (top.values[:, 0] - top.values[:, 1]) < 1e-3
            s[close, top.indices[close, 0]] += 1.0
            top = s.topk(2, 1).values
            assert float((top[:, 0] - top[:, 1]).min()) >= 1e-3
        y = torch.randint(0, K, (B,), generator=g)
        y[::3] = s.argmax(1)[::3]            # (so that some rows are right)
        if B > 1:
            y[1], y[B - 1] = -1, K           # no class: zero residual, counted nowhere
        valid = (y >= 0) & (y < K)
        scale = 1.0 / max(int(valid.sum()), 1)
        logits, ld = _padded(s, kpad - K + 4, float("nan"))
        d, loss, right = _xent(logits, ld, y.to(torch.int32).cuda(), B, K, kpad, scale)
        s64, yv = s.double(), y.clamp(0, K - 1)
        hot = torch.zeros(B, K, dtype=torch.float64).scatter_(1, yv[:, None], 1.0)
        want = scale * (torch.softmax(s64, 1) - hot) * valid[:, None]
        want_loss = float(((torch.logsumexp(s64, 1) - s64.gather(1, yv[:, None])[:, 0]) * valid).sum())
        want_right = int(((s64.argmax(1) == y) & valid).sum())
        got = d.cpu()
        assert bool(torch.isfinite(got).all())
        err = float((got[:, :K].double() - want).abs().max())
        assert err <= 8 * U * scale, f"K {K} B {B}: residual error {err:.3e} against {8 * U * scale:.3e}"
        assert not got[:, :K][~valid].any()
        assert not got[:, K:kpad].any(), "padded columns must be exactly 0"
        assert bool((got[:, kpad:] == SENTINEL).all())
        lim = B * (K + 8) * U * max(1.0, float(s.abs().max()))
        assert abs(float(loss) - want_loss) <= lim, f"K {K} B {B}: loss {float(loss)} against {want_loss} +- {lim:.3e}"
        assert int(right) == want_right, f"K {K} B {B}"
        d2, loss2, right2 = _xent(logits, ld, y.to(torch.int32).cuda(), B, K, kpad, scale)
        assert torch.equal(d2, d) and torch.equal(loss2, loss) and torch.equal(right2, right)


def test_softmax_xent_takes_the_lowest_index_on_ties():
    s = torch.tensor([[1.0, 5.0, 5.0, 0.0], [1.0, 5.0, 5.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, 0.0, 3.0, 3.0]])
    y = torch.tensor([1, 2, 0, 3], dtype=torch.int32)
    assert s.argmax(1).tolist() == [1, 1, 0, 2]
    _, _, right = _xent(s.cuda(), 4, y.cuda(), 4, 4, 8, 0.25)
    assert int(right) == 2
    wide = torch.zeros(2, 200)               # ties across lanes and across a lane's own columns
    wide[0, [70, 134, 6]] = 4.0
    wide[1, [199, 135]] = 4.0
    for labels, want in (([6, 135], 2), ([70, 199], 0)):
        _, _, right = _xent(wide.cuda(), 200, torch.tensor(labels, dtype=torch.int32).cuda(), 2, 200, 200, 0.5)
        assert int(right) == want


def _adamw(p, g, m, v, n, hp, t):
    lr, b1, b2, eps, wd = hp
    rc = _lib.lib().lla_adamw_step(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), n, lr, b1, b2, eps, wd, 1.0 - b1 ** t,
                                   1.0 - b2 ** t, _lib.stream_ptr())
    _lib.check(rc, "lla_adamw_step")
    torch.cuda.synchronize()


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("t", [1, 1000])
def test_adamw_step_against_float64(t, wd):
    gen = torch.Generator().manual_seed(7 * t + 1)
    hp = (1e-3, 0.9, 0.999, 1e-8, wd)
    lr, b1, b2, eps, _ = hp
    for n in (1, 3, 4, 1027):
        p0 = torch.randn(n, generator=gen)
        g = torch.randn(n, generator=gen)
        g[torch.arange(n) % 5 == 1] = 0.0                                            # exact zeros
        tiny = torch.arange(n) % 5 == 2
        g[tiny] = 1e-8 * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)[tiny]
        if n == 1:
            g[0] = 1e-8
        m0 = torch.randn(n, generator=gen) * 0.1
        v0 = torch.rand(n, generator=gen) * 0.01
        fresh = torch.arange(n) % 7 == 3                                             # moments that have seen nothing yet
        m0[fresh], v0[fresh] = 0.0, 0.0
        tail = torch.full((5,), SENTINEL)
        bufs = [torch.cat([x, tail]).cuda() for x in (p0, g, m0, v0)]
        _adamw(*bufs, n, hp, t)
        p, _, m, v = (b.cpu() for b in bufs)
        assert all(bool((b[n:] == SENTINEL).all()) for b in (p, m, v)) and torch.equal(bufs[1].cpu()[:n], g)
        g64 = g.double()
        m64 = b1 * m0.double() + (1 - b1) * g64
        v64 = b2 * v0.double() + (1 - b2) * g64 * g64
        update = (lr / (1 - b1 ** t)) * m64 / (v64.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        p64 = p0.double() * (1 - lr * wd) - update
        assert bool(((m[:n].double() - m64).abs() <= 4 * U * m64.abs()).all()), f"n {n}: m"
        assert bool(((v[:n].double() - v64).abs() <= 4 * U * v64.abs()).all()), f"n {n}: v"
        lim = 16 * U * (p0.double().abs() + update.abs())
        err = (p[:n].double() - p64).abs()
        assert bool((err <= lim).all()), f"n {n}: p error / bound = {float((err / lim.clamp_min(1e-300)).max()):.3g}"
        assert bool((v[:n] >= 0).all()) and bool(torch.isfinite(p[:n]).all())


def test_refusals_and_empty_calls():
    L = _lib.lib()
    buf = torch.zeros(1 << 14, dtype=torch.float32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    off = ctypes.c_void_p(buf.data_ptr() + 4)
    E, OK = _lib.LLA_EINVAL, _lib.LLA_OK
    nn = lambda **k: L.lla_gemm_f32_nn(*[{**dict(dY=p, ldy=8, W=p, ldw=8, H=None, ldh=0, dX=p, ldx=8, M=4, N=8, K=8, st=None), **k}[a]  # noqa: E731
                                         for a in ("dY", "ldy", "W", "ldw", "H", "ldh", "dX", "ldx", "M", "N", "K", "st")])
    assert nn(N=6) == E and nn(K=6) == E and nn(N=0) == E and nn(K=0) == E and nn(M=-1) == E
    assert nn(ldy=4) == E and nn(ldw=4) == E and nn(ldx=4) == E and nn(ldy=10) == E and nn(ldx=10) == E
    assert nn(H=p, ldh=4) == E and nn(H=p, ldh=10) == E and nn(H=off, ldh=8) == E
    assert nn(dY=off) == E and nn(dX=off) == E and nn(dY=None) == E and nn(W=None) == E and nn(dX=None) == E
    assert nn(M=0, dY=None, W=None, dX=None) == OK
    tn = lambda **k: L.lla_gemm_f32_tn(*[{**dict(dY=p, ldy=8, X=p, ldx=8, dW=p, ldw=8, db=None, M=4, N=8, K=8, st=None), **k}[a]  # noqa: E731
                                         for a in ("dY", "ldy", "X", "ldx", "dW", "ldw", "db", "M", "N", "K", "st")])
    assert tn(N=6) == E and tn(K=6) == E and tn(N=0) == E and tn(K=0) == E and tn(M=-1) == E
    assert tn(ldy=4) == E and tn(ldx=4) == E and tn(ldw=4) == E and tn(ldy=10) == E and tn(ldx=10) == E
    assert tn(dY=off) == E and tn(X=off) == E and tn(dY=None) == E and tn(X=None) == E and tn(dW=None) == E
    assert tn(M=0, dY=None, X=None, dW=None) == OK
    xe = lambda **k: L.lla_softmax_xent(*[{**dict(s=p, ld=8, y=p, B=4, K=8, kpad=8, scale=0.25, d=p, ldd=8, loss=p, right=p, ws=p, st=None),  # noqa: E731
                                          **k}[a] for a in ("s", "ld", "y", "B", "K", "kpad", "scale", "d", "ldd", "loss", "right", "ws", "st")])
    assert xe(K=0) == E and xe(K=1025, kpad=1032, ld=1032, ldd=1032) == E and xe(kpad=4) == E and xe(ld=4) == E
    assert xe(ldd=4) == E and xe(B=-1) == E
    for name in ("s", "y", "d", "loss", "right", "ws"):
        assert xe(**{name: None}) == E, name
    assert xe(B=0, s=None, y=None, d=None, loss=None, right=None, ws=None) == OK
    assert L.lla_softmax_xent_workspace_bytes(-1) == 0 and L.lla_softmax_xent_workspace_bytes(100) == 800
    ad = lambda **k: L.lla_adamw_step(*[{**dict(p=p, g=p, m=p, v=p, n=8, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, bc1=0.1, bc2=0.001,  # noqa: E731
                                                st=None), **k}[a] for a in ("p", "g", "m", "v", "n", "lr", "b1", "b2", "eps", "wd", "bc1", "bc2", "st")])
    assert ad(n=-1) == E and ad(b1=1.0) == E and ad(b2=-0.1) == E and ad(lr=-1.0) == E and ad(wd=-1.0) == E
    assert ad(bc1=0.0) == E and ad(bc2=0.0) == E and ad(eps=-1.0) == E
    for name in ("p", "g", "m", "v"):
        assert ad(**{name: None}) == E and ad(**{name: off}) == E, name
    assert ad(n=0, p=None, g=None, m=None, v=None) == OK
    torch.cuda.synchronize()
    assert not buf.any()                     # nothing was launched
