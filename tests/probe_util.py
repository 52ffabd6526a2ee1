"""Shared by test_probe_host.py and test_gpu_probe.py: seeded data, the LinearSVC objective in float64, a caller of
``lla_svm_pass`` and the rounding bound its outputs are held to (no test in here)."""
import ctypes

import numpy as np
import torch

U = 2.0 ** -24                       # unit roundoff of fp32


def gamma(n):
    return n * U / (1.0 - n * U)


def make_data(N, C, K, seed=1, sep=0.6):
    """Class means plus unit noise, fp32-representable -> (X float32 [N, C], y int64 [N] with every class present)."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(K, C, generator=g, dtype=torch.float64) * sep
    y = (torch.arange(N) % K)[torch.randperm(N, generator=g)]
    X = mu[y] + torch.randn(N, C, generator=g, dtype=torch.float64)
    return X.float(), y


def signs(idx, K):
    """class indexes [N] (anything outside [0, K) is negative everywhere) -> float64 [N, K] of +-1, on idx's device."""
    return torch.where(idx[:, None] == torch.arange(K, device=idx.device)[None, :], 1.0, -1.0).double()


def probe_signs(probe, y):
    """The +-1 matrix of a fitted LinearProbe / LinearSVC for labels y (two classes: one column, classes_[1] positive)."""
    classes = torch.from_numpy(np.asarray(probe.classes_))
    idx = torch.searchsorted(classes, y)
    if len(classes) == 2:
        return torch.where(idx == 1, 1.0, -1.0).double()[:, None]
    return signs(idx, len(classes))


def objective64(W, b, X, Y, Cw):
    """f_k summed over k, and its gradient (gW [K, C], gb [K]) in float64."""
    W, b, X = W.double(), b.double(), X.double()
    m = (1.0 - Y * (X @ W.T + b)).clamp_min(0.0)
    R = -2.0 * Cw * Y * m
    f = 0.5 * (W * W).sum() + 0.5 * (b * b).sum() + Cw * (m * m).sum()
    return f, W + R.T @ X, b + R.sum(0)


def grad_norms(W, b, X, Y, Cw):
    """-> (sup norm, 2-norm) of the float64 gradient with the intercept as one more column."""
    _, gW, gb = objective64(W, b, X, Y, Cw)
    g = torch.cat([gW, gb[:, None]], 1)
    return float(g.abs().max()), float(g.norm())


def svm_pass(z, ld_z, y, B, C, W, b, V, vb, K, out=None, accumulate=0):
    """``lla_svm_pass`` on device tensors -> (out_W [K, C], out_b [K], out_loss float64 [K]); ``z`` is the flat
    storage of [B, ld_z] rows."""
    from lossyless_amd import _lib
    L = _lib.lib()
    dev = W.device
    if out is None:
        out = (torch.full((K, C), 7.0, device=dev), torch.full((K,), 7.0, device=dev),
               torch.full((K,), 7.0, dtype=torch.float64, device=dev))
    ws = torch.empty(int(L.lla_svm_pass_workspace_bytes(C, K)), dtype=torch.uint8, device=dev)
    rc = L.lla_svm_pass(_lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, ld_z, _lib.ptr(y), B, C,
                        _lib.ptr(W), _lib.ptr(b), _lib.ptr(V), _lib.ptr(vb), K, C, _lib.ptr(out[0]), _lib.ptr(out[1]),
                        _lib.ptr(out[2]), accumulate, _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "lla_svm_pass")
    torch.cuda.synchronize()
    return out


def reference_and_bound(Z, y, W, b, V=None, vb=None):
    """float64 values of what ``lla_svm_pass`` returns for rows Z (already the values the kernel sees), and the
    elementwise bound on |kernel - float64| of an fp32 evaluation -- derived, not picked:

      scores      C products and C + 1 additions in some order:             Es = gamma_{C+2} (|Z| |W|^T + |b|)
      residuals   y s exact, 1 - y s rounded once, the hinge 1-Lipschitz,
                  the factor 2 exact:                                      Er = 2 (Es + u (1 + |s| + Es))
      sums        B terms added in some order (+ 8 for the partial sums):   |G^ - G| <= Er^T |Z| + gamma_{B+8} |R|^T |Z|
      loss        m^2 with |m^ - m| <= Er / 2, one rounding, then the sum.
    Hessian-vector mode: t has the scores' bound with V for W; where the margin is within its own rounding error of 0
    the kernel may take the element for active or not, so there the whole of 2 |t| is allowed.
    -> dict(W, b, loss) of float64 values and dict(W, b, loss) of bounds (loss: None in Hessian-vector mode)."""
    Z, W, b = Z.double(), W.double(), b.double()
    B, C = Z.shape
    K = W.shape[0]
    Y = signs(y.to(torch.int64), K)
    ones = torch.ones(B, 1, dtype=torch.float64, device=Z.device)
    s = Z @ W.T + b
    Es = gamma(C + 2) * (Z.abs() @ W.abs().T + b.abs())
    margin = 1.0 - Y * s
    m = margin.clamp_min(0.0)
    Er = 2.0 * (Es + U * (1.0 + s.abs() + Es))
    gB = gamma(B + 8)
    if V is None:
        R = -2.0 * Y * m
        Em = Er / 2.0
        El = Em * (2.0 * m + Em) + U * (m + Em) ** 2
        val = dict(W=R.T @ Z, b=R.sum(0), loss=(m * m).sum(0))
        bound = dict(W=Er.T @ Z.abs() + gB * (R.abs().T @ Z.abs()), b=(Er.T @ ones)[:, 0] + gB * R.abs().sum(0),
                     loss=El.sum(0) + gB * ((m + Em) ** 2).sum(0))
        return val, bound
    V, vb = V.double(), vb.double()
    t = Z @ V.T + vb
    Et = gamma(C + 2) * (Z.abs() @ V.abs().T + vb.abs())
    R = 2.0 * torch.where(margin > 0, t, torch.zeros_like(t))
    Er = torch.where(margin.abs() <= Er / 2.0, 2.0 * (t.abs() + Et), 2.0 * Et)
    val = dict(W=R.T @ Z, b=R.sum(0), loss=None)
    bound = dict(W=Er.T @ Z.abs() + gB * (R.abs().T @ Z.abs()), b=(Er.T @ ones)[:, 0] + gB * R.abs().sum(0), loss=None)
    return val, bound


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)
