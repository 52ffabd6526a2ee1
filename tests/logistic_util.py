"""Shared by test_logistic_probe_host.py and test_gpu_logistic_probe.py: the softmax-regression objective in float64, a
caller of ``lla_softmax_pass`` and the rounding bound its outputs are held to (no test in here)."""
import math

import torch

from probe_util import U, gamma

# Worst error of the device's expf / logf against float64, measured on an MI355X over every fp32 argument in the range
# the pass draws from (expf: all of [-inf, -0] with a normal result -- the row maximum is always subtracted; logf: all of
# [1, 4096] -- a row sum of at most K terms of at most 1, the largest 1), in ulps of the result: 0.8567 (at -5.28543615)
# and 1.8835 (at 992.580933).  The bound allows twice the measured error.  An error of c ulps is a
# relative error of at most 2 c u.
EXP_ULPS, LOG_ULPS = 2 * 0.8567, 2 * 1.8835
EPS_EXP, EPS_LOG = 2.0 * EXP_ULPS * U, 2.0 * LOG_ULPS * U
TINY = 2.0 ** -126                   # below it expf's result is subnormal: an absolute error instead of a relative one


def softmax_objective64(W, b, X, idx, w, Cw):
    """f = 1/2 (|W|^2 + |b|^2) + Cw sum_i w_i (lse_i - s_{i, y_i}) and its gradient (gW [K, C], gb [K]) in float64;
    idx [N] class indexes, w [N] row weights."""
    W, b, X, w = W.double(), b.double(), X.double(), w.double()
    s = X @ W.T + b
    lse = torch.logsumexp(s, 1)
    hot = torch.zeros_like(s).scatter_(1, idx[:, None], 1.0)
    R = Cw * w[:, None] * (torch.exp(s - lse[:, None]) - hot)
    f = 0.5 * (W * W).sum() + 0.5 * (b * b).sum() + Cw * (w * (lse - (s * hot).sum(1))).sum()
    return f, W + R.T @ X, b + R.sum(0)


def binomial_objective64(wv, b0, X, sign, w, Cw):
    """f = 1/2 (|w|^2 + b^2) + Cw sum_i w_i log(1 + exp(-y_i s_i)) and its gradient, float64; sign [N] of +-1."""
    wv, X, w, sign = wv.double(), X.double(), w.double(), sign.double()
    s = X @ wv + float(b0)
    r = -Cw * w * sign * torch.sigmoid(-sign * s)
    f = 0.5 * (wv * wv).sum() + 0.5 * float(b0) ** 2 + Cw * (w * torch.nn.functional.softplus(-sign * s)).sum()
    return f, wv + X.T @ r, float(b0) + r.sum()


def row_weights(probe, y, class_weight):
    """w_i = cw[y_i] as LogisticProbe / scikit-learn take ``class_weight`` -> (class index [N], w [N] float64)."""
    classes = torch.from_numpy(probe.classes_)
    idx = torch.searchsorted(classes, y)
    K = len(classes)
    if class_weight is None:
        cw = torch.ones(K, dtype=torch.float64)
    elif class_weight == "balanced":
        cw = y.numel() / (K * torch.bincount(idx, minlength=K).double())
    else:
        cw = torch.tensor([float(class_weight.get(int(c), 1.0)) for c in classes], dtype=torch.float64)
    return idx, cw[idx]


def softmax_pass(z, ld_z, y, B, C, W, b, V, vb, K, cw=None, out=None, accumulate=0):
    """``lla_softmax_pass`` on device tensors -> (out_W [K, C], out_b [K], out_loss float64 [K]); ``z`` is the flat
    storage of [B, ld_z] rows."""
    from lossyless_amd import _lib
    L = _lib.lib()
    dev = W.device
    if out is None:
        out = (torch.full((K, C), 7.0, device=dev), torch.full((K,), 7.0, device=dev),
               torch.full((K,), 7.0, dtype=torch.float64, device=dev))
    ws = torch.empty(int(L.lla_softmax_pass_workspace_bytes(C, K, B)), dtype=torch.uint8, device=dev)
    rc = L.lla_softmax_pass(_lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, ld_z, _lib.ptr(y), B, C,
                            _lib.ptr(W), _lib.ptr(b), _lib.ptr(V), _lib.ptr(vb), K, C, _lib.ptr(cw), _lib.ptr(out[0]),
                            _lib.ptr(out[1]), _lib.ptr(out[2]), accumulate, _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "lla_softmax_pass")
    torch.cuda.synchronize()
    return out


def softmax_reference_and_bound(Z, y, W, b, V=None, vb=None, cw=None):
    """float64 values of what ``lla_softmax_pass`` returns for rows Z (already the values the kernel sees), and the
    elementwise bound on |kernel - float64| of an fp32 evaluation -- derived as probe_util.reference_and_bound is, not
    picked.  With u the unit roundoff, eps_e / eps_l the relative error of expf / logf (above), D_i the spread of row i's
    computed scores (no argument of expf is larger in magnitude), T the number of class tiles and F = 1 (T = 1) or T + 1
    (T > 1) the exponential factors a term of the row sum passes through (its own, a rescale per later tile, the merge):

      scores     Es = gamma_{C+2} (|Z| |W|^T + |b|); lse is 1-Lipschitz in the sup norm: Esm_i = max_k Es_ik enters lse_i
      row sum    every term within exp(+-(u D + eps_e)) per factor, one rounding per rescale, K + 8 additions:
                                                                     Lsum = F (u D + eps_e) + (F - 1) u + gamma_{K+8}
      lse        max + logf(sum), log sum in [0, log K + Lsum], one rounding: E0 = Esm + Lsum + eps_l (log K + Lsum),
                                                                     Else = E0 + u (|lse| + E0)
      p          expf of the rounded s - lse:   Lp = Es + Else + u (|s - lse| + Es + Else) + eps_e,
                                                                     Ep = p expm1(Lp) + 2^-126
      a          weights p~ = e / sum within exp(+-La) of p, La = 2 (Esm + Lsum); t within Et of its value; K + 8 + F
                 more roundings in the numerator, one for the division:
                                          Ea0 = e^La sum_k p Et + (e^La (1 + gamma_{K+8+F}) - 1) sum_k p (|t| + Et),
                                                                     Ea = Ea0 + u (|a| + Ea0)
      residual   gradient: w (p^ - h), two roundings:                Er = w Ep + gamma_2 w (|p - h| + Ep)
                 HV: q = t - a, Eq = Et + Ea + u (|q| + Et + Ea);    Er = w (Ep |q| + (p + Ep) Eq) + gamma_2 w (p + Ep) (|q| + Eq)
      loss term  w (lse^ - s^_y): Ed = Else + Es_y + u (|lse - s_y| + Else + Es_y),   El = w Ed + u w (|lse - s_y| + Ed)
      sums       B terms added in some order (+ 8 for the partial sums):   Er^T |Z| + gamma_{B+8} (|R| + Er)^T |Z|
    A row whose label lies outside [0, K) weighs 0.  -> dict(W, b, loss) of float64 values and of bounds (loss: None in
    Hessian-vector mode)."""
    Z, W, b = Z.double(), W.double(), b.double()
    B, C = Z.shape
    K = W.shape[0]
    y = y.to(torch.int64)
    live = (y >= 0) & (y < K)
    yc = y.clamp(0, K - 1)
    w = (torch.ones(K, dtype=torch.float64, device=Z.device) if cw is None else cw.double())[yc] * live
    w = w[:, None]
    hot = torch.zeros((B, K), dtype=torch.float64, device=Z.device).scatter_(1, yc[:, None], 1.0) * live[:, None]
    ones = torch.ones(B, 1, dtype=torch.float64, device=Z.device)
    s = Z @ W.T + b
    Es = gamma(C + 2) * (Z.abs() @ W.abs().T + b.abs())
    Esm = Es.amax(1, keepdim=True)
    lse = torch.logsumexp(s, 1, keepdim=True)
    p = torch.exp(s - lse)
    T = -(-K // 32)
    F = 1 if T == 1 else T + 1
    D = s.amax(1, keepdim=True) - s.amin(1, keepdim=True) + 2.0 * Esm
    Lsum = F * (U * D + EPS_EXP) + (F - 1) * U + gamma(K + 8)
    E0 = Esm + Lsum + EPS_LOG * (math.log(K) + Lsum)
    Else = E0 + U * (lse.abs() + E0)
    Lp = Es + Else + U * ((s - lse).abs() + Es + Else) + EPS_EXP
    Ep = p * torch.expm1(Lp) + TINY
    gB = gamma(B + 8)
    if V is None:
        R = w * (p - hot)
        Er = w * Ep + gamma(2) * w * ((p - hot).abs() + Ep)
        d = lse - s                                                    # (only the label's column is used)
        Ed = Else + Es + U * (d.abs() + Else + Es)
        term = w * hot * d
        El = hot * (w * Ed + U * w * (d.abs() + Ed))
        val = dict(W=R.T @ Z, b=R.sum(0), loss=term.sum(0))
        loss_bound = El.sum(0) + gB * (term.abs() + El).sum(0)
    else:
        V, vb = V.double(), vb.double()
        t = Z @ V.T + vb
        Et = gamma(C + 2) * (Z.abs() @ V.abs().T + vb.abs())
        a = (p * t).sum(1, keepdim=True)
        La = 2.0 * (Esm + Lsum)
        Ea0 = torch.exp(La) * (p * Et).sum(1, keepdim=True) + \
            (torch.exp(La) * (1.0 + gamma(K + 8 + F)) - 1.0) * (p * (t.abs() + Et)).sum(1, keepdim=True)
        Ea = Ea0 + U * (a.abs() + Ea0)
        q = t - a
        Eq = Et + Ea + U * (q.abs() + Et + Ea)
        R = w * p * q
        Er = w * (Ep * q.abs() + (p + Ep) * Eq) + gamma(2) * w * (p + Ep) * (q.abs() + Eq)
        val = dict(W=R.T @ Z, b=R.sum(0), loss=None)
        loss_bound = None
    bound = dict(W=Er.T @ Z.abs() + gB * ((R.abs() + Er).T @ Z.abs()), b=(Er.T @ ones)[:, 0] + gB * (R.abs() + Er).sum(0),
                 loss=loss_bound)
    return val, bound
