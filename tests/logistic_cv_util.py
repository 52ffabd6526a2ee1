"""Shared by test_logistic_probe_cv_host.py and test_gpu_logistic_probe_cv.py: a caller of ``lla_softmax_grid_pass``, its
float64 values and bound per group (logistic_util.softmax_reference_and_bound on the group's own labels and weights), and
the checks of a fitted ``LogisticProbeCV`` against the float64 objective (no test in here)."""
import numpy as np
import torch

from logistic_util import binomial_objective64, softmax_objective64, softmax_reference_and_bound
from probe_cv_util import class_weights
from probe_util import make_data


# ------------------------------------------------------------------ the kernel
def softmax_grid_pass(z, ld_z, y, fold, B, C, W, b, V, vb, K, G, held, cw=None, out=None, accumulate=0):
    """``lla_softmax_grid_pass`` on device tensors -> (out_W [G K, C], out_b [G K], out_loss float64 [G K]); ``z`` is the
    flat storage of [B, ld_z] rows, ``held`` int32 [G], ``cw`` fp32 [G, K] or None, ``fold`` int32 [B] or None."""
    from lossyless_amd import _lib
    L = _lib.lib()
    dev = W.device
    if out is None:
        out = (torch.full((G * K, C), 7.0, device=dev), torch.full((G * K,), 7.0, device=dev),
               torch.full((G * K,), 7.0, dtype=torch.float64, device=dev))
    ws = torch.empty(int(L.lla_softmax_grid_pass_workspace_bytes(C, K, G)), dtype=torch.uint8, device=dev)
    rc = L.lla_softmax_grid_pass(_lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, ld_z, _lib.ptr(y),
                                 _lib.ptr(fold), B, C, _lib.ptr(W), _lib.ptr(b), _lib.ptr(V), _lib.ptr(vb), K, G, C,
                                 _lib.ptr(held), _lib.ptr(cw), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), accumulate,
                                 _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "lla_softmax_grid_pass")
    torch.cuda.synchronize()
    return out


def group_labels(y, fold, held, g):
    """The labels group g trains on: its held-out rows relabelled -1 (no class: weight 0)."""
    if fold is None:
        return y
    return torch.where(fold == held[g], torch.full_like(y, -1), y)


def grid_reference_and_bound(Z, y, fold, W, b, K, G, held, cw=None, V=None, vb=None):
    """softmax_reference_and_bound applied per group -- the selected weight adds no rounding, so the bound of
    ``lla_softmax_pass`` holds as it stands -> dicts of values and bounds in the dense [G K] layout."""
    vals, bounds = [], []
    for g in range(G):
        sl = slice(g * K, (g + 1) * K)
        val, bound = softmax_reference_and_bound(Z, group_labels(y, fold, held, g), W[sl], b[sl], None if V is None else V[sl],
                                                 None if vb is None else vb[sl], None if cw is None else cw[g])
        vals.append(val), bounds.append(bound)
    cat = lambda ds, k: None if ds[0][k] is None else torch.cat([d[k] for d in ds])          # noqa: E731
    return {k: cat(vals, k) for k in ("W", "b", "loss")}, {k: cat(bounds, k) for k in ("W", "b", "loss")}


# ------------------------------------------------------------------ the fitted search against the float64 objective
def unbalanced(N, C, K):
    """make_data with class k given about (k + 1) shares of the rows, every class at least three times (so that every
    training part of two or three stratified folds has it)."""
    X, _ = make_data(N, C, K)
    g = torch.Generator().manual_seed(N + K)
    shares = torch.arange(1, K + 1, dtype=torch.float64)
    y = torch.multinomial(shares / shares.sum(), N, replacement=True, generator=g)
    y[:3 * K] = torch.arange(K).repeat(3)
    mu = torch.randn(K, C, generator=g) * 0.6
    return (X + mu[y]).float(), y


def stacked(W, b):
    return torch.cat([W.double().cpu().reshape(W.shape[0], -1), b.double().cpu().reshape(-1, 1)], 1)


def gradient64(W, b, X, labels, classes, Cw, class_weight):
    """float64 gradient of the objective ``LogisticProbe`` documents at (W, b) as returned ([K, C] / [1, C] for two
    classes), over the rows (X, labels), class weights counted on those rows -> flat tensor."""
    labels = torch.as_tensor(np.asarray(labels))
    idx = torch.searchsorted(torch.from_numpy(np.asarray(classes)), labels)
    w = torch.from_numpy(class_weights(class_weight, classes, labels.numpy()))[idx]
    W, b = W.double().cpu(), b.double().cpu()
    if len(classes) == 2:
        _, gw, gb = binomial_objective64(W[0], b[0], X, 2.0 * idx.double() - 1.0, w, Cw)
        return torch.cat([gw, gb.reshape(1)])
    _, gW, gb = softmax_objective64(W, b, X, idx, w, Cw)
    return stacked(gW, gb).reshape(-1)


def within_strong_convexity(Wa, ba, Wb, bb, X, labels, classes, Cw, class_weight, what=""):
    """f is 1-strongly convex: |theta_a - theta_b|_2 <= |grad f(theta_a)|_2 + |grad f(theta_b)|_2."""
    d = float((stacked(Wa, ba) - stacked(Wb, bb)).norm())
    ga = float(gradient64(Wa, ba, X, labels, classes, Cw, class_weight).norm())
    gb = float(gradient64(Wb, bb, X, labels, classes, Cw, class_weight).norm())
    print(f"{what}: |a - b| {d:.3e} <= {ga:.3e} + {gb:.3e}")
    assert d <= ga + gb, f"{what}: {d:.3e} > {ga:.3e} + {gb:.3e}"
    return d
