"""Shared by test_probe_cv_host.py and test_gpu_probe_cv.py: a caller of ``lla_svm_grid_pass``, its float64 values with
the rounding bound of probe_util.reference_and_bound extended by the weight, liblinear's class-weighted objective in
float64 (written here from the definition, not taken from the package), and small class-separated containers (no test
in here)."""
import numpy as np
import torch

from probe_util import U, gamma


# ------------------------------------------------------------------ the kernel
def grid_pass(z, ld_z, y, fold, B, C, W, b, V, vb, cols, out=None, accumulate=0):
    """``lla_svm_grid_pass`` on device tensors -> (out_W [J, C], out_b [J], out_loss float64 [J]); ``z`` is the flat
    storage of [B, ld_z] rows, ``cols`` = (col_class, col_held int32 [J], col_cpos, col_cneg fp32 [J])."""
    from lossyless_amd import _lib
    L = _lib.lib()
    dev, J = W.device, W.shape[0]
    if out is None:
        out = (torch.full((J, C), 7.0, device=dev), torch.full((J,), 7.0, device=dev),
               torch.full((J,), 7.0, dtype=torch.float64, device=dev))
    ws = torch.empty(int(L.lla_svm_grid_pass_workspace_bytes(C, J)), dtype=torch.uint8, device=dev)
    rc = L.lla_svm_grid_pass(_lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, ld_z, _lib.ptr(y),
                             _lib.ptr(fold), B, C, _lib.ptr(W), _lib.ptr(b), _lib.ptr(V), _lib.ptr(vb), J, C,
                             *[_lib.ptr(t) for t in cols], _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), accumulate,
                             _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "lla_svm_grid_pass")
    torch.cuda.synchronize()
    return out


def signs_and_weights(y, fold, cols):
    """-> (y_ij of +-1, c_ij) float64 [B, J]: c_ij = 0 where fold[i] == col_held[j], else col_cpos / col_cneg by the sign."""
    cls, held, cpos, cneg = cols
    Y = torch.where(y[:, None] == cls[None, :], 1.0, -1.0).double()
    c = torch.where(Y > 0, cpos.double()[None, :], cneg.double()[None, :])
    if fold is not None:
        c = torch.where(fold[:, None] == held[None, :], torch.zeros((), dtype=torch.float64, device=c.device), c)
    return Y, c


def grid_reference_and_bound(Z, y, fold, W, b, cols, V=None, vb=None):
    """float64 values of what ``lla_svm_grid_pass`` returns, and the elementwise bound on |kernel - float64|: that of
    probe_util.reference_and_bound (scores Es, residuals Er, sums gamma_{B+8}, the loss term's El; same symbols) with one
    more fp32 rounding per element for the weight, which is an exact fp32 number:

      residual   c r, r known to Er, the product rounded once:      c (Er + u (|r| + Er))
      loss term  c m^2, m^2 known to El (its own rounding inside):  c (El + u (m^2 + El))
    A held-out element has c = 0: value 0, bound 0.
    -> dict(W, b, loss) of float64 values and dict(W, b, loss) of bounds (loss: None in Hessian-vector mode)."""
    Z, W, b = Z.double(), W.double(), b.double()
    B, C = Z.shape
    Y, c = signs_and_weights(y, fold, cols)
    ones = torch.ones(B, 1, dtype=torch.float64, device=Z.device)
    s = Z @ W.T + b
    Es = gamma(C + 2) * (Z.abs() @ W.abs().T + b.abs())
    margin = 1.0 - Y * s
    m = margin.clamp_min(0.0)
    Er = 2.0 * (Es + U * (1.0 + s.abs() + Es))
    gB = gamma(B + 8)
    loss = lbound = None
    if V is None:
        R0 = -2.0 * Y * m
        Em = Er / 2.0
        l0 = m * m
        El = Em * (2.0 * m + Em) + U * (m + Em) ** 2
        loss = (c * l0).sum(0)
        lbound = (c * (El + U * (l0 + El))).sum(0) + gB * (c * (m + Em) ** 2).sum(0)
    else:
        V, vb = V.double(), vb.double()
        t = Z @ V.T + vb
        Et = gamma(C + 2) * (Z.abs() @ V.abs().T + vb.abs())
        R0 = 2.0 * torch.where(margin > 0, t, torch.zeros_like(t))
        Er = torch.where(margin.abs() <= Er / 2.0, 2.0 * (t.abs() + Et), 2.0 * Et)
    R = c * R0
    Ec = c * (Er + U * (R0.abs() + Er))
    val = dict(W=R.T @ Z, b=R.sum(0), loss=loss)
    bound = dict(W=Ec.T @ Z.abs() + gB * (R.abs().T @ Z.abs()), b=(Ec.T @ ones)[:, 0] + gB * R.abs().sum(0), loss=lbound)
    return val, bound


# ------------------------------------------------------------------ liblinear's class-weighted objective
def class_weights(class_weight, classes, labels):
    """w[k] for the sorted labels ``classes`` (numpy), from the rows actually fitted: ``None`` -> 1, ``"balanced"`` ->
    n / (K count_k), a dict -> its values (1 for a label it leaves out)."""
    labels = np.asarray(labels)
    if class_weight is None:
        return np.ones(len(classes))
    if isinstance(class_weight, str):
        assert class_weight == "balanced"
        return len(labels) / (len(classes) * np.array([(labels == k).sum() for k in classes], dtype=np.float64))
    return np.array([float(class_weight.get(int(k), 1.0)) for k in classes])


def ovr_weights(labels, classes, Cw, class_weight):
    """-> (Y, c) float64 [N, K] ([N, 1] for two classes, positive ``classes[1]``): classifier k weighs the rows of class k
    by C w[k] and every other row by C; the single classifier of two classes weighs its negatives by C w[classes[0]]."""
    labels = torch.as_tensor(np.asarray(labels))
    w = torch.from_numpy(class_weights(class_weight, classes, labels.numpy()))
    cl = torch.from_numpy(np.asarray(classes))
    if len(classes) == 2:
        Y = torch.where(labels == cl[1], 1.0, -1.0).double()[:, None]
        return Y, Cw * torch.where(Y > 0, w[1], w[0])
    Y = torch.where(labels[:, None] == cl[None, :], 1.0, -1.0).double()
    return Y, torch.where(Y > 0, Cw * w[None, :], torch.full((), Cw, dtype=torch.float64))


def weighted_grad_norms(W, b, X, Y, c):
    """(sup norm, 2-norm) of the float64 gradient of sum_k 1/2 (|w_k|^2 + b_k^2) + sum_i c_ik max(0, 1 - y_ik s_ik)^2,
    the intercept as one more column."""
    W, b, X = W.double().cpu(), b.double().cpu(), X.double()
    m = (1.0 - Y * (X @ W.T + b)).clamp_min(0.0)
    R = -2.0 * c * Y * m
    g = torch.cat([W + R.T @ X, (b + R.sum(0))[:, None]], 1)
    return float(g.abs().max()), float(g.norm())


def distance(Wa, ba, Wb, bb):
    return float(torch.cat([Wa.double().cpu() - Wb.double().cpu(), (ba.double().cpu() - bb.double().cpu())[:, None]], 1).norm())


def within_strong_convexity(Wa, ba, Wb, bb, X, Y, c, what=""):
    """f is 1-strongly convex, so both points are within their gradient's norm of the minimiser:
    |Wa - Wb| <= |grad f(Wa)| + |grad f(Wb)|."""
    d = distance(Wa, ba, Wb, bb)
    ga, gb = weighted_grad_norms(Wa, ba, X, Y, c)[1], weighted_grad_norms(Wb, bb, X, Y, c)[1]
    print(f"{what}: |Wa - Wb| {d:.3e} <= {ga:.3e} + {gb:.3e}")
    assert d <= ga + gb, f"{what}: {d:.3e} > {ga:.3e} + {gb:.3e}"
    return d


def stratified_folds(labels, cv):
    """The r-th row, in file order, of each class goes to fold r % cv (written out row by row)."""
    seen, fold = {}, []
    for v in np.asarray(labels).tolist():
        fold.append(seen.get(v, 0) % cv)
        seen[v] = seen.get(v, 0) + 1
    return torch.tensor(fold, dtype=torch.int64)


def accuracy64(W, b, X, labels, classes):
    """-> (predictions right [N] bool, top-two score gap [N], fp32 score bound 2 gamma_{C+2} max_k (|z| |W_k| + |b_k|) [N]),
    scores in float64 from the coefficients as returned."""
    W, b, X = W.double().cpu(), b.double().cpu(), X.double()
    S = X @ W.T + b
    Es = 2.0 * gamma(X.shape[1] + 2) * (X.abs() @ W.abs().T + b.abs()).amax(1)
    cl = torch.from_numpy(np.asarray(classes))
    if len(classes) == 2:
        pred, gap = cl[(S[:, 0] > 0).long()], S[:, 0].abs()
    else:
        top = S.topk(2, dim=1).values
        pred, gap = cl[S.argmax(1)], top[:, 0] - top[:, 1]
    return pred == torch.as_tensor(np.asarray(labels)), gap, Es


def check_cv_scores(cv, X, labels, fold, cap=0.01):
    """``cv_scores_`` against the float64 accuracy from ``fold_coef_``: rows whose top-two gap is below the fp32 score
    bound are left out of the comparison (they may go either way) and may be at most ``cap`` of the held-out rows.
    -> the largest fraction of such rows over all (candidate, fold)."""
    worst = 0.0
    for c in range(len(cv.candidates)):
        for f, fid in enumerate(cv.folds_):
            rows = fold == fid
            right, gap, Es = accuracy64(cv.fold_coef_[c, f], cv.fold_intercept_[c, f], X[rows], labels[rows], cv.classes_)
            unsure = gap < Es
            n = int(rows.sum())
            got = float(cv.cv_scores_[c, f]) * n
            sure = int((right & ~unsure).sum())
            assert int(unsure.sum()) <= cap * n, f"candidate {c} fold {fid}: {int(unsure.sum())} of {n} rows inside the score bound"
            assert sure - 1e-6 <= got <= sure + int(unsure.sum()) + 1e-6, \
                f"candidate {c} fold {fid}: {got} right, float64 says {sure} (+ {int(unsure.sum())} undecided)"
            worst = max(worst, int(unsure.sum()) / n)
    return worst


# ------------------------------------------------------------------ small containers (as tests/test_gpu_probe.py builds its own)
def class_symbols(tab, n, n_classes, seed):
    """Symbols inside every channel's coding window (no escapes: rows of ordinary size) whose mean depends on row % n_classes."""
    rng = np.random.default_rng(seed)
    C = tab["cdf"].shape[0]
    width = (tab["cdf_len"].astype(np.int64) - 2)[None, :]                 # symbols offset .. offset + width - 1
    means = rng.normal(size=(n_classes, C)) * 1.5
    v = np.rint(width / 2 + means[np.arange(n) % n_classes] + rng.normal(size=(n, C)) * 1.5)
    return (tab["offset"][None, :] + np.clip(v, 0, width - 1)).astype(np.int32)
