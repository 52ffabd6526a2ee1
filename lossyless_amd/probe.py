"""The probes: downstream estimators trained and scored where the compressed copy lives.  In file order:

    shared      ``_Rows`` (the walk), ``_check_width`` / ``_z_args`` (what a device pass asks of a group of rows)
    hinge       ``_Problems``, ``_HostSums``, ``_DeviceNewtonSums`` (the base of the three device sums classes), ``_DeviceSums``,
                ``_newton_cg``, ``_affine_scores`` (the one ``lla_gemm_f32`` call site) and ``_Scores``, ``LinearProbe``,
                ``LinearProbeCV``
    softmax     the four softmax sums classes, ``_newton_cg_joint`` / ``_newton_cg_joint_groups``, ``LogisticProbe``,
                ``LogisticProbeCV``
    MLP         the float64 twins, ``_DeviceMLP``, ``MLPProbe``, ``BatchNormMLPProbe`` (optimiser and network primitives: _train.py)
    k-NN, k-means, ridge, zero-shot     ``KNNProbe``; ``KMeansProbe``; ``RidgeProbe`` / ``RidgeProbeCV``; ``ZeroShotProbe``

``LinearProbe`` is the downstream linear classifier, trained from the compressed copy on the device.

The reference's published workflow ends with ``LinearSVC(C=7e-3).fit(Z, Y)`` on the decompressed features (README.md:74-82
of the reference, notebooks/Hub.ipynb:415): scikit-learn's single-threaded liblinear over a host float32 array, which its
README notes does not reach ImageNet.  This class solves the same objective -- squared hinge, L2 penalty, one-vs-rest, the
intercept carried as one more feature of value 1 and regularised with the weights --

    f_k(w, b) = 1/2 (|w|^2 + b^2) + C sum_i max(0, 1 - y_ik (w . z_i + b))^2

for all classes at once, from a :class:`~lossyless_amd.latents.CompressedLatents` / ``HyperpriorLatents`` that stays
compressed in HBM: a pass walks the rows in file order, one decode group at a time (``take`` into one reused buffer), and
hands each group to ``lla_svm_grid_pass`` (csrc/probe.hip), which adds that group's share of the loss, the gradient or a
generalised-Hessian-vector product to the running totals.  No N x K state lives between passes.

The solver is a truncated Newton-CG (Jacobi-preconditioned by the data's column scales), batched over the classes (every class is its own strongly convex problem; all of
them advance in the same pass), with a per-class backtracking line search.  It is deterministic.

CPU data (or latents opened with ``device="cpu"``) run the same solver over a float64 torch evaluation of the same two
quantities: no GPU needed, and the oracle of the GPU tests.

What a pass walks is a set of J *problems* (:class:`_Problems`), not K classes: problem j separates one class from the
rest on the rows outside one held-out fold, with liblinear's class weights (``C w[k]`` for the rows of class k, ``C`` for
the others).  A plain fit is K problems with nothing held out; :class:`LinearProbeCV` lays every (candidate, fold, class)
of a search over ``C`` and ``class_weight`` side by side and solves them in the same passes (``lla_svm_grid_pass``).

:class:`LogisticProbe` is the softmax-regression sibling: one problem that couples all classes (``lla_softmax_pass``, a
joint Newton-CG), over the same walk of the rows and the same scoring path.

:class:`KMeansProbe` is the unsupervised sibling: Lloyd's k-means over the same walk (``lla_kmeans_pass``, csrc/kmeans.hip:
the argmax over the centres in the place of a residual), with the clusters scored against labels afterwards.

:class:`RidgeProbe` / :class:`RidgeProbeCV` are the closed-form siblings: one walk accumulates the rows' second moments
(``lla_gram_pass`` / ``lla_segment_sums``, csrc/gram.hip) and a float64 ``eigh`` gives every alpha and fold from them.
"""
import contextlib
import ctypes
import warnings

import numpy as np
import torch

from . import _lib
from ._train import (_Adam, _adamw, _adamw_step, _dropout_scale, _mlp_backward, _mlp_forward, _mlp_init,  # noqa: F401
                     dropout_keep, lr_schedule, philox4x32_10)
from .latents import _Latents

_CG_TOL = 0.1            # inner solve: |H d + g|_2 <= 0.1 |g|_2 per class (liblinear's TRON uses the same fraction)
_CG_MAX = 100
_ARMIJO = 1e-4
_BACKTRACKS = 30


def _is_latents(data):
    return isinstance(data, _Latents)


class _Rows:
    """The rows of a fit / predict call, walked in file order in groups: ``groups()`` yields (first row, rows [g, C]).
    With ``order`` set (an int64 permutation [N] on the rows' device that keeps every row inside its group), position i of
    the walk is row ``order[i]``: the ridge probes fetch each group sorted by (fold, class)."""

    def __init__(self, data, rows_per_pass, keep_rows):
        self.group = max(int(rows_per_pass), 1)
        self.kept = None
        self.order = None
        self.first_pass = True
        if _is_latents(data):
            self.latents, self.rows = data, None
            self.device, self.n, self.dim = data.device, len(data), int(data.z_dim)
            self.keep = bool(keep_rows)
            self.buf = None
        else:
            t = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data))
            if t.dim() != 2:
                raise ValueError("data must be [N, C]")
            ok = (torch.float32, torch.float16) if t.device.type == "cuda" else (torch.float32, torch.float64)
            if t.dtype not in ok:
                t = t.to(torch.float32)
            if t.device.type == "cuda" and (t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < t.shape[1]
                                            or t.data_ptr() % 16):
                t = t.contiguous()
            self.latents, self.rows = None, t
            self.device, self.n, self.dim = t.device, int(t.shape[0]), int(t.shape[1])
            self.keep = False

    def groups(self):
        first, self.first_pass = self.first_pass, False
        if self.kept is not None:
            yield from self.kept
            return
        kept = [] if self.keep else None
        for g0 in range(0, self.n, self.group):
            g = min(self.group, self.n - g0)
            if self.rows is not None:
                z = self.rows[g0:g0 + g] if self.order is None else self.rows.index_select(0, self.order[g0:g0 + g])
            else:
                idx = torch.arange(g0, g0 + g, device=self.device) if self.order is None else self.order[g0:g0 + g]
                if self.keep:
                    z = self.latents.take(idx, check=first)
                else:
                    if self.buf is None:      # one buffer, reused by every group of every pass
                        self.buf = torch.empty((min(self.group, self.n), self.dim), dtype=torch.float32, device=self.device)
                    z = self.latents.take(idx, out=self.buf[:g], check=first)
            if first and not bool(torch.isfinite(z).all()):
                raise ValueError(f"non-finite values in rows {g0} .. {g0 + g - 1}")
            if kept is not None:
                kept.append((g0, z))
            yield g0, z
        if kept is not None:
            self.kept = kept
            self.latents.release()

    def close(self):
        self.buf = self.kept = None
        if self.latents is not None:
            self.latents.release()


def _check_width(C, who):
    """The feature widths the row-tile kernels (csrc/row_tile.h) are built for; ``who`` names the estimator in the message."""
    if C % 8 or not 8 <= C <= 1024:
        raise ValueError(f"the device {who} needs a feature width that is a multiple of 8 in [8, 1024], got {C}")


def _z_args(z, C):
    """A group's rows z [g, C] (fp32 or fp16, unit column stride) as a device pass takes them: (pointer, ``LLA_Z_*`` code,
    pitch in elements -- C for a single row, whose stride says nothing)."""
    return _lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, int(z.stride(0)) if z.shape[0] > 1 else C


class _Problems:
    """J independent problems that share the rows of a walk.  Problem j: positive class ``cls[j]``, the rows of fold
    ``held[j]`` left out (``_NO_FOLD``: none), weight ``scale[j] * wpos[j]`` on its positive rows and ``scale[j] * wneg[j]``
    on the others; ``group[j]`` says which problems form one classifier (they share a stopping rule).  ``scale`` is the C
    of the objective and is applied to a pass's totals; ``wpos`` / ``wneg`` are the class weights and go into the pass, so
    that without class weights a pass multiplies by 1.0 and adds what ``lla_svm_pass`` adds."""

    def __init__(self, cls, held, wpos, wneg, scale, group):
        self.cls, self.held = torch.as_tensor(cls, dtype=torch.int32), torch.as_tensor(held, dtype=torch.int32)
        self.wpos, self.wneg = torch.as_tensor(wpos, dtype=torch.float64), torch.as_tensor(wneg, dtype=torch.float64)
        self.scale, self.group = torch.as_tensor(scale, dtype=torch.float64), torch.as_tensor(group, dtype=torch.int64)
        self.J = int(self.cls.numel())
        self.n_groups = int(self.group.max()) + 1

    def on(self, sums, device):
        """What the solver reads from a sums object: J, the groups, the totals' scale and the largest weight per problem."""
        sums.J, sums.n_groups = self.J, self.n_groups
        sums.group = self.group.to(device)
        sums.scale = self.scale.to(device)
        sums.cmax = (self.scale * torch.maximum(self.wpos, self.wneg)).to(device)


_NO_FOLD = -2            # a held-out fold id that no row carries (fold ids are >= -1)


def _class_weights(class_weight, classes, counts):
    """liblinear's w[k] for the sorted labels ``classes`` (numpy) with ``counts`` rows each (the rows actually fitted)."""
    K = len(classes)
    if class_weight is None:
        return torch.ones(K, dtype=torch.float64)
    if isinstance(class_weight, str):
        if class_weight != "balanced":
            raise ValueError(f"class_weight must be None, 'balanced' or a dict, got {class_weight!r}")
        return counts.sum().double() / (K * counts.double())
    w = torch.ones(K, dtype=torch.float64)
    for label, value in dict(class_weight).items():
        at = np.nonzero(classes == label)[0]
        if at.size != 1:
            raise ValueError(f"class_weight names the label {label!r}, which the data does not have")
        if not float(value) > 0:
            raise ValueError("class weights must be positive")
        w[int(at[0])] = float(value)
    return w


def _one_classifier(w, Cw, held, group):
    """The problems of one classifier with class weights w [K] -> lists (cls, held, wpos, wneg, scale, group).  Two classes
    are one problem: class index 0 is the positive class ``classes_[1]`` (see ``_class_indexes``) and carries w[1]."""
    K = int(w.numel())
    if K == 2:
        return [0], [held], [float(w[1])], [float(w[0])], [Cw], [group]
    return list(range(K)), [held] * K, w.tolist(), [1.0] * K, [Cw] * K, [group] * K


def _class_indexes(y):
    """labels [N] -> (sorted unique labels, class index per row as the passes want it, problems per classifier)."""
    classes = torch.unique(y)
    if classes.numel() < 2:
        raise ValueError("LinearProbe needs at least two classes")
    idx = torch.searchsorted(classes, y)
    if classes.numel() == 2:                # one classifier; index 0 = the positive class, classes_[1]
        return classes, 1 - idx, 1
    return classes, idx, int(classes.numel())


class _HostSums:
    """float64 torch evaluation of the two quantities ``lla_svm_grid_pass`` computes (the CPU path; the GPU tests' oracle)."""
    dtype = torch.float64
    slack = 1e-14

    def __init__(self, rows, y, prob, fold=None):
        self.rows, self.y, self.prob, self.fold = rows, y, prob, fold
        prob.on(self, rows.device)
        self.n_passes = 0

    def _signs(self, g0, g):
        """-> (y_ij, c_ij / scale_j) for the rows g0 .. g0 + g - 1."""
        p = self.prob
        ys = torch.where(self.y[g0:g0 + g, None] == p.cls[None, :], 1.0, -1.0).to(torch.float64)
        c = torch.where(ys > 0, p.wpos[None, :], p.wneg[None, :])
        if self.fold is not None:
            c = torch.where(self.fold[g0:g0 + g, None] == p.held[None, :], torch.zeros((), dtype=torch.float64), c)
        return ys, c

    def column_squares(self):
        sq = torch.zeros(self.rows.dim, dtype=torch.float64)
        for _, z in self.rows.groups():
            sq += (z.to(torch.float64) ** 2).sum(0)
        self.n_passes += 1
        return sq

    def gradient(self, W, b):
        loss, gW, gb = torch.zeros(self.J, dtype=torch.float64), torch.zeros_like(W), torch.zeros_like(b)
        for g0, z in self.rows.groups():
            z = z.to(torch.float64)
            ys, c = self._signs(g0, z.shape[0])
            m = (1.0 - ys * (z @ W.T + b)).clamp_min(0.0)
            r = -2.0 * ys * m * c
            loss += (m * m * c).sum(0)
            gW += r.T @ z
            gb += r.sum(0)
        self.n_passes += 1
        return self.scale * loss, self.scale[:, None] * gW, self.scale * gb

    def hessian_vector(self, W, b, V, vb):
        hW, hb = torch.zeros_like(W), torch.zeros_like(b)
        for g0, z in self.rows.groups():
            z = z.to(torch.float64)
            ys, c = self._signs(g0, z.shape[0])
            active = (1.0 - ys * (z @ W.T + b)) > 0
            t = 2.0 * torch.where(active, z @ V.T + vb, torch.zeros((), dtype=torch.float64)) * c
            hW += t.T @ z
            hb += t.sum(0)
        self.n_passes += 1
        return self.scale[:, None] * hW, self.scale * hb


class _DeviceNewtonSums:
    """The device side of a sums object of the Newton-CG solvers: the width check, the workspace, the walk of the decode
    groups under the device guard and the count of passes.  A subclass sets up its constant arguments, calls
    ``_workspace``, and gives ``_pass(W, b, V, vb, st)`` -> (loss or None, dW, db): zero-initialised accumulators, one
    library call (``accumulate=1``) per group of ``_groups()``, the scaling afterwards."""
    dtype = torch.float32
    slack = 1e-6          # Armijo slack, relative to f: the fp32 loss sums of two passes differ by rounding at this level

    def __init__(self, rows):
        _check_width(rows.dim, "probe")
        self.rows, self.dim, self.device = rows, rows.dim, rows.device
        self.L = _lib.lib()
        self.n_passes = 0

    def _workspace(self, nbytes, refused):
        """The pass's workspace; a size of 0 is the library refusing the shape (``refused``: the message)."""
        if int(nbytes) == 0:
            raise ValueError(refused)
        self.ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)

    def _groups(self):
        """-> (first row, n, then the rows [n, C] as ``_z_args`` gives them) of every decode group."""
        for g0, z in self.rows.groups():
            yield (g0, int(z.shape[0])) + _z_args(z, self.dim)

    def _run(self, W, b, V, vb):
        with torch.cuda.device(self.device):
            out = self._pass(W, b, V, vb, _lib.stream_ptr(self.device))
        self.n_passes += 1
        return out

    def column_squares(self):
        sq = torch.zeros(self.dim, dtype=torch.float64, device=self.device)
        for _, z in self.rows.groups():
            sq += (z.float() ** 2).sum(0, dtype=torch.float64)
        self.n_passes += 1
        return sq

    def gradient(self, W, b):
        return self._run(W.contiguous(), b.contiguous(), None, None)

    def hessian_vector(self, W, b, V, vb):
        return self._run(W.contiguous(), b.contiguous(), V.contiguous(), vb.contiguous())[1:]


class _DeviceSums(_DeviceNewtonSums):
    """The same two quantities from ``lla_svm_grid_pass``, one call per decode group, accumulated on the device."""

    def __init__(self, rows, y, prob, fold=None):
        super().__init__(rows)
        dev = self.device
        prob.on(self, dev)
        self.y = y.to(torch.int32).to(dev).contiguous()
        self.fold = None if fold is None else fold.to(torch.int32).to(dev).contiguous()
        self.cols = [prob.cls.to(dev), prob.held.to(dev), prob.wpos.to(torch.float32).to(dev),
                     prob.wneg.to(torch.float32).to(dev)]
        self.scale32 = self.scale.to(torch.float32)
        self._workspace(self.L.lla_svm_grid_pass_workspace_bytes(self.dim, self.J),
                        f"lla_svm_grid_pass refuses C = {self.dim}, J = {self.J}")

    def _pass(self, W, b, V, vb, st):
        J, C = self.J, self.dim
        oW = torch.zeros((J, C), dtype=torch.float32, device=self.device)
        ob = torch.zeros(J, dtype=torch.float32, device=self.device)
        loss = torch.zeros(J, dtype=torch.float64, device=self.device) if V is None else None
        cols = [_lib.ptr(t) for t in self.cols]
        for g0, g, zp, zt, ld in self._groups():
            fold = None if self.fold is None else self.fold[g0:g0 + g]
            rc = self.L.lla_svm_grid_pass(zp, zt, ld, _lib.ptr(self.y[g0:g0 + g]),
                                          _lib.ptr(fold), g, C, _lib.ptr(W), _lib.ptr(b), _lib.ptr(V), _lib.ptr(vb), J, C,
                                          *cols, _lib.ptr(oW), _lib.ptr(ob), _lib.ptr(loss), 1, _lib.ptr(self.ws), st)
            _lib.check(rc, "lla_svm_grid_pass")
        return (None if loss is None else self.scale * loss), self.scale32[:, None] * oW, self.scale32 * ob


def _newton_cg(sums, dim, n_rows, device, tol, max_iter):
    """Batched truncated Newton-CG on the J problems of ``sums``, f_j = 1/2 (|w|^2 + b^2) + (weighted loss)_j
    -> (W, b, f [J] float64, converged [groups] bool).  A problem stops once its gradient's sup norm is within ``tol`` of
    the largest gradient at 0 among the problems of its group (one classifier).  One host synchronisation per CG
    iteration and per line-search step."""
    dt, J = sums.dtype, sums.J
    W, b = torch.zeros((J, dim), dtype=dt, device=device), torch.zeros(J, dtype=dt, device=device)

    def evaluate(W, b):
        loss, gW, gb = sums.gradient(W, b)
        f = 0.5 * ((W.double() ** 2).sum(1) + b.double() ** 2) + loss
        return f, W + gW, b + gb

    def sup(gW, gb):          # per-problem sup norm of the gradient
        return torch.maximum(gW.abs().amax(1), gb.abs())

    # Jacobi preconditioner from the column scales of the data: 1 + 2 c_j sum_i z_ic^2, c_j the larger of the problem's
    # two weights and the sum over ALL rows, bounds the Hessian's diagonal for every problem, every active set and every
    # held-out fold (the intercept's column is all ones), so one vector of column scales serves the whole solve
    mW = (1.0 + (2.0 * sums.cmax)[:, None] * sums.column_squares()[None, :]).to(dt)
    mb = (1.0 + 2.0 * sums.cmax * n_rows).to(dt)
    f, gW, gb = evaluate(W, b)
    g0 = torch.zeros(sums.n_groups, dtype=dt, device=device).scatter_reduce(0, sums.group, sup(gW, gb), "amax")
    stop_at = (tol * g0.double())[sums.group].to(dt)
    for _ in range(int(max_iter)):
        live = sup(gW, gb) > stop_at     # problems still short of the stopping rule; the others stay where they are
        if not bool(live.any()):
            break
        lv = live.to(dt)
        # preconditioned CG on H d = -g, H v = v + (weighted generalised Hessian sums)(v), all problems in one pass
        dW, db = torch.zeros_like(W), torch.zeros_like(b)
        rW, rb = -gW * lv[:, None], -gb * lv
        yW, yb = rW / mW, rb / mb
        pW, pb = yW.clone(), yb.clone()
        rs = (rW * yW).sum(1) + rb * yb
        stop = _CG_TOL ** 2 * rs
        for _cg in range(_CG_MAX):
            hW, hb = sums.hessian_vector(W, b, pW, pb)
            hW, hb = pW + hW, pb + hb
            busy = (rs > stop).to(dt)
            alpha = busy * rs / ((pW * hW).sum(1) + pb * hb).clamp_min(torch.finfo(dt).tiny)
            dW += alpha[:, None] * pW
            db += alpha * pb
            rW -= alpha[:, None] * hW
            rb -= alpha * hb
            yW, yb = rW / mW, rb / mb
            rs2 = (rW * yW).sum(1) + rb * yb
            if bool((rs2 <= stop).all()):
                break
            beta = busy * rs2 / rs.clamp_min(torch.finfo(dt).tiny)
            pW, pb = yW + beta[:, None] * pW, yb + beta * pb
            rs = torch.where(busy > 0, rs2, rs)
        # per-problem backtracking: a problem keeps its step length once the Armijo condition holds for it
        gd = ((gW * dW).sum(1) + gb * db).double()
        t = torch.ones(J, dtype=dt, device=device)
        for _ls in range(_BACKTRACKS):
            W2, b2 = W + t[:, None] * dW, b + t * db
            f2, gW2, gb2 = evaluate(W2, b2)
            ok = f2 <= f + _ARMIJO * t.double() * gd + sums.slack * f.abs()
            if bool(ok.all()):
                break
            t = torch.where(ok, t, t * 0.5)
        else:                            # problems whose step never passed stay where they were
            t = torch.where(ok, t, torch.zeros_like(t))
            W2, b2 = W + t[:, None] * dW, b + t * db
            f2, gW2, gb2 = evaluate(W2, b2)
        W, b, f, gW, gb = W2, b2, f2, gW2, gb2
        if not bool((t > 0).any()):      # nothing moved: rounding has the last word
            break
    short = torch.zeros(sums.n_groups, dtype=dt, device=device).index_add_(0, sums.group, (sup(gW, gb) > stop_at).to(dt))
    return W, b, f, (short == 0).cpu()


def _labels_of(data, labels, n):
    if labels is None:
        if not _is_latents(data) or data._labels is None:
            raise ValueError("no labels: pass labels=, or open the latents with a label_file")
        labels = data._labels
    y = labels.detach().cpu() if isinstance(labels, torch.Tensor) else torch.from_numpy(np.asarray(labels))
    y = y.reshape(-1)
    if y.is_floating_point() or y.dtype == torch.bool:
        raise TypeError("labels must be integers")
    if y.numel() != n:
        raise ValueError(f"{y.numel()} labels for {n} rows")
    return y.to(torch.int64)


_SCORE_ELEMS = 1 << 25    # fp32 scores a scoring walk of a search holds at a time: larger groups are scored in pieces


def _f32_rows(z, C):
    """fp32 rows as the GEMMs want them: unit column stride, a pitch that is a multiple of 4, 16-byte aligned -> (z, pitch)."""
    if z.dtype != torch.float32:
        z = z.float()
    if z.stride(1) != 1 or (z.shape[0] > 1 and (z.stride(0) % 4 or z.stride(0) < C)) or z.data_ptr() % 16:
        z = z.contiguous()
    return z, (int(z.stride(0)) if z.shape[0] > 1 else C)


def _gemm_f32(x, ld, W, b, out, ldo, n, o, i, relu, st):
    """out [n, o] of pitch ldo = x [n, i] of pitch ld times W^T [o, i], plus b (None: no bias), through ReLU if ``relu``."""
    rc = _lib.lib().lla_gemm_f32(_lib.ptr(x), ld, _lib.ptr(W), i, _lib.ptr(b), _lib.ptr(out), ldo, n, o, i, relu, st)
    _lib.check(rc, "lla_gemm_f32")


def _pack_affine(W, b, dev):
    """Padded device copies of [K, C] weights and [K] biases for ``_affine_scores`` (as ``MLP._pack``) -> (fp32 [Npad8, C],
    fp32 [Npad8], Npad8): zero rows up to the next multiple of 8.  Leading dimensions (one set of weights per fold) stay."""
    K, C = W.shape[-2:]
    if C % 8:
        raise ValueError("the device path needs a feature width that is a multiple of 8")
    npad = -(-K // 8) * 8
    w = torch.zeros(W.shape[:-2] + (npad, C), dtype=torch.float32, device=dev)
    w[..., :K, :] = W.to(dev)
    bp = torch.zeros(b.shape[:-1] + (npad,), dtype=torch.float32, device=dev)
    bp[..., :K] = b.to(dev)
    return w, bp, npad


def _piece_rows(npad, group):
    """Rows of a decode group of ``group`` rows scored at a time against ``npad`` columns (``_SCORE_ELEMS``)."""
    return max(min(_SCORE_ELEMS // npad, group), 1)


def _affine_scores(z, w, b, out, piece=None, each=None):
    """The scores of a group's rows z [g, C] against packed weights (``_pack_affine``), on the current device and stream.
    Without ``piece``: one launch into out [g, Npad8].  With it: ``piece`` rows at a time into the reused out[:n], and
    ``each(first row of the piece, out[:n])`` after every launch.  -> the rows as they were scored (``_f32_rows``)."""
    npad, C = w.shape
    z, ld = _f32_rows(z, C)
    g, st = int(z.shape[0]), _lib.stream_ptr(z.device)
    piece = piece or max(g, 1)
    for r0 in range(0, g, piece):
        n = min(piece, g - r0)
        _gemm_f32(z[r0:r0 + n], ld if n > 1 else C, w, b, out, npad, n, npad, C, 0, st)
        if each is not None:
            each(r0, out[:n])
    return z


class _Scores:
    """Scoring shared by the probes: ``coef_`` [K, C] and ``intercept_`` [K] against the rows of a fit / predict call."""

    coef_ = intercept_ = classes_ = None

    @staticmethod
    def _rows_in(z):
        """What is scored in the place of a group's rows (ZeroShotProbe: the rows over their norms)."""
        return z

    def _set(self, W, b, classes, n_passes, objective, converged):
        self.coef_, self.intercept_ = W.to(torch.float32), b.to(torch.float32)
        self.classes_ = classes.numpy()
        self.n_passes_, self.objective_, self.converged_ = n_passes, objective, converged
        self._packed = None

    def _pack(self, dev):
        """``_pack_affine`` of the fitted weights, kept per device."""
        if self._packed is None or self._packed[0] != str(dev):
            self._packed = (str(dev),) + _pack_affine(self.coef_, self.intercept_, dev)
        return self._packed[1:]

    def _scores(self, data, rows_per_pass):
        """-> [N, K]: fp32 from ``lla_gemm_f32`` on the device, float64 on the CPU."""
        if self.coef_ is None:
            raise RuntimeError("fit first")
        rows = _Rows(data, rows_per_pass, False)
        rows.first_pass = _is_latents(data)       # (statuses of a decode are checked; tensors are taken as they are)
        K, C = self.coef_.shape
        if rows.dim != C:
            raise ValueError(f"data has {rows.dim} features, the probe was fitted on {C}")
        try:
            if rows.device.type == "cuda":
                w, b, npad = self._pack(rows.device)
                out = torch.empty((rows.n, npad), dtype=torch.float32, device=rows.device)
                with torch.cuda.device(rows.device):
                    for g0, z in rows.groups():
                        _affine_scores(self._rows_in(z), w, b, out[g0:g0 + int(z.shape[0])])
                s = out[:, :K]
            else:
                W, b = self.coef_.to(torch.float64).cpu(), self.intercept_.to(torch.float64).cpu()
                s = torch.cat([self._rows_in(z.to(torch.float64)) @ W.T + b for _, z in rows.groups()]) if rows.n else \
                    torch.zeros((0, K), dtype=torch.float64)
        finally:
            rows.close()
        return s

    def predict(self, data, rows_per_pass=65536):
        s = self.decision_function(data, rows_per_pass)
        which = (s > 0).to(torch.int64) if s.dim() == 1 else s.argmax(1)
        return torch.from_numpy(self.classes_).to(s.device)[which]

    def score(self, data, labels=None, rows_per_pass=65536):
        pred = self.predict(data, rows_per_pass)
        y = _labels_of(data, labels, pred.numel()).to(pred.device)
        return float((pred == y).double().mean())


class LinearProbe(_Scores):
    """``LinearProbe(C=7e-3, tol=1e-4, max_iter=100, class_weight=None)``: scikit-learn's ``LinearSVC(C)`` objective (its
    defaults: squared hinge, L2, one-vs-rest, regularised intercept), solved where the data lives.  ``class_weight`` is
    ``LinearSVC``'s: ``None``, ``"balanced"`` (``n / (K count_k)``) or a ``{label: weight}`` dict (labels left out weigh 1);
    the classifier of class k weighs the rows of class k by ``C w[k]`` and all other rows by ``C``, as liblinear does.

    ``fit(data, labels=None, rows_per_pass=65536, keep_rows=False)``
        data    a ``CompressedLatents`` / ``HyperpriorLatents`` (its own labels unless ``labels`` is given), or a
                ``[N, C]`` tensor / array together with ``labels``.
        rows_per_pass   rows decoded (``take``) and handed to ``lla_svm_grid_pass`` at a time; statuses are checked on the
                first pass only.
        keep_rows       decode once and keep the fp32 rows (N x C x 4 bytes) instead of decoding every pass.
    Stops when ``|grad f|_inf <= tol |grad f(0)|_inf``; warns and sets ``converged_ = False`` at ``max_iter`` Newton steps.

    After ``fit``: ``coef_`` fp32 ``[K, C]`` (``[1, C]`` for two classes, positive class ``classes_[1]``), ``intercept_``,
    ``classes_`` (sorted unique labels, numpy), ``n_passes_`` (passes over the data), ``objective_`` (sum of f_k),
    ``converged_``.  ``decision_function`` returns ``[N, K]`` (``[N]`` for two classes), fp32 from ``lla_gemm_f32`` on the
    device and float64 on the CPU; ``predict`` returns labels, ``score`` the mean accuracy."""

    def __init__(self, C=7e-3, tol=1e-4, max_iter=100, class_weight=None):
        if not C > 0 or not tol > 0 or int(max_iter) < 1:
            raise ValueError("C and tol must be positive, max_iter at least 1")
        if not (class_weight is None or class_weight == "balanced" or isinstance(class_weight, dict)):
            raise ValueError(f"class_weight must be None, 'balanced' or a dict, got {class_weight!r}")
        self.C, self.tol, self.max_iter, self.class_weight = float(C), float(tol), int(max_iter), class_weight
        self.coef_ = self.intercept_ = self.classes_ = None

    # ------------------------------------------------------------------ labels
    _labels_of = staticmethod(_labels_of)

    # ------------------------------------------------------------------ fit
    def fit(self, data, labels=None, rows_per_pass=65536, keep_rows=False):
        rows = _Rows(data, rows_per_pass, keep_rows)
        y = self._labels_of(data, labels, rows.n)
        classes, idx, _ = _class_indexes(y)
        counts = torch.bincount(torch.searchsorted(classes, y), minlength=int(classes.numel()))
        prob = _Problems(*_one_classifier(_class_weights(self.class_weight, classes.numpy(), counts), self.C, _NO_FOLD, 0))
        try:
            sums = (_DeviceSums if rows.device.type == "cuda" else _HostSums)(rows, idx, prob)
            W, b, f, converged = _newton_cg(sums, rows.dim, rows.n, rows.device, self.tol, self.max_iter)
        finally:
            rows.close()
        self._set(W, b, classes, sums.n_passes, float(f.sum()), bool(converged.all()))
        if not self.converged_:
            warnings.warn(f"LinearProbe stopped short of tol = {self.tol} after {self.max_iter} Newton steps", RuntimeWarning)
        return self

    # ------------------------------------------------------------------ predict
    def decision_function(self, data, rows_per_pass=65536):
        s = self._scores(data, rows_per_pass)
        return s[:, 0].contiguous() if len(self.classes_) == 2 else s.contiguous()


def _folds_of(cv_arg, cls_idx, n_classes):
    """-> (fold id per row int64 [N], sorted fold ids, class counts of each fold's training part); raises if a training part lacks a class or a fold is empty."""
    N = int(cls_idx.numel())
    if isinstance(cv_arg, (int, np.integer)):
        cv = int(cv_arg)
        if cv < 2:
            raise ValueError("cv must be at least 2")
        order = torch.argsort(cls_idx, stable=True)                         # file order within each class
        counts = torch.bincount(cls_idx, minlength=n_classes)
        rank = torch.arange(N) - (torch.cumsum(counts, 0) - counts)[cls_idx[order]]
        fold = torch.empty(N, dtype=torch.int64)
        fold[order] = rank % cv
        ids = list(range(cv))
    else:
        fold = torch.as_tensor(np.asarray(cv_arg.cpu() if isinstance(cv_arg, torch.Tensor) else cv_arg))
        if fold.is_floating_point() or fold.dtype == torch.bool or fold.dim() != 1 or fold.numel() != N:
            raise ValueError(f"cv must be an int or an int array of {N} fold ids")
        fold = fold.to(torch.int64)
        if int(fold.min()) < -1 or int(fold.max()) >= 2 ** 31 - 1:
            raise ValueError("fold ids must be >= -1 (-1: always train)")
        ids = [int(v) for v in torch.unique(fold) if int(v) >= 0]
        if not ids:
            raise ValueError("no row is ever held out")
    train_counts = []
    for f in ids:
        if not bool((fold == f).any()):
            raise ValueError(f"fold {f} holds no row")
        c = torch.bincount(cls_idx[fold != f], minlength=n_classes)
        if bool((c == 0).any()):
            raise ValueError(f"the training part of fold {f} lacks a class")
        train_counts.append(c)
    return fold, ids, train_counts


class LinearProbeCV:
    """``LinearProbeCV(candidates, cv=5, tol=1e-4, max_iter=100, refit=True, max_problems=4096)``: the search the reference
    evaluates a compressor with (its utils/Z_linear_eval.py:62-93: ``RandomizedSearchCV`` over ``C`` and ``class_weight``,
    scored by accuracy, the winner refitted), with every (candidate, fold, class) solved in the same passes over the data.

    candidates  a sequence of ``(C, class_weight)``; ``LinearProbeCV.sample(n, seed)`` draws the reference's distribution.
    cv          an int: stratified and unshuffled -- the r-th row, in file order, of each class goes to fold ``r % cv``;
                or an int array ``[N]`` of fold ids, -1 for a row that always trains and never validates (scikit-learn's
                ``PredefinedSplit``).  ``"balanced"`` weights are counted on the training part of each fold.
    refit       also fit every candidate on all rows, in the same passes: ``best_estimator_`` costs no second solve.
    max_problems  problems (classifiers x classes) solved side by side; more are solved in batches of whole classifiers.

    ``fit(data, labels=None, rows_per_pass=65536, keep_rows=False)`` takes what ``LinearProbe.fit`` takes.  Afterwards:
    ``cv_scores_`` float64 ``[candidates, folds]`` (accuracy on the held-out rows), ``mean_scores_``, ``best_index_`` (the
    first maximum, as scikit-learn ranks), ``best_params_``, ``fold_coef_`` / ``fold_intercept_`` fp32
    ``[candidates, folds, K or 1, C]``, ``best_estimator_`` (a fitted ``LinearProbe``; ``None`` without ``refit``),
    ``classes_``, ``folds_`` (the fold ids), ``n_passes_``, ``converged_`` bool ``[candidates, folds (+ 1 with refit)]``."""

    def __init__(self, candidates, cv=5, tol=1e-4, max_iter=100, refit=True, max_problems=4096):
        self.candidates = [(float(C), cw) for C, cw in candidates]
        if not self.candidates:
            raise ValueError("no candidates")
        for C, cw in self.candidates:
            LinearProbe(C=C, tol=tol, max_iter=max_iter, class_weight=cw)        # (its checks)
        if int(max_problems) < 1:
            raise ValueError("max_problems must be at least 1")
        self.cv, self.tol, self.max_iter = cv, float(tol), int(max_iter)
        self.refit, self.max_problems = bool(refit), int(max_problems)
        self.cv_scores_ = self.best_estimator_ = None

    @staticmethod
    def sample(n, seed, low=1e-3, high=1.0):
        """n candidates as the reference draws them: C log-uniform in [low, high], class_weight a coin between
        ``"balanced"`` and ``None``."""
        if not 0 < low <= high:
            raise ValueError("need 0 < low <= high")
        rng = np.random.default_rng(seed)
        Cs = np.exp(rng.uniform(np.log(low), np.log(high), size=int(n))).clip(low, high)
        coins = rng.integers(0, 2, size=int(n))
        return [(float(C), "balanced" if coin else None) for C, coin in zip(Cs, coins)]

    # ------------------------------------------------------------------ folds
    def _folds_of(self, cls_idx, n_classes):
        return _folds_of(self.cv, cls_idx, n_classes)

    # ------------------------------------------------------------------ fit
    def fit(self, data, labels=None, rows_per_pass=65536, keep_rows=False):
        rows = _Rows(data, rows_per_pass, keep_rows)
        y = _labels_of(data, labels, rows.n)
        classes, idx, Kp = _class_indexes(y)
        sorted_idx = torch.searchsorted(classes, y)
        n_classes = int(classes.numel())
        fold, ids, train_counts = self._folds_of(sorted_idx, n_classes)
        all_counts = torch.bincount(sorted_idx, minlength=n_classes)
        nc, nf = len(self.candidates), len(ids)
        per = nf + int(self.refit)
        # one classifier (group) per (candidate, fold), then per candidate one with nothing held out
        layout = [(c, f) for c in range(nc) for f in range(per)]
        step = max(self.max_problems // Kp, 1)
        device = rows.device
        Sums = _DeviceSums if device.type == "cuda" else _HostSums
        coef = torch.empty((nc, per, Kp, rows.dim), dtype=torch.float32, device=device)
        icpt = torch.empty((nc, per, Kp), dtype=torch.float32, device=device)
        objective = torch.empty((nc, per), dtype=torch.float64)
        converged = torch.empty((nc, per), dtype=torch.bool)
        self.n_passes_ = 0
        try:
            for at in range(0, len(layout), step):
                batch, cols = layout[at:at + step], [[] for _ in range(6)]
                for g, (c, f) in enumerate(batch):
                    Cw, cw = self.candidates[c]
                    w = _class_weights(cw, classes.numpy(), train_counts[f] if f < nf else all_counts)
                    for dst, src in zip(cols, _one_classifier(w, Cw, ids[f] if f < nf else _NO_FOLD, g)):
                        dst += src
                sums = Sums(rows, idx, _Problems(*cols), fold)
                W, b, fv, conv = _newton_cg(sums, rows.dim, rows.n, device, self.tol, self.max_iter)
                self.n_passes_ += sums.n_passes
                for g, (c, f) in enumerate(batch):
                    coef[c, f], icpt[c, f] = W[g * Kp:(g + 1) * Kp], b[g * Kp:(g + 1) * Kp]
                    objective[c, f], converged[c, f] = float(fv[g * Kp:(g + 1) * Kp].sum()), bool(conv[g])
            held = torch.tensor(ids, dtype=torch.int64).repeat(nc)
            right = self._score(rows, coef[:, :nf].reshape(nc * nf * Kp, rows.dim), icpt[:, :nf].reshape(-1), idx, fold, held, Kp)
            self.n_passes_ += 1
        finally:
            rows.close()
        n_held = torch.stack([(fold == f).sum() for f in ids]).double()
        self.cv_scores_ = right.reshape(nc, nf).double() / n_held[None, :]
        self.mean_scores_ = self.cv_scores_.mean(1)
        self.best_index_ = int(self.mean_scores_.argmax())                       # the first maximum
        self.best_params_ = dict(zip(("C", "class_weight"), self.candidates[self.best_index_]))
        self.fold_coef_, self.fold_intercept_ = coef[:, :nf].contiguous(), icpt[:, :nf].contiguous()
        self.classes_, self.folds_, self.converged_ = classes.numpy(), list(ids), converged
        self.best_estimator_ = None
        if self.refit:
            best = LinearProbe(C=self.best_params_["C"], tol=self.tol, max_iter=self.max_iter,
                               class_weight=self.best_params_["class_weight"])
            best._set(coef[self.best_index_, nf].clone(), icpt[self.best_index_, nf].clone(), classes, self.n_passes_,
                      float(objective[self.best_index_, nf]), bool(converged[self.best_index_, nf]))
            self.best_estimator_ = best
        if not bool(converged.all()):
            warnings.warn(f"LinearProbeCV: {int((~converged).sum())} of {converged.numel()} classifiers stopped short of "
                          f"tol = {self.tol} after {self.max_iter} Newton steps", RuntimeWarning)
        return self

    @staticmethod
    def _score(rows, W, b, idx, fold, held, Kp):
        """One walk: the scores of all problems (``lla_gemm_f32`` on the device, float64 on the CPU), the argmax within
        each classifier, and per classifier the number of rows of its held-out fold it gets right -> int64 [classifiers]
        on the CPU.  Reduced per decode group (in slices of it where [rows, problems] would be large)."""
        dev, (J, C) = rows.device, W.shape
        G = J // Kp
        idx, fold, held = idx.to(dev), fold.to(dev), held.to(dev)
        right = torch.zeros(G, dtype=torch.int64, device=dev)

        def count(S, r0):
            S = S.reshape(S.shape[0], G, Kp)
            pred = torch.where(S[:, :, 0] > 0, 0, 1) if Kp == 1 else S.argmax(2)
            n = S.shape[0]
            hit = (pred == idx[r0:r0 + n, None]) & (fold[r0:r0 + n, None] == held[None, :])
            right.add_(hit.sum(0))

        if dev.type == "cuda":
            w, bp, npad = _pack_affine(W, b, dev)
            piece = _piece_rows(npad, rows.group)
            out = torch.empty((min(piece, max(rows.n, 1)), npad), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                for g0, z in rows.groups():
                    _affine_scores(z, w, bp, out, piece, lambda r0, S: count(S[:, :J], g0 + r0))
        else:
            W64, b64 = W.to(torch.float64), b.to(torch.float64)
            for g0, z in rows.groups():
                count(z.to(torch.float64) @ W64.T + b64, g0)
        return right.cpu()


# ---------------------------------------------------------------------- softmax regression
_HOST_BLOCK = 4096       # rows per evaluation of the float64 twin, whatever rows_per_pass is


class _HostSoftmaxSums:
    """float64 torch evaluation of the two quantities ``lla_softmax_pass`` computes, times C (the CPU path; the GPU tests'
    oracle).  The rows are evaluated in blocks of ``_HOST_BLOCK`` cut from the walk's groups, so the bits do not depend
    on ``rows_per_pass``."""
    dtype = torch.float64
    slack = 1e-14

    def __init__(self, rows, idx, cw, C):
        self.rows, self.idx, self.cw, self.C = rows, idx, cw.to(torch.float64), float(C)
        self.K = int(cw.numel())
        self.cmax = self.C * float(cw.max())
        self.n_passes = 0

    def _blocks(self):
        """-> (first row, float64 rows [<= _HOST_BLOCK, C]) in file order, the same cuts for every grouping of the walk."""
        held, n_held, at = [], 0, 0
        for _, z in self.rows.groups():
            held.append(z.to(torch.float64))
            n_held += z.shape[0]
            while n_held >= _HOST_BLOCK:
                z = torch.cat(held) if len(held) > 1 else held[0]
                yield at, z[:_HOST_BLOCK]
                at, n_held = at + _HOST_BLOCK, n_held - _HOST_BLOCK
                held = [z[_HOST_BLOCK:]] if n_held else []
        if n_held:
            yield at, (torch.cat(held) if len(held) > 1 else held[0])

    def _rows_of(self, g0, z, W, b):
        """-> (scores, lse [g, 1], p, w_i [g, 1], one-hot labels) of the block."""
        y = self.idx[g0:g0 + z.shape[0]]
        s = z @ W.T + b
        lse = torch.logsumexp(s, 1, keepdim=True)
        hot = torch.zeros_like(s).scatter_(1, y[:, None], 1.0)
        return s, lse, torch.exp(s - lse), self.cw[y][:, None], hot

    def column_squares(self):
        sq = torch.zeros(self.rows.dim, dtype=torch.float64)
        for _, z in self._blocks():
            sq += (z ** 2).sum(0)
        self.n_passes += 1
        return sq

    def gradient(self, W, b):
        loss, gW, gb = torch.zeros((), dtype=torch.float64), torch.zeros_like(W), torch.zeros_like(b)
        for g0, z in self._blocks():
            s, lse, p, w, hot = self._rows_of(g0, z, W, b)
            r = w * (p - hot)
            loss += (w * (lse - (s * hot).sum(1, keepdim=True))).sum()
            gW += r.T @ z
            gb += r.sum(0)
        self.n_passes += 1
        return self.C * loss, self.C * gW, self.C * gb

    def hessian_vector(self, W, b, V, vb):
        hW, hb = torch.zeros_like(W), torch.zeros_like(b)
        for g0, z in self._blocks():
            _, _, p, w, _ = self._rows_of(g0, z, W, b)
            t = z @ V.T + vb
            r = w * p * (t - (p * t).sum(1, keepdim=True))
            hW += r.T @ z
            hb += r.sum(0)
        self.n_passes += 1
        return self.C * hW, self.C * hb


class _DeviceSoftmaxSums(_DeviceNewtonSums):
    """The same two quantities from ``lla_softmax_pass``, one call per decode group, accumulated on the device."""

    def __init__(self, rows, idx, cw, C):
        super().__init__(rows)
        dev = self.device
        self.C = float(C)
        self.K = int(cw.numel())
        self.cmax = self.C * float(cw.max())
        self.y = idx.to(torch.int32).to(dev).contiguous()
        self.cw = None if bool((cw == 1).all()) else cw.to(torch.float32).to(dev)
        self._workspace(self.L.lla_softmax_pass_workspace_bytes(self.dim, self.K, min(rows.group, max(rows.n, 1))),
                        f"lla_softmax_pass refuses C = {self.dim}, K = {self.K}")

    def _pass(self, W, b, V, vb, st):
        K, C = self.K, self.dim
        oW = torch.zeros((K, C), dtype=torch.float32, device=self.device)
        ob = torch.zeros(K, dtype=torch.float32, device=self.device)
        loss = torch.zeros(K, dtype=torch.float64, device=self.device) if V is None else None
        for g0, g, zp, zt, ld in self._groups():
            rc = self.L.lla_softmax_pass(zp, zt, ld, _lib.ptr(self.y[g0:g0 + g]), g, C,
                                         _lib.ptr(W), _lib.ptr(b), _lib.ptr(V), _lib.ptr(vb), K, C, _lib.ptr(self.cw),
                                         _lib.ptr(oW), _lib.ptr(ob), _lib.ptr(loss), 1, _lib.ptr(self.ws), st)
            _lib.check(rc, "lla_softmax_pass")
        return (None if loss is None else self.C * loss.sum()), self.C * oW, self.C * ob


def _newton_cg_joint(sums, dim, n_rows, device, tol, max_iter):
    """Truncated Newton-CG on ONE problem over the whole [K, C + 1] array -- the softmax couples the classes, so every
    inner product, step length and stopping rule is taken over all of them: f = 1/2 (|W|^2 + |b|^2) + C (weighted
    cross-entropy) -> (W, b, f float64, converged bool).  Stops once the gradient's sup norm is within ``tol`` of the one
    at 0.  One host synchronisation per CG iteration and per line-search step."""
    dt, K = sums.dtype, sums.K
    W, b = torch.zeros((K, dim), dtype=dt, device=device), torch.zeros(K, dtype=dt, device=device)

    def evaluate(W, b):
        loss, gW, gb = sums.gradient(W, b)
        return 0.5 * ((W.double() ** 2).sum() + (b.double() ** 2).sum()) + loss, W + gW, b + gb

    def dot(aW, ab, cW, cb):
        return (aW * cW).sum() + (ab * cb).sum()

    def sup(gW, gb):
        return float(torch.maximum(gW.abs().max(), gb.abs().max()))

    # Jacobi preconditioner: the Hessian's diagonal is 1 + C sum_i w_i p_ik (1 - p_ik) z_ic^2 and p (1 - p) <= 1/4, so
    # 1 + C / 4 max(w) sum_i z_ic^2 bounds it for every class and every iterate (the intercept's column is all ones)
    mW = (1.0 + 0.25 * sums.cmax * sums.column_squares()[None, :]).to(dt)
    mb = torch.full((K,), 1.0 + 0.25 * sums.cmax * n_rows, dtype=dt, device=device)
    f, gW, gb = evaluate(W, b)
    stop_at = tol * sup(gW, gb)
    for _ in range(int(max_iter)):
        if sup(gW, gb) <= stop_at:
            break
        # preconditioned CG on H d = -g, H v = v + C (Hessian-vector pass)(v), until |H d + g|_2 <= 0.1 |g|_2
        dW, db = torch.zeros_like(W), torch.zeros_like(b)
        rW, rb = -gW, -gb
        yW, yb = rW / mW, rb / mb
        pW, pb = yW.clone(), yb.clone()
        rs = dot(rW, rb, yW, yb)
        stop = _CG_TOL ** 2 * float(dot(rW, rb, rW, rb))
        for _cg in range(_CG_MAX):
            hW, hb = sums.hessian_vector(W, b, pW, pb)
            hW, hb = pW + hW, pb + hb
            alpha = rs / dot(pW, pb, hW, hb).clamp_min(torch.finfo(dt).tiny)
            dW += alpha * pW
            db += alpha * pb
            rW -= alpha * hW
            rb -= alpha * hb
            if float(dot(rW, rb, rW, rb)) <= stop:
                break
            yW, yb = rW / mW, rb / mb
            rs2 = dot(rW, rb, yW, yb)
            beta = rs2 / rs.clamp_min(torch.finfo(dt).tiny)
            pW, pb = yW + beta * pW, yb + beta * pb
            rs = rs2
        # backtracking until the Armijo condition holds (fp32 sums: with the slack of the per-class solver)
        gd = float(dot(gW, gb, dW, db))
        t = 1.0
        for _ls in range(_BACKTRACKS):
            W2, b2 = W + t * dW, b + t * db
            f2, gW2, gb2 = evaluate(W2, b2)
            if float(f2) <= float(f) + _ARMIJO * t * gd + sums.slack * abs(float(f)):
                break
            t *= 0.5
        else:                            # no step passed: rounding has the last word
            break
        W, b, f, gW, gb = W2, b2, f2, gW2, gb2
    return W, b, f, sup(gW, gb) <= stop_at


class LogisticProbe(_Scores):
    """``LogisticProbe(C=1.0, tol=1e-4, max_iter=100, class_weight=None)``: L2-regularised multinomial logistic regression
    (softmax regression, CLIP's own linear-probe protocol; the cross-entropy the reference's predictors minimise), solved
    where the data lives, from what ``LinearProbe.fit`` takes:

        f(W, b) = 1/2 (|W|^2 + |b|^2) + C sum_i w_i (lse_i - s_{i, y_i}),   s_ik = z_i . W_k + b_k,  lse_i = log sum_k exp(s_ik)

    The intercept is regularised as one more feature, as ``LinearProbe`` does: this is scikit-learn's
    ``LogisticRegression(C, fit_intercept=False)`` on ``[Z, 1]``, and f is 1-strongly convex.  ``class_weight`` is
    ``None``, ``"balanced"`` (``n / (K count_k)``) or a ``{label: weight}`` dict, and weighs the ROW: ``w_i = cw[y_i]``
    (scikit-learn's semantics for this estimator).  Two classes are scikit-learn's one binomial problem
    ``1/2 |w|^2 + C sum_i w_i log(1 + exp(-y_i s_i))``: the K = 2 softmax is solved with C / 2 and ``coef_ = W_1 - W_0``.

    ``fit(data, labels=None, rows_per_pass=65536, keep_rows=False)`` as ``LinearProbe.fit``; a pass hands each decode group
    to ``lla_softmax_pass`` (csrc/probe.hip).  The solver is one truncated Newton-CG over all classes (Jacobi
    preconditioner, Armijo backtracking), deterministic; it stops when ``|grad f|_inf <= tol |grad f(0)|_inf``, and warns
    and sets ``converged_ = False`` at ``max_iter`` Newton steps.  CPU data run a float64 torch evaluation of the same sums.

    After ``fit``: ``coef_`` fp32 ``[K, C]`` (``[1, C]`` for two classes, positive class ``classes_[1]``), ``intercept_``,
    ``classes_``, ``n_passes_``, ``objective_`` (f at the solution; the binomial objective for two classes),
    ``converged_``.  ``decision_function`` returns ``[N, K]`` (``[N]`` for two classes) through ``lla_gemm_f32`` on the
    device; ``predict_proba`` its softmax (the sigmoid for two classes: columns ``classes_[0]``, ``classes_[1]``);
    ``predict`` labels, ``score`` the mean accuracy."""

    def __init__(self, C=1.0, tol=1e-4, max_iter=100, class_weight=None):
        if not C > 0 or not tol > 0 or int(max_iter) < 1:
            raise ValueError("C and tol must be positive, max_iter at least 1")
        if not (class_weight is None or class_weight == "balanced" or isinstance(class_weight, dict)):
            raise ValueError(f"class_weight must be None, 'balanced' or a dict, got {class_weight!r}")
        self.C, self.tol, self.max_iter, self.class_weight = float(C), float(tol), int(max_iter), class_weight

    def fit(self, data, labels=None, rows_per_pass=65536, keep_rows=False):
        rows = _Rows(data, rows_per_pass, keep_rows)
        y = _labels_of(data, labels, rows.n)
        classes, _, _ = _class_indexes(y)
        idx = torch.searchsorted(classes, y)                  # class k is classes_[k], for two classes too
        K = int(classes.numel())
        cw = _class_weights(self.class_weight, classes.numpy(), torch.bincount(idx, minlength=K))
        try:
            Sums = _DeviceSoftmaxSums if rows.device.type == "cuda" else _HostSoftmaxSums
            sums = Sums(rows, idx, cw, self.C / 2 if K == 2 else self.C)
            W, b, f, converged = _newton_cg_joint(sums, rows.dim, rows.n, rows.device, self.tol, self.max_iter)
        finally:
            rows.close()
        if K == 2:                       # from zero the solution is symmetric (W_0 = -W_1): w = W_1 - W_0 minimises the binomial f
            W, b, f = W[1:] - W[:1], b[1:] - b[:1], 2.0 * f
        self._set(W, b, classes, sums.n_passes, float(f), bool(converged))
        if not self.converged_:
            warnings.warn(f"LogisticProbe stopped short of tol = {self.tol} after {self.max_iter} Newton steps", RuntimeWarning)
        return self

    def decision_function(self, data, rows_per_pass=65536):
        s = self._scores(data, rows_per_pass)
        return s[:, 0].contiguous() if len(self.classes_) == 2 else s.contiguous()

    def predict_proba(self, data, rows_per_pass=65536):
        s = self.decision_function(data, rows_per_pass)
        if s.dim() == 1:
            p = torch.sigmoid(s)
            return torch.stack([1.0 - p, p], 1)
        return torch.softmax(s, 1)


# ---------------------------------------------------------------------- cross-validated softmax regression
class _HostSoftmaxGridSums(_HostSoftmaxSums):
    """float64 torch evaluation of the two quantities ``lla_softmax_grid_pass`` computes for G groups of K classes, times
    each group's C (the CPU path; the GPU tests' oracle): ``held`` [G] fold ids, ``cw`` [G, K] class weights, ``scale`` [G].
    The fixed blocks of ``_HostSoftmaxSums``, one group at a time."""

    def __init__(self, rows, idx, fold, held, cw, scale):
        self.rows, self.idx, self.fold = rows, idx, fold
        self.held, self.cw, self.scale = held.to(torch.int64), cw.to(torch.float64), scale.to(torch.float64)
        self.G, self.K = int(cw.shape[0]), int(cw.shape[1])
        self.cmax = self.scale * self.cw.amax(1)
        self.n_passes = 0

    def _rows_of(self, g, g0, z, W, b):
        """-> (scores [n, K], lse [n, 1], p, w_ig [n, 1], one-hot labels [n, K]) of the block for group g."""
        n = z.shape[0]
        y = self.idx[g0:g0 + n]
        s = z @ W[g].T + b[g]
        lse = torch.logsumexp(s, 1, keepdim=True)
        hot = torch.zeros_like(s).scatter_(1, y[:, None], 1.0)
        w = torch.where(self.fold[g0:g0 + n] == self.held[g], torch.zeros((), dtype=torch.float64), self.cw[g][y])
        return s, lse, torch.exp(s - lse), w[:, None], hot

    # Every product and every sum below has the shape of ONE group: a group's numbers do not depend on how many groups
    # share the batch, so solving in several batches returns the bits of one batch.
    def gradient(self, W, b):
        loss, gW, gb = torch.zeros(self.G, dtype=torch.float64), torch.zeros_like(W), torch.zeros_like(b)
        for g0, z in self._blocks():
            for g in range(self.G):
                s, lse, p, w, hot = self._rows_of(g, g0, z, W, b)
                r = w * (p - hot)
                loss[g] += (w * (lse - (s * hot).sum(1, keepdim=True))).sum()
                gW[g] += r.T @ z
                gb[g] += r.sum(0)
        self.n_passes += 1
        return self.scale * loss, self.scale[:, None, None] * gW, self.scale[:, None] * gb

    def hessian_vector(self, W, b, V, vb):
        hW, hb = torch.zeros_like(W), torch.zeros_like(b)
        for g0, z in self._blocks():
            for g in range(self.G):
                _, _, p, w, _ = self._rows_of(g, g0, z, W, b)
                t = z @ V[g].T + vb[g]
                r = w * p * (t - (p * t).sum(1, keepdim=True))
                hW[g] += r.T @ z
                hb[g] += r.sum(0)
        self.n_passes += 1
        return self.scale[:, None, None] * hW, self.scale[:, None] * hb


class _DeviceSoftmaxGridSums(_DeviceNewtonSums):
    """The same two quantities on the device, one decode per group of rows for all G classifiers.  K <= 32: one
    ``lla_softmax_grid_pass(accumulate=1)`` per decode group.  K > 32: ``lla_softmax_pass`` once per classifier on the same
    taken buffer, with that classifier's held-out rows relabelled -1 (an out-of-range label contributes exactly nothing)."""

    def __init__(self, rows, idx, fold, held, cw, scale):
        super().__init__(rows)
        dim, dev = self.dim, self.device
        self.G, self.K = int(cw.shape[0]), int(cw.shape[1])
        self.scale = scale.to(torch.float64).to(dev)
        self.scale32 = self.scale.to(torch.float32)
        self.cmax = self.scale * cw.to(torch.float64).amax(1).to(dev)
        self.cw = None if bool((cw == 1).all()) else cw.to(torch.float32).to(dev).contiguous()
        self.fused = self.K <= 32
        y, fold, held = idx.to(torch.int32).to(dev), fold.to(torch.int32).to(dev), held.to(torch.int32).to(dev)
        if self.fused:
            self.y, self.fold, self.held = y.contiguous(), fold.contiguous(), held.contiguous()
            nbytes = self.L.lla_softmax_grid_pass_workspace_bytes(dim, self.K, self.G)
        else:
            self.y, self.fold, self.held = y.contiguous(), fold.contiguous(), held.tolist()
            nbytes = self.L.lla_softmax_pass_workspace_bytes(dim, self.K, min(rows.group, max(rows.n, 1)))
        self._workspace(nbytes, f"the softmax passes refuse C = {dim}, K = {self.K}, G = {self.G}")

    def _pass(self, W, b, V, vb, st):
        G, K, C = self.G, self.K, self.dim
        oW = torch.zeros((G, K, C), dtype=torch.float32, device=self.device)
        ob = torch.zeros((G, K), dtype=torch.float32, device=self.device)
        loss = torch.zeros((G, K), dtype=torch.float64, device=self.device) if V is None else None
        at = (lambda t, g: None if t is None else t[g])
        for g0, n, zp, zt, ld in self._groups():
            if self.fused:
                rc = self.L.lla_softmax_grid_pass(zp, zt, ld, _lib.ptr(self.y[g0:g0 + n]), _lib.ptr(self.fold[g0:g0 + n]),
                                                  n, C, _lib.ptr(W), _lib.ptr(b), _lib.ptr(V), _lib.ptr(vb), K, G, C,
                                                  _lib.ptr(self.held), _lib.ptr(self.cw), _lib.ptr(oW), _lib.ptr(ob),
                                                  _lib.ptr(loss), 1, _lib.ptr(self.ws), st)
                _lib.check(rc, "lla_softmax_grid_pass")
                continue
            yn, fn = self.y[g0:g0 + n], self.fold[g0:g0 + n]
            for g in range(G):       # this classifier's labels of the decode group: -1 on the rows it holds out
                yg = torch.where(fn == self.held[g], -1, yn).to(torch.int32)
                rc = self.L.lla_softmax_pass(zp, zt, ld, _lib.ptr(yg), n, C, _lib.ptr(W[g]),
                                             _lib.ptr(b[g]), _lib.ptr(at(V, g)), _lib.ptr(at(vb, g)), K, C,
                                             _lib.ptr(at(self.cw, g)), _lib.ptr(oW[g]), _lib.ptr(ob[g]), _lib.ptr(at(loss, g)),
                                             1, _lib.ptr(self.ws), st)
                _lib.check(rc, "lla_softmax_pass")
        return (None if loss is None else self.scale * loss.sum(1)), self.scale32[:, None, None] * oW, self.scale32[:, None] * ob


def _newton_cg_joint_groups(sums, dim, n_rows, device, tol, max_iter):
    """``_newton_cg_joint`` for G classifiers side by side: W [G, K, C], b [G, K]; every group is its own joint problem with
    its own inner products, CG residual test, step length and stopping rule, and a group that has converged stands still
    while the others go on (as the problems of ``_newton_cg``) -> (W, b, f [G] float64, converged [G] bool on the CPU)."""
    dt, G, K = sums.dtype, sums.G, sums.K
    W, b = torch.zeros((G, K, dim), dtype=dt, device=device), torch.zeros((G, K), dtype=dt, device=device)
    tiny = torch.finfo(dt).tiny

    def evaluate(W, b):
        loss, gW, gb = sums.gradient(W, b)
        return 0.5 * ((W.double() ** 2).sum((1, 2)) + (b.double() ** 2).sum(1)) + loss, W + gW, b + gb

    def dot(aW, ab, cW, cb):         # per-group inner product over [K, C + 1]
        return (aW * cW).sum((1, 2)) + (ab * cb).sum(1)

    def sup(gW, gb):
        return torch.maximum(gW.abs().amax((1, 2)), gb.abs().amax(1))

    # Jacobi preconditioner per group: 1 + C_g / 4 max(cw_g) sum_i z_ic^2 with the column sums over ALL rows, held-out ones
    # included -- an upper bound of the Hessian's diagonal for every fold (any positive diagonal is valid)
    cmax = sums.cmax.to(device)
    mW = (1.0 + 0.25 * cmax[:, None, None] * sums.column_squares()[None, None, :]).to(dt)
    mb = (1.0 + 0.25 * cmax * n_rows).to(dt)[:, None]
    f, gW, gb = evaluate(W, b)
    stop_at = tol * sup(gW, gb)
    for _ in range(int(max_iter)):
        live = sup(gW, gb) > stop_at     # groups still short of the stopping rule; the others stay where they are
        if not bool(live.any()):
            break
        lv = live.to(dt)
        dW, db = torch.zeros_like(W), torch.zeros_like(b)
        rW, rb = -gW * lv[:, None, None], -gb * lv[:, None]
        yW, yb = rW / mW, rb / mb
        pW, pb = yW.clone(), yb.clone()
        rs = dot(rW, rb, yW, yb)
        stop = _CG_TOL ** 2 * dot(rW, rb, rW, rb)
        busy = live.clone()
        for _cg in range(_CG_MAX):
            hW, hb = sums.hessian_vector(W, b, pW, pb)
            hW, hb = pW + hW, pb + hb
            alpha = busy.to(dt) * rs / dot(pW, pb, hW, hb).clamp_min(tiny)
            dW += alpha[:, None, None] * pW
            db += alpha[:, None] * pb
            rW -= alpha[:, None, None] * hW
            rb -= alpha[:, None] * hb
            busy = busy & (dot(rW, rb, rW, rb) > stop)       # |H d + g|_2 <= 0.1 |g|_2: the group's step is ready
            if not bool(busy.any()):
                break
            yW, yb = rW / mW, rb / mb
            rs2 = dot(rW, rb, yW, yb)
            beta = busy.to(dt) * rs2 / rs.clamp_min(tiny)
            pW, pb = yW + beta[:, None, None] * pW, yb + beta[:, None] * pb
            rs = torch.where(busy, rs2, rs)
        # per-group backtracking: a group keeps its step length once the Armijo condition holds for it
        gd = dot(gW, gb, dW, db).double()
        t = torch.ones(G, dtype=dt, device=device)
        for _ls in range(_BACKTRACKS):
            W2, b2 = W + t[:, None, None] * dW, b + t[:, None] * db
            f2, gW2, gb2 = evaluate(W2, b2)
            ok = f2 <= f + _ARMIJO * t.double() * gd + sums.slack * f.abs()
            if bool(ok.all()):
                break
            t = torch.where(ok, t, t * 0.5)
        else:                            # groups whose step never passed stay where they were
            t = torch.where(ok, t, torch.zeros_like(t))
            W2, b2 = W + t[:, None, None] * dW, b + t[:, None] * db
            f2, gW2, gb2 = evaluate(W2, b2)
        W, b, f, gW, gb = W2, b2, f2, gW2, gb2
        if not bool(((t > 0) & live).any()):      # nothing moved: rounding has the last word
            break
    return W, b, f, (sup(gW, gb) <= stop_at).cpu()


class LogisticProbeCV:
    """``LogisticProbeCV(candidates, cv=5, tol=1e-4, max_iter=100, refit=True, max_problems=4096)``: CLIP's linear-probe
    protocol -- softmax regression with the L2 strength chosen on held-out data -- as ``LinearProbeCV`` runs the hinge's
    search: every (candidate, fold) classifier of ``LogisticProbe``'s objective solved in the same passes over the data.

    candidates  a sequence of ``(C, class_weight)``: ``LogisticProbeCV.logspace(n, low, high)`` for the usual sweep;
                what ``LinearProbeCV.sample`` returns is accepted.
    cv          as ``LinearProbeCV``: an int (stratified, unshuffled) or an int array of fold ids with -1 for rows that
                always train; ``"balanced"`` weights are counted on each fold's training part.
    refit       also fit every candidate on all rows, in the same passes: ``best_estimator_`` costs no second solve.
    max_problems  at most ``max_problems // K`` classifiers are solved side by side; more are solved in batches.

    ``fit(data, labels=None, rows_per_pass=65536, keep_rows=False)`` takes what ``LogisticProbe.fit`` takes; a pass hands
    each decode group to ``lla_softmax_grid_pass`` (K <= 32; above, to ``lla_softmax_pass`` once per classifier on the same
    decoded rows).  Every classifier is its own joint Newton-CG problem; a converged one stands still while the others go
    on.  Two classes follow ``LogisticProbe`` (the K = 2 softmax with C / 2, ``coef = W_1 - W_0``).  Afterwards:
    ``cv_scores_`` float64 ``[candidates, folds]`` (accuracy on the held-out rows), ``mean_scores_``, ``best_index_`` (the
    first maximum), ``best_params_``, ``fold_coef_`` / ``fold_intercept_`` fp32 ``[candidates, folds, K or 1, C]``,
    ``best_estimator_`` (a fitted ``LogisticProbe``; ``None`` without ``refit``), ``classes_``, ``folds_``, ``n_passes_``,
    ``converged_`` bool ``[candidates, folds (+ 1 with refit)]``; warns when a classifier stops short of ``tol``."""

    def __init__(self, candidates, cv=5, tol=1e-4, max_iter=100, refit=True, max_problems=4096):
        self.candidates = [(float(C), cw) for C, cw in candidates]
        if not self.candidates:
            raise ValueError("no candidates")
        for C, cw in self.candidates:
            LogisticProbe(C=C, tol=tol, max_iter=max_iter, class_weight=cw)       # (its checks)
        if int(max_problems) < 1:
            raise ValueError("max_problems must be at least 1")
        self.cv, self.tol, self.max_iter = cv, float(tol), int(max_iter)
        self.refit, self.max_problems = bool(refit), int(max_problems)
        self.cv_scores_ = self.best_estimator_ = None

    @staticmethod
    def logspace(n, low, high, class_weight=None):
        """n candidates with C spaced evenly in the logarithm from low to high (both included), one ``class_weight``."""
        if int(n) < 1 or not 0 < low <= high:
            raise ValueError("need n >= 1 and 0 < low <= high")
        Cs = np.exp(np.linspace(np.log(low), np.log(high), int(n))).clip(low, high)
        Cs[0], Cs[-1] = low, high        # (exp(log(x)) may miss x by an ulp; n = 1: high)
        return [(float(C), class_weight) for C in Cs]

    def fit(self, data, labels=None, rows_per_pass=65536, keep_rows=False):
        rows = _Rows(data, rows_per_pass, keep_rows)
        y = _labels_of(data, labels, rows.n)
        classes, _, _ = _class_indexes(y)
        idx = torch.searchsorted(classes, y)                  # class k is classes_[k], for two classes too
        K = int(classes.numel())
        Kp = 1 if K == 2 else K                               # rows of a reported classifier
        fold, ids, train_counts = _folds_of(self.cv, idx, K)
        all_counts = torch.bincount(idx, minlength=K)
        nc, nf = len(self.candidates), len(ids)
        per = nf + int(self.refit)
        # one classifier (group) per (candidate, fold), then per candidate one with nothing held out
        layout = [(c, f) for c in range(nc) for f in range(per)]
        step = max(self.max_problems // K, 1)
        device = rows.device
        Sums = _DeviceSoftmaxGridSums if device.type == "cuda" else _HostSoftmaxGridSums
        coef = torch.empty((nc, per, Kp, rows.dim), dtype=torch.float32, device=device)
        icpt = torch.empty((nc, per, Kp), dtype=torch.float32, device=device)
        objective = torch.empty((nc, per), dtype=torch.float64)
        converged = torch.empty((nc, per), dtype=torch.bool)
        self.n_passes_ = 0
        try:
            for at in range(0, len(layout), step):
                batch = layout[at:at + step]
                held = torch.tensor([ids[f] if f < nf else _NO_FOLD for _, f in batch], dtype=torch.int64)
                cw = torch.stack([_class_weights(self.candidates[c][1], classes.numpy(), train_counts[f] if f < nf else all_counts)
                                  for c, f in batch])
                scale = torch.tensor([self.candidates[c][0] / 2 if K == 2 else self.candidates[c][0] for c, _ in batch],
                                     dtype=torch.float64)
                sums = Sums(rows, idx, fold, held, cw, scale)
                W, b, fv, conv = _newton_cg_joint_groups(sums, rows.dim, rows.n, device, self.tol, self.max_iter)
                self.n_passes_ += sums.n_passes
                if K == 2:               # as LogisticProbe: w = W_1 - W_0 minimises the binomial objective, which is 2 f
                    W, b, fv = W[:, 1:] - W[:, :1], b[:, 1:] - b[:, :1], 2.0 * fv
                for g, (c, f) in enumerate(batch):
                    coef[c, f], icpt[c, f] = W[g], b[g]
                    objective[c, f], converged[c, f] = float(fv[g]), bool(conv[g])
            # one scoring walk, shared with LinearProbeCV (two classes: its one-column rule, whose class 0 is classes_[1])
            score_held = torch.tensor(ids, dtype=torch.int64).repeat(nc)
            right = LinearProbeCV._score(rows, coef[:, :nf].reshape(nc * nf * Kp, rows.dim), icpt[:, :nf].reshape(-1),
                                         1 - idx if K == 2 else idx, fold, score_held, Kp)
            self.n_passes_ += 1
        finally:
            rows.close()
        n_held = torch.stack([(fold == f).sum() for f in ids]).double()
        self.cv_scores_ = right.reshape(nc, nf).double() / n_held[None, :]
        self.mean_scores_ = self.cv_scores_.mean(1)
        self.best_index_ = int(self.mean_scores_.argmax())                       # the first maximum
        self.best_params_ = dict(zip(("C", "class_weight"), self.candidates[self.best_index_]))
        self.fold_coef_, self.fold_intercept_ = coef[:, :nf].contiguous(), icpt[:, :nf].contiguous()
        self.classes_, self.folds_, self.converged_ = classes.numpy(), list(ids), converged
        self.best_estimator_ = None
        if self.refit:
            best = LogisticProbe(C=self.best_params_["C"], tol=self.tol, max_iter=self.max_iter,
                                 class_weight=self.best_params_["class_weight"])
            best._set(coef[self.best_index_, nf].clone(), icpt[self.best_index_, nf].clone(), classes, self.n_passes_,
                      float(objective[self.best_index_, nf]), bool(converged[self.best_index_, nf]))
            self.best_estimator_ = best
        if not bool(converged.all()):
            warnings.warn(f"LogisticProbeCV: {int((~converged).sum())} of {converged.numel()} classifiers stopped short of "
                          f"tol = {self.tol} after {self.max_iter} Newton steps", RuntimeWarning)
        return self


# ---------------------------------------------------------------------- the reference's MLP predictor
class _Twin:
    """What the two float64 twins share: the AdamW update of ``_params()`` and the sums of an epoch.  With ``step(x, y)``
    and ``fitted(n_out)`` of its own a twin has the interface of the device engine (``_DeviceMLP``)."""

    def __init__(self, adam):
        self.adam, self.t, self.sums = adam, 0, []
        self.moments = [(torch.zeros_like(p), torch.zeros_like(p)) for p in self._params()]

    def _update(self, loss, right, grads):
        self.t += 1
        _adamw(self._params(), grads, self.moments, self.adam, self.t)
        self.sums.append((loss, right))

    def epoch_totals(self):
        """-> (loss sum, rows right) over the steps since the last call."""
        sums, self.sums = self.sums, []
        return float(sum(s[0] for s in sums)), int(sum(s[1] for s in sums))


class _TwinMLP(_Twin):
    """The float64 twin of a training step: forward, softmax cross-entropy, backward and AdamW written out by hand, formula
    by formula what the kernels of csrc/mlp.hip compute -- no autograd, so that it can be tested against autograd.  The CPU
    path of ``MLPProbe`` and the oracle of its GPU tests."""

    def __init__(self, Ws, bs, adam):
        self.Ws, self.bs = [W.to(torch.float64).clone() for W in Ws], [b.to(torch.float64).clone() for b in bs]
        super().__init__(adam)

    def _params(self):
        return self.Ws + self.bs

    def forward(self, x, pre=None):
        """-> (logits, [x, h_1, ..., h_L]): h = relu(h W^T + b) (lla_gemm_f32, relu = 1), then the last Linear.  ``pre``, a
        list, receives the hidden pre-activations."""
        return _mlp_forward(self.Ws, self.bs, x.to(torch.float64), pre)

    @staticmethod
    def xent(s, y):
        """lla_softmax_xent -> (residual with scale = 1 / rows, sum of the row losses, rows got right)."""
        mx = s.max(1, keepdim=True).values
        e = torch.exp(s - mx)
        se = e.sum(1, keepdim=True)
        hot = torch.zeros_like(s).scatter_(1, y[:, None], 1.0)
        loss = ((mx - s.gather(1, y[:, None])) + torch.log(se)).sum()
        return (e / se - hot) * (1.0 / s.shape[0]), float(loss), int((s.argmax(1) == y).sum())

    def gradients(self, x, y):
        """-> (loss sum, rows right, dW per layer, db per layer) of the mean cross-entropy of the minibatch."""
        s, hs = self.forward(x)
        delta, loss, right = self.xent(s, y)
        gW, gb, _ = _mlp_backward(self.Ws, hs, delta)                         # (nothing reads the gradient below layer 0)
        return loss, right, gW, gb

    def step(self, x, y):
        loss, right, gW, gb = self.gradients(x, y)
        self._update(loss, right, gW + gb)                                   # lla_adamw_step

    def fitted(self, n_out):
        """-> (weights, biases), copies."""
        return [W.clone() for W in self.Ws], [b.clone() for b in self.bs]


class _DeviceMLP:
    """The same step on the device, for either kind of hidden block.  ``bn=None``: a plain block, one ``lla_gemm_f32`` with
    bias and relu = 1.  ``bn=(dropout p, seed, momentum, eps)``: a batchnorm block, ``lla_gemm_f32`` (bias = NULL, relu = 0)
    into the pre-norm buffer, then ``lla_bn_relu_dropout_fwd`` into the activation.  Parameters, gradients and the two
    moments each live in ONE flat fp32 buffer (``flat[0 .. 3]``: layer l's weight [out_l][in_l], then its bias -- under a
    batchnorm block gamma and beta instead; the class dimension padded to a multiple of 8 with zero rows that never receive
    a non-zero gradient), so one ``lla_adamw_step`` updates everything, gamma and beta included (the reference hands
    ``self.parameters()`` to one group: lossyless/predictors.py:226).  Running statistics live outside it.  Every launch is a
    method of its own and ``step`` is their sequence.  Step k of an epoch writes its loss sum and rows right to slot k;
    nothing is read back before ``epoch_totals()``.  ``max_steps=0`` is a forward-only engine: no gradients, moments,
    residuals or sums."""

    def __init__(self, Ws, bs, adam, device, max_rows, n_classes, max_steps=0, bn=None):
        self.L, self.device, self.adam, self.t, self.k = _lib.lib(), device, adam, 0, 0
        self.K, self.bn = int(n_classes), bn is not None
        self.dims = [int(Ws[0].shape[1])] + [int(W.shape[0]) for W in Ws[:-1]] + [-(-self.K // 8) * 8]
        if any(d % 8 for d in self.dims[:-1]):
            raise ValueError(f"the device path needs layer widths that are multiples of 8, got {self.dims[:-1]}")
        hidden, f32 = self.dims[1:-1], dict(dtype=torch.float32, device=device)
        self.n = sum(o * i + o for i, o in zip(self.dims[:-1], self.dims[1:])) + self.bn * sum(hidden)
        self.flat = [torch.zeros(self.n, **f32) for _ in range(4 if max_steps else 1)]     # parameters; gradients, two moments
        self.W, self.b, self.gamma, self.beta = self._views(self.flat[0])
        for l, W in enumerate(Ws):
            self.W[l][:W.shape[0]].copy_(W.to(torch.float32))
        for b, src in zip(self.b, bs):
            if b is not None:
                b[:src.shape[0]].copy_(src.to(torch.float32))
        for ga in self.gamma:
            ga.fill_(1.0)
        self.rows = max(int(max_rows), 2 if self.bn else 1)
        self.acts = [torch.empty((self.rows, o), **f32) for o in self.dims[1:]]
        if self.bn:
            self.p, self.seed, self.momentum, self.eps = float(bn[0]), int(bn[1]), float(bn[2]), float(bn[3])
            self.rm, self.rv = [torch.zeros(o, **f32) for o in hidden], [torch.ones(o, **f32) for o in hidden]
            self.mean, self.rstd = [torch.empty(o, **f32) for o in hidden], [torch.empty(o, **f32) for o in hidden]
            self.pre = [torch.empty((self.rows, o), **f32) for o in hidden]
        if max_steps:                        # a training engine: views of the gradients, residuals and the per-step sums
            self.gW, self.gb, self.ggamma, self.gbeta = self._views(self.flat[1])
            self.dlogits = torch.empty((self.rows, self.dims[-1]), **f32)
            self.delta = [torch.empty((self.rows, o), **f32) for o in hidden]
            self.loss = torch.zeros(max_steps, dtype=torch.float64, device=device)
            self.right = torch.zeros(max_steps, dtype=torch.int32, device=device)
            self.ws = torch.empty(int(self.L.lla_softmax_xent_workspace_bytes(self.rows)), dtype=torch.uint8, device=device)

    def _views(self, flat):
        """-> (weight per layer, bias per layer -- None under a batchnorm block --, gamma per block, beta per block)."""
        Ws, bs, gammas, betas, at = [], [], [], [], 0
        for l, (i, o) in enumerate(zip(self.dims[:-1], self.dims[1:])):
            Ws.append(flat[at:at + o * i].view(o, i))
            at += o * i
            if self.bn and l < len(self.dims) - 2:
                gammas.append(flat[at:at + o]), betas.append(flat[at + o:at + 2 * o]), bs.append(None)
                at += 2 * o
            else:
                bs.append(flat[at:at + o])
                at += o
        return Ws, bs, gammas, betas

    def forward(self, x, ld, st):
        """-> logits [rows, Kpad] (a view of the last activation buffer) of the fp32 rows x of pitch ld (``_f32_rows``)."""
        n, last = int(x.shape[0]), len(self.W) - 1
        for l in range(last + 1):
            i, o = self.dims[l], self.dims[l + 1]
            block = self.bn and l < last
            _gemm_f32(x, ld, self.W[l], self.b[l], self.pre[l] if block else self.acts[l], o, n, o, i,
                      int(l < last and not self.bn), st)
            if block:
                self.bn_fwd(l, n, st)
            x, ld = self.acts[l], o
        return self.acts[-1][:n]

    def bn_fwd(self, l, n, st):
        """Block l's pre-norm buffer -> its activation; batch and running statistics; the dropout mask of step ``t``."""
        P, o = _lib.ptr, self.dims[l + 1]
        rc = self.L.lla_bn_relu_dropout_fwd(P(self.pre[l]), o, P(self.gamma[l]), P(self.beta[l]), P(self.acts[l]), o,
                                            P(self.mean[l]), P(self.rstd[l]), P(self.rm[l]), P(self.rv[l]), n, o, self.eps,
                                            self.momentum, self.p, self.seed, self.t, l, st)
        _lib.check(rc, "lla_bn_relu_dropout_fwd")

    def xent(self, y, n, st):
        """The logits and y -> the residual (scale 1 / n) in ``dlogits``; the loss sum and rows right in slot ``k``."""
        P, kpad = _lib.ptr, self.dims[-1]
        rc = self.L.lla_softmax_xent(P(self.acts[-1]), kpad, P(y), n, self.K, kpad, 1.0 / n, P(self.dlogits), kpad,
                                     P(self.loss[self.k:]), P(self.right[self.k:]), P(self.ws), st)
        _lib.check(rc, "lla_softmax_xent")

    def tn(self, l, delta, ldd, below, ldb, n, st):
        """Layer l's dW = delta^T below, and the column sums of delta as db where the layer has a bias."""
        P, i, o = _lib.ptr, self.dims[l], self.dims[l + 1]
        rc = self.L.lla_gemm_f32_tn(P(delta), ldd, P(below), ldb, P(self.gW[l]), i, P(self.gb[l]), n, o, i, st)
        _lib.check(rc, "lla_gemm_f32_tn")

    def nn(self, l, delta, ldd, below, ldb, n, st):
        """-> the gradient below layer l (pitch in_l): delta W_l where ``below``, the output of block l - 1, is positive."""
        P, i, o, out = _lib.ptr, self.dims[l], self.dims[l + 1], self.delta[l - 1]
        rc = self.L.lla_gemm_f32_nn(P(delta), ldd, P(self.W[l]), i, P(below), ldb, P(out), i, n, o, i, st)
        _lib.check(rc, "lla_gemm_f32_nn")
        return out

    def bn_bwd(self, l, g, da, n, st):
        """The gradient g of block l's output -> dgamma, dbeta and the gradient da of its pre-norm buffer (in place: da = g)."""
        P, o = _lib.ptr, self.dims[l + 1]
        rc = self.L.lla_bn_bwd(P(g), o, P(self.pre[l]), o, P(self.gamma[l]), P(self.mean[l]), P(self.rstd[l]), self.p,
                               P(self.ggamma[l]), P(self.gbeta[l]), P(da), o, n, o, st)
        _lib.check(rc, "lla_bn_bwd")

    def adamw(self, bc1, bc2, st):
        _adamw_step(self.L, *self.flat, self.adam, bc1, bc2, st)

    def step(self, z, y):
        """One training step on the minibatch (z, y int32 class indexes), the epoch's next."""
        if self.k == self.loss.numel():
            raise RuntimeError(f"the engine was sized for {self.k} steps an epoch: epoch_totals() starts the next one")
        n = int(z.shape[0])
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            x, ld = _f32_rows(z, self.dims[0])
            self.forward(x, ld, st)
            self.xent(y, n, st)
            delta, ldd = self.dlogits, self.dims[-1]
            for l in range(len(self.W) - 1, -1, -1):
                below, ldb = (self.acts[l - 1], self.dims[l]) if l > 0 else (x, ld)
                self.tn(l, delta, ldd, below, ldb, n, st)
                if l > 0:
                    delta, ldd = self.nn(l, delta, ldd, below, ldb, n, st), self.dims[l]
                    if self.bn:
                        self.bn_bwd(l - 1, delta, delta, n, st)
            self.t += 1
            self.k += 1
            self.adamw(*self.adam.corrections(self.t), st)

    def epoch_totals(self):
        """-> (loss sum, rows right) over the epoch's steps, in one read-back; the next step is the next epoch's first."""
        k, self.k = self.k, 0
        loss, right = torch.stack((self.loss[:k].sum(), self.right[:k].sum().double())).tolist()
        return loss, int(right)

    def fitted(self, n_out):
        """-> (weights, biases), copies without the padding; with batchnorm blocks (weights, [the last bias], gammas, betas,
        running means, running variances)."""
        Ws = [W.clone() for W in self.W[:-1]] + [self.W[-1][:n_out].clone()]
        if not self.bn:
            return Ws, [b.clone() for b in self.b[:-1]] + [self.b[-1][:n_out].clone()]
        rest = (self.gamma, self.beta, self.rm, self.rv)
        return (Ws, [self.b[-1][:n_out].clone()]) + tuple([t.clone() for t in group] for group in rest)


class _MinibatchProbe(_Scores):
    """What ``MLPProbe`` and ``BatchNormMLPProbe`` share: the hyper-parameters of the network and of AdamW, the walk over
    shuffled minibatches, and the fit around an engine -- ``_DeviceMLP`` on the device, a float64 twin on the CPU, one
    interface: ``step(z, y)``, ``epoch_totals()``, ``fitted(n_out)``.  A subclass gives ``_trainer`` (-> the engine and the
    learning rate of every epoch, or None for a constant one; it may draw from the generator) and ``_store``."""

    _MIN_ROWS, _COUNTS = 1, "n_hid_layers, epochs and batch_size must be at least 1"     # (rows a minibatch needs)
    coefs_ = intercepts_ = None

    def __init__(self, hid_dim, n_hid_layers, lr, weight_decay, betas, eps, epochs, batch_size, seed):
        if int(hid_dim) < 8 or int(hid_dim) % 8:
            raise ValueError(f"hid_dim must be a positive multiple of 8, got {hid_dim}")
        if int(n_hid_layers) < 1 or int(epochs) < 1 or int(batch_size) < self._MIN_ROWS:
            raise ValueError(self._COUNTS)
        if not lr > 0 or weight_decay < 0 or not eps >= 0 or not all(0 <= b < 1 for b in betas):
            raise ValueError("need lr > 0, weight_decay >= 0, eps >= 0 and betas in [0, 1)")
        self.hid_dim, self.n_hid_layers, self.epochs, self.batch_size = int(hid_dim), int(n_hid_layers), int(epochs), int(batch_size)
        self.lr, self.weight_decay, self.betas, self.eps, self.seed = float(lr), float(weight_decay), tuple(betas), float(eps), int(seed)

    @staticmethod
    def _tensor(data):
        t = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data))
        if t.dim() != 2:
            raise ValueError("data must be [N, C]")
        if t.dtype == torch.float16:
            raise ValueError("fp16 rows are not built for MLPProbe: pass float32")
        if t.dtype not in (torch.float32, torch.float64) or (t.device.type == "cuda" and t.dtype != torch.float32):
            t = t.to(torch.float32)
        return t

    def _epoch(self, data, rows, n, g, decode_group):
        """-> (the epoch's order, an iterator over its minibatches of rows in that order)."""
        bs = self.batch_size
        if rows is None:                     # batches() draws randperm(n, generator=g) itself: the same draw from a copy of g
            twin = torch.Generator()
            twin.set_state(g.get_state())
            order = torch.randperm(n, generator=twin)
            walk = data.batches(bs, shuffle=True, generator=g, decode_group=decode_group)
            return order, (b[0] if isinstance(b, tuple) else b for b in walk)
        order = torch.randperm(n, generator=g)
        group = max(int(decode_group) // bs, 1) * bs

        def walk():
            for g0 in range(0, n, group):
                z = rows[order[g0:g0 + group].to(rows.device)]
                for b0 in range(0, int(z.shape[0]), bs):
                    yield z[b0:b0 + bs]
        return order, walk()

    def fit(self, data, labels=None, decode_group=65536):
        if _is_latents(data):
            rows, device, n, dim = None, data.device, len(data), int(data.z_dim)
        else:
            rows = self._tensor(data)
            device, n, dim = rows.device, int(rows.shape[0]), int(rows.shape[1])
        if dim % 8:
            raise ValueError(f"in_dim must be a multiple of 8, got {dim}")
        if 0 < n % self.batch_size < self._MIN_ROWS:
            raise ValueError(f"N = {n} rows with batch_size = {self.batch_size} leave a last minibatch of one row, which batchnorm "
                             "cannot normalise: choose another batch_size (no row is dropped silently)")
        y = _labels_of(data, labels, n)
        classes, _, _ = _class_indexes(y)
        idx = torch.searchsorted(classes, y)                  # class k is classes_[k], for two classes too
        K = int(classes.numel())
        if K > 1024:
            raise ValueError(f"lla_softmax_xent takes up to 1024 classes, got {K}")
        g = torch.Generator().manual_seed(self.seed)
        Ws, bs = _mlp_init([dim] + [self.hid_dim] * self.n_hid_layers + [K], g)
        adam = _Adam(self.lr, self.weight_decay, self.betas, self.eps)
        engine, rates = self._trainer(Ws, bs, adam, g, device, min(self.batch_size, n), K, -(-n // self.batch_size))
        if device.type == "cuda":
            idx = idx.to(torch.int32).to(device)
        self.loss_curve_, self.accuracy_curve_ = [], []
        for epoch in range(self.epochs):
            if rates is not None:
                adam.lr = rates[epoch]
            order, walk = self._epoch(data, rows, n, g, decode_group)
            y_epoch, at = idx[order.to(idx.device)].contiguous(), 0
            for z in walk:
                bn = int(z.shape[0])
                engine.step(z, y_epoch[at:at + bn])
                at += bn
            loss, right = engine.epoch_totals()
            self.loss_curve_.append(loss / n)
            self.accuracy_curve_.append(right / n)
        self.classes_, self.n_steps_ = classes.numpy(), engine.t
        self._store(*engine.fitted(K))
        return self

    def predict_proba(self, data, rows_per_pass=65536):
        return torch.softmax(self.decision_function(data, rows_per_pass), 1)


class MLPProbe(_MinibatchProbe):
    """``MLPProbe(hid_dim=2048, n_hid_layers=2, lr=1e-3, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8, epochs=10,
    batch_size=128, seed=0)``: the reference's non-linear predictor -- its ``MLP`` (lossyless/architectures.py:94-168) AT ITS
    CLASS DEFAULTS (``norm_layer="identity"``, ``activation="ReLU"``, ``dropout_p=0``: Linear -> ReLU per hidden layer with
    biases, then Linear), trained as lossyless/predictors.py:38-232 trains it: cross-entropy, AdamW (``weight_decay=0``: Adam)
    on shuffled minibatches -- from a dataset that stays compressed in HBM.  It is NOT the reference's
    ``config/architecture/mlp_probe.yaml``, which asks for batchnorm and dropout 0.2 -- that is ``BatchNormMLPProbe`` below:
    ``norm_layer="batchnorm"``, ``dropout_p > 0`` and a learning-rate ``scheduler`` raise ``ValueError`` here, as do regression
    targets and fp16 rows, which are not built.

    ``fit(data, labels=None, decode_group=65536)``
        data    a ``CompressedLatents`` / ``HyperpriorLatents`` (its own labels unless ``labels`` is given), or a ``[N, C]``
                tensor / array with ``labels``.  ``C % 8 == 0`` and ``hid_dim % 8 == 0``.
        Initialisation is the reference's ``weights_init`` (``kaiming_uniform_(nonlinearity="relu")``, zero biases), drawn on
        the CPU from ``torch.Generator().manual_seed(seed)`` in layer order; the same generator then gives every epoch its
        order, ``torch.randperm(N, generator=g)``.  Latents are walked through ``data.batches(batch_size, shuffle=True,
        generator=g, decode_group=decode_group)`` -- the random-access decode, a decode group per launch -- and a tensor is
        indexed by the same permutation, so both see the same minibatches.  The last, shorter batch is kept (its loss is
        the mean over its own rows).
    GPU latents and CUDA tensors train in the kernels of csrc/mlp.hip (see ``_DeviceMLP``): deterministic, bit for bit.  CPU
    latents and CPU tensors train in a float64 torch twin with a hand-written backward pass and AdamW (``_TwinMLP``).

    After ``fit``: ``coefs_`` / ``intercepts_`` (one per Linear layer; fp32 on the device, float64 from the twin),
    ``classes_`` (sorted unique labels; logit k belongs to ``classes_[k]``, for two classes too), ``loss_curve_`` (mean
    training loss per epoch), ``accuracy_curve_``, ``n_steps_``.  ``decision_function`` returns the logits ``[N, K]`` (fp32
    through ``lla_gemm_f32`` on the device, float64 on the CPU), ``predict_proba`` their softmax, ``predict`` labels,
    ``score`` the mean accuracy.  ``state_dict()`` has the keys of the reference's ``MLP``: ``module.0.weight``,
    ``module.0.bias``, ``module.4.weight``, ... (four modules per hidden block)."""

    _PIECE = 8192            # rows per forward pass when scoring (activations of hid_dim floats per row)

    def __init__(self, hid_dim=2048, n_hid_layers=2, lr=1e-3, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8, epochs=10,
                 batch_size=128, seed=0, norm_layer="identity", activation="ReLU", dropout_p=0, scheduler=None):
        if norm_layer not in ("identity", None):
            raise ValueError(f"norm_layer={norm_layer!r} is not built here: MLPProbe is the reference's MLP with norm_layer='identity' "
                             "(batchnorm: BatchNormMLPProbe)")
        if activation != "ReLU":
            raise ValueError(f"activation={activation!r} is not built: MLPProbe is the reference's MLP with activation='ReLU'")
        if dropout_p != 0:
            raise ValueError("dropout_p > 0 is not built here: MLPProbe is the reference's MLP with dropout_p=0 (dropout: BatchNormMLPProbe)")
        if scheduler is not None:
            raise ValueError("learning-rate schedulers are not built here (scheduler=: BatchNormMLPProbe)")
        super().__init__(hid_dim, n_hid_layers, lr, weight_decay, betas, eps, epochs, batch_size, seed)
        self._packed = None

    # ------------------------------------------------------------------ fit
    def _trainer(self, Ws, bs, adam, g, device, rows, K, steps):
        if device.type == "cuda":
            return _DeviceMLP(Ws, bs, adam, device, rows, K, steps), None
        return _TwinMLP(Ws, bs, adam), None

    def _store(self, coefs, intercepts):
        self.coefs_, self.intercepts_, self._packed = coefs, intercepts, None

    # ------------------------------------------------------------------ predict
    def _engine(self, dev):
        """A forward-only device engine holding the fitted weights (cached per device)."""
        if self._packed is None or self._packed[0] != str(dev):
            eng = _DeviceMLP(self.coefs_, self.intercepts_, None, dev, self._PIECE, len(self.classes_))
            self._packed = (str(dev), eng)
        return self._packed[1]

    def decision_function(self, data, rows_per_pass=65536):
        if self.coefs_ is None:
            raise RuntimeError("fit first")
        if not _is_latents(data):
            data = self._tensor(data)
        rows = _Rows(data, rows_per_pass, False)
        rows.first_pass = _is_latents(data)
        K, C = len(self.classes_), int(self.coefs_[0].shape[1])
        if rows.dim != C:
            raise ValueError(f"data has {rows.dim} features, the probe was fitted on {C}")
        try:
            if rows.device.type == "cuda":
                eng = self._engine(rows.device)
                out = torch.empty((rows.n, K), dtype=torch.float32, device=rows.device)
                with torch.cuda.device(rows.device):
                    st = _lib.stream_ptr(rows.device)
                    for g0, z in rows.groups():
                        for r0 in range(0, int(z.shape[0]), self._PIECE):
                            zz = z[r0:r0 + self._PIECE]
                            out[g0 + r0:g0 + r0 + int(zz.shape[0])] = eng.forward(*_f32_rows(zz, C), st)[:, :K]
                return out
            twin = _TwinMLP([W.cpu() for W in self.coefs_], [b.cpu() for b in self.intercepts_], None)
            parts = [twin.forward(z)[0] for _, z in rows.groups()]
            return torch.cat(parts) if parts else torch.zeros((0, K), dtype=torch.float64)
        finally:
            rows.close()

    def state_dict(self):
        """The fitted weights under the keys of the reference's ``MLP`` (``module`` is Linear, Norm, Activation, Dropout per
        hidden block, then Linear): fp32 CPU tensors that ``load_state_dict(strict=True)`` takes."""
        if self.coefs_ is None:
            raise RuntimeError("fit first")
        out = {}
        for l, (W, b) in enumerate(zip(self.coefs_, self.intercepts_)):
            out[f"module.{4 * l}.weight"] = W.detach().to(torch.float32).cpu().clone()
            out[f"module.{4 * l}.bias"] = b.detach().to(torch.float32).cpu().clone()
        return out


# ------------------------------------------------- the reference's predictor as configured: batchnorm, dropout, a schedule
def _fold_batchnorm(Ws, b_last, gammas, betas, rms, rvs, eps):
    """Evaluation-mode BatchNorm1d folded into the bias-free Linear below it, in float64 on the host:
    W' = diag(gamma / sqrt(rv + eps)) W,  b' = beta - gamma rm / sqrt(rv + eps)  -> (weights, biases) of a plain ReLU MLP."""
    fW, fb = [], []
    for W, ga, be, rm, rv in zip(Ws[:-1], gammas, betas, rms, rvs):
        sc = ga.double().cpu() / torch.sqrt(rv.double().cpu() + eps)
        fW.append(sc[:, None] * W.double().cpu())
        fb.append(be.double().cpu() - sc * rm.double().cpu())
    return fW + [Ws[-1].double().cpu()], fb + [b_last.double().cpu()]


class _TwinBNMLP(_Twin):
    """The float64 twin of a training step of Linear(bias=False) -> BatchNorm1d -> ReLU -> Dropout blocks and a last Linear:
    every formula of csrc/batchnorm.hip and csrc/mlp.hip written out by hand, no autograd.  The CPU path of
    ``BatchNormMLPProbe`` and the oracle of its GPU tests.  ``step`` numbers the minibatches from 0 (the dropout counter)."""

    def __init__(self, Ws, b_last, adam, p, seed, momentum, eps):
        f64 = torch.float64
        self.Ws, self.b = [W.to(f64).clone() for W in Ws], b_last.to(f64).clone()
        self.gammas = [torch.ones(W.shape[0], dtype=f64) for W in Ws[:-1]]
        self.betas = [torch.zeros(W.shape[0], dtype=f64) for W in Ws[:-1]]
        self.rms = [torch.zeros(W.shape[0], dtype=f64) for W in Ws[:-1]]
        self.rvs = [torch.ones(W.shape[0], dtype=f64) for W in Ws[:-1]]
        self.p, self.s, self.seed, self.momentum, self.eps = float(p), _dropout_scale(p), int(seed), float(momentum), float(eps)
        super().__init__(adam)

    def _params(self):
        return self.Ws + self.gammas + self.betas + [self.b]

    def keep(self, step, layer, rows, cols):
        return dropout_keep(self.seed, step, layer, rows, cols, self.p)

    def gradients(self, x, y, track=False):
        """-> (loss sum, rows right, grads) of the mean cross-entropy of the minibatch, grads in the order of
        ``_params()``: dW per layer, dgamma per block, dbeta per block, db of the last layer.  ``track``: also update the
        running statistics, as the forward of a module in training mode does."""
        zero = torch.zeros((), dtype=torch.float64)
        B = int(x.shape[0])
        hs, xhats, rstds = [x.to(torch.float64)], [], []
        for l, (W, ga, be) in enumerate(zip(self.Ws[:-1], self.gammas, self.betas)):
            a = hs[-1] @ W.T                                                 # lla_gemm_f32, bias = NULL
            mean = a.sum(0) / B                                              # lla_bn_relu_dropout_fwd
            d = a - mean
            var = (d * d).sum(0) / B
            rstd = 1.0 / torch.sqrt(var + self.eps)
            yv = ga * (d * rstd) + be
            h = torch.where(yv > 0, yv, zero)
            if self.p > 0:
                h = torch.where(self.keep(self.t, l, B, int(a.shape[1])), h * self.s, zero)
            if track:
                self.rms[l] = (1.0 - self.momentum) * self.rms[l] + self.momentum * mean
                self.rvs[l] = (1.0 - self.momentum) * self.rvs[l] + self.momentum * (var * (B / (B - 1)))
            hs.append(h), xhats.append(d * rstd), rstds.append(rstd)
        s = hs[-1] @ self.Ws[-1].T + self.b
        delta, loss, right = _TwinMLP.xent(s, y)
        n = len(self.Ws)
        gW, gg, gb = [None] * n, [None] * (n - 1), [None] * (n - 1)
        gW[-1], g_last = delta.T @ hs[-1], delta.sum(0)                      # lla_gemm_f32_tn
        g = torch.where(hs[-1] > 0, delta @ self.Ws[-1], zero)               # lla_gemm_f32_nn with H = out
        for l in range(n - 2, -1, -1):
            gh = self.s * g if self.p > 0 else g                             # lla_bn_bwd
            gb[l], gg[l] = gh.sum(0), (gh * xhats[l]).sum(0)
            da = self.gammas[l] * rstds[l] * (gh - gb[l] / B - xhats[l] * (gg[l] / B))
            gW[l] = da.T @ hs[l]                                             # lla_gemm_f32_tn, db = NULL
            if l > 0:
                g = torch.where(hs[l] > 0, da @ self.Ws[l], zero)
        return loss, right, gW + gg + gb + [g_last]

    def step(self, x, y):
        self._update(*self.gradients(x, y, track=True))                      # lla_adamw_step

    def fitted(self, n_out):
        """-> (Ws, b_last, gammas, betas, running means, running variances), copies."""
        return tuple([t.clone() for t in group] for group in (self.Ws, [self.b], self.gammas, self.betas, self.rms, self.rvs))


class BatchNormMLPProbe(_MinibatchProbe):
    """``BatchNormMLPProbe(hid_dim=2048, n_hid_layers=2, lr=3e-4, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8, epochs=10,
    batch_size=128, seed=0, norm_layer="batchnorm", activation="ReLU", dropout_p=0.2, scheduler=None, decay_factor=100,
    k_steps=3, bn_momentum=0.1, bn_eps=1e-5)``: the reference's predictor AS ITS CONFIGURATION BUILDS IT
    (config/architecture/mlp_probe.yaml with ``optimizer_pred: AdamW_lr3e-4_w1e-5``): every hidden block of its ``MLP``
    (lossyless/architectures.py:94-168) is Linear(bias=False) -> BatchNorm1d -> ReLU -> Dropout(p), the last Linear has a
    bias, and all parameters -- gamma and beta included -- are one AdamW group (lossyless/predictors.py:226).  Trained on
    shuffled minibatches from a dataset that stays compressed in HBM, exactly as ``MLPProbe`` walks it.

    ``scheduler``  None, ``"unifmultistep"`` (the configuration's ``unifmultistep100``: ``decay_factor=100, k_steps=3``) or
        ``"expdecay"`` over ``epochs``, stepped once per epoch (``lr_schedule``; lossyless/helpers.py:536-545).  The rate of
        every epoch is ``lr_curve_``.
    ``norm_layer`` any string containing ``"batch"``, as the reference's ``get_Normalization``; ``"identity"`` is ``MLPProbe``.
    Initialisation: ``MLPProbe``'s draw for the weights from ``torch.Generator().manual_seed(seed)``, gamma = 1, beta = 0, a
    zero last bias; then the 64-bit dropout seed (two 32-bit draws, low word first); then every epoch's permutation.  The
    dropout mask is ``dropout_keep(seed, step, layer, ...)`` with ``step`` the number of steps taken before: a function of the
    seed and the position alone, the same on the device and on the CPU.  A last minibatch of ONE row cannot be normalised:
    ``fit`` raises before any training.

    GPU latents and CUDA tensors train in the kernels of csrc/batchnorm.hip and csrc/mlp.hip (``_DeviceMLP`` with ``bn``):
    deterministic, bit for bit.  CPU data trains in the float64 twin (``_TwinBNMLP``).  ``decision_function`` / ``predict`` /
    ``predict_proba`` / ``score`` are evaluation mode: running statistics, no dropout -- each block folded on the host in
    float64 into a Linear with a bias and run as ``MLPProbe`` runs its forward pass (fp32 on the device, float64 on the CPU).

    After ``fit``: ``coefs_`` (one weight per Linear), ``intercepts_`` (the last Linear's bias, a list of one), ``bn_weights_``,
    ``bn_biases_``, ``running_means_``, ``running_vars_``, ``num_batches_tracked_``, ``classes_``, ``loss_curve_``,
    ``accuracy_curve_`` (training mode, with dropout), ``lr_curve_``, ``n_steps_``.  ``state_dict()`` has the keys of the
    reference's module and loads with ``strict=True``."""

    _MIN_ROWS, _COUNTS = 2, "n_hid_layers and epochs must be at least 1, batch_size at least 2"

    def __init__(self, hid_dim=2048, n_hid_layers=2, lr=3e-4, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8, epochs=10,
                 batch_size=128, seed=0, norm_layer="batchnorm", activation="ReLU", dropout_p=0.2, scheduler=None,
                 decay_factor=100, k_steps=3, bn_momentum=0.1, bn_eps=1e-5):
        if not isinstance(norm_layer, str) or "batch" not in norm_layer:
            raise ValueError(f"norm_layer={norm_layer!r}: BatchNormMLPProbe is the reference's MLP with a batchnorm norm_layer; "
                             "norm_layer='identity' is MLPProbe")
        if activation != "ReLU":
            raise ValueError(f"activation={activation!r} is not built: only activation='ReLU'")
        if not 0 <= dropout_p < 1 or not float(np.float32(dropout_p)) < 1:
            raise ValueError(f"dropout_p must satisfy 0 <= dropout_p < 1, got {dropout_p}")
        if scheduler not in (None, "unifmultistep", "expdecay"):
            raise ValueError(f"scheduler={scheduler!r} is not built: None, 'unifmultistep' or 'expdecay'")
        if not decay_factor > 0 or int(k_steps) < 1:
            raise ValueError("need decay_factor > 0 and k_steps >= 1")
        super().__init__(hid_dim, n_hid_layers, lr, weight_decay, betas, eps, epochs, batch_size, seed)
        if not 0 <= bn_momentum <= 1 or not bn_eps >= 0:
            raise ValueError("need 0 <= bn_momentum <= 1 and bn_eps >= 0")
        self.dropout_p, self.scheduler, self.decay_factor, self.k_steps = float(dropout_p), scheduler, decay_factor, int(k_steps)
        self.bn_momentum, self.bn_eps = float(bn_momentum), float(bn_eps)
        self._folded = None

    def _trainer(self, Ws, bs, adam, g, device, rows, K, steps):
        lo, hi = (int(w) for w in torch.randint(0, 2 ** 32, (2,), generator=g, dtype=torch.int64))
        self.dropout_seed_ = lo | (hi << 32)
        self.lr_curve_ = lr_schedule(self.scheduler, self.lr, self.epochs, self.decay_factor, self.k_steps)
        bn = (self.dropout_p, self.dropout_seed_, self.bn_momentum, self.bn_eps)
        if device.type == "cuda":
            return _DeviceMLP(Ws, bs, adam, device, rows, K, steps, bn), self.lr_curve_
        return _TwinBNMLP(Ws, bs[-1], adam, *bn), self.lr_curve_

    def _store(self, coefs, intercepts, gammas, betas, rms, rvs):
        self.coefs_, self.intercepts_, self.bn_weights_, self.bn_biases_ = coefs, intercepts, gammas, betas
        self.running_means_, self.running_vars_, self.num_batches_tracked_, self._folded = rms, rvs, self.n_steps_, None

    def _eval_probe(self):
        """The fitted network in evaluation mode as a plain ReLU MLP (``_fold_batchnorm``, rounded once to fp32 where the
        fit ran on the device), held by an ``MLPProbe`` whose forward pass scores it."""
        if self.coefs_ is None:
            raise RuntimeError("fit first")
        if self._folded is None:
            fW, fb = _fold_batchnorm(self.coefs_, self.intercepts_[0], self.bn_weights_, self.bn_biases_, self.running_means_,
                                     self.running_vars_, self.bn_eps)
            inner = MLPProbe(hid_dim=self.hid_dim, n_hid_layers=self.n_hid_layers)
            dev, dtype = self.coefs_[0].device, self.coefs_[0].dtype
            inner.coefs_, inner.intercepts_ = [W.to(dtype).to(dev) for W in fW], [b.to(dtype).to(dev) for b in fb]
            inner.classes_ = self.classes_
            self._folded = inner
        return self._folded

    def decision_function(self, data, rows_per_pass=65536):
        return self._eval_probe().decision_function(data, rows_per_pass)

    def state_dict(self):
        """The fitted tensors under the keys of the reference's ``MLP`` (``module`` is Linear, BatchNorm1d, ReLU, Dropout per
        hidden block, then Linear): CPU tensors (fp32, ``num_batches_tracked`` int64) that ``load_state_dict(strict=True)``
        takes."""
        if self.coefs_ is None:
            raise RuntimeError("fit first")
        f32 = lambda t: t.detach().to(torch.float32).cpu().clone()          # noqa: E731
        out, n = {}, len(self.coefs_) - 1
        for l in range(n):
            out[f"module.{4 * l}.weight"] = f32(self.coefs_[l])
            out[f"module.{4 * l + 1}.weight"] = f32(self.bn_weights_[l])
            out[f"module.{4 * l + 1}.bias"] = f32(self.bn_biases_[l])
            out[f"module.{4 * l + 1}.running_mean"] = f32(self.running_means_[l])
            out[f"module.{4 * l + 1}.running_var"] = f32(self.running_vars_[l])
            out[f"module.{4 * l + 1}.num_batches_tracked"] = torch.tensor(self.num_batches_tracked_, dtype=torch.int64)
        out[f"module.{4 * n}.weight"] = f32(self.coefs_[n])
        out[f"module.{4 * n}.bias"] = f32(self.intercepts_[0])
        return out


# ---------------------------------------------------------------------------------------------------------------- k-NN
def _knn_merge(val, idx, s, g0, k):
    """The float64 twin's list update: the running lists (val, idx) [Q, <= k] and the scores s [Q, g] of rows g0 .. g0 + g - 1
    -> the k best of both by (score descending, index ascending).  A stable descending sort keeps equal scores in the order
    they come in, and they come in index order: a group's columns ascend, and every index of the running list (itself in
    that order among equals) lies below g0."""
    sv, si = torch.sort(s, dim=1, descending=True, stable=True)
    val = torch.cat([val, sv[:, :k]], 1)
    idx = torch.cat([idx, si[:, :k] + g0], 1)
    val, order = torch.sort(val, dim=1, descending=True, stable=True)
    return val[:, :k].contiguous(), torch.gather(idx, 1, order)[:, :k].contiguous()


def _knn_votes64(val, idx, y, K, inv_T):
    """votes[i, c] = sum_r exp((s_ir - s_i0) inv_T) [y[idx_ir] == c] in float64, added serially in rank order."""
    Q, k = val.shape
    votes = torch.zeros((Q, K), dtype=torch.float64, device=val.device)
    w = torch.exp((val - val[:, :1]) * inv_T)
    rows = torch.arange(Q, device=val.device)
    for r in range(k):
        seen = idx[:, r] >= 0
        votes[rows[seen], y[idx[seen, r]]] += w[seen, r]
    return votes


class KNNProbe:
    """``KNNProbe(k=20, T=0.07, metric="cosine", weights="softmax")``: the weighted k-nearest-neighbour classifier of Wu et
    al. 2018 and DINO -- the training-free protocol for judging frozen features -- and the way to get *neighbours* out of a
    container.  A query's k best fitted rows by cosine similarity (``metric="dot"``: by inner product) vote for their class
    with weight ``exp(s / T)`` (``weights="uniform"``: 1); the class with the most votes wins, a tie going to the lower
    class index.  Nothing proportional to queries x rows is ever held: a block of queries stays resident, the fitted rows
    are walked once per block, one decode group at a time, through ``lla_knn_pass`` (csrc/knn.hip), whose scores never leave
    the chip, and ``lla_knn_finish`` writes the lists and the votes.

    ``fit(data, labels=None)``
        data    a ``CompressedLatents`` / ``HyperpriorLatents`` (it stays compressed: only its labels are taken), or an
                ``[N, C]`` tensor / array.  Without labels only ``kneighbors`` works.
    ``kneighbors(queries=None, k=None, rows_per_pass=65536, queries_per_pass=8192, exclude_self=False)``
        -> (similarity ``[Q, k]``, index ``[Q, k]`` int64 into the fitted rows), best first, ordered by (similarity
        descending, index ascending): duplicates of a row come out lowest index first.  fp32 from the device, float64 from
        the CPU twin.  ``exclude_self=True`` (the queries must be the fitted data: the same object, or ``None``) skips every
        query's own row -- the leave-one-out search that ``k`` and ``T`` are chosen by.
    ``predict_proba`` (votes / their sum), ``predict``, ``score(queries, labels=None, ...)`` take the same arguments;
    ``score_grid(queries, ks, Ts, labels=None, ...)`` -> ``{(k, T): accuracy}`` from ONE search at ``max(ks)``: the lists
    are sorted, so a query's top k' is the head of its top k.

    The lists are a pure function of the data: the same bits for any ``rows_per_pass`` and ``queries_per_pass``.  The device
    needs ``C % 8 == 0``, ``C <= 1024`` and ``k <= 256``.  CPU data (``device="cpu"`` latents, CPU tensors) run a float64
    torch twin with the same contract, a block of ``queries_per_pass x rows_per_pass`` scores at a time."""

    def __init__(self, k=20, T=0.07, metric="cosine", weights="softmax"):
        if int(k) < 1 or not T > 0:
            raise ValueError("k must be at least 1 and T positive")
        if metric not in ("cosine", "dot") or weights not in ("softmax", "uniform"):
            raise ValueError(f"metric must be 'cosine' or 'dot' and weights 'softmax' or 'uniform', got {metric!r}, {weights!r}")
        self.k, self.T, self.metric, self.weights = int(k), float(T), metric, weights
        self.classes_ = None
        self._data = None

    # ------------------------------------------------------------------ fit
    def fit(self, data, labels=None):
        rows = _Rows(data, 1, False)
        if rows.n < 1:
            raise ValueError("no rows to fit")
        self._data, self._n, self._dim, self._device = data, rows.n, rows.dim, rows.device
        if labels is None and not (_is_latents(data) and data._labels is not None):
            self._y = self._labels = self.classes_ = None
        else:
            self._labels = _labels_of(data, labels, rows.n)
            classes = torch.unique(self._labels)
            self._y = torch.searchsorted(classes, self._labels)
            self.classes_ = classes.numpy()
        self._y_dev = None
        return self

    # ------------------------------------------------------------------ the search
    def _inv_T(self, T):
        return 0.0 if self.weights == "uniform" else 1.0 / float(T)

    def _search(self, queries, k, rows_per_pass, queries_per_pass, exclude_self, lists, grid):
        """One neighbour search at ``k`` -> (similarity, index) if ``lists``, and the votes [Q, K] of every (k', inv_T) of
        ``grid``."""
        if self._data is None:
            raise RuntimeError("fit first")
        if queries is None:
            queries = self._data
        if exclude_self and queries is not self._data:
            raise ValueError("exclude_self needs the queries to be the fitted data (the same object, or queries=None)")
        k, dev = int(k), self._device
        on_device = dev.type == "cuda"
        usable = self._n - (1 if exclude_self else 0)
        if k < 1 or k > usable:
            raise ValueError(f"k = {k} for {usable} usable fitted rows")
        if grid and self._y is None:
            raise ValueError("no labels: fit with labels=, or with latents opened with a label_file")
        if any(kk < 1 or kk > k for kk, _ in grid):
            raise ValueError("every k of the grid must lie in [1, max(ks)]")
        qrows = _Rows(queries, queries_per_pass, False)
        qrows.first_pass = _is_latents(queries)
        train = _Rows(self._data, rows_per_pass, False)
        train.first_pass = _is_latents(self._data)
        if qrows.dim != self._dim:
            raise ValueError(f"the queries have {qrows.dim} features, the probe was fitted on {self._dim}")
        C, K = self._dim, 0 if self._y is None else len(self.classes_)
        if on_device:
            _check_width(C, "k-NN")
            if k > 256:
                raise ValueError(f"the device k-NN keeps lists of at most 256 neighbours, got k = {k}")
            if grid and (self._y_dev is None or self._y_dev.device != dev):
                self._y_dev = self._y.to(torch.int32).to(dev)
        dt = torch.float32 if on_device else torch.float64
        sims, idxs, votes = [], [], [[] for _ in grid]
        cosine = self.metric == "cosine"
        try:
            for b0, qz in qrows.groups():
                B = int(qz.shape[0])
                qn = qz.to(dev).to(torch.float64)
                if cosine:                       # (a row of zeros stays zero: its similarities are 0)
                    norm = qn.norm(dim=1, keepdim=True)
                    qn = qn / torch.where(norm > 0, norm, torch.ones_like(norm))
                own = torch.arange(b0, b0 + B, device=dev) if exclude_self else None
                if on_device:
                    val, idx, vs = self._device_block(qn.to(torch.float32).contiguous(), train, k, own, lists, grid, K)
                else:
                    val, idx, vs = self._host_block(qn, train, k, own, grid, K)
                if lists:
                    sims.append(val), idxs.append(idx)
                for slot, v in zip(votes, vs):
                    slot.append(v)
        finally:
            qrows.close()
            train.close()
        cat = lambda parts, width, dtype: (torch.cat(parts) if parts else                       # noqa: E731
                                           torch.zeros((0, width), dtype=dtype, device=dev))
        out_lists = (cat(sims, k, dt), cat(idxs, k, torch.int64)) if lists else None
        return out_lists, [cat(v, K, dt) for v in votes]

    def _device_block(self, qn, train, k, own, lists, grid, K):
        L, dev = _lib.lib(), qn.device
        B, C = int(qn.shape[0]), int(qn.shape[1])
        nbytes = int(L.lla_knn_pass_workspace_bytes(B, k))
        if nbytes == 0:
            raise ValueError(f"lla_knn_pass refuses Q = {B}, k = {k}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        own32 = None if own is None else own.to(torch.int32)
        metric = 1 if self.metric == "cosine" else 0
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            accumulate = 0
            for g0, z in train.groups():
                rc = L.lla_knn_pass(_lib.ptr(qn), C, B, *_z_args(z, C), int(z.shape[0]), C, g0, k, metric,
                                    _lib.ptr(own32), accumulate, _lib.ptr(ws), st)
                _lib.check(rc, "lla_knn_pass")
                accumulate = 1
            val = idx = None
            vs = []
            for kk, inv_T in grid or [(k, 0.0)]:
                tv = torch.empty((B, kk), dtype=torch.float32, device=dev)
                ti = torch.empty((B, kk), dtype=torch.int32, device=dev)
                v = torch.empty((B, K), dtype=torch.float32, device=dev) if grid else None
                rc = L.lla_knn_finish(B, k, kk, _lib.ptr(self._y_dev if grid else None), K, inv_T, _lib.ptr(tv), _lib.ptr(ti),
                                      _lib.ptr(v), _lib.ptr(ws), st)
                _lib.check(rc, "lla_knn_finish")
                if grid:
                    vs.append(v)
                if kk == k:
                    val, idx = tv, ti
            if lists and val is None:            # (no entry of the grid asked for all k)
                val = torch.empty((B, k), dtype=torch.float32, device=dev)
                idx = torch.empty((B, k), dtype=torch.int32, device=dev)
                _lib.check(L.lla_knn_finish(B, k, k, None, 0, 0.0, _lib.ptr(val), _lib.ptr(idx), None, _lib.ptr(ws), st),
                           "lla_knn_finish")
        return val, (idx.to(torch.int64) if lists else None), vs

    def _host_block(self, qn, train, k, own, grid, K):
        B = int(qn.shape[0])
        val = torch.zeros((B, 0), dtype=torch.float64)
        idx = torch.zeros((B, 0), dtype=torch.int64)
        for g0, z in train.groups():
            z = z.to(torch.float64)
            s = qn @ z.T
            if self.metric == "cosine":
                ss = (z * z).sum(1)
                s = s * torch.where(ss > 0, 1.0 / torch.sqrt(ss), torch.zeros_like(ss))[None, :]
            if own is not None:                  # (k <= N - 1 finite scores: a skipped row never stays listed)
                mine = (own >= g0) & (own < g0 + z.shape[0])
                s[torch.nonzero(mine)[:, 0], own[mine] - g0] = -float("inf")
            val, idx = _knn_merge(val, idx, s, g0, k)
        y = self._y
        return val, idx, [_knn_votes64(val[:, :kk], idx[:, :kk], y, K, inv_T) for kk, inv_T in grid]

    # ------------------------------------------------------------------ the public calls
    def kneighbors(self, queries=None, k=None, rows_per_pass=65536, queries_per_pass=8192, exclude_self=False):
        k = self.k if k is None else k
        return self._search(queries, k, rows_per_pass, queries_per_pass, exclude_self, True, [])[0]

    def _votes(self, queries, k, T, rows_per_pass, queries_per_pass, exclude_self):
        k = self.k if k is None else int(k)
        T = self.T if T is None else T
        return self._search(queries, k, rows_per_pass, queries_per_pass, exclude_self, False, [(k, self._inv_T(T))])[1][0]

    @staticmethod
    def _winners(votes):
        """argmax over the classes; a tie goes to the lower class index."""
        K = votes.shape[1]
        at = torch.arange(K, device=votes.device)[None, :].expand_as(votes)
        return torch.where(votes == votes.amax(1, keepdim=True), at, torch.full_like(at, K)).amin(1)

    def predict_proba(self, queries=None, k=None, T=None, rows_per_pass=65536, queries_per_pass=8192, exclude_self=False):
        votes = self._votes(queries, k, T, rows_per_pass, queries_per_pass, exclude_self)
        return votes / votes.sum(1, keepdim=True)

    def predict(self, queries=None, k=None, T=None, rows_per_pass=65536, queries_per_pass=8192, exclude_self=False):
        votes = self._votes(queries, k, T, rows_per_pass, queries_per_pass, exclude_self)
        return torch.from_numpy(self.classes_).to(votes.device)[self._winners(votes)]

    def _truth(self, queries, labels, n):
        if queries is None or (queries is self._data and labels is None):
            if labels is None:
                return self._labels
            queries = self._data
        return _labels_of(queries, labels, n)

    def score(self, queries=None, labels=None, k=None, T=None, rows_per_pass=65536, queries_per_pass=8192,
              exclude_self=False):
        pred = self.predict(queries, k, T, rows_per_pass, queries_per_pass, exclude_self)
        y = self._truth(queries, labels, pred.numel()).to(pred.device)
        return float((pred == y).double().mean())

    def score_grid(self, queries, ks, Ts, labels=None, exclude_self=False, rows_per_pass=65536, queries_per_pass=8192):
        ks, Ts = [int(k) for k in ks], [float(T) for T in Ts]
        if not ks or not Ts:
            raise ValueError("ks and Ts must not be empty")
        grid = [(k, T) for k in ks for T in Ts]
        votes = self._search(queries, max(ks), rows_per_pass, queries_per_pass, exclude_self, False,
                             [(k, self._inv_T(T)) for k, T in grid])[1]
        classes = torch.from_numpy(self.classes_)
        out = {}
        for key, v in zip(grid, votes):
            pred = classes.to(v.device)[self._winners(v)]
            y = self._truth(queries, labels, pred.numel()).to(pred.device)
            out[key] = float((pred == y).double().mean())
        return out


# ------------------------------------------------------------------------------------------------------------- k-means
def _first_argmax(s):
    """argmax over the columns; a tie goes to the lowest index (``torch.argmax`` promises no order among equals)."""
    K = s.shape[1]
    at = torch.arange(K, device=s.device)[None, :].expand_as(s)
    return torch.where(s == s.amax(1, keepdim=True), at, torch.full_like(at, K)).amin(1)


def _unit_rows(z, fallback=None):
    """Rows over their 2-norm; a row of zeros stays (or becomes the same row of ``fallback``)."""
    norm = z.norm(dim=1, keepdim=True)
    unit = z / torch.where(norm > 0, norm, torch.ones_like(norm))
    return unit if fallback is None else torch.where(norm > 0, unit, fallback)


def _take_rows(rows, idx):
    """Rows ``idx`` of what a :class:`_Rows` walks, through the container's random access -> float64 on its device."""
    idx = torch.as_tensor(idx, dtype=torch.int64).to(rows.device)
    z = rows.latents.take(idx) if rows.latents is not None else rows.rows[idx]
    if not bool(torch.isfinite(z).all()):
        raise ValueError("non-finite values in the rows drawn")
    return z.to(torch.float64)


class _TwinKMeans:
    """One Lloyd walk in float64 torch -- the CPU path of :class:`KMeansProbe` and the oracle of the GPU tests: the
    quantities of ``lla_kmeans_pass`` from the same affine scores, ``_HOST_BLOCK`` rows at a time."""

    def __init__(self, rows, K, cosine):
        self.rows, self.K, self.cosine, self.n_passes = rows, int(K), bool(cosine), 0

    @staticmethod
    def round(centres):
        return centres

    def bias(self, centres):
        return torch.zeros(self.K, dtype=torch.float64) if self.cosine else -0.5 * (centres * centres).sum(1)

    def rows_of(self, z, W, b):
        """-> (a, dist, w, n2) of the rows z [g, C] float64 against the scores z . W_k + b_k."""
        n2 = (z * z).sum(1)
        s = z @ W.T
        if self.cosine:
            w = torch.where(n2 > 0, 1.0 / torch.sqrt(n2), torch.zeros_like(n2))
            s = s * w[:, None] + b
        else:
            w = torch.ones_like(n2)
            s = s + b
        a = _first_argmax(s)
        best = torch.gather(s, 1, a[:, None])[:, 0]
        return a, (1.0 - best if self.cosine else (n2 - 2.0 * best).clamp_min(0.0)), w, n2

    def walk(self, centres, sums):
        """-> (a int64 [N], dist [N], sums [K, C], counts [K], stats [2]); without ``sums`` the last three are None."""
        N, C, K = self.rows.n, self.rows.dim, self.K
        W, b = centres.to(torch.float64), self.bias(centres.to(torch.float64))
        a, dist = torch.empty(N, dtype=torch.int64), torch.empty(N, dtype=torch.float64)
        S, cnt = torch.zeros((K, C), dtype=torch.float64), torch.zeros(K, dtype=torch.float64)
        stats = torch.zeros(2, dtype=torch.float64)
        for g0, zg in self.rows.groups():
            for r0 in range(0, int(zg.shape[0]), _HOST_BLOCK):
                z = zg[r0:r0 + _HOST_BLOCK].to(torch.float64)
                at = slice(g0 + r0, g0 + r0 + int(z.shape[0]))
                a[at], dist[at], w, n2 = self.rows_of(z, W, b)
                if sums:
                    S.index_add_(0, a[at], z * w[:, None])
                    cnt += torch.bincount(a[at], minlength=K).to(torch.float64)
                    stats += torch.stack([dist[at].sum(), n2.sum()])
        self.n_passes += 1
        return (a, dist, S, cnt, stats) if sums else (a, dist, None, None, None)


class _DeviceKMeans:
    """The same walk on the device: every decode group goes through ``lla_kmeans_pass`` (csrc/kmeans.hip), which adds the
    group's sums, counts and statistics to the running totals; scores never reach memory."""

    def __init__(self, rows, K, cosine):
        self.rows, self.K, self.cosine, self.n_passes = rows, int(K), bool(cosine), 0
        L, dev, C, N = _lib.lib(), rows.device, rows.dim, rows.n
        _check_width(C, "k-means")
        nbytes = int(L.lla_kmeans_pass_workspace_bytes(C, self.K))
        if nbytes == 0:
            raise ValueError(f"lla_kmeans_pass refuses C = {C}, K = {K}")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.assign = torch.empty(N, dtype=torch.int32, device=dev)
        self.dist = torch.empty(N, dtype=torch.float32, device=dev)
        self.sum = torch.empty((self.K, C), dtype=torch.float32, device=dev)
        self.count = torch.empty(self.K, dtype=torch.float64, device=dev)
        self.stats = torch.empty(2, dtype=torch.float64, device=dev)

    @staticmethod
    def round(centres):
        return centres.to(torch.float32).to(torch.float64)

    def bias(self, W):
        """b of the fp32 centres W: -1/2 |c_k|^2 in float64, rounded once (cosine: 0)."""
        if self.cosine:
            return torch.zeros(self.K, dtype=torch.float32, device=W.device)
        return (-0.5 * (W.to(torch.float64) ** 2).sum(1)).to(torch.float32)

    def run(self, z, W, b, assign, dist, sums, accumulate):
        """One ``lla_kmeans_pass`` over the rows z [g, C] on the current stream."""
        C, dev = int(W.shape[1]), W.device
        rc = _lib.lib().lla_kmeans_pass(
            *_z_args(z, C), int(z.shape[0]), C, _lib.ptr(W), _lib.ptr(b), self.K, C,
            1 if self.cosine else 0, _lib.ptr(assign), _lib.ptr(dist), _lib.ptr(self.sum if sums else None),
            _lib.ptr(self.count if sums else None), _lib.ptr(self.stats if sums else None), accumulate, _lib.ptr(self.ws),
            _lib.stream_ptr(dev))
        _lib.check(rc, "lla_kmeans_pass")

    def walk(self, centres, sums):
        W = centres.to(torch.float32).contiguous()
        b = self.bias(W)
        with torch.cuda.device(W.device):
            accumulate = 0
            for g0, z in self.rows.groups():
                g = int(z.shape[0])
                self.run(z, W, b, self.assign[g0:g0 + g], self.dist[g0:g0 + g], sums, accumulate)
                accumulate = 1
        self.n_passes += 1
        a, dist = self.assign.to(torch.int64), self.dist.to(torch.float64)
        return (a, dist, self.sum.to(torch.float64), self.count.clone(), self.stats.clone()) if sums else \
            (a, dist, None, None, None)


def _kmeans_init(rows, K, cosine, init, seed, init_size):
    """-> the initial centres, float64 [K, C] on the rows' device, drawn through the container's random access."""
    N = rows.n
    g = torch.Generator().manual_seed(int(seed))
    perm = torch.randperm(N, generator=g)
    if init == "random":
        return _take_rows(rows, perm[:K])
    S = min(N, max(4096, 32 * K)) if init_size is None else int(init_size)
    S = max(min(S, N), K)
    z = _take_rows(rows, perm[:S])
    if cosine:
        z = _unit_rows(z)
    # k-means++ (Arthur & Vassilvitskii 2007): every next centre is drawn with probability proportional to D^2
    u = torch.rand(K, generator=g, dtype=torch.float64)
    n2 = (z * z).sum(1)
    dist_to = lambda at: (n2 - 2.0 * (z @ z[at]) + n2[at]).clamp_min(0.0)                       # noqa: E731
    chosen = [torch.tensor(min(int(float(u[0]) * S), S - 1), device=z.device)]
    d = dist_to(chosen[0])
    u = u.to(z.device)
    for j in range(1, K):
        cum = torch.cumsum(d, 0)
        chosen.append(torch.searchsorted(cum, (u[j] * cum[-1])[None], right=True)[0].clamp(max=S - 1))
        d = torch.minimum(d, dist_to(chosen[-1]))
    return z[torch.stack(chosen)]


def _relocate_empty(S, cnt, a, dist, rows, cosine):
    """Empty clusters, in ascending index, each receive the row with the largest dist not already given away (the lowest
    index on ties; a row that is its cluster's last is passed over), which leaves its own cluster -- scikit-learn's rule."""
    empty = torch.nonzero(cnt == 0)[:, 0].tolist()
    if not empty:
        return S, cnt
    K = int(cnt.numel())
    order = torch.sort(dist, descending=True, stable=True)[1][:len(empty) + K]
    left = cnt.tolist()
    moves = []
    for row, donor in zip(order.tolist(), a[order].tolist()):
        if len(moves) == len(empty):
            break
        if left[donor] > 1:
            left[donor] -= 1
            moves.append((row, donor, empty[len(moves)]))
    if not moves:
        return S, cnt
    z = _take_rows(rows, [m[0] for m in moves])
    if cosine:
        z = _unit_rows(z)
    S, cnt = S.clone(), cnt.clone()
    for j, (_, donor, k) in enumerate(moves):
        S[donor] -= z[j]
        cnt[donor] -= 1
        S[k] = z[j]
        cnt[k] = 1
    return S, cnt


def _lloyd(engine, rows, centres, cosine, max_iter, tol):
    """Lloyd's iterations from ``centres`` with scikit-learn's stopping rules -> dict of the fitted state."""
    N, C = rows.n, rows.dim
    centres = engine.round(_unit_rows(centres) if cosine else centres)
    prev, tol_abs, converged, curve, n_iter = None, None, False, [], 0
    for _ in range(max_iter):
        a, dist, S, cnt, stats = engine.walk(centres, True)
        curve.append(float(stats[0]))
        if tol_abs is None:                      # tol x the mean per-column variance, from the first pass's own totals
            mean = S.sum(0) / N
            second = 1.0 if cosine else float(stats[1]) / N
            tol_abs = tol * max((second - float((mean * mean).sum())) / C, 0.0)
        S, cnt = _relocate_empty(S, cnt, a, dist, rows, cosine)
        new = torch.where(cnt[:, None] > 0, S / cnt.clamp_min(1.0)[:, None], centres)
        new = engine.round(_unit_rows(new, centres) if cosine else new)
        shift = float(((new - centres) ** 2).sum())
        centres = new
        n_iter += 1
        if prev is not None and torch.equal(a, prev):
            converged = True
            break
        if shift <= tol_abs:
            converged = True
            break
        prev = a
    a, dist, _, _, _ = engine.walk(centres, False)
    return dict(centres=centres, labels=a, inertia=float(dist.sum()), n_iter=n_iter, curve=curve, converged=converged)


def _contingency(labels, assigned):
    """-> float64 [classes, clusters] counts of two integer labelings."""
    y = labels.detach().cpu() if isinstance(labels, torch.Tensor) else torch.from_numpy(np.asarray(labels))
    c = assigned.detach().cpu() if isinstance(assigned, torch.Tensor) else torch.from_numpy(np.asarray(assigned))
    y, c = y.reshape(-1), c.reshape(-1)
    if y.is_floating_point() or c.is_floating_point():
        raise TypeError("labels must be integers")
    if y.numel() != c.numel() or y.numel() == 0:
        raise ValueError(f"{y.numel()} labels for {c.numel()} assignments")
    yi, ci = torch.unique(y, return_inverse=True)[1], torch.unique(c, return_inverse=True)[1]
    nb = int(ci.max()) + 1
    return torch.bincount(yi * nb + ci, minlength=(int(yi.max()) + 1) * nb).reshape(-1, nb).to(torch.float64)


class KMeansProbe:
    """``KMeansProbe(n_clusters, metric="euclidean", init="k-means++", n_init=1, max_iter=100, tol=1e-4, seed=0,
    init_size=None)``: Lloyd's k-means on the frozen representations -- the unsupervised protocol (cluster, then score the
    clusters against the labels by NMI / ARI / purity: DeepCluster, SCAN) and the way to build codebooks or pseudo-labels
    from a container that stays compressed.  ``metric="cosine"`` is spherical k-means: rows and centres on the unit sphere.

    ``fit(data, rows_per_pass=65536, keep_rows=False)``
        data    a ``CompressedLatents`` / ``HyperpriorLatents``, an ``[N, C]`` device tensor (fp32 or fp16) or CPU data.
        Every Lloyd iteration is one walk of the rows, one decode group at a time, through ``lla_kmeans_pass``
        (csrc/kmeans.hip): assignment, per-cluster sums and counts and the inertia in one pass whose scores never leave the
        chip.  The centres are the sums over the counts in float64, rounded to fp32; an empty cluster receives the row
        farthest from its centre (scikit-learn's rule, made deterministic: ascending cluster index, lowest row on ties).
        Stops when no label changed, or when the squared centre shift is at most ``tol`` times the mean per-column variance
        (scikit-learn's rule), or after ``max_iter`` iterations; one assign-only pass then makes ``labels_`` and ``inertia_``
        those of ``cluster_centers_``.
    ``init``    ``"k-means++"`` (D^2 sampling on a seeded subsample of ``init_size`` rows, default ``min(N, max(4096, 32 K))``),
                ``"random"`` (K distinct rows) or an array ``[K, C]``; the rows are drawn with ``take``.  ``n_init`` restarts
                run seeds ``seed, seed + 1, ...`` one after another and the lowest inertia is kept.

    After ``fit``: ``cluster_centers_`` ``[K, C]`` (fp32 from the device, float64 from the CPU twin), ``labels_`` int64
    ``[N]``, ``inertia_`` (sum of squared distances; cosine: of ``1 - cos``), ``n_iter_``, ``inertia_curve_`` (the inertia
    each iteration's pass saw), ``converged_``, ``n_passes_``.  ``predict(data)`` -> labels; ``transform(data)`` -> distances
    ``[N, K]`` (Euclidean, or ``1 - cos``) on ``lla_gemm_f32``; ``cluster_scores(labels, assigned=None)`` -> ``{"nmi", "ari",
    "purity"}`` of ``assigned`` (default ``labels_``) against ``labels``, NMI with the arithmetic mean as ``sklearn.metrics``.

    Deterministic: the same inputs, seed and ``rows_per_pass`` give the same bits, with ``keep_rows`` or without.  CPU data
    (``device="cpu"`` latents, CPU tensors) run the float64 torch twin of the same algorithm."""

    def __init__(self, n_clusters, metric="euclidean", init="k-means++", n_init=1, max_iter=100, tol=1e-4, seed=0,
                 init_size=None):
        if int(n_clusters) < 1 or int(n_init) < 1 or int(max_iter) < 1 or not tol >= 0:
            raise ValueError("n_clusters, n_init and max_iter must be at least 1 and tol non-negative")
        if metric not in ("euclidean", "cosine"):
            raise ValueError(f"metric must be 'euclidean' or 'cosine', got {metric!r}")
        if isinstance(init, str):
            if init not in ("k-means++", "random"):
                raise ValueError(f"init must be 'k-means++', 'random' or an array [K, C], got {init!r}")
        else:
            init = torch.as_tensor(np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init)).to(torch.float64)
            if init.dim() != 2 or init.shape[0] != int(n_clusters):
                raise ValueError(f"init must be [{int(n_clusters)}, C], got {tuple(init.shape)}")
        if init_size is not None and int(init_size) < 1:
            raise ValueError("init_size must be at least 1")
        self.n_clusters, self.metric, self.init, self.n_init = int(n_clusters), metric, init, int(n_init)
        self.max_iter, self.tol, self.seed, self.init_size = int(max_iter), float(tol), int(seed), init_size
        self.cluster_centers_ = self.labels_ = None
        self._packed = None

    @property
    def _cosine(self):
        return self.metric == "cosine"

    @staticmethod
    def _engine(rows, K, cosine):
        return (_DeviceKMeans if rows.device.type == "cuda" else _TwinKMeans)(rows, K, cosine)

    # ------------------------------------------------------------------ fit
    def fit(self, data, rows_per_pass=65536, keep_rows=False):
        rows = _Rows(data, rows_per_pass, keep_rows)
        K = self.n_clusters
        if K > rows.n:
            raise ValueError(f"n_clusters = {K} for {rows.n} rows")
        if not isinstance(self.init, str) and self.init.shape[1] != rows.dim:
            raise ValueError(f"init must be [{K}, {rows.dim}], got {tuple(self.init.shape)}")
        best = None
        try:
            engine = self._engine(rows, K, self._cosine)
            for r in range(self.n_init):
                if isinstance(self.init, str):
                    centres = _kmeans_init(rows, K, self._cosine, self.init, self.seed + r, self.init_size)
                else:
                    centres = self.init.to(rows.device)
                run = _lloyd(engine, rows, centres, self._cosine, self.max_iter, self.tol)
                if best is None or run["inertia"] < best["inertia"]:
                    best = run
        finally:
            rows.close()
        on_device = rows.device.type == "cuda"
        self.cluster_centers_ = best["centres"].to(torch.float32) if on_device else best["centres"]
        self.labels_, self.inertia_, self.n_iter_ = best["labels"], best["inertia"], best["n_iter"]
        self.inertia_curve_, self.converged_, self.n_passes_ = best["curve"], best["converged"], engine.n_passes
        self._packed = None
        if not self.converged_:
            warnings.warn(f"KMeansProbe stopped short of tol = {self.tol} after {self.max_iter} iterations", RuntimeWarning)
        return self

    # ------------------------------------------------------------------ predict / transform
    def _rows_for(self, data, rows_per_pass):
        if self.cluster_centers_ is None:
            raise RuntimeError("fit first")
        rows = _Rows(data, rows_per_pass, False)
        rows.first_pass = _is_latents(data)
        if rows.dim != self.cluster_centers_.shape[1]:
            rows.close()
            raise ValueError(f"data has {rows.dim} features, the probe was fitted on {self.cluster_centers_.shape[1]}")
        return rows

    def predict(self, data, rows_per_pass=65536):
        rows = self._rows_for(data, rows_per_pass)
        try:
            if rows.n == 0:
                return torch.zeros(0, dtype=torch.int64, device=rows.device)
            engine = self._engine(rows, self.n_clusters, self._cosine)
            return engine.walk(self.cluster_centers_.to(rows.device).to(torch.float64), False)[0]
        finally:
            rows.close()

    def _pack(self, dev):
        """``_pack_affine`` of the centres rounded to fp32, with b = -1/2 |c_k|^2 (cosine: 0), kept per device."""
        if self._packed is None or self._packed[0] != str(dev):
            W = self.cluster_centers_.to(dev).to(torch.float32)
            b = torch.zeros_like(W[:, 0]) if self._cosine else (-0.5 * (W.to(torch.float64) ** 2).sum(1)).to(torch.float32)
            self._packed = (str(dev),) + _pack_affine(W, b, dev)
        return self._packed[1:]

    def transform(self, data, rows_per_pass=65536):
        """Distances to every centre, [N, K]: Euclidean (``sqrt(max(0, |z|^2 - 2 (z . c - 1/2 |c|^2)))``), or ``1 - cos``."""
        rows = self._rows_for(data, rows_per_pass)
        K, C = self.cluster_centers_.shape
        cosine = self._cosine
        try:
            if rows.device.type != "cuda":
                twin = _TwinKMeans(rows, K, cosine)
                W = self.cluster_centers_.to(torch.float64)
                b = twin.bias(W)
                out = []
                for _, z in rows.groups():
                    z = z.to(torch.float64)
                    n2 = (z * z).sum(1, keepdim=True)
                    if cosine:
                        out.append(1.0 - (z @ W.T) * torch.where(n2 > 0, 1.0 / torch.sqrt(n2), torch.zeros_like(n2)))
                    else:
                        out.append(torch.sqrt((n2 - 2.0 * (z @ W.T + b)).clamp_min(0.0)))
                return torch.cat(out) if out else torch.zeros((0, K), dtype=torch.float64)
            dev = rows.device
            w, b, npad = self._pack(dev)
            out = torch.empty((rows.n, npad), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                for g0, z in rows.groups():
                    o = out[g0:g0 + int(z.shape[0])]
                    z = _affine_scores(z, w, b, o)
                    n2 = (z * z).sum(1, keepdim=True)
                    if cosine:
                        o.copy_(1.0 - o * torch.where(n2 > 0, 1.0 / torch.sqrt(n2), torch.zeros_like(n2)))
                    else:
                        o.copy_(torch.sqrt((n2 - 2.0 * o).clamp_min(0.0)))
            return out[:, :K].contiguous()
        finally:
            rows.close()

    # ------------------------------------------------------------------ scores against labels
    def cluster_scores(self, labels, assigned=None):
        """``{"nmi", "ari", "purity"}`` of the clustering ``assigned`` (default: ``labels_``) against ``labels``, from their
        contingency table in float64: NMI = MI / ((H(labels) + H(assigned)) / 2); ARI from the pair counts (Hubert & Arabie
        1985); purity = the share of rows in their cluster's most frequent class."""
        if assigned is None:
            if self.labels_ is None:
                raise RuntimeError("fit first")
            assigned = self.labels_
        n = _contingency(labels, assigned)
        N = n.sum()
        rows, cols = n.sum(1), n.sum(0)
        entropy = lambda m: float(-(m[m > 0] / N * torch.log(m[m > 0] / N)).sum())              # noqa: E731
        h_rows, h_cols = entropy(rows), entropy(cols)
        if n.shape[0] == 1 and n.shape[1] == 1:
            nmi = 1.0
        else:
            outer = rows[:, None] * cols[None, :]
            on = n > 0
            mi = float((n[on] / N * (torch.log(n[on]) + (torch.log(N) - torch.log(outer[on])))).sum())
            nmi = max(mi, 0.0) / max((h_rows + h_cols) / 2.0, float(np.finfo(np.float64).eps))
        squares = float((n * n).sum())
        N = float(N)
        c11 = squares - N
        c01 = float((cols * cols).sum()) - squares
        c10 = float((rows * rows).sum()) - squares
        c00 = N * N - c01 - c10 - squares
        ari = 1.0 if c01 == 0 and c10 == 0 else 2.0 * (c00 * c11 - c01 * c10) / ((c00 + c01) * (c01 + c11) + (c00 + c10) * (c10 + c11))
        return {"nmi": nmi, "ari": ari, "purity": float(n.amax(0).sum()) / N}


# ---------------------------------------------------------------------- ridge regression from one Gram pass
def _ridge_targets(data, labels, n):
    """-> ("classify", class labels int64 [N]) or ("regress", targets float64 [N, T], whether they came as [N])."""
    if labels is not None:
        y = labels.detach().cpu() if isinstance(labels, torch.Tensor) else torch.from_numpy(np.asarray(labels))
        if y.is_floating_point():
            if y.dim() not in (1, 2) or y.shape[0] != n or (y.dim() == 2 and y.shape[1] < 1):
                raise ValueError(f"targets of shape {tuple(y.shape)} for {n} rows: need [N] or [N, T]")
            t = y.to(torch.float64).reshape(n, -1)
            if not bool(torch.isfinite(t).all()):
                raise ValueError("non-finite targets")
            return "regress", t, y.dim() == 1
    return "classify", _labels_of(data, labels, n), False


def _kfolds_of(cv_arg, N):
    """Folds of a regression: an int is scikit-learn's unshuffled ``KFold`` (contiguous in file order, the first ``N % cv``
    folds one row longer); an int array [N] is taken as ``_folds_of`` takes it.  -> (fold id per row int64 [N], fold ids)."""
    if isinstance(cv_arg, (int, np.integer)):
        cv = int(cv_arg)
        if cv < 2 or cv > N:
            raise ValueError(f"cv must be at least 2 and at most the number of rows, got {cv} for {N} rows")
        sizes = torch.full((cv,), N // cv, dtype=torch.int64)
        sizes[:N % cv] += 1
        return torch.repeat_interleave(torch.arange(cv), sizes), list(range(cv))
    fold, ids, _ = _folds_of(cv_arg, torch.zeros(N, dtype=torch.int64), 1)      # (a fold that holds every row is refused there)
    return fold, ids


class _TwinMoments:
    """The second moments of runs of rows in float64 torch -- the CPU path of the ridge probes and the oracle of the GPU
    tests.  Bucket f holds ``gram`` [C, C], ``sum`` [C] and ``cross`` [K or T, C] (class sums, or sum t z^T) of the runs
    added to it, and for regression ``tsum`` / ``tsq`` [T]."""

    def __init__(self, rows, nb, n_cross, regress):
        C = rows.dim
        self.gram = torch.zeros((nb, C, C), dtype=torch.float64)
        self.sum = torch.zeros((nb, C), dtype=torch.float64)
        self.cross = torch.zeros((nb, n_cross, C), dtype=torch.float64)
        self.tsum = torch.zeros((nb, n_cross), dtype=torch.float64)
        self.tsq = torch.zeros((nb, n_cross), dtype=torch.float64)

    def targets(self, t):
        return t

    def add(self, f, z, seg, t):
        """Run z [r, C] into bucket f: ``seg`` int32 [K + 1] are the offsets of its class runs, or ``t`` [r, T] its targets."""
        z = z.to(torch.float64)
        self.gram[f] += z.T @ z
        self.sum[f] += z.sum(0)
        if seg is not None:
            which = torch.repeat_interleave(torch.arange(len(seg) - 1), torch.diff(seg.to(torch.int64)))
            self.cross[f].index_add_(0, which, z)
        else:
            self.cross[f] += t.T @ z
            self.tsum[f] += t.sum(0)
            self.tsq[f] += (t * t).sum(0)

    def result(self):
        return self.gram, self.sum, self.cross, self.tsum, self.tsq


class _DeviceMoments:
    """The same on the device: a run is one ``lla_gram_pass`` (csrc/gram.hip) accumulating into its bucket, plus one
    ``lla_segment_sums`` for its class sums; regression targets go through the Gram pass, rounded to fp32."""

    def __init__(self, rows, nb, n_cross, regress):
        C, dev = rows.dim, rows.device
        _check_width(C, "ridge")
        self.T = n_cross if regress else 0
        nbytes = int(_lib.lib().lla_gram_pass_workspace_bytes(C, self.T))
        if nbytes == 0:
            raise ValueError(f"lla_gram_pass refuses C = {C}, T = {self.T}")
        self.dev, self.C = dev, C
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.gram = torch.zeros((nb, C, C), dtype=torch.float64, device=dev)
        self.sum = torch.zeros((nb, C), dtype=torch.float64, device=dev)
        self.cross = torch.zeros((nb, n_cross, C), dtype=torch.float64, device=dev)
        pad = -(-n_cross // 2) * 2                 # (every bucket's row 16-byte aligned)
        self.tsum = torch.zeros((nb, pad), dtype=torch.float64, device=dev)
        self.tsq = torch.zeros((nb, pad), dtype=torch.float64, device=dev)
        self.n_cross = n_cross

    def targets(self, t):
        return t.to(torch.float32).to(self.dev).contiguous()

    def add(self, f, z, seg, t):
        L, C, r = _lib.lib(), self.C, int(z.shape[0])
        za = _z_args(z, C)
        st = _lib.stream_ptr(self.dev)
        with_t = seg is None
        rc = L.lla_gram_pass(*za, r, C, _lib.ptr(t) if with_t else None, self.T, self.T,
                             _lib.ptr(self.gram[f]), _lib.ptr(self.sum[f]), _lib.ptr(self.cross[f]) if with_t else None,
                             _lib.ptr(self.tsum[f]) if with_t else None, _lib.ptr(self.tsq[f]) if with_t else None, 1,
                             _lib.ptr(self.ws), st)
        _lib.check(rc, "lla_gram_pass")
        if seg is not None:
            rc = L.lla_segment_sums(*za, r, C, ctypes.c_void_p(seg.data_ptr()), int(seg.numel()) - 1,
                                    _lib.ptr(self.cross[f]), 1, st)
            _lib.check(rc, "lla_segment_sums")

    def result(self):
        n = self.n_cross
        return self.gram.cpu(), self.sum.cpu(), self.cross.cpu(), self.tsum[:, :n].cpu(), self.tsq[:, :n].cpu()


class _RidgeWalk:
    """What the ridge probes walk: the rows sorted inside every decode group by (bucket, class), so that a bucket -- a
    held-out fold, or the rows no fold holds -- is one contiguous run of every group, and its classes are runs of that run.
    ``runs(g0, g)`` yields (bucket, first, last + 1 within the group, class offsets int32 [K + 1] or None)."""

    def __init__(self, rows, bucket, nb, cls, K):
        self.nb, self.K = int(nb), int(K)
        N, G = rows.n, rows.group
        group = torch.arange(N, dtype=torch.int64) // G
        key = bucket if cls is None else bucket * self.K + cls
        self.sorted = cls is not None or nb > 1
        self.order = torch.argsort(group * (self.nb * self.K) + key, stable=True) if self.sorted else None
        self.key = key[self.order] if self.sorted else key
        self.with_classes = cls is not None
        if self.sorted:
            rows.order = self.order.to(rows.device)

    def take(self, x):
        return x[self.order] if self.sorted else x

    def runs(self, g0, g):
        cnt = torch.bincount(self.key[g0:g0 + g], minlength=self.nb * self.K).reshape(self.nb, self.K)
        first = 0
        for f in range(self.nb):
            r = int(cnt[f].sum())
            if r:
                seg = None
                if self.with_classes:
                    seg = torch.zeros(self.K + 1, dtype=torch.int32)
                    seg[1:] = torch.cumsum(cnt[f], 0)
                yield f, first, first + r, seg
            first += r


def _ridge_moments(rows, walk, t):
    """One walk of the rows -> per bucket (gram [C, C], sum [C], cross [K or T, C], tsum [T], tsq [T]) float64 on the CPU."""
    regress = t is not None
    Engine = _DeviceMoments if rows.device.type == "cuda" else _TwinMoments
    engine = Engine(rows, walk.nb, t.shape[1] if regress else walk.K, regress)
    tp = engine.targets(walk.take(t)) if regress else None
    with torch.cuda.device(rows.device) if rows.device.type == "cuda" else contextlib.nullcontext():
        for g0, z in rows.groups():
            for f, a, b, seg in walk.runs(g0, int(z.shape[0])):
                engine.add(f, z[a:b], seg, tp[g0 + a:g0 + b] if regress else None)
        return engine.result()


def _signed_targets(n, s, class_sums, counts):
    """The cross-moments of the +1 / -1 targets of ``RidgeClassifier`` from the class sums: ``Z^T Y`` with
    ``Y = 2 onehot - 1`` is ``2 R_classsum - s``; two classes are the one column of ``classes_[1]``.
    -> (R [K or 1, C], ts [K or 1])."""
    R, ts = 2.0 * class_sums - s[None, :], 2.0 * counts - n
    return (R[1:2], ts[1:2]) if R.shape[0] == 2 else (R, ts)


def _ridge_solve(n, G, s, R, ts, alphas, fit_intercept=True):
    """``min |T - Z W^T - b|^2 + alpha |W|^2`` (the intercept not penalised) for every alpha, from the moments of the rows
    in float64: n, G = sum z z^T [C, C], s = sum z [C], R = sum t z^T [T, C], ts = sum t [T].  One ``eigh`` of the centred
    Gram matrix serves all alphas: ``W = (Rc V) / (lam + alpha) V^T``, ``b = mt - W mu``.  -> (W [A, T, C], b [A, T])."""
    G, s, R, ts = (x.to(torch.float64) for x in (G, s, R, ts))
    n = float(n)
    if fit_intercept:
        mu, mt = s / n, ts / n
        G = G - n * torch.outer(mu, mu)
        R = R - n * torch.outer(mt, mu)
    lam, V = torch.linalg.eigh((G + G.T) / 2)
    lam = lam.clamp_min(0.0)
    RV = R @ V
    Ws, bs = [], []
    for alpha in alphas:
        d = lam + float(alpha)
        W = (RV * torch.where(d > 0, 1.0 / d, torch.zeros_like(d))[None, :]) @ V.T
        Ws.append(W)
        bs.append(mt - W @ mu if fit_intercept else torch.zeros_like(ts))
    return torch.stack(Ws), torch.stack(bs)


def _check_alpha(alpha):
    alpha = float(alpha)
    if not alpha >= 0 or not np.isfinite(alpha):
        raise ValueError(f"alpha must be finite and non-negative, got {alpha}")
    return alpha


class RidgeProbe(_Scores):
    """``RidgeProbe(alpha=1.0, fit_intercept=True)``: scikit-learn's ``Ridge`` / ``RidgeClassifier`` on the frozen
    representations, ``min |T - Z W^T - b|^2 + alpha |W|^2`` with the intercept not penalised, from ONE walk of the rows.
    The walk accumulates the rows' second moments (``lla_gram_pass`` / ``lla_segment_sums``, csrc/gram.hip: fp32 MFMA chains
    joined in double); the solve is one float64 ``eigh`` of the centred C x C Gram matrix on the host.

    ``fit(data, labels=None, rows_per_pass=65536, keep_rows=False)`` takes what ``LinearProbe.fit`` takes.  Integer labels
    mean classification: targets +1 / -1 per class, two classes solved as the one column of ``classes_[1]``, ``classes_``
    set.  Floating labels ``[N]`` or ``[N, T]`` mean regression (on the device they are rounded to fp32).  CPU data run the
    float64 twin of the same moments and the same solve.  Sample weights and ``class_weight`` are not built.

    After ``fit``: ``coef_`` float64 ``[K, C]`` (``[1, C]`` for two classes, ``[T, C]`` for regression) and ``intercept_``
    on the CPU, ``moments_`` (the float64 statistics: ``n``, ``gram``, ``sum``, ``cross`` -- class sums or ``sum t z^T`` --
    ``tsum`` -- class counts or ``sum t`` -- and ``tsq``), ``n_passes_ = 1``.  ``path(alphas)`` returns fitted probes for
    other alphas from ``moments_`` with no data pass.  ``decision_function`` / ``predict`` run on ``lla_gemm_f32`` (fp32) on
    the device and in float64 on the CPU; ``score`` is the accuracy, or scikit-learn's R^2 (uniform average over targets)."""

    def __init__(self, alpha=1.0, fit_intercept=True):
        self.alpha, self.fit_intercept = _check_alpha(alpha), bool(fit_intercept)
        self.coef_ = self.intercept_ = self.classes_ = self.moments_ = None

    def fit(self, data, labels=None, rows_per_pass=65536, keep_rows=False):
        rows = _Rows(data, rows_per_pass, keep_rows)
        try:
            self.moments_ = _fit_moments(rows, data, labels, None)[0]
        finally:
            rows.close()
        return self._solve()

    def _solve(self):
        m = self.moments_
        R, ts = _signed_targets(m["n"], m["sum"], m["cross"], m["tsum"]) if m["kind"] == "classify" else (m["cross"], m["tsum"])
        W, b = _ridge_solve(m["n"], m["gram"], m["sum"], R, ts, [self.alpha], self.fit_intercept)
        self.coef_, self.intercept_ = W[0], b[0]
        self.classes_ = m["classes"]
        self.n_passes_, self._packed = 1, None
        return self

    def path(self, alphas):
        """Fitted probes for ``alphas`` from ``moments_``: no pass over the data."""
        if self.moments_ is None:
            raise RuntimeError("fit first")
        out = []
        for alpha in alphas:
            probe = RidgeProbe(alpha, self.fit_intercept)
            probe.moments_ = self.moments_
            out.append(probe._solve())
        return out

    def decision_function(self, data, rows_per_pass=65536):
        s = self._scores(data, rows_per_pass)
        m = self.moments_
        one = len(self.classes_) == 2 if m["kind"] == "classify" else m["squeeze"]
        return s[:, 0].contiguous() if one else s.contiguous()

    def predict(self, data, rows_per_pass=65536):
        if self.coef_ is not None and self.moments_["kind"] == "regress":
            return self.decision_function(data, rows_per_pass)
        return super().predict(data, rows_per_pass)

    def score(self, data, labels=None, rows_per_pass=65536):
        if self.coef_ is None or self.moments_["kind"] == "classify":
            return super().score(data, labels, rows_per_pass)
        pred = self.predict(data, rows_per_pass).to(torch.float64)
        pred = pred.reshape(pred.shape[0], -1)
        kind, t, _ = _ridge_targets(data, labels, pred.shape[0])
        if kind != "regress" or t.shape[1] != pred.shape[1]:
            raise ValueError(f"a regression probe with {pred.shape[1]} targets needs floating targets of that shape")
        t = t.to(pred.device)
        res, tot = ((t - pred) ** 2).sum(0), ((t - t.mean(0)) ** 2).sum(0)
        return float((1.0 - res / tot).mean())


def _fit_moments(rows, data, labels, cv):
    """The walk of a ridge fit: -> (total moments dict, per-fold held-out moments, walk, targets' bookkeeping).  ``cv`` None:
    nothing is held out (one bucket)."""
    if rows.n < 1:
        raise ValueError("no rows")
    kind, y, squeeze = _ridge_targets(data, labels, rows.n)
    classes = cls = None
    if kind == "classify":
        classes = torch.unique(y)
        if classes.numel() < 2:
            raise ValueError("a ridge classifier needs at least two classes")
        cls = torch.searchsorted(classes, y)
    K = int(classes.numel()) if classes is not None else 1
    if cv is None:
        fold, ids = torch.full((rows.n,), -1, dtype=torch.int64), []
    elif kind == "classify":
        fold, ids, _ = _folds_of(cv, cls, K)
    else:
        fold, ids = _kfolds_of(cv, rows.n)
    nf = len(ids)
    bucket = torch.full((rows.n,), nf, dtype=torch.int64)             # rows no fold holds: the last bucket
    for i, f in enumerate(ids):
        bucket[fold == f] = i
    walk = _RidgeWalk(rows, bucket, nf + 1, cls, K)
    gram, s, cross, tsum, tsq = _ridge_moments(rows, walk, y if kind == "regress" else None)
    n = torch.bincount(bucket, minlength=nf + 1).to(torch.float64)
    if kind == "classify":                                           # class counts and sum y^2, exactly, from the labels
        tsum = torch.bincount(bucket * K + cls, minlength=(nf + 1) * K).reshape(nf + 1, K).to(torch.float64)
        tsq = n[:, None].expand(nf + 1, K).clone()
    extra = dict(kind=kind, classes=classes.numpy() if classes is not None else None, squeeze=squeeze)
    parts = [dict(n=float(n[f]), gram=gram[f], sum=s[f], cross=cross[f], tsum=tsum[f], tsq=tsq[f], **extra)
             for f in range(nf + 1)]
    total = dict(n=float(n.sum()), gram=gram.sum(0), sum=s.sum(0), cross=cross.sum(0), tsum=tsum.sum(0), tsq=tsq.sum(0), **extra)
    return total, parts[:nf], walk, (fold, ids, cls)


def _ridge_fold_fits(total, held, alphas, fit_intercept):
    """Every (fold, alpha) of a search from the moments: fold f trains on ``total - held[f]``, one ``eigh`` per fold.
    -> (W [folds, A, T, C], b [folds, A, T])."""
    classify = total["kind"] == "classify"
    Ws, bs = [], []
    for h in held:
        train = {k: total[k] - h[k] for k in ("n", "gram", "sum", "cross", "tsum")}
        R, ts = _signed_targets(train["n"], train["sum"], train["cross"], train["tsum"]) if classify else \
            (train["cross"], train["tsum"])
        W, b = _ridge_solve(train["n"], train["gram"], train["sum"], R, ts, alphas, fit_intercept)
        Ws.append(W)
        bs.append(b)
    return torch.stack(Ws), torch.stack(bs)


def _ridge_held_out_mse(held, W, b):
    """The held-out mean squared error of every (alpha, fold) from the fold's own moments, no data pass:
    ``SSE_f = tt_f - 2 <W, R_f> - 2 b . ts_f + <W G_f, W> + 2 (W s_f) . b + n_f |b|^2``, over ``n_f T``.  -> [A, folds]."""
    mse = torch.empty((W.shape[1], len(held)), dtype=torch.float64)
    for f, h in enumerate(held):
        Wf, bf = W[f], b[f]                                       # [A, T, C], [A, T]
        sse = h["tsq"][None] - 2 * (Wf * h["cross"][None]).sum(2) - 2 * bf * h["tsum"][None] \
            + ((Wf @ h["gram"]) * Wf).sum(2) + 2 * (Wf @ h["sum"]) * bf + h["n"] * bf * bf
        mse[:, f] = sse.sum(1) / (h["n"] * Wf.shape[1])
    return mse


class RidgeProbeCV:
    """``RidgeProbeCV(alphas, cv=5, fit_intercept=True)``: the K-fold search over ``alpha`` of a :class:`RidgeProbe` from
    the moments of ONE walk.  The moments add over rows, so the walk keeps them per fold, a fold's training moments are the
    total minus its own, one ``eigh`` per fold serves every alpha, and ``best_estimator_`` is solved from the total.

    Walks of the data: classification 2 (the moments, then one walk that scores every fold's rows against that fold's
    ``len(alphas)`` classifiers on ``lla_gemm_f32``); regression 1 (the held-out squared error is a closed form of the
    fold's own moments: ``SSE_f = tt_f - 2 <W, R_f> - 2 b . ts_f + <W G_f, W> + 2 (W s_f) . b + n_f |b|^2``).

    cv      an int: stratified and unshuffled as ``LinearProbeCV`` for classification, scikit-learn's unshuffled ``KFold``
            (contiguous in file order) for regression; or an int array ``[N]`` of fold ids (-1: always trains).
    Inside every decode group the rows are fetched in (fold, class) order (``take`` / ``index_select``), so each fold is one
    run per group: one ``lla_gram_pass`` and, for class labels, one ``lla_segment_sums``.

    ``fit(data, labels=None, rows_per_pass=65536, keep_rows=False)``; afterwards ``cv_scores_`` float64
    ``[len(alphas), folds]`` (accuracy, or negative mean squared error), ``mean_scores_``, ``best_index_`` (the LOWEST alpha
    among the best means), ``best_params_``, ``best_estimator_`` (a fitted ``RidgeProbe``, no further pass), ``folds_``,
    ``fold_coef_`` / ``fold_intercept_`` float64 ``[len(alphas), folds, K or T, C]``, ``fold_moments_`` (every fold's own
    moments, as ``RidgeProbe.moments_``), ``classes_``, ``n_passes_``.  Sample weights and ``class_weight`` are not built."""

    def __init__(self, alphas, cv=5, fit_intercept=True):
        self.alphas = [_check_alpha(a) for a in alphas]
        if not self.alphas:
            raise ValueError("no alphas")
        self.cv, self.fit_intercept = cv, bool(fit_intercept)
        self.cv_scores_ = self.best_estimator_ = None

    @staticmethod
    def logspace(n, low, high):
        """n alphas spaced evenly on a log scale from ``low`` to ``high``."""
        if not 0 < low <= high or int(n) < 1:
            raise ValueError("need 0 < low <= high and n >= 1")
        return [float(a) for a in np.exp(np.linspace(np.log(low), np.log(high), int(n))).clip(low, high)]

    def fit(self, data, labels=None, rows_per_pass=65536, keep_rows=False):
        rows = _Rows(data, rows_per_pass, keep_rows)
        A = len(self.alphas)
        try:
            total, held, walk, (fold, ids, cls) = _fit_moments(rows, data, labels, self.cv)
            classify = total["kind"] == "classify"
            W, b = _ridge_fold_fits(total, held, self.alphas, self.fit_intercept)
            self.n_passes_ = 1
            if classify:
                right = self._score(rows, walk, W, b, walk.take(cls))
                self.n_passes_ = 2
                n_held = torch.tensor([h["n"] for h in held], dtype=torch.float64)
                self.cv_scores_ = right.T.double() / n_held[None, :]
            else:
                self.cv_scores_ = -_ridge_held_out_mse(held, W, b)
        finally:
            rows.close()
        self.mean_scores_ = self.cv_scores_.mean(1)
        best = [i for i in range(A) if float(self.mean_scores_[i]) == float(self.mean_scores_.max())]
        self.best_index_ = min(best, key=lambda i: self.alphas[i])                 # the lowest alpha on ties
        self.best_params_ = {"alpha": self.alphas[self.best_index_]}
        self.fold_coef_, self.fold_intercept_ = W.transpose(0, 1).contiguous(), b.transpose(0, 1).contiguous()
        self.classes_, self.folds_, self.fold_moments_ = total["classes"], list(ids), held
        probe = RidgeProbe(self.best_params_["alpha"], self.fit_intercept)
        probe.moments_ = total
        self.best_estimator_ = probe._solve()
        return self

    @staticmethod
    def _score(rows, walk, W, b, cls):
        """The scoring walk: the run of fold f in every group against fold f's classifiers (``lla_gemm_f32`` on the device,
        float64 on the CPU) -> matches int64 [folds, A] on the CPU."""
        nf, A, Kp, C = W.shape
        dev = rows.device
        right = torch.zeros((nf, A), dtype=torch.int64, device=dev)
        cls = cls.to(dev)

        def count(S, f, r0):
            S = S.reshape(S.shape[0], A, Kp)
            pred = (S[:, :, 0] > 0).to(torch.int64) if Kp == 1 else S.argmax(2)
            right[f] += (pred == cls[r0:r0 + S.shape[0], None]).sum(0)

        if dev.type == "cuda":
            J = A * Kp
            w, bp, npad = _pack_affine(W.reshape(nf, J, C), b.reshape(nf, J), dev)
            piece = _piece_rows(npad, rows.group)
            out = torch.empty((min(piece, rows.n), npad), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                for g0, z in rows.groups():
                    z = _f32_rows(z, C)[0]                 # (fp16 rows: widened once per group, not once per run)
                    for f, a0, a1, _ in walk.runs(g0, int(z.shape[0])):
                        if f < nf:
                            _affine_scores(z[a0:a1], w[f], bp[f], out, piece, lambda r0, S: count(S[:, :J], f, g0 + a0 + r0))
        else:
            for g0, z in rows.groups():
                z = z.to(torch.float64)
                for f, a0, a1, _ in walk.runs(g0, int(z.shape[0])):
                    if f < nf:
                        count(z[a0:a1] @ W[f].reshape(A * Kp, C).T + b[f].reshape(-1), f, g0 + a0)
        return right.cpu()


# ------------------------------------------------------------------------------------------------------------- zero-shot
class ZeroShotProbe(_Scores):
    """``ZeroShotProbe(class_embeddings [K, E], logit_scale=None, classes=None)``: CLIP's zero-shot classifier over coded
    features -- no training rows, no ``fit``.  The logit of row i for class k is

        logit_scale * (z_i / |z_i|) . w_k

    with ``w_k`` the class embeddings as given (:meth:`from_tokens` makes them with a text tower's ``encode_classes``:
    unit-norm prompt ensembles) and ``logit_scale`` 100 unless given (CLIP's trained ``exp(logit_scale)``).  A row of zeros
    gives zero logits.

    ``decision_function`` ``[N, K]``, ``predict``, ``predict_proba`` (softmax of the logits), ``score(X, y=None)`` and
    ``top_k_score(X, k, y=None)`` take a ``CompressedLatents`` / ``HyperpriorLatents`` (its own labels unless ``y`` is
    given), a tensor or an ndarray, and score one decode group at a time with the walk of the other probes' ``predict``:
    ``lla_unit_rows`` (the row norm in a fixed order), then ``lla_gemm_f32``, fp32 -- the same bits for a container, its
    kept rows and the decoded tensor.  CPU data run the float64 twin.  ``coef_`` fp32 ``[K, E]``, ``intercept_`` zeros,
    ``classes_`` (numpy; ``arange(K)`` unless given)."""

    def __init__(self, class_embeddings, logit_scale=None, classes=None):
        W = class_embeddings.detach().cpu() if isinstance(class_embeddings, torch.Tensor) else \
            torch.from_numpy(np.asarray(class_embeddings))
        if W.dim() != 2 or not W.is_floating_point() or not bool(torch.isfinite(W).all()):
            raise ValueError("class_embeddings must be finite floats [K, E]")
        K = int(W.shape[0])
        classes = torch.arange(K) if classes is None else torch.from_numpy(np.asarray(classes)).reshape(-1)
        if classes.numel() != K:
            raise ValueError(f"{classes.numel()} classes for {K} class embeddings")
        self.logit_scale = 100.0 if logit_scale is None else float(logit_scale)
        if not self.logit_scale > 0:
            raise ValueError("logit_scale must be positive")
        self._set(W, torch.zeros(K), classes, 0, None, True)

    @classmethod
    def from_tokens(cls, text_tower, tokens, classes=None, logit_scale=None):
        """Class embeddings from ``text_tower.encode_classes(tokens [K, n_templates, T])``; ``logit_scale`` defaults to the
        ``exp(logit_scale)`` of the tower's state dict when it holds one, otherwise 100."""
        if logit_scale is None:
            logit_scale = text_tower.logit_scale
        return cls(text_tower.encode_classes(tokens), logit_scale, classes)

    @staticmethod
    def _rows_in(z):
        from .clip_text import unit_rows
        return unit_rows(z)

    def decision_function(self, data, rows_per_pass=65536):
        return (self._scores(data, rows_per_pass) * self.logit_scale).contiguous()

    def predict(self, data, rows_per_pass=65536):
        s = self.decision_function(data, rows_per_pass)
        return torch.from_numpy(self.classes_).to(s.device)[_first_argmax(s)]

    def predict_proba(self, data, rows_per_pass=65536):
        return torch.softmax(self.decision_function(data, rows_per_pass), 1)

    def score(self, data, y=None, rows_per_pass=65536):
        return self.top_k_score(data, 1, y, rows_per_pass)

    def top_k_score(self, data, k, y=None, rows_per_pass=65536):
        """The share of rows whose label is among the ``k`` classes of largest logit (ties go to the lower index)."""
        s = self.decision_function(data, rows_per_pass)
        K = int(s.shape[1])
        if not 1 <= int(k) <= K:
            raise ValueError(f"k = {k} outside [1, {K}]")
        y = _labels_of(data, y, int(s.shape[0])).to(s.device)
        cls = torch.from_numpy(self.classes_).to(s.device)
        own = (y[:, None] == cls[None, :])
        if not bool(own.any(1).all()):
            raise ValueError("labels outside classes_")
        mine = (s * own).sum(1, keepdim=True)                      # the logit of the row's own class
        at = torch.arange(K, device=s.device)[None, :]
        ahead = ((s > mine) | ((s == mine) & (at < own.to(torch.int64).argmax(1, keepdim=True)))).sum(1)
        return float((ahead < int(k)).double().mean()) if s.shape[0] else float("nan")
