"""``LinearProbe`` -- the downstream linear classifier, trained from the compressed copy on the device.

The reference's published workflow ends with ``LinearSVC(C=7e-3).fit(Z, Y)`` on the decompressed features (README.md:74-82
of the reference, notebooks/Hub.ipynb:415): scikit-learn's single-threaded liblinear over a host float32 array, which its
README notes does not reach ImageNet.  This class solves the same objective -- squared hinge, L2 penalty, one-vs-rest, the
intercept carried as one more feature of value 1 and regularised with the weights --

    f_k(w, b) = 1/2 (|w|^2 + b^2) + C sum_i max(0, 1 - y_ik (w . z_i + b))^2

for all classes at once, from a :class:`~lossyless_amd.latents.CompressedLatents` / ``HyperpriorLatents`` that stays
compressed in HBM: a pass walks the rows in file order, one decode group at a time (``take`` into one reused buffer), and
hands each group to ``lla_svm_pass`` (csrc/probe.hip), which adds that group's share of the loss, the gradient or a
generalised-Hessian-vector product to the running totals.  No N x K state lives between passes.

The solver is a truncated Newton-CG (Jacobi-preconditioned by the data's column scales), batched over the classes (every class is its own strongly convex problem; all of
them advance in the same pass), with a per-class backtracking line search.  It is deterministic.

CPU data (or latents opened with ``device="cpu"``) run the same solver over a float64 torch evaluation of the same two
quantities: no GPU needed, and the oracle of the GPU tests.
"""
import warnings

import numpy as np
import torch

from . import _lib
from .latents import _Latents

_CG_TOL = 0.1            # inner solve: |H d + g|_2 <= 0.1 |g|_2 per class (liblinear's TRON uses the same fraction)
_CG_MAX = 100
_ARMIJO = 1e-4
_BACKTRACKS = 30


def _is_latents(data):
    return isinstance(data, _Latents)


class _Rows:
    """The rows of a fit / predict call, walked in file order in groups: ``groups()`` yields (first row, rows [g, C])."""

    def __init__(self, data, rows_per_pass, keep_rows):
        self.group = max(int(rows_per_pass), 1)
        self.kept = None
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
                z = self.rows[g0:g0 + g]
            else:
                idx = torch.arange(g0, g0 + g, device=self.device)
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


class _HostSums:
    """float64 torch evaluation of the two quantities ``lla_svm_pass`` computes (the CPU path; the GPU tests' oracle)."""
    dtype = torch.float64
    slack = 1e-14

    def __init__(self, rows, y, K):
        self.rows, self.y, self.K = rows, y, K
        self.n_passes = 0

    def _signs(self, g0, g):
        return torch.where(self.y[g0:g0 + g, None] == torch.arange(self.K)[None, :], 1.0, -1.0).to(torch.float64)

    def column_squares(self):
        sq = torch.zeros(self.rows.dim, dtype=torch.float64)
        for _, z in self.rows.groups():
            sq += (z.to(torch.float64) ** 2).sum(0)
        self.n_passes += 1
        return sq

    def gradient(self, W, b):
        loss, gW, gb = torch.zeros(self.K, dtype=torch.float64), torch.zeros_like(W), torch.zeros_like(b)
        for g0, z in self.rows.groups():
            z = z.to(torch.float64)
            ys = self._signs(g0, z.shape[0])
            m = (1.0 - ys * (z @ W.T + b)).clamp_min(0.0)
            r = -2.0 * ys * m
            loss += (m * m).sum(0)
            gW += r.T @ z
            gb += r.sum(0)
        self.n_passes += 1
        return loss, gW, gb

    def hessian_vector(self, W, b, V, vb):
        hW, hb = torch.zeros_like(W), torch.zeros_like(b)
        for g0, z in self.rows.groups():
            z = z.to(torch.float64)
            ys = self._signs(g0, z.shape[0])
            active = (1.0 - ys * (z @ W.T + b)) > 0
            t = 2.0 * torch.where(active, z @ V.T + vb, torch.zeros((), dtype=torch.float64))
            hW += t.T @ z
            hb += t.sum(0)
        self.n_passes += 1
        return hW, hb


class _DeviceSums:
    """The same two quantities from ``lla_svm_pass``, one call per decode group, accumulated on the device."""
    dtype = torch.float32
    slack = 1e-6          # Armijo slack, relative to f: the fp32 loss sums of two passes differ by rounding at this level

    def __init__(self, rows, y, K):
        C, dev = rows.dim, rows.device
        if C % 8 or not 8 <= C <= 1024:
            raise ValueError(f"the device probe needs a feature width that is a multiple of 8 in [8, 1024], got {C}")
        self.rows, self.K, self.C, self.device = rows, K, C, dev
        self.y = y.to(torch.int32).to(dev).contiguous()
        self.L = _lib.lib()
        nbytes = int(self.L.lla_svm_pass_workspace_bytes(C, K))
        if nbytes == 0:
            raise ValueError(f"lla_svm_pass refuses C = {C}, K = {K}")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.n_passes = 0

    def _pass(self, W, b, V, vb):
        K, C = self.K, self.C
        oW = torch.zeros((K, C), dtype=torch.float32, device=self.device)
        ob = torch.zeros(K, dtype=torch.float32, device=self.device)
        loss = torch.zeros(K, dtype=torch.float64, device=self.device) if V is None else None
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            for g0, z in self.rows.groups():
                g = int(z.shape[0])
                zt = _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32
                rc = self.L.lla_svm_pass(_lib.ptr(z), zt, int(z.stride(0)) if g > 1 else C, _lib.ptr(self.y[g0:g0 + g]), g, C,
                                         _lib.ptr(W), _lib.ptr(b), _lib.ptr(V), _lib.ptr(vb), K, C, _lib.ptr(oW),
                                         _lib.ptr(ob), _lib.ptr(loss), 1, _lib.ptr(self.ws), st)
                _lib.check(rc, "lla_svm_pass")
        self.n_passes += 1
        return loss, oW, ob

    def column_squares(self):
        sq = torch.zeros(self.C, dtype=torch.float64, device=self.device)
        for _, z in self.rows.groups():
            sq += (z.float() ** 2).sum(0, dtype=torch.float64)
        self.n_passes += 1
        return sq

    def gradient(self, W, b):
        return self._pass(W.contiguous(), b.contiguous(), None, None)

    def hessian_vector(self, W, b, V, vb):
        return self._pass(W.contiguous(), b.contiguous(), V.contiguous(), vb.contiguous())[1:]


def _newton_cg(sums, K, dim, n_rows, device, Cw, tol, max_iter):
    """Batched truncated Newton-CG on f_k = 1/2 (|w|^2 + b^2) + Cw loss_k -> (W, b, f [K] float64, converged).
    One host synchronisation per CG iteration and per line-search step."""
    dt = sums.dtype
    W, b = torch.zeros((K, dim), dtype=dt, device=device), torch.zeros(K, dtype=dt, device=device)

    def evaluate(W, b):
        loss, gW, gb = sums.gradient(W, b)
        f = 0.5 * ((W.double() ** 2).sum(1) + b.double() ** 2) + Cw * loss
        return f, W + Cw * gW, b + Cw * gb

    def sup(gW, gb):          # per-class sup norm of the gradient
        return torch.maximum(gW.abs().amax(1), gb.abs())

    # Jacobi preconditioner from the column scales of the data: 1 + 2 Cw sum_i z_ic^2 bounds the Hessian's diagonal for
    # every class and every active set (the intercept's column is all ones), so one vector serves the whole solve
    mW = (1.0 + 2.0 * Cw * sums.column_squares()).to(dt)[None, :]
    mb = 1.0 + 2.0 * Cw * n_rows
    f, gW, gb = evaluate(W, b)
    g0 = float(sup(gW, gb).max())
    for _ in range(int(max_iter)):
        live = sup(gW, gb) > tol * g0    # classes still short of the stopping rule; the others stay where they are
        if not bool(live.any()):
            break
        lv = live.to(dt)
        # preconditioned CG on H d = -g, H v = v + Cw (generalised Hessian sums)(v), all classes in one pass
        dW, db = torch.zeros_like(W), torch.zeros_like(b)
        rW, rb = -gW * lv[:, None], -gb * lv
        yW, yb = rW / mW, rb / mb
        pW, pb = yW.clone(), yb.clone()
        rs = (rW * yW).sum(1) + rb * yb
        stop = _CG_TOL ** 2 * rs
        for _cg in range(_CG_MAX):
            hW, hb = sums.hessian_vector(W, b, pW, pb)
            hW, hb = pW + Cw * hW, pb + Cw * hb
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
        # per-class backtracking: a class keeps its step length once the Armijo condition holds for it
        gd = ((gW * dW).sum(1) + gb * db).double()
        t = torch.ones(K, dtype=dt, device=device)
        for _ls in range(_BACKTRACKS):
            W2, b2 = W + t[:, None] * dW, b + t * db
            f2, gW2, gb2 = evaluate(W2, b2)
            ok = f2 <= f + _ARMIJO * t.double() * gd + sums.slack * f.abs()
            if bool(ok.all()):
                break
            t = torch.where(ok, t, t * 0.5)
        else:                            # classes whose step never passed stay where they were
            t = torch.where(ok, t, torch.zeros_like(t))
            W2, b2 = W + t[:, None] * dW, b + t * db
            f2, gW2, gb2 = evaluate(W2, b2)
        W, b, f, gW, gb = W2, b2, f2, gW2, gb2
        if not bool((t > 0).any()):      # nothing moved: rounding has the last word
            break
    converged = bool((sup(gW, gb) <= tol * g0).all())
    return W, b, f, converged


class LinearProbe:
    """``LinearProbe(C=7e-3, tol=1e-4, max_iter=100)``: scikit-learn's ``LinearSVC(C)`` objective (its defaults: squared
    hinge, L2, one-vs-rest, regularised intercept), solved where the data lives.

    ``fit(data, labels=None, rows_per_pass=65536, keep_rows=False)``
        data    a ``CompressedLatents`` / ``HyperpriorLatents`` (its own labels unless ``labels`` is given), or a
                ``[N, C]`` tensor / array together with ``labels``.
        rows_per_pass   rows decoded (``take``) and handed to ``lla_svm_pass`` at a time; statuses are checked on the
                first pass only.
        keep_rows       decode once and keep the fp32 rows (N x C x 4 bytes) instead of decoding every pass.
    Stops when ``|grad f|_inf <= tol |grad f(0)|_inf``; warns and sets ``converged_ = False`` at ``max_iter`` Newton steps.

    After ``fit``: ``coef_`` fp32 ``[K, C]`` (``[1, C]`` for two classes, positive class ``classes_[1]``), ``intercept_``,
    ``classes_`` (sorted unique labels, numpy), ``n_passes_`` (passes over the data), ``objective_`` (sum of f_k),
    ``converged_``.  ``decision_function`` returns ``[N, K]`` (``[N]`` for two classes), fp32 from ``lla_gemm_f32`` on the
    device and float64 on the CPU; ``predict`` returns labels, ``score`` the mean accuracy."""

    def __init__(self, C=7e-3, tol=1e-4, max_iter=100):
        if not C > 0 or not tol > 0 or int(max_iter) < 1:
            raise ValueError("C and tol must be positive, max_iter at least 1")
        self.C, self.tol, self.max_iter = float(C), float(tol), int(max_iter)
        self.coef_ = self.intercept_ = self.classes_ = None

    # ------------------------------------------------------------------ labels
    @staticmethod
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

    # ------------------------------------------------------------------ fit
    def fit(self, data, labels=None, rows_per_pass=65536, keep_rows=False):
        rows = _Rows(data, rows_per_pass, keep_rows)
        y = self._labels_of(data, labels, rows.n)
        classes = torch.unique(y)           # sorted
        if classes.numel() < 2:
            raise ValueError("LinearProbe needs at least two classes")
        idx = torch.searchsorted(classes, y)
        if classes.numel() == 2:            # one classifier; label 0 = the positive class, classes_[1]
            K, idx = 1, 1 - idx
        else:
            K = int(classes.numel())
        try:
            if rows.device.type == "cuda":
                sums = _DeviceSums(rows, idx, K)
            else:
                sums = _HostSums(rows, idx, K)
            W, b, f, converged = _newton_cg(sums, K, rows.dim, rows.n, rows.device, self.C, self.tol, self.max_iter)
        finally:
            rows.close()
        self.coef_, self.intercept_ = W.to(torch.float32), b.to(torch.float32)
        self.classes_ = classes.numpy()
        self.n_passes_, self.objective_, self.converged_ = sums.n_passes, float(f.sum()), converged
        self._packed = None
        if not converged:
            warnings.warn(f"LinearProbe stopped short of tol = {self.tol} after {self.max_iter} Newton steps", RuntimeWarning)
        return self

    # ------------------------------------------------------------------ predict
    def _pack(self, dev):
        """Padded device copies of the weights for ``lla_gemm_f32`` (as ``MLP._pack``): fp32 [Npad8][C], bias [Npad8]."""
        if self._packed is None or self._packed[0] != str(dev):
            K, C = self.coef_.shape
            npad = -(-K // 8) * 8
            w = torch.zeros((npad, C), dtype=torch.float32, device=dev)
            w[:K] = self.coef_.to(dev)
            b = torch.zeros(npad, dtype=torch.float32, device=dev)
            b[:K] = self.intercept_.to(dev)
            self._packed = (str(dev), w, b, npad)
        return self._packed[1:]

    def decision_function(self, data, rows_per_pass=65536):
        if self.coef_ is None:
            raise RuntimeError("fit first")
        rows = _Rows(data, rows_per_pass, False)
        rows.first_pass = _is_latents(data)       # (statuses of a decode are checked; tensors are taken as they are)
        K, C = self.coef_.shape
        if rows.dim != C:
            raise ValueError(f"data has {rows.dim} features, the probe was fitted on {C}")
        try:
            if rows.device.type == "cuda":
                if C % 8:
                    raise ValueError("the device path needs a feature width that is a multiple of 8")
                w, b, npad = self._pack(rows.device)
                out = torch.empty((rows.n, npad), dtype=torch.float32, device=rows.device)
                L = _lib.lib()
                with torch.cuda.device(rows.device):
                    for g0, z in rows.groups():
                        z = z if z.dtype == torch.float32 else z.float()
                        z = z if z.stride(1) == 1 and z.stride(0) % 4 == 0 else z.contiguous()
                        g = int(z.shape[0])
                        o = out[g0:g0 + g]
                        rc = L.lla_gemm_f32(_lib.ptr(z), int(z.stride(0)) if g > 1 else C, _lib.ptr(w), C, _lib.ptr(b),
                                            _lib.ptr(o), npad, g, npad, C, 0, _lib.stream_ptr(rows.device))
                        _lib.check(rc, "lla_gemm_f32")
                s = out[:, :K]
            else:
                W, b = self.coef_.to(torch.float64).cpu(), self.intercept_.to(torch.float64).cpu()
                s = torch.cat([z.to(torch.float64) @ W.T + b for _, z in rows.groups()]) if rows.n else \
                    torch.zeros((0, K), dtype=torch.float64)
        finally:
            rows.close()
        return s[:, 0].contiguous() if len(self.classes_) == 2 else s.contiguous()

    def predict(self, data, rows_per_pass=65536):
        s = self.decision_function(data, rows_per_pass)
        which = (s > 0).to(torch.int64) if s.dim() == 1 else s.argmax(1)
        return torch.from_numpy(self.classes_).to(s.device)[which]

    def score(self, data, labels=None, rows_per_pass=65536):
        pred = self.predict(data, rows_per_pass)
        y = self._labels_of(data, labels, pred.numel()).to(pred.device)
        return float((pred == y).double().mean())
