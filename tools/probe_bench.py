"""The linear probe's data pass, measured (MI355X; writes its table to stdout and, with --out, to a file).

N records stay resident on the device, as in tools/latents_bench.py.  For K = 10 and K = 1000 classes at C = 512:

(a)  one gradient pass of ``lla_svm_pass`` over the N rows already decoded (fp32, resident),
(c)  the same quantities from the parts the library offered before: ``lla_gemm_f32`` for the scores (K padded to a
     multiple of 8), torch elementwise ops for the residuals and the loss, ``R.T @ Z`` and ``R.sum(0)`` in torch,
(a') a whole streamed pass over a ``CompressedLatents`` -- ``take`` of a decode group into one reused buffer, then
     ``lla_svm_pass(accumulate=1)`` -- against the ``take`` calls alone.

Every arm is warmed up, then timed with device events; the arms are interleaved and the round is repeated ``--reps``
times.  (a) is checked against (c) before anything is timed.  Bar: the median of (a) may not exceed the median of (c)
by more than the spread of (c)'s own runs.

Reference point, reported and not gated: wall time of ``LinearProbe.fit`` on an STL10-shaped problem (5000 x 512,
K = 10) next to scikit-learn's ``LinearSVC(C=7e-3).fit`` on the same rows on this host, when scikit-learn is installed.

``--grid`` measures the cross-validated search instead: K = 10, 8 candidates x 5 folds = 400 problems,

(g)  one ``lla_svm_grid_pass`` over all N rows, every problem masking its own held-out fold,
(s)  what the library offered before: 40 ``lla_svm_pass(K = 10)`` calls, each over a contiguous copy of that fold's
     training rows (the copies are made outside the timed region),
both with the rows resident and streamed (``take`` of the rows a call needs, then the pass); a scale arm (K = 1000,
2 candidates x 2 folds = 4000 problems) is reported only.  Bar: the median of (g) lies below the median of (s) by more
than the spread of (s)'s own runs, resident and streamed.  Reported, not gated: wall time of ``LinearProbeCV.fit`` at the
STL10 shape against the same search as a loop of ``LinearProbe.fit``.

``--softmax`` measures the softmax-regression pass instead, at K = 10 (the row statistics inside the
pass) and K = 1000 (the row-statistics kernel first), in gradient and in Hessian-vector mode:

(a)  one ``lla_softmax_pass`` over the N resident rows,
(c)  ``lla_gemm_f32`` for the scores (and for t), torch ``log_softmax`` and elementwise ops, ``R.T @ Z`` and ``R.sum(0)``,
(a') streamed: ``take`` of a decode group, then ``lla_softmax_pass(accumulate=1)``, against the ``take`` calls alone.
Bar, as above: the median of (a) may not exceed the median of (c) by more than the spread of (c)'s own runs.

``--softmax-grid`` measures the cross-validated softmax regression instead: K = 10, 8 candidates x 5 folds =
40 classifiers (14 tiles), in gradient and in Hessian-vector mode,

(g)  one ``lla_softmax_grid_pass`` over all N rows, every classifier leaving its own fold out,
(s)  what the library offered before: 40 ``lla_softmax_pass(K = 10)`` calls, each over a contiguous copy of that fold's
     training rows (the copies are made outside the timed region),
both resident and streamed; (g) is checked against (s) first.  Bar: the median of (g) lies below the median of (s) by more
than (s)'s spread, resident and streamed.  Reported, not gated: ``LogisticProbeCV.fit`` at the STL10 shape against the same
search as a loop of ``LogisticProbe.fit``, and the pass time of the K = 1000 fallback (``lla_softmax_pass`` per classifier).

usage (GPU box): python tools/probe_bench.py [--records 131072] [--reps 3] [--out profiles/linear_probe.txt]
                 python tools/probe_bench.py --grid --out profiles/linear_probe_cv.txt
                 python tools/probe_bench.py --softmax --out profiles/logistic_probe.txt
                 python tools/probe_bench.py --softmax-grid --out profiles/logistic_probe_cv.txt
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import hubconf  # noqa: E402
from latents_bench import interleaved, med  # noqa: E402
from lossyless_amd import LinearProbe, LinearProbeCV, LogisticProbe, LogisticProbeCV, _lib  # noqa: E402


def grid_arms(args, say, dev, ds, Z, g):
    """The --grid table (module docstring)."""
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    N, C = Z.shape
    group = 65536
    buf = torch.empty((min(group, N), C), dtype=torch.float32, device=dev)
    pieces = lambda idx: [idx[i:i + group] for i in range(0, idx.numel(), group)]       # noqa: E731
    for K, n_cand, n_fold, gated in ((10, 8, 5, True), (1000, 2, 2, False)):
        G = n_cand * n_fold
        J = G * K
        inner = args.inner or (10 if gated else 4)
        y = torch.randint(0, K, (N,), generator=g).to(torch.int32).to(dev)
        fold = (torch.arange(N) % n_fold).to(torch.int32).to(dev)
        W = (torch.randn(J, C, generator=g) * 0.03).to(dev)
        b = (torch.randn(J, generator=g) * 0.1).to(dev)
        # problem (candidate c, fold f, class k) is column (c n_fold + f) K + k; candidate c weighs its positives by 1 + c / 8
        cols = [torch.arange(K, dtype=torch.int32).repeat(G).to(dev),
                torch.arange(n_fold, dtype=torch.int32).repeat_interleave(K).repeat(n_cand).to(dev),
                (1.0 + torch.arange(n_cand) / 8.0).repeat_interleave(n_fold * K).to(dev), torch.ones(J, device=dev)]
        ws = torch.empty(int(L.lla_svm_grid_pass_workspace_bytes(C, J)), dtype=torch.uint8, device=dev)
        oW, ob = torch.empty((J, C), device=dev), torch.empty(J, device=dev)
        ol = torch.empty(J, dtype=torch.float64, device=dev)

        def grid(rows=Z, labels=y, folds=fold, acc=0):
            rc = L.lla_svm_grid_pass(_lib.ptr(rows), _lib.LLA_Z_F32, C, _lib.ptr(labels), _lib.ptr(folds), rows.shape[0], C,
                                     _lib.ptr(W), _lib.ptr(b), None, None, J, C, *[_lib.ptr(t) for t in cols], _lib.ptr(oW),
                                     _lib.ptr(ob), _lib.ptr(ol), acc, _lib.ptr(ws), st)
            _lib.check(rc, "lla_svm_grid_pass")

        # (s): the parent's path.  One contiguous copy of every fold's training rows, one call per (candidate, fold)
        train_idx = [torch.nonzero(fold != f)[:, 0] for f in range(n_fold)]
        train_rows = [Z[idx] for idx in train_idx] if gated or N * C * 4 * n_fold <= 2 ** 31 else None
        train_y = [y[idx].contiguous() for idx in train_idx]
        ws1 = torch.empty(int(L.lla_svm_pass_workspace_bytes(C, K)), dtype=torch.uint8, device=dev)
        sW, sb = torch.empty((J, C), device=dev), torch.empty(J, device=dev)
        sl = torch.empty(J, dtype=torch.float64, device=dev)

        def one(rows, labels, at, acc):
            rc = L.lla_svm_pass(_lib.ptr(rows), _lib.LLA_Z_F32, C, _lib.ptr(labels), rows.shape[0], C, _lib.ptr(W[at:at + K]),
                                _lib.ptr(b[at:at + K]), None, None, K, C, _lib.ptr(sW[at:at + K]), _lib.ptr(sb[at:at + K]),
                                _lib.ptr(sl[at:at + K]), acc, _lib.ptr(ws1), st)
            _lib.check(rc, "lla_svm_pass")

        def loop():
            for c in range(n_cand):
                for f in range(n_fold):
                    one(train_rows[f], train_y[f], (c * n_fold + f) * K, 0)

        idxs = [(g0, torch.arange(g0, min(g0 + group, N), device=dev)) for g0 in range(0, N, group)]
        train_pieces = [[(p, y[p].contiguous()) for p in pieces(idx)] for idx in train_idx]

        def grid_streamed():
            oW.zero_(), ob.zero_(), ol.zero_()
            for g0, idx in idxs:
                rows = ds.take(idx, out=buf[:idx.numel()], check=False)
                grid(rows, y[g0:g0 + idx.numel()], fold[g0:g0 + idx.numel()], 1)

        def loop_streamed():
            sW.zero_(), sb.zero_(), sl.zero_()
            for c in range(n_cand):
                for f in range(n_fold):
                    for idx, labels in train_pieces[f]:
                        one(ds.take(idx, out=buf[:idx.numel()], check=False), labels, (c * n_fold + f) * K, 1)

        # the same sums from both paths before anything is timed: (s) unweighted, so (g)'s positives are compared through
        # the weight -- the loss is linear in it only per sign, so the check is on candidate 0 (weight 1) for every fold
        grid(), loop()
        torch.cuda.synchronize(dev)
        first = n_fold * K
        scale = float(sW[:first].abs().max())
        err = float((oW[:first] - sW[:first]).abs().max()) / scale
        lerr = float(((ol[:first] - sl[:first]).abs() / sl[:first]).max())
        assert err < 1e-4 and lerr < 1e-5, f"arms disagree: {err:.2e} {lerr:.2e}"
        arms = {"(g) one lla_svm_grid_pass, rows resident": grid, f"(s) {G} lla_svm_pass calls, rows resident": loop}
        if gated:
            keep = oW.clone()
            grid_streamed()
            torch.cuda.synchronize(dev)
            assert float((oW - keep).abs().max()) / scale < 1e-4, "the streamed grid pass disagrees"
            arms["(g') streamed: take + lla_svm_grid_pass"] = grid_streamed
            arms[f"(s') streamed: {G} x (take + lla_svm_pass)"] = loop_streamed
        times = interleaved(arms, inner, args.reps, dev)
        say()
        say(f"K = {K}, {n_cand} candidates x {n_fold} folds = {J} problems ({-(-J // 32)} problem tiles): ms per pass over {N} rows, "
            f"device events over {inner} back-to-back passes, {args.reps} interleaved runs   (max |(g) - (s)| / max |(s)| = {err:.1e})")
        for k, ts in times.items():
            runs = "  ".join(f"{x:9.4f}" for x in ts)
            say(f"    {k:46s} {runs}   median {med(ts):9.4f} ms")
        names = list(times)
        for gk, sk in zip(names[0::2], names[1::2]):
            gt, stt = times[gk], times[sk]
            spread = max(stt) - min(stt)
            verdict = ("MET" if med(gt) < med(stt) - spread else "MISSED") if gated else "reported only"
            say(f"    {gk[:4].strip()} / {sk[:4].strip()} medians = {med(gt) / med(stt):.3f};  spread of {sk[:4].strip()} = {spread:.4f} ms;  "
                f"{sk[:4].strip()} - {gk[:4].strip()} = {med(stt) - med(gt):+.4f} ms   -> bar {verdict}")
        gt = times[names[0]]
        say(f"    (g): {4.0 * N * C * (-(-J // 32) * 32) / med(gt) / 1e9:.1f} TFLOP/s on the padded tiles, z read {-(-J // 32)} times "
            f"({N * C * 4 * -(-J // 32) / med(gt) / 1e9:.2f} TB/s, mostly from cache)")
        del train_rows, train_pieces, W, oW, sW

    # whole call at the STL10 shape: the search in shared passes against the same search as a loop of fits
    n, k, C = 5000, 10, Z.shape[1]
    labels = torch.arange(n) % k
    mu = torch.randn(k, C, generator=g) * 0.1
    Xd = (mu[labels] + torch.randn(n, C, generator=g) * 0.5).to(dev)
    cands = LinearProbeCV.sample(8, seed=0)
    LinearProbeCV(cands[:2], cv=5).fit(Xd[:512], labels[:512])            # (code objects loaded)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    cv = LinearProbeCV(cands, cv=5).fit(Xd, labels)
    torch.cuda.synchronize(dev)
    cv_s = time.perf_counter() - t0
    fold = torch.empty(n, dtype=torch.int64)
    for c in range(k):                                                   # the r-th row of a class goes to fold r % 5
        at = torch.nonzero(labels == c)[:, 0]
        fold[at] = torch.arange(at.numel()) % 5
    t0 = time.perf_counter()
    passes, scores = 0, torch.zeros(len(cands), 5, dtype=torch.float64)
    for c, (Cw, cw) in enumerate(cands):
        for f in range(5):
            tr, te = torch.nonzero(fold != f)[:, 0].to(dev), torch.nonzero(fold == f)[:, 0].to(dev)
            p = LinearProbe(C=Cw, class_weight=cw).fit(Xd[tr], labels[tr.cpu()])
            scores[c, f] = p.score(Xd[te], labels[te.cpu()])
            passes += p.n_passes_ + 1
    best = int(scores.mean(1).argmax())
    p = LinearProbe(C=cands[best][0], class_weight=cands[best][1]).fit(Xd, labels)
    torch.cuda.synchronize(dev)
    loop_s = time.perf_counter() - t0
    say()
    say(f"STL10-shaped search ({n} x {C}, K = {k}, 8 candidates x 5 folds + refit): LinearProbeCV.fit {cv_s:.3f} s wall, "
        f"{cv.n_passes_} passes, all converged {bool(cv.converged_.all())}, best {cv.best_index_} "
        f"(mean accuracy {float(cv.mean_scores_[cv.best_index_]):.4f})")
    say(f"    the same search as a loop of LinearProbe.fit (40 fits + scores + 1 refit): {loop_s:.3f} s wall, {passes + p.n_passes_} passes, "
        f"best {best} (mean accuracy {float(scores.mean(1)[best]):.4f}); max |score difference| "
        f"{float((scores - cv.cv_scores_).abs().max()):.4f}   (reported, not gated)")


def softmax_arms(args, say, dev, ds, Z, g):
    """The --softmax table (module docstring)."""
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    N, C = Z.shape
    group = 65536
    buf = torch.empty((min(group, N), C), dtype=torch.float32, device=dev)
    idxs = [(g0, torch.arange(g0, min(g0 + group, N), device=dev)) for g0 in range(0, N, group)]
    for K in (10, 1000):
        inner = args.inner or (40 if K <= 32 else 8)
        y = torch.randint(0, K, (N,), generator=g).to(torch.int32).to(dev)
        y64 = y.to(torch.int64)
        W = (torch.randn(K, C, generator=g) * 0.03).to(dev)
        b = (torch.randn(K, generator=g) * 0.1).to(dev)
        V = (torch.randn(K, C, generator=g) * 0.03).to(dev)
        vb = (torch.randn(K, generator=g) * 0.1).to(dev)
        cw = (0.5 + torch.rand(K, generator=g)).to(dev)
        ws = torch.empty(int(L.lla_softmax_pass_workspace_bytes(C, K, N)), dtype=torch.uint8, device=dev)
        oW, ob = torch.empty((K, C), device=dev), torch.empty(K, device=dev)
        ol = torch.empty(K, dtype=torch.float64, device=dev)
        npad = -(-K // 8) * 8
        Wp, bp = torch.zeros((npad, C), device=dev), torch.zeros(npad, device=dev)
        Vp, vbp = torch.zeros((npad, C), device=dev), torch.zeros(npad, device=dev)
        Wp[:K], bp[:K], Vp[:K], vbp[:K] = W, b, V, vb
        S, T = torch.empty((N, npad), device=dev), torch.empty((N, npad), device=dev)
        wi = cw[y64][:, None]
        for hv in (False, True):
            Vm, vbm = (V, vb) if hv else (None, None)
            parts = {}

            def fused(rows=Z, labels=y, acc=0):
                rc = L.lla_softmax_pass(_lib.ptr(rows), _lib.LLA_Z_F32, C, _lib.ptr(labels), rows.shape[0], C, _lib.ptr(W),
                                        _lib.ptr(b), _lib.ptr(Vm), _lib.ptr(vbm), K, C, _lib.ptr(cw), _lib.ptr(oW), _lib.ptr(ob),
                                        _lib.ptr(ol), acc, _lib.ptr(ws), st)
                _lib.check(rc, "lla_softmax_pass")

            def from_parts():
                rc = L.lla_gemm_f32(_lib.ptr(Z), C, _lib.ptr(Wp), C, _lib.ptr(bp), _lib.ptr(S), npad, N, npad, C, 0, st)
                _lib.check(rc, "lla_gemm_f32")
                logp = torch.log_softmax(S[:, :K], 1)
                if hv:
                    rc = L.lla_gemm_f32(_lib.ptr(Z), C, _lib.ptr(Vp), C, _lib.ptr(vbp), _lib.ptr(T), npad, N, npad, C, 0, st)
                    _lib.check(rc, "lla_gemm_f32")
                    pk, t = logp.exp(), T[:, :K]
                    R = wi * pk * (t - (pk * t).sum(1, keepdim=True))
                else:
                    R = logp.exp()
                    R[torch.arange(N, device=dev), y64] -= 1.0
                    R *= wi
                    parts["loss"] = -(wi[:, 0] * logp[torch.arange(N, device=dev), y64]).sum(dtype=torch.float64)
                parts["W"], parts["b"] = R.T @ Z, R.sum(0)

            def take_only():
                for _, idx in idxs:
                    ds.take(idx, out=buf[:idx.numel()], check=False)

            def streamed():
                oW.zero_(), ob.zero_(), ol.zero_()
                for g0, idx in idxs:
                    rows = ds.take(idx, out=buf[:idx.numel()], check=False)
                    fused(rows, y[g0:g0 + idx.numel()], 1)

            # same sums from both paths, before anything is timed (fp32 in different orders: relative to the absolute sums)
            fused(), from_parts()
            torch.cuda.synchronize(dev)
            scale = float(parts["W"].abs().max())
            err = float((oW - parts["W"]).abs().max()) / scale
            lerr = 0.0 if hv else abs(float(ol.sum()) - float(parts["loss"])) / float(parts["loss"])
            assert err < 1e-4 and lerr < 1e-5, f"arms disagree: {err:.2e} {lerr:.2e}"
            first = oW.clone()
            streamed()
            torch.cuda.synchronize(dev)
            assert float((oW - first).abs().max()) / scale < 1e-4, "the streamed pass disagrees"

            mode = "Hessian-vector" if hv else "gradient"
            names = ["(a) lla_softmax_pass, rows resident", "(c) gemm_f32 + log_softmax + R.T @ Z",
                     "(a') streamed: take + lla_softmax_pass", "     take alone"]
            times = interleaved(dict(zip(names, (fused, from_parts, streamed, take_only))), inner, args.reps, dev)
            say()
            say(f"K = {K}, {mode} mode ({'one kernel' if K <= 32 else 'row statistics + pass'}): ms per pass over {N} rows, device "
                f"events over {inner} back-to-back calls, {args.reps} interleaved runs   (max |(a) - (c)| / max |(c)| = {err:.1e})")
            for k, ts in times.items():
                runs = "  ".join(f"{x:9.4f}" for x in ts)
                say(f"    {k:40s} {runs}   median {med(ts):9.4f} ms")
            a, c = times[names[0]], times[names[1]]
            ok = med(a) <= med(c) + (max(c) - min(c))
            say(f"    (a) / (c) medians = {med(a) / med(c):.3f};  spread of (c) = {max(c) - min(c):.4f} ms;  "
                f"(a) - (c) = {med(a) - med(c):+.4f} ms   -> bar {'MET' if ok else 'MISSED'}")

    # reference point: an STL10-shaped fit
    n, k = 5000, 10
    labels = torch.arange(n) % k
    mu = torch.randn(k, C, generator=g) * 0.1
    X = mu[labels] + torch.randn(n, C, generator=g) * 0.5
    Xd = X.to(dev)
    LogisticProbe().fit(Xd[:512], labels[:512])          # (code objects loaded)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    p = LogisticProbe().fit(Xd, labels)
    torch.cuda.synchronize(dev)
    fit_s = time.perf_counter() - t0
    say()
    say(f"STL10-shaped fit ({n} x {C}, K = {k}): LogisticProbe.fit {fit_s:.3f} s wall, {p.n_passes_} passes, converged "
        f"{p.converged_}, train accuracy {p.score(Xd, labels):.4f}")
    try:
        from sklearn.linear_model import LogisticRegression
        X1 = torch.cat([X, torch.ones(n, 1)], 1).numpy()
        t0 = time.perf_counter()
        clf = LogisticRegression(C=1.0, fit_intercept=False, max_iter=1000).fit(X1, labels.numpy())
        say(f"    scikit-learn LogisticRegression(C=1, fit_intercept=False) on [Z, 1] on this host: {time.perf_counter() - t0:.3f} s "
            f"wall, train accuracy {clf.score(X1, labels.numpy()):.4f}   (reported, not gated)")
    except ImportError:
        say("    scikit-learn is not installed here: no host reference")


def softmax_grid_arms(args, say, dev, ds, Z, g):
    """The --softmax-grid table (module docstring)."""
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    N, C = Z.shape
    group = 65536
    buf = torch.empty((min(group, N), C), dtype=torch.float32, device=dev)
    pieces = lambda idx: [idx[i:i + group] for i in range(0, idx.numel(), group)]       # noqa: E731
    K, n_cand, n_fold = 10, 8, 5
    G = n_cand * n_fold
    J = G * K
    inner = args.inner or 10
    y = torch.randint(0, K, (N,), generator=g).to(torch.int32).to(dev)
    fold = (torch.arange(N) % n_fold).to(torch.int32).to(dev)
    W = (torch.randn(J, C, generator=g) * 0.03).to(dev)
    b = (torch.randn(J, generator=g) * 0.1).to(dev)
    V = torch.randn(J, C, generator=g).to(dev)
    vb = torch.randn(J, generator=g).to(dev)
    # classifier (candidate c, fold f) is group c n_fold + f; candidate c weighs class k by 1 + (c + k) / 16
    held = torch.arange(n_fold, dtype=torch.int32).repeat(n_cand).to(dev)
    cw = (1.0 + (torch.arange(n_cand)[:, None, None] + torch.arange(K)[None, None, :]) / 16.0).expand(n_cand, n_fold, K) \
        .reshape(G, K).contiguous().to(dev)
    ws = torch.empty(int(L.lla_softmax_grid_pass_workspace_bytes(C, K, G)), dtype=torch.uint8, device=dev)
    ws1 = torch.empty(int(L.lla_softmax_pass_workspace_bytes(C, K, N)), dtype=torch.uint8, device=dev)
    oW, ob, ol = torch.empty((J, C), device=dev), torch.empty(J, device=dev), torch.empty(J, dtype=torch.float64, device=dev)
    sW, sb, sl = torch.empty((J, C), device=dev), torch.empty(J, device=dev), torch.empty(J, dtype=torch.float64, device=dev)
    train_idx = [torch.nonzero(fold != f)[:, 0] for f in range(n_fold)]
    train_rows = [Z[idx] for idx in train_idx]
    train_y = [y[idx].contiguous() for idx in train_idx]
    idxs = [(g0, torch.arange(g0, min(g0 + group, N), device=dev)) for g0 in range(0, N, group)]
    train_pieces = [[(p, y[p].contiguous()) for p in pieces(idx)] for idx in train_idx]
    tiles = -(-G // (32 // K))
    for hv in (False, True):
        Vm, vbm = (V, vb) if hv else (None, None)

        def grid(rows=Z, labels=y, folds=fold, acc=0):
            rc = L.lla_softmax_grid_pass(_lib.ptr(rows), _lib.LLA_Z_F32, C, _lib.ptr(labels), _lib.ptr(folds), rows.shape[0], C,
                                         _lib.ptr(W), _lib.ptr(b), _lib.ptr(Vm), _lib.ptr(vbm), K, G, C, _lib.ptr(held),
                                         _lib.ptr(cw), _lib.ptr(oW), _lib.ptr(ob), _lib.ptr(ol), acc, _lib.ptr(ws), st)
            _lib.check(rc, "lla_softmax_grid_pass")

        def one(rows, labels, gi, acc):
            at = gi * K
            rc = L.lla_softmax_pass(_lib.ptr(rows), _lib.LLA_Z_F32, C, _lib.ptr(labels), rows.shape[0], C, _lib.ptr(W[at:at + K]),
                                    _lib.ptr(b[at:at + K]), _lib.ptr(None if Vm is None else Vm[at:at + K]),
                                    _lib.ptr(None if vbm is None else vbm[at:at + K]), K, C, _lib.ptr(cw[gi]),
                                    _lib.ptr(sW[at:at + K]), _lib.ptr(sb[at:at + K]), _lib.ptr(sl[at:at + K]), acc, _lib.ptr(ws1), st)
            _lib.check(rc, "lla_softmax_pass")

        def loop():
            for gi in range(G):
                one(train_rows[gi % n_fold], train_y[gi % n_fold], gi, 0)

        def grid_streamed():
            oW.zero_(), ob.zero_(), ol.zero_()
            for g0, idx in idxs:
                rows = ds.take(idx, out=buf[:idx.numel()], check=False)
                grid(rows, y[g0:g0 + idx.numel()], fold[g0:g0 + idx.numel()], 1)

        def loop_streamed():
            sW.zero_(), sb.zero_(), sl.zero_()
            for gi in range(G):
                for idx, labels in train_pieces[gi % n_fold]:
                    one(ds.take(idx, out=buf[:idx.numel()], check=False), labels, gi, 1)

        # the same sums from both paths before anything is timed (fp32 in different orders: relative to the largest sum)
        grid(), loop()
        torch.cuda.synchronize(dev)
        scale = float(sW.abs().max())
        err = float((oW - sW).abs().max()) / scale
        lerr = 0.0 if hv else float(((ol - sl).abs() / sl.abs().clamp_min(1e-30)).max())
        assert err < 1e-4 and lerr < 1e-5, f"arms disagree: {err:.2e} {lerr:.2e}"
        keep = oW.clone()
        grid_streamed()
        torch.cuda.synchronize(dev)
        assert float((oW - keep).abs().max()) / scale < 1e-4, "the streamed grid pass disagrees"
        arms = {"(g) one lla_softmax_grid_pass, rows resident": grid, f"(s) {G} lla_softmax_pass calls, rows resident": loop,
                "(g') streamed: take + lla_softmax_grid_pass": grid_streamed,
                f"(s') streamed: {G} x (take + lla_softmax_pass)": loop_streamed}
        times = interleaved(arms, inner, args.reps, dev)
        say()
        say(f"{'Hessian-vector' if hv else 'gradient'} mode, K = {K}, {n_cand} candidates x {n_fold} folds = {G} classifiers ({tiles} "
            f"tiles): ms per pass over {N} rows, device events over {inner} back-to-back passes, {args.reps} interleaved runs   "
            f"(max |(g) - (s)| / max |(s)| = {err:.1e})")
        for k, ts in times.items():
            runs = "  ".join(f"{x:9.4f}" for x in ts)
            say(f"    {k:50s} {runs}   median {med(ts):9.4f} ms")
        names = list(times)
        for gk, sk in zip(names[0::2], names[1::2]):
            gt, stt = times[gk], times[sk]
            spread = max(stt) - min(stt)
            verdict = "MET" if med(gt) < med(stt) - spread else "MISSED"
            say(f"    {gk[:4].strip()} / {sk[:4].strip()} medians = {med(gt) / med(stt):.3f};  spread of {sk[:4].strip()} = {spread:.4f} ms;  "
                f"{sk[:4].strip()} - {gk[:4].strip()} = {med(stt) - med(gt):+.4f} ms   -> bar {verdict}")
    del train_rows, train_pieces

    # the K > 32 fallback of LogisticProbeCV: lla_softmax_pass per classifier over ALL rows, held-out rows relabelled -1
    K2, G2 = 1000, 4
    y2 = torch.randint(0, K2, (N,), generator=g).to(torch.int32).to(dev)
    yg = torch.where(fold[None, :] % 2 == torch.arange(G2, device=dev)[:, None] % 2, -1, y2[None, :]).to(torch.int32).contiguous()
    W2, b2 = (torch.randn(G2, K2, C, generator=g) * 0.03).to(dev), (torch.randn(G2, K2, generator=g) * 0.1).to(dev)
    o2W, o2b = torch.empty((G2, K2, C), device=dev), torch.empty((G2, K2), device=dev)
    o2l = torch.empty((G2, K2), dtype=torch.float64, device=dev)
    ws2 = torch.empty(int(L.lla_softmax_pass_workspace_bytes(C, K2, N)), dtype=torch.uint8, device=dev)

    def fallback():
        for gi in range(G2):
            rc = L.lla_softmax_pass(_lib.ptr(Z), _lib.LLA_Z_F32, C, _lib.ptr(yg[gi]), N, C, _lib.ptr(W2[gi]), _lib.ptr(b2[gi]), None,
                                    None, K2, C, None, _lib.ptr(o2W[gi]), _lib.ptr(o2b[gi]), _lib.ptr(o2l[gi]), 0, _lib.ptr(ws2), st)
            _lib.check(rc, "lla_softmax_pass")
    ts = interleaved({"fallback": fallback}, 2, args.reps, dev)["fallback"]
    say()
    say(f"K = {K2} fallback (2 candidates x 2 folds = {G2} lla_softmax_pass calls over all {N} rows, gradient mode): "
        f"{'  '.join(f'{x:9.4f}' for x in ts)}   median {med(ts):9.4f} ms per pass   (reported, not gated)")

    # whole call at the STL10 shape: the search in shared passes against the same search as a loop of fits
    n, k = 5000, 10
    labels = torch.arange(n) % k
    mu = torch.randn(k, C, generator=g) * 0.1
    Xd = (mu[labels] + torch.randn(n, C, generator=g) * 0.5).to(dev)
    cands = LogisticProbeCV.logspace(8, 1e-3, 10.0)
    LogisticProbeCV(cands[:2], cv=5).fit(Xd[:512], labels[:512])            # (code objects loaded)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    cv = LogisticProbeCV(cands, cv=5).fit(Xd, labels)
    torch.cuda.synchronize(dev)
    cv_s = time.perf_counter() - t0
    fold5 = torch.empty(n, dtype=torch.int64)
    for c in range(k):                                                   # the r-th row of a class goes to fold r % 5
        at = torch.nonzero(labels == c)[:, 0]
        fold5[at] = torch.arange(at.numel()) % 5
    t0 = time.perf_counter()
    passes, scores = 0, torch.zeros(len(cands), 5, dtype=torch.float64)
    for c, (Cw, cwt) in enumerate(cands):
        for f in range(5):
            tr, te = torch.nonzero(fold5 != f)[:, 0].to(dev), torch.nonzero(fold5 == f)[:, 0].to(dev)
            p = LogisticProbe(C=Cw, class_weight=cwt).fit(Xd[tr], labels[tr.cpu()])
            scores[c, f] = p.score(Xd[te], labels[te.cpu()])
            passes += p.n_passes_ + 1
    best = int(scores.mean(1).argmax())
    p = LogisticProbe(C=cands[best][0], class_weight=cands[best][1]).fit(Xd, labels)
    torch.cuda.synchronize(dev)
    loop_s = time.perf_counter() - t0
    say()
    say(f"STL10-shaped search ({n} x {C}, K = {k}, 8 candidates x 5 folds + refit): LogisticProbeCV.fit {cv_s:.3f} s wall, "
        f"{cv.n_passes_} passes, all converged {bool(cv.converged_.all())}, best {cv.best_index_} "
        f"(mean accuracy {float(cv.mean_scores_[cv.best_index_]):.4f})")
    say(f"    the same search as a loop of LogisticProbe.fit (40 fits + scores + 1 refit): {loop_s:.3f} s wall, {passes + p.n_passes_} "
        f"passes, best {best} (mean accuracy {float(scores.mean(1)[best]):.4f}); max |score difference| "
        f"{float((scores - cv.cv_scores_).abs().max()):.4f}   (reported, not gated)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=0, help="calls per timed window (0: 40 at K = 10, 8 at K = 1000)")
    ap.add_argument("--grid", action="store_true", help="measure the cross-validated search (lla_svm_grid_pass) instead")
    ap.add_argument("--softmax", action="store_true", help="measure the softmax-regression pass (lla_softmax_pass) instead")
    ap.add_argument("--softmax-grid", action="store_true",
                    help="measure the cross-validated softmax regression (lla_softmax_grid_pass) instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_bench.py measures on an MI355X: no GPU here, nothing measured")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", torch.cuda.current_device())
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    eb, t = comp.entropy_bottleneck, comp._tables()
    L, N, C = _lib.lib(), args.records, comp.z_dim
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(N, C, generator=g) * 0.5).to(dev)
    payload, offsets, _ = eb.encode_device(z, t, record_prefix=True)
    torch.cuda.synchronize(dev)
    total = int(offsets[-1])
    with tempfile.TemporaryDirectory() as d:      # the container file CompressedLatents opens: be32(N) + the body
        f = os.path.join(d, "Z.bin")
        with open(f, "wb") as fh:
            fh.write(N.to_bytes(4, "big"))
            fh.write(payload[:total].cpu().numpy().tobytes())
        ds = comp.open_dataset(f)
    del payload, offsets, z
    Z = ds.all()
    say(f"device: {torch.cuda.get_device_name(dev)}   N = {N} records resident, {ds.nbytes / 2**20:.1f} MiB compressed against "
        f"{N * C * 4 / 2**20:.0f} MiB of fp32 rows; C = {C}")
    st = _lib.stream_ptr(dev)
    group = 65536
    buf = torch.empty((min(group, N), C), dtype=torch.float32, device=dev)
    idxs = [(g0, torch.arange(g0, min(g0 + group, N), device=dev)) for g0 in range(0, N, group)]

    if args.grid or args.softmax or args.softmax_grid:
        (grid_arms if args.grid else softmax_grid_arms if args.softmax_grid else softmax_arms)(args, say, dev, ds, Z, g)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return

    for K in (10, 1000):
        inner = args.inner or (40 if K <= 32 else 8)
        y = torch.randint(0, K, (N,), generator=g).to(torch.int32).to(dev)
        W = (torch.randn(K, C, generator=g) * 0.03).to(dev)
        b = (torch.randn(K, generator=g) * 0.1).to(dev)
        ws = torch.empty(int(L.lla_svm_pass_workspace_bytes(C, K)), dtype=torch.uint8, device=dev)
        oW, ob = torch.empty((K, C), device=dev), torch.empty(K, device=dev)
        ol = torch.empty(K, dtype=torch.float64, device=dev)

        def fused(rows=Z, labels=y, acc=0):
            rc = L.lla_svm_pass(_lib.ptr(rows), _lib.LLA_Z_F32, C, _lib.ptr(labels), rows.shape[0], C, _lib.ptr(W), _lib.ptr(b),
                                None, None, K, C, _lib.ptr(oW), _lib.ptr(ob), _lib.ptr(ol), acc, _lib.ptr(ws), st)
            _lib.check(rc, "lla_svm_pass")

        npad = -(-K // 8) * 8
        Wp, bp = torch.zeros((npad, C), device=dev), torch.zeros(npad, device=dev)
        Wp[:K], bp[:K] = W, b
        S = torch.empty((N, npad), device=dev)
        cls = torch.arange(npad, device=dev, dtype=torch.int32)[None, :]
        parts = {}

        def from_parts():
            rc = L.lla_gemm_f32(_lib.ptr(Z), C, _lib.ptr(Wp), C, _lib.ptr(bp), _lib.ptr(S), npad, N, npad, C, 0, st)
            _lib.check(rc, "lla_gemm_f32")
            ys = torch.where(y[:, None] == cls, 1.0, -1.0)
            m = (1.0 - ys * S).clamp_min_(0.0)
            m[:, K:] = 0.0
            R = -2.0 * ys * m
            parts["loss"], parts["W"], parts["b"] = (m * m).sum(0, dtype=torch.float64), R.T @ Z, R.sum(0)

        def take_only():
            for _, idx in idxs:
                ds.take(idx, out=buf[:idx.numel()], check=False)

        def streamed():
            oW.zero_(), ob.zero_(), ol.zero_()
            for g0, idx in idxs:
                rows = ds.take(idx, out=buf[:idx.numel()], check=False)
                fused(rows, y[g0:g0 + idx.numel()], 1)

        # same sums from both paths, before anything is timed (fp32 in different orders: relative to the absolute sums)
        fused(), from_parts()
        torch.cuda.synchronize(dev)
        scale = float(parts["W"].abs().max())
        err = float((oW - parts["W"][:K]).abs().max()) / scale
        lerr = float(((ol - parts["loss"][:K]).abs() / parts["loss"][:K]).max())
        assert err < 1e-4 and lerr < 1e-5, f"arms disagree: {err:.2e} {lerr:.2e}"
        first = oW.clone()
        streamed()
        torch.cuda.synchronize(dev)
        assert float((oW - first).abs().max()) / scale < 1e-4, "the streamed pass disagrees"

        arms = {"(a) lla_svm_pass, rows resident": fused, "(c) gemm_f32 + torch + R.T @ Z": from_parts,
                "(a') streamed: take + lla_svm_pass": streamed, "     take alone": take_only}
        times = interleaved(arms, inner, args.reps, dev)
        say()
        say(f"K = {K}: ms per pass over {N} rows, device events over {inner} back-to-back calls, {args.reps} interleaved runs"
            f"   (max |(a) - (c)| / max |(c)| = {err:.1e})")
        for k, ts in times.items():
            runs = "  ".join(f"{x:9.4f}" for x in ts)
            say(f"    {k:38s} {runs}   median {med(ts):9.4f} ms")
        a, c = times["(a) lla_svm_pass, rows resident"], times["(c) gemm_f32 + torch + R.T @ Z"]
        flop = 4.0 * N * C * (-(-K // 32) * 32)
        say(f"    (a): {N * C * 4 * -(-K // 32) / med(a) / 1e9:.2f} TB/s of z read ({-(-K // 32)} class tile(s)), "
            f"{flop / med(a) / 1e9:.1f} TFLOP/s on the padded tiles")
        ok = med(a) <= med(c) + (max(c) - min(c))
        say(f"    (a) / (c) medians = {med(a) / med(c):.3f};  spread of (c) = {max(c) - min(c):.4f} ms;  "
            f"(a) - (c) = {med(a) - med(c):+.4f} ms   -> bar {'MET' if ok else 'MISSED'}")

    # reference point: an STL10-shaped fit
    n, k = 5000, 10
    labels = torch.arange(n) % k
    mu = torch.randn(k, C, generator=g) * 0.1
    X = (mu[labels] + torch.randn(n, C, generator=g) * 0.5)
    Xd = X.to(dev)
    LinearProbe().fit(Xd[:512], labels[:512])            # (code objects loaded)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    p = LinearProbe().fit(Xd, labels)
    torch.cuda.synchronize(dev)
    fit_s = time.perf_counter() - t0
    say()
    say(f"STL10-shaped fit ({n} x {C}, K = {k}): LinearProbe.fit {fit_s:.3f} s wall, {p.n_passes_} passes, converged {p.converged_}, "
        f"train accuracy {p.score(Xd, labels):.4f}")
    try:
        from sklearn.svm import LinearSVC
        t0 = time.perf_counter()
        clf = LinearSVC(C=7e-3).fit(X.numpy(), labels.numpy())
        say(f"    scikit-learn LinearSVC(C=7e-3).fit on this host: {time.perf_counter() - t0:.3f} s wall, train accuracy "
            f"{clf.score(X.numpy(), labels.numpy()):.4f}   (reported, not gated)")
    except ImportError:
        say("    scikit-learn is not installed here: no host reference")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
