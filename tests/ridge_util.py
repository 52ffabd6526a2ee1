"""Shared by test_ridge_probe_host.py and test_gpu_ridge_probe.py: callers of ``lla_gram_pass`` / ``lla_segment_sums``, seeded
data, the float64 moments with the bounds the kernels are held to, and the measurement the end-to-end tolerance comes from
(no test in here)."""
import numpy as np
import torch

from probe_util import U

U64 = 2.0 ** -53


def make_ridge_data(N, C, K, n_targets, seed, sep=1.0):
    """-> (X float32 [N, C] around K class means of scale ``sep`` (small: the classes overlap), y int64 [N] with every class
    present, T float32 [N, n_targets] = a linear map of X plus noise): everything fp32-representable, so that the device and
    the float64 twin see the same numbers."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(K, C, generator=g, dtype=torch.float64) * sep
    y = (torch.arange(N) % K)[torch.randperm(N, generator=g)]
    X = (mu[y] + torch.randn(N, C, generator=g, dtype=torch.float64)).float()
    A = torch.randn(C, n_targets, generator=g, dtype=torch.float64) / C ** 0.5
    T = (X.double() @ A + 0.5 + 0.3 * torch.randn(N, n_targets, generator=g, dtype=torch.float64)).float()
    return X, y, T


def gram_pass(z, ld_z, B, C, t=None, ld_t=0, T=0, out=None, accumulate=0):
    """``lla_gram_pass`` on device tensors -> (out_gram [C, C], out_sum [C], out_cross [T, C], out_tsum [T], out_tsq [T]), all
    float64 and filled with 7.0 before the call; ``z`` / ``t`` are the flat storage of [B, ld_z] / [B, ld_t] rows."""
    from lossyless_amd import _lib
    L = _lib.lib()
    dev = z.device
    if out is None:
        out = tuple(torch.full(s, 7.0, dtype=torch.float64, device=dev) for s in ((C, C), (C,), (max(T, 1), C), (max(T, 2),), (max(T, 2),)))
    ws = torch.empty(int(L.lla_gram_pass_workspace_bytes(C, T)), dtype=torch.uint8, device=dev)
    with_t = t is not None
    rc = L.lla_gram_pass(_lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, ld_z, B, C,
                         _lib.ptr(t), ld_t, T, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]) if with_t else None,
                         _lib.ptr(out[3]) if with_t else None, _lib.ptr(out[4]) if with_t else None, accumulate, _lib.ptr(ws),
                         _lib.stream_ptr())
    _lib.check(rc, "lla_gram_pass")
    torch.cuda.synchronize()
    return out


def segment_sums(z, ld_z, B, C, offsets, out=None, accumulate=0):
    """``lla_segment_sums`` on a device tensor with host offsets -> out float64 [S, C] (filled with 7.0 before the call)."""
    import ctypes
    from lossyless_amd import _lib
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    S = len(off) - 1
    if out is None:
        out = torch.full((S, C), 7.0, dtype=torch.float64, device=z.device)
    rc = _lib.lib().lla_segment_sums(_lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, ld_z, B, C,
                                     off.ctypes.data_as(ctypes.c_void_p), S, _lib.ptr(out), accumulate, _lib.stream_ptr())
    _lib.check(rc, "lla_segment_sums")
    torch.cuda.synchronize()
    return out


def moments_and_bounds(Z, T=None):
    """float64 moments of rows Z [B, C] (and targets T [B, n]) -- the values the kernel sees -- with the elementwise bounds on
    |kernel - float64|, derived, not measured.  An fp32 MFMA chain is never longer than the call's B rows and chains are
    joined in double, so with gamma = (B + 2) 2^-24:
        |G - G64| <= gamma |Z|^T |Z|        |R - R64| <= gamma |T|^T |Z|
    and the sums taken in double throughout are within (B + 2) 2^-53 of their absolute sums.
    -> dict of (value, bound) for gram, sum, cross, tsum, tsq (the last three only with T)."""
    Z = Z.double()
    B = Z.shape[0]
    g32, g64 = (B + 2) * U, (B + 2) * U64
    A = Z.abs()
    out = dict(gram=(Z.T @ Z, g32 * (A.T @ A)), sum=(Z.sum(0), g64 * A.sum(0)))
    if T is not None:
        T = T.double()
        out.update(cross=(T.T @ Z, g32 * (T.abs().T @ A)), tsum=(T.sum(0), g64 * T.abs().sum(0)),
                   tsq=((T * T).sum(0), g64 * (T * T).sum(0)))
    return out


def check_moments(out, ref, C, T, what):
    """The outputs of ``gram_pass`` against ``moments_and_bounds`` -> the worst error / bound of the Gram matrix."""
    names = ("gram", "sum") + (("cross", "tsum", "tsq") if T else ())
    worst = 0.0
    for name, got in zip(names, (out[0], out[1], out[2][:T], out[3][:T], out[4][:T])):
        want, lim = ref[name]
        err = (got.cpu() - want.cpu()).abs()
        ratio = float((err / lim.cpu().clamp_min(1e-300)).max()) if err.numel() else 0.0
        assert bool((err <= lim.cpu()).all()), f"{what}: {name} error / bound = {ratio:.3g}"
        if name == "gram":
            worst = ratio
    return worst


def f32_moments_coefficient_error(X, targets, alphas, classify):
    """What fp32 accumulation of the moments does to the coefficients, measured on the CPU: the solver of the float64 twin fed
    float64 moments against the same solver fed moments accumulated in numpy float32 (``X.T @ X``, sums and cross-moments in
    fp32) -> max over alphas of max |W32 - W64| (absolute).  The GPU end-to-end tolerance is 4 x this."""
    from lossyless_amd.probe import _ridge_solve, _signed_targets
    X32 = X.numpy().astype(np.float32)
    n = float(X.shape[0])

    def moments(dtype):
        Z = X32.astype(dtype)
        G, s = Z.T @ Z, Z.sum(0, dtype=dtype)
        if classify:
            K = int(targets.max()) + 1
            Y = np.eye(K, dtype=dtype)[targets.numpy()]
            R, ts = _signed_targets(n, torch.from_numpy(s.astype(np.float64)), torch.from_numpy((Y.T @ Z).astype(np.float64)),
                                    torch.from_numpy(Y.sum(0).astype(np.float64)))
        else:
            Tt = targets.numpy().astype(dtype)
            R, ts = torch.from_numpy((Tt.T @ Z).astype(np.float64)), torch.from_numpy(Tt.sum(0, dtype=dtype).astype(np.float64))
        return torch.from_numpy(G.astype(np.float64)), torch.from_numpy(s.astype(np.float64)), R, ts

    W64, _ = _ridge_solve(n, *moments(np.float64), alphas)
    W32, _ = _ridge_solve(n, *moments(np.float32), alphas)
    return float((W32 - W64).abs().max())


def f32_moments_cv_mse_error(X, T, fold, alphas):
    """What fp32 accumulation of the per-fold moments does to the closed-form held-out MSE of a regression search, measured on
    the CPU the same way: the twin's fold fits and its SSE formula (``_ridge_fold_fits``, ``_ridge_held_out_mse``) fed per-fold
    moments accumulated in float64 against the same fed moments accumulated in numpy float32 (Gram matrix, sums, cross-moments
    and sums of squares of every fold; the total is their sum).  ``fold`` int64 [N] with ids 0 .. F-1 (-1: always trains).
    -> max over (alpha, fold) of |MSE32 - MSE64| (absolute).  The GPU tolerance is 4 x this."""
    from lossyless_amd.probe import _ridge_fold_fits, _ridge_held_out_mse
    X32, T32, f = X.numpy().astype(np.float32), T.numpy().astype(np.float32), fold.numpy()
    ids = sorted(int(v) for v in np.unique(f) if v >= 0)

    def scores(dtype):
        parts = []
        for i in ids + [-1]:
            Z, Tt = X32[f == i].astype(dtype), T32[f == i].astype(dtype)
            m = dict(n=float(len(Z)), gram=Z.T @ Z, sum=Z.sum(0, dtype=dtype), cross=Tt.T @ Z, tsum=Tt.sum(0, dtype=dtype),
                     tsq=(Tt * Tt).sum(0, dtype=dtype))
            parts.append({k: (torch.from_numpy(np.asarray(v, dtype=np.float64)) if k != "n" else v) for k, v in m.items()})
        total = {k: sum(p[k] for p in parts) for k in parts[0]}
        total["kind"] = "regress"
        held = parts[:len(ids)]
        W, b = _ridge_fold_fits(total, held, alphas, True)
        return _ridge_held_out_mse(held, W, b)

    return float((scores(np.float32) - scores(np.float64)).abs().max())
