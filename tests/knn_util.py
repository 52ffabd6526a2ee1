"""Shared by test_knn_probe_host.py, test_gpu_knn_probe.py and test_gpu_row_tile_walks.py: callers of ``lla_knn_pass`` /
``lla_knn_finish``, the float64 scores with the rounding bound the kernel's are held to, a brute-force search, the list
properties of a search and the votes in float64 (no test in here)."""
import numpy as np
import torch

from probe_util import U, gamma

# ulp allowances for the device's sqrtf, 1 / x and expf, in units of u = 2^-24 (1 ulp <= 2 u).  HIP documents sqrtf and the
# division as correctly rounded or within 1 ulp and expf within 1 ulp; 2 ulp each is allowed.
SQRT_U, DIV_U, EXP_U = 4.0, 4.0, 4.0


def knn_search(q, ld_q, Q, z, ld_z, n, C, k, metric, q_self=None, groups=None, labels=None, K=0, inv_T=0.0, k_out=None,
               row_base=0):
    """``lla_knn_pass`` over the rows in groups of ``groups`` (None: one call), then ``lla_knn_finish``
    -> (top_val [Q, k_out], top_idx [Q, k_out] int32, votes [Q, K] or None); ``q`` / ``z`` are the flat storage of [Q, ld_q] /
    [n, ld_z] rows on the device."""
    from lossyless_amd import _lib
    L = _lib.lib()
    dev = q.device
    k_out = k if k_out is None else k_out
    ws = torch.empty(int(L.lla_knn_pass_workspace_bytes(Q, k)), dtype=torch.uint8, device=dev)
    zt = _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32
    step = n if groups is None else groups
    acc = 0
    for g0 in range(0, n, max(step, 1)):
        g = min(step, n - g0)
        rc = L.lla_knn_pass(_lib.ptr(q), ld_q, Q, _lib.ptr(z[g0:g0 + g]), zt, ld_z, g, C, row_base + g0, k, metric,
                            _lib.ptr(q_self), acc, _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "lla_knn_pass")
        acc = 1
    val = torch.full((Q, k_out), 7.0, device=dev)
    idx = torch.full((Q, k_out), 7, dtype=torch.int32, device=dev)
    votes = torch.full((Q, K), 7.0, device=dev) if labels is not None else None
    rc = L.lla_knn_finish(Q, k, k_out, _lib.ptr(labels), K, inv_T, _lib.ptr(val), _lib.ptr(idx), _lib.ptr(votes), _lib.ptr(ws),
                          _lib.stream_ptr())
    _lib.check(rc, "lla_knn_finish")
    torch.cuda.synchronize()
    return val, idx, votes


def scores_and_bound(q, Z, metric):
    """float64 scores [Q, n] of queries q against rows Z (the values the kernel sees, any float dtype) and the elementwise
    bound on |kernel - float64| of an fp32 evaluation -- derived, not picked:

      dot      C products and C + 3 additions (four chains from zero, then their sum) in some order:
                   Ed = gamma_{C+2} |q| . |z|
      norm     ss = sum of C rounded squares in some order: relative error gamma_{C+2} (all terms positive); the square root
               halves it (bounded here by the whole) and adds SQRT_U u, the reciprocal DIV_U u:
                   Er = 1.01 (gamma_{C+2} + (SQRT_U + DIV_U) u)          r^ = r (1 + e), |e| <= Er
      cosine   s^ = fl(d^ r^):   |s^ - d r| <= r (Ed (1 + Er) (1 + u) + |d| (Er + u + Er u))
    A row of zeros scores exactly 0 under the cosine metric, on both sides."""
    q, Z = q.double(), Z.double()
    C = Z.shape[1]
    d = q @ Z.T
    Ed = gamma(C + 2) * (q.abs() @ Z.abs().T)
    if metric == 0:
        return d, Ed
    ss = (Z * Z).sum(1)
    r = torch.where(ss > 0, 1.0 / torch.sqrt(ss), torch.zeros_like(ss))[None, :]
    Er = 1.01 * (gamma(C + 2) + (SQRT_U + DIV_U) * U)
    return d * r, r * (Ed * (1 + Er) * (1 + U) + d.abs() * (Er + U + Er * U))


def brute_force(s, k, skip=None):
    """scores [Q, n] float64 -> indices [Q, k] of the k best by the keys (-score, index) (numpy lexsort); ``skip`` [Q]: one
    index per query that is left out."""
    s = s.cpu().numpy().copy()
    Q, n = s.shape
    out = np.zeros((Q, k), dtype=np.int64)
    for i in range(Q):
        order = np.lexsort((np.arange(n), -s[i]))
        if skip is not None:
            order = order[order != int(skip[i])]
        out[i] = order[:k]
    return torch.from_numpy(out)


def check_lists(val, idx, s, E, k, n, q_self, what):
    """The issue's list properties of one search against the float64 scores s and their bound E [Q, n]."""
    val64, idx64 = val.double().cpu(), idx.to(torch.int64).cpu()
    s, E = s.cpu(), E.cpu()
    Q = s.shape[0]
    skip = torch.full((Q,), -1, dtype=torch.int64) if q_self is None else q_self.to(torch.int64).cpu()
    usable = n - ((skip >= 0) & (skip < n)).to(torch.int64)
    worst = 0.0
    for i in range(Q):
        used = int(min(k, int(usable[i])))
        ids, vs = idx64[i, :used], val64[i, :used]
        assert bool((idx64[i, used:] == -1).all()) and bool(torch.isinf(val64[i, used:]).all()) \
            and bool((val64[i, used:] < 0).all()), f"{what} query {i}: unused slots"
        assert bool(((ids >= 0) & (ids < n)).all()) and ids.unique().numel() == used, f"{what} query {i}: range / unique"
        assert not bool((ids == skip[i]).any()), f"{what} query {i}: lists the row it skips"
        err, lim = (vs - s[i, ids]).abs(), E[i, ids]
        assert bool((err <= lim).all()), f"{what} query {i}: score error / bound = {float((err / lim).max()):.3g}"
        worst = max(worst, float((err / lim.clamp_min(1e-300)).max()) if used else 0.0)
        v32, i32 = val[i, :used].cpu(), ids
        assert bool(((v32[1:] < v32[:-1]) | ((v32[1:] == v32[:-1]) & (i32[1:] > i32[:-1]))).all()), f"{what} query {i}: order"
        out = torch.ones(n, dtype=torch.bool)
        out[ids] = False
        if 0 <= int(skip[i]) < n:
            out[skip[i]] = False
        if used < k:
            assert not bool(out.any()), f"{what} query {i}: a short list misses rows"
        elif bool(out.any()):
            last = ids[-1]
            assert bool((s[i, out] <= vs[-1] + E[i, out] + E[i, last]).all()), f"{what} query {i}: completeness"
    return worst


def votes64(val, idx, y, K, inv_T):
    """The votes of lists (val [Q, k] as returned, idx [Q, k], -1 = empty) in float64, and their bound for an fp32 evaluation:
    the exponent fl(fl(v_r - v_0) inv_T) carries two roundings (2.01 u |arg| on the weight), expf EXP_U u, and the serial sum of
    k terms gamma_k:   E = sum_r w_r (2.01 u |arg_r| + EXP_U u) (1 + gamma_k) + gamma_k sum_r w_r   over the ranks of the class."""
    val, idx, y = val.double().cpu(), idx.to(torch.int64).cpu(), y.to(torch.int64).cpu()
    Q, k = val.shape
    arg = (val - val[:, :1]) * inv_T
    cls = torch.where(idx >= 0, y[idx.clamp_min(0)], torch.full_like(idx, -1))
    live = (cls >= 0) & (cls < K)
    w = torch.where(live, torch.exp(torch.where(live, arg, torch.zeros_like(arg))), torch.zeros_like(arg))
    e = w * (2.01 * U * torch.where(live, arg.abs(), torch.zeros_like(arg)) + EXP_U * U) * (1 + gamma(k)) + gamma(k) * w
    onehot = (cls[:, :, None] == torch.arange(K)[None, None, :]).double()
    return (w[:, :, None] * onehot).sum(1), (e[:, :, None] * onehot).sum(1)
