"""Shared by test_kmeans_probe_host.py and test_gpu_kmeans_probe.py: a caller of ``lla_kmeans_pass``, the float64 scores with
the rounding bounds its outputs are held to, and the margin condition under which the device fit and its float64 twin must
agree label for label (no test in here)."""
import torch

from knn_util import DIV_U, SQRT_U
from probe_util import U, gamma

U64 = 2.0 ** -53


def kmeans_pass(z, ld_z, B, C, W, b, K, ld_w, metric, sums=True, out=None, accumulate=0):
    """``lla_kmeans_pass`` on device tensors -> (out_assign int32 [B], out_dist [B], out_sum [K, ld_w], out_count float64 [K],
    out_stats float64 [2]); ``z`` / ``W`` are the flat storage of [B, ld_z] / [K, ld_w] rows.  ``sums=False``: out_sum is NULL
    and the count and statistics buffers are passed all the same (they must come back untouched)."""
    from lossyless_amd import _lib
    L = _lib.lib()
    dev = W.device
    if out is None:
        out = (torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev), torch.full((max(B, 1),), 7.0, device=dev),
               torch.full((K, ld_w), 7.0, device=dev), torch.full((K,), 7.0, dtype=torch.float64, device=dev),
               torch.full((2,), 7.0, dtype=torch.float64, device=dev))
    ws = torch.empty(int(L.lla_kmeans_pass_workspace_bytes(C, K)), dtype=torch.uint8, device=dev)
    rc = L.lla_kmeans_pass(_lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, ld_z, B, C, _lib.ptr(W),
                           _lib.ptr(b), K, ld_w, metric, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]) if sums else None,
                           _lib.ptr(out[3]), _lib.ptr(out[4]), accumulate, _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "lla_kmeans_pass")
    torch.cuda.synchronize()
    return out


def scores_and_bound(Z, W, b, metric):
    """float64 quantities of rows Z [B, C] against the affine scores of W [K, C], b [K] (the values the kernel sees, any float
    dtype), and the elementwise bounds on |kernel - float64| of an fp32 evaluation -- derived, not picked (the symbols of
    knn_util.scores_and_bound):

      dot      C products and C + 3 additions in some order:     Ed = gamma_{C+2} |z| . |W_k|
      n2       C rounded squares added in some order:            En = gamma_{C+2} n2
      r        1 / sqrt(n2):  r^ = r (1 + e), |e| <= Er = 1.01 (gamma_{C+2} + (SQRT_U + DIV_U) u)
      metric 0   s^ = fl(d^ + b):          Es = Ed + u (|d| + Ed + |b|)
      metric 1   t^ = fl(d^ r^):           Et = r (Ed (1 + Er) (1 + u) + |d| (Er + u + Er u))
                 s^ = fl(t^ + b):          Es = Et + u (|t| + Et + |b|)
    -> dict(s [B, K], Es [B, K], n2 [B], En [B], w [B] (the row weight: 1, or r), Ew (its relative bound: 0, or Er))."""
    Z, W, b = Z.double(), W.double(), b.double()
    C = Z.shape[1]
    d = Z @ W.T
    Ed = gamma(C + 2) * (Z.abs() @ W.abs().T)
    n2 = (Z * Z).sum(1)
    En = gamma(C + 2) * n2
    if metric == 0:
        return dict(s=d + b, Es=Ed + U * (d.abs() + Ed + b.abs()), n2=n2, En=En, w=torch.ones_like(n2), Ew=0.0)
    r = torch.where(n2 > 0, 1.0 / torch.sqrt(n2), torch.zeros_like(n2))
    Er = 1.01 * (gamma(C + 2) + (SQRT_U + DIV_U) * U)
    t = d * r[:, None]
    Et = r[:, None] * (Ed * (1 + Er) * (1 + U) + d.abs() * (Er + U + Er * U))
    return dict(s=t + b, Es=Et + U * (t.abs() + Et + b.abs()), n2=n2, En=En, w=r, Ew=Er)


def dist_and_bound(ref, a, metric):
    """float64 dist of every row at the assignment ``a`` (int64 [B]) and its bound:
      metric 0   fl(n2^ - 2 s^) (2 s^ is exact), then max(0, .), which is 1-Lipschitz:   En + 2 Es + u (n2 + En + 2 |s| + 2 Es)
      metric 1   fl(1 - s^):                                                            Es + u (1 + |s| + Es)"""
    s = torch.gather(ref["s"], 1, a[:, None])[:, 0]
    Es = torch.gather(ref["Es"], 1, a[:, None])[:, 0]
    if metric == 0:
        return (ref["n2"] - 2 * s).clamp_min(0.0), ref["En"] + 2 * Es + U * (ref["n2"] + ref["En"] + 2 * s.abs() + 2 * Es)
    return 1.0 - s, Es + U * (1 + s.abs() + Es)


def check_assignment(ref, a, what=""):
    """The device's a_i is an argmax up to the scores' rounding: s[a_i] >= s[k] - Es[a_i] - Es[k] for every k (never more than
    the issue's 2 E), and it IS the float64 argmax wherever the gap to the runner-up exceeds twice the row's largest bound.
    -> the number of rows inside that margin."""
    s, Es = ref["s"], ref["Es"]
    K = s.shape[1]
    assert bool(((a >= 0) & (a < K)).all()), f"{what}: an assignment outside [0, K)"
    sa, Ea = torch.gather(s, 1, a[:, None]), torch.gather(Es, 1, a[:, None])
    assert bool((sa >= s - Ea - Es).all()), f"{what}: an assigned score below the best by more than the bound"
    inside = margin_inside(s, 2 * Es.amax(1))
    want = first_argmax(s)
    assert torch.equal(a[~inside], want[~inside]), f"{what}: not the float64 argmax outside the margin"
    return int(inside.sum())


def first_argmax(s):
    """argmax over the columns, the lowest index among equals (written out: torch.argmax promises no order)."""
    K = s.shape[1]
    at = torch.arange(K, device=s.device)[None, :].expand_as(s)
    return torch.where(s == s.amax(1, keepdim=True), at, torch.full_like(at, K)).amin(1)


def margin_inside(s, margin):
    """rows whose best float64 score leads the runner-up by no more than ``margin`` [B] (K = 1: none)."""
    if s.shape[1] < 2:
        return torch.zeros(s.shape[0], dtype=torch.bool, device=s.device)
    top = s.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) <= margin


def sums_and_bound(Z, ref, a, K):
    """float64 sums S [K, C], counts [K] of the assignment ``a`` and the bound on the kernel's fp32 sums: n_k terms w_i z_ic
    (the product is exact inside the fma; w^ carries Ew) added in some order -- walkers, the ordered reduction and the
    accumulation over calls are all additions of that one sum, and a zero adds exactly nothing:
        (gamma_{n_k + 2} + Ew (1 + gamma_{n_k + 2})) sum_i |w_i z_ic|."""
    Z = Z.double()
    wz = Z * ref["w"][:, None]
    S = torch.zeros((K, Z.shape[1]), dtype=torch.float64, device=Z.device).index_add_(0, a, wz)
    A = torch.zeros((K, Z.shape[1]), dtype=torch.float64, device=Z.device).index_add_(0, a, wz.abs())
    cnt = torch.bincount(a, minlength=K).double()
    g = gamma(cnt + 2)[:, None]
    return S, cnt, (g + ref["Ew"] * (1 + g)) * A


def check_totals(Z, ref, out, K, C, metric, what=""):
    """out_sum, out_count and out_stats of a call (or of accumulated calls) against float64 at the device's own
    assignment.  The statistics are double sums of fp32 values: the terms' own bounds, + gamma64_{B + 512} of their size."""
    a = out[0].to(torch.int64)[:Z.shape[0]]
    S, cnt, ES = sums_and_bound(Z, ref, a, K)
    err = (out[2][:, :C].double() - S).abs()
    assert bool((err <= ES).all()), f"{what}: sums error / bound = {float((err / ES.clamp_min(1e-300)).max()):.3g}"
    assert torch.equal(out[3], cnt), f"{what}: counts"
    d64, Ed = dist_and_bound(ref, a, metric)
    g64 = (Z.shape[0] + 512) * U64
    for got, want, lim in ((out[4][0], d64, Ed), (out[4][1], ref["n2"], ref["En"])):
        bound = float(lim.sum()) + g64 * float((want.abs() + lim).sum())
        assert abs(float(got) - float(want.sum())) <= bound, f"{what}: stats off by {abs(float(got) - float(want.sum())):.3g} > {bound:.3g}"
    return float((err / ES.clamp_min(1e-300)).max())


# ------------------------------------------------------------------ the fit against its twin
def centre_bound(Z, a, centres):
    """Elementwise bound [K, C] on |device centre - float64 mean of the members| when the labels agree: the fp32 sum's bound
    over n_k (w = 1: sums_and_bound with Ew = 0) and the rounding of the centre to fp32."""
    Z = Z.double()
    K = centres.shape[0]
    A = torch.zeros((K, Z.shape[1]), dtype=torch.float64, device=Z.device).index_add_(0, a, Z.abs())
    cnt = torch.bincount(a, minlength=K).double().clamp_min(1.0)
    return gamma(cnt + 2)[:, None] * A / cnt[:, None] * (1 + U) + U * centres.double().abs()


def twin_margins(Z, init, max_iter=100):
    """Lloyd's iterations of the float64 twin on rows Z (Euclidean, tol = 0) from ``init``, watching the condition under which
    the device run must agree with it label for label: at every iteration, a row is *inside the margin* when its two best
    float64 scores differ by no more than twice (the fp32 score bound Es against the twin's centres + what the device's
    centres may differ by: |z| . dc + |c| . dc + the rounding of b, dc = centre_bound).  By induction over the iterations: with no
    row inside, the labels agree, so the device's centres are within dc of the twin's, and so on.
    -> (labels, n_iter, the largest fraction of rows inside the margin, whether a cluster ever ran empty)."""
    from lossyless_amd.probe import _Rows, _TwinKMeans, _lloyd
    Z = Z.double()
    rows = _Rows(Z, 1 << 30, False)
    engine = _TwinKMeans(rows, init.shape[0], False)
    worst, emptied = [0.0], [False]
    walk = engine.walk

    def watched(centres, sums):
        out = walk(centres, sums)
        a = out[0]
        b = engine.bias(centres)
        ref = scores_and_bound(Z, centres, b, 0)
        dc = centre_bound(Z, a, centres)          # (of the PREVIOUS labels' sums; the current ones' differ by a rounding)
        shift = Z.abs() @ dc.T + (centres.abs() * dc).sum(1) + U * b.abs()
        inside = margin_inside(ref["s"], 2 * (ref["Es"] + shift).amax(1))
        worst[0] = max(worst[0], float(inside.double().mean()))
        if sums:
            emptied[0] = emptied[0] or bool((out[3] == 0).any())
        return out

    engine.walk = watched
    run = _lloyd(engine, rows, init.double(), False, max_iter, 0.0)
    return run["labels"], run["n_iter"], worst[0], emptied[0]
