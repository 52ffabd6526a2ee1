"""The probes' one affine-scoring helper (lossyless_amd/probe.py: ``_pack_affine`` + ``_affine_scores``) at the edges its
callers can hand it: a class count that pads to 8 columns, a last decode group of ONE row (pitch C), fp16 and fp32 rows, a row
view whose pitch is no multiple of 4 elements (fp32: the ``.contiguous()`` branch; fp16: widened into a dense copy), and
pieces smaller than a group into a reused buffer.  Scores against ``z.double() @ W.T + b`` within the bound
tests/test_gpu_probe.py holds ``decision_function`` to: gamma(C + 2) (|z| |W|^T + |b|)."""
import pytest
import torch

from probe_util import gamma

pytestmark = pytest.mark.gpu

C, K, N, GROUP = 8, 3, 9, 8              # K pads to 8 columns; groups of 8 and 1 rows


@pytest.fixture(scope="module")
def problem():
    g = torch.Generator().manual_seed(0)
    return torch.randn(N, C, generator=g), torch.randn(K, C, generator=g), torch.randn(K, generator=g)


def _want(z, W, b):
    """-> (float64 scores of the rows as stored, the elementwise bound)."""
    z, W, b = z.double().cpu(), W.double(), b.double()
    return z @ W.T + b, gamma(C + 2) * (z.abs() @ W.abs().T + b.abs())


@pytest.mark.parametrize("piece", [None, 3])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_affine_scores_of_groups(problem, dtype, strided, piece):
    from lossyless_amd.probe import _affine_scores, _pack_affine
    X, W, b = problem
    rows = X.to(dtype).cuda()
    if strided:                                            # a pitch of 10 elements
        wide = torch.zeros((N, C + 2), dtype=dtype, device="cuda")
        wide[:, :C] = rows
        rows = wide[:, :C]
        assert rows.stride(0) % 4
    w, bp, npad = _pack_affine(W, b, rows.device)
    assert npad == 8 and tuple(w.shape) == (8, C) and not bool(w[K:].any()) and not bool(bp[K:].any())
    out = torch.full((N, npad), float("nan"), device="cuda")
    buf = torch.empty((piece or 1, npad), device="cuda")
    launches = []
    for g0 in range(0, N, GROUP):
        z = rows[g0:g0 + GROUP]
        n = int(z.shape[0])
        if piece is None:
            scored = _affine_scores(z, w, bp, out[g0:g0 + n])
            launches.append(1)
        else:
            seen = []
            scored = _affine_scores(z, w, bp, buf, piece,
                                    lambda r0, S: (seen.append(r0), out[g0 + r0:g0 + r0 + S.shape[0]].copy_(S)))
            launches.append(len(seen))
            assert seen == list(range(0, n, piece))
        assert scored.dtype == torch.float32 and scored.stride(1) == 1 and (n == 1 or scored.stride(0) % 4 == 0)
        assert torch.equal(scored, z.float())
    assert launches == ([1, 1] if piece is None else [3, 1])
    want, bound = _want(rows, W, b)
    err = (out[:, :K].double().cpu() - want).abs()
    print(f"{dtype} strided {strided} piece {piece}: max err {float(err.max()):.3e}, bound there {float(bound[err == err.max()].max()):.3e}")
    assert bool((err <= bound).all())
    assert not bool(out[:, K:].any())                      # (the padding: zero weights, zero bias)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_decision_function_with_a_last_group_of_one_row(problem, dtype):
    """The same through a probe's ``decision_function``: N = 9 rows walked 8 at a time."""
    from lossyless_amd import LinearProbe
    X, W, b = problem
    rows = X.to(dtype).cuda()
    probe = LinearProbe()
    probe._set(W, b, torch.arange(K), 0, 0.0, True)
    s = probe.decision_function(rows, rows_per_pass=GROUP)
    want, bound = _want(rows, W, b)
    assert tuple(s.shape) == (N, K) and s.dtype == torch.float32
    assert bool(((s.double().cpu() - want).abs() <= bound).all())
    assert torch.equal(s, probe.decision_function(rows, rows_per_pass=N))
