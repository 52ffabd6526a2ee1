"""GPU parity, kernel by kernel, for the GEMM paths that only the ViT tower reaches: every one against a float64 reference of
the same operation (torch, on the device), at the shapes where the code takes another path.

  B1  the residual GEMM with LayerNorm in its epilogue + its clean-up kernel (EPI_RESID_LNX, csrc/gemm_q4_kernel.h,
      through lla_gemm_resid_layernorm768 -- the sequence the tower's layer loop launches): one row tile, fewer tiles than
      CUs, the last shape of the plain walk, the first of the triple walk, three rounds; every wait policy, both directions.
  B2  strided and offset operands on the eight-wave, ping-pong, lock-step and one-tile kernels through lla_gemm_f16_ex:
      the last block's K/V projection (ldc > N, C offset by a column block) and the class-row GEMMs (lda = ldc = 50 x 768).
  B3  the one-pass LayerNorm variance (csrc/gemm_common.h ln_finish) under a row offset of up to 36 sigma.

Every test prints its largest error-to-bound ratio before it asserts (pytest -s shows them)."""
import ctypes

import pytest
import torch

from lossyless_amd import _lib
from tower_kernel_util import GUARD as _GUARD, guarded as _guarded, guards_intact as _guards_intact, worst as _worst

pytestmark = pytest.mark.gpu

_GK_TILE256, _GK_PERSIST1, _GK_PERSIST2, _GK_PP, _GK_Q4, _GK_W8 = 2, 3, 4, 5, 6, 7      # enum GemmKernel (csrc/gemm_plan.h)
_EPI_LNX = 9
_H_POISON = 0x7D5A          # an fp16 NaN: no LayerNorm output has these bits
_X_SENTINEL, _H_SENTINEL = -12345.0, -777.0


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _plan(epi, M, N, K, lda, ldc):
    k, rows, grid = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = _lib.lib().lla_gemm_plan(epi, 0, M, N, K, lda, ldc, 0, _cus(), ctypes.byref(k), ctypes.byref(rows), ctypes.byref(grid))
    return rc, k.value, rows.value, grid.value


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device="cuda")


def _layernorm_f64(x, gamma, beta):
    """Two-pass LayerNorm over 768 in float64 (mean, then the mean of the squared deviations)."""
    xd = x.double()
    mean = xd.mean(dim=1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=1, keepdim=True)
    return (xd - mean) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()


def _layernorm_kernel(x, gamma, beta):
    rows = x.shape[0]
    y = torch.empty(rows, 768, dtype=torch.float16, device="cuda")
    _lib.check(_lib.lib().lla_layernorm768(_lib.ptr(x), 768, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(y), rows,
                                           _lib.stream_ptr()), "lla_layernorm768")
    return y


# ---------------------------------------------------------------------------------------------------------------------
# B1: residual GEMM + LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
class _Lnx:
    """Operands of one (M, K) case and a caller of lla_gemm_resid_layernorm768 that keeps ONE workspace for all its calls:
    the first call finds it filled with 0xFF bytes, every later one with what the call before left there."""

    def __init__(self, M, K):
        g = _gen(M * 7 + K)
        self.M, self.K = M, K
        self.A = (_randn(g, M, K) * 0.5).half()
        self.W = (_randn(g, 768, K) * 0.05).half()
        self.bias = _randn(g, 768)
        self.gamma = 1 + 0.3 * _randn(g, 768)
        self.beta = 0.2 * _randn(g, 768)
        # every sibling's partial sums distinct: column chunk c (a column tile) offset 4 (c - 1) and scale 1 + c, row r a
        # further scale 1 + r % 7, two columns + 50: a swapped, stale or missing granule, or a neighbouring row's
        # statistics, moves h by O(1)
        chunk = torch.arange(768, device="cuda") // 256
        x0 = _randn(g, M, 768) * (1 + chunk).float() + 4.0 * (chunk - 1).float()
        x0 = x0 * (1 + torch.arange(M, device="cuda") % 7).float()[:, None]
        x0[:, 77] += 50.0
        x0[:, 500] += 50.0
        self.x0 = x0
        L = _lib.lib()
        self.ws_bytes = int(L.lla_gemm_resid_layernorm768_workspace_bytes(M))
        assert self.ws_bytes == (M // 256) * (3 * 256 * 16 + 24)
        self.ws_buf, self.ws = _guarded(self.ws_bytes, torch.uint8, 0xFF)
        self.ws.fill_(0xFF)
        self.default = None

    def call(self, wait=24000, rev=0):
        """-> (x, h) of a call on fresh outputs: x = x0, h poisoned, guards around both; asserts what must hold for every call."""
        M = self.M
        xbuf, x = _guarded(M * 768, torch.float32, _X_SENTINEL)
        hbuf, h = _guarded(M * 768, torch.float16, _H_SENTINEL)
        x, h = x.view(M, 768), h.view(M, 768)
        x.copy_(self.x0)
        h.view(torch.int16).fill_(_H_POISON)
        rc = _lib.lib().lla_gemm_resid_layernorm768(_lib.ptr(self.A), self.K, _lib.ptr(self.W), _lib.ptr(self.bias), _lib.ptr(x),
                                                    _lib.ptr(self.gamma), _lib.ptr(self.beta), _lib.ptr(h), M, self.K, wait, rev,
                                                    _lib.ptr(self.ws), _lib.stream_ptr())
        _lib.check(rc, "lla_gemm_resid_layernorm768")
        torch.cuda.synchronize()
        poisoned = h.view(torch.int16) == _H_POISON
        assert not bool(poisoned.any()), f"h not written at (row, col) {poisoned.nonzero()[:8].tolist()} ... ({int(poisoned.sum())} elements)"
        assert _guards_intact(xbuf, _X_SENTINEL) and _guards_intact(hbuf, _H_SENTINEL) and _guards_intact(self.ws_buf, 0xFF)
        return x, h

    def default_call(self):
        if self.default is None:
            self.default = self.call()
        return self.default


_LNX_CASES = {}


def _lnx_case(M, K):
    if (M, K) not in _LNX_CASES:
        _LNX_CASES[(M, K)] = _Lnx(M, K)
    return _LNX_CASES[(M, K)]


def _first_difference(a, b):
    d = (a.view(torch.int32 if a.dtype == torch.float32 else torch.int16) !=
         b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))
    return f"{int(d.sum())} elements differ, first (row, col) {d.nonzero()[:8].tolist()}"


# (M, K) -> workgroups on a 256-CU device: one row tile and the shortest K; 9 tiles over 8 XCDs; the tower's smallest slice (one
# round); 255 tiles = the last shape of the plain walk; 86 row tiles = the first triple walk (round 1 holds ONE unit); 171 row
# tiles = three rounds of 85 + 85 + 1
_LNX_SHAPES = {(256, 256): 3, (768, 768): 9, (9216, 768): 108, (9216, 3072): 108, (21760, 256): 255, (22016, 768): 256,
               (22016, 3072): 256, (43776, 256): 256}


@pytest.mark.parametrize("M,K", list(_LNX_SHAPES))
def test_resid_layernorm_gemm_against_fp64(M, K):
    """x += A W^T + b and h = LayerNorm(x) from ONE call, against float64 and against the kernels that compute the same values
    on their own.  Bounds: x as EPI_RESID in test_gpu_vit.py (1e-4 (1 + |ref|), here the smaller of the GEMM term's and the
    whole sum's), h as test_layernorm768 (fp16 output rounding: 2^-10 |ref| + 1e-3)."""
    rc, kernel, rows, grid = _plan(_EPI_LNX, M, 768, K, K, 768)
    assert (rc, kernel, rows) == (0, _GK_Q4, 256), (rc, kernel, rows)
    if _cus() == 256:
        assert grid == _LNX_SHAPES[(M, K)], grid        # (M >= 22016: exactly 256 = the triple walk; a change of selection moves this)
    c = _lnx_case(M, K)
    x, h = c.default_call()
    # 1. x against float64
    gemm = c.A.double() @ c.W.double().t() + c.bias.double()
    ref = c.x0.double() + gemm
    err = (x.double() - ref).abs()
    bound = 1e-4 * (1 + torch.minimum(ref.abs(), gemm.abs()))
    wx, r, col = _worst(err, bound, f"B1 ({M}, {K}) x")
    del gemm, ref, bound, err
    assert wx <= 1.0, (wx, r, col)
    # 2. the same bits as the residual GEMM without LayerNorm, whichever kernel that is
    x2 = c.x0.clone()
    _lib.check(_lib.lib().lla_gemm_f16(_lib.ptr(c.A), _lib.ptr(c.W), _lib.ptr(c.bias), _lib.ptr(x2), M, 768, K,
                                       _lib.LLA_EPI_RESID_F32, _lib.stream_ptr()), "lla_gemm_f16")
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), x2.view(torch.int32)), _first_difference(x, x2)
    # 3. h has the bits of the LayerNorm kernel on the x this call wrote
    h2 = _layernorm_kernel(x, c.gamma, c.beta)
    torch.cuda.synchronize()
    assert torch.equal(h.view(torch.int16), h2.view(torch.int16)), _first_difference(h, h2)
    # 4. ... and is that x's LayerNorm
    ref = _layernorm_f64(x, c.gamma, c.beta)
    err = (h.double() - ref).abs()
    assert bool(torch.isfinite(h).all())
    wh, r, col = _worst(err, ref.abs() * 2 ** -10 + 1e-3, f"B1 ({M}, {K}) h")
    assert wh <= 1.0, (wh, r, col)
    # (5. no poison left in h, guards intact: _Lnx.call)  The workspace now holds this call's words and granules: again
    x3, h3 = c.call()
    assert torch.equal(x.view(torch.int32), x3.view(torch.int32)), _first_difference(x, x3)
    assert torch.equal(h.view(torch.int16), h3.view(torch.int16)), _first_difference(h, h3)


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("wait", [24000, 0, -1, 1 << 24])
@pytest.mark.parametrize("M,K", [(768, 768), (21760, 256), (22016, 768)])
def test_resid_layernorm_gemm_wait_policies_and_directions_keep_the_bits(M, K, wait, rev):
    """Looking once, never looking (every row tile through the clean-up kernel), waiting as long as it takes (bounded: 2^24
    cycles) and walking the rows backwards: the bits of the default call, for x and for h."""
    c = _lnx_case(M, K)
    x, h = c.default_call()
    xv, hv = c.call(wait, rev)
    assert torch.equal(x.view(torch.int32), xv.view(torch.int32)), _first_difference(x, xv)
    assert torch.equal(h.view(torch.int16), hv.view(torch.int16)), _first_difference(h, hv)


def test_resid_layernorm_gemm_refuses_what_the_kernel_does_not_take():
    """Decided from the shape alone: a refused call leaves x and h alone."""
    c = _lnx_case(256, 256)
    L, st = _lib.lib(), _lib.stream_ptr()
    x = c.x0.clone()
    h = torch.zeros(256, 768, dtype=torch.float16, device="cuda")
    call = lambda M, K, lda, rev=0, x_=x, ws=c.ws: L.lla_gemm_resid_layernorm768(
        _lib.ptr(c.A), lda, _lib.ptr(c.W), _lib.ptr(c.bias), _lib.ptr(x_), _lib.ptr(c.gamma), _lib.ptr(c.beta), _lib.ptr(h), M, K, 24000,
        rev, _lib.ptr(ws), st)
    assert call(255, 256, 256) == -1 and call(0, 256, 256) == -1 and call(-256, 256, 256) == -1        # whole row tiles
    assert call(256, 192, 192) == -1 and call(256, 128, 256) == -1 and call(256, 288, 288) == -1       # K >= 256, K % 64
    assert call(256, 256, 248) == -1 and call(256, 256, 260) == -1                                     # lda >= K, lda % 8
    assert call(256, 256, 256, rev=2) == -1
    assert call(256, 256, 256, x_=x.view(-1)[1:]) == -1 and call(256, 256, 256, ws=None) == -1         # alignment, NULL
    assert L.lla_gemm_resid_layernorm768_workspace_bytes(255) == 0 and L.lla_gemm_resid_layernorm768_workspace_bytes(0) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, c.x0) and not bool(h.any())


# ---------------------------------------------------------------------------------------------------------------------
# B2: strided and offset operands through lla_gemm_f16_ex
# ---------------------------------------------------------------------------------------------------------------------
_F16, _QGELU, _RESID = _lib.LLA_EPI_F16, _lib.LLA_EPI_QUICKGELU_F16, _lib.LLA_EPI_RESID_F32
_ROW = 50 * 768      # the tower's class rows: one row per image of the [B * 50][768] token matrix

# (M, N, K, lda, ldc, column offset of C, epilogues, kernels)
_STRIDED = {
    "kv_projection_of_the_last_block": (12800, 1536, 768, 768, 2304, 768, (_F16,), (_GK_W8,)),
    "kv_projection_smallest_ragged": (9001, 256, 128, 128, 768, 256, (_F16, _QGELU), (_GK_W8,)),
    "eight_wave_lda_beyond_k": (9001, 256, 128, 192, 256, 0, (_F16,), (_GK_W8,)),
    "ping_pong_ldc_beyond_n": (9217, 768, 256, 256, 1536, 0, (_RESID,), (_GK_PP,)),
    "lock_step_ldc_beyond_n": (9001, 256, 128, 128, 512, 0, (_RESID,), (_GK_PERSIST1, _GK_PERSIST2)),
    "class_rows_130_resid": (130, 768, 768, _ROW, _ROW, 0, (_RESID,), (_GK_TILE256,)),
    "class_rows_300_resid": (300, 768, 768, _ROW, _ROW, 0, (_RESID,), (_GK_TILE256,)),
    "class_rows_300_f16": (300, 768, 768, _ROW, 3 * _ROW, 0, (_F16,), (_GK_TILE256,)),
}


@pytest.mark.parametrize("case", list(_STRIDED))
def test_gemm_ex_strided_and_offset_operands_against_fp64(case):
    """Operands and bounds of test_gemm_f16_against_fp64 (test_gpu_vit.py) with a row pitch beyond K (the padding holds NaN), a
    row pitch beyond N and a column offset on C (what the call must not touch, and a guard behind the last row, hold a
    sentinel)."""
    M, N, K, lda, ldc, coff, epis, kernels = _STRIDED[case]
    g = _gen(M * 7 + N)
    A = torch.full((M, lda), float("nan"), dtype=torch.float16, device="cuda")
    A[:, :K] = (_randn(g, M, K) * 0.5).half()
    W = (_randn(g, N, K) * 0.05).half()
    bias = _randn(g, N)
    ref = A[:, :K].double() @ W.double().t() + bias.double()
    L = _lib.lib()
    for epi in epis:
        rc, kernel, _, _ = _plan(epi, M, N, K, lda, ldc)
        assert rc == 0 and kernel in kernels, (rc, kernel)
        fp32 = epi == _RESID
        sentinel = _X_SENTINEL if fp32 else _H_SENTINEL
        buf, C = _guarded(M * ldc, torch.float32 if fp32 else torch.float16, sentinel)
        C = C.view(M, ldc)
        X0 = _randn(g, M, N) if fp32 else None
        if fp32:
            C[:, coff:coff + N] = X0
        rc = L.lla_gemm_f16_ex(_lib.ptr(A), lda, _lib.ptr(W), _lib.ptr(bias), _lib.ptr(C.view(-1)[coff:]), ldc, None, 0, M, N, K, epi,
                               _lib.stream_ptr())
        _lib.check(rc, "lla_gemm_f16_ex")
        torch.cuda.synchronize()
        out = C[:, coff:coff + N].double()
        if epi == _F16:
            want, bound = ref, ref.abs() * 2 ** -10 + 1e-3
        elif epi == _QGELU:
            want = ref * torch.sigmoid(1.702 * ref)
            bound = want.abs() * 2 ** -10 + 2e-3
        else:
            want, bound = X0.double() + ref, 1e-4 * (1 + ref.abs())
        err = (out - want).abs()
        err[torch.isnan(err)] = float("inf")          # (a NaN from A's padding is an error, not a pass)
        w, r, col = _worst(err, bound, f"B2 {case} epi {epi}")
        assert w <= 1.0, (w, r, col)
        assert bool((C[:, :coff] == sentinel).all()) and bool((C[:, coff + N:] == sentinel).all()), "columns outside C were written"
        assert _guards_intact(buf, sentinel)


# ---------------------------------------------------------------------------------------------------------------------
# B3: the one-pass variance under a row offset
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0, 4, 36])
@pytest.mark.parametrize("sigma", [0.3, 3.0])
def test_layernorm_under_a_row_offset(sigma, ratio):
    """var = Q / 768 - mean^2 in fp32 (csrc/gemm_common.h ln_finish) loses |mean|^2 / sigma^2 of its resolution: rows
    sigma randn + ratio sigma, two outlier columns, through the LayerNorm kernel and through the residual GEMM's epilogue
    (A = 0: x stays, h is its LayerNorm), against a two-pass float64 LayerNorm within the fp16 output bound 2^-10 |ref| + 1e-3.
    (A float32 restatement of the formula uses 0.46 of the bound at ratio 4, 0.51 at 36 and breaks it at 100.)"""
    M, K = 768, 256
    g = _gen(int(sigma * 10) * 100 + ratio)
    x0 = sigma * _randn(g, M, 768) + ratio * sigma
    x0[:, 77] += 20 * sigma
    x0[:, 500] += 20 * sigma
    gamma = 1 + 0.3 * _randn(g, 768)
    beta = 0.2 * _randn(g, 768)
    ref = _layernorm_f64(x0, gamma, beta)
    bound = ref.abs() * 2 ** -10 + 1e-3
    h1 = _layernorm_kernel(x0, gamma, beta)
    torch.cuda.synchronize()
    w1, r1, c1 = _worst((h1.double() - ref).abs(), bound, f"B3 sigma {sigma} ratio {ratio} layernorm768")
    A = torch.zeros(M, K, dtype=torch.float16, device="cuda")
    W = (_randn(g, 768, K) * 0.05).half()
    x = x0.clone()
    h2 = torch.empty(M, 768, dtype=torch.float16, device="cuda")
    h2.view(torch.int16).fill_(_H_POISON)
    L = _lib.lib()
    ws = torch.zeros(int(L.lla_gemm_resid_layernorm768_workspace_bytes(M)), dtype=torch.uint8, device="cuda")
    _lib.check(L.lla_gemm_resid_layernorm768(_lib.ptr(A), K, _lib.ptr(W), None, _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta),
                                             _lib.ptr(h2), M, K, 24000, 0, _lib.ptr(ws), _lib.stream_ptr()),
               "lla_gemm_resid_layernorm768")
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), x0.view(torch.int32)), "x + 0 changed x"
    err2 = (h2.double() - ref).abs()
    err2[torch.isnan(err2)] = float("inf")
    w2, r2, c2 = _worst(err2, bound, f"B3 sigma {sigma} ratio {ratio} residual GEMM epilogue")
    assert w1 <= 1.0, (w1, r1, c1)
    assert w2 <= 1.0, (w2, r2, c2)
    assert torch.equal(h1.view(torch.int16), h2.view(torch.int16)), _first_difference(h1, h2)
