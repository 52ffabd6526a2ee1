"""GPU parity, kernel by kernel, for the GEMM paths that only the RN50 tower reaches (csrc/gemm_plan.h): every call through
lla_gemm_f16_ex against a float64 reference of the same operation (torch, on the device), and bit for bit against the
one-tile-per-workgroup kernel on slices of fewer than 9000 rows ("an output does not depend on the kernel that computed it").

  B1-B6  ReLU / add + ReLU 1x1 convolutions of >= 9000 rows, N % 256 == 0: gemm_persistent_kernel, NJ = 2, whose line-assembling
         epilogue (gemm_epilogue_staged<EPI_RELU / EPI_ADDRELU>, csrc/gemm_common.h) takes the wave tiles that lie wholly inside
         M and leaves the others to the masked gemm_epilogue -- 256- and 320-row tiles, ragged and whole last row tiles, row
         pitches of A, C and the identity beyond K and N, a column offset on C, the conv3 | downsample GEMM over the
         concatenated buffer (B6)
  B7-B8  narrow outputs (ldc < N: only the first ldc columns are stored) on thousands of tiles of gemm256_f16_kernel
  C1-C3  fp16 outputs that the eight-wave kernel refuses: N > 3072 (the attention pool's K/V projection: ping-pong kernel with
         EPI_F16) and K < 128 (lock-step kernel, NJ = 1)
  C4     ... and one that it takes: a later stage's downsample convolution when it runs on its own
  D1     the attention pool's query and output projections: a handful of class rows 50 x 2048 apart on gemm_f16_kernel

Operands and bounds are the project's: A = 0.5 randn, W = 0.05 randn, bias = randn; 2^-10 |ref| + 2e-3 for the ReLU kinds
(test_gpu_rn50.py), 2^-10 |ref| + 1e-3 for EPI_F16 (test_gpu_tower_gemms.py).  The identity carries a term that depends on the
row and on the 64-column chunk, so that a neighbouring row, a swapped 16-byte chunk or a stale unit moves the output by O(1).
Every case prints its largest error-to-bound ratio before it asserts (pytest -s shows them).  Measured on an MI355X:
  B1 0.247, B1w 0.247, B2 0.396, B3 0.397, B4 0.397, B4w 0.398, B5 0.397, B6 0.327, B6t 0.329, B7 0.244, B8 0.396,
  C1 0.396, C2 0.398, C3 0.330, C4 0.389, D1 0.378
(half an fp16 unit of the largest outputs: 2^-11 of values below 2, 4 or 8 against 2^-10 |ref| + the flat term), every slice
call bit-equal to the big call, every second call bit-equal to the first.

The case table is also what tests/test_host.py::test_every_gemm_path_of_the_rn50_tower_has_a_kernel_level_case reads: every
(kernel, epilogue, tile rows) that lla_rn50_forward reaches has to appear here or in test_gpu_rn50.py."""
import ctypes

import pytest
import torch

from lossyless_amd import _lib
from tower_kernel_util import guarded as _guarded, guards_intact as _guards_intact, worst as _worst

pytestmark = pytest.mark.gpu

_GK_TILE128, _GK_TILE256, _GK_PERSIST1, _GK_PERSIST2, _GK_PP, _GK_W8 = 1, 2, 3, 4, 5, 7       # enum GemmKernel (csrc/gemm_plan.h)
_F16, _RELU, _ADDRELU = _lib.LLA_EPI_F16, _lib.LLA_EPI_RELU_F16, _lib.LLA_EPI_ADD_RELU_F16
_SENTINEL = -777.0          # no output has this value: the ReLU kinds are >= 0, the others are sums of a few units
_SLICE = 8192               # rows of the calls that the one-tile kernel takes (< 9000: kBigM)
_ROW = 50 * 2048            # the attention pool's class rows: one per image of the [n * 50][2048] token matrix

# id -> (M, N, K, lda, ldc, ldr, column offset of C, epilogue, kernel, tile rows on 256 CUs).  The row counts are the smallest
# that reach the path (tall_tiles / balanced_grid for 256 CUs); *w: the same on whole row tiles only, so that no masked tile runs.
CASES = {
    "B1": (9001, 256, 64, 64, 256, 0, 0, _RELU, _GK_PERSIST2, 256),              # one K-tile; last row tile: 41 rows
    "B1w": (9216, 256, 64, 64, 256, 0, 0, _RELU, _GK_PERSIST2, 256),
    "B2": (9001, 256, 64, 128, 320, 288, 32, _ADDRELU, _GK_PERSIST2, 256),       # every pitch beyond its matrix, C offset
    "B3": (9217, 1024, 256, 256, 1024, 1024, 0, _ADDRELU, _GK_PERSIST2, 256),    # last row tile: ONE row
    "B4": (18001, 1024, 256, 256, 1024, 1280, 0, _ADDRELU, _GK_PERSIST2, 320),   # last 320-row tile: 81 rows
    "B4w": (17920, 1024, 256, 256, 1024, 1280, 0, _ADDRELU, _GK_PERSIST2, 320),
    "B5": (9016, 2048, 512, 512, 2048, 2048, 0, _ADDRELU, _GK_PERSIST2, 320),    # layer4's conv3 at 184 images
    "B6": (9016, 512, 384, 384, 512, 0, 0, _RELU, _GK_PERSIST2, 256),            # conv3 | downsample over [main | block input]
    "B6t": (9016, 2048, 384, 384, 2048, 0, 0, _RELU, _GK_PERSIST2, 320),         # ... as wide as layer4's: 320-row tiles
    "B7": (12544, 128, 64, 64, 64, 0, 0, _RELU, _GK_TILE256, 256),               # n_store = 64
    "B8": (12545, 128, 256, 256, 32, 32, 0, _ADDRELU, _GK_TILE256, 256),         # n_store = 32, identity, ragged M
    "C1": (9001, 4096, 256, 256, 4096, 0, 0, _F16, _GK_PP, 320),                 # the shortest K of the ping-pong loop
    "C2": (9800, 4096, 2048, 2048, 4096, 0, 0, _F16, _GK_PP, 320),               # the K/V projection at 196 images
    "C3": (9001, 256, 64, 128, 256, 0, 0, _F16, _GK_PERSIST1, 256),              # layer1's downsample convolution on its own
    "C4": (9001, 512, 256, 320, 512, 0, 0, _F16, _GK_W8, 256),                   # a stage's downsample convolution on its own
    "D1": (4, 1024, 2048, _ROW, 1024, 0, 0, _F16, _GK_TILE128, 128),             # the query / output projection of a chunk of 4
}


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _plan(epi, M, N, K, lda, ldc):
    k, rows, grid = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = _lib.lib().lla_gemm_plan(epi, 0, M, N, K, lda, ldc, 0, _cus(), ctypes.byref(k), ctypes.byref(rows), ctypes.byref(grid))
    return rc, k.value, rows.value


def _first_difference(a, b):
    d = a.view(torch.int16) != b.view(torch.int16)
    return f"{int(d.sum())} elements differ, first (row, col) {d.nonzero()[:8].tolist()}"


class _Operands:
    """A [M][lda], W [N][K], bias [N] and the identity R [M][ldr] of one case (padding beyond K and N: fp16 NaN), and a caller
    of lla_gemm_f16_ex for any run of its rows that checks what must hold for every call."""

    def __init__(self, case):
        self.M, self.N, self.K, self.lda, self.ldc, self.ldr, self.coff, self.epi = CASES[case][:8]
        M, N, K = self.M, self.N, self.K
        g = torch.Generator(device="cuda").manual_seed(M * 7 + N + K)
        randn = lambda *shape: torch.randn(*shape, generator=g, device="cuda")
        self.A = torch.full((M, self.lda), float("nan"), dtype=torch.float16, device="cuda")
        self.A[:, :K] = (randn(M, K) * 0.5).half()
        self.W = (randn(N, K) * 0.05).half()
        self.bias = randn(N)
        self.stored = min(N, self.ldc)          # columns the call stores
        self.R = None
        if self.epi == _ADDRELU:
            cols = min(N, self.ldr)
            m, n = torch.arange(M, device="cuda")[:, None], torch.arange(cols, device="cuda")[None, :]
            self.R = torch.full((M, self.ldr), float("nan"), dtype=torch.float16, device="cuda")
            self.R[:, :cols] = (randn(M, cols) + ((m % 7) - 3).float() + 0.5 * ((n // 64) % 5).float()).half()

    def reference(self):
        """float64, on the device: (A[:, :K] W^T + bias) [+ R], clamped at 0 for the ReLU kinds; the stored columns."""
        s = self.stored
        ref = self.A[:, :self.K].double() @ self.W[:s].double().t() + self.bias[:s].double()
        if self.epi == _ADDRELU:
            ref += self.R[:, :s].double()
        return ref.clamp_min_(0) if self.epi in (_RELU, _ADDRELU) else ref

    def call(self, r0=0, rows=None):
        """Rows [r0, r0 + rows) as a call of their own into a fresh M x ldc buffer of sentinels between two guard blocks ->
        the stored columns [rows][stored] (a view).  Columns outside [coff, coff + stored) and the guards must stay."""
        rows = self.M - r0 if rows is None else rows
        ldc, coff = self.ldc, self.coff
        buf, C = _guarded(rows * ldc, torch.float16, _SENTINEL)
        A = self.A.view(-1)[r0 * self.lda:]
        R = None if self.R is None else _lib.ptr(self.R.view(-1)[r0 * self.ldr:])
        rc = _lib.lib().lla_gemm_f16_ex(_lib.ptr(A), self.lda, _lib.ptr(self.W), _lib.ptr(self.bias), _lib.ptr(C[coff:]), ldc, R,
                                        self.ldr, rows, self.N, self.K, self.epi, _lib.stream_ptr())
        _lib.check(rc, "lla_gemm_f16_ex")
        torch.cuda.synchronize()
        C = C.view(rows, ldc)
        assert bool((C[:, :coff] == _SENTINEL).all()) and bool((C[:, coff + self.stored:] == _SENTINEL).all()), \
            "columns outside C were written"
        assert _guards_intact(buf, _SENTINEL), "a guard block was written"
        return C[:, coff:coff + self.stored]


@pytest.mark.parametrize("case", list(CASES))
def test_rn50_gemm_paths_against_fp64_and_the_one_tile_kernel(case):
    M, N, K, lda, ldc, ldr, coff, epi, kernel, rows = CASES[case]
    # 1. the plan: the kernel this case is about (a change of selection fails here instead of testing another kernel)
    rc, got_kernel, got_rows = _plan(epi, M, N, K, lda, ldc)
    assert (rc, got_kernel) == (0, kernel), (rc, got_kernel)
    if _cus() == 256:
        assert got_rows == rows, got_rows
    op = _Operands(case)
    out = op.call()
    # 2. against float64
    ref = op.reference()
    err = (out.double() - ref).abs()
    bound = ref.abs() * 2 ** -10 + (1e-3 if epi == _F16 else 2e-3)
    w, r, col = _worst(err, bound, f"{case} ({M}, {N}, {K}) epi {epi}")
    print(f"{case}: the worst element sits in row tile {r // rows} of {-(-M // rows)} ({rows} rows), row {r % rows} of it")
    del ref, err, bound
    assert w <= 1.0, (w, r, col)
    # 3. the same bits as the one-tile kernel on runs of fewer than 9000 rows: the first 8192 and the last min(M, 8192)
    if kernel in (_GK_PERSIST1, _GK_PERSIST2, _GK_PP, _GK_W8):
        n = min(M, _SLICE)
        assert _plan(epi, n, N, K, lda, ldc)[:2] == (0, _GK_TILE256)
        for r0 in (0, M - n):
            part = op.call(r0, n)
            assert torch.equal(part.view(torch.int16), out[r0:r0 + n].view(torch.int16)), \
                f"rows {r0}..{r0 + n}: " + _first_difference(part, out[r0:r0 + n])
            del part
    # 4. a second identical call gives the same bits  (5. columns outside C and the guards: _Operands.call)
    again = op.call()
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), _first_difference(out, again)


def test_persistent_relu_path_refuses_an_output_pitch_of_8k_plus_4():
    """gemm_epilogue_staged stores 16 bytes per lane at C + m ldc + nw + 8 q: with ldc % 8 == 4 every other row is 8 bytes
    off that store's alignment.  The towers pass multiples of 32 and nothing in the project relies on what the memory
    pipeline does with such a store, so the shape is refused before any launch (csrc/gemm_plan.h) -- by the plan and by the
    entry point, for the ReLU kinds and for the fp16 epilogue of the ping-pong kernel; below 9000 rows (8-byte stores)
    the pitch stays supported, and computes the same values as pitch 320."""
    M, N, K, lda, _, ldr, _, epi = CASES["B2"][:8]
    assert _plan(epi, M, N, K, lda, 324)[0] == -1 and _plan(_RELU, M, N, K, lda, 324)[0] == -1
    assert _plan(_F16, 9001, 4096, 256, 256, 4100)[0] == -1
    assert _plan(epi, M, N, K, lda, 320)[:2] == (0, _GK_PERSIST2) and _plan(epi, 8192, N, K, lda, 324)[:2] == (0, _GK_TILE256)
    op = _Operands("B2")
    L, st = _lib.lib(), _lib.stream_ptr()
    C = torch.full((M, 324), _SENTINEL, dtype=torch.float16, device="cuda")
    for e, R in ((epi, _lib.ptr(op.R)), (_RELU, None)):
        assert L.lla_gemm_f16_ex(_lib.ptr(op.A), lda, _lib.ptr(op.W), _lib.ptr(op.bias), _lib.ptr(C), 324, R, ldr, M, N, K, e, st) == -1
    torch.cuda.synchronize()
    assert bool((C == _SENTINEL).all())
    # ... and the one-tile kernel at that pitch
    rows = 1000
    _lib.check(L.lla_gemm_f16_ex(_lib.ptr(op.A), lda, _lib.ptr(op.W), _lib.ptr(op.bias), _lib.ptr(C), 324, _lib.ptr(op.R), ldr, rows, N, K,
                                 epi, st), "lla_gemm_f16_ex")
    torch.cuda.synchronize()
    want = op.call(0, rows)
    assert torch.equal(C[:rows, :N].view(torch.int16), want.view(torch.int16)), _first_difference(C[:rows, :N], want)
    assert bool((C[:rows, N:] == _SENTINEL).all()) and bool((C[rows:] == _SENTINEL).all())


def test_big_m_refusals_launch_nothing():
    """Decided from the shape alone, C left as it was: an identity narrower than N, no identity at all, and a narrow output
    pitch with an epilogue that does not know about n_store -- all at M >= 9000."""
    M, N, K, lda, ldc, ldr, _, epi = CASES["B2"][:8]
    op = _Operands("B2")
    L, st = _lib.lib(), _lib.stream_ptr()
    C = torch.full((M, ldc), _SENTINEL, dtype=torch.float16, device="cuda")
    call = lambda ldc_, R, ldr_, e: L.lla_gemm_f16_ex(_lib.ptr(op.A), lda, _lib.ptr(op.W), _lib.ptr(op.bias), _lib.ptr(C), ldc_, R, ldr_,
                                                      M, N, K, e, st)
    assert call(ldc, _lib.ptr(op.R), N - 32, epi) == -1 and call(ldc, _lib.ptr(op.R), N - 4, epi) == -1       # ldr < N
    assert call(ldc, None, ldr, epi) == -1                                                                    # no identity
    assert call(N - 64, None, 0, _F16) == -1 and call(64, None, 0, _F16) == -1                                # ldc < N, EPI_F16
    torch.cuda.synchronize()
    assert bool((C == _SENTINEL).all())
    assert call(ldc, _lib.ptr(op.R), ldr, epi) == 0                                                           # (the case itself)
    torch.cuda.synchronize()
    assert not bool((C[:, :N] == _SENTINEL).any())
