"""Shared by the ordered-MLP tests: an exact restatement of the chain ``lla_gemm_f32_ordered`` promises (the contract in
lossyless_amd/csrc/gemm_f32_ordered.hip), the inputs that tell it from its look-alikes, and ctypes callers.

Python 3.10 has no ``math.fma``; the chain is restated in exact rational arithmetic on integers (``fractions.Fraction`` of
a float is exact, a binary32 value being a dyadic rational): ``a * w + acc`` is formed exactly and rounded ONCE to the
nearest binary32, ties to even, denormals kept, with IEEE 754's rules for the sign of a zero result.
"""
import ctypes
import math
from fractions import Fraction

import numpy as np
import torch

F32 = np.float32
MIN_NORMAL = 2.0 ** -126


def _round_f32(x, negative_zero):
    """Exact rational ``x`` -> nearest binary32 (as a Python float), ties to even; an exact zero takes the given sign."""
    if x == 0:
        return -0.0 if negative_zero else 0.0
    sign, mag = (-1.0 if x < 0 else 1.0), abs(x)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()      # 2**(e-1) <= mag < 2**(e+1)
    if mag < Fraction(2) ** e:
        e -= 1                                                         # now 2**e <= mag < 2**(e+1)
    quantum = Fraction(2) ** (max(e, -126) - 23)                       # spacing of binary32 there (denormals: 2**-149)
    q = mag / quantum
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    out = n * quantum
    assert out < Fraction(2) ** 128, "overflow is outside what these tests feed"
    return sign * float(out) if out else (-0.0 if sign < 0 else 0.0)


def fma_f32(a, w, acc):
    """``fmaf(a, w, acc)`` on binary32 values held as Python floats, exactly."""
    product_negative = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, w) < 0)
    acc_negative = math.copysign(1.0, acc) < 0
    # an exact zero sum is +0 (round to nearest) unless both addends are negative zeros / negative
    return _round_f32(Fraction(a) * Fraction(w) + Fraction(acc), product_negative and acc_negative)


def chain_reference(A, W, bias=None, relu=False):
    """The contract, element by element -> (C as float32 ndarray, smallest non-zero |intermediate acc| seen)."""
    M, K = A.shape
    N = W.shape[0]
    out = np.zeros((M, N), dtype=F32)
    tiniest = math.inf
    a_rows, w_rows = A.astype(np.float64).tolist(), W.astype(np.float64).tolist()
    for m in range(M):
        for n in range(N):
            acc = 0.0
            for k in range(K):
                acc = fma_f32(a_rows[m][k], w_rows[n][k], acc)
                if acc != 0.0:
                    tiniest = min(tiniest, abs(acc))
            if bias is not None:
                acc = fma_f32(1.0, float(bias[n]), acc)          # one rounded add
            if relu:
                acc = acc if acc > 0.0 else 0.0
            out[m, n] = acc
    return out, tiniest


def mul_then_add_reference(A, W):
    """The look-alike the chain must NOT be: every product rounded to binary32 before it is added (k ascending)."""
    acc = np.zeros((A.shape[0], W.shape[0]), dtype=F32)
    for k in range(A.shape[1]):
        acc = (acc + (A[:, k, None] * W[None, :, k]).astype(F32)).astype(F32)
    return acc


def ordered_inputs(M, N, K, seed):
    """-> (A [M,K], W [N,K], bias [N]) float32 with, besides seeded normal values:
    * element (0, 0): k = 0 gives acc = -1, k = 1 multiplies (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24, whose last bit a rounded
      product loses and a fused one keeps (2^-11 + 2^-24 against 2^-11), and the other weights of that output are zero;
    * column N-1 of the output: weights near 1e-38, so every chain there walks through denormals;
    * M > 1: row M-1 of A and row N-2 of W are +-1e-30, so element (M-1, N-2) is a chain of products that underflow to -0."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(M, K)).astype(F32)
    W = rng.normal(size=(N, K)).astype(F32)
    bias = rng.normal(size=N).astype(F32)
    A[0, 0], W[0, 0] = 1.0, -1.0
    A[0, 1] = W[0, 1] = F32(1.0 + 2.0 ** -12)
    W[0, 2:] = 0.0            # (the rest of that chain adds zeros: the element ends at 2^-11 + 2^-24)
    W[N - 1, :] = (rng.normal(size=K) * 1e-38).astype(F32)
    if M > 1:
        A[M - 1, :] = (np.abs(rng.normal(size=K)) * 1e-30 + 1e-31).astype(F32)
        W[N - 2, :] = -(np.abs(rng.normal(size=K)) * 1e-30 + 1e-31).astype(F32)
    return A, W, bias


def bits(x):
    """float32 tensor / ndarray -> int32 tensor of its bits (``torch.equal`` on these tells -0 from +0 and NaNs apart)."""
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x.contiguous()
    return t.view(torch.int32)


def P(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def host_gemm(A, W, bias, relu, lda=None, ldw=None, ldc=None, sentinel=None):
    """``lla_gemm_f32_ordered_host`` on numpy operands (views with a pitch are fine) -> C [M, N] (a view of a [M, ldc] buffer
    pre-filled with ``sentinel`` when one is given: returned whole then)."""
    from lossyless_amd import _lib
    M, K = A.shape
    N = W.shape[0]
    lda, ldw = lda or A.strides[0] // 4, ldw or W.strides[0] // 4
    ldc = ldc or N
    full = np.full((M, ldc), 0.0 if sentinel is None else sentinel, dtype=F32)
    rc = _lib.lib().lla_gemm_f32_ordered_host(P(A), lda, P(W), ldw, P(bias), P(full), ldc, M, N, K, int(relu))
    _lib.check(rc, "lla_gemm_f32_ordered_host")
    return full if sentinel is not None else full[:, :N]


def mixed_rows(B, C, seed, row_scale=2.0):
    """Seeded feature rows of mixed scale (what the synthetic hyperprior needs to use many table rows): [B, C] fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, generator=g) * torch.exp(torch.linspace(-2, 2, B))[:, None] * row_scale


def ordered_model(coded_means="scales", precision="ordered", device="cpu"):
    from lossyless_amd.rates import HRateHyperprior, synthetic_hyperprior_state_dict
    m = HRateHyperprior(512, mlp_precision=precision, coded_means=coded_means).eval()
    m.load_state_dict(synthetic_hyperprior_state_dict(0))
    m.update()
    return m.to(device)


def golden_state_dict():
    """The state dict of the committed container (tests/golden/ordered_hyperprior.*): ``synthetic_hyperprior_state_dict(0)``
    with the one tensor that is not bit-reproducible from machine to machine replaced.  Its scale biases are
    ``exp(linspace(...))`` evaluated in fp32 by torch's vectorised kernels, which differ in the last bit between CPUs
    (every other tensor, tables included, was found identical); a container is only as portable as its state dict, so
    here they are evaluated in float64, rounded once to fp32, and permuted arithmetically."""
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    sd = synthetic_hyperprior_state_dict(0)
    spread = np.exp(np.linspace(math.log(0.03), math.log(400.0), 512)).astype(F32)
    sd["z_encoder.module.8.bias"][:512] = torch.from_numpy(spread[(np.arange(512) * 37 + 11) % 512])
    return sd

