"""What the minibatch trainers of this package share: the AdamW step on the host and on the device, the small ReLU network
in float64 (initialisation, forward, backward), the learning-rate schedules of the reference and the Philox stream that the
dropout masks and the rate models' noise are drawn from.  Used by the MLP probes (``probe.py``), ``bottleneck_fit.py``
and ``hyperprior_fit.py``; it imports none of them."""
import numpy as np
import torch

from . import _lib


def _mlp_init(dims, generator):
    """``weights_init`` of the reference (lossyless/helpers.py:153-178) for the Linear layers dims[l] -> dims[l + 1]:
    ``kaiming_uniform_(nonlinearity="relu")`` -- U(-b, b), b = sqrt(2) sqrt(3 / fan_in) -- on every weight, drawn in fp32 on the
    CPU from ``generator`` in layer order, and zero biases -> (weights, biases)."""
    Ws, bs = [], []
    for fan_in, fan_out in zip(dims[:-1], dims[1:]):
        bound = (2.0 ** 0.5) * (3.0 / fan_in) ** 0.5
        Ws.append(torch.empty((fan_out, fan_in), dtype=torch.float32).uniform_(-bound, bound, generator=generator))
        bs.append(torch.zeros(fan_out, dtype=torch.float32))
    return Ws, bs


class _Adam:
    """The hyper-parameters of a fit and the two bias corrections of step t, in double on the host (``lla_adamw_step``)."""

    def __init__(self, lr, weight_decay, betas, eps):
        self.lr, self.wd, self.b1, self.b2, self.eps = float(lr), float(weight_decay), float(betas[0]), float(betas[1]), float(eps)

    def corrections(self, t):
        return 1.0 - self.b1 ** t, 1.0 - self.b2 ** t


def _adamw(params, grads, moments, a, t):
    """``lla_adamw_step`` on the host: step ``t`` of AdamW with the hyper-parameters ``a`` on a list of tensors, in place;
    ``moments`` holds (m, v) per parameter."""
    bc1, bc2 = a.corrections(t)
    for p, g, (m, v) in zip(params, grads, moments):
        p.mul_(1.0 - a.lr * a.wd)
        m.copy_(a.b1 * m + (1.0 - a.b1) * g)
        v.copy_(a.b2 * v + (1.0 - a.b2) * g * g)
        p.sub_((a.lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + a.eps))


def _adamw_step(L, p, g, m, v, a, bc1, bc2, st):
    """``lla_adamw_step`` on the device: AdamW with the hyper-parameters ``a`` and the bias corrections (bc1, bc2) on the whole
    of the fp32 buffers p (parameters), g (gradients), m and v (moments), in place, on stream ``st``."""
    rc = L.lla_adamw_step(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), p.numel(), a.lr, a.b1, a.b2, a.eps, a.wd, bc1, bc2, st)
    _lib.check(rc, "lla_adamw_step")


def _mlp_forward(Ws, bs, x, pre=None):
    """-> (output, [x, h_1, ..., h_L]): h = relu(h W^T + b) (``lla_gemm_f32``, relu = 1), then the last Linear.  ``pre``, a
    list, receives the hidden pre-activations."""
    hs = [x]
    for W, b in zip(Ws[:-1], bs[:-1]):
        a = hs[-1] @ W.T + b
        if pre is not None:
            pre.append(a)
        hs.append(torch.where(a > 0, a, torch.zeros((), dtype=a.dtype)))
    return hs[-1] @ Ws[-1].T + bs[-1], hs


def _mlp_backward(Ws, hs, delta, below=False):
    """The output's gradient -> (dW per layer, db per layer, the input's gradient -- computed only with ``below``, else None):
    ``lla_gemm_f32_tn``, and ``lla_gemm_f32_nn`` with the ReLU mask of the layer below."""
    gW, gb = [None] * len(Ws), [None] * len(Ws)
    for l in range(len(Ws) - 1, -1, -1):
        gW[l], gb[l] = delta.T @ hs[l], delta.sum(0)
        if l > 0:
            delta = torch.where(hs[l] > 0, delta @ Ws[l], torch.zeros((), dtype=delta.dtype))
    return gW, gb, delta @ Ws[0] if below else None


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on the CPU: ``counter`` [..., 4] and ``key`` [..., 2] of 32-bit words (anything
    numpy broadcasts) -> uint32 [..., 4].  The definition csrc/batchnorm.hip draws its dropout masks from."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def dropout_keep(seed, step, layer, rows, cols, p):
    """The keep pattern of ``lla_bn_relu_dropout_fwd`` -> bool tensor [rows, cols] (``cols % 4 == 0``): the quad of columns
    j .. j + 3 of row i takes the four words of Philox4x32-10 with key (seed_lo, seed_hi) and counter (e_lo, e_hi, step,
    layer), e = (i cols + j) / 4; a word w gives u = (w >> 8) 2^-24 and the element is kept iff u >= float32(p)."""
    if cols % 4:
        raise ValueError("cols must be a multiple of 4")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    e = np.arange(rows * cols // 4, dtype=np.uint64)
    counter = np.stack([e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), np.full_like(e, int(step) & 0xFFFFFFFF),
                        np.full_like(e, int(layer) & 0xFFFFFFFF)], -1)
    words = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    u = (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return torch.from_numpy((u >= np.float32(p)).reshape(rows, cols))


def _dropout_scale(p):
    """s = (float)(1 / (1 - (double)p)), as a Python float holding the fp32 value."""
    return float(np.float32(1.0 / (1.0 - float(p))))


def lr_schedule(scheduler, lr, epochs, decay_factor=100, k_steps=3):
    """The learning rate of every epoch -> list of ``epochs`` doubles, as lossyless/helpers.py:536-545 builds the schedulers
    and ``torch.optim.lr_scheduler`` steps them once per epoch (the chained form: each rate is the previous one times a
    factor).  None: constant.  "unifmultistep": ``MultiStepLR`` with milestones ``(epochs // (k_steps + 1)) i``, i = 1 ..
    k_steps, and ``gamma = (1 / decay_factor) ** (1 / k_steps)``.  "expdecay": ``ExponentialLR`` with
    ``gamma = (1 / decay_factor) ** (1 / epochs)``."""
    lr, epochs = float(lr), int(epochs)
    if scheduler is None:
        return [lr] * epochs
    if scheduler == "unifmultistep":
        delta = epochs // (k_steps + 1)
        milestones = [delta * i for i in range(1, k_steps + 1)]
        gamma = (1 / decay_factor) ** (1 / k_steps)
        out = []
        for e in range(epochs):
            n = milestones.count(e)
            lr = lr * gamma ** n if n else lr
            out.append(lr)
        return out
    if scheduler == "expdecay":
        gamma = (1 / decay_factor) ** (1 / epochs)
        out = []
        for e in range(epochs):
            lr = lr * gamma if e else lr
            out.append(lr)
        return out
    raise ValueError(f"scheduler={scheduler!r} is not built: None, 'unifmultistep' or 'expdecay'")
