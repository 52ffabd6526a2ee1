"""``BottleneckFit`` -- train a factorized rate point (``HRateFactorizedPrior``) on frozen features, on the device.

The reference makes its hub checkpoints with ``main.py`` and ``config/featurizer/bottleneck_clip_lossyZ*.yaml``: the CLIP
encoder is frozen, the distortion is ``lossy_Z`` with ``p_norm: 1`` (lossyless/distortions.py:408-449) and
``HRateFactorizedPrior`` (lossyless/rates.py:509-564) learns ``scaling``, ``biasing`` and the ``EntropyBottleneck``
parameters -- 63 numbers per channel -- under ``loss = mean dist + beta_t mean rate``
(lossyless/learnable_compressors.py:241-275), with a second optimiser on the quantiles' auxiliary loss (:277-303, :370-410).
This module is that loop for a matrix of features: a step is ``lla_eb_train_pass`` (forward, noise and backward of the whole
minibatch: csrc/eb_train.hip), ``lla_eb_aux_grad`` and two ``lla_adamw_step`` calls.  include/lossyless_amd.h states the
mathematics.

CPU data runs the float64 twin below instead, as every estimator of this package does: the same formulas written out by hand in
torch (NO autograd: the backward is the kernel's, line for line), the same noise, the same step order.  The tests hold the
twin to torch autograd and the kernels to the twin.

Not built: the encoder's training, the other distortions, ``HRateEstimator.reset_parameters``' ``weights_init`` (the
module's own initialisation is kept), lightning's logging.  The hyperprior's training is hyperprior_fit.py.
"""
import math

import numpy as np
import torch

from . import _lib
from ._train import _Adam, _adamw, _adamw_step, lr_schedule, philox4x32_10
from .rates import BASE_LOG, HRateFactorizedPrior

FILTERS = (3, 3, 3, 3)
N_MAT, N_BIAS, N_FAC = 33, 13, 12
N_NET = N_MAT + N_BIAS + N_FAC          # 58 numbers of a channel's cumulative network
N_MAIN = N_NET + 2                      # ... of the main optimiser: scaling, biasing, the network
NOISE_TAG = 0x6E6F6973
LIK_BOUND = 1e-9
_NET_NAMES = [f"_matrix{i}" for i in range(5)] + [f"_bias{i}" for i in range(5)] + [f"_factor{i}" for i in range(4)]


def hyperprior_noise(seed, step, rows, cols, tag=NOISE_TAG):
    """The noise of ``lla_eb_train_pass`` and ``lla_gaussian_train_pass`` (``tag`` 0x6e6f6973) and of ``lla_eb_side_pass``
    (``hyperprior_fit.SIDE_TAG``) -> fp32 tensor [rows, cols] on the CPU, any ``cols``: element f = i cols + c is word f % 4 of
    Philox4x32-10 with key (seed_lo, seed_hi) and counter (f / 4 lo, f / 4 hi, step, tag), as
    ``u = float32(word >> 8) 2^-24 - 0.5`` in [-0.5, 0.5).  The ONE implementation of the stream the kernels are held to."""
    seed, n = int(seed) & 0xFFFFFFFFFFFFFFFF, int(rows) * int(cols)
    e = np.arange(-(-n // 4), dtype=np.uint64)
    counter = np.stack([e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), np.full_like(e, int(step) & 0xFFFFFFFF),
                        np.full_like(e, int(tag) & 0xFFFFFFFF)], -1)
    words = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).reshape(-1)[:n]
    u = (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) - np.float32(0.5)
    return torch.from_numpy(u.reshape(int(rows), int(cols)))


def bottleneck_noise(seed, step, rows, cols):
    """The noise of ``lla_eb_train_pass`` -> fp32 tensor [rows, cols] on the CPU (``cols % 4 == 0``): element (i, c) is word
    ``c % 4`` of Philox4x32-10 with key (seed_lo, seed_hi) and counter (e_lo, e_hi, step, 0x6e6f6973), e = (i cols + c) / 4,
    as ``u = float32(word >> 8) 2^-24 - 0.5`` in [-0.5, 0.5).  The definition the kernel is held to; :func:`hyperprior_noise`
    restricted to the widths ``lla_eb_train_pass`` takes."""
    if cols % 4:
        raise ValueError("cols must be a multiple of 4")
    return hyperprior_noise(seed, step, rows, cols)


def beta_schedule(beta, total_steps, mode="linear"):
    """beta_t of every step -> list of ``total_steps`` doubles: lossyless/helpers.py ``Annealer(1e-5 beta, beta,
    ceil(total_steps / 10), mode)`` read at ``n_update_calls = t`` (lossyless/learnable_compressors.py:39-46, :246)."""
    if mode not in ("linear", "constant"):
        raise ValueError(f"beta_anneal={mode!r} is not built: 'linear' or 'constant'")
    beta, n = float(beta), math.ceil(total_steps / 10)
    if mode == "constant":
        return [beta] * total_steps
    first = beta * 1e-5
    factor = (beta - first) / n
    return [first + factor * t if t < n else beta for t in range(total_steps)]


def pack_network(eb, dtype=torch.float64):
    """The 58 numbers per channel of an ``EntropyBottleneck`` -> [58, C] in the order of ``lla_eb_train_pass``'s ``params``."""
    return torch.cat([getattr(eb, n).detach().to("cpu", dtype).reshape(eb.channels, -1).t() for n in _NET_NAMES], 0).contiguous()


def unpack_network_(eb, net):
    """Inverse of :func:`pack_network`, in place."""
    at = 0
    with torch.no_grad():
        for n in _NET_NAMES:
            p = getattr(eb, n)
            k = p[0].numel()
            p.copy_(net[at:at + k].t().reshape(p.shape).to(p.device, p.dtype))
            at += k


# ------------------------------------------------------------------------------------------ the float64 twin of the kernels
def _twin_net(net):
    """[58, C] -> (softplus(matrix) [33, C], bias [13, C], tanh(factor) [12, C]); softplus(m) = max(m, 0) + log1p(exp(-|m|))."""
    M = net[:N_MAT]
    return torch.clamp(M, min=0) + torch.log1p(torch.exp(-M.abs())), net[N_MAT:N_MAT + N_BIAS], torch.tanh(net[N_MAT + N_BIAS:])


def _twin_forward(sp, b, tf, x):
    """eb_forward of csrc/eb_train.hip on x [B, C] -> (L(x), activations)."""
    h, t = [], []
    pre = [sp[j] * x + b[j] for j in range(3)]
    t.append([torch.tanh(p) for p in pre])
    h.append([pre[j] + tf[j] * t[0][j] for j in range(3)])
    for k in range(1, 4):
        m = sp[3 + 9 * (k - 1):3 + 9 * k]
        pre = [((m[3 * j] * h[k - 1][0] + m[3 * j + 1] * h[k - 1][1]) + m[3 * j + 2] * h[k - 1][2]) + b[3 * k + j] for j in range(3)]
        t.append([torch.tanh(p) for p in pre])
        h.append([pre[j] + tf[3 * k + j] * t[k][j] for j in range(3)])
    out = ((sp[30] * h[3][0] + sp[31] * h[3][1]) + sp[32] * h[3][2]) + b[12]
    return out, (x, h, t)


def _twin_backward(sp, tf, act, g, acc=None):
    """eb_backward: g dL/dx, and (``acc`` = (sp, b, tf) accumulators [., C]) the row sums of g times the derivatives."""
    x, h, t = act
    add = (lambda buf, k, v: buf[k].add_(v.sum(0))) if acc is not None else (lambda *a: None)
    a_sp, a_b, a_tf = acc if acc is not None else (None, None, None)
    dh = [g * sp[30 + i] for i in range(3)]
    for i in range(3):
        add(a_sp, 30 + i, g * h[3][i])
    add(a_b, 12, g)
    for k in (3, 2, 1):
        da = [dh[j] * (1 + tf[3 * k + j] * (1 - t[k][j] * t[k][j])) for j in range(3)]
        for j in range(3):
            add(a_tf, 3 * k + j, dh[j] * t[k][j])
            add(a_b, 3 * k + j, da[j])
            for i in range(3):
                add(a_sp, 3 + 9 * (k - 1) + 3 * j + i, da[j] * h[k - 1][i])
        m = sp[3 + 9 * (k - 1):3 + 9 * k]
        dh = [(m[i] * da[0] + m[3 + i] * da[1]) + m[6 + i] * da[2] for i in range(3)]
    dx = 0
    for j in range(3):
        da = dh[j] * (1 + tf[j] * (1 - t[0][j] * t[0][j]))
        add(a_tf, j, dh[j] * t[0][j])
        add(a_b, j, da)
        add(a_sp, j, da * x)
        dx = dx + sp[j] * da
    return dx


def _sigmoid_diff(a, b):
    """sigmoid(a) - sigmoid(b) by the header's formula (a + b <= 0)."""
    ea, eb = torch.exp(-a.abs()), torch.exp(-b.abs())
    d = a - b
    tail = torch.where(d >= 0, -(ea * torch.expm1(-d.abs())), eb * torch.expm1(-d.abs())) / ((1 + ea) * (1 + eb))
    sa = torch.where(a <= 0, ea / (1 + ea), 1 / (1 + ea))
    sb = torch.where(b <= 0, eb / (1 + eb), 1 / (1 + eb))
    return torch.where((a <= 0) & (b <= 0), tail, sa - sb)


def _sigmoid_slope(t):
    e = torch.exp(-t.abs())
    return e / ((1 + e) * (1 + e))


def twin_likelihood(net, v):
    """eb_lik_step and eb_store_grads of csrc/eb_net.h in the dtype of ``net`` [58, C] at v [B, C] (noise already added) ->
    (d rate / dv [B, C], d rate / d net [58, C], rate = sum -log lik).  Backward by hand; the likelihood of ``twin_pass`` and
    of ``hyperprior_fit.twin_side_pass``."""
    sp, b, tf = _twin_net(net)
    lower, act_lo = _twin_forward(sp, b, tf, v - 0.5)
    upper, act_up = _twin_forward(sp, b, tf, v + 0.5)
    sgn = -torch.sign(lower + upper)
    a, bb = sgn * upper, sgn * lower
    diff = _sigmoid_diff(a, bb)
    lik = diff.abs().clamp(min=LIK_BOUND)
    gl = -1 / lik * torch.sign(diff) * sgn
    acc = (torch.zeros_like(sp), torch.zeros_like(b), torch.zeros_like(tf))
    dv = _twin_backward(sp, tf, act_up, gl * _sigmoid_slope(a), acc) + _twin_backward(sp, tf, act_lo, -gl * _sigmoid_slope(bb), acc)
    M = net[:N_MAT]
    e = torch.exp(-M.abs())                 # the chain rule through softplus (its derivative: the sigmoid) and tanh
    grads = torch.cat([acc[0] * torch.where(M <= 0, e / (1 + e), 1 / (1 + e)), acc[1], acc[2] * (1 - tf * tf)], 0)
    return dv, grads, -torch.log(lik).sum()


def twin_pass(z, main, u):
    """``lla_eb_train_pass`` in the dtype of ``main`` [60, C] (rows: scaling, biasing, the 58 of the network) on rows z [B, C]
    and noise u [B, C] -> (grads [2, 60, C]: of sum dist, of sum rate; sum dist; sum rate).  Backward by hand."""
    dt = main.dtype
    z, u = z.to(dt), u.to(dt)
    s, bz = main[0], main[1]
    es, ems = torch.exp(s), torch.exp(-s)
    y = (z + bz) * es
    dv, g_net, rate = twin_likelihood(main[2:], y + u)
    r = u * ems
    d = r + 1e-6
    grads = torch.zeros((2,) + tuple(main.shape), dtype=dt)
    grads[0, 0] = (-torch.sign(d) * r).sum(0)
    grads[1, 0] = (dv * y).sum(0)
    grads[1, 1] = (dv * es).sum(0)
    grads[1, 2:] = g_net
    return grads, d.abs().sum(), rate


def twin_aux(net, q, target):
    """``lla_eb_aux_grad`` in the dtype of ``net`` [58, C]: quantiles q [C, 3], target [3] -> (grad_q [C, 3], aux)."""
    sp, b, tf = _twin_net(net)
    out, act = _twin_forward(sp, b, tf, q.t().to(net.dtype))          # [3, C]: a "row" per quantile
    r = out - target.to(net.dtype)[:, None]
    dx = _twin_backward(sp, tf, act, torch.ones_like(out))
    return (torch.sign(r) * dx).t().contiguous(), r.abs().sum()


class _Engine:
    """What the four engines of this module and of hyperprior_fit.py share: the two optimisers and the step count, the log of
    an epoch's steps (``width`` doubles a step) and, on a device, the slots the kernels write those sums to (read once per
    epoch: one synchronisation) and the rows of a minibatch as the library reads them."""

    def __init__(self, width, adam, adam_coder, seed, device=None, max_batch=0, steps_per_epoch=0):
        self.adam, self.adam_coder, self.seed, self.t = adam, adam_coder, int(seed), 0
        self.width, self.log, self.n_log, self.sums = width, [], 0, None
        if device is not None:
            self.L, self.dev, self.rows = _lib.lib(), torch.device(device), max(int(max_batch), 1)
            self.sums = torch.zeros((max(int(steps_per_epoch), 1), width), dtype=torch.float64, device=self.dev)

    def _minibatch(self, z, C):
        """-> (z in fp16 or fp32 with a unit column stride, its ``LLA_Z_*`` code, its pitch), for the epoch's next slot."""
        B = z.shape[0]
        if B > self.rows or self.n_log >= self.sums.shape[0]:
            raise ValueError("a minibatch larger, or an epoch longer, than the engine was sized for")
        if z.dtype not in (torch.float16, torch.float32):
            z = z.float()
        if z.stride(1) != 1 or (B > 1 and z.stride(0) < C):
            z = z.contiguous()
        return z, _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, z.stride(0) if B > 1 else C

    def epoch_log(self):
        """-> [steps, width] doubles, the sums of the steps since the last call."""
        if self.sums is None:
            out, self.log = np.asarray(self.log, dtype=np.float64).reshape(-1, self.width), []
        else:
            out, self.n_log = self.sums[:self.n_log].cpu().numpy().copy(), 0
        return out


class _TwinEngine(_Engine):
    """One training step in float64 on the host: the CPU path of ``BottleneckFit`` and the oracle of its GPU tests.  A step's
    log: sum dist, sum rate, aux."""

    def __init__(self, main, q, target, adam, adam_coder, seed):
        super().__init__(3, adam, adam_coder, seed)
        self.main, self.q, self.target = main.double().clone(), q.double().clone(), target.double()
        self.C = self.main.shape[1]
        self.mom = [(torch.zeros_like(self.main), torch.zeros_like(self.main))]
        self.mom_q = [(torch.zeros_like(self.q), torch.zeros_like(self.q))]

    def step(self, z, step, beta_t):
        B = z.shape[0]
        grads, dist, rate = twin_pass(z.detach().cpu(), self.main, bottleneck_noise(self.seed, step, B, self.C))
        self.t += 1
        _adamw([self.main], [(grads[0] + beta_t * grads[1]) / B], self.mom, self.adam, self.t)
        gq, aux = twin_aux(self.main[2:], self.q, self.target)
        _adamw([self.q], [gq], self.mom_q, self.adam_coder, self.t)
        self.log.append((float(dist), float(rate), float(aux)))

    def state(self):
        return self.main.clone(), self.q.clone()


class _DeviceEngine(_Engine):
    """The same step on the GPU: fp32 flat buffers, ``lla_eb_train_pass`` + ``lla_eb_aux_grad`` + 2 x ``lla_adamw_step``."""

    def __init__(self, main, q, target, adam, adam_coder, seed, device, max_batch, steps_per_epoch):
        super().__init__(3, adam, adam_coder, seed, device, max_batch, steps_per_epoch)
        f = lambda t: t.to(self.dev, torch.float32).contiguous()
        self.main, self.q, self.target = f(main), f(q), f(target)
        self.C = self.main.shape[1]
        if self.C % 4:
            raise ValueError("the device engine needs a channel count that is a multiple of 4")
        z = lambda t: torch.zeros_like(t)
        self.g, self.m, self.v = z(self.main), z(self.main), z(self.main)
        self.gq, self.mq, self.vq = z(self.q), z(self.q), z(self.q)
        self.raw = torch.zeros((2,) + tuple(self.main.shape), dtype=torch.float32, device=self.dev)
        self.ws = torch.empty(max(int(self.L.lla_eb_train_pass_workspace_bytes(self.rows, self.C)), 16), dtype=torch.uint8,
                              device=self.dev)

    def step(self, z, step, beta_t):
        B, C, L = z.shape[0], self.C, self.L
        z, code, ldz = self._minibatch(z, C)
        _lib.require_cuda(self.main, "parameters")
        slot = self.sums[self.n_log]
        with torch.cuda.device(self.dev):
            st = _lib.stream_ptr(self.dev)
            rc = L.lla_eb_train_pass(_lib.ptr(z), code, ldz, B, C, _lib.ptr(self.main[2:]), _lib.ptr(self.main[0]),
                                     _lib.ptr(self.main[1]), self.seed & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF,
                                     _lib.ptr(self.raw), _lib.ptr(slot), _lib.ptr(self.ws), st)
            _lib.check(rc, "lla_eb_train_pass")
            torch.add(self.raw[0], self.raw[1], alpha=float(beta_t), out=self.g)      # (g_dist + beta_t g_rate) / B
            self.g.div_(float(B))
            self.t += 1
            _adamw_step(L, self.main, self.g, self.m, self.v, self.adam, *self.adam.corrections(self.t), st)
            rc = L.lla_eb_aux_grad(_lib.ptr(self.main[2:]), _lib.ptr(self.q), _lib.ptr(self.target), C, _lib.ptr(self.gq),
                                   _lib.ptr(slot[2:]), st)
            _lib.check(rc, "lla_eb_aux_grad")
            _adamw_step(L, self.q, self.gq, self.mq, self.vq, self.adam_coder, *self.adam_coder.corrections(self.t), st)
        self.n_log += 1

    def state(self):
        return self.main.detach().cpu().clone(), self.q.detach().cpu().clone()


# ------------------------------------------------------------------------------------------------------------- the estimator
class BottleneckFit:
    """``BottleneckFit(beta, epochs=10, batch_size=1024, ...).fit(Z)``: a trained ``HRateFactorizedPrior`` for the features Z.

    beta                    weight of the rate (nats) against the L1 distortion; the shipped rate points are 1e-1, 5e-2, 1e-2.
    epochs, batch_size      passes over Z and rows per step; rows are shuffled per epoch (seeded), the last short batch is kept.
    lr, weight_decay        AdamW of ``scaling``, ``biasing`` and the bottleneck's network (the reference: 1e-3, 3e-8).
    lr_coder, weight_decay_coder   AdamW of the quantiles on the auxiliary loss (the reference: 3e-4, 1e-6).
    scheduler, decay_factor both rates per epoch through :func:`lossyless_amd.lr_schedule` (None, "unifmultistep", "expdecay").
    beta_anneal             "linear": beta_t rises from 1e-5 beta to beta over the first ceil(steps / 10) steps; "constant".
    init_scale, filters     of ``EntropyBottleneck``; only filters (3, 3, 3, 3) is built.
    seed                    of the ``_bias`` initialisation, the shuffles and the noise stream.

    ``fit(Z)``: Z a [N, C] tensor or array -- on a GPU: the HIP engine (C % 4 == 0, fp16 or fp32 rows); on the CPU: the
    float64 twin -- or a :class:`~lossyless_amd.CompressedLatents`, read through ``batches()`` (a rate point trained from a
    higher-rate container; its device selects the engine).  Afterwards: ``rate_estimator_`` (tables updated, ready for
    ``compress`` / ``decompress``), ``state_dict()`` (the key set of the shipped ``assets/*_factorized_rate.pt``),
    ``rate_curve_`` (bits per row per epoch), ``distortion_curve_``, ``loss_curve_`` (mean dist + beta mean rate in nats, at the
    FINAL beta while beta_t anneals, as the reference logs it: lossyless/learnable_compressors.py:256-261),
    ``aux_curve_``, ``beta_curve_`` (beta_t of the epoch's last step) and ``lr_curve_``."""

    def __init__(self, beta, epochs=10, batch_size=1024, lr=1e-3, weight_decay=3e-8, lr_coder=3e-4, weight_decay_coder=1e-6,
                 scheduler="unifmultistep", decay_factor=1000, beta_anneal="linear", init_scale=10, filters=FILTERS, seed=0):
        if tuple(filters) != FILTERS:
            raise ValueError(f"filters={tuple(filters)} is not built: the kernels hold the (3, 3, 3, 3) network in registers")
        if beta_anneal not in ("linear", "constant"):
            raise ValueError(f"beta_anneal={beta_anneal!r} is not built: 'linear' or 'constant'")
        if not (beta > 0) or int(epochs) < 1 or int(batch_size) < 1:
            raise ValueError("beta must be positive, epochs and batch_size at least 1")
        self.beta, self.epochs, self.batch_size = float(beta), int(epochs), int(batch_size)
        self.lr, self.weight_decay, self.lr_coder, self.weight_decay_coder = lr, weight_decay, lr_coder, weight_decay_coder
        self.scheduler, self.decay_factor, self.beta_anneal = scheduler, decay_factor, beta_anneal
        self.init_scale, self.seed = init_scale, int(seed)
        self.lr_curve_ = lr_schedule(scheduler, lr, self.epochs, decay_factor=decay_factor)      # (ValueError: unknown scheduler)
        self._lr_coder_curve = lr_schedule(scheduler, lr_coder, self.epochs, decay_factor=decay_factor)

    def _draw_biases(self, eb, g):
        """The ``_bias*`` values of an ``EntropyBottleneck``, uniform in +-0.5 from the seeded generator: its first draws."""
        with torch.no_grad():
            for i in range(5):
                b = getattr(eb, f"_bias{i}")
                b.copy_(torch.empty(b.shape).uniform_(-0.5, 0.5, generator=g))

    def initial_estimator(self, z_dim, generator=None):
        """The untrained module: ``EntropyBottleneck.__init__`` (``scaling`` = 1, ``biasing`` = 0, lossyless/rates.py:423-424)
        with the ``_bias`` values drawn from the seeded generator."""
        g = generator if generator is not None else torch.Generator().manual_seed(self.seed)
        with torch.random.fork_rng(devices=[]):
            m = HRateFactorizedPrior(int(z_dim), kwargs_ent_bottleneck=dict(init_scale=self.init_scale, filters=FILTERS))
        self._draw_biases(m.entropy_bottleneck, g)
        return m

    # ---- the three hooks of ``fit``, which HyperpriorFit replaces
    def _engine(self, m, adam, adam_coder, dev, max_batch, steps_per_epoch):
        """The freshly initialised module -> its engine: the device's for ``dev`` a GPU, else the twin."""
        eb = m.entropy_bottleneck
        main = torch.cat([m.scaling.detach().double()[None], m.biasing.detach().double()[None], pack_network(eb)], 0)
        q = eb.quantiles.detach().double().reshape(-1, 3)
        if dev.type == "cuda":
            return _DeviceEngine(main, q, eb.target, adam, adam_coder, self.seed, dev, max_batch, steps_per_epoch)
        return _TwinEngine(main, q, eb.target, adam, adam_coder, self.seed)

    def _curve_entries(self, log, N):
        """One epoch's ``epoch_log()`` -> {curve: the epoch's entry}."""
        return self._rate_entries(log[:, 0], log[:, 1], log[:, 2], N)

    def _rate_entries(self, dist, rate, aux, N):
        return dict(rate=float(rate.sum() / N / math.log(BASE_LOG)), distortion=float(dist.sum() / N),
                    loss=float((dist + self.beta * rate).sum() / N), aux=float(aux.mean()))

    def _store(self, m, state):
        """The engine's ``state()`` back into the module."""
        main, q = state
        with torch.no_grad():
            m.scaling.copy_(main[0].float())
            m.biasing.copy_(main[1].float())
            unpack_network_(m.entropy_bottleneck, main[2:].float())
            m.entropy_bottleneck.quantiles.copy_(q.float().reshape(-1, 1, 3))

    def _batches(self, Z, g):
        """One epoch of minibatches of Z in an order drawn from g."""
        if hasattr(Z, "batches"):
            for item in Z.batches(self.batch_size, shuffle=True, generator=g):
                yield item[0] if isinstance(item, tuple) else item
            return
        order = torch.randperm(Z.shape[0], generator=g).to(Z.device)
        for b0 in range(0, Z.shape[0], self.batch_size):
            yield Z[order[b0:b0 + self.batch_size]]

    def fit(self, Z):
        if hasattr(Z, "batches"):
            N, C, dev = len(Z), int(Z.z_dim), torch.device(Z.device)
        else:
            if not isinstance(Z, torch.Tensor):
                Z = torch.from_numpy(np.ascontiguousarray(Z))
            if Z.dim() != 2 or Z.shape[0] < 1:
                raise ValueError("Z must be a non-empty [N, C] matrix")
            N, C, dev = int(Z.shape[0]), int(Z.shape[1]), Z.device
        g = torch.Generator().manual_seed(self.seed)
        m = self.initial_estimator(C, g)
        steps_per_epoch = -(-N // self.batch_size)
        betas = beta_schedule(self.beta, self.epochs * steps_per_epoch, self.beta_anneal)
        adam = _Adam(self.lr, self.weight_decay, (0.9, 0.999), 1e-8)
        adam_coder = _Adam(self.lr_coder, self.weight_decay_coder, (0.9, 0.999), 1e-8)
        eng = self._engine(m, adam, adam_coder, dev, min(self.batch_size, N), steps_per_epoch)
        curves, step = {}, 0
        for epoch in range(self.epochs):
            adam.lr, adam_coder.lr = self.lr_curve_[epoch], self._lr_coder_curve[epoch]
            for zb in self._batches(Z, g):
                eng.step(zb, step, betas[step])
                step += 1
            for k, v in dict(self._curve_entries(eng.epoch_log(), N), beta=float(betas[step - 1])).items():
                curves.setdefault(k, []).append(v)
        for k, v in curves.items():
            setattr(self, f"{k}_curve_", v)
        self._store(m, eng.state())
        m.eval()
        m.update(force=True)
        self.engine_ = "device" if dev.type == "cuda" else "twin"
        self.rate_estimator_ = m.to(dev) if dev.type == "cuda" else m
        return self

    def state_dict(self):
        """What the reference's module saves: for ``BottleneckFit`` the key set of the shipped ``assets/*_factorized_rate.pt``
        (loads into ``ClipCompressor(pretrained_state_dict=...)`` and the reference's ``HRateFactorizedPrior``), for
        ``HyperpriorFit`` that of ``synthetic_hyperprior_state_dict`` (loads into ``hubconf.clip_hyperprior_compressor`` and,
        ``strict=True``, into ``HRateHyperprior(z_dim)``)."""
        return {k: v.detach().cpu().clone() for k, v in self.rate_estimator_.state_dict().items()}
