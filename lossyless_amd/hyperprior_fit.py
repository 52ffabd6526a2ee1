"""``HyperpriorFit`` -- train the scale-hyperprior rate model (``HRateHyperprior``) on frozen features, on the device.

The reference trains its hyperprior rate points with ``main.py``: the encoder frozen, the ``lossy_Z`` distortion with
``p_norm: 1`` and ``HRateHyperprior`` (lossyless/rates.py:571-678, :428-438) learning ``scaling``, ``biasing``, the side
information's ``EntropyBottleneck`` (58 numbers per side channel), the side encoder and the z encoder (two MLPs,
z_dim -> H -> H -> side_z_dim and side_z_dim -> H -> H -> 2 z_dim, H = max(z_dim, 256)) under ``loss = mean dist + beta_t mean
rate`` (lossyless/learnable_compressors.py:241-275), with a second optimiser on the bottleneck's quantiles (:277-303,
:343-416).  This module is that loop for a matrix of features.  A device step is, in order: the prologue of
``lla_gaussian_train_pass`` (y), 3 x ``lla_gemm_f32`` (side encoder), ``lla_eb_side_pass``, 3 x ``lla_gemm_f32`` (z encoder),
``lla_gaussian_train_pass``, the z encoder's backward (``lla_gemm_f32_tn`` / ``_nn``), ``dx += d s_hat``, the side encoder's
backward, ``dy += `` its input gradient, ``lla_affine_grad``, ONE ``lla_adamw_step`` over the flat main buffer,
``lla_eb_aux_grad_any`` and ``lla_adamw_step`` on the quantiles.  include/lossyless_amd.h states the mathematics.

CPU data runs the float64 twin below, as ``BottleneckFit`` does: the same formulas by hand in torch (NO autograd), the same
noise, the same step order.  The tests hold the twin to autograd and the kernels to the twin.

The reference's quirk is kept: CODING passes the predicted scales as ``means`` (rates.py:694-696, ``get_indexes_means_hat``),
while the TRAINING likelihood -- here as there -- uses the predicted means.  The trained means therefore lower the rate the
loss sees, not the bits the coder writes.

Initialisation is ``weights_init`` (lossyless/helpers.py:173-178): every Linear weight uniform in +-sqrt(6 / fan_in)
(``kaiming_uniform_(nonlinearity="relu")``), zero biases, from the seeded generator; ``scaling`` = 1, ``biasing`` = 0.

Not built: ``is_pred_mean=False``, the encoder's training, the other distortions, lightning's logging.
"""
import math

import numpy as np
import torch

from . import _lib
from ._train import _adamw, _adamw_step, _mlp_backward, _mlp_forward
from .bottleneck_fit import (FILTERS, LIK_BOUND, N_NET, NOISE_TAG, BottleneckFit, _Engine, hyperprior_noise, pack_network, twin_aux,
                             twin_likelihood, unpack_network_)
from .rates import BASE_LOG, HRateHyperprior

SIDE_TAG = 0x73696465                   # fourth counter word of the side information's noise (``hyperprior_noise(..., tag)``)
_INV_SQRT2, _INV_SQRT2PI = 2.0 ** -0.5, 1.0 / math.sqrt(2.0 * math.pi)


# ------------------------------------------------------------------------------------------ the float64 twin of the kernels
def twin_side_pass(x, net, u, scale=1.0):
    """``lla_eb_side_pass`` in the dtype of ``net`` [58, S] on x [B, S] and noise u -> (s_hat, dx = scale d rate / dx,
    grads [58, S] = scale d rate / d net, sum rate).  Backward by hand (``bottleneck_fit.twin_likelihood``)."""
    v = x.to(net.dtype) + u.to(net.dtype)
    dv, grads, rate = twin_likelihood(net, v)
    return v, scale * dv, scale * grads, rate


def twin_gaussian_pass(z, scaling, biasing, gp, u, bound, scale=1.0):
    """``lla_gaussian_train_pass`` in the dtype of ``scaling`` [C] on rows z [B, C], gp [B, 2C] (scales | means) and noise u
    -> (y, dgp [B, 2C], dy, g_dist [C] (not scaled), sum dist, sum rate_z).  Backward by hand."""
    dt = scaling.dtype
    z, u, gp = z.to(dt), u.to(dt), gp.to(dt)
    C = z.shape[1]
    es, ems = torch.exp(scaling), torch.exp(-scaling)
    y = (z + biasing) * es
    v = y + u
    sraw, mu = gp[:, :C], gp[:, C:2 * C]
    d = v - mu
    t = d.abs()
    sc = sraw.clamp(min=bound)
    au, al = (0.5 - t) / sc, (-0.5 - t) / sc
    lik = (0.5 * torch.erfc(-_INV_SQRT2 * au) - 0.5 * torch.erfc(-_INV_SQRT2 * al)).clamp(min=LIK_BOUND)
    g = -1 / lik
    pu, pl = torch.exp(-0.5 * (au * au)) * _INV_SQRT2PI, torch.exp(-0.5 * (al * al)) * _INV_SQRT2PI
    g_t = g * (-(pu - pl) / sc)
    g_sc = g * (-(au * pu - al * pl) / sc)
    sg = torch.sign(d)
    d_scale = torch.where((sraw >= bound) | (g_sc < 0), scale * g_sc, torch.zeros((), dtype=dt))
    r = u * ems
    dd = r + 1e-6
    return (y, torch.cat([d_scale, scale * (g_t * -sg)], 1), scale * (g_t * sg), (-torch.sign(dd) * r).sum(0), dd.abs().sum(),
            -torch.log(lik).sum())


def twin_affine_grad(dy_total, y, scaling, g_dist=None, add_scale=0.0):
    """``lla_affine_grad`` -> (g_scaling, g_biasing)."""
    gs = (dy_total * y).sum(0)
    if g_dist is not None:
        gs = gs + add_scale * g_dist
    return gs, torch.exp(scaling) * dy_total.sum(0)


def twin_step_gradients(P, z, u_s, u_z, bound, beta_t):
    """The main optimiser's gradients of ``mean dist + beta_t mean rate`` for the parameters P (dict: scaling, biasing, net,
    side_W, side_b, z_W, z_b) in the order of a device step -> (dict of gradients, (sum dist, sum rate_z, sum rate_s))."""
    B = z.shape[0]
    scale = float(np.float32(beta_t / B))                                  # what the kernels receive as `float scale`
    y = (z.to(P["scaling"].dtype) + P["biasing"]) * torch.exp(P["scaling"])          # the prologue
    x, hs_s = _mlp_forward(P["side_W"], P["side_b"], y)
    s_hat, dx, g_net, rate_s = twin_side_pass(x, P["net"], u_s, scale)
    gp, hs_z = _mlp_forward(P["z_W"], P["z_b"], s_hat)
    _, dgp, dy, g_dist, dist, rate_z = twin_gaussian_pass(z, P["scaling"], P["biasing"], gp, u_z, bound, scale)
    gW_z, gb_z, ds = _mlp_backward(P["z_W"], hs_z, dgp, below=True)
    gW_s, gb_s, dy_enc = _mlp_backward(P["side_W"], hs_s, dx + ds, below=True)
    g_s, g_b = twin_affine_grad(dy + dy_enc, y, P["scaling"], g_dist, float(np.float32(1.0 / B)))
    return dict(scaling=g_s, biasing=g_b, net=g_net, side_W=gW_s, side_b=gb_s, z_W=gW_z, z_b=gb_z), (dist, rate_z, rate_s)


def _flatten(P):
    """The tensors of the main optimiser, in the order of the device's flat buffer."""
    out = [P["scaling"], P["biasing"], P["net"]]
    for w, b in (("side_W", "side_b"), ("z_W", "z_b")):
        for W, bb in zip(P[w], P[b]):
            out += [W, bb]
    return out


class _TwinEngine(_Engine):
    """One training step in float64 on the host: the CPU path of ``HyperpriorFit`` and the oracle of its GPU tests.  A step's
    log: sum dist, sum rate_z, sum rate_s, aux."""

    def __init__(self, P, q, target, bound, adam, adam_coder, seed):
        super().__init__(4, adam, adam_coder, seed)
        cp = lambda v: [t.double().clone() for t in v] if isinstance(v, (list, tuple)) else v.double().clone()
        self.P, self.q, self.target, self.bound = {k: cp(v) for k, v in P.items()}, q.double().clone(), target.double(), float(bound)
        self.C, self.S = self.P["scaling"].shape[0], self.P["net"].shape[1]
        self.mom = [(torch.zeros_like(p), torch.zeros_like(p)) for p in _flatten(self.P)]
        self.mom_q = [(torch.zeros_like(self.q), torch.zeros_like(self.q))]

    def step(self, z, step, beta_t):
        B = z.shape[0]
        z = z.detach().cpu()
        u_s, u_z = hyperprior_noise(self.seed, step, B, self.S, SIDE_TAG), hyperprior_noise(self.seed, step, B, self.C, NOISE_TAG)
        G, (dist, rate_z, rate_s) = twin_step_gradients(self.P, z, u_s, u_z, self.bound, beta_t)
        self.t += 1
        _adamw(_flatten(self.P), _flatten(G), self.mom, self.adam, self.t)
        gq, aux = twin_aux(self.P["net"], self.q, self.target)
        _adamw([self.q], [gq], self.mom_q, self.adam_coder, self.t)
        self.log.append((float(dist), float(rate_z), float(rate_s), float(aux)))

    def state(self):
        cp = lambda v: [t.clone() for t in v] if isinstance(v, list) else v.clone()
        return {k: cp(v) for k, v in self.P.items()}, self.q.clone()


def _pad(n, k):
    return -(-int(n) // k) * k


class _DeviceEngine(_Engine):
    """The same step on the GPU.  Parameters, gradients and the two moments of the main optimiser each live in ONE flat fp32
    buffer -- scaling [C], biasing [C], the network [58][S], then per Linear layer the weight [out_p][in_p] and the bias [out_p],
    every piece starting on a multiple of 4 elements and every layer width padded to a multiple of 8 as ``_DeviceMLP`` pads
    (zero weights and zero biases, whose gradients are zero: AdamW leaves them zero) -- so one ``lla_adamw_step`` updates
    everything.  ``_forward`` and ``_backward`` stay apart from that ``_DeviceMLP`` on purpose: EVERY width is padded here
    and only the class width there, and the batchnorm blocks and the cross-entropy slot exist only there; one class for both
    would be switches for all of that."""

    def __init__(self, P, q, target, bound, adam, adam_coder, seed, device, max_batch, steps_per_epoch):
        super().__init__(4, adam, adam_coder, seed, device, max_batch, steps_per_epoch)
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.C, self.S = int(P["scaling"].shape[0]), int(P["net"].shape[1])
        C, S = self.C, self.S
        self.H = H = int(P["side_W"][0].shape[0])
        self.Cp, self.Sp, self.Hp, self.Gp = _pad(C, 8), _pad(S, 8), _pad(H, 8), _pad(2 * C, 8)
        self.dims_s, self.dims_z = [self.Cp, self.Hp, self.Hp, self.Sp], [self.Sp, self.Hp, self.Hp, self.Gp]
        sizes = [C, C, N_NET * S]
        for dims in (self.dims_s, self.dims_z):
            for i, o in zip(dims[:-1], dims[1:]):
                sizes += [o * i, o]
        self.offsets = np.concatenate([[0], np.cumsum([_pad(n, 4) for n in sizes])]).tolist()
        self.sizes, self.n = sizes, self.offsets[-1]
        self.flat = [torch.zeros(self.n, **f32) for _ in range(4)]               # parameters, gradients, two moments
        self.p, self.g = self._views(self.flat[0]), self._views(self.flat[1])
        with torch.no_grad():
            self.p["scaling"].copy_(P["scaling"])
            self.p["biasing"].copy_(P["biasing"])
            self.p["net"].copy_(P["net"])
            for w, b in (("side_W", "side_b"), ("z_W", "z_b")):
                for dst, src in zip(self.p[w], P[w]):
                    dst[:src.shape[0], :src.shape[1]].copy_(src)
                for dst, src in zip(self.p[b], P[b]):
                    dst[:src.shape[0]].copy_(src)
        self.q, self.target = q.to(**f32).contiguous(), target.to(**f32).contiguous()
        self.gq, self.mq, self.vq = (torch.zeros_like(self.q) for _ in range(3))
        self.bound, R = float(bound), self.rows
        buf = lambda n: torch.zeros((R, n), **f32)
        self.y, self.dy, self.dy_enc = buf(self.Cp), buf(self.Cp), buf(self.Cp)
        self.s_hat, self.dx, self.ds = buf(self.Sp), buf(self.Sp), buf(self.Sp)
        self.acts_s, self.acts_z = [buf(o) for o in self.dims_s[1:]], [buf(o) for o in self.dims_z[1:]]
        self.dgp = buf(self.Gp)
        self.delta_s, self.delta_z = [buf(self.Hp), buf(self.Hp)], [buf(self.Hp), buf(self.Hp)]
        self.g_dist = torch.zeros(_pad(C, 4), **f32)
        nws = max(int(self.L.lla_eb_side_pass_workspace_bytes(R, S)), int(self.L.lla_gaussian_train_pass_workspace_bytes(R, C)),
                  int(self.L.lla_affine_grad_workspace_bytes(R, C)), 16)
        self.ws = torch.empty(nws, dtype=torch.uint8, device=self.dev)

    def _views(self, flat):
        at = iter(zip(self.offsets, self.sizes))
        take = lambda: (lambda o, n: flat[o:o + n])(*next(at))
        v = dict(scaling=take(), biasing=take(), net=take().view(N_NET, self.S))
        for w, b, dims in (("side_W", "side_b", self.dims_s), ("z_W", "z_b", self.dims_z)):
            v[w], v[b] = [], []
            for i, o in zip(dims[:-1], dims[1:]):
                v[w].append(take().view(o, i))
                v[b].append(take())
        return v

    # every launch is a method of its own; ``step`` is their sequence
    def _gaussian(self, z, code, ldz, B, step, scale, st, full):
        P, L = _lib.ptr, self.L
        slot = self.sums[self.n_log]
        rc = L.lla_gaussian_train_pass(P(z), code, ldz, B, self.C, P(self.p["scaling"]), P(self.p["biasing"]),
                                       P(self.acts_z[2]) if full else None, self.Gp, self.bound, self.seed & 0xFFFFFFFFFFFFFFFF,
                                       int(step) & 0xFFFFFFFF, scale, P(self.dgp), P(self.y), self.Cp, P(self.dy), P(self.g_dist),
                                       P(slot), P(self.ws), st)
        _lib.check(rc, "lla_gaussian_train_pass")

    def _forward(self, Ws, bs, dims, x, acts, B, st):
        for l in range(3):
            i, o = dims[l], dims[l + 1]
            rc = self.L.lla_gemm_f32(_lib.ptr(x), i, _lib.ptr(Ws[l]), i, _lib.ptr(bs[l]), _lib.ptr(acts[l]), o, B, o, i,
                                     int(l < 2), st)
            _lib.check(rc, "lla_gemm_f32")
            x = acts[l]

    def _backward(self, Ws, gWs, gbs, dims, x, acts, delta, hidden, below, B, st):
        """``delta`` [B][dims[3]] at the output -> the weights' and biases' gradients; the input's gradient into ``below``."""
        P, L = _lib.ptr, self.L
        ins = [x, acts[0], acts[1]]
        for l in (2, 1, 0):
            i, o = dims[l], dims[l + 1]
            rc = L.lla_gemm_f32_tn(P(delta), o, P(ins[l]), i, P(gWs[l]), i, P(gbs[l]), B, o, i, st)
            _lib.check(rc, "lla_gemm_f32_tn")
            out = hidden[l - 1] if l > 0 else below
            rc = L.lla_gemm_f32_nn(P(delta), o, P(Ws[l]), i, P(ins[l]) if l > 0 else None, i, P(out), i, B, o, i, st)
            _lib.check(rc, "lla_gemm_f32_nn")
            delta = out

    def step(self, z, step, beta_t):
        B, C, S, L, P = int(z.shape[0]), self.C, self.S, self.L, _lib.ptr
        z, code, ldz = self._minibatch(z, C)
        _lib.require_cuda(self.flat[0], "parameters")
        scale, slot, p, g = float(beta_t) / B, self.sums[self.n_log], self.p, self.g
        with torch.cuda.device(self.dev):
            st = _lib.stream_ptr(self.dev)
            self._gaussian(z, code, ldz, B, step, scale, st, full=False)                        # y
            self._forward(p["side_W"], p["side_b"], self.dims_s, self.y, self.acts_s, B, st)
            rc = L.lla_eb_side_pass(P(self.acts_s[2]), self.Sp, B, S, P(p["net"]), self.seed & 0xFFFFFFFFFFFFFFFF,
                                    int(step) & 0xFFFFFFFF, scale, P(self.s_hat), self.Sp, P(self.dx), self.Sp, P(g["net"]),
                                    P(slot[2:]), P(self.ws), st)
            _lib.check(rc, "lla_eb_side_pass")
            self._forward(p["z_W"], p["z_b"], self.dims_z, self.s_hat, self.acts_z, B, st)
            self._gaussian(z, code, ldz, B, step, scale, st, full=True)
            self._backward(p["z_W"], g["z_W"], g["z_b"], self.dims_z, self.s_hat, self.acts_z, self.dgp, self.delta_z, self.ds, B, st)
            self.dx[:B].add_(self.ds[:B])
            self._backward(p["side_W"], g["side_W"], g["side_b"], self.dims_s, self.y, self.acts_s, self.dx, self.delta_s,
                           self.dy_enc, B, st)
            self.dy[:B].add_(self.dy_enc[:B])
            rc = L.lla_affine_grad(P(self.dy), self.Cp, P(self.y), self.Cp, P(p["scaling"]), B, C, P(self.g_dist), 1.0 / B,
                                   P(g["scaling"]), P(g["biasing"]), P(self.ws), st)
            _lib.check(rc, "lla_affine_grad")
            self.t += 1
            _adamw_step(L, *self.flat, self.adam, *self.adam.corrections(self.t), st)
            rc = L.lla_eb_aux_grad_any(P(p["net"]), P(self.q), P(self.target), S, P(self.gq), P(slot[3:]), st)
            _lib.check(rc, "lla_eb_aux_grad_any")
            _adamw_step(L, self.q, self.gq, self.mq, self.vq, self.adam_coder, *self.adam_coder.corrections(self.t), st)
        self.n_log += 1

    def state(self):
        """-> (parameters without their padding, quantiles) on the CPU."""
        C, S, H, p = self.C, self.S, self.H, self.p
        real_s, real_z = [(H, C), (H, H), (S, H)], [(H, S), (H, H), (2 * C, H)]
        cut = lambda Ws, shapes: [W[:o, :i].detach().cpu().clone() for W, (o, i) in zip(Ws, shapes)]
        cutb = lambda bs, shapes: [b[:o].detach().cpu().clone() for b, (o, _) in zip(bs, shapes)]
        P = dict(scaling=p["scaling"].detach().cpu().clone(), biasing=p["biasing"].detach().cpu().clone(),
                 net=p["net"].detach().cpu().clone(), side_W=cut(p["side_W"], real_s), side_b=cutb(p["side_b"], real_s),
                 z_W=cut(p["z_W"], real_z), z_b=cutb(p["z_b"], real_z))
        return P, self.q.detach().cpu().clone()


def _linears(mlp):
    return [m for m in mlp.module if isinstance(m, torch.nn.Linear)]


def pack_parameters(m, dtype=torch.float64):
    """An ``HRateHyperprior`` -> (the dict of the main optimiser's parameters, quantiles [S, 3]) on the CPU."""
    f = lambda t: t.detach().to("cpu", dtype).clone()
    eb = m.entropy_bottleneck
    P = dict(scaling=f(m.scaling), biasing=f(m.biasing), net=pack_network(eb, dtype),
             side_W=[f(l.weight) for l in _linears(m.side_encoder)], side_b=[f(l.bias) for l in _linears(m.side_encoder)],
             z_W=[f(l.weight) for l in _linears(m.z_encoder)], z_b=[f(l.bias) for l in _linears(m.z_encoder)])
    return P, f(eb.quantiles).reshape(eb.channels, 3)


def unpack_parameters_(m, P, q):
    """Inverse of :func:`pack_parameters`, in place."""
    with torch.no_grad():
        m.scaling.copy_(P["scaling"].float())
        m.biasing.copy_(P["biasing"].float())
        unpack_network_(m.entropy_bottleneck, P["net"].float())
        m.entropy_bottleneck.quantiles.copy_(q.float().reshape(-1, 1, 3))
        for mlp, w, b in ((m.side_encoder, "side_W", "side_b"), (m.z_encoder, "z_W", "z_b")):
            for lin, W, bb in zip(_linears(mlp), P[w], P[b]):
                lin.weight.copy_(W.float())
                lin.bias.copy_(bb.float())


# ------------------------------------------------------------------------------------------------------------- the estimator
class HyperpriorFit(BottleneckFit):
    """``HyperpriorFit(beta, epochs=10, batch_size=1024, ...).fit(Z)``: a trained ``HRateHyperprior`` for the features Z.

    The arguments of :class:`BottleneckFit` (``lr`` / ``weight_decay`` now also cover the two MLPs, ``lr_coder`` /
    ``weight_decay_coder`` the side bottleneck's quantiles), plus
    factor_dim, side_z_dim   ``side_z_dim = max(10, z_dim // factor_dim)`` unless given (lossyless/rates.py:602-603).
    is_pred_mean             only True is built.

    ``fit(Z)``: Z a [N, C] tensor or array -- on a GPU: the HIP engine (any C, fp16 or fp32 rows); on the CPU: the float64
    twin -- or anything with ``batches()`` such as a :class:`~lossyless_amd.CompressedLatents`.  Afterwards:
    ``rate_estimator_`` (an ``HRateHyperprior`` in eval mode, tables updated: ``compress`` / ``encode_device`` work),
    ``state_dict()`` (the key set of ``synthetic_hyperprior_state_dict``; loads into ``hubconf.clip_hyperprior_compressor``),
    ``rate_curve_`` (bits per row per epoch, z and side together), ``side_rate_curve_`` (the side information's share),
    ``distortion_curve_``, ``loss_curve_``, ``aux_curve_``, ``beta_curve_``, ``lr_curve_`` and ``engine_``.

    Coding passes the scales as ``means`` (the reference's quirk, rates.py:694-696) while this training's likelihood uses the
    predicted means: see the module docstring."""

    def __init__(self, beta, epochs=10, batch_size=1024, lr=1e-3, weight_decay=3e-8, lr_coder=3e-4, weight_decay_coder=1e-6,
                 scheduler="unifmultistep", decay_factor=1000, beta_anneal="linear", init_scale=10, filters=FILTERS, seed=0,
                 factor_dim=5, side_z_dim=None, is_pred_mean=True):
        super().__init__(beta, epochs=epochs, batch_size=batch_size, lr=lr, weight_decay=weight_decay, lr_coder=lr_coder,
                         weight_decay_coder=weight_decay_coder, scheduler=scheduler, decay_factor=decay_factor,
                         beta_anneal=beta_anneal, init_scale=init_scale, filters=filters, seed=seed)
        if not is_pred_mean:
            raise ValueError("is_pred_mean=False is not built")
        if int(factor_dim) < 1 or (side_z_dim is not None and int(side_z_dim) < 1):
            raise ValueError("factor_dim and side_z_dim must be at least 1")
        self.factor_dim, self.side_z_dim = int(factor_dim), None if side_z_dim is None else int(side_z_dim)

    def initial_estimator(self, z_dim, generator=None):
        """The untrained module as the reference's ``reset_parameters`` leaves it: ``scaling`` = 1, ``biasing`` = 0, the
        bottleneck's own initialisation with its ``_bias`` values drawn from the seeded generator, then ``weights_init``: every
        Linear weight uniform in +-sqrt(6 / fan_in), zero biases -- side encoder first, layer by layer."""
        g = generator if generator is not None else torch.Generator().manual_seed(self.seed)
        with torch.random.fork_rng(devices=[]):
            m = HRateHyperprior(int(z_dim), factor_dim=self.factor_dim, side_z_dim=self.side_z_dim,
                                kwargs_ent_bottleneck=dict(init_scale=self.init_scale, filters=FILTERS))
        self._draw_biases(m.entropy_bottleneck, g)
        with torch.no_grad():
            for mlp in (m.side_encoder, m.z_encoder):
                for lin in _linears(mlp):
                    a = math.sqrt(6.0 / lin.weight.shape[1])
                    lin.weight.copy_(torch.empty(lin.weight.shape).uniform_(-a, a, generator=g))
                    lin.bias.zero_()
        return m

    # ---- the three hooks of ``BottleneckFit.fit``
    def _engine(self, m, adam, adam_coder, dev, max_batch, steps_per_epoch):
        P, q = pack_parameters(m)
        target = m.entropy_bottleneck.target
        bound = float(m.gaussian_conditional.lower_bound_scale.bound.float().item())
        if dev.type == "cuda":
            return _DeviceEngine(P, q, target, bound, adam, adam_coder, self.seed, dev, max_batch, steps_per_epoch)
        return _TwinEngine(P, q, target, bound, adam, adam_coder, self.seed)

    def _curve_entries(self, log, N):
        return dict(self._rate_entries(log[:, 0], log[:, 1] + log[:, 2], log[:, 3], N),
                    side_rate=float(log[:, 2].sum() / N / math.log(BASE_LOG)))

    def _store(self, m, state):
        unpack_parameters_(m, *state)
