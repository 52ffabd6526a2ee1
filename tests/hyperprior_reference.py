"""What the two HyperpriorFit test files share: a restatement of the hyperprior's training loss in torch WITH autograd over
compressai's formulation (the LowerBound rule as an autograd Function, from eb_reference.py), the cases, and the comparison per
group.  Not a test module."""
import numpy as np
import torch
import torch.nn.functional as F

import eb_reference as R
from lossyless_amd.hyperprior_fit import HyperpriorFit, pack_parameters

BOUND = float(torch.tensor(0.11, dtype=torch.float32))          # compressai's scale bound as the module's fp32 buffer holds it
GAUSS_CASES = ("plain", "lowscale", "negative", "likbound", "tie")


def _phi_cdf(a):
    return 0.5 * torch.erfc(-(2 ** -0.5) * a)


def gaussian_rate(y, gp, u, bound=BOUND):
    """compressai's GaussianConditional._likelihood + likelihood_lower_bound on v = y + u -> sum of -log lik."""
    dt, C = y.dtype, y.shape[1]
    scales = R._LowerBound.apply(gp[:, :C], torch.tensor(bound, dtype=dt))
    values = torch.abs(y + u.to(dt) - gp[:, C:2 * C])
    lik = _phi_cdf((0.5 - values) / scales) - _phi_cdf((-0.5 - values) / scales)
    return -torch.log(R._LowerBound.apply(lik, torch.tensor(1e-9, dtype=dt))).sum()


def distortion(z, scaling, biasing, u):
    """lossy_Z with p_norm 1 on z_hat = process_z_out(process_z_in(z) + u)."""
    z = z.to(scaling.dtype)
    z_hat = ((z + biasing) * torch.exp(scaling) + u.to(scaling.dtype)) / torch.exp(scaling) - biasing
    return F.pairwise_distance(z_hat, z, p=1).sum()


def reference_gaussian(z, scaling, biasing, gp, u, bound=BOUND):
    """-> dict(y, dgp, dy, g_dist, dist, rate) by autograd in scaling's dtype (scale = 1)."""
    dt = scaling.dtype
    y = ((z.to(dt) + biasing) * torch.exp(scaling)).detach().requires_grad_(True)
    gp = gp.to(dt).detach().clone().requires_grad_(True)
    rate = gaussian_rate(y, gp, u, bound)
    dgp, dy = torch.autograd.grad(rate, (gp, y))
    s = scaling.detach().clone().requires_grad_(True)
    dist = distortion(z, s, biasing, u)
    g_dist, = torch.autograd.grad(dist, s)
    return dict(y=y.detach(), dgp=dgp, dy=dy, g_dist=g_dist, dist=dist.detach(), rate=rate.detach())


def side_rate(x, net, u):
    v = x + u.to(x.dtype)
    xx = v.t()[:, None, :]
    lower, upper = R.logits(net, xx - 0.5), R.logits(net, xx + 0.5)
    sgn = -torch.sign(lower + upper).detach()
    lik = torch.abs(torch.sigmoid(sgn * upper) - torch.sigmoid(sgn * lower))
    return -torch.log(R._LowerBound.apply(lik, torch.tensor(1e-9, dtype=x.dtype))).sum(), v


def reference_side(x, net, u):
    """-> dict(s_hat, dx, grads [58, S], rate) by autograd in net's dtype (scale = 1)."""
    x = x.to(net.dtype).detach().clone().requires_grad_(True)
    net = net.detach().clone().requires_grad_(True)
    rate, v = side_rate(x, net, u)
    dx, g = torch.autograd.grad(rate, (x, net))
    return dict(s_hat=v.detach(), dx=dx, grads=g, rate=rate.detach())


def _mlp(Ws, bs, x):
    for W, b in zip(Ws[:-1], bs[:-1]):
        x = torch.relu(F.linear(x, W, b))
    return F.linear(x, Ws[-1], bs[-1])


def reference_step(P, z, u_s, u_z, beta_t, bound=BOUND):
    """The gradients of ``float32(1 / B) sum dist + float32(beta_t / B) sum rate`` for the parameter dict P by autograd ->
    (dict of gradients in P's layout, (dist, rate_z, rate_s))."""
    B = z.shape[0]
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    Q = {k: [leaf(t) for t in v] if isinstance(v, list) else leaf(v) for k, v in P.items()}
    dt = Q["scaling"].dtype
    y = (z.to(dt) + Q["biasing"]) * torch.exp(Q["scaling"])
    rate_s, s_hat = side_rate(_mlp(Q["side_W"], Q["side_b"], y), Q["net"], u_s)
    rate_z = gaussian_rate(y, _mlp(Q["z_W"], Q["z_b"], s_hat), u_z, bound)
    dist = distortion(z, Q["scaling"], Q["biasing"], u_z)
    loss = float(np.float32(1.0 / B)) * dist + float(np.float32(beta_t / B)) * (rate_s + rate_z)
    flat, index = [], []
    for k, v in Q.items():
        for j, t in enumerate(v if isinstance(v, list) else [v]):
            flat.append(t)
            index.append((k, j if isinstance(v, list) else None))
    grads = torch.autograd.grad(loss, flat)
    G = {k: [None] * len(v) if isinstance(v, list) else None for k, v in Q.items()}
    for (k, j), g in zip(index, grads):
        if j is None:
            G[k] = g
        else:
            G[k][j] = g
    return G, (dist.detach(), rate_z.detach(), rate_s.detach())


def initial_parameters(C, seed=0, side_z_dim=None, dtype=torch.float64):
    """A fresh module's parameters, perturbed so that no gradient vanishes by symmetry (the z encoder's last bias spreads the
    scales over 0.05 .. 8 and moves the means) -> (P, q, target)."""
    m = HyperpriorFit(0.05, seed=seed, side_z_dim=side_z_dim).initial_estimator(C)
    P, q = pack_parameters(m)
    g = torch.Generator().manual_seed(seed + 1)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    P["net"] = P["net"] + 0.2 * rnd(*P["net"].shape)
    P["scaling"] = 1 + 0.3 * rnd(C)
    P["biasing"] = 0.3 * rnd(C)
    for k in ("side_b", "z_b"):
        P[k] = [b + 0.1 * rnd(*b.shape) for b in P[k]]
    P["z_b"][-1][:C] += torch.exp(torch.linspace(np.log(0.05), np.log(8.0), C, dtype=torch.float64))[torch.randperm(C, generator=g)]
    q = q + 0.5 * rnd(*q.shape)
    cast = lambda v: [t.to(dtype) for t in v] if isinstance(v, list) else v.to(dtype)
    return {k: cast(v) for k, v in P.items()}, q.to(dtype), m.entropy_bottleneck.target.clone()


def side_case(B, S, seed=0):
    """-> (x [B, S] float32, net [58, S] float64, q, target): side-encoder outputs on either side of every channel's mode."""
    main, q, target = R.initial_main(S, seed)
    g = torch.Generator().manual_seed(seed + 3)
    x = 2.0 * torch.randn(B, S, generator=g) + torch.linspace(-3, 3, B)[:, None]
    return x, main[2:].contiguous(), q, target


def gaussian_case(name, B, C, u, seed=0):
    """-> (z [B, C] float32, scaling, biasing [C] float64, gp [B, 2C] float32) of one of the issue's cases; u is the noise the
    pass will draw (the tie case needs it)."""
    g = torch.Generator().manual_seed(seed + 5)
    z = torch.randn(B, C, generator=g) * torch.exp(0.7 * torch.randn(B, 1, generator=g))
    scaling = 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    biasing = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    scales = torch.exp(torch.empty(B, C).uniform_(np.log(0.05), np.log(8.0), generator=g))
    means = 0.5 * torch.randn(B, C, generator=g)
    if name == "lowscale":        # every scale below the bound; far and near means give both signs of its gradient
        scales = torch.empty(B, C).uniform_(0.01, 0.1, generator=g)
        means = torch.where(torch.arange(C)[None, :] % 2 == 0, ((z.double() + biasing) * torch.exp(scaling)).float(), means)
    elif name == "negative":
        scales = -torch.empty(B, C).uniform_(0.01, 3.0, generator=g)
    elif name == "likbound":      # means so far off that the likelihood underflows to the 1e-9 bound
        means = means + torch.where(torch.arange(B)[:, None] % 2 == 0, 60.0, -60.0)
    elif name == "tie":           # y = 0 exactly (z = 0, biasing = 0), so v = u and means = u ties in every precision
        biasing = torch.zeros(C, dtype=torch.float64)
        z[::2] = 0.0
        means[::2] = u[::2]
    elif name != "plain":
        raise KeyError(name)
    return z, scaling, biasing, torch.cat([scales, means], 1).contiguous()


def close(got, ref, rel=1e-9):
    """Every element within ``rel`` of its own size plus ``rel`` of its group's largest."""
    got, ref = got.double(), ref.double()
    return bool(((got - ref).abs() <= rel * ref.abs() + rel * float(ref.abs().max())).all())


def flat_groups(P):
    """The parameter dict as {group name: one flat tensor}."""
    return {k: torch.cat([t.reshape(-1) for t in v]) if isinstance(v, list) else v.reshape(-1) for k, v in P.items()}
