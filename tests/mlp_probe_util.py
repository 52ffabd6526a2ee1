"""Shared by test_gpu_mlp_probe.py (no test in here): the two seeded problems of the device-against-twin tests, the twin's
run of one of them, and the fp32 yardstick -- everything here runs on the CPU."""
import torch

# ---- short horizon: in 8, hid 32, 2 hidden layers, 4 classes, 96 rows, batch 32, 2 epochs (6 steps)
SHORT = dict(hid_dim=32, n_hid_layers=2, epochs=2, batch_size=32, seed=0, lr=1e-3, weight_decay=1e-5)
SHORT_DATA_SEED = 2


def short_data(seed=SHORT_DATA_SEED):
    """96 fp32 rows in 8 dimensions around 4 class means."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(96) % 4
    mu = torch.randn(4, 8, generator=g, dtype=torch.float64)
    return (mu[y] + 0.5 * torch.randn(96, 8, generator=g, dtype=torch.float64)).float(), y


def replay(kw, X, y, dtype):
    """The fit ``MLPProbe(**kw).fit(X, y)`` performs, replayed step by step on the CPU (the same initialisation, the same
    generator, the same minibatches).  float64: on the twin -> (parameters, smallest |hidden pre-activation| over all
    steps).  float32: ``nn.Sequential`` + autograd + ``torch.optim.AdamW`` in fp32 -> (parameters, None)."""
    from lossyless_amd.probe import _Adam, _TwinMLP, _mlp_init
    n, bs = X.shape[0], kw["batch_size"]
    K = int(y.max()) + 1
    g = torch.Generator().manual_seed(kw["seed"])
    Ws, bias = _mlp_init([X.shape[1]] + [kw["hid_dim"]] * kw["n_hid_layers"] + [K], g)
    if dtype == torch.float64:
        twin = _TwinMLP(Ws, bias, _Adam(kw["lr"], kw["weight_decay"], (0.9, 0.999), 1e-8))
        closest = float("inf")
    else:
        nn = torch.nn
        layers = []
        for W, b in zip(Ws, bias):
            lin = nn.Linear(W.shape[1], W.shape[0])
            with torch.no_grad():
                lin.weight.copy_(W), lin.bias.copy_(b)
            layers += [lin, nn.ReLU()]
        net = nn.Sequential(*layers[:-1])
        opt = torch.optim.AdamW(net.parameters(), lr=kw["lr"], weight_decay=kw["weight_decay"], betas=(0.9, 0.999), eps=1e-8)
    for _ in range(kw["epochs"]):
        order = torch.randperm(n, generator=g)
        for b0 in range(0, n, bs):
            xb, yb = X[order[b0:b0 + bs]], y[order[b0:b0 + bs]]
            if dtype == torch.float64:
                pre = []
                twin.forward(xb, pre)
                closest = min(closest, min(float(a.abs().min()) for a in pre))
                twin.step(xb, yb)
            else:
                opt.zero_grad()
                torch.nn.functional.cross_entropy(net(xb), yb).backward()
                opt.step()
    if dtype == torch.float64:
        return twin.Ws + twin.bs, closest
    lins = [m for m in net if isinstance(m, torch.nn.Linear)]
    return [m.weight.detach() for m in lins] + [m.bias.detach() for m in lins], None


def largest_difference(a, b):
    return max(float((p.double().cpu() - q.double().cpu()).abs().max()) for p, q in zip(a, b))


# ---- what a linear probe cannot learn: the XOR of two signs
XOR = dict(hid_dim=32, n_hid_layers=2, epochs=12, batch_size=128, seed=0, lr=1e-2, weight_decay=1e-5)


def xor_data(n, seed):
    """n fp32 rows in 8 dimensions, |z_0|, |z_1| >= 0.25, label = [sign z_0 != sign z_1]."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, 8, generator=g, dtype=torch.float64)
    z[:, :2] = torch.sign(z[:, :2]) * (0.25 + z[:, :2].abs())
    return z.float(), ((z[:, 0] > 0) != (z[:, 1] > 0)).to(torch.int64)
