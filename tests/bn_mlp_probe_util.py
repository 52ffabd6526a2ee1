"""Shared by test_bn_mlp_probe_host.py and test_gpu_bn_mlp_probe.py (no test in here): the reference's ``MLP.module`` with a
batchnorm norm layer rebuilt from ``torch.nn``, its forward pass with explicit dropout masks, and the fit of
``BatchNormMLPProbe`` replayed step by step on the CPU -- in the float64 twin and in a torch fp32 module that is given the
twin's masks (the fp32 yardstick of the device tests)."""
import torch

from lossyless_amd import dropout_keep, lr_schedule


def reference_module(in_dim, hid_dim, n_hid_layers, out_dim, dropout_p=0.2, dtype=torch.float32):
    """``MLP.module`` of the reference for ``norm_layer="batchnorm"``: Linear(bias=False), BatchNorm1d, ReLU, Dropout per hidden
    block, then Linear."""
    nn = torch.nn
    layers, width = [], in_dim
    for _ in range(n_hid_layers):
        layers += [nn.Linear(width, hid_dim, bias=False), nn.BatchNorm1d(hid_dim), nn.ReLU(), nn.Dropout(p=dropout_p)]
        width = hid_dim
    return nn.Sequential(*layers, nn.Linear(width, out_dim)).to(dtype)


def forward_with_masks(net, x, masks):
    """``net(x)`` with every Dropout replaced by a multiplication with the next of ``masks`` (keep . s, in x's dtype)."""
    masks = list(masks)
    for m in net:
        x = x * masks.pop(0) if isinstance(m, torch.nn.Dropout) else m(x)
    return x


def masks_of(seed, step, n_blocks, rows, cols, p, dtype):
    """keep . s per block for one step, s = float32(1 / (1 - p)); all ones for p == 0."""
    if p == 0:
        return [torch.ones((rows, cols), dtype=dtype) for _ in range(n_blocks)]
    s = float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float64).float())
    return [dropout_keep(seed, step, l, rows, cols, p).to(dtype) * s for l in range(n_blocks)]


def tensors_of(net):
    """-> [weights of the Linears, gammas, betas, the last bias, running means, running variances], flattened in that order."""
    lins = [m for m in net if isinstance(m, torch.nn.Linear)]
    bns = [m for m in net if isinstance(m, torch.nn.BatchNorm1d)]
    return ([m.weight.detach() for m in lins] + [m.weight.detach() for m in bns] + [m.bias.detach() for m in bns]
            + [lins[-1].bias.detach()] + [m.running_mean for m in bns] + [m.running_var for m in bns])


def fitted_tensors(probe):
    """The same list from a fitted ``BatchNormMLPProbe``."""
    return (list(probe.coefs_) + list(probe.bn_weights_) + list(probe.bn_biases_) + list(probe.intercepts_)
            + list(probe.running_means_) + list(probe.running_vars_))


def twin_tensors(twin):
    return twin.Ws + twin.gammas + twin.betas + [twin.b] + twin.rms + twin.rvs


def replay(kw, X, y, dtype):
    """The fit ``BatchNormMLPProbe(**kw).fit(X, y)`` performs, replayed step by step on the CPU (the same initialisation, the
    same generator, the same minibatches, masks and learning rates).  float64: on the twin; float32: ``nn.Sequential`` +
    autograd + ``torch.optim.AdamW`` in fp32 with the twin's masks.  -> the tensors in the order of ``tensors_of``."""
    from lossyless_amd.probe import _Adam, _TwinBNMLP, _mlp_init
    n, bs, p = X.shape[0], kw["batch_size"], kw["dropout_p"]
    K, L = int(y.max()) + 1, kw["n_hid_layers"]
    g = torch.Generator().manual_seed(kw["seed"])
    Ws, bias = _mlp_init([X.shape[1]] + [kw["hid_dim"]] * L + [K], g)
    lo, hi = (int(w) for w in torch.randint(0, 2 ** 32, (2,), generator=g, dtype=torch.int64))
    seed = lo | (hi << 32)
    rates = lr_schedule(kw.get("scheduler"), kw["lr"], kw["epochs"])
    if dtype == torch.float64:
        adam = _Adam(kw["lr"], kw["weight_decay"], (0.9, 0.999), 1e-8)
        twin = _TwinBNMLP(Ws, bias[-1], adam, p, seed, 0.1, 1e-5)
    else:
        net = reference_module(X.shape[1], kw["hid_dim"], L, K, p)
        with torch.no_grad():
            for m, W in zip([m for m in net if isinstance(m, torch.nn.Linear)], Ws):
                m.weight.copy_(W)
            net[-1].bias.zero_()
        opt = torch.optim.AdamW(net.parameters(), lr=kw["lr"], weight_decay=kw["weight_decay"], betas=(0.9, 0.999), eps=1e-8)
    step = 0
    for epoch in range(kw["epochs"]):
        order = torch.randperm(n, generator=g)
        for b0 in range(0, n, bs):
            xb, yb = X[order[b0:b0 + bs]], y[order[b0:b0 + bs]]
            if dtype == torch.float64:
                adam.lr = rates[epoch]
                twin.step(xb, yb)
            else:
                opt.param_groups[0]["lr"] = rates[epoch]
                opt.zero_grad()
                masks = masks_of(seed, step, L, xb.shape[0], kw["hid_dim"], p, torch.float32)
                torch.nn.functional.cross_entropy(forward_with_masks(net, xb, masks), yb).backward()
                opt.step()
            step += 1
    return twin_tensors(twin) if dtype == torch.float64 else tensors_of(net)


def differences(got, want):
    """max |difference| per tensor, in double on the CPU."""
    return [float((p.double().cpu() - q.double().cpu()).abs().max()) for p, q in zip(got, want)]
