#!/usr/bin/env python3
"""Time one BottleneckFit training step on the MI355X against the same step in torch eager with autograd, in one process.

A step is: the main loss and its gradients, AdamW on {scaling, biasing, network}, the auxiliary loss at the updated
parameters, AdamW on the quantiles.
  device   lla_eb_train_pass + the two-launch gradient combination + lla_adamw_step + lla_eb_aux_grad + lla_adamw_step
  eager    the loss restated with torch ops on [C, 3, B] tensors (compressai's formulation, fp32), loss.backward(), two
           torch.optim.AdamW steps (foreach), torch.rand noise
Both run on the same GPU and the same features; the arms alternate, each timed over `--repeats` windows that end in a
device synchronise, after `--warmup` steps of every shape.  A window is sized by TIME, per arm and shape: as many steps as
fill `--window` seconds (0.5 by default) at the rate a first short window measured, and never fewer than `--steps`.
Reported: median and min .. max of the windows' per-step times, and the rows/s the median implies.  Times are whole-step wall times, launch gaps included (that is what a
fit pays); kernel times are not separated here.

    python tools/bottleneck_fit_bench.py [--out profiles/bottleneck_fit.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lossyless_amd import BottleneckFit, _lib                                      # noqa: E402
from lossyless_amd.bottleneck_fit import _DeviceEngine, pack_network              # noqa: E402
from lossyless_amd._train import _Adam                                             # noqa: E402


class Eager(torch.nn.Module):
    """The training-mode forward of HRateFactorizedPrior + the L1 distortion on frozen features, with autograd."""

    def __init__(self, m):
        super().__init__()
        self.m = m
        self.main = [m.scaling, m.biasing] + [p for n, p in m.entropy_bottleneck.named_parameters() if n != "quantiles"]
        self.opt = torch.optim.AdamW(self.main, lr=1e-3, weight_decay=3e-8)
        self.opt_q = torch.optim.AdamW([m.entropy_bottleneck.quantiles], lr=3e-4, weight_decay=1e-6)

    def logits(self, x, detach=False):
        eb = self.m.entropy_bottleneck
        get = (lambda n: getattr(eb, n).detach()) if detach else (lambda n: getattr(eb, n))
        for i in range(5):
            x = torch.matmul(F.softplus(get(f"_matrix{i}")), x) + get(f"_bias{i}")
            if i < 4:
                x = x + torch.tanh(get(f"_factor{i}")) * torch.tanh(x)
        return x

    def step(self, z, beta):
        m, eb = self.m, self.m.entropy_bottleneck
        es = torch.exp(m.scaling)
        v = (z + m.biasing) * es + (torch.rand_like(z) - 0.5)
        x = v.t()[:, None, :]
        lower, upper = self.logits(x - 0.5), self.logits(x + 0.5)
        sgn = -torch.sign(lower + upper).detach()
        lik = torch.abs(torch.sigmoid(sgn * upper) - torch.sigmoid(sgn * lower)).clamp_min(1e-9)
        rate = -torch.log(lik).sum() / z.shape[0]
        dist = F.pairwise_distance(v / es - m.biasing, z, p=1).mean()
        self.opt.zero_grad(set_to_none=True)
        (dist + beta * rate).backward()
        self.opt.step()
        aux = torch.abs(self.logits(eb.quantiles, detach=True) - eb.target).sum()
        self.opt_q.zero_grad(set_to_none=True)
        aux.backward()
        self.opt_q.step()


def windows(fn, steps, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="least steps per window")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bottleneck_fit_bench needs an MI355X: a CPU run says nothing about step time")
    dev = torch.device("cuda")
    lines = [f"# one training step, device engine vs torch eager (fp32, autograd), same process; {a.repeats} windows of at least "
             f"{a.window} s and {a.steps} steps per arm after {a.warmup} warm-up steps; library sha {_lib.lib().lla_source_sha().decode()}; {torch.cuda.get_device_name(0)}",
             "# C      B   device us/step (min..max)     rows/s   eager us/step (min..max)      rows/s   eager/device   steps/window"]
    for C in (512, 1024):
        for B in (1024, 4096, 16384):
            g = torch.Generator().manual_seed(0)
            z = (torch.randn(B, C, generator=g) * torch.linspace(0.05, 2, C) + torch.linspace(-1, 1, C)).to(dev)
            m = BottleneckFit(0.05, seed=0).initial_estimator(C)
            eb = m.entropy_bottleneck
            main_ = torch.cat([m.scaling.detach().double()[None], m.biasing.detach().double()[None], pack_network(eb)], 0)
            eng = _DeviceEngine(main_, eb.quantiles.detach().reshape(C, 3), eb.target, _Adam(1e-3, 3e-8, (0.9, 0.999), 1e-8),
                                _Adam(3e-4, 1e-6, (0.9, 0.999), 1e-8), 0, dev, B, 1)
            eager = Eager(m.to(dev).train())

            def dstep(i):
                eng.n_log = 0
                eng.step(z, i, 0.05)

            estep = lambda i: eager.step(z, 0.05)                                  # noqa: E731
            for i in range(a.warmup):
                dstep(i), estep(i)
            nd = max(a.steps, int(a.window / windows(dstep, a.steps, 1)[0]) + 1)
            ne = max(a.steps, int(a.window / windows(estep, a.steps, 1)[0]) + 1)
            d, e = [], []
            for _ in range(a.repeats):                                              # the arms alternate
                d += windows(dstep, nd, 1)
                e += windows(estep, ne, 1)
            md, me = statistics.median(d), statistics.median(e)
            lines.append(f"{C:5d} {B:6d}   {md * 1e6:9.1f} ({min(d) * 1e6:.1f}..{max(d) * 1e6:.1f})   {B / md:10.3e}   "
                         f"{me * 1e6:9.1f} ({min(e) * 1e6:.1f}..{max(e) * 1e6:.1f})   {B / me:10.3e}   {me / md:6.1f}x   {nd} / {ne}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
