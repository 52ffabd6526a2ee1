"""``MLPProbe``'s training step, measured (MI355X; writes its table to stdout and, with --out, to a file).

For in 512, hid 2048 x 2, 10 and 1000 classes, batch 128 and 1024, two arms run the same step on resident fp32 rows:

(a) the device path of ``MLPProbe`` (``_DeviceMLP.step``: 3 x ``lla_gemm_f32``, ``lla_softmax_xent``, 3 x ``lla_gemm_f32_tn``,
    2 x ``lla_gemm_f32_nn``, ``lla_adamw_step``),
(b) torch eager fp32 on the same device: ``nn.Sequential`` (Linear, ReLU, Linear, ReLU, Linear) + ``F.cross_entropy`` +
    ``torch.optim.AdamW``.

Every arm is warmed up, then timed with device events over ``--inner`` back-to-back steps; the arms are interleaved and the
round is repeated ``--reps`` times (3), as tools/latents_bench.py does.  The kernels of (a) are then timed on their own the
same way.  Last, the whole-epoch time of ``MLPProbe(epochs=1).fit`` from a resident ``CompressedLatents`` of ``--records``
records (131072), decode included: a host clock around a call that ends in a device synchronise, three runs per batch size.

With ``--bn`` the same four shapes and the same protocol measure ``BatchNormMLPProbe``'s step instead, three
interleaved arms:

(c) its device path (``_DeviceMLP.step`` with ``bn``: the launches of (a) -- the hidden GEMMs without bias and ReLU -- plus 2 x
    ``lla_bn_relu_dropout_fwd`` and 2 x ``lla_bn_bwd``),
(d) torch eager fp32 on the same device: ``nn.Sequential`` (Linear(bias=False), BatchNorm1d, ReLU, Dropout(0.2) per block, then
    Linear) in training mode + ``F.cross_entropy`` + ``torch.optim.AdamW``,
(a) ``MLPProbe``'s step as above, for the cost of the two added modules.
The two new kernels are then timed on their own on the second block's buffers, with the bytes they must move (forward: read a,
write out; backward: read g and a, write da) per second and per second and CU of their grid of N / 32 workgroups.

usage (GPU box): python tools/mlp_probe_bench.py [--out profiles/mlp_probe.txt]
                 python tools/mlp_probe_bench.py --bn [--out profiles/bn_mlp_probe.txt]
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import hubconf  # noqa: E402
from lossyless_amd import BatchNormMLPProbe, MLPProbe, _lib  # noqa: E402
from lossyless_amd.probe import _Adam, _DeviceMLP, _f32_rows, _mlp_init  # noqa: E402
from latents_bench import interleaved, med  # noqa: E402

IN, HID, LAYERS = 512, 2048, 2


def eager_arm(Ws, bs, x, y, dev):
    nn = torch.nn
    layers = []
    for W, b in zip(Ws, bs):
        lin = nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(W), lin.bias.copy_(b)
        layers += [lin, nn.ReLU()]
    net = nn.Sequential(*layers[:-1]).to(dev)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-5)
    y64 = y.to(torch.int64)

    def step():
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(net(x), y64).backward()
        opt.step()
    return step


def one_step(eng, x, y):
    """An arm: one training step of an engine sized for one step an epoch, each into slot 0."""
    def arm():
        eng.step(x, y)
        eng.k = 0
    return arm


def kernels_of(eng, x, y):
    """The launches of one step of (a), each as a call of the engine's own method on the engine's buffers."""
    st, n, d = _lib.stream_ptr(eng.device), int(x.shape[0]), eng.dims
    one_step(eng, x, y)()
    out = {"3 x lla_gemm_f32 (forward)": lambda: eng.forward(*_f32_rows(x, d[0]), st),
           "lla_softmax_xent": lambda: eng.xent(y, n, st)}
    below = [x] + eng.acts[:-1]
    delta = eng.delta + [eng.dlogits]                      # layer l's incoming gradient: the values do not matter here
    for l in (2, 1, 0):
        i, o = d[l], d[l + 1]
        out[f"lla_gemm_f32_tn layer {l} (dW [{o}][{i}])"] = lambda l=l, i=i, o=o: eng.tn(l, delta[l], o, below[l], i, n, st)
        if l > 0:
            out[f"lla_gemm_f32_nn layer {l} (reduction {o})"] = lambda l=l, i=i, o=o: eng.nn(l, delta[l], o, below[l], i, n, st)
    out[f"lla_adamw_step ({eng.n} parameters)"] = lambda: eng.adamw(0.1, 0.001, st)
    return out


DROPOUT = 0.2


def bn_eager_arm(Ws, b_last, x, y, dev):
    nn = torch.nn
    layers = []
    for W in Ws[:-1]:
        lin = nn.Linear(W.shape[1], W.shape[0], bias=False)
        with torch.no_grad():
            lin.weight.copy_(W)
        layers += [lin, nn.BatchNorm1d(W.shape[0]), nn.ReLU(), nn.Dropout(p=DROPOUT)]
    last = nn.Linear(Ws[-1].shape[1], Ws[-1].shape[0])
    with torch.no_grad():
        last.weight.copy_(Ws[-1]), last.bias.copy_(b_last)
    net = nn.Sequential(*layers, last).to(dev).train()
    opt = torch.optim.AdamW(net.parameters(), lr=3e-4, weight_decay=1e-5)
    y64 = y.to(torch.int64)

    def step():
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(net(x), y64).backward()
        opt.step()
    return step


def bn_kernels_of(eng, x, y):
    """The two new launches of one step of (c), on the second block's buffers, each as a call of the engine's own method."""
    st, n = _lib.stream_ptr(eng.device), int(x.shape[0])
    one_step(eng, x, y)()
    g, da = eng.delta[0], torch.empty_like(eng.delta[0])
    return {"lla_bn_relu_dropout_fwd": lambda: eng.bn_fwd(1, n, st), "lla_bn_bwd": lambda: eng.bn_bwd(1, g, da, n, st)}


def resident_dataset(args, g, dev):
    """-> (a resident ``CompressedLatents`` of ``--records`` records, their labels in 10 classes)."""
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    N = args.records
    z = (torch.randn(N, comp.z_dim, generator=g) * 0.5).to(dev)
    payload, offsets, _ = comp.entropy_bottleneck.encode_device(z, comp._tables(), record_prefix=True)
    total = int(offsets[-1])
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "Z.bin")
        with open(f, "wb") as fh:
            fh.write(N.to_bytes(4, "big"))
            fh.write(payload[:total].cpu().numpy().tobytes())
        ds = comp.open_dataset(f)
    return ds, torch.arange(N) % 10


def time_fits(Probe, ds, labels, args, say, dev):
    """One warm-up ``Probe(epochs=1).fit`` and ``--reps`` timed ones per batch size, a host clock around each."""
    for B in (128, 1024):
        runs = []
        for r in range(args.reps + 1):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            probe = Probe(epochs=1, batch_size=B).fit(ds, labels)
            torch.cuda.synchronize(dev)
            runs.append(time.perf_counter() - t0)
        runs = runs[1:]
        say(f"    batch {B:5d} ({probe.n_steps_} steps)   " + "  ".join(f"{t:8.3f}" for t in runs) +
            f"   median {med(runs):8.3f} s   {1e3 * med(runs) / probe.n_steps_:.4f} ms / step   loss {probe.loss_curve_[-1]:.4f}")


def bn_main(args, say, dev):
    say(f"device: {torch.cuda.get_device_name(dev)}   MLP {IN} -> {HID} x {LAYERS} -> classes, Linear(bias=False) -> BatchNorm1d -> "
        f"ReLU -> Dropout({DROPOUT}) per block, fp32, AdamW(lr 3e-4, wd 1e-5)")
    g = torch.Generator().manual_seed(0)
    A, C, D = "(a) MLPProbe device step", "(c) BatchNormMLPProbe device step", "(d) torch eager fp32 step (BN, dropout)"
    for K in (10, 1000):
        for B in (128, 1024):
            Ws, bs = _mlp_init([IN] + [HID] * LAYERS + [K], g)
            x = torch.randn(B, IN, generator=g).to(dev)
            y = torch.randint(0, K, (B,), generator=g).to(torch.int32).to(dev)
            plain = _DeviceMLP(Ws, bs, _Adam(1e-3, 1e-5, (0.9, 0.999), 1e-8), dev, B, K, 1)
            eng = _DeviceMLP(Ws, bs, _Adam(3e-4, 1e-5, (0.9, 0.999), 1e-8), dev, B, K, 1, (DROPOUT, 12345, 0.1, 1e-5))
            arms = {C: one_step(eng, x, y), D: bn_eager_arm(Ws, bs[-1], x, y, dev), A: one_step(plain, x, y)}
            times = interleaved(arms, args.inner, args.reps, dev)
            say()
            say(f"classes {K}, batch {B}: ms per training step, device events over {args.inner} back-to-back steps, "
                f"{args.reps} interleaved runs")
            for k, ts in times.items():
                say(f"    {k:44s} " + "  ".join(f"{t:9.4f}" for t in ts) + f"   median {med(ts):9.4f} ms")
            c, d, a = med(times[C]), med(times[D]), med(times[A])
            say(f"    (c) / (d) medians = {c / d:.3f};  spread of (d) = {max(times[D]) - min(times[D]):.4f} ms;  (c) - (d) = {c - d:+.4f} ms;  "
                f"(c) - (a) = {c - a:+.4f} ms")
            times = interleaved(bn_kernels_of(eng, x, y), args.inner, args.reps, dev)
            say("    the two new launches of (c), timed on their own (one block; a step runs each twice):")
            total = 0.0
            for (k, ts), passes in zip(times.items(), (2, 3)):
                nbytes, wgs = passes * B * HID * 4, HID // 32
                rate = nbytes / (med(ts) * 1e-3)
                total += med(ts)
                say(f"    {k:44s} " + "  ".join(f"{t:9.4f}" for t in ts) + f"   median {med(ts):9.4f} ms   {nbytes / 2**20:.1f} MiB   "
                    f"{rate / 1e12:.3f} TB/s   {rate / wgs / 1e9:.1f} GB/s per workgroup of {wgs}")
            say(f"    2 x (forward + backward) = {2 * total:.4f} ms = {100 * 2 * total / c:.1f} % of (c)")
            del eng, plain, arms
    ds, labels = resident_dataset(args, g, dev)
    say()
    say(f"one epoch of BatchNormMLPProbe.fit from a resident CompressedLatents: N = {len(ds)} records, 10 classes; host clock around "
        f"fit(epochs=1), which ends in a synchronise (initialisation, decode and label gather included); one warm-up fit, then "
        f"{args.reps} runs")
    time_fits(BatchNormMLPProbe, ds, labels, args, say, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=200, help="steps per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bn", action="store_true", help="measure BatchNormMLPProbe's step instead (DESIGN.md 5.15)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mlp_probe_bench.py measures on an MI355X: no GPU here, nothing measured")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", torch.cuda.current_device())
    if args.bn:
        bn_main(args, say, dev)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    say(f"device: {torch.cuda.get_device_name(dev)}   MLP {IN} -> {HID} x {LAYERS} -> classes, fp32, AdamW(lr 1e-3, wd 1e-5)")
    g = torch.Generator().manual_seed(0)
    for K in (10, 1000):
        for B in (128, 1024):
            Ws, bs = _mlp_init([IN] + [HID] * LAYERS + [K], g)
            x = torch.randn(B, IN, generator=g).to(dev)
            y = torch.randint(0, K, (B,), generator=g).to(torch.int32).to(dev)
            eng = _DeviceMLP(Ws, bs, _Adam(1e-3, 1e-5, (0.9, 0.999), 1e-8), dev, B, K, 1)
            arms = {"(a) MLPProbe device step": one_step(eng, x, y), "(b) torch eager fp32 step": eager_arm(Ws, bs, x, y, dev)}
            times = interleaved(arms, args.inner, args.reps, dev)
            say()
            say(f"classes {K}, batch {B}: ms per training step, device events over {args.inner} back-to-back steps, "
                f"{args.reps} interleaved runs")
            for k, ts in times.items():
                say(f"    {k:44s} " + "  ".join(f"{t:9.4f}" for t in ts) + f"   median {med(ts):9.4f} ms")
            a, b = times["(a) MLPProbe device step"], times["(b) torch eager fp32 step"]
            say(f"    (a) / (b) medians = {med(a) / med(b):.3f};  spread of (b) = {max(b) - min(b):.4f} ms;  "
                f"(a) - (b) = {med(a) - med(b):+.4f} ms")
            times = interleaved(kernels_of(eng, x, y), args.inner, args.reps, dev)
            say("    the launches of (a), timed on their own:")
            for k, ts in times.items():
                say(f"    {k:44s} " + "  ".join(f"{t:9.4f}" for t in ts) + f"   median {med(ts):9.4f} ms")
            say(f"    sum of their medians {sum(med(ts) for ts in times.values()):.4f} ms")
            del eng, arms

    # the whole epoch from a resident container, decode included
    ds, labels = resident_dataset(args, g, dev)
    say()
    say(f"one epoch of MLPProbe.fit from a resident CompressedLatents: N = {len(ds)} records, {ds.nbytes / 2**20:.1f} MiB "
        f"compressed, 10 classes; host clock around fit(epochs=1), which ends in a synchronise (initialisation, the decode "
        f"of 2 groups of 65536 records and the label gather included); one warm-up fit, then {args.reps} runs")
    time_fits(MLPProbe, ds, labels, args, say, dev)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
