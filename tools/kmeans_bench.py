#!/usr/bin/env python3
"""One Lloyd pass of lla_kmeans_pass (assignment + per-cluster sums, counts and inertia) against the torch-eager formulation
on the same decoded rows: per group ``z @ c.T`` - 1/2 |c|^2, ``argmax``, ``index_add_``.  Reports the time of one pass over
all rows and the peak device memory of both, with the rows resident as an fp32 tensor and streamed from a compressed
container (``take`` of one decode group into a reused buffer, then the pass on it).

    python tools/kmeans_bench.py [--records 65536 262144] [--clusters 10 100 1000] [--repeats 7] [--warmup 2] [--out FILE]

Timing: device events around a whole pass, ``--warmup`` unrecorded passes first, then ``--repeats`` passes; the median and
the min .. max spread are printed.  Memory: torch's peak allocation above what is resident before the pass (the rows or the
container, the centres, the fused pass's workspace and outputs).  Before anything is timed the two paths' assignments and
sums are compared (fp32 in different orders: reported, not gated).  No speed-up is promised: what is printed is what was
measured, including where torch wins."""
import argparse
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hubconf  # noqa: E402
from lossyless_amd import _lib  # noqa: E402

GROUP = 65536


class Fused:
    def __init__(self, N, C, K, dev):
        L = _lib.lib()
        self.K, self.C = K, C
        self.ws = torch.empty(int(L.lla_kmeans_pass_workspace_bytes(C, K)), dtype=torch.uint8, device=dev)
        self.assign = torch.empty(N, dtype=torch.int32, device=dev)
        self.dist = torch.empty(N, device=dev)
        self.sum = torch.empty((K, C), device=dev)
        self.count = torch.empty(K, dtype=torch.float64, device=dev)
        self.stats = torch.empty(2, dtype=torch.float64, device=dev)

    def group(self, z, g0, W, b, acc):
        g = z.shape[0]
        rc = _lib.lib().lla_kmeans_pass(_lib.ptr(z), _lib.LLA_Z_F32, self.C, g, self.C, _lib.ptr(W), _lib.ptr(b), self.K, self.C, 0,
                                        _lib.ptr(self.assign[g0:]), _lib.ptr(self.dist[g0:]), _lib.ptr(self.sum),
                                        _lib.ptr(self.count), _lib.ptr(self.stats), acc, _lib.ptr(self.ws), _lib.stream_ptr())
        _lib.check(rc, "lla_kmeans_pass")


def eager_group(z, W, b, sums, count):
    s = z @ W.T + b
    best, a = s.max(1)
    sums.index_add_(0, a, z)
    count += torch.bincount(a, minlength=W.shape[0])
    return a, ((z * z).sum(1) - 2.0 * best).clamp_min_(0.0).sum(dtype=torch.float64)


def measure(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return times, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--clusters", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kmeans_bench.py measures on an MI355X: no GPU here, nothing measured")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", torch.cuda.current_device())
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    eb, t, C = comp.entropy_bottleneck, comp._tables(), comp.z_dim
    say(f"device {torch.cuda.get_device_name(dev)}, library {_lib.lib().lla_source_sha().decode()}, C = {C}, rows per group {GROUP}, "
        f"{args.warmup} warm-up + {args.repeats} timed passes: median [min .. max]")
    line = lambda ts: f"{statistics.median(ts):8.2f} ms [{min(ts):.2f} .. {max(ts):.2f}]"      # noqa: E731
    for N in args.records:
        g = torch.Generator().manual_seed(0)
        means = torch.randn(1000, C, generator=g) * 0.5
        z = (means[torch.randint(0, 1000, (N,), generator=g)] + torch.randn(N, C, generator=g) * 0.5).to(dev)
        payload, offsets, _ = eb.encode_device(z, t, record_prefix=True)
        torch.cuda.synchronize(dev)
        with tempfile.TemporaryDirectory() as d:      # the container file CompressedLatents opens: be32(N) + the body
            f = os.path.join(d, "Z.bin")
            with open(f, "wb") as fh:
                fh.write(N.to_bytes(4, "big"))
                fh.write(payload[:int(offsets[-1])].cpu().numpy().tobytes())
            ds = comp.open_dataset(f)
        del payload, offsets, z
        Z = ds.all()
        buf = torch.empty((min(GROUP, N), C), device=dev)
        idxs = [(g0, torch.arange(g0, min(g0 + GROUP, N), device=dev)) for g0 in range(0, N, GROUP)]
        say()
        say(f"N = {N}: {ds.nbytes / 2 ** 20:.1f} MiB compressed against {N * C * 4 / 2 ** 20:.0f} MiB of fp32 rows")

        def take_only():
            for _, idx in idxs:
                ds.take(idx, out=buf[:idx.numel()], check=False)

        tt, _ = measure(take_only, args.warmup, args.repeats)
        say(f"  decode alone (take of every group)   {line(tt)}")
        for K in args.clusters:
            W = Z[torch.randperm(N, generator=g)[:K].to(dev)].contiguous()
            b = (-0.5 * (W.double() ** 2).sum(1)).float()
            fused = Fused(N, C, K, dev)
            esum, ecnt = torch.empty((K, C), device=dev), torch.empty(K, dtype=torch.int64, device=dev)
            eassign = torch.empty(N, dtype=torch.int64, device=dev)
            einertia = torch.zeros((), dtype=torch.float64, device=dev)

            def fused_resident():
                for g0, idx in idxs:
                    fused.group(Z[g0:g0 + idx.numel()], g0, W, b, int(g0 > 0))

            def fused_streamed():
                for g0, idx in idxs:
                    fused.group(ds.take(idx, out=buf[:idx.numel()], check=False), g0, W, b, int(g0 > 0))

            def eager(rows_of):
                esum.zero_(), ecnt.zero_(), einertia.zero_()
                for g0, idx in idxs:
                    a, inertia = eager_group(rows_of(g0, idx), W, b, esum, ecnt)
                    eassign[g0:g0 + idx.numel()] = a
                    einertia.add_(inertia)

            eager_resident = lambda: eager(lambda g0, idx: Z[g0:g0 + idx.numel()])                       # noqa: E731
            eager_streamed = lambda: eager(lambda g0, idx: ds.take(idx, out=buf[:idx.numel()], check=False))   # noqa: E731

            fused_resident(), eager_resident()
            torch.cuda.synchronize(dev)
            same = float((fused.assign.to(torch.int64) == eassign).double().mean())
            agree = fused.assign.to(torch.int64) == eassign
            serr = float((fused.sum - esum).abs().max()) / float(esum.abs().max())
            say(f"  K = {K}: same assignment {same:.6f} of the rows; max |sum difference| {serr:.2e} of the largest sum"
                f"{'' if bool(agree.all()) else ' (rows assigned differently included)'}; inertia {float(fused.stats[0]):.6e} "
                f"against {float(einertia):.6e}")
            flops = 2.0 * N * K * C
            for name, fn in (("fused, rows resident ", fused_resident), ("eager, rows resident ", eager_resident),
                             ("fused, rows streamed ", fused_streamed), ("eager, rows streamed ", eager_streamed)):
                ts, mem = measure(fn, args.warmup, args.repeats)
                say(f"    {name} {line(ts)}  {flops / statistics.median(ts) / 1e9:6.1f} TFLOP/s of scores  peak {mem / 2 ** 20:8.1f} MiB")
            say(f"    (the fused pass's workspace, resident before the pass: {fused.ws.numel() / 2 ** 20:.1f} MiB)")
        del Z, ds, buf
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
