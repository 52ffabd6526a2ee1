"""Random-access decode, measured (MI355X; writes its table to stdout and, with --out, to a file).

A body of N records stays resident on the device (``encode_device`` of seeded random embeddings).  For B = 1024 and
B = 65536 three arms produce B dequantised fp32 rows:

(a) ``lla_rans_decode_gather`` on a random permutation (B of the N records, no repeats),
(b) the same call on ``arange(B)``,
(c) the two-kernel path it fuses, on CONTIGUOUS records already resident: ``decode_device`` (``lla_rans_decode_batch``,
    int32 symbols to global memory) then ``lla_dequantise`` -- the arrangement most favourable to that path (for a
    shuffled batch it would first have to rebuild a contiguous sub-body).

Every arm is warmed up, then timed with device events over ``--inner`` back-to-back calls; the arms are interleaved and
the whole round is repeated ``--reps`` times (3: the bar compares (a) with the spread of (c)'s own runs).  (a) is
checked against (c) on the same records before anything is timed.

usage (GPU box): python tools/latents_bench.py [--records 131072] [--reps 3] [--out profiles/latents_gather.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import hubconf  # noqa: E402
from lossyless_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=0, help="calls per timed window (0: 1000 at B = 1024, 400 at B = 65536: windows of 0.15 - 0.3 s)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("latents_bench.py measures on an MI355X: no GPU here, nothing measured")

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", torch.cuda.current_device())
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    eb, t = comp.entropy_bottleneck, comp._tables()
    L, N, C = _lib.lib(), args.records, comp.z_dim
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(N, C, generator=g) * 0.5).to(dev)
    payload, offsets, _ = eb.encode_device(z, t, record_prefix=True)
    torch.cuda.synchronize(dev)
    total = int(offsets[-1])
    payload = torch.cat([payload[:total], torch.zeros(8, dtype=torch.uint8, device=dev)])   # the resident body, padded
    say(f"device: {torch.cuda.get_device_name(dev)}   N = {N} records resident, {total / N:.1f} B/record "
        f"({total / 2**20:.1f} MiB against {N * C * 4 / 2**20:.0f} MiB of fp32 rows)")

    def gather(idx, out, status):
        rc = L.lla_rans_decode_gather(_lib.ptr(payload), _lib.ptr(offsets), 1, N, _lib.ptr(idx), idx.numel(), C,
                                      _lib.ptr(t["cdf"]), t["W"], _lib.ptr(t["cdf_len"]), _lib.ptr(t["offset"]),
                                      _lib.ptr(t["bias"]), _lib.ptr(t["exp_scale"]), _lib.ptr(t["median"]), _lib.ptr(out),
                                      _lib.LLA_Z_F32, C, _lib.ptr(status), _lib.stream_ptr(dev))
        _lib.check(rc, "lla_rans_decode_gather")

    def two_kernels(B, out):
        sym, status = eb.decode_device(payload, offsets, B, t, record_prefix=True)
        rc = L.lla_dequantise(_lib.ptr(sym), B, C, _lib.ptr(t["bias"]), _lib.ptr(t["exp_scale"]), _lib.ptr(t["median"]),
                              _lib.ptr(out), _lib.stream_ptr(dev))
        _lib.check(rc, "lla_dequantise")
        return status

    def window(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / inner      # ms per call

    for B in (1024, 65536):
        if B > N:
            continue
        inner = args.inner or (1000 if B <= 1024 else 400)
        perm = torch.randperm(N, generator=g)[:B].to(dev)
        ident = torch.arange(B, device=dev)
        out_a, out_c = (torch.empty((B, C), dtype=torch.float32, device=dev) for _ in range(2))
        status = torch.empty(B, dtype=torch.int32, device=dev)
        arms = {"(a) gather, random permutation": lambda: gather(perm, out_a, status),
                "(b) gather, arange": lambda: gather(ident, out_a, status),
                "(c) decode_batch + dequantise": lambda: two_kernels(B, out_c)}
        # same rows from both paths, before anything is timed
        gather(ident, out_a, status)
        st_c = two_kernels(B, out_c)
        torch.cuda.synchronize(dev)
        assert int(status.max()) == 0 and int(st_c.max()) == 0 and torch.equal(out_a, out_c), "arms disagree"
        for fn in arms.values():                 # warm-up of every arm at this shape
            fn(), fn()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():
                times[k].append(window(fn, inner))
        say()
        say(f"B = {B}: ms per call, device events over {inner} back-to-back calls, {args.reps} interleaved runs")
        for k, ts in times.items():
            runs = "  ".join(f"{x:9.4f}" for x in ts)
            say(f"    {k:34s} {runs}   median {sorted(ts)[len(ts) // 2]:9.4f} ms   {B / sorted(ts)[len(ts) // 2] / 1e3:8.2f} M rows/s")
        a, c = times["(a) gather, random permutation"], times["(c) decode_batch + dequantise"]
        med = lambda ts: sorted(ts)[len(ts) // 2]
        say(f"    (a) / (c) medians = {med(a) / med(c):.3f};  spread of (c) = {max(c) - min(c):.4f} ms;  "
            f"(a) - (c) = {med(a) - med(c):+.4f} ms")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
