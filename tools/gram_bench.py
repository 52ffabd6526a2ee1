#!/usr/bin/env python3
"""The Gram pass of the ridge probes, lla_gram_pass (sum z z^T and the column sums in double, from fp32 MFMA chains), against
``z.T @ z`` in torch and against lla_gemm_f32_tn on the same rows: the time of one pass over all rows and the peak device
memory, with the rows resident (fp32 and fp16) and streamed from a compressed container (``take`` of one decode group into a
reused buffer, then the pass on it).  Then one search: ``RidgeProbeCV`` (8 alphas x 5 folds) against ``LinearProbeCV`` (8 values
of C x 5 folds) on the same container, as wall time per search.

    python tools/gram_bench.py [--records 65536 1048576] [--repeats 7] [--warmup 2] [--search-records 65536] [--out FILE]

Timing: device events around a whole pass, ``--warmup`` unrecorded passes first, then ``--repeats`` passes; the median and the
min .. max spread are printed.  Memory: torch's peak allocation above what is resident before the pass.  Before anything is
timed the three results are compared (reported, not gated).  No speed-up is promised: what is printed is what was measured,
including where torch wins."""
import argparse
import os
import statistics
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hubconf  # noqa: E402
from lossyless_amd import LinearProbeCV, RidgeProbeCV, _lib  # noqa: E402

GROUP = 65536


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


def write_container(comp, z, path):
    """The container file CompressedLatents opens: be32(N) + the length-prefixed records, encoded a decode group at a time."""
    eb, t = comp.entropy_bottleneck, comp._tables()
    with open(path, "wb") as fh:
        fh.write(int(z.shape[0]).to_bytes(4, "big"))
        for g0 in range(0, z.shape[0], GROUP):
            payload, offsets, _ = eb.encode_device(z[g0:g0 + GROUP], t, record_prefix=True)
            fh.write(payload[:int(offsets[-1])].cpu().numpy().tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--search-records", type=int, default=65536, help="rows of the RidgeProbeCV / LinearProbeCV search (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gram_bench.py measures on an MI355X: no GPU here, nothing measured")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", torch.cuda.current_device())
    comp, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    C, L = comp.z_dim, _lib.lib()
    say(f"device {torch.cuda.get_device_name(dev)}, library {L.lla_source_sha().decode()}, C = {C}, rows per group {GROUP}, "
        f"{args.warmup} warm-up + {args.repeats} timed passes: median [min .. max]")
    line = lambda ts: f"{statistics.median(ts):8.2f} ms [{min(ts):.2f} .. {max(ts):.2f}]"      # noqa: E731
    ws = torch.empty(int(L.lla_gram_pass_workspace_bytes(C, 0)), dtype=torch.uint8, device=dev)
    gram, s = torch.empty((C, C), dtype=torch.float64, device=dev), torch.empty(C, dtype=torch.float64, device=dev)
    g32, part = torch.empty((C, C), device=dev), torch.empty((C, C), device=dev)

    def gram_group(z, acc):
        zt = _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32
        _lib.check(L.lla_gram_pass(_lib.ptr(z), zt, C, z.shape[0], C, None, 0, 0, _lib.ptr(gram), _lib.ptr(s), None, None, None,
                                   acc, _lib.ptr(ws), _lib.stream_ptr()), "lla_gram_pass")

    def tn_group(z, acc):
        _lib.check(L.lla_gemm_f32_tn(_lib.ptr(z), C, _lib.ptr(z), C, _lib.ptr(part if acc else g32), C, None, z.shape[0], C, C,
                                     _lib.stream_ptr()), "lla_gemm_f32_tn")
        if acc:
            g32.add_(part)

    def torch_group(z, acc):
        z = z.float() if z.dtype == torch.float16 else z
        if acc:
            g32.addmm_(z.T, z)
        else:
            torch.mm(z.T, z, out=g32)

    for N in args.records:
        g = torch.Generator().manual_seed(0)
        # 1000 clusters in 10 classes of 100: the class of a row is its cluster // 100
        means = (torch.randn(10, C, generator=g) * 0.5)[torch.arange(1000) // 100] + torch.randn(1000, C, generator=g) * 0.35
        which = torch.randint(0, 1000, (N,), generator=g)
        z = torch.cat([(means[which[g0:g0 + GROUP]] + torch.randn(min(GROUP, N - g0), C, generator=g) * 0.5).to(dev)
                       for g0 in range(0, N, GROUP)])
        with tempfile.TemporaryDirectory() as d:
            write_container(comp, z, os.path.join(d, "Z.bin"))
            ds = comp.open_dataset(os.path.join(d, "Z.bin"))
        del z
        Z = ds.all()
        Zh = Z.half()
        buf = torch.empty((min(GROUP, N), C), device=dev)
        idxs = [(g0, torch.arange(g0, min(g0 + GROUP, N), device=dev)) for g0 in range(0, N, GROUP)]
        say()
        say(f"N = {N}: {ds.nbytes / 2 ** 20:.1f} MiB compressed against {N * C * 4 / 2 ** 20:.0f} MiB of fp32 rows")

        def over(fn, rows):
            def run():
                for g0, idx in idxs:
                    fn(rows(g0, idx), int(g0 > 0))
            return run

        resident = lambda g0, idx: Z[g0:g0 + idx.numel()]                                        # noqa: E731
        resident16 = lambda g0, idx: Zh[g0:g0 + idx.numel()]                                     # noqa: E731
        streamed = lambda g0, idx: ds.take(idx, out=buf[:idx.numel()], check=False)              # noqa: E731

        over(gram_group, resident)()
        want = gram.clone()
        over(torch_group, resident)()
        e_torch = float((g32.double() - want).abs().max()) / float(want.abs().max())
        over(tn_group, resident)()
        e_tn = float((g32.double() - want).abs().max()) / float(want.abs().max())
        say(f"  against lla_gram_pass, max |difference| over the largest entry: torch z.T @ z {e_torch:.2e}, lla_gemm_f32_tn {e_tn:.2e}")
        tt, _ = measure(over(lambda z, acc: None, streamed), args.warmup, args.repeats)
        say(f"  decode alone (take of every group)           {line(tt)}")
        flops = 2.0 * N * C * C
        for name, fn in (("lla_gram_pass, fp32 rows resident  ", over(gram_group, resident)),
                         ("lla_gram_pass, fp16 rows resident  ", over(gram_group, resident16)),
                         ("lla_gram_pass, rows streamed       ", over(gram_group, streamed)),
                         ("torch z.T @ z, fp32 rows resident  ", over(torch_group, resident)),
                         ("torch z.T @ z, fp16 rows resident  ", over(torch_group, resident16)),
                         ("torch z.T @ z, rows streamed       ", over(torch_group, streamed)),
                         ("lla_gemm_f32_tn, fp32 rows resident", over(tn_group, resident)),
                         ("lla_gemm_f32_tn, rows streamed     ", over(tn_group, streamed))):
            ts, mem = measure(fn, args.warmup, args.repeats)
            say(f"    {name} {line(ts)}  {flops / statistics.median(ts) / 1e9:6.1f} TFLOP/s of z^T z  peak {mem / 2 ** 20:8.1f} MiB")
        say(f"    (lla_gram_pass's workspace, resident before the pass: {ws.numel() / 2 ** 20:.1f} MiB; its flops are counted as the "
            f"full C x C product; it walks the upper-triangular 128 x 128 tiles and skips the 32 x 32 blocks below the diagonal: "
            f"0.53 of that product at C = 512)")
        if N == args.search_records:
            y = (which // 100).numpy()
            alphas = RidgeProbeCV.logspace(8, 1e-3, 1e3)
            say(f"  search on this container, {N} rows, 10 classes, 5 stratified folds, wall time per search (second of two runs):")
            for name, make in (("RidgeProbeCV, 8 alphas ", lambda: RidgeProbeCV(alphas, cv=5)),
                               ("LinearProbeCV, 8 values of C", lambda: LinearProbeCV([(c, None) for c in np.logspace(-3, 0, 8)], cv=5))):
                for _ in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        cv = make().fit(ds, y)
                    torch.cuda.synchronize()
                    wall = time.perf_counter() - t0
                say(f"    {name} {wall:8.3f} s  ({cv.n_passes_} walks of the container; best {cv.best_params_}, "
                    f"mean held-out accuracy {float(cv.mean_scores_.max()):.4f})")
        del Z, Zh, ds, buf
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
