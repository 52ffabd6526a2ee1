#!/usr/bin/env python3
"""The fused k-NN pass (lla_knn_pass + lla_knn_finish) against the torch-eager formulation on the same resident decoded
rows: per group of rows ``q @ z.T``, ``topk``, merge with the running list.  Reports the time of one search (every group
of the train rows once) and the peak device memory of both, and the insertions the fused pass made.

    python tools/knn_bench.py [--repeats 7] [--warmup 2] [--group 65536]

Timing: device events around a whole search, ``--warmup`` unrecorded runs first, then ``--repeats`` runs; the median and
the min .. max spread are printed.  Memory: torch's peak allocation above what the operands themselves take.  The eager
path returns its neighbours in topk's order (ties in no fixed order); the fused pass's contract is stricter, so only the
scores of the two are compared."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lossyless_amd import _lib  # noqa: E402

SHAPES = [("Q 8192 x N 131072 x C 512, k 20", 8192, 131072, 512, 20),
          ("Q 8192 x N 131072 x C 512, k 200", 8192, 131072, 512, 200),
          ("Q 8000 x N 5000 x C 512, k 20 (STL10-like)", 8000, 5000, 512, 20),
          ("Q 8000 x N 5000 x C 512, k 200 (STL10-like)", 8000, 5000, 512, 200)]


def fused(q, z, k, group, ws):
    L, Q, C, n = _lib.lib(), q.shape[0], q.shape[1], z.shape[0]
    st, acc = _lib.stream_ptr(), 0
    for g0 in range(0, n, group):
        g = min(group, n - g0)
        _lib.check(L.lla_knn_pass(_lib.ptr(q), C, Q, _lib.ptr(z[g0:g0 + g]), _lib.LLA_Z_F32, C, g, C, g0, k, 1, None, acc,
                                  _lib.ptr(ws), st), "lla_knn_pass")
        acc = 1
    val = torch.empty((Q, k), device=q.device)
    idx = torch.empty((Q, k), dtype=torch.int32, device=q.device)
    _lib.check(L.lla_knn_finish(Q, k, k, None, 0, 0.0, _lib.ptr(val), _lib.ptr(idx), None, _lib.ptr(ws), st), "lla_knn_finish")
    return val, idx


def eager(q, z, k, group):
    val = idx = None
    for g0 in range(0, z.shape[0], group):
        zg = z[g0:g0 + group]
        s = (q @ zg.T) / zg.norm(dim=1)[None, :]
        v, i = torch.topk(s, min(k, s.shape[1]), dim=1)
        i = i + g0
        if val is not None:
            v, at = torch.topk(torch.cat([val, v], 1), k, dim=1)
            i = torch.gather(torch.cat([idx, i], 1), 1, at)
        val, idx = v, i
    return val, idx


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
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return out, times, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--group", type=int, default=65536)
    args = ap.parse_args()
    print(f"device {torch.cuda.get_device_name(0)}, library {_lib.lib().lla_source_sha().decode()}, rows per group {args.group}, "
          f"{args.warmup} warm-up + {args.repeats} timed searches: median [min .. max]")
    for name, Q, N, C, k in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        z = torch.randn(N, C, device="cuda", generator=g)
        q = torch.randn(Q, C, device="cuda", generator=g)
        q = q / q.norm(dim=1, keepdim=True)
        ws = torch.zeros(int(_lib.lib().lla_knn_pass_workspace_bytes(Q, k)), dtype=torch.uint8, device="cuda")
        (fv, fi), ft, fm = measure(lambda: fused(q, z, k, args.group, ws), args.warmup, args.repeats)
        inserted = int(ws[-8:].view(torch.int64).item()) / (args.warmup + args.repeats)
        (ev, ei), et, em = measure(lambda: eager(q, z, k, args.group), args.warmup, args.repeats)
        flops = 2.0 * Q * N * C
        line = lambda t: f"{statistics.median(t):8.2f} ms [{min(t):.2f} .. {max(t):.2f}]"      # noqa: E731
        print(f"{name}")
        print(f"  fused  {line(ft)}  {flops / statistics.median(ft) / 1e9:6.1f} TFLOP/s  peak {fm / 2 ** 20:8.1f} MiB above the "
              f"operands (workspace {ws.numel() / 2 ** 20:.1f} MiB more)")
        print(f"  eager  {line(et)}  {flops / statistics.median(et) / 1e9:6.1f} TFLOP/s  peak {em / 2 ** 20:8.1f} MiB")
        print(f"  insertions per search {inserted:.0f} = {inserted / Q:.1f} per query, {inserted / (Q * N):.2e} of the candidates; "
              f"max |score difference| {float((fv - ev).abs().max()):.2e}, same neighbours {float((fi == ei).float().mean()):.4f}")


if __name__ == "__main__":
    main()
