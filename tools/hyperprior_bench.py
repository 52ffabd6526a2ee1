"""Hyperprior dataset path, measured (MI355X; writes its table to stdout and, with --out, to a file).

(a) entropy stage alone at B = 1024 on fixed embeddings: ``HRateHyperprior.encode_device`` (records stay on the device; the
    timed call ends with the one copy of the bytes a caller needs) against the unchanged ``HRateHyperprior.compress`` (three
    host round trips), same process, arms interleaved; decode likewise.
(b) ``compress_dataset`` of N synthetic images: ``HyperpriorClipCompressor`` against the factorized ``ClipCompressor`` on
    the same tower, same process, arms interleaved.  The extra work is ~3 MFLOP per image against 8.8 GFLOP: parity is
    the expectation.

Weights are synthetic (seeded): bits/img is printed for completeness and MEANS NOTHING.

usage (GPU box): python tools/hyperprior_bench.py [--images 32768] [--reps 5] [--out profiles/hyperprior_dataset.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import hubconf  # noqa: E402
from lossyless_amd.compressor import SyntheticImages  # noqa: E402
from lossyless_amd.rates import synthetic_hyperprior_state_dict  # noqa: E402


def _timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def _summary(ts):
    return f"median {1e3 * statistics.median(ts):9.3f} ms   min {1e3 * min(ts):9.3f}   max {1e3 * max(ts):9.3f}   (n={len(ts)})"


def entropy_stage(hp, z, reps, say):
    dev = z.device
    B = z.shape[0]

    def device_arm():          # records on the device + the copy of the used bytes a writer would make
        payload, offsets = hp.encode_device(z)
        return payload[: int(offsets[-1])].cpu()

    arms = {"compress (host round trips)": lambda: hp.compress(z), "encode_device + fetch": device_arm}
    for fn in arms.values():   # warm-up: code objects, tables, allocator
        fn(), fn()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            times[k].append(_timed(fn, dev)[0])
    say(f"(a) entropy stage, B = {B} fixed embeddings, {reps} interleaved repetitions")
    for k, ts in times.items():
        say(f"    {k:30s} {_summary(ts)}   {B / statistics.median(ts):12.0f} img/s")
    base, new = (statistics.median(times[k]) for k in arms)
    say(f"    factor (median / median): {base / new:.1f}x")

    strings = hp.compress(z)
    payload, offsets = hp.encode_device(z)
    padded = torch.cat([payload[: int(offsets[-1])], torch.zeros(4, dtype=torch.uint8, device=dev)])
    assert torch.equal(hp.decode_device(padded, offsets, B), hp.decompress(strings))
    d_arms = {"decompress (strings from host)": lambda: hp.decompress(strings),
              "decode_device": lambda: hp.decode_device(padded, offsets, B)}
    d_times = {k: [] for k in d_arms}
    for _ in range(reps):
        for k, fn in d_arms.items():
            d_times[k].append(_timed(fn, dev)[0])
    for k, ts in d_times.items():
        say(f"    {k:30s} {_summary(ts)}   {B / statistics.median(ts):12.0f} img/s")
    n_bytes = sum(map(len, strings[0])) + sum(map(len, strings[1]))
    say(f"    bits/img {8 * n_bytes / B:.1f} (side {8 * sum(map(len, strings[1])) / B:.1f}) -- synthetic weights: means nothing")


def dataset(hyper, fact, n, reps, say):
    dev = torch.device("cuda")
    ds = SyntheticImages(n, seed=0)
    arms = {"ClipCompressor (factorized)": fact, "HyperpriorClipCompressor": hyper}
    times, sizes = {k: [] for k in arms}, {}
    with tempfile.TemporaryDirectory() as d:
        for k, c in arms.items():      # warm-up at full size: every shape the timed window uses
            c.compress_dataset(ds, os.path.join(d, "w.bin"), is_info=False)
        for _ in range(reps):
            for k, c in arms.items():
                f = os.path.join(d, "z.bin")
                times[k].append(_timed(lambda: c.compress_dataset(ds, f, is_info=False), dev)[0])
                sizes[k] = os.path.getsize(f)
    say(f"(b) compress_dataset, {n} synthetic images generated on the device, {reps} interleaved repetitions")
    for k, ts in times.items():
        say(f"    {k:30s} {_summary(ts)}   {n / statistics.median(ts):10.0f} img/s   "
            f"{8 * sizes[k] / n:8.1f} bits/img (synthetic weights: means nothing)")
    f_med, h_med = (statistics.median(times[k]) for k in arms)
    say(f"    hyperprior / factorized throughput: {f_med / h_med:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stage-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/hyperprior_bench.py on {torch.cuda.get_device_name(0)}")
    hyper, _ = hubconf.clip_hyperprior_compressor(synthetic_hyperprior_state_dict(0), device="cuda", clip_weights="synthetic")
    fact, _ = hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")
    z = hyper.clip(SyntheticImages(1024, seed=3).device_batch(0, 1024, "cuda"))
    entropy_stage(hyper.hyperprior, z, a.stage_reps, say)
    dataset(hyper, fact, a.images, a.reps, say)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
