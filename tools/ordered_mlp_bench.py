"""What the ordered hyperprior mode costs on the device (run on an MI355X; output kept in profiles/ordered_mlp.txt).

  (a) ``lla_gemm_f32_ordered`` (VALU, one ascending fmaf chain per output) against ``lla_gemm_f32`` (fp32 MFMA) at the three
      layer shapes of z_encoder (102 -> 512 -> 512 -> 1024, K padded to 104) for M = 1 024 and 8 704 rows;
  (b) ``HRateHyperprior.encode_device`` and ``decode_device`` at B = 1 024 with ``mlp_precision="fp32"`` and ``"ordered"``.

Each figure is the median of ``--reps`` timed runs of ``--iters`` back-to-back calls (HIP events), after a warm-up.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lossyless_amd import _lib  # noqa: E402
from lossyless_amd.rates import HRateHyperprior, synthetic_hyperprior_state_dict  # noqa: E402


def timed(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / iters)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    L, st = _lib.lib(), _lib.stream_ptr()
    print(f"# {torch.cuda.get_device_name(0)}, library {L.lla_source_sha().decode()}, median of {args.reps} x {args.iters} calls")
    print("# (a) one Linear layer, bias + ReLU: ms per call (TFLOP/s)")
    print(f"{'M':>6} {'N':>5} {'K':>4} {'lla_gemm_f32':>22} {'lla_gemm_f32_ordered':>24} {'ratio':>6}")
    g = torch.Generator().manual_seed(0)
    for M in (1024, 8704):
        for N, K in ((512, 104), (512, 512), (1024, 512)):
            a = torch.randn(M, K, generator=g).cuda()
            w = torch.randn(N, K, generator=g).cuda()
            b = torch.randn(N, generator=g).cuda()
            c = torch.empty(M, N, device="cuda")
            ms = []
            for name in ("lla_gemm_f32", "lla_gemm_f32_ordered"):
                fn = getattr(L, name)
                call = lambda: _lib.check(fn(_lib.ptr(a), K, _lib.ptr(w), K, _lib.ptr(b), _lib.ptr(c), N, M, N, K, 1, st), name)
                ms.append(timed(call, args.iters, args.reps))
            tf = [2e-9 * M * N * K / t for t in ms]
            print(f"{M:>6} {N:>5} {K:>4} {ms[0]:>12.4f} ({tf[0]:6.2f}) {ms[1]:>14.4f} ({tf[1]:6.2f}) {ms[1] / ms[0]:>6.2f}")

    print("# (b) HRateHyperprior(512) at B = 1024, fp16 z: ms per call (images/s)")
    B = 1024
    z = (torch.randn(B, 512, generator=g) * 2).half().cuda()
    res = {}
    for mode in ("fp32", "ordered"):
        m = HRateHyperprior(512, mlp_precision=mode).eval()
        m.load_state_dict(synthetic_hyperprior_state_dict(0))
        m = m.cuda()
        payload, offsets = m.encode_device(z)
        res[mode] = (timed(lambda: m.encode_device(z), args.iters, args.reps),
                     timed(lambda: m.decode_device(payload, offsets, B), args.iters, args.reps))
    for i, what in enumerate(("encode_device", "decode_device")):
        f, o = res["fp32"][i], res["ordered"][i]
        print(f"{what:>14}  fp32 {f:8.4f} ({B / f * 1e3:10.0f})   ordered {o:8.4f} ({B / o * 1e3:10.0f})   ratio {o / f:5.3f}")


if __name__ == "__main__":
    main()
