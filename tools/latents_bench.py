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

``--hyperprior`` measures ``HyperpriorLatents`` the same way (weights of ``synthetic_hyperprior_state_dict(0)``, the
records of ``encode_device``): (a) ``take`` of a random permutation, (b) ``take(arange)``, (c) the path it has to match,
``HRateHyperprior.decode_device`` on the contiguous first B images (two records each) of the same body; then the three
steps of (a) on their own -- side gather, MLP, conditional gather -- each timed the same way.

usage (GPU box): python tools/latents_bench.py [--records 131072] [--reps 3] [--out profiles/latents_gather.txt]
                 python tools/latents_bench.py --hyperprior --out profiles/hyperprior_latents.txt
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import hubconf  # noqa: E402
from lossyless_amd import _lib  # noqa: E402


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner      # ms per call


def med(ts):
    return sorted(ts)[len(ts) // 2]


def interleaved(arms, inner, reps, dev):
    """Warm every arm up, then time the arms in turn, ``reps`` rounds -> {name: [ms per call of every round]}."""
    for fn in arms.values():
        fn(), fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            times[k].append(window(fn, inner))
    return times


def table(say, times, B):
    for k, ts in times.items():
        runs = "  ".join(f"{x:9.4f}" for x in ts)
        say(f"    {k:34s} {runs}   median {med(ts):9.4f} ms   {B / med(ts) / 1e3:8.2f} M rows/s")


def hyperprior(args, say, dev):
    """The three arms and the per-step times of ``HyperpriorLatents.take`` (module docstring)."""
    import tempfile
    from lossyless_amd.hyperprior_compressor import HyperpriorClipCompressor
    from lossyless_amd.rates import synthetic_hyperprior_state_dict
    comp = HyperpriorClipCompressor(synthetic_hyperprior_state_dict(0), device="cuda", clip_weights="synthetic")
    m, L, N, C = comp.hyperprior, _lib.lib(), args.records, comp.z_dim
    g = torch.Generator().manual_seed(0)
    chunks, base = [], 0
    offsets = [torch.zeros(1, dtype=torch.int64, device=dev)]
    for i in range(0, N, 16384):                 # (coded in pieces: the encoder's scratch is sized by the batch)
        z = (torch.randn(min(16384, N - i), C, generator=g) * 0.7).to(dev)
        p, o = m.encode_device(z)
        used = int(o[-1])
        chunks.append(p[:used].clone())
        offsets.append(o[1:] + base)
        base += used
    payload = torch.cat(chunks + [torch.zeros(8, dtype=torch.uint8, device=dev)])
    offsets = torch.cat(offsets)
    del chunks
    with tempfile.TemporaryDirectory() as d:     # the container file HyperpriorLatents opens: be32(2N) + the body
        f = os.path.join(d, "Z.bin")
        with open(f, "wb") as fh:
            fh.write((2 * N).to_bytes(4, "big"))
            fh.write(payload[:base].cpu().numpy().tobytes())
        ds = comp.open_dataset(f)
    say(f"device: {torch.cuda.get_device_name(dev)}   N = {N} images resident, {base / N:.1f} B/image in two records "
        f"({ds.nbytes / 2**20:.1f} MiB with the offsets against {N * C * 4 / 2**20:.0f} MiB of fp32 rows)")

    r = ds.lds_report()
    say(f"conditional gather: {r['granted']} B of dynamic LDS granted per workgroup; front {r['front']} B + packed rows "
        f"{r['packed_rows']} B = {r['front'] + r['packed_rows']} B -> rows searched in "
        f"{'LDS' if r['rows_in_lds'] else 'GLOBAL MEMORY (fallback)'}")
    assert r["rows_in_lds"], "the packed rows of the 64-level table must stay in LDS"
    p, ebt, gct = m._device_params(), m.entropy_bottleneck.device_tables(), m.gaussian_conditional.device_tables()
    for B in (1024, 65536):
        if B > N:
            continue
        inner = args.inner or (200 if B <= 1024 else 40)
        perm = torch.randperm(N, generator=g)[:B].to(dev)
        ident = torch.arange(B, device=dev)
        out_a = torch.empty((B, C), dtype=torch.float32, device=dev)
        sub_off = offsets[:2 * B + 1].contiguous()
        # same rows from both paths, before anything is timed
        ds.take(ident, out=out_a)
        assert torch.equal(out_a, m.decode_device(payload, sub_off, B)), "arms disagree"
        assert torch.equal(ds.take(perm)[:64], ds.take(perm[:64])), "take depends on the batch"
        arms = {"(a) take, random permutation": lambda: ds.take(perm, out=out_a, check=False),
                "(b) take, arange": lambda: ds.take(ident, out=out_a, check=False),
                "(c) decode_device, contiguous": lambda: m.decode_device(payload, sub_off, B)}
        times = interleaved(arms, inner, args.reps, dev)
        say()
        say(f"B = {B}: ms per call, device events over {inner} back-to-back calls, {args.reps} interleaved runs")
        table(say, times, B)
        a, c = times["(a) take, random permutation"], times["(c) decode_device, contiguous"]
        say(f"    (a) / (c) medians = {med(a) / med(c):.3f};  spread of (c) = {max(c) - min(c):.4f} ms;  "
            f"(a) - (c) = {med(a) - med(c):+.4f} ms;  bar (a) - (c) <= spread of (c): "
            f"{'met' if med(a) - med(c) <= max(c) - min(c) else 'MISSED'}")

        # the steps of (a), each in its own windows, on the buffers take() uses
        s_hat, status, acts = ds._buffers(B)
        S, st = m.side_z_dim, _lib.stream_ptr(dev)

        def side():
            _lib.check(L.lla_rans_decode_gather_strided(
                _lib.ptr(ds._body), _lib.ptr(ds._off), 1, 1, 2, N, _lib.ptr(perm), B, S, _lib.ptr(ebt["cdf"]), ebt["W"],
                _lib.ptr(ebt["cdf_len"]), _lib.ptr(ebt["offset"]), _lib.ptr(p["side_bias"]), _lib.ptr(p["side_scale"]),
                _lib.ptr(ebt["median"]), _lib.ptr(s_hat), _lib.LLA_Z_F32, s_hat.shape[1], _lib.ptr(status[0]), st),
                "lla_rans_decode_gather_strided")

        params = m.z_encoder.forward_padded(s_hat, acts)

        def cond():
            _lib.check(L.lla_gaussian_decode_gather(
                _lib.ptr(ds._body), _lib.ptr(ds._off), 1, 0, 2, N, _lib.ptr(perm), B, C, _lib.ptr(p["bias"]),
                _lib.ptr(p["exp_scale"]), _lib.ptr(params), params.stride(0), _lib.ptr(p["scale_table"]), p["scale_bound"],
                _lib.ptr(gct["cdf"]), gct["T"], gct["W"], _lib.ptr(gct["cdf_len"]), _lib.ptr(gct["offset"]),
                _lib.ptr(out_a), _lib.LLA_Z_F32, C, _lib.ptr(status[0]), _lib.ptr(status[1]), st),
                "lla_gaussian_decode_gather")

        # ... and the steps of (c) the last two are to be held against
        side_sym = torch.empty((B, S), dtype=torch.int32, device=dev)
        z_hat = torch.empty((B, C), dtype=torch.float32, device=dev)

        def side_c():
            _lib.check(L.lla_rans_decode_batch_strided(
                _lib.ptr(payload), _lib.ptr(sub_off), 1, 1, 2, B, S, _lib.ptr(ebt["cdf"]), ebt["W"], _lib.ptr(ebt["cdf_len"]),
                _lib.ptr(ebt["offset"]), _lib.ptr(side_sym), _lib.ptr(status[0]), st), "lla_rans_decode_batch_strided")

        def cond_c():
            _lib.check(L.lla_gaussian_decode_dequantise(
                _lib.ptr(payload), _lib.ptr(sub_off), 1, 0, 2, B, C, _lib.ptr(p["bias"]), _lib.ptr(p["exp_scale"]),
                _lib.ptr(params), params.stride(0), _lib.ptr(p["scale_table"]), p["scale_bound"], _lib.ptr(gct["cdf"]),
                gct["T"], gct["W"], _lib.ptr(gct["cdf_len"]), _lib.ptr(gct["offset"]), _lib.ptr(z_hat),
                _lib.ptr(status[1]), st), "lla_gaussian_decode_dequantise")

        side(), side_c()
        steps = {"(a) step 1: side gather": side,
                 "(a) step 2: MLP (3 x lla_gemm_f32)": lambda: m.z_encoder.forward_padded(s_hat, acts),
                 "(a) step 3: conditional gather": cond,
                 "(c) side: decode_batch_strided": side_c,
                 "(c) MLP: _scales_of": lambda: m._scales_of(side_sym),
                 "(c) z: gaussian_decode_dequantise": cond_c}
        times = interleaved(steps, inner, args.reps, dev)
        say(f"    steps, timed on their own ({inner} back-to-back calls, {args.reps} interleaved runs):")
        table(say, times, B)
        torch.cuda.synchronize(dev)
        assert int(status.max()) == 0
        say(f"    working buffers cached by take() at this B: {ds.workspace_nbytes / 2**20:.1f} MiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=0, help="calls per timed window (0: 1000 at B = 1024, 400 at B = 65536: windows of 0.15 - 0.3 s; with --hyperprior 200 and 40)")
    ap.add_argument("--hyperprior", action="store_true", help="measure HyperpriorLatents.take instead (DESIGN.md 5.9)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("latents_bench.py measures on an MI355X: no GPU here, nothing measured")

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", torch.cuda.current_device())
    if args.hyperprior:
        hyperprior(args, say, dev)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
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
        times = interleaved(arms, inner, args.reps, dev)     # (every arm warmed up at this shape first)
        say()
        say(f"B = {B}: ms per call, device events over {inner} back-to-back calls, {args.reps} interleaved runs")
        table(say, times, B)
        a, c = times["(a) gather, random permutation"], times["(c) decode_batch + dequantise"]
        say(f"    (a) / (c) medians = {med(a) / med(c):.3f};  spread of (c) = {max(c) - min(c):.4f} ms;  "
            f"(a) - (c) = {med(a) - med(c):+.4f} ms")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
