"""Entropy-stage micro-benchmark (bench.py's entropy_stage / hyperprior legs alone).
usage (GPU box): python tools/entropy_bench.py
                 python tools/entropy_bench.py --wide [--out FILE]    the windowed coder (lla_*_wide) against the resident
                     kernels at 512 x 33, and alone on shapes the resident kernels refuse, the window swept"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import hubconf  # noqa: E402

WIDE = "--wide" in sys.argv
comp = None if WIDE else hubconf.clip_compressor_b005(device="cuda", clip_weights="synthetic")[0]
if not WIDE and not (len(sys.argv) > 1 and sys.argv[1] == "--raw-decode"):
    e = bench.entropy_stage_leg(comp, "cuda")
    print({k: e[k] for k in ("img_per_sec", "decode_img_per_sec", "bits_per_img")})
    h = bench.hyperprior_leg("cuda")
    print({k: h[k] for k in ("encode_rows_per_sec", "decode_rows_per_sec", "encode_ms", "decode_ms")})


def raw_decode_timing(B=1024, iters=20):
    """Decode timing without the equality check (timing only)."""
    import numpy as np
    import torch
    from lossyless_amd import _lib
    t = comp._tables()
    rng = np.random.default_rng(2)
    z = torch.from_numpy(rng.normal(size=(B, 512)).astype(np.float32) * 0.3).cuda()
    eb = comp.entropy_bottleneck
    payload, offsets, _ = eb.encode_device(z, t, record_prefix=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for B_ in (B,):
        eb.decode_device(payload, offsets, B_, t, record_prefix=True)
        e0.record()
        for _ in range(iters):
            eb.decode_device(payload, offsets, B_, t, record_prefix=True)
        e1.record()
        torch.cuda.synchronize()
        print(f"raw decode B={B_}: {e0.elapsed_time(e1) / iters * 1e3:.1f} us per batch")


if len(sys.argv) > 1 and sys.argv[1] == "--raw-decode":
    raw_decode_timing()
    raw_decode_timing(B=16384)


def wide_leg(out=None, B=8192, rounds=5, inner=10):
    """Encode, decode and gather of B records: device-event times of `inner` back-to-back launches, the median of
    `rounds` rounds, the arms of one shape alternating within a round.  The tables are random (a different row length per
    channel up to W), the symbols drawn inside them with 2 % escapes; every arm's output is compared with the first arm's
    before it is timed.  GB/s counts the bytes the kernel writes: int32 symbols for the decoder, fp32 rows for the gather,
    the coded streams for the encoder (its input is 4 B * C bytes per record)."""
    import ctypes
    import numpy as np
    import torch
    from lossyless_amd import _lib
    from lossyless_amd.entropy import pmf_to_quantized_cdf
    L = _lib.lib()
    lines = []

    def say(msg):
        print(msg, flush=True)
        lines.append(msg)

    def tables(C, W, seed):
        rng = np.random.default_rng(seed)
        cdf, cdf_len = np.zeros((C, W), np.int32), rng.integers(max(3, W // 2), W + 1, size=C).astype(np.int32)
        for c in range(C):
            pmf = rng.random(int(cdf_len[c]) - 1) + 0.02
            pmf[-1] *= 0.05
            cdf[c, :cdf_len[c]] = pmf_to_quantized_cdf(pmf / pmf.sum()).astype(np.int64)
        offset = (-(cdf_len // 2)).astype(np.int32)
        sym = offset[None, :] + (rng.random((B, C)) * (cdf_len - 2)[None, :]).astype(np.int32)
        esc = rng.random((B, C)) < 0.02
        sym = np.where(esc, sym + rng.integers(40, 4000, size=(B, C)), sym).astype(np.int32)
        f32 = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
        d = {k: torch.from_numpy(v).cuda() for k, v in dict(cdf=cdf, cdf_len=cdf_len, offset=offset).items()}
        d.update(bias=f32(rng.normal(0, 0.2, C)), exp_scale=f32(np.exp(rng.normal(0, 0.3, C))), median=f32(rng.uniform(-0.5, 0.5, C)))
        return d, torch.from_numpy(sym).cuda()

    def timed(arms):
        """{name: fn} -> {name: median ms per launch}; a round times every arm once, in turn."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = {k: [] for k in arms}
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in arms.items():
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / inner)
        return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}

    def shape(C, W, windows):
        d, sym = tables(C, W, seed=C + W)
        st = _lib.stream_ptr()
        stride = int(L.lla_rans_max_encoded_bytes(C))
        scratch = torch.empty(B * stride, dtype=torch.uint8, device="cuda")
        lengths = torch.empty(B, dtype=torch.int32, device="cuda")
        tab = (_lib.ptr(d["cdf"]), W, _lib.ptr(d["cdf_len"]), _lib.ptr(d["offset"]))
        aff = (_lib.ptr(d["bias"]), _lib.ptr(d["exp_scale"]), _lib.ptr(d["median"]))
        fits = [L.lla_rans_table_fits(C, W, k) for k in range(3)]
        say(f"--- C = {C}, W = {W}, B = {B}: resident entry points take it: encode {fits[0]}, decode {fits[1]}, gather {fits[2]}")

        def enc(window):
            if window is None:
                return lambda: _lib.check(L.lla_rans_encode_batch(_lib.ptr(sym), B, C, *tab, _lib.ptr(scratch), stride,
                                                                  _lib.ptr(lengths), st), "encode")
            return lambda: _lib.check(L.lla_quantise_encode_wide(_lib.ptr(sym), _lib.LLA_Z_SYMBOLS, B, C, None, None, None, *tab,
                                                                 _lib.ptr(scratch), stride, _lib.ptr(lengths), None, window, st),
                                      "encode_wide")
        arms = {"resident": None} if all(fits) else {}
        arms.update({f"window {w}": w for w in windows})
        enc(next(iter(arms.values())))()
        from lossyless_amd.entropy import EntropyBottleneck
        payload, offsets = EntropyBottleneck.compact_device(scratch, stride, lengths, B, record_prefix=True)
        ref_len = lengths.clone()
        coded = int(ref_len.sum())
        out = torch.empty((B, C), dtype=torch.int32, device="cuda")
        z = torch.empty((B, C), dtype=torch.float32, device="cuda")
        status = torch.empty(B, dtype=torch.int32, device="cuda")
        idx = torch.randperm(B, generator=torch.Generator().manual_seed(1)).cuda()
        head = (_lib.ptr(payload), _lib.ptr(offsets), 1)

        def dec(window):
            if window is None:
                return lambda: _lib.check(L.lla_rans_decode_batch(*head, B, C, *tab, _lib.ptr(out), _lib.ptr(status), st), "decode")
            return lambda: _lib.check(L.lla_rans_decode_batch_wide(*head, 0, 1, B, C, *tab, _lib.ptr(out), _lib.ptr(status), window,
                                                                   st), "decode_wide")

        def gat(window):
            tail = (B, _lib.ptr(idx), B, C, *tab, *aff, _lib.ptr(z), _lib.LLA_Z_F32, C, _lib.ptr(status))
            if window is None:
                return lambda: _lib.check(L.lla_rans_decode_gather(*head, *tail, st), "gather")
            return lambda: _lib.check(L.lla_rans_decode_gather_wide(*head, 0, 1, *tail, window, st), "gather_wide")

        z_ref = None
        for name, w in arms.items():      # every arm computes the same thing, checked before anything is timed
            lengths.zero_()
            enc(w)()
            assert torch.equal(lengths, ref_len), f"encode {name}: lengths differ"
            out.zero_()
            dec(w)()
            assert torch.equal(out, sym) and int(status.max()) == 0, f"decode {name}: symbols differ"
            z.zero_()
            gat(w)()
            z_ref = z.clone() if z_ref is None else z_ref
            assert torch.equal(z, z_ref) and int(status.max()) == 0, f"gather {name}: rows differ"
        for kernel, make, kind, written in (("encode", enc, 0, coded), ("decode", dec, 1, 4 * B * C), ("gather", gat, 2, 4 * B * C)):
            t = timed({k: make(w) for k, w in arms.items()})
            for k, w in arms.items():
                if w is None:
                    info = "whole table resident"
                else:
                    lds = ctypes.c_size_t(0)
                    wc = L.lla_rans_wide_window(C, W, kind, w, ctypes.byref(lds))
                    nwin = -(-C // wc)
                    info = (f"{wc} channels x {nwin} windows, LDS {lds.value} B / workgroup, "
                            f"{2 * C * W + 32 * C} B of rows and parameters staged / workgroup")
                med, lo, hi = t[k]
                say(f"{kernel:6s} {k:11s} {med * 1e3:9.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  {B / med / 1e3:8.2f} M rec/s  "
                    f"{written / med / 1e6:7.2f} GB/s written  [{info}]")

    say(f"windowed coder, {torch.cuda.get_device_name(0)}; median of {rounds} rounds of {inner} launches, device events")
    shape(512, 33, (0, 16, 48, 192))       # (192 x 33: the largest window here whose two buffers leave the gather its staging)
    shape(1024, 33, (0, 16, 48, 192))
    shape(2048, 33, (0, 16, 48, 192))
    shape(512, 129, (0, 4, 32, 64))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if WIDE:
    wide_leg(out=sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None)
