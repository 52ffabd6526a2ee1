#!/usr/bin/env python3
"""Time the device text tower (lossyless_amd.clip_text.TextTransformer) against the same network written with torch ops in
fp32 eager, on the same GPU, in one process.

  device   lla_text_embed, lla_layernorm_rows, lla_gemm_f32, lla_attention_causal, lla_text_pointwise (csrc/text_tower.hip)
  eager    F.embedding, F.layer_norm, F.linear, matmul + masked softmax attention, x * sigmoid(1.702 x), fp32, in chunks of
           the same 256 prompts
Shapes: the ViT-B/32 text tower (width 512, 12 layers, 8 heads, context 77, embedding 512; synthetic weights, vocabulary cut to
`--vocab` rows -- the embedding is a gather), P prompts at full length (EOT at position 76) and with the EOT at position 12,
`truncate` on and off.  The eager arm always runs the full 77 positions (that is what `encode_text` does).  The arms alternate;
both start every pass from host token ids (the eager arm copies them to the device, the device arm also validates them and
takes the EOT positions on the host, and copies a chunk at a time);
each window is as many forward passes as fill `--window` seconds and ends in a device synchronise, after `--warmup` passes of
every shape.  Reported: the median (min .. max) of the windows, prompts/s, and the TFLOP/s of the GEMM class that the device
arm's whole-pass time implies (its FLOPs counted from the shapes at the length the pass ran at) against the 157.3 TFLOP/s fp32
matrix peak -- an end-to-end figure, not a kernel's share of peak; per-kernel shares come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/text_tower_bench.py --prompts 1024 --repeats 1` run.

    python tools/text_tower_bench.py [--out profiles/text_tower.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lossyless_amd import _lib                                                              # noqa: E402
from lossyless_amd.clip_text import TextTransformer, synthetic_text_state_dict             # noqa: E402

PEAK_FP32_MATRIX = 157.3e12


def eager_forward(W, tok, layers, heads, chunk):
    out = []
    T = tok.shape[1]
    mask = torch.full((T, T), float("-inf"), device=tok.device).triu(1)
    for c0 in range(0, tok.shape[0], chunk):
        t = tok[c0:c0 + chunk]
        P = t.shape[0]
        x = F.embedding(t, W["token_embedding.weight"]) + W["positional_embedding"][:T]
        D = x.shape[-1]
        for l in range(layers):
            p = f"transformer.resblocks.{l}."
            h = F.layer_norm(x, (D,), W[p + "ln_1.weight"], W[p + "ln_1.bias"], 1e-5)
            q, k, v = (a.reshape(P, T, heads, 64).transpose(1, 2)
                       for a in F.linear(h, W[p + "attn.in_proj_weight"], W[p + "attn.in_proj_bias"]).chunk(3, -1))
            a = torch.softmax(q @ k.transpose(-1, -2) / 8 + mask, -1) @ v
            x = x + F.linear(a.transpose(1, 2).reshape(P, T, D), W[p + "attn.out_proj.weight"], W[p + "attn.out_proj.bias"])
            h = F.linear(F.layer_norm(x, (D,), W[p + "ln_2.weight"], W[p + "ln_2.bias"], 1e-5), W[p + "mlp.c_fc.weight"],
                         W[p + "mlp.c_fc.bias"])
            x = x + F.linear(h * torch.sigmoid(1.702 * h), W[p + "mlp.c_proj.weight"], W[p + "mlp.c_proj.bias"])
        pooled = x[torch.arange(P, device=x.device), t.argmax(-1)]
        out.append(F.layer_norm(pooled, (D,), W["ln_final.weight"], W["ln_final.bias"], 1e-5) @ W["text_projection"])
    return torch.cat(out)


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def gemm_flops(P, T, D, layers, E):
    return 2.0 * P * T * layers * (3 * D * D + D * D + 8 * D * D) + 2.0 * P * D * E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_tower_bench needs an MI355X: a CPU run says nothing about time")
    dev = torch.device("cuda")
    sd = synthetic_text_state_dict(seed=1, vocab=a.vocab)
    W = {k: v.to(dev) for k, v in sd.items()}
    towers = {tr: TextTransformer(sd, chunk=a.chunk, truncate=tr).to(dev) for tr in (True, False)}
    D, layers, E = 512, 12, 512
    lines = [f"# text tower, ViT-B/32 text shape (width 512, 12 layers, 8 heads, context 77), fp32: device kernels vs torch eager, same "
             f"process; {a.repeats} windows of at least {a.window} s per arm, arms alternating, after {a.warmup} warm-up pass(es); chunks "
             f"of {a.chunk} prompts; both arms take host token ids on every pass; library sha {_lib.lib().lla_source_sha().decode()}; {torch.cuda.get_device_name(0)}",
             "#      P  EOT  truncate   device s/pass (min..max)   prompts/s   GEMM-class TFLOP/s (of 157.3 peak)   eager s/pass (min..max)   "
             "prompts/s   eager/device   max |device - eager| / max |eager|"]
    for P in a.prompts:
        for eot in (76, 12):
            rng = np.random.default_rng(P + eot)
            tok = rng.integers(1, a.vocab - 1, size=(P, 77))
            tok[:, eot], tok[:, eot + 1:] = a.vocab - 1, 0
            # both arms start from the host's token ids: the eager arm copies them up on every pass, the device arm also
            # checks their range and finds the EOT positions on the host (TextTransformer.forward)
            estep = lambda: eager_forward(W, torch.from_numpy(tok).to(dev), layers, 8, a.chunk)   # noqa: E731
            ref = estep()
            for tr in (True, False):
                tower = towers[tr]
                dstep = lambda: tower(tok)                                                  # noqa: E731
                diff = float((dstep() - ref).abs().max() / ref.abs().max())
                for _ in range(a.warmup):
                    dstep(), estep()
                nd = max(1, int(a.window / window(dstep, 1)) + 1)
                ne = max(1, int(a.window / window(estep, 1)) + 1)
                d, e = [], []
                for _ in range(a.repeats):
                    d.append(window(dstep, nd))
                    e.append(window(estep, ne))
                md, me = statistics.median(d), statistics.median(e)
                T = eot + 1 if tr else 77
                tf = gemm_flops(P, T, D, layers, E) / md / 1e12
                lines.append(f"{P:8d} {eot:4d} {str(tr):>9s}   {md:8.4f} ({min(d):.4f}..{max(d):.4f})   {P / md:10.1f}   "
                             f"{tf:7.2f} ({100 * tf * 1e12 / PEAK_FP32_MATRIX:.1f} %)   {me:8.4f} ({min(e):.4f}..{max(e):.4f})   "
                             f"{P / me:10.1f}   {me / md:6.2f}x   {diff:.2e}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
