"""Shared by test_text_tower_host.py, test_gpu_text_tower.py and test_gpu_zero_shot_probe.py: references of the text
tower's kernels, generic in the dtype (float64 = the reference, float32 on the CPU = the arm the bound is taken from), the
bound rule, token and weight fixtures (no test in here).

The bound rule (DESIGN.md 5.19's): the device's error against float64 must stay within FACTOR x the error of the same
computation done by torch in fp32 on the CPU against float64; an error is the largest absolute difference over the tensor
relative to the tensor's largest magnitude.  The bound comes from the two reference arms, never from the device result."""
import functools

import numpy as np
import torch
import torch.nn as nn

FACTOR = 4.0
EPS = 1e-5


def rel_err(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def bound_of(fp32_arm, ref):
    return FACTOR * rel_err(fp32_arm, ref)


def held(name, got, fp32_arm, ref):
    """Print the measured error and its bound, then assert."""
    err, bound = rel_err(got, ref), bound_of(fp32_arm, ref)
    print(f"{name}: error {err:.3g} bound {bound:.3g}")
    assert err <= bound, (name, err, bound)          # (a zero bound -- both arms exact -- asks for exactness)
    return err, bound


# ------------------------------------------------------------------ kernel references (any float dtype)
def ref_embed(tokens, tok_emb, pos):
    return (tok_emb[tokens.long()] + pos[None, :tokens.shape[1]]).reshape(-1, tok_emb.shape[1])


def ref_layernorm(x, w, b, eps=EPS):
    c = x - x.mean(-1, keepdim=True)
    return c / torch.sqrt(c.square().mean(-1, keepdim=True) + eps) * w + b


def ref_attention(qkv, P, T, heads):
    D = 64 * heads
    q, k, v = (a.reshape(P, T, heads, 64).transpose(1, 2) for a in qkv.reshape(P, T, 3 * D).chunk(3, -1))
    s = q @ k.transpose(-1, -2) / 8
    s = s.masked_fill(~torch.ones(T, T, dtype=torch.bool).tril(), float("-inf"))
    e = torch.exp(s - s.amax(-1, keepdim=True))
    return ((e / e.sum(-1, keepdim=True)) @ v).transpose(1, 2).reshape(P * T, D)


def ref_quick_gelu(y):
    return y * (1 / (1 + torch.exp(-1.702 * y)))


# ------------------------------------------------------------------ the tower, restated with torch's own modules
class _Block(nn.Module):
    def __init__(self, width, heads):
        super().__init__()
        self.ln_1, self.ln_2 = nn.LayerNorm(width, eps=EPS), nn.LayerNorm(width, eps=EPS)
        self.attn = nn.MultiheadAttention(width, heads)
        self.c_fc, self.c_proj = nn.Linear(width, 4 * width), nn.Linear(4 * width, width)

    def forward(self, x, mask):
        h = self.ln_1(x)
        x = x + self.attn(h, h, h, need_weights=False, attn_mask=mask)[0]
        h = self.c_fc(self.ln_2(x))
        return x + self.c_proj(h * torch.sigmoid(1.702 * h))


def mha_tower(sd, tokens, dtype):
    """clip/model.py's encode_text over ``nn.MultiheadAttention`` (attn_mask = triu(-inf, 1)) and ``nn.LayerNorm`` in
    ``dtype``, sequence-first as CLIP runs it: float64 = the independent statement the twin is held to, float32 = the
    CPU arm of the bound."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    width = sd["token_embedding.weight"].shape[1]
    layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
    tok = torch.as_tensor(np.asarray(tokens)).long()
    P, T = tok.shape
    x = (sd["token_embedding.weight"][tok] + sd["positional_embedding"][:T]).permute(1, 0, 2)
    mask = torch.full((T, T), float("-inf"), dtype=dtype).triu(1)
    with torch.no_grad():
        for l in range(layers):
            blk = _Block(width, width // 64).to(dtype)
            p = f"transformer.resblocks.{l}."
            blk.load_state_dict({"ln_1.weight": sd[p + "ln_1.weight"], "ln_1.bias": sd[p + "ln_1.bias"],
                                 "ln_2.weight": sd[p + "ln_2.weight"], "ln_2.bias": sd[p + "ln_2.bias"],
                                 "attn.in_proj_weight": sd[p + "attn.in_proj_weight"], "attn.in_proj_bias": sd[p + "attn.in_proj_bias"],
                                 "attn.out_proj.weight": sd[p + "attn.out_proj.weight"], "attn.out_proj.bias": sd[p + "attn.out_proj.bias"],
                                 "c_fc.weight": sd[p + "mlp.c_fc.weight"], "c_fc.bias": sd[p + "mlp.c_fc.bias"],
                                 "c_proj.weight": sd[p + "mlp.c_proj.weight"], "c_proj.bias": sd[p + "mlp.c_proj.bias"]})
            x = blk(x, mask)
        x = x.permute(1, 0, 2)
        ln = nn.LayerNorm(width, eps=EPS).to(dtype)
        ln.load_state_dict({"weight": sd["ln_final.weight"], "bias": sd["ln_final.bias"]})
        x = ln(x)
        return x[torch.arange(P), tok.argmax(-1)] @ sd["text_projection"]


# ------------------------------------------------------------------ fixtures
def make_tokens(P, T, V, seed, eot=None):
    """Token ids in [1, V - 2], the EOT id V - 1 (the largest: the pooled position) at ``eot`` (drawn from [1, T - 1] when
    None), zeros after it -> int64 numpy [P, T]."""
    rng = np.random.default_rng(seed)
    tok = rng.integers(1, V - 1, size=(P, T))
    at = rng.integers(1, T, size=P) if eot is None else np.broadcast_to(np.asarray(eot), (P,))
    for p in range(P):
        tok[p, at[p]] = V - 1
        tok[p, at[p] + 1:] = 0
    return tok.astype(np.int64)


CASE_A = dict(width=128, layers=2, context=77, vocab=512, embed_dim=64)
CASE_B = dict(width=512, layers=12, context=77, vocab=1000, embed_dim=512)


@functools.lru_cache(maxsize=None)
def tower_case(name):
    """-> (state dict, tokens [P, 77], twin output float64, fp32 CPU arm) of case "A" (P = 5) or "B" (P = 2); computed
    once and shared: treat as read-only."""
    from lossyless_amd.clip_text import TextTransformer, synthetic_text_state_dict
    cfg, P = (CASE_A, 5) if name == "A" else (CASE_B, 2)
    sd = synthetic_text_state_dict(seed=3, **cfg)
    tok = make_tokens(P, cfg["context"], cfg["vocab"], seed=17)
    tok[0, :] = make_tokens(1, cfg["context"], cfg["vocab"], seed=18, eot=cfg["context"] - 1)[0]     # one full-length prompt
    twin = TextTransformer(sd, device="cpu")(tok)
    return sd, tok, twin, mha_tower(sd, tok, torch.float32)


# ------------------------------------------------------------------ zero-shot
def logit_bound(E, logit_scale, W):
    """Worst-case fp32 bound on a device logit against the float64 twin on the SAME fp32 rows and class embeddings:
    u = z / |z| carries at most ~(C / 64 + 8) roundings of relative size 2^-24 and has norm <= 1 + that, the dot product
    over E terms (any order) at most E more, the scale one: |error| <= logit_scale (E + 16) 2^-24 max_k |w_k| for
    C = E <= 512."""
    return float(logit_scale) * (E + 16) * 2.0 ** -24 * float(torch.as_tensor(W).double().norm(dim=1).max())


def direct_logits(z, W, logit_scale):
    """float64: logit_scale (z_i / |z_i|) . w_k, a zero row giving zeros."""
    z, W = torch.as_tensor(z).double(), torch.as_tensor(W).double()
    norm = z.norm(dim=1, keepdim=True)
    return logit_scale * (z / torch.where(norm > 0, norm, torch.ones_like(norm))) @ W.T


def planted_rows(W, n, noise, seed):
    """z_i = a_i w_{y_i} + noise, a_i log-uniform in (0.1, 10) -> (fp32 rows [n, E], labels int64 [n])."""
    g = torch.Generator().manual_seed(seed)
    W = torch.as_tensor(W).double()
    K, E = W.shape
    y = torch.arange(n) % K
    a = 10 ** (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1)
    z = a[:, None] * W[y] + noise * torch.randn(n, E, generator=g, dtype=torch.float64)
    return z.float(), y
