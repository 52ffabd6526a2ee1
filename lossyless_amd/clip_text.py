"""CLIP text tower on MI355X: ``TextTransformer`` stands in for ``model.encode_text`` (clip/model.py).

The reference featurises captions with ``encode_text`` (utils/data/images.py:1299-1323); CLIP's zero-shot classification
compares an image embedding with the text embeddings of class prompts (:class:`~lossyless_amd.probe.ZeroShotProbe`).  The
``ViT-B-32.pt`` file that :func:`~lossyless_amd.clip_vit.resolve_clip_weights` reads for the visual tower holds the text
transformer's weights next to it; :func:`load_clip_text_state_dict` keeps those.

The network, for integer tokens ``[P, T]`` (T <= context):

    x = token_embedding[tokens] + positional_embedding[:T]
    per block:  x = x + out_proj(causal_attention(in_proj(ln_1(x))));  x = x + c_proj(quick_gelu(c_fc(ln_2(x))))
    out = ln_final(x[p, argmax_t tokens[p]]) @ text_projection                  (the first maximum: the EOT token)

On the device everything is fp32: the Linear layers on ``lla_gemm_f32`` (``text_projection`` as a bias-free Linear on its
transpose), the rest in csrc/text_tower.hip; no torch op touches the activations except the gather of the pooled rows.
``device="cpu"`` runs the float64 twin -- plain torch, written out -- which is also the oracle of the GPU tests.

No tokenizer or vocabulary ships here: tokens come as integers, strings only through a ``tokenizer=`` callable (or the
``clip`` package's when it is installed).
"""

import numpy as np
import torch
import torch.nn as nn

from . import _lib

EPS = 1e-5
HEAD_DIM = 64
_BLOCK_KEYS = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
               "attn.out_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
               "mlp.c_proj.bias")
_GLOBAL_KEYS = ("token_embedding.weight", "positional_embedding", "ln_final.weight", "ln_final.bias", "text_projection",
                "logit_scale")


def synthetic_text_state_dict(seed=1, width=512, layers=12, context=77, vocab=49408, embed_dim=512):
    """Random-init text-tower weights in the OpenAI layout, with CLIP's initialisation scales (clip/model.py
    ``initialize_parameters``) and, unlike it, small non-zero biases and LayerNorm parameters off (1, 0) so that every
    term of the arithmetic is exercised.  FOR TESTS AND THE BENCH TOOL ONLY: embeddings of these weights mean nothing."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s, std: torch.randn(*s, generator=g) * std
    attn_std, proj_std, fc_std = width ** -0.5, (width ** -0.5) * ((2 * layers) ** -0.5), (2 * width) ** -0.5
    sd = {
        "token_embedding.weight": n(vocab, width, std=0.02),
        "positional_embedding": n(context, width, std=0.01),
        "ln_final.weight": 1 + n(width, std=0.1), "ln_final.bias": n(width, std=0.1),
        "text_projection": n(width, embed_dim, std=width ** -0.5),
        "logit_scale": torch.tensor(float(np.log(1 / 0.07))),
    }
    for l in range(layers):
        p = f"transformer.resblocks.{l}."
        sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = 1 + n(width, std=0.1), n(width, std=0.1)
        sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = n(3 * width, width, std=attn_std), n(3 * width, std=0.02)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = n(width, width, std=proj_std), n(width, std=0.02)
        sd[p + "ln_2.weight"], sd[p + "ln_2.bias"] = 1 + n(width, std=0.1), n(width, std=0.1)
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = n(4 * width, width, std=fc_std), n(4 * width, std=0.02)
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = n(width, 4 * width, std=proj_std), n(width, std=0.02)
    return sd


def _text_keys(sd):
    return {k: v for k, v in sd.items()
            if k in _GLOBAL_KEYS or (k.startswith("transformer.resblocks.") and k.split(".", 3)[-1] in _BLOCK_KEYS)}


def load_clip_text_state_dict(path):
    """Read OpenAI ``ViT-B-32.pt`` / ``RN50.pt`` (TorchScript archive) or a plain state-dict and return the text tower's
    tensors: ``token_embedding.weight``, ``positional_embedding``, ``transformer.resblocks.{i}.*``, ``ln_final.*``,
    ``text_projection`` and ``logit_scale`` (the keys under ``visual.`` are dropped)."""
    try:
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    except Exception:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if "state_dict" in sd:
            sd = sd["state_dict"]
    return _text_keys(sd)


def resolve_clip_text_weights(spec=None):
    """The text-side sibling of :func:`~lossyless_amd.clip_vit.resolve_clip_weights`, with its rules (one shared
    implementation): ``spec`` is a state-dict, a path to OpenAI ``ViT-B-32.pt`` / a state-dict file, the literal
    ``"synthetic"`` (seed-1 random weights: tests and the bench tool only), or None = the path in
    ``$LOSSYLESS_CLIP_WEIGHTS``, then CLIP's download cache, then ``clip.load``.  Returns (state_dict, description);
    raises ``ValueError`` when nothing is configured."""
    from .clip_vit import _resolve_weights
    return _resolve_weights(spec, load_clip_text_state_dict, lambda model: _text_keys(model.state_dict()),
                            lambda: synthetic_text_state_dict(1), "CLIP ViT-B/32 text-tower weights", "a state-dict")


def unit_rows(z):
    """Rows over their 2-norm, a row of zeros staying zeros: ``lla_unit_rows`` for an fp32 ``[N, C]`` tensor on the device
    (a fixed order of the sum: the same row gives the same bits in any batch), float64 torch on the CPU."""
    if z.device.type != "cuda":
        z = z.to(torch.float64)
        norm = z.square().sum(1, keepdim=True).sqrt()
        return torch.where(norm > 0, z / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.zeros_like(z))
    z = z if z.dtype == torch.float32 else z.float()
    z = z if z.stride(1) == 1 else z.contiguous()
    out = torch.empty(z.shape, dtype=torch.float32, device=z.device)
    n, C = int(z.shape[0]), int(z.shape[1])
    with torch.cuda.device(z.device):
        rc = _lib.lib().lla_unit_rows(_lib.ptr(z), int(z.stride(0)) if n > 1 else C, _lib.ptr(out), C, n, C,
                                      _lib.stream_ptr(z.device))
    _lib.check(rc, "lla_unit_rows")
    return out


def ln64(x, w, b):
    """LayerNorm over the last axis in the tensor's own dtype, written out (biased two-pass variance, eps 1e-5)."""
    c = x - x.mean(-1, keepdim=True)
    return c / torch.sqrt(c.square().mean(-1, keepdim=True) + EPS) * w + b


class TextTransformer(nn.Module):
    """``TextTransformer(state_dict, chunk=256, truncate=True)``: ``forward(tokens [P, T]) -> [P, embed_dim]``, unnormalised,
    as ``encode_text`` returns it -- fp32 on the device, float64 from the twin on the CPU (``device="cpu"``, the default
    until ``.to("cuda")``).

    Width, layers, heads (``width // 64``), context, vocabulary and embedding width are read from the tensors' shapes (the
    ViT-B/32 and RN50 text towers both load); the weights are used at the values the state dict holds, widened to fp32
    (fp16 widens exactly).  Prompts are processed ``chunk`` at a time out of one workspace.  ``truncate=True`` runs each
    chunk at its largest EOT position + 1 instead of T: attention is causal, so later positions cannot reach the pooled
    row, and no kernel's value depends on the number of rows -- the result is bit-identical to ``truncate=False``.
    """

    def __init__(self, state_dict, chunk=256, truncate=True, device="cpu", tokenizer=None):
        super().__init__()
        sd = {k: v.detach().to("cpu", torch.float32).contiguous() for k, v in _text_keys(state_dict).items()}
        missing = [k for k in _GLOBAL_KEYS[:-1] if k not in sd]
        if missing:
            raise ValueError(f"not a CLIP text state dict: {missing} missing")
        self.vocab, self.width = (int(s) for s in sd["token_embedding.weight"].shape)
        self.context = int(sd["positional_embedding"].shape[0])
        self.embed_dim = int(sd["text_projection"].shape[1])
        self.layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
        for l in range(self.layers):
            for k in _BLOCK_KEYS:
                if f"transformer.resblocks.{l}.{k}" not in sd:
                    raise ValueError(f"transformer.resblocks.{l}.{k} missing")
        if self.width % HEAD_DIM or not 64 <= self.width <= 1024 or self.embed_dim % 4 or not 1 <= self.context <= 77:
            raise ValueError(f"unsupported text tower: width {self.width}, context {self.context}, embed {self.embed_dim} "
                             "(width a multiple of 64 up to 1024, context up to 77, embedding width a multiple of 4)")
        self.heads = self.width // HEAD_DIM
        if int(chunk) < 1:
            raise ValueError("chunk must be at least 1")
        self.chunk, self.truncate, self.tokenizer = int(chunk), bool(truncate), tokenizer
        self.state = sd
        self.device = torch.device(device)
        self._dev = None       # (device, fp32 copies laid out for the kernels): a cache
        self._ws = None
        self._w64 = None

    @property
    def logit_scale(self):
        """``exp(logit_scale)`` of the state dict, or None when it holds none."""
        return float(self.state["logit_scale"].exp()) if "logit_scale" in self.state else None

    def __getstate__(self):
        """Pickling / ``copy.deepcopy`` / ``torch.save``: device copies, the workspace and the float64 copies are
        per-process caches, re-made on first use."""
        state = self.__dict__.copy()
        state["_dev"] = state["_ws"] = state["_w64"] = None
        return state

    def _apply(self, fn, recurse=True):
        """``.to(device)`` / ``.cuda()`` / ``.cpu()`` choose where ``forward`` runs; the weights go up on first use."""
        like = fn(torch.empty(0, device=self.device))
        self.device = like.device
        return super()._apply(fn, recurse)

    # ------------------------------------------------------------------ tokens
    def _tokens(self, tokens, tokenizer=None):
        """-> validated host int64 [P, T] numpy array."""
        if isinstance(tokens, str) or (isinstance(tokens, (list, tuple)) and tokens and isinstance(tokens[0], str)):
            tokenizer = tokenizer or self.tokenizer
            if tokenizer is None:
                try:
                    import clip  # noqa: PLC0415
                    tokenizer = clip.tokenize
                except ImportError:
                    raise ValueError("strings need a tokenizer: pass tokenizer=<callable returning [P, T] token ids> (no "
                                     "vocabulary ships with lossyless_amd and the `clip` package is not installed)") from None
            tokens = tokenizer([tokens] if isinstance(tokens, str) else list(tokens))
        t = tokens.detach().cpu().numpy() if isinstance(tokens, torch.Tensor) else np.asarray(tokens)
        if t.ndim != 2 or t.dtype.kind not in "iu":
            raise ValueError("tokens must be integers [P, T]")
        t = t.astype(np.int64)
        if not 1 <= t.shape[1] <= self.context:
            raise ValueError(f"T = {t.shape[1]} outside [1, {self.context}]")
        if t.size and (t.min() < 0 or t.max() >= self.vocab):
            raise ValueError(f"token ids must lie in [0, {self.vocab}): found {int(t.min())} .. {int(t.max())}")
        return t

    # ------------------------------------------------------------------ float64 twin
    def _twin(self, tok):
        if self._w64 is None:
            self._w64 = {k: v.to(torch.float64) for k, v in self.state.items()}
        W = self._w64
        P, T = tok.shape
        H = self.heads
        t = torch.from_numpy(tok)
        x = W["token_embedding.weight"][t] + W["positional_embedding"][:T]
        allowed = torch.ones(T, T, dtype=torch.bool).tril()
        for l in range(self.layers):
            p = f"transformer.resblocks.{l}."
            qkv = ln64(x, W[p + "ln_1.weight"], W[p + "ln_1.bias"]) @ W[p + "attn.in_proj_weight"].T + W[p + "attn.in_proj_bias"]
            q, k, v = (a.reshape(P, T, H, HEAD_DIM).transpose(1, 2) for a in qkv.chunk(3, -1))      # [P, H, T, 64]
            s = (q @ k.transpose(-1, -2) / 8).masked_fill(~allowed, float("-inf"))
            e = torch.exp(s - s.amax(-1, keepdim=True))
            o = ((e / e.sum(-1, keepdim=True)) @ v).transpose(1, 2).reshape(P, T, self.width)
            x = x + o @ W[p + "attn.out_proj.weight"].T + W[p + "attn.out_proj.bias"]
            m = ln64(x, W[p + "ln_2.weight"], W[p + "ln_2.bias"]) @ W[p + "mlp.c_fc.weight"].T + W[p + "mlp.c_fc.bias"]
            m = m * (1 / (1 + torch.exp(-1.702 * m)))
            x = x + m @ W[p + "mlp.c_proj.weight"].T + W[p + "mlp.c_proj.bias"]
        pooled = x[torch.arange(P), torch.from_numpy(tok.argmax(-1))]
        return ln64(pooled, W["ln_final.weight"], W["ln_final.bias"]) @ W["text_projection"]

    # ------------------------------------------------------------------ device
    def _weights(self, dev):
        if self._dev is None or self._dev[0] != dev:
            w = {k: v.to(dev) for k, v in self.state.items() if k not in ("text_projection", "logit_scale")}
            w["text_projection_t"] = self.state["text_projection"].t().contiguous().to(dev)
            self._dev = (dev, w)
        return self._dev[1]

    def _workspace(self, dev):
        # x, h, a [R][D] and one [R][4 D] shared by qkv and the MLP's hidden layer; pooled [chunk][D] twice
        need = self.chunk * (self.context * 7 + 2) * self.width
        if self._ws is None or self._ws.device != dev or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float32, device=dev)
        return self._ws

    def _chunk(self, L, W, ws, tok, eot, out, dev, st):
        """The tower over one chunk: host tokens [p, T] (already cut to the chunk's length), EOT positions [p]."""
        p, T = tok.shape
        D, R = self.width, p * T
        cap = self.chunk * self.context * D
        x, h, a = (ws[i * cap:i * cap + R * D] for i in range(3))
        big = ws[3 * cap:7 * cap]
        pool = ws[7 * cap:7 * cap + 2 * self.chunk * D]
        P_, ck = _lib.ptr, _lib.check
        tk = torch.from_numpy(np.ascontiguousarray(tok, dtype=np.int32)).to(dev)
        ck(L.lla_text_embed(P_(tk), p, T, P_(W["token_embedding.weight"]), self.vocab, P_(W["positional_embedding"]), D,
                            P_(x), st), "lla_text_embed")

        def ln(src, name, dst, rows):
            ck(L.lla_layernorm_rows(P_(src), D, P_(W[name + ".weight"]), P_(W[name + ".bias"]), P_(dst), D, rows, D, EPS, st),
               "lla_layernorm_rows")

        def linear(src, w, b, dst, rows, N, K):
            ck(L.lla_gemm_f32(P_(src), K, P_(w), K, None if b is None else P_(b), P_(dst), N, rows, N, K, 0, st), "lla_gemm_f32")

        for l in range(self.layers):
            q = f"transformer.resblocks.{l}."
            ln(x, q + "ln_1", h, R)
            linear(h, W[q + "attn.in_proj_weight"], W[q + "attn.in_proj_bias"], big, R, 3 * D, D)
            ck(L.lla_attention_causal(P_(big), P_(a), p, T, self.heads, st), "lla_attention_causal")
            linear(a, W[q + "attn.out_proj.weight"], W[q + "attn.out_proj.bias"], h, R, D, D)
            ck(L.lla_text_pointwise(P_(x), P_(h), R * D, 0, st), "lla_text_pointwise")
            ln(x, q + "ln_2", h, R)
            linear(h, W[q + "mlp.c_fc.weight"], W[q + "mlp.c_fc.bias"], big, R, 4 * D, D)
            ck(L.lla_text_pointwise(None, P_(big), R * 4 * D, 1, st), "lla_text_pointwise")
            linear(big, W[q + "mlp.c_proj.weight"], W[q + "mlp.c_proj.bias"], h, R, D, 4 * D)
            ck(L.lla_text_pointwise(P_(x), P_(h), R * D, 0, st), "lla_text_pointwise")
        rows = torch.from_numpy(np.arange(p, dtype=np.int64) * T + eot).to(dev)
        pooled, normed = pool[:p * D].view(p, D), pool[self.chunk * D:self.chunk * D + p * D].view(p, D)
        torch.index_select(x.view(R, D), 0, rows, out=pooled)
        ln(pooled, "ln_final", normed, p)
        linear(normed, W["text_projection_t"], None, out, p, self.embed_dim, D)

    def forward(self, tokens, tokenizer=None):
        tok = self._tokens(tokens, tokenizer)
        P = tok.shape[0]
        dev = self.device
        if dev.type != "cuda":
            return self._twin(tok) if P else torch.zeros((0, self.embed_dim), dtype=torch.float64)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((P, self.embed_dim), dtype=torch.float32, device=dev)
        eot = tok.argmax(-1)            # numpy: the first maximum, as torch.argmax gives on these rows
        L = _lib.lib()
        with torch.cuda.device(dev):
            W, ws, st = self._weights(dev), self._workspace(dev), _lib.stream_ptr(dev)
            for c0 in range(0, P, self.chunk):
                c1 = min(c0 + self.chunk, P)
                T = int(eot[c0:c1].max()) + 1 if self.truncate else tok.shape[1]
                self._chunk(L, W, ws, tok[c0:c1, :T], eot[c0:c1], out[c0:c1], dev, st)
        return out

    def encode_classes(self, tokens, tokenizer=None):
        """CLIP's prompt ensembling: tokens ``[K, n_templates, T]`` -> class embeddings ``[K, embed_dim]``: every prompt's
        embedding over its 2-norm, the mean over a class's templates (added in template order), over its 2-norm again."""
        t = tokens.detach().cpu().numpy() if isinstance(tokens, torch.Tensor) else np.asarray(tokens)
        if t.ndim != 3:
            raise ValueError("tokens must be [K, n_templates, T]")
        K, n, T = t.shape
        e = unit_rows(self.forward(t.reshape(K * n, T), tokenizer)).view(K, n, self.embed_dim)
        mean = e[:, 0]
        for j in range(1, n):
            mean = mean + e[:, j]
        return unit_rows(mean / n)
