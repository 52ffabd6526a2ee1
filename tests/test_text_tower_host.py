"""The text tower's float64 twin and ZeroShotProbe on the CPU (no GPU): the twin against an independent statement of the
network, pooling, causality, prompt ensembling, the probe against a direct computation, argument checks, the ABI."""
import pickle

import numpy as np
import pytest
import torch

from text_tower_util import CASE_A, direct_logits, make_tokens, mha_tower, planted_rows, tower_case


def _tower(**kw):
    from lossyless_amd.clip_text import TextTransformer
    return TextTransformer(tower_case("A")[0], device="cpu", **kw)


def test_twin_equals_the_multihead_attention_statement():
    sd, tok, twin, _ = tower_case("A")
    want = mha_tower(sd, tok, torch.float64)
    assert twin.dtype == torch.float64 and tuple(twin.shape) == (5, CASE_A["embed_dim"])
    err = float((twin - want).abs().max() / want.abs().max())
    print(f"twin against nn.MultiheadAttention / nn.LayerNorm in float64: {err:.3g}")
    assert err <= 1e-10


def test_shapes_are_read_from_the_tensors():
    from lossyless_amd.clip_text import TextTransformer, synthetic_text_state_dict
    t = TextTransformer(synthetic_text_state_dict(seed=2, width=192, layers=1, context=20, vocab=50, embed_dim=1024))
    assert (t.width, t.layers, t.heads, t.context, t.vocab, t.embed_dim) == (192, 1, 3, 20, 50, 1024)
    assert tuple(t(make_tokens(2, 20, 50, 1)).shape) == (2, 1024)
    assert abs(t.logit_scale - 1 / 0.07) < 1e-4


def test_pooling_takes_the_first_maximum():
    sd, tok, _, _ = tower_case("A")
    t = _tower()
    tok = tok[:2].copy()
    tok[0, 5], tok[0, 6:] = CASE_A["vocab"] - 1, 0
    twice = tok.copy()
    twice[0, 30] = CASE_A["vocab"] - 1              # a second maximum later in the row: position 5 stays the pooled one
    cut = tok.copy()
    cut[0, 6:] = 0
    assert torch.equal(t(twice)[0], t(cut)[0])


def test_tokens_after_the_eot_do_not_matter():
    sd, tok, twin, _ = tower_case("A")
    other = tok.copy()
    rng = np.random.default_rng(5)
    for p in range(tok.shape[0]):
        at = int(tok[p].argmax())
        other[p, at + 1:] = rng.integers(0, CASE_A["vocab"] - 1, size=tok.shape[1] - at - 1)
    assert (other != tok).any()
    assert torch.equal(_tower()(other), twin)
    short = _tower()(tok[1:, :int(tok[1:].argmax(-1).max()) + 1])       # ... nor do the positions themselves
    assert float((short - twin[1:]).abs().max()) <= 1e-12 * float(twin.abs().max())


def test_encode_classes_is_the_ensembling_formula():
    t = _tower()
    tok = make_tokens(6, 77, CASE_A["vocab"], seed=4).reshape(2, 3, 77)
    e = t(tok.reshape(6, 77))
    e = (e / e.norm(dim=1, keepdim=True)).reshape(2, 3, -1).mean(1)
    want = e / e.norm(dim=1, keepdim=True)
    got = t.encode_classes(tok)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-14


def test_zero_shot_probe_on_cpu_data():
    from lossyless_amd import ZeroShotProbe
    t = _tower()
    tok = make_tokens(21, 77, CASE_A["vocab"], seed=6).reshape(7, 3, 77)
    probe = ZeroShotProbe.from_tokens(t, tok)
    assert abs(probe.logit_scale - 1 / 0.07) < 1e-4 and probe.coef_.dtype == torch.float32
    assert tuple(probe.coef_.shape) == (7, 64) and np.array_equal(probe.classes_, np.arange(7))
    assert not hasattr(probe, "fit")
    z, y = planted_rows(probe.coef_, 200, 0.05, seed=1)
    z[3] = 0
    want = direct_logits(z, probe.coef_, probe.logit_scale)
    got = probe.decision_function(z)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-10
    assert torch.equal(got[3], torch.zeros(7, dtype=torch.float64))
    scaled = probe.decision_function(z * torch.linspace(0.01, 50, 200)[:, None])
    assert float((scaled - want).abs().max()) <= 1e-4                     # (fp32 rows: the product rounds)
    assert torch.equal(probe.predict(z), want.argmax(1))
    assert float((probe.predict_proba(z) - torch.softmax(want, 1)).abs().max()) <= 1e-12
    own = want[torch.arange(200), y][:, None]                   # ties go to the lower index, as in predict (the zero row)
    rank = ((want > own) | ((want == own) & (torch.arange(7)[None, :] < y[:, None]))).sum(1)
    assert rank[3] == 3
    for k in (1, 2, 7):
        assert probe.top_k_score(z, k, y) == float((rank < k).double().mean())
    assert probe.score(z, y) == probe.top_k_score(z, 1, y) and probe.top_k_score(z, 7, y) == 1.0
    assert probe.score(z.numpy(), y.numpy()) == probe.score(z, y)
    named = ZeroShotProbe(probe.coef_, logit_scale=50, classes=[10, 11, 12, 13, 14, 15, 16])
    assert named.logit_scale == 50 and torch.equal(named.predict(z), want.argmax(1) + 10)
    assert named.score(z, y + 10) == probe.score(z, y)
    no_scale = {k: v for k, v in tower_case("A")[0].items() if k != "logit_scale"}
    from lossyless_amd.clip_text import TextTransformer
    assert ZeroShotProbe.from_tokens(TextTransformer(no_scale), tok).logit_scale == 100.0
    with pytest.raises(ValueError):
        probe.top_k_score(z, 8, y)
    with pytest.raises(ValueError):
        probe.decision_function(torch.zeros(3, 32))


def test_argument_checks():
    t = _tower()
    with pytest.raises(ValueError, match="token ids"):
        t(np.full((1, 77), CASE_A["vocab"]))
    with pytest.raises(ValueError, match="token ids"):
        t(np.full((1, 77), -1))
    with pytest.raises(ValueError):
        t(np.zeros((1, 78), dtype=np.int64))
    with pytest.raises(ValueError):
        t(np.zeros((1, 77)))
    try:
        import clip  # noqa: F401
    except ImportError:
        with pytest.raises(ValueError, match="tokenizer"):
            t(["a photo of a dog"])
    seen = []

    def tokenizer(texts):
        seen.append(list(texts))
        return make_tokens(len(texts), 77, CASE_A["vocab"], seed=9)

    assert tuple(t(["a", "b"], tokenizer=tokenizer).shape) == (2, 64) and seen == [["a", "b"]]
    assert tuple(_tower(tokenizer=tokenizer)("a").shape) == (1, 64)


def test_state_dict_loading_and_pickling(tmp_path, monkeypatch):
    import hubconf
    from lossyless_amd.clip_text import load_clip_text_state_dict, resolve_clip_text_weights
    sd, tok, twin, _ = tower_case("A")
    both = dict(sd)
    both["visual.proj"] = torch.zeros(3, 3)
    both["input_resolution"] = torch.tensor(224)
    torch.save({k: v.half() if v.dim() else v for k, v in both.items()}, tmp_path / "clip.pt")
    got = load_clip_text_state_dict(tmp_path / "clip.pt")
    assert set(got) == set(sd) and got["text_projection"].dtype == torch.float16
    assert resolve_clip_text_weights(sd)[0] is sd
    monkeypatch.setenv("LOSSYLESS_CLIP_WEIGHTS", str(tmp_path / "clip.pt"))
    enc = hubconf.clip_text_encoder(device="cpu")
    half = {k: v.half().float() if v.dim() else v for k, v in sd.items()}
    from lossyless_amd.clip_text import TextTransformer
    assert torch.equal(enc(tok), TextTransformer(half)(tok))            # fp16 weights are used at their own values
    again = pickle.loads(pickle.dumps(enc))
    assert again._w64 is None and again._dev is None and torch.equal(again(tok), enc(tok))
    assert resolve_clip_text_weights("synthetic")[1] == "synthetic-seed1"


def test_symbols_and_abi():
    from lossyless_amd import _lib
    L = _lib.lib()
    for name in ("lla_text_embed", "lla_layernorm_rows", "lla_attention_causal", "lla_text_pointwise", "lla_unit_rows"):
        assert name in _lib.EXPORTS and getattr(L, name) is not None
    assert _lib.ABI_VERSION == 4 and L.lla_abi_version() == 4


def test_refusals_come_before_any_device_call():
    """Invalid shapes are LLA_EINVAL and P == 0 is LLA_OK with NULL pointers: decided on the host (no GPU here)."""
    from lossyless_amd import _lib
    L, E = _lib.lib(), _lib.LLA_EINVAL
    assert L.lla_text_embed(None, 0, 77, None, 10, None, 64, None, None) == 0
    assert L.lla_text_embed(None, 1, 77, None, 10, None, 66, None, None) == E
    assert L.lla_text_embed(None, 1, 77, None, 10, None, 64, None, None) == E
    assert L.lla_layernorm_rows(None, 64, None, None, None, 64, 0, 64, 1e-5, None) == 0
    for D in (32, 96, 1088):
        assert L.lla_layernorm_rows(None, 2048, None, None, None, 2048, 0, D, 1e-5, None) == E
    assert L.lla_layernorm_rows(None, 64, None, None, None, 128, 0, 128, 1e-5, None) == E       # pitch < D
    assert L.lla_attention_causal(None, None, 0, 77, 8, None) == 0
    for T, heads in ((0, 8), (78, 8), (77, 0)):
        assert L.lla_attention_causal(None, None, 0, T, heads, None) == E
    assert L.lla_attention_causal(None, None, 1, 77, 8, None) == E
    assert L.lla_text_pointwise(None, None, 0, 1, None) == 0
    assert L.lla_text_pointwise(None, None, 0, 2, None) == E and L.lla_text_pointwise(None, None, -1, 0, None) == E
    assert L.lla_unit_rows(None, 64, None, 64, 0, 64, None) == 0 and L.lla_unit_rows(None, 8, None, 64, 0, 64, None) == E
