"""csrc/text_tower.hip on the device: each kernel against its float64 reference under the bound rule of
text_tower_util (4 x the error of torch's fp32 CPU arithmetic), the structural properties that must hold to the bit, and the
whole tower against the float64 twin."""
import numpy as np
import pytest
import torch

from text_tower_util import (CASE_A, held, make_tokens, ref_attention, ref_embed, ref_layernorm, ref_quick_gelu,
                             tower_case)

pytestmark = pytest.mark.gpu


def _call(name, *args):
    from lossyless_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.stream_ptr()), name)


def _p(t):
    from lossyless_amd import _lib
    return _lib.ptr(t)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def test_embed_is_the_fp32_sum():
    V, D, P, T = 97, 128, 3, 77
    emb, pos = _randn(V, D, seed=1).float(), _randn(T, D, seed=2).float()
    tok = torch.from_numpy(make_tokens(P, T, V, seed=3)).to(torch.int32)
    x = torch.full((P * T, D), float("nan"), device="cuda")
    tok_d, emb_d, pos_d = tok.cuda(), emb.cuda(), pos.cuda()       # (named: a temporary would be freed before the launch)
    _call("lla_text_embed", _p(tok_d), P, T, _p(emb_d), V, _p(pos_d), D, _p(x))
    assert torch.equal(x.cpu(), ref_embed(tok, emb, pos))
    wild = tok.clone()
    wild[0, 0], wild[1, 1] = -5, V + 1000            # the kernel clamps: rows 0 and V - 1, nothing outside the table
    wild_d = wild.cuda()
    _call("lla_text_embed", _p(wild_d), P, T, _p(emb_d), V, _p(pos_d), D, _p(x))
    assert torch.equal(x.cpu(), ref_embed(wild.clamp(0, V - 1), emb, pos))


@pytest.mark.parametrize("D", [64, 512, 1024])
@pytest.mark.parametrize("rows", [5, 231])
def test_layernorm_rows(D, rows):
    stride = D + 12
    x = _randn(rows, stride, seed=D + rows).float()
    x[rows // 2] += 300.0                              # a row with a large common offset
    w, b = (1 + _randn(D, seed=5, scale=0.2)).float(), _randn(D, seed=6, scale=0.2).float()
    y = torch.full((rows, stride), -7.0, device="cuda")
    x_d, w_d, b_d = x.cuda(), w.cuda(), b.cuda()
    _call("lla_layernorm_rows", _p(x_d), stride, _p(w_d), _p(b_d), _p(y), stride, rows, D, 1e-5)
    assert (y[:, D:] == -7.0).all()
    ref = ref_layernorm(x[:, :D].double(), w.double(), b.double())
    held(f"layernorm D={D} rows={rows}", y[:, :D], ref_layernorm(x[:, :D], w, b), ref)
    one = torch.empty(D, device="cuda")              # a row alone gives the bits it has in the batch
    last = x[rows - 1].cuda()
    _call("lla_layernorm_rows", _p(last), stride, _p(w_d), _p(b_d), _p(one), D, 1, D, 1e-5)
    assert torch.equal(one, y[rows - 1, :D])


@pytest.mark.parametrize("D", [64, 1024])
def test_layernorm_of_a_row_fp32_cannot_resolve(D):
    """1000 + 1e-3 noise: the row's spread is ~16 ulps of its values, so both fp32 arms are far from float64 and the row
    is held on its OWN arm pair -- in the tensor of test_layernorm_rows it would set the bound for every other row."""
    x = (_randn(1, D, seed=D) * 1e-3 + 1000.0).float()
    w, b = (1 + _randn(D, seed=5, scale=0.2)).float(), _randn(D, seed=6, scale=0.2).float()
    y = torch.full((1, D), float("nan"), device="cuda")
    x_d, w_d, b_d = x.cuda(), w.cuda(), b.cuda()
    _call("lla_layernorm_rows", _p(x_d), D, _p(w_d), _p(b_d), _p(y), D, 1, D, 1e-5)
    assert bool(torch.isfinite(y).all())
    held(f"layernorm D={D}, 1000 + 1e-3 noise", y, ref_layernorm(x, w, b), ref_layernorm(x.double(), w.double(), b.double()))


def _attention(qkv, P, T, heads):
    o = torch.full((P * T, 64 * heads), float("nan"), device="cuda")
    qkv_d = qkv.cuda().contiguous()
    _call("lla_attention_causal", _p(qkv_d), _p(o), P, T, heads)
    return o


@pytest.mark.parametrize("P,T,heads,gain", [(3, 77, 2, 1.0), (5, 9, 1, 1.0), (1, 1, 8, 1.0), (3, 77, 2, 2.7)])
def test_attention_causal(P, T, heads, gain):
    D = 64 * heads
    qkv = _randn(P * T, 3 * D, seed=T + heads).float()
    qkv[:, :2 * D] *= gain                            # gain 2.7: scores q . k / 8 with a standard deviation of ~7, tails at +-60 ...
    if gain != 1.0:
        qkv[5, :64] = qkv[3, D:D + 64]                # ... and two planted at ~ +60 and -60 (queries 5 and 6, key 3, head 0)
        qkv[6, :64] = -qkv[3, D:D + 64]
        assert 40 < float(qkv[5, :64] @ qkv[3, D:D + 64]) / 8 < 90
    o = _attention(qkv, P, T, heads)
    ref = ref_attention(qkv.double(), P, T, heads)
    held(f"attention P={P} T={T} heads={heads} gain={gain}", o, ref_attention(qkv, P, T, heads), ref)
    v = qkv[:, 2 * D:].reshape(P, T, D)
    assert torch.equal(o.cpu().reshape(P, T, D)[:, 0], v[:, 0])          # row 0 attends to itself alone: v_0 exactly
    if T > 1:                                                             # the future cannot reach a row's bits
        i = T // 2
        other = qkv.clone().reshape(P, T, 3 * D)
        other[:, i + 1:, D:] = _randn(P, T - i - 1, 2 * D, seed=9, scale=5.0).float()
        other[:, T - 1, D:] = float("inf")
        o2 = _attention(other.reshape(P * T, 3 * D), P, T, heads)
        assert torch.equal(o2.reshape(P, T, D)[:, :i + 1], o.reshape(P, T, D)[:, :i + 1])
        alone = _attention(qkv.reshape(P, T, 3 * D)[P - 1], 1, T, heads)   # a prompt alone: the bits it has in the batch
        assert torch.equal(alone, o.reshape(P, T, D)[P - 1])


@pytest.mark.parametrize("n", [1027, 256 * 4 * 3 + 2, 3])
def test_pointwise(n):
    x, y = _randn(n, seed=n).float(), _randn(n, seed=n + 1, scale=4.0).float()
    y[:3] = torch.tensor([-60.0, 60.0, 0.0])[:min(n, 3)]
    xd, yd = x.cuda(), y.cuda()
    _call("lla_text_pointwise", _p(xd), _p(yd), n, 0)
    assert torch.equal(xd.cpu(), x + y) and torch.equal(yd.cpu(), y)
    _call("lla_text_pointwise", None, _p(yd), n, 1)
    held(f"quick_gelu n={n}", yd, ref_quick_gelu(y), ref_quick_gelu(y.double()))
    assert float(yd[0]) == 0.0 or abs(float(yd[0])) < 1e-30


def test_unit_rows():
    from lossyless_amd.clip_text import unit_rows
    z = _randn(70, 200, seed=4).float() * torch.logspace(-3, 3, 70)[:, None]
    z[7] = 0
    u = unit_rows(z.cuda())
    assert torch.equal(u[7], torch.zeros(200, device="cuda"))
    held("unit rows", u, z / z.norm(dim=1, keepdim=True).clamp_min(1e-30), unit_rows(z))
    assert torch.equal(unit_rows(z[40:41].cuda())[0], u[40])
    assert torch.equal(unit_rows(z.cuda()[:, :64])[3], unit_rows(z[:, :64].contiguous().cuda())[3])     # a pitch


# ------------------------------------------------------------------ the tower
def _device_tower(name, **kw):
    from lossyless_amd.clip_text import TextTransformer
    return TextTransformer(tower_case(name)[0], **kw).to("cuda")


@pytest.mark.parametrize("name", ["A", "B"])
def test_tower_against_the_twin(name):
    sd, tok, twin, arm = tower_case(name)
    out = _device_tower(name, chunk=2)(tok)           # case A: P = 5 in chunks of 2, a ragged last chunk
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == tuple(twin.shape)
    held(f"tower case {name}", out, arm, twin)


def test_tower_bits_do_not_depend_on_the_batch():
    sd, tok, _, _ = tower_case("A")
    P = tok.shape[0]
    base = _device_tower("A", chunk=P)(tok)
    assert torch.equal(_device_tower("A", chunk=1)(tok), base)
    assert torch.equal(_device_tower("A", chunk=P, truncate=False)(tok), base)
    assert torch.equal(_device_tower("A", chunk=2, truncate=False)(tok), base)
    t = _device_tower("A", chunk=P)
    assert torch.equal(t(tok[3:4])[0], base[3])                              # a prompt alone
    assert torch.equal(t(tok[[3, 0, 3, 1]]), base[[3, 0, 3, 1]])             # ... and elsewhere in a batch
    after = tok.copy()
    rng = np.random.default_rng(8)
    for p in range(1, P):
        at = int(tok[p].argmax())
        after[p, at + 1:] = rng.integers(0, CASE_A["vocab"] - 1, size=tok.shape[1] - at - 1)
    assert (after != tok).any() and torch.equal(t(after), base)              # arbitrary tokens after the EOT
    assert torch.equal(t(tok), base)                                         # two runs
    assert torch.equal(t(torch.from_numpy(tok).cuda()), base)


def test_encode_classes_and_the_hub_entry():
    import hubconf
    sd = tower_case("A")[0]
    tok = make_tokens(21, 77, CASE_A["vocab"], seed=6).reshape(7, 3, 77)
    dev = hubconf.clip_text_encoder(sd, device="cuda", chunk=8)
    got = dev.encode_classes(tok)
    want = hubconf.clip_text_encoder(sd, device="cpu").encode_classes(tok)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (7, CASE_A["embed_dim"])
    # unit vectors: the tower's bound for case A (measured in test_tower_against_the_twin's arm) does not carry over; held
    # to 4 x the fp32 CPU arm of the same formula
    from text_tower_util import mha_tower
    e = mha_tower(sd, tok.reshape(21, 77), torch.float32)
    e = (e / e.norm(dim=1, keepdim=True)).reshape(7, 3, -1).mean(1)
    held("encode_classes", got, e / e.norm(dim=1, keepdim=True), want)
    assert float((got.double().norm(dim=1) - 1).abs().max()) < 1e-6
