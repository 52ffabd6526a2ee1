"""GPU parity, kernel by kernel, for the towers' kernels that are not GEMMs -- attention50, ln_pre_ln1, layernorm768 (both
walks), and the RN50 tower's avgpool2, attnpool_tokens and attnpool_attend -- through entry points that make the launches the
towers make.  Every kernel against the float64 reference and the derived elementwise bound of tower_kernel_util.py (which
test_tower_kernel_refs_host.py keeps honest on the CPU), at the smallest shapes at which the code can still go wrong.

Every output sits between guard blocks and is pre-filled with an fp16 NaN pattern (the fp32 x of ln_pre_ln1: NaN on the class
rows the kernel has to build); after the call no poison is left and the guards are intact.  Every test prints its largest
error / bound ratio before it asserts (pytest -s shows them)."""
import pytest
import torch

import tower_kernel_util as tk
from lossyless_amd import _lib

pytestmark = pytest.mark.gpu

_SENTINEL = -777.0
_X_SENTINEL = -12345.0


def _out(n, fill_poison=True):
    """A guarded fp16 output of n elements, poisoned: (whole buffer, the n elements)."""
    buf, o = tk.guarded(n, torch.float16, _SENTINEL)
    if fill_poison:
        o.view(torch.int16).fill_(tk.H_POISON)
    return buf, o


def _written(buf, o, what):
    torch.cuda.synchronize()
    left = o.view(torch.int16) == tk.H_POISON
    assert not bool(left.any()), f"{what}: {int(left.sum())} elements not written, first {left.reshape(-1).nonzero()[:8, 0].tolist()}"
    assert tk.guards_intact(buf, _SENTINEL), f"{what}: guard overwritten"


def _untouched(buf, o):
    torch.cuda.synchronize()
    return bool((o.view(torch.int16) == tk.H_POISON).all()) and tk.guards_intact(buf, _SENTINEL)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    d = _bits(a) != _bits(b)
    return not bool(d.any()), f"{int(d.sum())} elements differ, first {d.reshape(-1).nonzero()[:8, 0].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# attention50
# ---------------------------------------------------------------------------------------------------------------------
def _attention(qkv, B, rev=None):
    """-> o fp16 [B * 50][768] of lla_attention50_ex (rev None: lla_attention50), poison and guards checked."""
    buf, o = _out(B * tk.TOKENS * tk.WIDTH)
    L = _lib.lib()
    if rev is None:
        rc = L.lla_attention50(_lib.ptr(qkv), _lib.ptr(o), B, _lib.stream_ptr())
    else:
        rc = L.lla_attention50_ex(_lib.ptr(qkv), _lib.ptr(o), B, rev, _lib.stream_ptr())
    _lib.check(rc, "lla_attention50_ex")
    _written(buf, o, "attention50")
    return o.view(B * tk.TOKENS, tk.WIDTH)


_ATTENTION = {}


def _attention_case(kind, B, seed=0):
    """(qkv, float64 reference, bound, the kernel's output) of a case, computed once and left unchanged."""
    key = (kind, B, seed)
    if key not in _ATTENTION:
        qkv = tk.attention_case(kind, B, seed).cuda()
        ref, bound = tk.attention_bound(qkv, B)
        _ATTENTION[key] = (qkv, ref, bound, _attention(qkv, B, 0))
    return _ATTENTION[key]


@pytest.mark.parametrize("B", [1, 3, 67])
@pytest.mark.parametrize("kind", tk.ATTENTION_KINDS)
def test_attention50_against_fp64(kind, B):
    qkv, ref, bound, o = _attention_case(kind, B)
    w, r, c = tk.worst((o.double() - ref).abs(), bound, f"attention50 {kind} B {B}")
    assert w <= 1.0, (w, r, c)
    q, k, v = tk.split_heads(qkv, B)
    if kind == "one_hot":       # every query returns the V row of its key, to the rounding of the output
        perm = tk.one_hot_permutations(B, 0).cuda()
        want = torch.gather(v, 2, perm[..., None].expand(-1, -1, -1, tk.HEAD_DIM))
        assert torch.equal(o, tk.merge_heads(want, B)), "a query did not return the V row of its key"
    if kind == "uniform":       # every row of an image is the same mean of its 50 V rows
        rows = o.view(B, tk.TOKENS, tk.WIDTH)
        ok, msg = _same_bits(rows, rows[:, :1].expand(-1, tk.TOKENS, -1).contiguous())
        assert ok, msg


def test_attention50_rounds_p_to_nearest():
    """The mean signed error / bound over four draws of the largest random case: within four standard deviations of zero
    (truncating P instead leaves -0.16: test_p_truncated_instead_of_rounded_would_show)."""
    B, bias = 67, []
    for seed in tk.BIAS_SEEDS:
        _, ref, bound, o = _attention_case("random", B, seed)
        bias.append(tk.signed_bias(o, ref, bound))
    n = len(bias) * B * tk.TOKENS * tk.WIDTH
    bias = sum(bias) / len(bias)
    print(f"attention50 signed bias {bias:+.5f} (limit {tk.signed_bias_limit(n):.5f})")
    assert abs(bias) <= tk.signed_bias_limit(n)


@pytest.mark.parametrize("B", [3, 67])
def test_attention50_walks_and_entry_points_give_the_same_bits(B):
    for kind in ("random", "large"):
        qkv, _, _, o = _attention_case(kind, B)
        for rev in (1, None):
            ok, msg = _same_bits(o, _attention(qkv, B, rev))
            assert ok, (kind, rev, msg)


def test_attention50_images_are_independent():
    qkv1 = tk.attention_case("random", 1, seed=5).cuda()
    alone = _attention(qkv1, 1, 0)
    qkv = torch.empty(3 * tk.TOKENS, 3 * tk.WIDTH, dtype=torch.float16, device="cuda")
    qkv[:tk.TOKENS] = float("nan")
    qkv[tk.TOKENS:2 * tk.TOKENS] = qkv1
    sign = torch.where(torch.rand(tk.TOKENS, 3 * tk.WIDTH, generator=torch.Generator().manual_seed(6)) < 0.5, -1.0, 1.0)
    qkv[2 * tk.TOKENS:] = (65504.0 * sign).half().cuda()
    for rev in (0, 1):
        o = _attention(qkv, 3, rev)
        ok, msg = _same_bits(o[tk.TOKENS:2 * tk.TOKENS], alone)
        assert ok, (rev, msg)
        assert bool(torch.isfinite(o[tk.TOKENS:2 * tk.TOKENS]).all()) and bool(torch.isnan(o[:tk.TOKENS]).all())


def test_attention50_refusals():
    L, st = _lib.lib(), _lib.stream_ptr()
    qkv = tk.attention_case("random", 1).cuda()
    buf, o = _out(tk.TOKENS * tk.WIDTH)
    assert L.lla_attention50_ex(_lib.ptr(qkv), _lib.ptr(o), -1, 0, st) == -1
    assert L.lla_attention50_ex(None, _lib.ptr(o), 1, 0, st) == -1 and L.lla_attention50_ex(_lib.ptr(qkv), None, 1, 0, st) == -1
    assert L.lla_attention50_ex(_lib.ptr(qkv), _lib.ptr(o), 1, 2, st) == -1 and L.lla_attention50_ex(_lib.ptr(qkv), _lib.ptr(o), 1, -1, st) == -1
    assert L.lla_attention50_ex(_lib.ptr(qkv), _lib.ptr(o), 0, 0, st) == 0 and L.lla_attention50_ex(None, None, 0, 1, st) == 0
    assert _untouched(buf, o)


# ---------------------------------------------------------------------------------------------------------------------
# ln_pre_ln1
# ---------------------------------------------------------------------------------------------------------------------
def _ln_pre_ln1(c, rows):
    """-> (x fp32 [rows][768], h fp16 [rows][768]) of one call on fresh guarded buffers."""
    xbuf, x = tk.guarded(rows * tk.WIDTH, torch.float32, _X_SENTINEL)
    hbuf, h = _out(rows * tk.WIDTH)
    x, h = x.view(rows, tk.WIDTH), h.view(rows, tk.WIDTH)
    x.copy_(c["x"])
    rc = _lib.lib().lla_ln_pre_ln1_768(_lib.ptr(x), _lib.ptr(c["cls"]), _lib.ptr(c["pos"]), _lib.ptr(c["wpre"]), _lib.ptr(c["bpre"]),
                                       _lib.ptr(c["w1"]), _lib.ptr(c["b1"]), _lib.ptr(h), rows, _lib.stream_ptr())
    _lib.check(rc, "lla_ln_pre_ln1_768")
    _written(hbuf, h, "ln_pre_ln1 h")
    assert tk.guards_intact(xbuf, _X_SENTINEL), "ln_pre_ln1 x: guard overwritten"
    assert bool(torch.isfinite(x).all()), "ln_pre_ln1 x: a class row was not built (or was read)"
    return x, h


@pytest.mark.parametrize("rows", tk.LN_ROWS)
def test_ln_pre_ln1_against_fp64(rows):
    c = {k: v.cuda() for k, v in tk.ln_pre_case(rows).items()}
    x, h = _ln_pre_ln1(c, rows)
    # x against the two-pass float64 ln_pre of the assembled rows
    ref_x, bound_x = tk.ln_pre_x_bound(c)
    wx, r, col = tk.worst((x.double() - ref_x).abs(), bound_x, f"ln_pre_ln1 rows {rows} x")
    # its class rows: the same bits in every image
    cls_rows = x[0::tk.TOKENS]
    same_cls, msg_cls = _same_bits(cls_rows, cls_rows[:1].expand_as(cls_rows).contiguous())
    # h: the bits of the LayerNorm kernel on the x this call wrote
    h2 = torch.empty_like(h)
    _lib.check(_lib.lib().lla_layernorm768(_lib.ptr(x), tk.WIDTH, _lib.ptr(c["w1"]), _lib.ptr(c["b1"]), _lib.ptr(h2), rows,
                                           _lib.stream_ptr()), "lla_layernorm768")
    torch.cuda.synchronize()
    same_h, msg_h = _same_bits(h, h2)
    # ... that x's ln_1, and the ln_1 of the float64 ln_pre
    own = tk.layernorm_f64(x, c["w1"], c["b1"])
    w1, r1, c1 = tk.worst((h.double() - own).abs(), tk.layernorm_f16_bound(own), f"ln_pre_ln1 rows {rows} h against ln_1 of its x")
    ref_h = tk.layernorm_f64(ref_x, c["w1"], c["b1"])
    w2, r2, c2 = tk.worst((h.double() - ref_h).abs(), tk.layernorm_f16_bound(ref_h), f"ln_pre_ln1 rows {rows} h against ln_1(ln_pre)")
    assert wx <= 1.0, (wx, r, col)
    assert same_cls, msg_cls
    assert same_h, msg_h
    assert w1 <= 1.0 and w2 <= 1.0, (w1, r1, c1, w2, r2, c2)
    # again: the same bits
    x3, h3 = _ln_pre_ln1(c, rows)
    ok, msg = _same_bits(x, x3)
    assert ok, msg
    ok, msg = _same_bits(h, h3)
    assert ok, msg


def test_ln_pre_ln1_refusals():
    L, st = _lib.lib(), _lib.stream_ptr()
    c = {k: v.cuda() for k, v in tk.ln_pre_case(50).items()}
    x0 = tk.ln_pre_input(c)
    x = x0.clone()
    buf, h = _out(50 * tk.WIDTH)
    names = ("x", "cls", "pos", "wpre", "bpre", "w1", "b1", "h")
    args = dict(c, x=x, h=h)
    call = lambda rows, null=None: L.lla_ln_pre_ln1_768(*[None if n == null else _lib.ptr(args[n]) for n in names], rows, st)
    assert call(-1) == -1 and call(-50) == -1
    for n in names:
        assert call(50, null=n) == -1, n
    assert call(0) == 0 and call(0, null="x") == 0
    assert _untouched(buf, h) and torch.equal(x, x0)


# ---------------------------------------------------------------------------------------------------------------------
# layernorm768_ex
# ---------------------------------------------------------------------------------------------------------------------
def _layernorm(flat, stride, w, b, rows, rev):
    buf, y = _out(rows * tk.WIDTH)
    L = _lib.lib()
    if rev is None:
        rc = L.lla_layernorm768(_lib.ptr(flat), stride, _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), rows, _lib.stream_ptr())
    else:
        rc = L.lla_layernorm768_ex(_lib.ptr(flat), stride, _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), rows, rev, _lib.stream_ptr())
    _lib.check(rc, "lla_layernorm768_ex")
    _written(buf, y, "layernorm768")
    return y.view(rows, tk.WIDTH)


@pytest.mark.parametrize("rows,stride", [(1, 768), (5, 768), (1001, 768), (7, 50 * 768)])
def test_layernorm768_both_walks_against_fp64(rows, stride):
    flat, w, b = (t.cuda() for t in tk.layernorm_rows_case(rows, stride))
    ref = tk.layernorm_f64(flat.view(rows, stride)[:, :tk.WIDTH], w, b)
    y0 = _layernorm(flat, stride, w, b, rows, 0)
    wst, r, c = tk.worst((y0.double() - ref).abs(), tk.layernorm_f16_bound(ref), f"layernorm768 ({rows}, {stride})")
    assert wst <= 1.0, (wst, r, c)
    for rev in (1, None):
        ok, msg = _same_bits(y0, _layernorm(flat, stride, w, b, rows, rev))
        assert ok, (rev, msg)


def test_layernorm768_ex_refusals():
    L, st = _lib.lib(), _lib.stream_ptr()
    flat, w, b = (t.cuda() for t in tk.layernorm_rows_case(5, 768))
    buf, y = _out(5 * tk.WIDTH)
    call = lambda stride, rows, rev: L.lla_layernorm768_ex(_lib.ptr(flat), stride, _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), rows, rev, st)
    assert call(764, 5, 0) == -1 and call(770, 5, 0) == -1 and call(768, -1, 0) == -1
    assert call(768, 5, 2) == -1 and call(768, 5, -1) == -1
    assert call(768, 0, 0) == 0 and call(768, 0, 1) == 0
    assert _untouched(buf, y)


# ---------------------------------------------------------------------------------------------------------------------
# avgpool2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W,pitch,C,out_pitch,off", tk.AVGPOOL_CASES)
def test_avgpool2_against_fp64(n, H, W, pitch, C, out_pitch, off):
    x = tk.avgpool_case(n, H, W, pitch, C).cuda()
    px = n * (H // 2) * (W // 2)
    buf, out = tk.guarded(px * out_pitch, torch.float16, _SENTINEL)
    out = out.view(px, out_pitch)
    out.view(torch.int16)[:, off:off + C] = tk.H_POISON
    rc = _lib.lib().lla_rn50_avgpool2_f16(_lib.ptr(x), n, H, W, pitch, C, _lib.ptr(out.view(-1)[off:]), out_pitch, _lib.stream_ptr())
    _lib.check(rc, "lla_rn50_avgpool2_f16")
    torch.cuda.synchronize()
    got = out[:, off:off + C].contiguous()
    assert not bool((_bits(got) == tk.H_POISON).any()), "avgpool2: elements not written"
    assert bool((out[:, :off] == _SENTINEL).all()) and bool((out[:, off + C:] == _SENTINEL).all()), "columns outside the output were written"
    assert tk.guards_intact(buf, _SENTINEL)
    ref, bound = tk.avgpool_bound(x, C)
    w, r, c = tk.worst((got.double() - ref.reshape(px, C)).abs(), bound.reshape(px, C), f"avgpool2 {(n, H, W, pitch, C, out_pitch, off)}")
    assert w <= 1.0, (w, r, c)
    ok, msg = _same_bits(got, tk.avgpool_exact(x, C).reshape(px, C).contiguous())
    assert ok, msg


def test_avgpool2_refusals():
    L, st = _lib.lib(), _lib.stream_ptr()
    x = tk.avgpool_case(1, 4, 4, 16, 16).cuda()
    buf, out = _out(4 * 16)
    call = lambda H=4, W=4, pitch=16, C=16, out_pitch=16, i=x, o=out, n=1: L.lla_rn50_avgpool2_f16(
        None if i is None else _lib.ptr(i), n, H, W, pitch, C, None if o is None else _lib.ptr(o), out_pitch, st)
    assert call(H=3) == -1 and call(W=3) == -1
    assert call(C=12) == -1 and call(pitch=20) == -1 and call(out_pitch=20) == -1 and call(C=0) == -1
    assert call(C=16, pitch=8) == -1 and call(C=16, out_pitch=8) == -1
    assert call(i=x.view(-1)[4:]) == -1 and call(o=out[4:]) == -1 and call(i=None) == -1 and call(o=None) == -1
    assert call(n=-1) == -1 and call(n=0) == 0
    assert _untouched(buf, out)


# ---------------------------------------------------------------------------------------------------------------------
# attnpool_tokens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 5])
def test_attnpool_tokens_against_fp64(B):
    x, pos = (t.cuda() for t in tk.tokens_case(B))
    buf, tok = _out(B * tk.RN_TOKENS * tk.RN_EMBED)
    _lib.check(_lib.lib().lla_rn50_attnpool_tokens_f16(_lib.ptr(x), _lib.ptr(pos), _lib.ptr(tok), B, _lib.stream_ptr()),
               "lla_rn50_attnpool_tokens_f16")
    _written(buf, tok, "attnpool_tokens")
    tok = tok.view(B, tk.RN_TOKENS, tk.RN_EMBED)
    ref, bound = tk.tokens_mean_bound(x, pos)
    w, r, c = tk.worst((tok[:, 0].double() - ref).abs(), bound, f"attnpool_tokens B {B} mean row")
    assert w <= 1.0, (w, r, c)
    ok, msg = _same_bits(tok[:, 1:].contiguous(), tk.tokens_rows_exact(x, pos))
    assert ok, msg
    L, st = _lib.lib(), _lib.stream_ptr()
    buf, t2 = _out(tk.RN_TOKENS * tk.RN_EMBED)
    assert L.lla_rn50_attnpool_tokens_f16(_lib.ptr(x), _lib.ptr(pos), _lib.ptr(t2), -1, st) == -1
    assert L.lla_rn50_attnpool_tokens_f16(None, _lib.ptr(pos), _lib.ptr(t2), 1, st) == -1
    assert L.lla_rn50_attnpool_tokens_f16(_lib.ptr(x), None, _lib.ptr(t2), 1, st) == -1
    assert L.lla_rn50_attnpool_tokens_f16(_lib.ptr(x), _lib.ptr(pos), None, 1, st) == -1
    assert L.lla_rn50_attnpool_tokens_f16(_lib.ptr(x), _lib.ptr(pos), _lib.ptr(t2), 0, st) == 0
    assert _untouched(buf, t2)


# ---------------------------------------------------------------------------------------------------------------------
# attnpool_attend
# ---------------------------------------------------------------------------------------------------------------------
def _attend(q, kv, B):
    buf, o = _out(B * tk.RN_EMBED)
    _lib.check(_lib.lib().lla_rn50_attnpool_attend_f16(_lib.ptr(q), _lib.ptr(kv), _lib.ptr(o), B, _lib.stream_ptr()),
               "lla_rn50_attnpool_attend_f16")
    _written(buf, o, "attnpool_attend")
    return o.view(B, tk.RN_EMBED)


@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("kind", tk.ATTEND_KINDS)
def test_attnpool_attend_against_fp64(kind, B):
    q, kv = (t.cuda() for t in tk.attend_case(kind, B))
    o = _attend(q, kv, B)
    ref, bound = tk.attend_bound(q, kv, B)
    w, r, c = tk.worst((o.double() - ref).abs(), bound, f"attnpool_attend {kind} B {B}")
    assert w <= 1.0, (w, r, c)
    if kind == "one_hot":       # the V row of the chosen key, to the rounding of the output
        keys = tk.attend_keys(B).cuda()
        v = kv.view(B, tk.RN_TOKENS, 2, tk.RN_HEADS, tk.HEAD_DIM)[:, :, 1].permute(0, 2, 1, 3)        # [B][32][50][64]
        want = torch.gather(v, 2, keys[..., None, None].expand(-1, -1, 1, tk.HEAD_DIM))[:, :, 0]
        assert torch.equal(o, want.reshape(B, tk.RN_EMBED)), "a head did not return the V row of its key"
    ok, msg = _same_bits(o, _attend(q, kv, B))
    assert ok, msg


def test_attnpool_attend_images_are_independent_and_refusals():
    q1, kv1 = (t.cuda() for t in tk.attend_case("random", 1, seed=5))
    alone = _attend(q1, kv1, 1)
    q = torch.empty(3, tk.RN_EMBED, dtype=torch.float16, device="cuda")
    kv = torch.empty(3 * tk.RN_TOKENS, 2 * tk.RN_EMBED, dtype=torch.float16, device="cuda")
    q[0], kv[:tk.RN_TOKENS] = float("nan"), float("nan")
    q[1], kv[tk.RN_TOKENS:2 * tk.RN_TOKENS] = q1[0], kv1
    sign = torch.where(torch.rand(tk.RN_TOKENS, 2 * tk.RN_EMBED, generator=torch.Generator().manual_seed(6)) < 0.5, -1.0, 1.0)
    q[2], kv[2 * tk.RN_TOKENS:] = 65504.0, (65504.0 * sign).half().cuda()
    o = _attend(q, kv, 3)
    ok, msg = _same_bits(o[1:2], alone)
    assert ok, msg
    assert bool(torch.isfinite(o[1]).all()) and bool(torch.isnan(o[0]).all())
    L, st = _lib.lib(), _lib.stream_ptr()
    buf, o2 = _out(tk.RN_EMBED)
    assert L.lla_rn50_attnpool_attend_f16(_lib.ptr(q1), _lib.ptr(kv1), _lib.ptr(o2), -1, st) == -1
    assert L.lla_rn50_attnpool_attend_f16(None, _lib.ptr(kv1), _lib.ptr(o2), 1, st) == -1
    assert L.lla_rn50_attnpool_attend_f16(_lib.ptr(q1), None, _lib.ptr(o2), 1, st) == -1
    assert L.lla_rn50_attnpool_attend_f16(_lib.ptr(q1), _lib.ptr(kv1), None, 1, st) == -1
    assert L.lla_rn50_attnpool_attend_f16(_lib.ptr(q1), _lib.ptr(kv1), _lib.ptr(o2), 0, st) == 0
    assert _untouched(buf, o2)
