"""CPU: the bounds of tower_kernel_util.py are honest.  For every case test_gpu_tower_kernels.py runs (same seeds and shapes, CPU
tensors) the float32 / fp16 restatement of the kernel's arithmetic is within the bound everywhere (its largest error / bound
ratio is printed: pytest -s), and float64 variants that are wrong on purpose break the bound by more than 10 x on the case named
for them.  No kernel runs here."""
import pytest
import torch

import tower_kernel_util as tk
from probe_util import U


def _ratio(out, ref, bound, what):
    return tk.worst((out.double() - ref).abs(), bound, what)[0]


# ---------------------------------------------------------------------------------------------------------------------
# attention50
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 67])
@pytest.mark.parametrize("kind", tk.ATTENTION_KINDS)
def test_attention_restatement_is_within_the_bound(kind, B):
    qkv = tk.attention_case(kind, B)
    ref, bound = tk.attention_bound(qkv, B)
    assert _ratio(tk.attention_restated(qkv, B), ref, bound, f"attention50 restated {kind} B {B}") <= 1.0


def _attention_variant(qkv, B, slots64=False, swap=None, scale=0.125, clamp=None, truncate_p=False):
    """softmax(q k^T scale) v in float64 with one thing wrong."""
    q, k, v = tk.split_heads(qkv.double(), B)
    s = q @ k.transpose(-1, -2) * scale
    if slots64:                        # keys 50..63 unmasked: 14 more slots of logit 0 (zero keys), zero values
        s = torch.cat([s, torch.zeros(B, tk.HEADS, tk.TOKENS, 14, dtype=s.dtype)], dim=-1)
    if clamp is not None:              # no max subtraction; the logits clamped instead so that nothing overflows
        e = torch.exp(s.clamp(-clamp, clamp))
        p = e / e.sum(dim=-1, keepdim=True)
    else:
        p = torch.softmax(s, dim=-1)
    p = p[..., :tk.TOKENS]
    if truncate_p:                     # P to fp16 towards zero
        h = p.half()
        over = h.double() > p
        h = torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)
        p = h.double()
    if swap is not None:               # P's slots j0 and j1 of one head meet each other's V rows
        head, j0, j1 = swap
        v = v.clone()
        v[:, head, [j0, j1]] = v[:, head, [j1, j0]]
    return tk.merge_heads(p @ v, B)


@pytest.mark.parametrize("name,kind,wrong", [
    ("denominator over 64 slots", "uniform", dict(slots64=True)),
    ("keys 31 and 32 swapped between P and V in head 5", "one_hot", dict(swap=(5, 31, 32))),
    ("keys 48 and 49 swapped between P and V in head 0", "one_hot", dict(swap=(0, 48, 49))),
    ("scale 0.125 (1 + 2^-7)", "large", dict(scale=0.125 * (1 + 2.0 ** -7))),
    ("no max subtraction, logits clamped to +-30", "large", dict(clamp=30.0)),
    ("keys 48, 49 dropped", "zero_v_tail", dict()),
])
def test_a_wrong_attention_would_show(name, kind, wrong):
    B = 3
    qkv = tk.attention_case(kind, B)
    ref, bound = tk.attention_bound(qkv, B)
    if name.startswith("keys 48, 49 dropped"):
        cut = qkv.clone()
        tk.split_heads(cut, B)[1][:, :, 48:] = 0          # their keys zeroed is not their probability zeroed:
        q, k, v = tk.split_heads(qkv.double(), B)          # drop them from the softmax and from the sum
        p = torch.softmax((q @ k.transpose(-1, -2) / 8.0)[..., :48], dim=-1)
        out = tk.merge_heads(p @ v[:, :, :48], B)
    else:
        out = _attention_variant(qkv, B, **wrong)
    assert _ratio(out, ref, bound, f"attention50 WRONG ({name}) on {kind}") > 10.0
    if kind == "large" and "clamped" in name:             # ... and it is the all-negative rows that show it
        rows = (torch.arange(B * tk.TOKENS) % tk.TOKENS) % 4 == 2
        assert float(((out - ref).abs() / bound)[rows].max()) > 10.0


def test_p_truncated_instead_of_rounded_would_show():
    """Truncation moves a probability by less than 2^-10 of itself, so it can pass twice the elementwise bound at the most, never
    10 x: what shows it is that every probability moves DOWN.  The mean signed error / bound (tk.signed_bias) of a
    round-to-nearest implementation is within tk.signed_bias_limit; truncation leaves more than 10 x that."""
    B, good, bad = 67, [], []
    for seed in tk.BIAS_SEEDS:            # (four draws of the largest case: the limit falls with the number of elements)
        qkv = tk.attention_case("random", B, seed)
        ref, bound = tk.attention_bound(qkv, B)
        good.append(tk.signed_bias(tk.attention_restated(qkv, B), ref, bound))
        bad.append(tk.signed_bias(_attention_variant(qkv, B, truncate_p=True).half(), ref, bound))
    limit = tk.signed_bias_limit(len(tk.BIAS_SEEDS) * ref.numel())
    good, bad = sum(good) / len(good), sum(bad) / len(bad)
    print(f"attention50 signed bias: restated {good:+.4f}, P truncated {bad:+.4f}, limit {limit:.4f}")
    assert abs(good) <= limit
    assert abs(bad) > 10.0 * limit


# ---------------------------------------------------------------------------------------------------------------------
# attnpool_attend
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("kind", tk.ATTEND_KINDS)
def test_attend_restatement_is_within_the_bound(kind, B):
    q, kv = tk.attend_case(kind, B)
    ref, bound = tk.attend_bound(q, kv, B)
    assert _ratio(tk.attend_restated(q, kv, B), ref, bound, f"attnpool_attend restated {kind} B {B}") <= 1.0


def test_a_wrong_attend_would_show():
    """Key 49 dropped (one_hot: heads 1 and 31 attend to it) and the scale off by 2^-7 (large)."""
    B = 3
    q, kv = tk.attend_case("one_hot", B)
    ref, bound = tk.attend_bound(q, kv, B)
    cut = kv.clone().view(B, tk.RN_TOKENS, 2, tk.RN_HEADS, tk.HEAD_DIM)
    cut[:, 49, 1] = 0
    out, _ = tk.attend_bound(q, cut.view(B * tk.RN_TOKENS, -1), B)
    assert _ratio(out, ref, bound, "attnpool_attend WRONG (value row 49 dropped) on one_hot") > 10.0
    q, kv = tk.attend_case("large", B)
    ref, bound = tk.attend_bound(q, kv, B)
    out, _ = tk.attend_bound((q.double() * (1 + 2.0 ** -7)), kv, B)
    assert _ratio(out, ref, bound, "attnpool_attend WRONG (scale 0.125 (1 + 2^-7)) on large") > 10.0


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", tk.LN_ROWS)
def test_ln_pre_ln1_restatement_is_within_the_bounds(rows):
    c = tk.ln_pre_case(rows)
    ref_x, bound_x = tk.ln_pre_x_bound(c)
    ref_h = tk.layernorm_f64(ref_x, c["w1"], c["b1"])
    for order in tk.SUM_ORDERS:
        x, h = tk.ln_pre_ln1_restated(c, order)
        assert _ratio(x, ref_x, bound_x, f"ln_pre_ln1 restated ({order}) rows {rows} x") <= 0.25       # k = 4 x the worst restatement
        assert _ratio(h, ref_h, tk.layernorm_f16_bound(ref_h), f"ln_pre_ln1 restated ({order}) rows {rows} h") <= 1.0
        own = tk.layernorm_f64(x, c["w1"], c["b1"])
        assert _ratio(h, own, tk.layernorm_f16_bound(own), f"ln_pre_ln1 restated ({order}) rows {rows} h of its own x") <= 1.0


def test_the_constant_of_the_x_bound_is_four_times_the_worst_restatement():
    """LN_K as ln_pre_x_bound's docstring derives it -- and the form without the mean's term has no constant: there the worst
    ratio sits at a column that happens to lie at the row's mean."""
    worst_with, worst_without = 0.0, 0.0
    for rows in tk.LN_ROWS:
        c = tk.ln_pre_case(rows)
        ref, mean, var = tk.layernorm_f64(tk.ln_pre_input(c).double(), c["wpre"], c["bpre"], with_stats=True)
        for order in tk.SUM_ORDERS:
            x, _ = tk.ln_pre_ln1_restated(c, order)
            excess = ((x.double() - ref).abs() - 2.0 ** -23 * ref.abs()).clamp_min(0.0)
            w = float((excess / tk.ln_pre_x_unit(c, ref, mean, var)).max())
            wo = float((excess / tk.ln_pre_x_unit(c, ref, mean, var, mean_term=False)).max())
            print(f"ln_pre x rows {rows} {order}: k needed {w:.2f} (without the mean's term {wo:.1f})")
            worst_with, worst_without = max(worst_with, w), max(worst_without, wo)
    assert worst_with <= tk.LN_K / 4.0 <= 2.0 * worst_with + 1.0
    assert worst_without > 25.0 * worst_with


def test_a_wrong_ln_pre_ln1_would_show():
    rows = 150
    c = tk.ln_pre_case(rows)
    ref_x, bound_x = tk.ln_pre_x_bound(c)
    ref_h = tk.layernorm_f64(ref_x, c["w1"], c["b1"])
    bound_h = tk.layernorm_f16_bound(ref_h)
    cls_rows = torch.arange(rows) % tk.TOKENS == 0
    # the class row without pos[0]
    no_pos = dict(c, pos=torch.zeros_like(c["pos"]))
    x = tk.layernorm_f64(tk.ln_pre_input(no_pos).double(), c["wpre"], c["bpre"])
    assert float(((x - ref_x).abs() / bound_x)[cls_rows].max()) > 10.0
    assert _ratio(tk.layernorm_f64(x, c["w1"], c["b1"]), ref_h, bound_h, "ln_pre_ln1 WRONG (class row without pos) h") > 10.0
    # ln_1 of the un-normalised input
    h = tk.layernorm_f64(tk.ln_pre_input(c).double(), c["w1"], c["b1"])
    assert _ratio(h, ref_h, bound_h, "ln_pre_ln1 WRONG (ln_1 of the input) h") > 10.0
    # a variance that has lost its resolution: Q / 768 off by an fp16 rounding (2^-11 mean^2) at mean = 36 sigma
    xin = tk.ln_pre_input(c).double()
    mean = xin.mean(dim=1, keepdim=True)
    var = ((xin - mean) ** 2).mean(dim=1, keepdim=True) + 2.0 ** -11 * mean ** 2
    x = (xin - mean) / torch.sqrt(var + 1e-5) * c["wpre"].double() + c["bpre"].double()
    assert _ratio(x, ref_x, bound_x, "ln_pre_ln1 WRONG (var off by 2^-11 mean^2) x") > 10.0


@pytest.mark.parametrize("rows,stride", [(1, 768), (5, 768), (1001, 768), (7, 50 * 768)])
def test_layernorm_restatement_is_within_the_bound(rows, stride):
    flat, w, b = tk.layernorm_rows_case(rows, stride)
    x = flat.view(rows, stride)[:, :tk.WIDTH]
    ref = tk.layernorm_f64(x, w, b)
    assert _ratio(tk.layernorm_restated(x, w, b).half(), ref, tk.layernorm_f16_bound(ref), f"layernorm768 restated ({rows}, {stride})") <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the RN50 tower's pools
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 5])
def test_tokens_restatement_and_a_wrong_mean(B):
    x, pos = tk.tokens_case(B)
    ref, bound = tk.tokens_mean_bound(x, pos)
    tok = tk.tokens_restated(x, pos)
    assert _ratio(tok[:, 0], ref, bound, f"attnpool_tokens restated B {B} mean row") <= 1.0
    assert float((tok[:, 1:].double() - (x.double() + pos[1:].double())).abs().max()) <= 2.0 ** -11 * 64     # |x + pos| < 64
    over50 = x.double().sum(dim=1) / 50.0 + pos[0].double()
    assert _ratio(over50, ref, bound, f"attnpool_tokens WRONG (mean over 50) B {B}") > 10.0


@pytest.mark.parametrize("n,H,W,pitch,C,out_pitch,off", tk.AVGPOOL_CASES)
def test_avgpool_restatement_and_a_wrong_window(n, H, W, pitch, C, out_pitch, off):
    x = tk.avgpool_case(n, H, W, pitch, C)
    ref, bound = tk.avgpool_bound(x, C)
    out = tk.avgpool_exact(x, C)
    assert bool(torch.isfinite(out).all())
    flat = lambda t: t.reshape(-1, C)
    assert _ratio(flat(out), flat(ref), flat(bound), f"avgpool2 restated {(n, H, W, C)}") <= 1.0
    # the window taken over a row-neighbour: pixels (y, x), (y, x + 1), (y, x + 2), (y, x + 3) of an unpitched walk -> (a + b) twice
    a, b, _, _ = (t.double() for t in tk._windows(x, C))
    wrong = (a + b + a + b) * 0.25
    assert _ratio(flat(wrong), flat(ref), flat(bound), f"avgpool2 WRONG (row neighbour) {(n, H, W, C)}") > 10.0


def test_the_unit_roundoff_is_fp32s():
    assert U == 2.0 ** -24 and tk.GUARD == 4096
