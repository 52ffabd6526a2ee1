"""Shared by test_tower_kernel_refs_host.py, test_gpu_tower_kernels.py and test_gpu_tower_gemms.py: for each of the towers'
kernels that is not a GEMM (csrc/layernorm_attention.hip, csrc/rn50.hip) the seeded cases, a float64 reference written from
the definition of the operation, the elementwise bound on |kernel - float64| derived from the kernel's arithmetic, and a
float32 / fp16 restatement of that arithmetic in torch -- the same rounding points (P to fp16, fp32 accumulation, fp16 output),
a summation order of its own.  The restatement only shows that a correct implementation reaches the bound (and how much of
it such an implementation uses); no kernel is ever compared with it.  Everything works on the device of its arguments; the
cases are drawn on the CPU, so a CPU test and a GPU test of the same (kind, shape) see the same values.  No test in here.

Worst restatement error / bound per case family (test_tower_kernel_refs_host.py prints them):
  attention50 random 0.76, one_hot 0.00 (P is exactly one-hot), uniform 0.47, large 0.62, zero_v_tail 0.85;
  attnpool_attend random 0.77, one_hot 0.00, uniform 0.93, large 0.66;  layernorm768 0.44;  h of ln_pre_ln1 0.44;
  x of ln_pre_ln1 0.245 (by construction of k, see ln_pre_x_bound);  attnpool_tokens mean row 0.98;  avgpool2 1.00."""
import torch

from probe_util import U, gamma

GUARD = 4096                # elements in front of and behind every guarded output
H_POISON = 0x7D5A           # an fp16 NaN: no kernel output has these bits
TOKENS, WIDTH, HEADS, HEAD_DIM = 50, 768, 12, 64        # the ViT tower
RN_TOKENS, RN_EMBED, RN_HEADS = 50, 2048, 32            # the RN50 tower's attention pool
LOGIT_RANGE = 56.0          # sum_d |q_d| |k_d| / 8 of every generated (query, key): see attention_bound


# ---------------------------------------------------------------------------------------------------------------------
# guards and the error / bound ratio
# ---------------------------------------------------------------------------------------------------------------------
def guarded(n, dtype, sentinel, device="cuda"):
    """A flat buffer of n elements between two guard blocks: (whole buffer, the n elements)."""
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, sentinel):
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[-GUARD:] == sentinel).all())


def worst(err, bound, what):
    """Largest err / bound, printed with the row and column it sits at (a NaN error counts as infinite)."""
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = err / bound
    flat = int(ratio.argmax())
    r, c = divmod(flat, ratio.shape[1])
    w = float(ratio.reshape(-1)[flat])
    print(f"{what}: max err/bound {w:.3f} at row {r} col {c} (err {float(err[r, c]):.3e})")
    return w, r, c


def _cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# attention50: qkv fp16 [B * 50][2304] = (q | k | v), 12 heads of 64 -> o fp16 [B * 50][768]
# ---------------------------------------------------------------------------------------------------------------------
ATTENTION_KINDS = ("random", "one_hot", "uniform", "large", "zero_v_tail")


def split_heads(qkv, B):
    """qkv [B * 50][2304] -> q, k, v, each [B][12][50][64] (views, in qkv's dtype)."""
    return qkv.view(B, TOKENS, 3, HEADS, HEAD_DIM).permute(2, 0, 3, 1, 4)


def merge_heads(o, B):
    return o.permute(0, 2, 1, 3).reshape(B * TOKENS, WIDTH)


def one_hot_permutations(B, seed):
    """[B][12][50] int64: query i of (image, head) attends to key perm[i]; every (image, head) has another permutation, all of
    them map 49 -> 49 (heads 0 mod 3), or 0 -> 49 and 49 -> 0 (heads 1 mod 3), or 31 <-> 32 and 47 <-> 48 (heads 2 mod 3)."""
    g = _cpu_gen(1000 + seed)
    perm = torch.empty(B, HEADS, TOKENS, dtype=torch.int64)
    for b in range(B):
        for h in range(HEADS):
            kind = h % 3
            fixed = {0: {49: 49}, 1: {0: 49, 49: 0}, 2: {31: 32, 32: 31, 47: 48, 48: 47}}[kind]
            rest = [i for i in range(TOKENS) if i not in fixed]
            targets = [j for j in range(TOKENS) if j not in fixed.values()]
            shuffled = [targets[int(t)] for t in torch.randperm(len(targets), generator=g)]
            p = dict(fixed)
            p.update(zip(rest, shuffled))
            perm[b, h] = torch.tensor([p[i] for i in range(TOKENS)])
    return perm


def attention_case(kind, B, seed=0):
    """-> qkv fp16 [B * 50][2304] on the CPU.  Every kind keeps sum_d |q_d| |k_d| / 8 <= LOGIT_RANGE for every (query, key) and
    sum_j |v_jd| >= 1 for every (image, head, d): the assumptions of attention_bound (asserted here).
      random       N(0, 1), Q x 2 (test_attention50's inputs)
      one_hot      k_j = 8 e_j, q_i = +20 e_perm(i) - 20 (every other e_j): the logit of key perm(i) leads by 40
      uniform      Q = 0: every output row is the mean of the 50 V rows
      large        k_j = 8 e_j, so q_i IS the row of logits: a random ranking of the keys, logit = top - step * rank with (top,
                   step) = (56, 1.5) [mixed signs, down to -17.5], (20, 1.5), (-30, 0.5) [all <= -30, down to -54.5] and (0, 0.5) in
                   turn over the queries; V is zero in columns 0..7 for keys 0..24 and in columns 8..15 for keys 25..49, so that
                   those columns show the probabilities of keys that do NOT lead
      zero_v_tail  random, but V rows 48, 49 are +-(4 + |N|) and the others 1/64 of N(0, 1)"""
    g = _cpu_gen(seed * 131 + B * 7 + ATTENTION_KINDS.index(kind))
    qkv = torch.randn(B * TOKENS, 3 * WIDTH, generator=g)
    q, k, v = split_heads(qkv, B)
    if kind == "random":
        q *= 2.0
    elif kind == "uniform":
        q.zero_()
    elif kind == "zero_v_tail":
        q *= 2.0
        v[:, :, :48] *= 1.0 / 64
        v[:, :, 48:] = torch.sign(v[:, :, 48:]) * (4.0 + v[:, :, 48:].abs())
    else:
        eye = torch.zeros(TOKENS, HEAD_DIM)
        eye[torch.arange(TOKENS), torch.arange(TOKENS)] = 1.0
        k.copy_((8.0 * eye).expand(B, HEADS, TOKENS, HEAD_DIM))
        q.zero_()
        if kind == "one_hot":
            perm = one_hot_permutations(B, seed)
            q[..., :TOKENS] = -20.0
            q[..., :TOKENS].scatter_(3, perm[..., None], 20.0)
        else:
            rank = torch.rand(B, HEADS, TOKENS, TOKENS, generator=g).argsort(dim=-1).argsort(dim=-1).float()
            i = torch.arange(TOKENS) % 4
            top = torch.tensor([56.0, 20.0, -30.0, 0.0])[i][:, None]
            step = torch.tensor([1.5, 1.5, 0.5, 0.5])[i][:, None]
            q[..., :TOKENS] = top - step * rank
            v[:, :, :25, 0:8] = 0.0
            v[:, :, 25:, 8:16] = 0.0
    qkv = qkv.half()
    q, k, v = split_heads(qkv.double(), B)
    assert float((q.abs() @ k.abs().transpose(-1, -2)).max()) / 8.0 <= LOGIT_RANGE
    assert float(v.abs().sum(dim=2).min()) >= 1.0
    return qkv


def attention_f64(qkv, B):
    """softmax(q k^T / 8) v per (image, head) in float64 -> [B * 50][768]."""
    q, k, v = split_heads(qkv.double(), B)
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    return merge_heads(p @ v, B)


def _softmax_fp32_terms(absdot, s, n_sum):
    """The relative error of a probability computed in fp32 from exact products, per query ([..., queries, 1]):
         scores   64 exact products added in fp32 in some order, the scale 1/8 exact: |s^ - s| <= gamma_64 A, A = sum_d |q_d| |k_d| / 8;
                  it enters exp(s_j) / sum_k exp(s_k) relatively, once above and once below the line: 2 gamma_64 A_max
         t = s - max rounded once, t log2(e) rounded once, log2(e) itself rounded: exp(t) is off by 3 u |t| relatively, and the
                  hardware exponential (__expf: v_exp_f32, 1 ulp) by 2 u; above and below the line: 2 (3 u T + 2 u), T = max_j |t_j|
                  (an exponential below 2^-126 is flushed: an absolute error of 2^-126 in p, far inside the 2^-25 term of the bounds)
         the sum of n_sum exponentials in some order gamma_{n_sum}, the reciprocal 4 u (correctly rounded or not), e * inv u."""
    A = absdot.amax(dim=-1, keepdim=True)
    T = (s - s.amax(dim=-1, keepdim=True)).abs().amax(dim=-1, keepdim=True)
    return 2.0 * gamma(64) * A + 2.0 * (3.0 * U * T + 2.0 * U) + gamma(n_sum) + 5.0 * U


def attention_bound(qkv, B):
    """float64 reference and the elementwise bound on |attention50_kernel - float64|  (p = the float64 softmax):

        2^-11 |ref|  +  c_i sum_j p_ij |v_jd|  +  2^-25 sum_j |v_jd|

      2^-11 |ref|              the output's rounding to fp16
      c_i = (2^-11 + f_i + gamma_64) (1 + 2^-9)
          2^-11                P's rounding to fp16 (normal range)
          f_i                  the fp32 terms of _softmax_fp32_terms (64 key slots are summed)
          gamma_64             the fp32 accumulation of 64 slots of exact fp16 x fp16 products in the second MFMA
          (1 + 2^-9)           the products of these terms with each other and with the output's rounding
      2^-25 sum_j |v_jd|       probabilities below fp16's normal range (2^-14) are rounded to a multiple of 2^-24; with
                               sum_j |v_jd| >= 1 (attention_case asserts it) the term also holds an output below 2^-14
    No flat term.  With A <= R for all pairs of a query (hence T <= 2 R), f_i <= (128 R + 12 R + 4 + 64 + 5 + eps) u, which stays
    below 2^-11 = 8192 u for R <= 57.9: LOGIT_RANGE = 56, and attention_case keeps every case inside it, so c_i < 2^-10 (1 + 2^-9)
    everywhere -- the bound computes f_i from the case, which is smaller still where the logits are.
    -> (ref [B * 50][768], bound [B * 50][768])."""
    q, k, v = split_heads(qkv.double(), B)
    s = q @ k.transpose(-1, -2) / 8.0
    p = torch.softmax(s, dim=-1)
    f = _softmax_fp32_terms(q.abs() @ k.abs().transpose(-1, -2) / 8.0, s, 64)
    c = (2.0 ** -11 + f + gamma(64)) * (1.0 + 2.0 ** -9)
    ref = p @ v
    bound = 2.0 ** -11 * ref.abs() + c * (p @ v.abs()) + 2.0 ** -25 * v.abs().sum(dim=2, keepdim=True)
    return merge_heads(ref, B), merge_heads(bound, B)


def attention_restated(qkv, B):
    """attention50_kernel's arithmetic in torch: fp32 scores from the fp16 operands, x 1/8, - max, exp, sum, reciprocal, P to fp16,
    P V accumulated in fp32, the output to fp16."""
    q, k, v = split_heads(qkv.float(), B)
    s = (q @ k.transpose(-1, -2)) * 0.125
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    p = (e * (1.0 / e.sum(dim=-1, keepdim=True))).half()
    return merge_heads((p.float() @ v).half(), B)


def signed_bias(out, ref, bound):
    """mean of sign(ref) (out - ref) / bound.  Every term lies in [-1, 1] for an implementation within its bound and has mean zero
    when its roundings are to nearest.  P's rounding is shared by the 64 columns of a (query, head), so of N elements N / 64
    count as independent: |bias| <= 4 / sqrt(N / 64) is four standard deviations of that mean at the most."""
    return float((torch.sign(ref) * (out.double() - ref) / bound).mean())


BIAS_SEEDS = (0, 1, 2, 3)


def signed_bias_limit(n):
    return 4.0 / (n / 64.0) ** 0.5


# ---------------------------------------------------------------------------------------------------------------------
# attnpool_attend: q fp16 [B][2048], kv fp16 [B * 50][4096] = (k | v), 32 heads of 64 -> o fp16 [B][2048]
# ---------------------------------------------------------------------------------------------------------------------
ATTEND_KINDS = ("random", "one_hot", "uniform", "large")


def attend_keys(B, seed=0):
    """The key each (image, head) of the one_hot kind attends to: [B][32], keys 0 and 49 among them in every image."""
    keys = torch.randint(0, RN_TOKENS, (B, RN_HEADS), generator=_cpu_gen(2000 + seed))
    keys[:, 0] = 0
    keys[:, 1] = 49
    keys[:, 31] = 49
    return keys


def attend_case(kind, B, seed=0):
    """-> (q fp16 [B][2048], kv fp16 [B * 50][4096]) on the CPU, inside LOGIT_RANGE and with sum_j |v_jd| >= 1 (asserted).
    random: N(0, 1), q x 2;  one_hot: k_j = 8 e_j, q = +-20 as attention_case;  uniform: q = 0;  large: k_j = 8 e_j, the logits
    top - step * rank of attention_case's large kind with (top, step) in turn over the heads."""
    g = _cpu_gen(seed * 131 + B * 11 + ATTEND_KINDS.index(kind))
    q = torch.randn(B, RN_HEADS, HEAD_DIM, generator=g) * 2.0
    kv = torch.randn(B, RN_TOKENS, 2, RN_HEADS, HEAD_DIM, generator=g)
    if kind == "uniform":
        q.zero_()
    elif kind != "random":
        eye = torch.zeros(RN_TOKENS, HEAD_DIM)
        eye[torch.arange(RN_TOKENS), torch.arange(RN_TOKENS)] = 1.0
        kv[:, :, 0] = (8.0 * eye)[None, :, None, :]
        q.zero_()
        if kind == "one_hot":
            q[..., :RN_TOKENS] = -20.0
            q[..., :RN_TOKENS].scatter_(2, attend_keys(B, seed)[..., None], 20.0)
        else:
            rank = torch.rand(B, RN_HEADS, RN_TOKENS, generator=g).argsort(dim=-1).argsort(dim=-1).float()
            i = torch.arange(RN_HEADS) % 4
            top = torch.tensor([56.0, 20.0, -30.0, 0.0])[i][:, None]
            step = torch.tensor([1.5, 1.5, 0.5, 0.5])[i][:, None]
            q[..., :RN_TOKENS] = top - step * rank
            kv[:, :25, 1, :, 0:8] = 0.0
            kv[:, 25:, 1, :, 8:16] = 0.0
    q, kv = q.reshape(B, RN_EMBED).half(), kv.reshape(B * RN_TOKENS, 2 * RN_EMBED).half()
    qd, kd, vd = _attend_split(q.double(), kv.double(), B)
    assert float((qd.abs()[:, :, None, :] * kd.abs()).sum(-1).max()) / 8.0 <= LOGIT_RANGE
    assert float(vd.abs().sum(dim=2).min()) >= 1.0
    return q, kv


def _attend_split(q, kv, B):
    """-> q [B][32][64], k [B][32][50][64], v [B][32][50][64]."""
    kv = kv.view(B, RN_TOKENS, 2, RN_HEADS, HEAD_DIM).permute(2, 0, 3, 1, 4)
    return q.view(B, RN_HEADS, HEAD_DIM), kv[0], kv[1]


def attend_bound(q, kv, B):
    """float64 softmax(q k^T / 8) v of the class query per (image, head) and the bound on |attnpool_attend_kernel - float64|:

        2^-11 |ref|  +  c sum_j p_j |v_jd|  +  2^-25 sum_j |v_jd|

    the form of attention_bound without P's rounding to fp16 -- everything stays fp32 until the output:
      c = (f + gamma_51 + u) (1 + 2^-9):  f the fp32 terms of _softmax_fp32_terms (q / 8 exact, the 64 products exact, their
          sum a 64-lane DPP tree: at most gamma_64; 50 exponentials summed); p_j v_j rounded once (u) and 50 of them accumulated
      2^-25 sum_j |v_jd| holds an output below fp16's normal range (sum_j |v_jd| >= 1: attend_case asserts it).
    -> (ref [B][2048], bound [B][2048])."""
    qd, k, v = _attend_split(q.double(), kv.double(), B)
    s = (qd[:, :, None, :] * k).sum(-1) / 8.0                         # [B][32][50]
    absdot = (qd.abs()[:, :, None, :] * k.abs()).sum(-1) / 8.0
    p = torch.softmax(s, dim=-1)
    c = (_softmax_fp32_terms(absdot, s, 50) + gamma(51) + U) * (1.0 + 2.0 ** -9)
    ref = (p[..., None] * v).sum(2)
    bound = 2.0 ** -11 * ref.abs() + c * (p[..., None] * v.abs()).sum(2) + 2.0 ** -25 * v.abs().sum(2)
    return ref.reshape(B, RN_EMBED), bound.reshape(B, RN_EMBED)


def attend_restated(q, kv, B):
    qf, k, v = _attend_split(q.float(), kv.float(), B)
    s = ((qf * 0.125)[:, :, None, :] * k).sum(-1)
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    p = e * (1.0 / e.sum(dim=-1, keepdim=True))
    return (p[..., None] * v).sum(2).half().reshape(B, RN_EMBED)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm over 768: layernorm768_kernel and ln_pre_ln1_kernel
# ---------------------------------------------------------------------------------------------------------------------
def layernorm_f64(x, gamma_, beta, with_stats=False):
    """Two-pass LayerNorm over the last dimension in float64 (mean, then the mean of the squared deviations), eps 1e-5."""
    xd = x.double()
    mean = xd.mean(dim=1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=1, keepdim=True)
    y = (xd - mean) / torch.sqrt(var + 1e-5) * gamma_.double() + beta.double()
    return (y, mean, var) if with_stats else y


def layernorm_f16_bound(ref):
    """The project's bound on an fp16 LayerNorm output (test_layernorm768, B1, B3): 2^-10 |ref| + 1e-3."""
    return ref.abs() * 2.0 ** -10 + 1e-3


def _sum_sequential(v):
    acc = torch.zeros_like(v[:, 0])
    for c in range(v.shape[1]):
        acc = acc + v[:, c]
    return acc


def _sum_pairwise(v):
    while v.shape[1] > 1:
        if v.shape[1] % 2:
            v = torch.cat([v[:, :-2], (v[:, -2] + v[:, -1])[:, None]], dim=1)
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def _sum_kernel_order(v):
    """row_stats' tree: the lane's quad (a + b) + (c + d), the 64 lanes of a 256-column tile pairwise, then (t0 + t1) + t2."""
    quad = v.view(-1, 3, 64, 4)
    t = (quad[..., 0] + quad[..., 1]) + (quad[..., 2] + quad[..., 3])
    while t.shape[2] > 1:
        t = t[:, :, 0::2] + t[:, :, 1::2]
    t = t[:, :, 0]
    return (t[:, 0] + t[:, 1]) + t[:, 2]


SUM_ORDERS = {"sequential": _sum_sequential, "pairwise": _sum_pairwise, "kernel": _sum_kernel_order}


def layernorm_restated(x, gamma_, beta, order="kernel"):
    """ln_finish / ln_affine (csrc/gemm_common.h) in float32: the ONE-pass statistics mean = S / 768, var = max(Q / 768 - mean^2,
    0), rstd = 1 / sqrt(var + 1e-5), y = (x - mean) rstd gamma + beta, every operation rounded on its own (the library is
    built without contraction).  -> float32."""
    x = x.float()
    add = SUM_ORDERS[order]
    inv = torch.tensor(1.0 / 768.0, dtype=torch.float32, device=x.device)
    mean = (add(x) * inv)[:, None]
    var = torch.clamp_min(add(x * x)[:, None] * inv - mean * mean, 0.0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    return (x - mean) * rstd * gamma_.float() + beta.float()


LN_ROWS = (50, 150, 203, 3400)
LN_K = 108.0                # see ln_pre_x_bound


def ln_pre_case(rows, seed=0):
    """-> dict of CPU tensors: x fp32 [rows][768] (class rows r % 50 == 0 NaN: the kernel must not read them), cls, pos (row 0
    of the positional embedding), wpre, bpre, w1, b1.  Patch row r holds sigma randn + ratio sigma with (sigma, ratio) =
    ((0.3, 3)[r % 2], (0, 4, 36)[r % 3]) -- the values of test_layernorm_under_a_row_offset, every pair among any 6 rows -- and
    two outlier columns + 20 sigma; cls + pos has an offset of its own (4 sigma at sigma 0.5); all four affine vectors differ."""
    g = _cpu_gen(seed * 17 + rows)
    r = torch.arange(rows)
    sigma = torch.tensor([0.3, 3.0])[r % 2][:, None]
    ratio = torch.tensor([0.0, 4.0, 36.0])[r % 3][:, None]
    x = sigma * torch.randn(rows, WIDTH, generator=g) + ratio * sigma
    x[:, 77] += 20 * sigma[:, 0]
    x[:, 500] += 20 * sigma[:, 0]
    x[r % TOKENS == 0] = float("nan")
    c = dict(x=x, cls=0.5 * torch.randn(WIDTH, generator=g) + 1.5, pos=0.1 * torch.randn(WIDTH, generator=g) + 0.5,
             wpre=1 + 0.3 * torch.randn(WIDTH, generator=g), bpre=0.2 * torch.randn(WIDTH, generator=g),
             w1=0.7 + 0.2 * torch.randn(WIDTH, generator=g), b1=0.1 * torch.randn(WIDTH, generator=g) - 0.05)
    return c


def ln_pre_input(c):
    """What ln_pre sees: the patch rows of x, and cls + pos[0] (one fp32 addition) on the class rows."""
    x = c["x"].clone()
    cls_rows = torch.arange(x.shape[0], device=x.device) % TOKENS == 0
    x[cls_rows] = c["cls"] + c["pos"]
    return x


def ln_pre_x_bound(c, k=LN_K):
    """Two-pass float64 ln_pre of the assembled rows and the bound on the fp32 x that ln_pre_ln1_kernel writes:

        k 2^-24 [ (1 + mean^2 / var) |ref - beta|  +  (1 + |mean| / sigma) |gamma| ]  +  2^-23 |ref|         sigma^2 = var + eps

      (1 + mean^2 / var) |ref - beta|   var = Q / 768 - mean^2 subtracts two numbers of size mean^2 + var that each carry a few u
                                        of relative error: rstd is off by that times (1 + mean^2 / var) / 2, and so is
                                        (x - mean) rstd gamma = ref - beta
      (1 + |mean| / sigma) |gamma|      the computed mean is off by a few u (|mean| + sigma), and x - mean with it, in EVERY column:
                                        gamma / sigma times that, however small |ref - beta| is
      2^-23 |ref|                       the last product and the addition of beta
    The issue that asked for this bound named the first and the last term only.  The restatement shows that no k serves
    then: at mean = 36 sigma the columns with x within sigma / 100 of the mean have |ref - beta| -> 0 while their error stays at
    36 u |gamma| ((err - 2^-23 |ref|) / (2^-24 (1 + mean^2 / var) |ref - beta|) reaches 2.9e4 at one such column for rows 50 and
    8.7e5 for rows 3400, sequential order; 4.0e3 and 1.6e5 in the kernel's order: it grows with the number of columns drawn).  With the second term the ratio is flat over the columns.
    k: the float32 restatement layernorm_restated in its three summation orders over ln_pre_case(rows) for rows in LN_ROWS gives
    (err - 2^-23 |ref|) / (2^-24 [...]) <= 26.43 (sequential 26.43 at rows 3400, pairwise 3.14, the kernel's order 3.64); k = 4 x 27 =
    108, the margin for summation orders the restatement does not reproduce.  Not tuned on kernel output.
    -> (ref, bound), float64 [rows][768]."""
    ref, mean, var = layernorm_f64(ln_pre_input(c).double(), c["wpre"], c["bpre"], with_stats=True)
    return ref, k * ln_pre_x_unit(c, ref, mean, var) + 2.0 ** -23 * ref.abs()


def ln_pre_x_unit(c, ref, mean, var, mean_term=True):
    """2^-24 [...] of ln_pre_x_bound (mean_term False: the first term alone)."""
    unit = (1.0 + mean ** 2 / var) * (ref - c["bpre"].double()).abs()
    if mean_term:
        unit = unit + (1.0 + mean.abs() / torch.sqrt(var + 1e-5)) * c["wpre"].double().abs()
    return U * unit


def ln_pre_ln1_restated(c, order="kernel"):
    """-> (x float32, h fp16): ln_pre of the assembled rows in float32, ln_1 of THAT x, rounded to fp16."""
    x = layernorm_restated(ln_pre_input(c), c["wpre"], c["bpre"], order)
    return x, layernorm_restated(x, c["w1"], c["b1"], order).half()


def layernorm_rows_case(rows, stride, seed=0):
    """-> (flat fp32 [rows * stride] whose padding between the 768-wide rows is NaN, gamma, beta) on the CPU."""
    g = _cpu_gen(seed * 13 + rows + stride)
    x = torch.full((rows, stride), float("nan"))
    x[:, :WIDTH] = torch.randn(rows, WIDTH, generator=g) * 3 + 1
    return x.view(-1), torch.randn(WIDTH, generator=g), torch.randn(WIDTH, generator=g)


# ---------------------------------------------------------------------------------------------------------------------
# attnpool_tokens: x fp16 [B][49][2048], pos fp32 [50][2048] -> tok fp16 [B][50][2048]
# ---------------------------------------------------------------------------------------------------------------------
def tokens_case(B, seed=0):
    """x = a per-channel mean of +-30 + 0.5 N(0, 1) (the mean row cancels nothing, the sum of 49 is not exact in fp32);
    pos N(0, 1)."""
    g = _cpu_gen(seed * 19 + B)
    base = 30.0 * torch.sign(torch.randn(RN_EMBED, generator=g))
    x = (base + 0.5 * torch.randn(B, 49, RN_EMBED, generator=g)).half()
    return x, torch.randn(RN_TOKENS, RN_EMBED, generator=g)


def tokens_rows_exact(x, pos):
    """Token rows 1 + j: one IEEE addition in fp32, one rounding to nearest even -- the kernel's operations, so its bits."""
    return (x.float() + pos[1:].float()).half()


def tokens_mean_bound(x, pos):
    """The mean row in float64 and its bound 2^-11 |ref| + gamma_51 (sum_j |x_j| / 49 + |pos_0|): 49 additions, the product with
    the rounded 1 / 49 and the addition of pos (which may be contracted, so no bit comparison), then the rounding to fp16."""
    xd = x.double()
    ref = xd.mean(dim=1) + pos[0].double()
    return ref, 2.0 ** -11 * ref.abs() + gamma(51) * (xd.abs().sum(dim=1) / 49.0 + pos[0].double().abs())


def tokens_restated(x, pos):
    """-> tok fp16 [B][50][2048]: the mean row from a pairwise fp32 sum."""
    xf = x.float()
    mean = _sum_pairwise(xf.permute(0, 2, 1).reshape(-1, 49)).view(x.shape[0], RN_EMBED)
    row0 = (mean * torch.tensor(1.0 / 49.0, dtype=torch.float32, device=x.device) + pos[0].float()).half()
    return torch.cat([row0[:, None], tokens_rows_exact(x, pos)], dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# avgpool2: in fp16 NHWC [n][H][W][pitch] -> out fp16 [n][H/2][W/2][out_pitch], the first C channels
# ---------------------------------------------------------------------------------------------------------------------
# (n, H, W, pitch, C, out_pitch, column offset of out): a 2 x 3 map of outputs; the smallest call; odd numbers of 16-byte vectors per
# pixel and padding on both sides; the write into the right part of the concatenated buffer (cat + c2.cout)
AVGPOOL_CASES = ((2, 4, 6, 64, 64, 64, 0), (1, 2, 2, 8, 8, 8, 0), (1, 14, 14, 320, 256, 288, 0), (3, 28, 28, 512, 512, 1536, 512))


def avgpool_case(n, H, W, pitch, C, seed=0):
    """-> fp16 [n][H][W][pitch] on the CPU: N(0, 1) x 2^e with e uniform in -10..10 (so the fp32 additions are not all exact),
    the padding channels NaN."""
    g = _cpu_gen(seed * 23 + n * H * W + C)
    x = torch.full((n, H, W, pitch), float("nan"))
    x[..., :C] = torch.randn(n, H, W, C, generator=g) * 2.0 ** torch.randint(-10, 11, (n, H, W, C), generator=g).float()
    return x.half()


def _windows(x, C):
    """-> a, b, c, d: the 2 x 2 window's pixels (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1), each [n][H/2][W/2][C]."""
    x = x[..., :C]
    return x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]


def avgpool_exact(x, C):
    """The kernel's arithmetic: no fma opportunity, the product with 0.25 exact -- so its bits."""
    a, b, c, d = (t.float() for t in _windows(x, C))
    return (((a + b) + (c + d)) * 0.25).half()


def avgpool_bound(x, C):
    """The float64 mean of the window and the bound 2^-11 |ref| + 3 2^-24 (|a| + |b| + |c| + |d|) / 4 + 2^-25: the output's
    rounding, three fp32 additions, and an output below fp16's normal range."""
    a, b, c, d = (t.double() for t in _windows(x, C))
    ref = (a + b + c + d) / 4.0
    return ref, 2.0 ** -11 * ref.abs() + 3.0 * U * (a.abs() + b.abs() + c.abs() + d.abs()) / 4.0 + 2.0 ** -25
