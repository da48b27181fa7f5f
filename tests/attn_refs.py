"""float64 restatement of Self_Attn (layers/attention_layer.py:8-40) and of its gradients, the reference of
tests/test_attn_cpu.py and tests/test_gpu_attn_kernels.py, with the inputs those tests share.

With d = C / 8, N = H W and x seen as (B, C, N):
    q = Wq x + bq (d x N)     k = Wk x + bk (d x N)     v = Wv x + bv (C x N)
    S[i, j] = sum_r q[r, i] k[r, j]      P = softmax over j of S
    o[c, i] = sum_j v[c, j] P[i, j]      y = gamma o + x
and for a cotangent dy of y, with do = gamma dy and D[i] = sum_c do[c, i] o[c, i]:
    dv[c, j] = sum_i do[c, i] P[i, j]    dP[i, j] = sum_c do[c, i] v[c, j]     dS = P o (dP - D[i])
    dq[:, i] = sum_j dS[i, j] k[:, j]    dk[:, j] = sum_i dS[i, j] q[:, i]      dgamma = sum dy o
    dx = dy + Wq^T dq + Wk^T dk + Wv^T dv,   dW* = d* x^T summed over the batch,   db* = d* summed over B, N

The key bias has no effect on the output: it adds q[r, i] bk[r] to every score of row i, and a softmax
ignores a constant added to its row.  Its gradient sum_j dk[r, j] is therefore exactly zero, every
rows's dS summing to zero, and what any implementation returns is the rounding left by that cancellation.
grad_err measures it against the cancellation's own scale, sum_j |dk[r, j]| (``key_conv.bias.scale``).
"""
import collections
import functools

import torch

NAMES = ("query_conv.weight", "query_conv.bias", "key_conv.weight", "key_conv.bias", "value_conv.weight",
         "value_conv.bias", "gamma")


def normwise(out, ref):
    out, ref = out.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    return float(torch.linalg.vector_norm(out - ref) / torch.clamp(torch.linalg.vector_norm(ref), min=1e-300))


def grad_err(name, out, grads):
    """normwise error of gradient ``name`` against grads[name]; the key bias against its cancellation scale"""
    if name == "key_conv.bias":
        d = out.detach().cpu().double().reshape(-1) - grads[name].reshape(-1)
        scale = torch.linalg.vector_norm(grads["key_conv.bias.scale"])   # 0 at N = 1, where dk itself is 0
        return float(torch.linalg.vector_norm(d) / torch.clamp(scale, min=1e-300))
    return normwise(out, grads[name])


def _f64(p):
    return {k: v.detach().cpu().double() for k, v in p.items()}


def attn_ref(x, p):
    """-> dict(out (B, C, H, W), attention (B, N, N), and the intermediates q, k, v, o) in float64.
    p: the layer's state_dict (conv weights (M, C, 1, 1))"""
    p = _f64(p)
    x = x.detach().cpu().double()
    B, C, H, W = x.shape
    xf = x.reshape(B, C, H * W)

    def proj(name):
        w = p[name + ".weight"]
        return torch.einsum("mc,bcn->bmn", w.reshape(w.shape[0], C), xf) + p[name + ".bias"].reshape(1, -1, 1)

    q, k, v = proj("query_conv"), proj("key_conv"), proj("value_conv")
    S = torch.einsum("bri,brj->bij", q, k)
    P = torch.softmax(S, dim=-1)
    o = torch.einsum("bcj,bij->bci", v, P)
    out = (p["gamma"].reshape(()) * o + xf).reshape(B, C, H, W)
    return dict(out=out, attention=P, q=q, k=k, v=v, o=o, S=S)


def attn_ref_backward(x, p, dy):
    """gradients of <out, dy> from the formulas above -> dict: "x" and every name of NAMES, float64"""
    r = attn_ref(x, p)
    p = _f64(p)
    x = x.detach().cpu().double()
    B, C, H, W = x.shape
    xf, dyf = x.reshape(B, C, -1), dy.detach().cpu().double().reshape(B, C, -1)
    q, k, v, o, P = r["q"], r["k"], r["v"], r["o"], r["attention"]
    do = p["gamma"].reshape(()) * dyf
    D = (do * o).sum(1)
    dv = torch.einsum("bci,bij->bcj", do, P)
    dP = torch.einsum("bci,bcj->bij", do, v)
    dS = P * (dP - D[:, :, None])
    dq = torch.einsum("bij,brj->bri", dS, k)
    dk = torch.einsum("bij,bri->brj", dS, q)
    g = {"gamma": (dyf * o).sum().reshape(1)}
    dx = dyf.clone()
    for name, dz in (("query_conv", dq), ("key_conv", dk), ("value_conv", dv)):
        w = p[name + ".weight"]
        dx = dx + torch.einsum("mc,bmn->bcn", w.reshape(w.shape[0], C), dz)
        g[name + ".weight"] = torch.einsum("bmn,bcn->mc", dz, xf).reshape(w.shape)
        g[name + ".bias"] = dz.sum((0, 2))
    g["key_conv.bias.scale"] = dk.abs().sum((0, 2))
    g["x"] = dx.reshape(B, C, H, W)
    return g


def aten_composition(x, p):
    """the reference's forward as ATen calls in the dtype of x (conv2d, bmm, softmax, bmm) -> (out, attention);
    differentiable"""
    F = torch.nn.functional
    B, C, H, W = x.shape
    N = H * W
    q = F.conv2d(x, p["query_conv.weight"], p["query_conv.bias"]).view(B, -1, N).permute(0, 2, 1)
    k = F.conv2d(x, p["key_conv.weight"], p["key_conv.bias"]).view(B, -1, N)
    attention = torch.softmax(torch.bmm(q, k), dim=-1)
    v = F.conv2d(x, p["value_conv.weight"], p["value_conv.bias"]).view(B, -1, N)
    out = torch.bmm(v, attention.permute(0, 2, 1)).view(B, C, H, W)
    return p["gamma"] * out + x, attention


# --------------------------------------------------------------------------- the GPU tests' inputs
# name: (B, C, H, W)
SHAPES = {
    "b1_c8_1x1": (1, 8, 1, 1),          # a single key, d = 1
    "b3_c16_6x6": (3, 16, 6, 6),        # below one tile, odd B, d = 2
    "b2_c64_8x8": (2, 64, 8, 8),        # one exact tile at the callers' C
    "b2_c32_10x10": (2, 32, 10, 10),    # N = 100: not a multiple of 16, 32 or 64
    "b1_c64_24x24": (1, 64, 24, 24),    # the 3 * 2^k plane family: several key tiles, ragged against 128
    "b2_c64_32x32": (2, 64, 32, 32),    # many key tiles, the smallest shipped plane
}
DIRECTED = ("late_max", "mask", "gamma0")
GAMMA = 0.7


def _random_params(C, gen, gamma=GAMMA):
    """x ~ N(0, 1) makes q, k ~ N(0, s^2 C) per component for N(0, s^2) weights, so a score (d terms) has
    standard deviation d^0.5 s^2 C: s is chosen for a score deviation of 2.  Value weights N(0, 1 / C)."""
    d = C // 8
    s = (2.0 / (d ** 0.5 * C)) ** 0.5
    return {
        "query_conv.weight": torch.randn(d, C, 1, 1, generator=gen) * s,
        "query_conv.bias": torch.randn(d, generator=gen) * 0.1,
        "key_conv.weight": torch.randn(d, C, 1, 1, generator=gen) * s,
        "key_conv.bias": torch.randn(d, generator=gen) * 0.1,
        "value_conv.weight": torch.randn(C, C, 1, 1, generator=gen) / C ** 0.5,
        "value_conv.bias": torch.randn(C, generator=gen) * 0.1,
        "gamma": torch.full((1,), gamma),
    }


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(x, p (state_dict, fp32), dy, ref (attn_ref), grads (attn_ref_backward)); computed once per
    process and never modified"""
    if name in SHAPES:
        B, C, H, W = SHAPES[name]
        gen = torch.Generator().manual_seed(100 + list(SHAPES).index(name))
        x = torch.randn(B, C, H, W, generator=gen)
        p = _random_params(C, gen)
        # |S| <= 12 comes first: a product of Gaussians has heavy tails, so over N^2 pairs the largest score
        # of the bigger planes passes 12 at a deviation of 2.  The query projection is shrunk to put the
        # largest at 11.5 there (deviation 1.2 at N = 1024, 1.5 at N = 576)
        smax = float(attn_ref(x, p)["S"].abs().max())
        if smax > 11.5:
            p["query_conv.weight"].mul_(11.5 / smax)
            p["query_conv.bias"].mul_(11.5 / smax)
    elif name == "late_max":
        # scores rise with the key index: x's channel 0 carries the ramp j / N, Wk reads it into k[0], and
        # bq makes q[0] about +8 for every query, so S[i, j] = 8 j / N + small: each row's largest score is
        # in the last key tile and every tile raises the running maximum
        B, C, H, W = 1, 64, 24, 24
        gen = torch.Generator().manual_seed(201)
        x = torch.randn(B, C, H, W, generator=gen) * 0.05
        x[:, 0] = (torch.arange(H * W, dtype=torch.float32) / (H * W)).reshape(H, W)
        p = _random_params(C, gen)
        for n in ("query_conv", "key_conv"):
            p[n + ".weight"].mul_(0.05)
            p[n + ".bias"].zero_()
        p["query_conv.bias"][0] = 8.0
        p["key_conv.weight"][0, 0, 0, 0] = 1.0
    elif name == "mask":
        # every real score is near -10 (bq = 10^0.5, bk = -10^0.5 on component 0, small weights): a padded
        # key left at score 0 would outweigh all N = 100 real keys together by e^10 / 100
        B, C, H, W = 2, 32, 10, 10
        gen = torch.Generator().manual_seed(202)
        x = torch.randn(B, C, H, W, generator=gen)
        p = _random_params(C, gen)
        for n in ("query_conv", "key_conv"):
            p[n + ".weight"].mul_(0.2)
            p[n + ".bias"].zero_()
        p["query_conv.bias"][0] = 10.0 ** 0.5
        p["key_conv.bias"][0] = -(10.0 ** 0.5)
    elif name == "gamma0":
        B, C, H, W = 2, 64, 8, 8
        gen = torch.Generator().manual_seed(203)
        x = torch.randn(B, C, H, W, generator=gen)
        p = _random_params(C, gen, gamma=0.0)
    else:
        raise KeyError(name)
    dy = torch.randn(x.shape, generator=gen)
    return dict(x=x, p=p, dy=dy, ref=attn_ref(x, p), grads=attn_ref_backward(x, p, dy))


# =========================================================================== the kernels themselves (C ABI)
# What follows serves tests/test_gpu_attn_abi.py (the five ffc_attn_* entry points called with raw pointers)
# and tests/test_attn_refs_cpu.py (which proves these references, inputs and measures without a GPU).  The
# entry points take q, k (B, d, N), v, x, dy (B, C, N) and a scalar gamma; there is no projection here.
TOL = 1e-5                 # the project's kernel-level bound
ROOM = 0.25                # plain fp32 on the CPU must stay inside this share of every bound
P_FLOOR = 2.0 ** -126      # the smallest normal fp32: __expf may flush below it what float64 keeps
GUARD = 64
CoreBwd = collections.namedtuple("CoreBwd", "dq dk dv dgamma D dq_scale dk_scale dgamma_scale dq_zero dk_zero")


def _d(t):
    return t.detach().cpu().double()


def core_ref(q, k, v, x, gamma):
    """-> y (B, C, N), L (B, N), o (B, C, N), P (B, N, N), S (B, N, N) in float64"""
    q, k, v = _d(q), _d(k), _d(v)
    S = torch.einsum("bri,brj->bij", q, k)
    L = torch.logsumexp(S, dim=-1)
    P = torch.softmax(S, dim=-1)
    o = torch.einsum("bcj,bij->bci", v, P)
    return float(gamma) * o + _d(x).reshape(o.shape), L, o, P, S


def core_bwd_ref(dy, q, k, v, gamma):
    """-> CoreBwd in float64: dq, dk (B, d, N), dv (B, C, N), dgamma (scalar), D (B, N) = sum_c do o with
    do = gamma dy, and the scales of the sums' cancellation: dq_scale[r, i] = sum_j |dS[i, j]| |k[r, j]|,
    dk_scale[r, j] = sum_i |dS[i, j]| |q[r, i]|, dgamma_scale = sum |dy o|.

    At N = 1 dS itself is exactly zero (P = 1 and dP = D), so dq_scale and dk_scale are zero with it: there
    the cancellation is the one inside dS = P (dP - D), a difference of two sums over c, and its scale is
    |dS|' = P (sum_c |do[c, i] v[c, j]| + sum_c |do[c, i] o[c, i]|).  dq_zero and dk_zero are dq_scale and
    dk_scale with |dS|' in place of |dS|; they bound what a result that is zero in mathematics may hold."""
    dy, q, k, v = _d(dy), _d(q), _d(k), _d(v)
    dy = dy.reshape(v.shape)
    g = float(gamma)
    _, _, o, P, _ = core_ref(q, k, v, torch.zeros_like(v), 0.0)
    do = g * dy
    D = (do * o).sum(1)
    dv = torch.einsum("bci,bij->bcj", do, P)
    dP = torch.einsum("bci,bcj->bij", do, v)
    dS = P * (dP - D[:, :, None])
    dq = torch.einsum("bij,brj->bri", dS, k)
    dk = torch.einsum("bij,bri->brj", dS, q)
    aS = dS.abs()
    aS0 = P * (torch.einsum("bci,bcj->bij", do.abs(), v.abs()) + (do * o).abs().sum(1)[:, :, None])
    return CoreBwd(dq, dk, dv, (dy * o).sum(), D,
                   torch.einsum("bij,brj->bri", aS, k.abs()), torch.einsum("bij,bri->brj", aS, q.abs()),
                   (dy * o).abs().sum(),
                   torch.einsum("bij,brj->bri", aS0, k.abs()), torch.einsum("bij,bri->brj", aS0, q.abs()))


def fma_f32(g, a, x):
    """fmaf(g, a, x) of float32 operands, exactly: the product of two float32 is exact in float64, the sum is
    rounded to odd in float64 (53 >= 2 * 24 + 2 bits) and then once to float32"""
    p = torch.as_tensor(g, dtype=torch.float32).double() * a.double()
    x = x.double().reshape(p.shape)
    s = p + x
    bb = s - p
    e = (p - (s - bb)) + (x - bb)                       # TwoSum: p + x = s + e exactly
    bits = s.contiguous().view(torch.int64).clone()
    fix = (e != 0) & (bits % 2 == 0) & torch.isfinite(s)
    step = torch.where((e > 0) == (s > 0), 1, -1)        # towards the exact sum
    bits[fix] += step[fix]
    return bits.view(torch.float64).float()


# --------------------------------------------------------------------------- inputs
# name: (B, C, H, W), one case per branch (the table is in tests/test_gpu_attn_abi.py's docstring)
ABI_RANDOM = {
    "1x8x1x1": (1, 8, 1, 1),
    "2x24x1x31": (2, 24, 1, 31),
    "1x32x32x1": (1, 32, 32, 1),
    "3x40x1x33": (3, 40, 1, 33),
    "2x64x6x6": (2, 64, 6, 6),
    "1x56x127x1": (1, 56, 127, 1),
    "2x32x1x128": (2, 32, 1, 128),
    "3x24x3x43": (3, 24, 3, 43),
    "1x40x1x255": (1, 40, 1, 255),
    "2x8x16x16": (2, 8, 16, 16),
    "1x64x257x1": (1, 64, 257, 1),
}
# The generator seeds.  From N = 127 on the first seed tried (300 + the case's index) left plain float32 at 0.28
# to 0.50 of the dq bound -- a peaked row's dS = P (dP - D) cancels, and the float32 rounding of a score near
# 11 moves it -- so those cases took the first seed of 300 + index + 100 t under 0.2: the input is changed,
# never the bound.
ABI_SEEDS = {"1x56x127x1": 605, "2x32x1x128": 1006, "3x24x3x43": 1607, "1x40x1x255": 908, "2x8x16x16": 509,
             "1x64x257x1": 3110}
ABI_DIRECTED = ("offset", "neg_offset", "early_max", "late_max", "one_hot", "uniform", "gamma_neg", "gamma_zero")
EXACT_SCORES = ("offset", "neg_offset", "early_max", "late_max", "one_hot", "uniform")
GRID_LIMIT = "65535x8x1x1"
ABI_ALL = tuple(ABI_RANDOM) + ABI_DIRECTED + (GRID_LIMIT,)
FORMS = ("2x64x6x6", "3x24x3x43")            # the cases that are run in every calling form
ONE_HOT_HIT, ONE_HOT_REST = 160.0, 120.0


def one_hot_perm(N=129):
    """a fixed permutation of the keys that crosses tiles and halves (37 is coprime to 129 = 3 * 43)"""
    return (torch.arange(N) * 37 + 5) % N


def _random_core(B, C, N, seed, gamma=GAMMA, nxn=True):
    """q, k ~ N(0, s^2) with s^2 = 2 / d^0.5 give a score (d terms) the deviation 2; then the rule of case():
    q is shrunk so that max |S| <= 11.5.  v, x, dy ~ N(0, 1)."""
    d = C // 8
    gen = torch.Generator().manual_seed(seed)
    s = (2.0 / d ** 0.5) ** 0.5
    q, k = torch.randn(B, d, N, generator=gen) * s, torch.randn(B, d, N, generator=gen) * s
    v, x, dy = (torch.randn(B, C, N, generator=gen) for _ in range(3))
    if nxn:
        smax = float(torch.einsum("bri,brj->bij", q.double(), k.double()).abs().max())
    else:                  # d = 1: the largest |q_i k_j| is the product of the largest factors
        assert d == 1
        smax = float((q.double().abs().amax(-1) * k.double().abs().amax(-1)).max())
    if smax > 11.5:
        q = q * (11.5 / smax * (1 - 2.0 ** -20))        # the float32 product may round up
    return dict(q=q, k=k, v=v, x=x, dy=dy, gamma=gamma)


def _directed_core(name):
    """Scores beyond +-12 are products of short mantissas (d = 1, or +-1 against +-20 over 8 components), so
    the float32 scores are the float64 scores and the bound tests the kernel, not float32 products."""
    if name == "gamma_neg":
        return (2, 32, 1, 33), _random_core(2, 32, 33, 402, gamma=-1.3)
    if name == "gamma_zero":
        return (2, 40, 5, 7), _random_core(2, 40, 35, 403, gamma=0.0)
    shape = {"offset": (2, 16, 6, 6), "neg_offset": (2, 16, 1, 33), "early_max": (1, 8, 257, 1),
             "late_max": (1, 8, 1, 257), "one_hot": (1, 64, 3, 43), "uniform": (2, 24, 3, 43)}[name]
    B, C, H, W = shape
    N, d = H * W, C // 8
    c = _random_core(B, C, N, 410 + EXACT_SCORES.index(name))
    i = torch.arange(N, dtype=torch.float32)
    b = torch.arange(B, dtype=torch.float32).reshape(B, 1, 1)
    if name in ("offset", "neg_offset"):
        # S[i, j] = +-100 + a_i b_j, a in quarters and b in eighths inside +-2: every score within 4 of +-100 and
        # exact in float32.  exp overflows float32 unless the running maximum is subtracted; at N = 33 the last
        # tile has 31 padded keys, and one left at score 0 outweighs everything at -100.  (With d = 1 a score
        # near 100 needs k_j = 100 / q_i (1 + a few percent), and dq = sum_j dS k_j then cancels thirtyfold:
        # plain float32 reached 4 to 7 times the dq bound on that input, so the offset sits on a component of
        # its own.)
        a = ((7 * i) % 17 - 8) * 0.25
        bb = ((5 * i + 3 * b) % 33 - 16) * 0.125
        sign = 1.0 if name == "offset" else -1.0
        # 100 = 100 * 1, not 10 * 10: dq[0, i] = k0 sum_j dS[i, j] is zero in mathematics, and its rounding
        # grows with k0 (plain float32 reached 1.7 times the dq bound at k0 = 10)
        c["q"] = torch.stack([torch.full((B, N), 100.0), a.expand(B, N)], 1)
        c["k"] = torch.cat([torch.full((B, 1, N), sign), bb.expand(B, 1, N)], 1)
    elif name == "early_max":
        # S[i, j] = -j / 2: the first tile holds every row's maximum, later tiles run alpha = 1 and their
        # exp underflows (from j = 175 on even the float32 subnormals)
        c["q"], c["k"] = torch.ones(B, 1, N), (-0.5 * i).reshape(1, 1, N).clone()
    elif name == "late_max":
        c["q"], c["k"] = torch.ones(B, 1, N), (0.5 * (i - (N - 1))).reshape(1, 1, N).clone()
    if name in ("early_max", "late_max"):
        # every row of P is the same here, so dv[c, j] = P[j] sum_i do[c, i]: with a zero-mean dy that one sum
        # of 257 terms cancels and plain float32 reached 0.37 of the dv bound; dy is given the mean 1
        c["dy"] = 1.0 + 0.5 * c["dy"]
    elif name == "one_hot":
        # A permutation matrix has rank N and S has rank d <= 8, so "40 at perm(i), 0 elsewhere" cannot be
        # formed.  With k[:, j] the 8 bits of j as +-1 and q[:, i] = 20 times the bits of perm(i),
        # S[i, j] = 160 - 40 hamming(perm(i), j): 160 at perm(i) and at most 120 anywhere else, so
        # o[:, i] is v[:, perm(i)] to about 8 e^-40
        bits = ((torch.arange(N)[None, :] >> torch.arange(d)[:, None]) & 1).float() * 2 - 1     # (8, N)
        c["k"] = bits.reshape(1, d, N).clone()
        c["q"] = (20.0 * bits[:, one_hot_perm(N)]).reshape(1, d, N).clone()
    elif name == "uniform":
        c["q"] = torch.zeros(B, d, N)
    return shape, c


@functools.lru_cache(maxsize=None)
def abi_case(name):
    """-> dict(shape (B, C, H, W), q, k, v, x, dy (float32), gamma, fwd = core_ref's y, L, o, P, S,
    bwd = core_bwd_ref's CoreBwd); computed once per process and never modified"""
    if name in ABI_RANDOM or name == GRID_LIMIT:
        shape = ABI_RANDOM.get(name, (65535, 8, 1, 1))
        B, C, H, W = shape
        c = _random_core(B, C, H * W, ABI_SEEDS.get(name, 300 + ABI_ALL.index(name)))
    elif name in ABI_DIRECTED:
        shape, c = _directed_core(name)
    else:
        raise KeyError(name)
    c["shape"], c["name"] = shape, name
    c["fwd"] = dict(zip("yLoPS", core_ref(c["q"], c["k"], c["v"], c["x"], c["gamma"])))
    c["bwd"] = core_bwd_ref(c["dy"], c["q"], c["k"], c["v"], c["gamma"])
    return c


def three_copies(name):
    """sample 0 of a case three times over (uncached: a few small tensors)"""
    c = abi_case(name)
    out = {k: c[k][:1].repeat(3, 1, 1) for k in ("q", "k", "v", "x", "dy")}
    out.update(gamma=c["gamma"], shape=(3,) + c["shape"][1:], name=name + " x3")
    return out


def one_sample(name, b):
    c = abi_case(name)
    out = {k: c[k][b:b + 1].clone() for k in ("q", "k", "v", "x", "dy")}
    out.update(gamma=c["gamma"], shape=(1,) + c["shape"][1:], name=f"{name}[{b}]")
    return out


LIMIT_SHAPE = (1, 8, 256, 256)


@functools.lru_cache(maxsize=None)
def limit_case():
    """N = 65536, forward only: float64 rows for the first tile, the last tile and 64 other fixed queries;
    nothing N x N is formed.  -> dict(q, k, v, x, gamma, rows (128 query indices), y (C, 128), L (128))"""
    B, C, H, W = LIMIT_SHAPE
    N = H * W
    c = _random_core(B, C, N, 499, nxn=False)
    rows = torch.cat([torch.arange(32), torch.arange(N - 32, N), (torch.arange(64) * 1021 + 77) % (N - 64) + 32])
    assert rows.unique().numel() == 128
    S = _d(c["q"])[0, 0, rows, None] * _d(c["k"])[0, 0, None, :]
    assert float(S.abs().max()) <= 11.5
    o = _d(c["v"])[0] @ torch.softmax(S, -1).T
    c.update(shape=LIMIT_SHAPE, rows=rows, L=torch.logsumexp(S, -1), o=o, y=c["gamma"] * o + _d(c["x"])[0][:, rows])
    return c


def limit_fp32(c):
    """the sampled rows of limit_case() in plain float32 -> dict(y, L)"""
    S = c["q"][0, 0, c["rows"], None] * c["k"][0, 0, None, :]
    o = c["v"][0] @ torch.softmax(S, -1).T
    return dict(y=c["gamma"] * o + c["x"][0][:, c["rows"]], L=torch.logsumexp(S, -1))


# --------------------------------------------------------------------------- the error measures
def _share(diff, lim):
    """largest |diff| / lim; where lim is 0 the result has to be exact"""
    r = torch.where(lim > 0, diff / lim.clamp_min(1e-300), torch.where(diff == 0, 0.0, float("inf")))
    return float(r.max())


def tensor_share(got, ref, over, floor=0.0):
    """y, o, dq, dk, dv (over = (1, 2): the sample's tensor) and P (over = (2,): the row): the largest
    |got - ref| / (TOL (|ref| + rms)), rms the root mean square of ref over ``over``"""
    got, ref = _d(got).reshape(ref.shape), ref.double()
    rms = ref.pow(2).mean(over, keepdim=True).sqrt()
    return _share((got - ref).abs(), (TOL * (ref.abs() + rms)).clamp_min(floor))


def L_share(got, ref):
    got = _d(got).reshape(ref.shape)
    return _share((got - ref).abs(), TOL * ref.abs().clamp_min(1.0))


def scale_share(got, ref, scale):
    """dgamma, D and results that are zero in mathematics: |got - ref| / (TOL scale), scale the sum of the
    absolute values of the terms that cancel"""
    got = _d(got).reshape(ref.shape)
    return _share((got - ref).abs(), TOL * scale.double().reshape(ref.shape))


def shares(c, got, p_floor=False):
    """{name: share of its bound} for whichever of y, L, o, P, dq, dk, dv, dgamma ``got`` holds, against
    case c's float64 results.  dq and dk are measured against dq_zero / dk_zero where they are zero in
    mathematics: at N = 1, and on the one-hot case (zero to e^-40: a one-hot softmax has no gradient)."""
    f, w = c["fwd"], c["bwd"]
    N = 1 if c.get("name") == "one_hot" else f["L"].shape[-1]
    out = {}
    for k in got:
        if k in ("y", "o"):
            out[k] = tensor_share(got[k], f[k], (1, 2))
        elif k == "P":
            out[k] = tensor_share(got[k], f["P"], (2,), P_FLOOR if p_floor else 0.0)
        elif k == "L":
            out[k] = L_share(got[k], f["L"])
        elif k in ("dq", "dk") and N == 1:
            out[k] = scale_share(got[k], getattr(w, k), getattr(w, k + "_zero"))
        elif k in ("dq", "dk", "dv"):
            out[k] = tensor_share(got[k], getattr(w, k), (1, 2))
        elif k == "dgamma":
            out[k] = scale_share(got[k], w.dgamma, w.dgamma_scale)
    return out


# --------------------------------------------------------------------------- float32 emulations
# Plain float32 on the CPU (torch matmul, softmax, logsumexp, the gradients from the formulas): what proves
# that an input leaves room under the bounds.  ``defect`` plants one mistake a kernel could make.
DEFECTS = {    # name: (case it is planted on, the results whose bound it has to exceed)
    "padded_key_at_score_0": ("neg_offset", ("y", "o", "L")),
    "last_key_tile_dropped": ("3x40x1x33", ("y", "o", "L")),
    "no_alpha_rescale_of_o": ("late_max", ("y", "o")),
    "l_from_one_half": ("2x64x6x6", ("y", "o", "L")),
    "D_left_out_of_dS": ("3x24x3x43", ("dq", "dk")),
    "gamma_twice_on_dk": ("3x24x3x43", ("dk",)),
    "sample_1_reads_sample_0_k": ("3x24x3x43", ("y", "o", "L", "P", "dq", "dk", "dv")),
    "o_column_from_neighbour_key": ("one_hot", ("y", "o")),
    "L_off_by_1e-4": ("2x64x6x6", ("L",)),
}
FLASH_DEFECTS = tuple(DEFECTS)[:4]


def fp32_forward(c, defect=None):
    q, k, v, x, g = c["q"], c["k"], c["v"], c["x"], c["gamma"]
    if defect == "sample_1_reads_sample_0_k":
        k = k.clone()
        k[1] = k[0]
    S = q.transpose(1, 2) @ k
    P = torch.softmax(S, -1)
    L = torch.logsumexp(S, -1)
    o = v @ P.transpose(1, 2)
    if defect == "o_column_from_neighbour_key":
        o = o.clone()
        o[0, :, 70] = v[0, :, (int(one_hot_perm(o.shape[-1])[70]) + 1) % o.shape[-1]]
    if defect == "L_off_by_1e-4":
        L = L + 1e-4
    return dict(y=g * o + x, L=L, o=o, P=P)


def fp32_backward(c, defect=None):
    q, k, v, dy, g = c["q"], c["k"], c["v"], c["dy"], c["gamma"]
    if defect == "sample_1_reads_sample_0_k":
        k = k.clone()
        k[1] = k[0]
    P = torch.softmax(q.transpose(1, 2) @ k, -1)
    o = v @ P.transpose(1, 2)
    do = g * dy
    D = (do * o).sum(1)
    dP = do.transpose(1, 2) @ v
    dS = P * dP if defect == "D_left_out_of_dS" else P * (dP - D[:, :, None])
    dk = q @ dS
    if defect == "gamma_twice_on_dk":
        dk = g * dk
    return dict(dq=k @ dS.transpose(1, 2), dk=dk, dv=do @ P, dgamma=(dy * o).sum())


def fp32_flash(c, defect=None):
    """the forward as the kernel walks it, in float32: key tiles of 32, a running maximum m, the sum l kept
    rescaled by alpha = exp(m_old - m_new), o rescaled with it -> dict(y, L, o)"""
    q, k, v, x, g = c["q"], c["k"], c["v"], c["x"], c["gamma"]
    B, C, N = v.shape
    m = torch.full((B, N), float("-inf"))
    l = torch.zeros(B, N)
    o = torch.zeros(B, C, N)
    tiles = list(range(0, N, 32))
    if defect == "last_key_tile_dropped":
        tiles = tiles[:-1]
    for j0 in tiles:
        j = torch.arange(j0, j0 + 32)
        jc = j.clamp_max(N - 1)
        S = q.transpose(1, 2) @ k[:, :, jc]                       # (B, N, 32)
        if defect == "padded_key_at_score_0":
            S[:, :, j >= N] = 0.0
        else:
            S[:, :, j >= N] = float("-inf")
        mn = torch.maximum(m, S.amax(-1))
        alpha = torch.exp(m - mn)
        p = torch.exp(S - mn[:, :, None])
        half0 = ((j - j0) // 4) % 2 == 0                          # rowkey(t, 0): keys 0-3, 8-11, ... of the tile
        l = l * alpha + (p[:, :, half0].sum(-1) if defect == "l_from_one_half" else p.sum(-1))
        if defect != "no_alpha_rescale_of_o":
            o = o * alpha[:, None, :]
        o = o + v[:, :, jc] @ p.transpose(1, 2)
        m = mn
    o = o / l[:, None, :]
    return dict(y=g * o + x, L=m + torch.log(l), o=o)
