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
