"""Inputs, float32 restatements and bounds of the wide Self_Attn kernels (72 <= C <= 256, ffc_attnw_*), shared
by tests/test_attn_wide_refs_cpu.py and tests/test_gpu_attn_wide.py.  The float64 references are those of
tests/attn_refs.py (attn_ref / attn_ref_backward for the layer, core_ref / core_bwd_ref for the entry points).

The bound of an output on an input comes from plain float32 on the CPU, never from the kernels: it is the
project's 1e-5 normwise (TOL_K) where the float32 restatement of the same formulas stays under a quarter of
it, and four times the restatement's own error where it does not (dP sums 256 channels here, four times the
64 of the narrow kernels).  Results that are zero in mathematics (the key bias's gradient; dq and dk at
N = 1, where a softmax over one key has no gradient) are measured against the scale of their cancellation.
"""
import functools

import torch

import attn_refs as R

TOL_K = 1e-5
ROOM = 0.25
CHANNELS = (72, 136, 256)        # d = 9 (odd, first past the narrow path, 8 rows in the second channel block), 17, 32
PLANES = ((1, 1), (4, 4), (3, 11), (10, 16))   # one key; the SAGAN critic's; N = 33: ragged, unaligned; N = 160
BATCHES = (1, 3)
SHAPES = {f"b{B}_c{C}_{H}x{W}": (B, C, H, W) for C in CHANNELS for H, W in PLANES for B in BATCHES}
# The first seed (700 + the case's index) gave b1_c72_4x4 a gamma gradient, sum dy o over 1152 terms, that cancels
# to a hundredth of its terms' scale: plain float32 missed TOL_K there (1.6e-5).  The input is changed, not the bound.
SEEDS = {"b1_c72_4x4": 802}
LAYER_OUTPUTS = ("out", "attention", "x") + R.NAMES
CORE_OUTPUTS = ("y", "L", "o", "P", "dq", "dk", "dv", "dgamma")


def _norm(t):
    return float(torch.linalg.vector_norm(t.detach().cpu().double().reshape(-1)))


def _against(got, ref, scale=None):
    """normwise error; against ``scale`` (the terms that cancel) where the reference is zero in mathematics"""
    diff = _norm(got.detach().cpu().double().reshape(-1) - ref.detach().cpu().double().reshape(-1))
    den = _norm(ref) if scale is None else _norm(scale)
    return diff / max(den, 1e-300)


# --------------------------------------------------------------------------- the layer
@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(x, p, dy, ref, grads, zero): as attn_refs.case, with attn_refs' rule max |S| <= 11.5; ``zero``
    holds the cancellation scales of the query / key gradients at N = 1 (None otherwise)"""
    B, C, H, W = SHAPES[name]
    gen = torch.Generator().manual_seed(SEEDS.get(name, 700 + list(SHAPES).index(name)))
    x = torch.randn(B, C, H, W, generator=gen)
    p = R._random_params(C, gen)
    smax = float(R.attn_ref(x, p)["S"].abs().max())
    if smax > 11.5:
        p["query_conv.weight"].mul_(11.5 / smax)
        p["query_conv.bias"].mul_(11.5 / smax)
    dy = torch.randn(x.shape, generator=gen)
    ref, grads = R.attn_ref(x, p), R.attn_ref_backward(x, p, dy)
    zero = None
    if H * W == 1:
        w = R.core_bwd_ref(dy.reshape(B, C, 1), ref["q"], ref["k"], ref["v"], float(p["gamma"]))
        ax = x.double().abs().reshape(B, C, 1)
        zero = {"query_conv.weight": torch.einsum("bmn,bcn->mc", w.dq_zero, ax), "query_conv.bias": w.dq_zero.sum((0, 2)),
                "key_conv.weight": torch.einsum("bmn,bcn->mc", w.dk_zero, ax), "key_conv.bias": w.dk_zero.sum((0, 2))}
    return dict(name=name, x=x, p=p, dy=dy, ref=ref, grads=grads, zero=zero)


def layer_errors(c, got):
    """{output: error} for whichever of LAYER_OUTPUTS ``got`` holds"""
    errs = {}
    for k, t in got.items():
        if k in ("out", "attention"):
            errs[k] = _against(t, c["ref"][k])
        elif k == "x":
            errs[k] = _against(t, c["grads"]["x"])
        elif c["zero"] is not None and k in c["zero"]:
            errs[k] = _against(t, c["grads"][k], c["zero"][k])
        else:
            errs[k] = R.grad_err(k, t, c["grads"])
    return errs


def fp32_core(q, k, v, dy, gamma, defect=None):
    """the formulas of attn_refs' docstring in plain float32 (no autograd, so that one mistake can be planted)
    -> dict(L, o, P, dq, dk, dv, dgamma)"""
    B, C, N = v.shape
    qs, ks = (q[:, :8], k[:, :8]) if defect == "d_truncated_to_8" else (q, k)
    S = qs.transpose(1, 2) @ ks
    if defect == "padded_key_in_the_sum":      # the 32 - N % 32 padded keys of the last tile at score 0
        pad = (-N) % 32
        assert pad > 0
        S = torch.cat([S, torch.zeros(B, N, pad)], -1)
    L = torch.logsumexp(S, -1)
    P = torch.exp(S - L[:, :, None])[:, :, :N]
    vv = v
    if defect == "channel_block_dropped":      # the last 32-row block of channels never accumulated
        vv = v.clone()
        vv[:, (C - 1) // 32 * 32:] = 0.0
    o = vv @ P.transpose(1, 2)
    do = gamma * dy
    D = (do * o).sum(1)
    dP = do[:, :64].transpose(1, 2) @ v[:, :64] if defect == "dP_over_64_channels" else do.transpose(1, 2) @ v
    dS = P * (dP - D[:, :, None])
    return dict(L=L, o=o, P=P, dq=k @ dS.transpose(1, 2), dk=q @ dS, dv=do @ P, dgamma=(dy * o).sum())


def fp32_layer(c, defect=None):
    """the whole layer in plain float32 from the formulas -> {output: tensor} over LAYER_OUTPUTS"""
    x, p, dy = c["x"], c["p"], c["dy"]
    B, C, H, W = x.shape
    xf, dyf = x.reshape(B, C, -1), dy.reshape(B, C, -1)

    def w2(n):
        return p[n + ".weight"].reshape(-1, C)

    q, k, v = (torch.einsum("mc,bcn->bmn", w2(n), xf) + p[n + ".bias"].reshape(1, -1, 1)
               for n in ("query_conv", "key_conv", "value_conv"))
    g = float(p["gamma"])
    r = fp32_core(q, k, v, dyf, g, defect)
    out = {"out": (g * r["o"] + xf).reshape(x.shape), "attention": r["P"], "gamma": r["dgamma"].reshape(1)}
    dx = dyf.clone()
    for n, dz in (("query_conv", r["dq"]), ("key_conv", r["dk"]), ("value_conv", r["dv"])):
        dx = dx + torch.einsum("mc,bmn->bcn", w2(n), dz)
        out[n + ".weight"] = torch.einsum("bmn,bcn->mc", dz, xf).reshape(p[n + ".weight"].shape)
        out[n + ".bias"] = dz.sum((0, 2))
    out["x"] = dx.reshape(x.shape)
    return out


def _bounds(errs):
    return {k: TOL_K if e <= ROOM * TOL_K else 4.0 * e for k, e in errs.items()}


@functools.lru_cache(maxsize=None)
def layer_fp32_errors(name):
    c = case(name)
    return layer_errors(c, fp32_layer(c))


def layer_bounds(name):
    """{output: bound} of case ``name``: TOL_K, or 4x the float32 restatement's error where that passes TOL_K / 4"""
    return _bounds(layer_fp32_errors(name))


# --------------------------------------------------------------------------- the entry points
# name: (B, C, H, W); q, k, v, x, dy given directly (attn_refs._random_core)
CORE_RANDOM = {"3x72x1x1": (3, 72, 1, 1), "1x72x3x11": (1, 72, 3, 11), "3x136x4x4": (3, 136, 4, 4),
               "1x136x10x16": (1, 136, 10, 16), "3x256x3x11": (3, 256, 3, 11), "3x256x10x16": (3, 256, 10, 16),
               "1x256x4x4": (1, 256, 4, 4)}
CORE_DIRECTED = {"offset": (3, 136, 10, 16), "neg_offset": (3, 256, 3, 11), "early_max": (1, 72, 10, 16),
                 "late_max": (1, 256, 10, 16), "gamma_zero": (3, 256, 3, 11)}
CORE_ALL = tuple(CORE_RANDOM) + tuple(CORE_DIRECTED)


@functools.lru_cache(maxsize=None)
def core_case(name):
    """-> as attn_refs.abi_case.  The directed scores follow attn_refs._directed_core with the structure on the
    first and the last of the d >= 9 components (the last is half h = 0 of an odd d's final k-step) and zeros
    between them, so that the float32 scores are exact: offset / neg_offset put every score within 4 of +-100, exact in float32 (N = 33 has 31
    padded keys in its last tile); early_max / late_max are S[i, j] = -j / 2 and (j - N + 1) / 2 over five key
    tiles, so the first or the last tile holds every row's maximum."""
    shape = CORE_RANDOM.get(name) or CORE_DIRECTED[name]
    B, C, H, W = shape
    N, d = H * W, C // 8
    c = R._random_core(B, C, N, 800 + CORE_ALL.index(name), gamma=0.0 if name == "gamma_zero" else R.GAMMA)
    i = torch.arange(N, dtype=torch.float32)
    b = torch.arange(B, dtype=torch.float32).reshape(B, 1, 1)
    if name in ("offset", "neg_offset"):
        a = ((7 * i) % 17 - 8) * 0.25
        bb = ((5 * i + 3 * b) % 33 - 16) * 0.125
        q, k = torch.zeros(B, d, N), torch.zeros(B, d, N)
        q[:, 0], k[:, 0] = 100.0, 1.0 if name == "offset" else -1.0
        q[:, d - 1], k[:, d - 1] = a.expand(B, N), bb.reshape(B, N)     # the last component: the odd k-step's half
        c["q"], c["k"] = q, k
    elif name in ("early_max", "late_max"):
        q, k = torch.zeros(B, d, N), torch.zeros(B, d, N)
        q[:, d - 1] = 1.0
        k[:, d - 1] = -0.5 * i if name == "early_max" else 0.5 * (i - (N - 1))
        c["q"], c["k"] = q, k
        c["dy"] = 1.0 + 0.5 * c["dy"]          # attn_refs._directed_core: a zero-mean dy cancels in dv here
    c["shape"], c["name"] = shape, name
    c["fwd"] = dict(zip("yLoPS", R.core_ref(c["q"], c["k"], c["v"], c["x"], c["gamma"])))
    c["bwd"] = R.core_bwd_ref(c["dy"], c["q"], c["k"], c["v"], c["gamma"])
    return c


def core_errors(c, got):
    """{output: normwise error} for whichever of CORE_OUTPUTS ``got`` holds; dq and dk against their
    cancellation scale at N = 1, dgamma against sum |dy o|"""
    f, w = c["fwd"], c["bwd"]
    errs = {}
    for k, t in got.items():
        if k in ("y", "L", "o", "P"):
            errs[k] = _against(t, f[k])
        elif k in ("dq", "dk") and f["L"].shape[-1] == 1:
            errs[k] = _against(t, getattr(w, k), getattr(w, k + "_zero"))
        elif k == "dgamma":
            errs[k] = _against(t, w.dgamma, w.dgamma_scale)
        elif k in ("dq", "dk", "dv"):
            errs[k] = _against(t, getattr(w, k))
    return errs


def fp32_core_case(c, defect=None):
    r = fp32_core(c["q"], c["k"], c["v"], c["dy"], c["gamma"], defect)
    r["y"] = c["gamma"] * r["o"] + c["x"]
    return r


@functools.lru_cache(maxsize=None)
def core_fp32_errors(name):
    c = core_case(name)
    return core_errors(c, {k: v for k, v in fp32_core_case(c).items() if k in CORE_OUTPUTS})


def core_bounds(name):
    return _bounds(core_fp32_errors(name))


# name: (core case it is planted on, the outputs whose bound it has to exceed)
DEFECTS = {
    "channel_block_dropped": ("3x72x1x1", ("y", "o")),
    "d_truncated_to_8": ("3x136x4x4", ("y", "o", "L", "P", "dq", "dk", "dv")),
    "padded_key_in_the_sum": ("neg_offset", ("y", "o", "L", "P")),
    "dP_over_64_channels": ("3x256x10x16", ("dq", "dk")),
}
