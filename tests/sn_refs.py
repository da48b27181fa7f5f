"""float64 restatement of torch.nn.utils.spectral_norm's pre-hook (SpectralNorm.compute_weight, one
power iteration) and of its derivative, the reference of tests/test_sn_cpu.py and tests/test_gpu_sn.py.

With the weight seen as a matrix Wm (M x K) over ``dim`` (SpectralNorm.reshape_weight_to_matrix) and
normalize(x) = x / max(||x||_2, eps):
    training:  v <- normalize(Wm^T u),  u <- normalize(Wm v)
    sigma = u . (Wm v),  W = W_orig / sigma
u and v are constants for autograd, so
    dW_orig = dW / sigma - (<dW, W_orig> / sigma^2) * u v^T     (u v^T folded back into W's layout)
"""
import torch


def to_matrix(w, dim):
    """SpectralNorm.reshape_weight_to_matrix"""
    if dim != 0:
        w = w.permute(dim, *[d for d in range(w.dim()) if d != dim])
    return w.reshape(w.size(0), -1)


def from_matrix(m, shape, dim):
    """the inverse of to_matrix for a weight of ``shape``"""
    shape = tuple(shape)
    if dim == 0:
        return m.reshape(shape)
    order = [dim] + [d for d in range(len(shape)) if d != dim]
    inv = [order.index(d) for d in range(len(shape))]
    return m.reshape([shape[d] for d in order]).permute(*inv)


def _normalize(x, eps):
    return x / torch.clamp(torch.linalg.vector_norm(x), min=eps)


def sn_ref(w_orig, u, v, dim, training, eps=1e-12):
    """-> (w, u', v', sigma) in float64"""
    w64, u, v = w_orig.detach().double(), u.detach().double(), v.detach().double()
    wm = to_matrix(w64, dim)
    if training:
        v = _normalize(wm.t() @ u, eps)
        u = _normalize(wm @ v, eps)
    sigma = torch.dot(u, wm @ v)
    return w64 / sigma, u, v, sigma


def sn_ref_backward(dw, w_orig, u, v, sigma, dim=0):
    """-> dW_orig in float64, (u, v, sigma) as returned by sn_ref for the same call"""
    dw, w64 = dw.detach().double(), w_orig.detach().double()
    sigma = torch.as_tensor(sigma, dtype=torch.float64)
    dot = (dw * w64).sum()
    uv = from_matrix(torch.outer(u.double(), v.double()), w64.shape, dim)
    return dw / sigma - (dot / sigma ** 2) * uv


def normwise(out, ref):
    out, ref = out.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    return float(torch.linalg.vector_norm(out - ref) / torch.clamp(torch.linalg.vector_norm(ref), min=1e-300))


def sn_hook(mod):
    from torch.nn.utils.spectral_norm import SpectralNorm
    return next(h for h in mod._forward_pre_hooks.values() if isinstance(h, SpectralNorm))


def run_hook(mod):
    """what calling the module does before its forward: -> (weight, weight_u, weight_v) after the hook"""
    sn_hook(mod)(mod, None)
    return mod.weight, mod.weight_u, mod.weight_v


# ============================================================================ the C ABI tests
# (tests/test_sn_refs_cpu.py, tests/test_gpu_sn_abi.py): the cases, elementwise bounds of the form
# TOL * scale with scale the float64 sum of the absolute terms of the quantity, and a plain fp32
# restatement of csrc/sn_kernels.hip's arithmetic (its index maps, tiles and chunks; numpy's own
# summation order inside a tile) with the defects test_sn_refs_cpu.py plants.
import functools  # noqa: E402

import numpy as np  # noqa: E402

TOL = 1e-5       # the smallest power of ten that keeps sn_f32 under a quarter of every bound (test_sn_refs_cpu.py)
EPS = np.float32(1e-12)
RA, RB, CB, EC, MAX_JOBS = 64, 16, 2048, 16384, 16   # tile constants of sn_kernels.hip

# name: (weight shape, dim) -> (M, K, R)
ABI_CASES = {
    "T5x7x3x3": ((5, 7, 3, 3), 1),       # 7, 45, 9: the smallest dim-1 scalar form
    "T66x3x3x3": ((66, 3, 3, 3), 1),     # 3, 594, 9: the head's shape class
    "T19x65x3x3": ((19, 65, 3, 3), 1),   # 65, 171, 9: two row chunks, M K % 4 != 0
    "T8x20x2x2": ((8, 20, 2, 2), 1),     # 20, 32, 4: the smallest dim-1 vector form
    "17x64": ((17, 64), 0), "16x65": ((16, 65), 0), "65x256": ((65, 256), 0), "64x260": ((64, 260), 0),
    "257x64": ((257, 64), 0),
    "1000x3": ((1000, 3), 0), "3x1000": ((3, 1000), 0),
    "8x2048": ((8, 2048), 0), "8x2049": ((8, 2049), 0), "8x2052": ((8, 2052), 0),
    "127x129": ((127, 129), 0), "128x128": ((128, 128), 0), "1x16385": ((1, 16385), 0), "4x4097": ((4, 4097), 0),
    "1x1": ((1, 1), 0), "1x4": ((1, 4), 0), "4x1": ((4, 1), 0),
}
ABI_NAMES = list(ABI_CASES)
FORMS = ("T19x65x3x3", "T8x20x2x2", "64x260")
LAMBDAS = (0.0, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0, 512.0, 1024.0)


def view(shape, dim):
    """(M, K, R, stride_m, stride_i) of include/ffc_amd.h's matrix view for a dense weight"""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    if dim == 0:
        M = shape[0]
        return M, n // M, n // M, n // M, 0
    assert dim == 1
    M = shape[1]
    R = n // (shape[0] * M)
    return M, shape[0] * R, R, R, M * R


def elem_index(M, K, R, stride_i):
    """(M, K) int64: the element of w_orig's storage that is Wm[m][k] (the header's formula; sn_col)"""
    k = np.arange(K)
    col = k if R == K else (k // R) * stride_i + k % R
    return col[None, :] + np.arange(M)[:, None] * (K if R == K else R)


def mk_index(M, K, R, stride_i):
    """(m, k) of every storage element e, the inverse of elem_index (sn_mk)"""
    e = np.arange(M * K)
    if R == K:
        return e // K, e % K
    i, rem = e // stride_i, e % stride_i
    m = rem // R
    return m, i * R + rem % R


def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)


def _f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)


def rank_ratio(g, w, u, v, sigma, dim):
    """median over elements of |c u_m v_k| / |g / sigma|, c = <g, w> / sigma^2, in float64"""
    g, w = _f64(g), _f64(w)
    M, K, R, _, si = view(w.shape, dim)
    m, k = mk_index(M, K, R, si)
    c = float((g * w).sum()) / float(sigma) ** 2
    return float(np.median(np.abs(c * _f64(u)[m] * _f64(v)[k]) / np.abs(g.reshape(-1) / float(sigma))))


def make_case(name, shape, dim, w=None, u=None, seed=None, scale=0.02):
    """fp32 inputs on the CPU and the float64 results; g = noise + lambda w with the smallest lambda of
    LAMBDAS at which the rank-one term's median share of dw / sigma is at least 0.1"""
    gen = torch.Generator().manual_seed(1000 + (ABI_NAMES.index(name) if seed is None else seed))
    M, K, R, sm, si = view(shape, dim)
    if w is None:
        w = torch.randn(shape, generator=gen) * scale
    if u is None:
        u = torch.nn.functional.normalize(torch.randn(M, generator=gen), dim=0, eps=1e-12)
    v = torch.nn.functional.normalize(torch.randn(K, generator=gen), dim=0, eps=1e-12)
    noise = torch.randn(shape, generator=gen)
    train, ev = sn_ref(w, u, v, dim, True), sn_ref(w, u, v, dim, False)
    for lam in LAMBDAS:
        g = noise + lam * w
        ratio = rank_ratio(g, w, train[1], train[2], train[3], dim)
        if ratio >= 0.1:
            break
    return dict(name=name, shape=tuple(shape), dim=dim, M=M, K=K, R=R, stride_m=sm, stride_i=si, w=w, u=u, v=v, g=g,
                lam=lam, ratio=ratio, train=train, eval=ev)


@functools.lru_cache(maxsize=None)
def abi_case(name):
    return make_case(name, *ABI_CASES[name])


def _wm64(c):
    return _f64(c["w"]).reshape(-1)[elem_index(c["M"], c["K"], c["R"], c["stride_i"])]


def _share(got, ref, scale):
    """max |got - ref| / (TOL scale); a zero scale admits only an exact result"""
    got, ref, scale = _f64(got).reshape(-1), _f64(ref).reshape(-1), np.broadcast_to(_f64(scale), _f64(ref).shape).reshape(-1)
    err = np.abs(got - ref)
    if not np.isfinite(err).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(err == 0, 0.0, err / (TOL * scale))
    return float(s.max()) if s.size else 0.0


def forward_shares(c, got, training):
    """shares of the bounds for a forward's results.  got: sigma, and in training mode u, v (this call's),
    p (the sum of the pa partials) and tb (the sum of the pb partials: Wm p, not yet divided); in eval
    mode tb = Wm v.  W is not here: see w_exact."""
    Wm, aW = _wm64(c), np.abs(_wm64(c))
    out = {}
    if training:
        _, ru, rv, rs = (_f64(x) for x in c["train"])
        u0 = _f64(c["u"])
        p_ref, p_scale = Wm.T @ u0, aW.T @ np.abs(u0)
        out["p"] = _share(got["p"], p_ref, p_scale)
        pg = _f64(got["p"])
        out["t"] = _share(got["tb"], Wm @ pg, aW @ np.abs(pg))
        out["v"] = _share(got["v"], rv, p_scale / np.linalg.norm(p_ref))
        t_ref = Wm @ rv
        out["u"] = _share(got["u"], ru, (aW @ np.abs(rv)) / np.linalg.norm(t_ref))
        out["sigma"] = _share(got["sigma"], rs, float(np.abs(ru * t_ref).sum()))
    else:
        u0, v0 = _f64(c["u"]), _f64(c["v"])
        t_ref = Wm @ v0
        out["t"] = _share(got["tb"], t_ref, aW @ np.abs(v0))
        out["sigma"] = _share(got["sigma"], _f64(c["eval"][3]), float(np.abs(u0 * t_ref).sum()))
    return out


def w_exact(c, w_got, sigma_got):
    """number of elements of W that are not fl(w_orig / sigma_got), the correctly rounded fp32 quotient"""
    want = _f32(c["w"]) / np.float32(_f32(sigma_got).reshape(-1)[0])
    return int((_f32(w_got).reshape(want.shape).view(np.int32) != want.view(np.int32)).sum())


def backward_shares(c, dw_orig, u, v, sigma):
    """dw_orig against float64 at the (u, v, sigma) the forward under test produced ("own"), scale
    |dw / sigma| + |c u_m v_k|, and against float64 throughout ("e2e").  End to end the forward's errors
    come along: u'_m and v'_k are known to TOL times their own scales su_m, sv_k (forward_shares), which
    exceed |u'_m|, |v'_k| where the sums cancel, so that scale is |dw / sigma| + |c| su_m sv_k."""
    out = {}
    m, k = mk_index(c["M"], c["K"], c["R"], c["stride_i"])
    g, w = _f64(c["g"]).reshape(-1), _f64(c["w"]).reshape(-1)
    Wm, aW = _wm64(c), np.abs(_wm64(c))
    _, ru, rv, rs = (_f64(x) for x in c["train"])
    su = (aW @ np.abs(rv)) / np.linalg.norm(Wm @ rv)
    sv = (aW.T @ np.abs(_f64(c["u"]))) / np.linalg.norm(Wm.T @ _f64(c["u"]))
    for key, (uu, vv, ss) in (("own", (u, v, sigma)), ("e2e", (ru, rv, rs))):
        uu, vv, ss = _f64(uu), _f64(vv), float(_f64(ss).reshape(-1)[0])
        if not (np.isfinite(ss) and ss != 0.0):
            out["dw_" + key] = float("inf")
            continue
        coef = float((g * w).sum()) / ss ** 2
        rank = coef * uu[m] * vv[k]
        scale = np.abs(g / ss) + (np.abs(rank) if key == "own" else abs(coef) * su[m] * sv[k])
        out["dw_" + key] = _share(dw_orig, g / ss - rank, scale)
    return out


# ---------------------------------------------------------------------------- plain fp32
SN_DEFECTS = ("col_ignores_stride_i", "chunk_last_unscaled", "drop_last_pa", "psq_short", "drop_last_pb", "nv_twice",
              "eval_refreshed_u")
SN_BWD_DEFECTS = ("mk_swapped", "u_next_last_row", "pdot_short", "coef_sigma_once")


def _tiles(n, size):
    return [slice(a, min(n, a + size)) for a in range(0, n, size)]


def sn_f32(c, training, defect=None):
    """the forward of sn_kernels.hip in plain fp32 (fp64 where the kernels merge in fp64)
    -> dict(p, tb, u, v, sigma, w) as float32 arrays"""
    f32, f64 = np.float32, np.float64
    M, K, R, si = c["M"], c["K"], c["R"], c["stride_i"]
    flat, u0, v0 = _f32(c["w"]).reshape(-1), _f32(c["u"]), _f32(c["v"])
    idx = elem_index(M, K, R, si)
    if defect == "col_ignores_stride_i" and R != K:
        idx = np.arange(K)[None, :] + np.arange(M)[:, None] * R
    Wm = flat[idx]
    nv = f32(1.0)
    if training:
        pa = np.stack([(Wm[r] * u0[r, None]).sum(0, dtype=f32) for r in _tiles(M, RA)])
        if defect == "drop_last_pa":
            pa[-1] = 0
        p = pa.astype(f64).sum(0).astype(f32)
        psq = [float((p[s].astype(f64) ** 2).sum()) for s in _tiles(K, CB)]
        if defect == "psq_short":
            psq = psq[:-1]
        nv = max(f32(np.sqrt(f64(sum(psq)))), EPS)
    else:
        p = v0
    pb = np.stack([(Wm[:, s] * p[None, s]).sum(1, dtype=f32) for s in _tiles(K, CB)])
    if defect == "drop_last_pb":
        pb[-1] = 0
    tb = pb.astype(f64).sum(0).astype(f32)
    t = tb / nv if training else tb
    if defect == "nv_twice" and training:
        t = t / nv
    nt = max(f32(np.sqrt((t.astype(f64) ** 2).sum())), EPS)
    if training:
        un, vn = t / nt, p / nv
    else:
        un, vn = (t / nt if defect == "eval_refreshed_u" else u0), v0
    sigma = f32((un.astype(f64) * t.astype(f64)).sum())
    w = flat / sigma
    if defect == "chunk_last_unscaled":
        for s in _tiles(M * K, EC):
            w[s.stop - 1] = flat[s.stop - 1]
    return dict(p=p, tb=tb, u=un, v=vn, sigma=np.array([sigma], dtype=f32), w=w.reshape(c["shape"]))


def sn_bwd_f32(c, u, v, sigma, defect=None):
    """the backward of sn_kernels.hip at (u, v, sigma) -> dw_orig, float32"""
    f32, f64 = np.float32, np.float64
    M, K, R, si = c["M"], c["K"], c["R"], c["stride_i"]
    g, flat = _f32(c["g"]).reshape(-1), _f32(c["w"]).reshape(-1)
    u, v, sigma = _f32(u), _f32(v), f32(_f32(sigma).reshape(-1)[0])
    pdot = [float((g[s].astype(f64) * flat[s].astype(f64)).sum()) for s in _tiles(M * K, EC)]
    if defect == "pdot_short":
        pdot = pdot[:-1]
    dot = f64(sum(pdot))
    inv = f32(1.0) / sigma
    coef = f32(dot / f64(sigma)) if defect == "coef_sigma_once" else f32(dot / (f64(sigma) * f64(sigma)))
    m, k = mk_index(M, K, R, si)
    if defect == "mk_swapped" and R != K:
        m, k = k % M, m % K
    um = u[m]
    if defect == "u_next_last_row":   # what lies behind u: taken as 0
        um = np.concatenate([u, np.zeros(1, f32)])[np.where(m == M - 1, M, m)]
    cu = -(coef * um)
    out = (cu.astype(f64) * v[k].astype(f64) + (g * inv).astype(f64)).astype(f32)   # fmaf
    return out.reshape(c["shape"])


def rank_one_case():
    """w_orig = a b^T (fp32 products), u parallel to a: one iteration is at the fixed point"""
    gen = torch.Generator().manual_seed(77)
    a, b = torch.randn(33, generator=gen), torch.randn(70, generator=gen) * 0.02
    w = torch.outer(a, b)
    c = make_case("rank_one", (33, 70), 0, w=w, u=torch.nn.functional.normalize(a, dim=0), seed=77)
    c["a"], c["b"] = a, b
    return c


def scaled_case(e):
    """the 64x260 weights at unit variance times 2^e (exact): at 2^-40 ||Wm^T u|| and ||Wm v|| stay above the
    1e-12 of normalize(), which N(0, 0.02) weights would not (about 3e-13), so no clamp breaks the scaling"""
    base = make_case("scaled", (64, 260), 0, seed=78, scale=1.0)
    return make_case("scaled", (64, 260), 0, w=base["w"] * 2.0 ** e, u=base["u"], seed=78)
