"""float64 restatement of the SAGAN baseline (benchmark_models/sagan/: spectral.py, sagan_models.py at
image_size = 32, the hinge losses of trainer.py:93-168), functional over a state dict, and the deterministic
``fill`` every SAGAN test seeds its models with.  The models cannot be shrunk (the attention widths are hard-coded)
and 1.1 M weights do not belong in a fixture, so the fixtures under tests/golden/sagan/ hold inputs and results only;
the weights come from ``fill`` on both sides.

State dicts here are {key: tensor} with the reference's keys.  ``dtype`` float64 gives the reference, float32 the
plain single-precision evaluation of the same formulas whose error the GPU bounds are derived from
(tests/test_sagan_refs_cpu.py prints it)."""
import os

import numpy as np
import torch
import torch.nn.functional as tF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sagan")
Z_DIM = 128
EPS = 1e-12
STRIDE = 97          # weight-gradient digests keep every 97th element
P2_ROWS = 8          # the generator's attention matrix is recorded at every 8th row, plus its column sums
G_SN = ("l1.0", "l2.0", "l3.0")
D_SN = ("l1.0", "l2.0", "l3.0")
GAMMA = {"attn1.gamma": 0.5, "attn2.gamma": -0.3}
GAMMA_COND = {}      # self_attn's note of the last backward through each attention layer


# --------------------------------------------------------------------------- fill
def fill(sd, seed):
    """writes every tensor of ``sd`` (a model's state_dict: the writes land in the model) from one
    numpy RandomState(seed), in key order.  Every value is a float32 number, so float64 and float32 models hold
    the same weights.  weight_u / weight_v: unit vectors; gamma: 0.5 (attn1), -0.3 (attn2); BatchNorm weight
    1 + 0.1 n, running_var in [0.5, 1.5); num_batches_tracked 0; biases and running_mean 0.1 n; every other weight
    n / sqrt(numel / shape[0])."""
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for k, t in sd.items():
            if k.endswith("num_batches_tracked"):
                t.zero_()
                continue
            n = rs.standard_normal(tuple(t.shape))
            if k in GAMMA:
                x = np.full(tuple(t.shape), GAMMA[k])
            elif k.endswith(("weight_u", "weight_v")):
                x = n / np.sqrt((n * n).sum())
            elif k.endswith("running_var"):
                x = 0.5 + rs.random_sample(tuple(t.shape))
            elif k.endswith(("bias", "running_mean")):
                x = 0.1 * n
            elif t.dim() == 1:
                x = 1.0 + 0.1 * n
            else:
                x = n / np.sqrt(t.numel() / t.shape[0])
            t.copy_(torch.from_numpy(x.astype(np.float32)).to(t.dtype))
    return sd


def inputs(B, seed=0):
    """(z_g, z_d, real) of a fixture: float32 numbers as float64 tensors"""
    rs = np.random.RandomState(1000 + 10 * seed + B)
    mk = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).double()
    return mk(B, Z_DIM), mk(B, Z_DIM), torch.tanh(mk(B, 3, 32, 32)).float().double()


def cast(sd, dtype):
    return {k: (v.detach().to(dtype) if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}


# --------------------------------------------------------------------------- the wrapper
def l2n_add(x):
    return x / (x.norm() + EPS)


def l2n_max(x):
    """the hook form's normalize (torch.nn.functional.normalize): NOT what the wrapper does"""
    return x / x.norm().clamp_min(EPS)


def sn_refresh(w_bar, u, v, normalize=l2n_add):
    """one call of the wrapper: -> (W, u', v', sigma); the gradient flows through w_bar in sigma's W only"""
    Wm = w_bar.reshape(w_bar.shape[0], -1)
    with torch.no_grad():
        v = normalize(Wm.t().mv(u))
        u = normalize(Wm.mv(v))
    sigma = u.dot(Wm.mv(v))
    return w_bar / sigma, u, v, sigma


def sn_backward(dw, w_bar, u, v, sigma):
    """dw_bar of W = w_bar / sigma, sigma = u^T Wm v, u and v constants"""
    c = (dw * w_bar).sum() / (sigma * sigma)
    return dw / sigma - c * torch.outer(u, v).reshape(w_bar.shape)


def _sn(sd, pre, new):
    """the wrapper inside a model: sd's u and v tensors are the reference's Parameters -- the graph holds them, and
    every call replaces their ``.data`` (spectral.py:30-34), so a backward that runs after a later call takes its
    rank-one term from that call's vectors.  ``new`` gets copies of this call's."""
    U, V, w_bar = sd[pre + ".module.weight_u"], sd[pre + ".module.weight_v"], sd[pre + ".module.weight_bar"]
    Wm = w_bar.reshape(w_bar.shape[0], -1)
    with torch.no_grad():
        V.data = l2n_add(Wm.t().mv(U))
        U.data = l2n_add(Wm.mv(V))
    sigma = U.dot(Wm.mv(V))
    new[pre + ".module.weight_u"], new[pre + ".module.weight_v"] = U.detach().clone(), V.detach().clone()
    return w_bar / sigma, sd[pre + ".module.bias"]


# --------------------------------------------------------------------------- layers
def batch_norm(x, sd, pre, new, training, eps=1e-5, momentum=0.1):
    if training:
        mean = x.mean((0, 2, 3))
        var = ((x - mean[None, :, None, None]) ** 2).mean((0, 2, 3))
        n = x.numel() // x.shape[1]
        with torch.no_grad():
            new[pre + ".running_mean"] = (1 - momentum) * sd[pre + ".running_mean"] + momentum * mean
            new[pre + ".running_var"] = (1 - momentum) * sd[pre + ".running_var"] + momentum * var * n / (n - 1)
            new[pre + ".num_batches_tracked"] = sd[pre + ".num_batches_tracked"] + 1
    else:
        mean, var = sd[pre + ".running_mean"], sd[pre + ".running_var"]
    xh = (x - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps)
    return xh * sd[pre + ".weight"][None, :, None, None] + sd[pre + ".bias"][None, :, None, None]


def self_attn(x, sd, pre):
    """-> (gamma * (value . attention^T) + x, attention (B, N, N)), attention[b, i, :] = softmax_j(q_i . k_j)"""
    B, C, H, W = x.shape
    proj = lambda name: tF.conv2d(x, sd[f"{pre}.{name}.weight"], sd[f"{pre}.{name}.bias"]).reshape(B, -1, H * W)
    q, k, val = proj("query_conv"), proj("key_conv"), proj("value_conv")
    att = torch.softmax(torch.einsum("bri,brj->bij", q, k), dim=-1)
    o = torch.einsum("bcj,bij->bci", val, att).reshape(B, C, H, W)
    out = sd[pre + ".gamma"] * o + x
    if out.requires_grad:      # gamma's gradient is <dy, o>: keep its condition number ||dy|| ||o|| / |<dy, o>|
        def note(dy, o=o.detach()):
            GAMMA_COND[pre] = float(dy.norm() * o.norm() / (dy * o).sum().abs())
        out.register_hook(note)
    return out, att


def generator(sd, z, training=True):
    """-> (img float, p2, new): ``new`` holds what the forward changes (u, v of every wrapper; BN statistics)"""
    new = {}
    x = z.reshape(z.shape[0], -1, 1, 1)
    for pre, geom in (("l1", (1, 0)), ("l2", (2, 1)), ("l3", (2, 1))):
        w, b = _sn(sd, pre + ".0", new)
        x = tF.conv_transpose2d(x, w, b, stride=geom[0], padding=geom[1])
        x = torch.relu(batch_norm(x, sd, pre + ".1", new, training))
    x, p2 = self_attn(x, sd, "attn2")
    img = torch.tanh(tF.conv_transpose2d(x, sd["last.0.weight"], sd["last.0.bias"], stride=2, padding=1))
    return img, p2, new


def quantize(img):
    """the eval-mode output: uint8(255 * (img * 0.5 + 0.5)), truncating"""
    return (255 * (img * 0.5 + 0.5)).to(torch.uint8)


def discriminator(sd, x):
    """-> (out squeezed, p1, new)"""
    new = {}
    for pre in ("l1", "l2", "l3"):
        w, b = _sn(sd, pre + ".0", new)
        x = tF.leaky_relu(tF.conv2d(x, w, b, stride=2, padding=1), 0.1)
    x, p1 = self_attn(x, sd, "attn1")
    out = tF.conv2d(x, sd["last.0.weight"], sd["last.0.bias"])
    return out.squeeze(), p1, new


def advance(sd, new):
    """sd with the BatchNorm statistics a forward left (u and v are advanced in place by the forward itself)"""
    out = dict(sd)
    out.update({k: v for k, v in new.items() if not k.endswith(("weight_u", "weight_v"))})
    return out


def d_losses(d_real, d_fake):
    return torch.relu(1.0 - d_real).mean(), torch.relu(1.0 + d_fake).mean()


def g_loss(d_fake):
    return -d_fake.mean()


def leaves(sd):
    """the state dict with every trained tensor a fresh leaf that records gradients"""
    skip = ("weight_u", "weight_v", "running_mean", "running_var", "num_batches_tracked")
    return {k: (v.detach().clone().requires_grad_(True) if not k.endswith(skip) else v.detach().clone())
            for k, v in sd.items()}


def trained(sd):
    skip = ("weight_u", "weight_v", "running_mean", "running_var", "num_batches_tracked")
    return [k for k in sd if not k.endswith(skip)]


# --------------------------------------------------------------------------- the two recorded scenarios
def scenario_g(gsd, dsd, z):
    """from the fill state: img, p2 = G(z); out, p1 = D(img); g_loss.backward() -> results, G's gradients"""
    g, d = leaves(gsd), leaves(dsd)
    img, p2, gnew = generator(g, z)
    out, p1, dnew = discriminator(d, img)
    loss = g_loss(out)
    loss.backward()
    res = dict(img=img.detach(), p2=p2.detach(), d_out=out.detach(), p1=p1.detach(), g_loss=loss.detach())
    res.update({"G." + k: v for k, v in gnew.items()})
    res.update({"D." + k: v for k, v in dnew.items()})
    grads = {k: g[k].grad for k in trained(g) if g[k].grad is not None}
    return res, grads


def scenario_d(gsd, dsd, z, real):
    """from the fill state: d_real = D(real); d_fake = D(G(z)) with G's graph cut; d_loss.backward() -> results,
    D's gradients; D's u, v after its two forwards"""
    d = leaves(dsd)
    with torch.no_grad():
        img, _, _ = generator(gsd, z)
    o_real, _, _ = discriminator(d, real)
    o_fake, _, new2 = discriminator(d, img)      # u, v advanced in place
    lr, lf = d_losses(o_real, o_fake)
    (lr + lf).backward()
    res = dict(d_real=o_real.detach(), d_fake=o_fake.detach(), d_loss_real=lr.detach(), d_loss_fake=lf.detach())
    res.update({"D." + k: v for k, v in new2.items()})
    grads = {k: d[k].grad for k in trained(d) if d[k].grad is not None}
    return res, grads


def digest(key, g):
    """what a fixture keeps of a gradient: all of a bias / gamma / BN affine, (sum, L2 norm, every 97th) of a weight"""
    if g.dim() <= 1:
        return {key: g}
    flat = g.reshape(-1)
    return {key + "#sum": flat.sum(), key + "#norm": flat.norm(), key + "#every97": flat[::STRIDE].clone()}


def compact(res):
    """p2 (B, 256, 256) at every 8th row and as column sums"""
    out = dict(res)
    p2 = out.pop("p2")
    out["p2#rows"] = p2[:, ::P2_ROWS].clone()
    out["p2#colsum"] = p2.sum(1)
    return out


def record(B, dtype=torch.float64):
    """everything a fixture holds for batch size B, computed by this restatement in ``dtype``"""
    from fastfourierconvolution_amd import SAGANDiscriminator, SAGANGenerator
    gsd = cast(fill(SAGANGenerator(B, 32, Z_DIM, 64).state_dict(), 0), dtype)
    dsd = cast(fill(SAGANDiscriminator(B, 32, 64).state_dict(), 0), dtype)
    z_g, z_d, real = (t.to(dtype) for t in inputs(B))
    out = {}
    res, grads = scenario_g(gsd, dsd, z_g)
    out.update({"g/" + k: v for k, v in compact(res).items()})
    for k, g in grads.items():
        out.update(digest("g/grad/" + k, g))
    res, grads = scenario_d(gsd, dsd, z_d, real)
    out.update({"d/" + k: v for k, v in res.items()})
    for k, g in grads.items():
        out.update(digest("d/grad/" + k, g))
    return out


def load(B):
    with np.load(os.path.join(GOLDEN, f"b{B}.npz")) as f:
        return {k: torch.from_numpy(f[k]) for k in f.files}


# gradients that are zero in exact arithmetic (float64 leaves rounding noise around 1e-17), compared absolutely:
# key_conv.bias (it shifts every logit of a softmax row alike); in G a bias in front of a train-mode BatchNorm; in
# the D scenario, with every hinge term active, what does not depend on the input: d_loss adds -out(real) and
# +out(fake), so the gradients of value_conv.bias and last.0.bias cancel
def is_zero_grad(key):
    if "/grad/" not in key:
        return False
    if key.endswith("key_conv.bias"):
        return True
    if key.startswith("g/"):
        return key.endswith(".0.module.bias")
    return key.endswith(("value_conv.bias", "last.0.bias"))


def nerr(a, ref, absolute=False):
    """normwise error ||a - ref|| / ||ref|| in float64; ``absolute``: ||a - ref||"""
    a, ref = a.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    d = float((a - ref).norm())
    n = float(ref.norm())
    return d if absolute or n == 0 else d / n


def bound(f32_err):
    """the project's rule: 1e-5 normwise where the float32 restatement stays under 2.5e-6,
    four times the restatement's error otherwise"""
    return 1e-5 if f32_err < 2.5e-6 else 4.0 * f32_err
