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
