"""float64 references and fixed-seed input builders of the forward spectral-branch kernels
(csrc/fu_kernels.hip, fu2d_kernels.hip, st_prologue.hip, st_pw.hip, the SE gate, dense.hip), shared by
test_gpu_spectral_kernels.py (kernel against reference on the GPU) and test_spectral_refs_cpu.py
(reference against an independent statement of the same operation).

Written from the contracts in include/ffc_amd.h ("spectral branch") and the module semantics of
ffc/fourier_unity.py / ffc/spectral_transform.py.  Everything here is plain torch on the CPU in
float64; inputs are float32 tensors (what the kernels read), widened exactly.  Nothing in this file
imports the package under test."""
import torch
import torch.nn.functional as F

KINK = 1e-3       # no ReLU / LeakyReLU pre-activation of a built input lies within this of 0
BN_EPS = 1e-5
SLOPE = 0.1


def act64(z, code, slope=SLOPE):
    return {0: lambda v: v, 1: F.relu, 2: lambda v: F.leaky_relu(v, slope), 3: torch.tanh, 4: torch.sigmoid,
            5: F.gelu}[code](z)


def _per_channel(v):
    return None if v is None else v.double()[None, :, None, None]


# --------------------------------------------------------------------------- Fourier unit
def fu_input(t, in_scale, in_shift, in_relu):
    """float64 t * in_scale[c] + in_shift[c] (when given), then ReLU (when in_relu): bn1 + act1"""
    s = t.double()
    if in_scale is not None:
        s = s * _per_channel(in_scale) + _per_channel(in_shift)
    return F.relu(s) if in_relu else s


def fu_stages(t, in_scale, in_shift, in_relu, up, wmix):
    """(s, Z, Y): s = transformed t nearest-upsampled by `up` (B, C, H, W); Z = rfftn(s, ortho) as
    interleaved channels 2c = Re, 2c + 1 = Im (B, 2C, H, W/2+1); Y = wmix Z, wmix (2C, 2C) the 1x1
    conv_layer weight"""
    s = fu_input(t, in_scale, in_shift, in_relu)
    if up > 1:
        s = s.repeat_interleave(up, dim=2).repeat_interleave(up, dim=3)
    B, C, H, W = s.shape
    X = torch.fft.rfftn(s, dim=(-2, -1), norm="ortho")
    Z = torch.stack((X.real, X.imag), dim=2).reshape(B, 2 * C, H, W // 2 + 1)
    Y = torch.einsum("oi,bihw->bohw", wmix.double().reshape(2 * C, 2 * C), Z)
    return s, Z, Y


def spectrum_of(Y):
    """interleaved Re/Im channels (B, 2C, H, WP) -> complex (B, C, H, WP)"""
    B, C2, H, WP = Y.shape
    Yv = Y.reshape(B, C2 // 2, 2, H, WP)
    return torch.complex(Yv[:, :, 0], Yv[:, :, 1])


def bn_relu(Y, bn_scale, bn_shift):
    return F.relu(Y.double() * _per_channel(bn_scale) + _per_channel(bn_shift))


def fu_out(Y, bn_scale, bn_shift, s, residual, H, W):
    """irfftn(relu(Y * scale + shift), s=(H, W), ortho) (+ s)"""
    out = torch.fft.irfftn(spectrum_of(bn_relu(Y, bn_scale, bn_shift)), s=(H, W), dim=(-2, -1), norm="ortho")
    return out + s if residual else out


def fu2d_T(t, in_scale, in_shift, in_relu):
    """staged R2C: unnormalised rfft2 of the un-upsampled transformed t, (B, C, h, w/2+1, 2)"""
    X = torch.fft.rfftn(fu_input(t, in_scale, in_shift, in_relu), dim=(-2, -1), norm="backward")
    return torch.view_as_real(X).contiguous()


def fu2d_Y(Y):
    """interleaved channel planes (B, 2C, H, WP) -> the staged FU's (B, C, H, WP, 2) complex64 layout"""
    return torch.view_as_real(spectrum_of(Y).contiguous()).contiguous()


def fu2d_Yc(Y, bn_scale, bn_shift):
    """column-fused pass 1: the unnormalised inverse FFT over H of relu(Y * scale + shift), stored
    column-major (B, C, W/2+1, H, 2)"""
    X = spectrum_of(bn_relu(Y, bn_scale, bn_shift))
    Xc = torch.fft.ifft(X, dim=2, norm="forward")          # norm="forward": no scale on the inverse
    return torch.view_as_real(Xc.transpose(2, 3).contiguous()).contiguous()


def fu2d_rows(Yc, s, residual, H, W):
    """rows-only C2R of Yc (B, C, W/2+1, H, 2): inverse real FFT over W (Im of bins 0 and W/2 ignored),
    ortho scale 1 / sqrt(H W) (+ s)"""
    X = torch.view_as_complex(Yc.double().contiguous()).transpose(2, 3)
    out = torch.fft.irfft(X, n=W, dim=-1, norm="forward") / (H * W) ** 0.5
    return out + s if residual else out


# --------------------------------------------------------------------------- BatchNorm statistics
def channel_stats(Y):
    """(n, mean, biased var) per channel of (B, C, ...) in float64"""
    Yd = Y.double().transpose(0, 1).reshape(Y.shape[1], -1)
    return float(Yd.shape[1]), Yd.mean(dim=1), Yd.var(dim=1, unbiased=False)


def merge_slab(slab):
    """partial rows [rows][C] {n, mean, M2, ...} -> (n [C], mean [C], biased var [C]) in float64 (the
    merge of tests/test_gpu_convq.py); rows with n = 0 contribute nothing"""
    s = slab.double()
    n = s[..., 0].sum(0)
    mean = (s[..., 0] * s[..., 1]).sum(0) / n
    m2 = (s[..., 2] + s[..., 0] * (s[..., 1] - mean) ** 2).sum(0)
    return n, mean, m2 / n


def make_slab(x, parts):
    """float32 partial rows {n, mean, M2, 0} of x (B, C, P...) flattened per channel and cut at the
    element offsets `parts`: a slab whose merge is x's statistics"""
    xd = x.double().transpose(0, 1).reshape(x.shape[1], -1)
    edges = [0] + list(parts) + [xd.shape[1]]
    rows = []
    for a, b in zip(edges[:-1], edges[1:]):
        seg = xd[:, a:b]
        n = float(b - a)
        if n == 0:
            rows.append(torch.zeros(x.shape[1], 4, dtype=torch.float64))
            continue
        m = seg.mean(dim=1)
        rows.append(torch.stack((torch.full_like(m, n), m, ((seg - m[:, None]) ** 2).sum(dim=1), torch.zeros_like(m)),
                                dim=1))
    return torch.stack(rows).float()


def bn_finalize(n, mean, var, gamma, beta, eps=BN_EPS, momentum=0.1, count_mult=1.0, running_mean=None,
                running_var=None, num_batches_tracked=0):
    """nn.BatchNorm2d train step from batch statistics: y = x * scale + shift with the biased variance;
    running_var takes the unbiased variance over n * count_mult samples; momentum < 0 is momentum=None
    (cumulative average 1 / (num_batches_tracked + 1)).  Returns scale, shift, running_mean, running_var,
    num_batches_tracked (the running values None when none were given)."""
    g = gamma.double() if gamma is not None else torch.ones_like(mean)
    b = beta.double() if beta is not None else torch.zeros_like(mean)
    scale = g / torch.sqrt(var + eps)
    shift = b - mean * scale
    if running_mean is None:
        return scale, shift, None, None, num_batches_tracked
    nfull = torch.as_tensor(n, dtype=torch.float64) * count_mult
    unb = var * nfull / (nfull - 1.0)
    fm = momentum if momentum >= 0 else 1.0 / (num_batches_tracked + 1)
    rm = (1 - fm) * running_mean.double() + fm * mean
    rv = (1 - fm) * running_var.double() + fm * unb
    return scale, shift, rm, rv, num_batches_tracked + 1


# --------------------------------------------------------------------------- SpectralTransform prologue
def se_gate(x, pool, w1, w2):
    """SELayer gate sigmoid(W2 relu(W1 mean_hw x)) of the (2x2 average pooled) input, (B, C); w1 (hidden, C),
    w2 (C, hidden); hidden = 0 (w1 None or empty): gate 0.5"""
    xd = F.avg_pool2d(x.double(), 2, 2) if pool else x.double()
    m = xd.mean(dim=(2, 3))
    if w1 is None or w1.shape[0] == 0:
        return torch.full_like(m, 0.5)
    return torch.sigmoid(F.relu(m @ w1.double().t()) @ w2.double().t())


def pw_gate_conv(x, gate, w):
    """t[b, o, p] = sum_c w[o, c] gate[b, c] x[b, c, p]; x (B, Cin, ...), gate (B, Cin) or None, w (M, Cin)"""
    xd = x.double()
    if gate is not None:
        xd = xd * gate.double().reshape(gate.shape + (1,) * (xd.dim() - 2))
    return torch.einsum("oc,bc...->bo...", w.double(), xd)


def st_prologue(x, pool, w1, w2, wconv1):
    """[2x2 average pool] -> SE gate -> conv1 (1x1): gate (B, Cin), t (B, c, h, w), channel_stats(t)"""
    gate = se_gate(x, pool, w1, w2)
    xd = F.avg_pool2d(x.double(), 2, 2) if pool else x.double()
    t = pw_gate_conv(xd, gate, wconv1)
    return gate, t, channel_stats(t)


def dense(A, Wt, bias, act, slope=SLOPE):
    """act(A Wt + bias), A (B, K), Wt (K, N)"""
    out = A.double() @ Wt.double()
    if bias is not None:
        out = out + bias.double()
    return act64(out, act, slope)


# --------------------------------------------------------------------------- kink-free builders
def clear_offset(v, nominal, kink=KINK):
    """the offset closest to `nominal` that keeps every v + offset at least 2.5 kink from 0 (v: 1-d float64)"""
    p = torch.sort(-v.double().reshape(-1)).values
    cands = torch.cat((torch.tensor([float(nominal)], dtype=torch.float64), p - 2.5 * kink, p + 2.5 * kink))
    i = torch.searchsorted(p, cands).clamp(1, max(1, p.numel() - 1))
    near = torch.minimum((cands - p[i - 1]).abs(), (cands - p[i.clamp(max=p.numel() - 1)]).abs())
    ok = near >= 2.4 * kink
    assert ok.any(), "no kink-free offset"
    score = torch.where(ok, (cands - nominal).abs(), torch.full_like(cands, float("inf")))
    return float(cands[score.argmin()])


def clear_shifts(Y, scale, shift):
    """per-channel float32 shift near `shift` such that no Y * scale + shift (fp64, the float32 scale / shift
    widened) is within KINK of 0; Y (B, C, ...)"""
    sc = scale.float().double()
    out = shift.clone().float()
    Yc = Y.double().transpose(0, 1).reshape(Y.shape[1], -1)
    for c in range(Y.shape[1]):
        out[c] = clear_offset(Yc[c] * sc[c], float(shift[c]))
    pre = Yc * sc[:, None] + out.double()[:, None]
    assert pre.abs().min() >= KINK
    return out


def clear_input(t, in_scale, in_shift):
    """float32 t moved so that no t * in_scale + in_shift (fp64) is within KINK of 0: an offending element
    goes to +-2 KINK on its own side"""
    if in_scale is None:
        return t
    sc, sh = _per_channel(in_scale), _per_channel(in_shift)
    for _ in range(20):
        z = t.double() * sc + sh
        bad = z.abs() < KINK
        if not bad.any():
            return t
        target = torch.where(z >= 0, 2 * KINK, -2 * KINK)
        t = torch.where(bad, (target - sh) / sc, t.double()).float()
    raise AssertionError("kink-free input builder did not converge")


def fu_inputs(B, C, h, w, up, affine, relu, seed=0):
    """fixed-seed float32 inputs of one Fourier-unit case: t (B, C, h, w), in_scale / in_shift (None without
    `affine`), the mix weight wmix (2C, 2C), and the FU BN's gamma / beta; kink-free at the input ReLU.
    The FU BN's shift is cleared against Y by fu_case."""
    gen = torch.Generator().manual_seed(7000 + 131 * C + 17 * h + 3 * w + up + 1000 * seed)
    t = torch.randn(B, C, h, w, generator=gen)
    in_scale = in_shift = None
    if affine:
        in_scale = (0.6 + 0.8 * torch.rand(C, generator=gen)) * (1 - 2 * (torch.arange(C) % 2)).float()
        in_shift = 0.3 * torch.randn(C, generator=gen)
        if relu:
            t = clear_input(t, in_scale, in_shift)
    wmix = torch.randn(2 * C, 2 * C, generator=gen) / (2 * C) ** 0.5
    gamma = (0.5 + torch.rand(2 * C, generator=gen)) * (1 - 2 * (torch.arange(2 * C) % 2)).float()
    beta = 0.2 * torch.randn(2 * C, generator=gen)
    return dict(t=t, in_scale=in_scale, in_shift=in_shift, wmix=wmix, gamma=gamma, beta=beta)


def fu_case(B, C, h, w, up, affine, relu, seed=0):
    """inputs + float64 stages of a Fourier-unit case with the FU's BatchNorm on batch statistics:
    s, Z, Y, stats = channel_stats(Y), float32 bn_scale / bn_shift (beta moved so that no BN output is
    within KINK of 0), out / out_res (without / with the residual)"""
    d = fu_inputs(B, C, h, w, up, affine, relu, seed)
    s, Z, Y = fu_stages(d["t"], d["in_scale"], d["in_shift"], relu, up, d["wmix"])
    n, mean, var = channel_stats(Y)
    scale, shift, _, _, _ = bn_finalize(n, mean, var, d["gamma"], d["beta"])
    bn_scale = scale.float()
    bn_shift = clear_shifts(Y, bn_scale, shift.float())
    # the beta that yields bn_shift under the batch statistics (for the cases that fold the BN in-kernel)
    d["beta"] = (bn_shift.double() + mean * scale).float()
    H, W = h * up, w * up
    d.update(s=s, Z=Z, Y=Y, stats=(n, mean, var), bn_scale=bn_scale, bn_shift=bn_shift, H=H, W=W,
             out=fu_out(Y, bn_scale, bn_shift, s, False, H, W), out_res=fu_out(Y, bn_scale, bn_shift, s, True, H, W))
    return d


def se_weights(x, pool, hidden, gen):
    """w1 (hidden, C), w2 (C, hidden) with no hidden pre-activation w1 . mean(x) within KINK of 0 (w1 moved
    along the offending sample's mean)"""
    C = x.shape[1]
    if hidden == 0:
        return None, None
    w1 = torch.randn(hidden, C, generator=gen) / C ** 0.5
    w2 = torch.randn(C, hidden, generator=gen) / hidden ** 0.5
    xd = F.avg_pool2d(x.double(), 2, 2) if pool else x.double()
    m = xd.mean(dim=(2, 3))
    for _ in range(200):
        pre = m @ w1.double().t()
        bad = pre.abs() < KINK
        if not bad.any():
            return w1, w2
        b, j = [int(v) for v in bad.nonzero()[0]]
        target = 2 * KINK if pre[b, j] >= 0 else -2 * KINK
        w1 = w1.clone()
        w1[j] = (w1[j].double() + (target - pre[b, j]) / (m[b] @ m[b]) * m[b]).float()
    raise AssertionError("SE builder did not converge")


def st_inputs(B, Cin, c, H, W, pool, hidden):
    gen = torch.Generator().manual_seed(8000 + 7 * Cin + 11 * c + 13 * H + W + 100 * pool + 1000 * hidden)
    x = torch.randn(B, Cin, H, W, generator=gen) + 0.3
    w1, w2 = se_weights(x, pool, hidden, gen)
    wconv1 = torch.randn(c, Cin, generator=gen) / Cin ** 0.5
    return x, w1, w2, wconv1


def dense_inputs(B, K, N, with_bias, act):
    """A (B, K), Wt (K, N), bias (N) or None; for LeakyReLU the bias is moved per column so that no
    pre-activation is within KINK of 0"""
    gen = torch.Generator().manual_seed(9000 + 7 * B + 11 * K + N + act)
    A = torch.randn(B, K, generator=gen)
    Wt = torch.randn(K, N, generator=gen) / K ** 0.5
    bias = 0.5 * torch.randn(N, generator=gen) if with_bias else None
    if act in (1, 2):
        assert with_bias, "the kink-free builder moves the bias"
        pre = A.double() @ Wt.double()
        for j in range(N):
            bias[j] = clear_offset(pre[:, j], float(bias[j]))
        assert (pre + bias.double()).abs().min() >= KINK
    return A, Wt, bias
