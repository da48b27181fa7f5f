"""References and fixed-seed input builders of the conditional generator's stem, the label-embedding row
gather / scatter and the stem's four backward kernels (csrc/cond_kernels.hip), and of ffc_noise_wgrad
(csrc/caller_kernels.hip), shared by test_gpu_cond_kernels.py (kernel against reference on the GPU) and
test_cond_refs_cpu.py (reference against torch.nn and autograd).

Plain torch on the CPU in float64; inputs are float32 tensors (what the kernels read), widened exactly.
scatter_rows_f32 is the exception: the kernel's sum is defined in fp32 in sample order, so it is stated in
fp32.  A label outside [0, num_classes) -- as an int64, so 2^32 + 1 is outside -- reads as a NaN row in the
forward and is dropped from every gradient of the label path.  Nothing in this file imports the package
under test."""
import torch
import torch.nn as nn

CH = 256             # channels per branch (CS_CH)
COLS = 4096          # CH * 4 * 4: columns per branch (CS_N)
TILE = 32            # samples per workgroup, and per slab row (CS_BM)
CHUNK = 64           # k per staged chunk (CS_KC)
NAN = float("nan")


def in_range(labels, num_classes):
    """bool (B,): which int64 labels name a class"""
    assert labels.dtype == torch.int64
    return (labels >= 0) & (labels < num_classes)


def bad_labels(num_classes):
    """the out-of-range labels of the tests: below, just above, and two whose low 32 bits are valid classes"""
    return (-1, num_classes, 2 ** 32, 2 ** 32 + 1)


# --------------------------------------------------------------------------- rows
def gather_rows(table, labels):
    """table[labels] (B, D) in table's dtype: exact indexing, a NaN row for a label outside the table"""
    ok = in_range(labels, table.shape[0])
    out = torch.full((labels.shape[0], table.shape[1]), NAN, dtype=table.dtype)
    out[ok] = table[labels[ok]]
    return out


def scatter_rows_f32(grad, labels, num_classes):
    """(num_classes, D) float32: the rows of grad (B, D) of each class added in sample order in float32, from 0
    (embed_scatter_kernel's definition: bit-exact); labels outside the table add nothing"""
    assert grad.dtype == torch.float32
    out = torch.zeros(num_classes, grad.shape[1], dtype=torch.float32)
    for b, l in enumerate(labels.tolist()):
        if 0 <= l < num_classes:
            out[l] = out[l] + grad[b]
    return out


# --------------------------------------------------------------------------- stem forward
def _bias_cols(b):
    return b.double().repeat_interleave(16)[None, :]


def stem_pre(z, labels, embed, w_in, b_in, w_label, b_label):
    """(B, 512, 4, 4) float64: x . W.view(K, 4096) + bias[c] for x = z (channels 0..255) and x =
    embed[labels] (256..511).  A label out of range: NaN in that sample's label half, nowhere else."""
    B, Kz = z.shape
    NC = embed.shape[0]
    a = z.double() @ w_in.double().reshape(Kz, COLS) + _bias_cols(b_in)
    ok = in_range(labels, NC)
    lab = torch.full((B, COLS), NAN, dtype=torch.float64)
    lab[ok] = embed.double()[labels[ok]] @ w_label.double().reshape(NC, COLS) + _bias_cols(b_label)
    return torch.cat((a, lab), dim=1).reshape(B, 2 * CH, 4, 4)


def _tiles(pre, B):
    """pre (B, 512, 4, 4) -> one (2, 256, nv * 16) float64 tensor per 32-sample tile"""
    x = pre.double().reshape(B, 2, CH, 16)
    return [x[t:t + TILE].permute(1, 2, 0, 3).reshape(2, CH, -1) for t in range(0, B, TILE)]


def stem_slab(pre, B):
    """(2, rows, 256, 3) float64 {n, mean, M2} of the pre it is given, one row per 32-sample tile and branch:
    what cond_stem_kernel's epilogue writes (bn_common.h slab format without the padding float)"""
    rows = []
    for x in _tiles(pre, B):
        m = x.mean(dim=2)
        rows.append(torch.stack((torch.full_like(m, float(x.shape[2])), m, ((x - m[..., None]) ** 2).sum(dim=2)),
                                dim=-1))
    return torch.stack(rows, dim=1)


def stem_slab_abs(pre, B):
    """(2, rows, 256) float64: sum |x| over each slab row's elements (the mean bound's scale)"""
    return torch.stack([x.abs().sum(dim=2) for x in _tiles(pre, B)], dim=1)


# --------------------------------------------------------------------------- stem backward
def stem_backward(dpre, z, labels, embed, w_in, w_label):
    """dict of float64 gradients of sum(pre * dpre): dz (B, Kz), dlabel_embed (NC, NC), dw_in (Kz, 256, 4, 4),
    db_in (256), dw_label (NC, 256, 4, 4), db_label (256).  Samples whose label is out of range are dropped
    from dw_label and dlabel_embed and from nothing else.  abs_dw_in / abs_dw_label: per element
    sum_b |a[b][k] g[b][n]|, the scale of the weight gradients' bound (same samples as the gradient)."""
    B, Kz = z.shape
    NC = embed.shape[0]
    g = dpre.double().reshape(B, 2, COLS)
    g_in, g_lab = g[:, 0], g[:, 1]
    zd = z.double()
    ok = in_range(labels, NC)
    rows = embed.double()[labels[ok]]
    drow = g_lab @ w_label.double().reshape(NC, COLS).t()
    dembed = torch.zeros(NC, NC, dtype=torch.float64)
    dembed.index_add_(0, labels[ok], drow[ok])
    return {
        "dz": g_in @ w_in.double().reshape(Kz, COLS).t(),
        "dlabel_embed": dembed,
        "dw_in": (zd.t() @ g_in).reshape(Kz, CH, 4, 4),
        "db_in": g_in.reshape(B, CH, 16).sum(dim=(0, 2)),
        "dw_label": (rows.t() @ g_lab[ok]).reshape(NC, CH, 4, 4),
        "db_label": g_lab.reshape(B, CH, 16).sum(dim=(0, 2)),
        "abs_dw_in": (zd.abs().t() @ g_in.abs()).reshape(Kz, CH, 4, 4),
        "abs_dw_label": (rows.abs().t() @ g_lab[ok].abs()).reshape(NC, CH, 4, 4),
    }


GRADS = ("dw_in", "db_in", "dw_label", "db_label", "dz", "dlabel_embed")     # the C ABI's output order

# (B, z_size, num_classes) of the GPU tests (test_gpu_cond_kernels.py names the branch each is there for)
FWD_CASES = [(1, 1, 1), (31, 63, 3), (32, 64, 64), (33, 65, 65), (65, 129, 130)]
BWD_CASES = [(1, 1, 1), (3, 5, 2), (4, 16, 17), (5, 64, 65), (6, 1024, 3), (37, 70, 130)]
CONTRACT = (40, 5, 3)                       # the label contract: two tiles, the second of 8 samples
CONTRACT_BAD = (2, 5, 35, 36)               # bad labels in both tiles
CONTRACT_BAD_TILE1 = (32, 33, 35, 36)       # ... in tile 1 only
ROW_D = (1, 3, 4, 1020, 1024, 1028, 1030, 16384)
NOISE_CASES = [(1, 1, 4), (3, 5, 96), (2, 3, 1024), (2, 3, 1028), (1, 2, 4100), (2, 300, 36)]


# --------------------------------------------------------------------------- bounds (derived in test_gpu_cond_kernels.py)
U = 2.0 ** -24                   # one fp32 rounding
SECOND_ORDER = 1.0 + 2.0 ** -20  # covers (1 + u)^k - 1 - k u for the k used here
TOL = 1e-5                       # normwise, the kernel-level files' bound
D_MEAN = 21                      # roundings on the way to a slab row's mean
K_M2 = 23                        # ... to its M2, relative


def mean_limit(abs_sum, n):
    return D_MEAN * U * SECOND_ORDER * abs_sum / n


def m2_limit(m2, n, mean_lim):
    return K_M2 * U * SECOND_ORDER * m2 + n * mean_lim ** 2 * SECOND_ORDER


def wgrad_limit(B, abs_sum):
    """a chain of one fma per sample: gamma_B sum_b |a g|"""
    return B * U / (1.0 - B * U) * abs_sum


def noise_wgrad_limit(ref, abs_sum):
    return U * ref.abs() * SECOND_ORDER + 2.0 ** -40 * abs_sum


# --------------------------------------------------------------------------- NoiseInjection weight gradient
def noise_wgrad(g, noise):
    """dw[c] = sum_{b, hw} g[b, c, hw] noise[b, hw] and sum |g noise| per channel, float64; g (B, C, HW),
    noise (B, 1, HW)"""
    p = g.double() * noise.double().reshape(g.shape[0], 1, -1)
    return p.sum(dim=(0, 2)), p.abs().sum(dim=(0, 2))


# --------------------------------------------------------------------------- the stem's modules
class Stem(nn.Module):
    """Embedding -> ConvTranspose2d -> BatchNorm2d -> GELU for the labels, ConvTranspose2d -> BatchNorm2d ->
    GELU for z, concatenated: the conditional generator's stem on torch modules, under the model's names
    (what _autograd.cond_stem reads; in float64 the reference of the wrapper-level test)"""

    def __init__(self, z_size, num_classes):
        super().__init__()
        self.label_conv = nn.Sequential(nn.ConvTranspose2d(num_classes, CH, 4, 1, 0), nn.BatchNorm2d(CH), nn.GELU())
        self.input_conv = nn.Sequential(nn.ConvTranspose2d(z_size, CH, 4, 1, 0), nn.BatchNorm2d(CH), nn.GELU())
        self.label_embed = nn.Embedding(num_classes, num_classes)

    def forward(self, z, labels):
        e = self.label_embed(labels).view(labels.shape[0], -1, 1, 1)
        return torch.cat([self.input_conv(z.reshape(z.size(0), -1, 1, 1)), self.label_conv(e)], dim=1)


# --------------------------------------------------------------------------- input builders
def _draw(gen, *shape):
    """float32, mean 0.5, deviation 0.5: both signs occur, and a sum of products of two such draws keeps
    |sum| within a small factor of sum |term| (test_cond_refs_cpu.py checks the factor), so no reference
    value is the residue of a cancellation"""
    return 0.5 + 0.5 * torch.randn(*shape, generator=gen)


def stem_inputs(B, z_size, num_classes, seed=0):
    """z (B, Kz), embed (NC, NC), w_in (Kz, 256, 4, 4), b_in (256), w_label (NC, 256, 4, 4), b_label (256)"""
    gen = torch.Generator().manual_seed(11000 + 4099 * B + 131 * z_size + num_classes + 100003 * seed)
    return (_draw(gen, B, z_size), _draw(gen, num_classes, num_classes), _draw(gen, z_size, CH, 4, 4),
            0.3 * torch.randn(CH, generator=gen), _draw(gen, num_classes, CH, 4, 4),
            0.3 * torch.randn(CH, generator=gen))


def dpre_inputs(B, seed=0):
    """the (B, 512, 4, 4) gradient handed to the stem's backward"""
    return _draw(torch.Generator().manual_seed(12000 + B + 100003 * seed), B, 2 * CH, 4, 4)


def label_patterns(B, num_classes, seed=0):
    """dict of int64 (B,) in-range label vectors: 'one-class' (the last class); with more than one class
    'classes-left-out' (random, the last class always absent, the first sample's class repeated); with more than one tile and class 'per-tile'
    (tile 0 all class 0, the later tiles random classes other than 0, the last sample the last class)"""
    gen = torch.Generator().manual_seed(13000 + 67 * B + num_classes + 100003 * seed)
    pats = {"one-class": torch.full((B,), num_classes - 1, dtype=torch.int64)}
    if num_classes > 1:
        pats["classes-left-out"] = torch.randint(0, num_classes - 1, (B,), generator=gen)
        pats["classes-left-out"][-1] = pats["classes-left-out"][0]        # B > 1: a class occurs twice
        if B > TILE:
            p = torch.zeros(B, dtype=torch.int64)
            p[TILE:] = torch.randint(1, num_classes, (B - TILE,), generator=gen)
            p[-1] = num_classes - 1
            pats["per-tile"] = p
    return pats


def with_bad_labels(labels, positions, num_classes):
    """labels with bad_labels(num_classes) written at `positions`"""
    out = labels.clone()
    for p, v in zip(positions, bad_labels(num_classes)):
        out[p] = v
    return out


def row_inputs(B, num_classes, D, seed=0):
    """table (NC, D) and grad (B, D), float32 standard normal (the row sums are compared bit for bit)"""
    gen = torch.Generator().manual_seed(14000 + 31 * B + num_classes + 7 * D + 100003 * seed)
    return torch.randn(num_classes, D, generator=gen), torch.randn(B, D, generator=gen)


def row_labels(B, num_classes=7):
    """B = 1: class 3.  B = 9 (7 classes): class 3 three times, 0 and 6 once, 1 / 2 / 4 / 5 absent, and the
    four bad labels"""
    if B == 1:
        return torch.tensor([3], dtype=torch.int64)
    assert B == 9 and num_classes == 7
    bad = bad_labels(num_classes)
    return torch.tensor([3, 0, 3, bad[0], 6, bad[1], 3, bad[2], bad[3]], dtype=torch.int64)


def noise_inputs(B, C, HW, seed=0):
    """g (B, C, HW), noise (B, 1, HW): a different draw per sample"""
    gen = torch.Generator().manual_seed(15000 + 131 * B + 17 * C + HW + 100003 * seed)
    return _draw(gen, B, C, HW), _draw(gen, B, 1, HW)
