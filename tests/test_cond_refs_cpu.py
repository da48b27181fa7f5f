"""The references of tests/cond_refs.py against independent statements of the same operations
(torch.nn.Embedding, torch.nn.ConvTranspose2d and autograd in float64), to 1e-12; float32 emulations of the
kernels' products with one planted defect each, which must exceed the bounds test_gpu_cond_kernels.py uses
(so those bounds can fail); and the input builders: fixed, and drawn so that a correct float32 evaluation
sits inside every bound.  No GPU."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as tF

import cond_refs as cr
import norm_refs as nr
from oracle.ffc_oracle import normwise_err

TOL = 1e-12
REF_CASES = [(3, 5, 2), (5, 64, 65), (33, 65, 65), (37, 70, 130)]       # four of the GPU shapes


def _close(a, b, tol=TOL):
    e = normwise_err(a, b)
    assert e <= tol, e


def _labels(B, NC):
    """a batch with a repeated and an absent class"""
    pats = cr.label_patterns(B, NC)
    lab = pats["classes-left-out"]
    assert NC - 1 not in lab.tolist() and len(set(lab.tolist())) < B
    return lab


# --------------------------------------------------------------------------- float32 emulations
def fma32(a, b, c):
    """fl32(a * b + c): the product of two float32 is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def pre32(x, w, b, drop_k=None):
    """x (B, K) . w (K, 4096) + b[c] as a float32 chain of one fma per k (drop_k: that term left out)"""
    acc = torch.zeros(x.shape[0], cr.COLS)
    for k in range(x.shape[1]):
        if k != drop_k:
            acc = fma32(x[:, k:k + 1], w.reshape(-1, cr.COLS)[k][None], acc)
    return acc + b.repeat_interleave(16)[None]


def stem32(z, labels, embed, w_in, b_in, w_label, b_label, drop_k=None, wrap=False):
    """the stem's forward in float32 (wrap: labels taken modulo 2^32 before the range test)"""
    lab = labels & 0xFFFFFFFF if wrap else labels
    rows = cr.gather_rows(embed, lab)
    return torch.cat((pre32(z, w_in, b_in, drop_k), pre32(rows, w_label, b_label, drop_k)), 1).reshape(-1, 512, 4, 4)


def slab32(pre, B, drop_last=False):
    """{n, mean, M2} rows in float32 arithmetic (drop_last: the last sample of a partly filled tile is left out
    of the sums, not of n)"""
    rows = []
    for x in cr._tiles(pre, B):
        x = x.float()
        n = float(x.shape[2])
        if drop_last and x.shape[2] < 16 * cr.TILE:
            x = x[..., :-16]
        m = x.sum(dim=2) / n
        rows.append(torch.stack((torch.full_like(m, n), m, ((x - m[..., None]) ** 2).sum(dim=2)), dim=-1))
    return torch.stack(rows, dim=1)


def wgrad32(a, g, samples):
    """sum over `samples` (in order) of a[b][k] g[b][n] as a float32 fma chain -> (K, 4096)"""
    acc = torch.zeros(a.shape[1], cr.COLS)
    for b in samples:
        acc = fma32(a[b][:, None], g[b][None, :], acc)
    return acc


def backward32(dpre, z, labels, embed, w_in, w_label, drop_last=False, wrap=False):
    """the stem's backward in float32; drop_last: the last sample left out of dw / db; wrap: labels modulo 2^32"""
    B, Kz = z.shape
    NC = embed.shape[0]
    lab = labels & 0xFFFFFFFF if wrap else labels
    g = dpre.reshape(B, 2, cr.COLS)
    ok = cr.in_range(lab, NC).tolist()
    every = list(range(B - 1 if drop_last else B))
    rows = cr.gather_rows(embed, lab)
    drow = g[:, 1] @ w_label.reshape(NC, cr.COLS).t()
    gs = g[:B - 1] if drop_last else g
    return {"dz": g[:, 0] @ w_in.reshape(Kz, cr.COLS).t(),
            "dlabel_embed": cr.scatter_rows_f32(drow, lab, NC),
            "dw_in": wgrad32(z, g[:, 0], every).reshape(Kz, 256, 4, 4),
            "db_in": gs[:, 0].reshape(-1, 256, 16).sum(dim=(0, 2)),
            "dw_label": wgrad32(rows, g[:, 1], [b for b in every if ok[b]]).reshape(NC, 256, 4, 4),
            "db_label": gs[:, 1].reshape(-1, 256, 16).sum(dim=(0, 2))}


def _bwd_ok(got, ref, B):
    """the GPU test's acceptance of one backward call, per output: True where it passes"""
    res = {}
    for k in cr.GRADS:
        if k.startswith("dw"):
            diff = (got[k].double() - ref[k]).abs()
            res[k] = bool((diff <= cr.wgrad_limit(B, ref["abs_" + k])).all())
        else:
            res[k] = normwise_err(got[k], ref[k]) <= cr.TOL
    return res


# --------------------------------------------------------------------------- references against torch
@pytest.mark.parametrize("B,Kz,NC", REF_CASES)
def test_stem_references_match_torch_modules_and_autograd(B, Kz, NC):
    z, embed, w_in, b_in, w_label, b_label = cr.stem_inputs(B, Kz, NC)
    labels = _labels(B, NC)
    dpre = cr.dpre_inputs(B)
    emb = nn.Embedding(NC, NC).double()
    with torch.no_grad():
        emb.weight.copy_(embed)
    assert torch.equal(cr.gather_rows(embed, labels).double(), emb(labels).detach())
    leaves = [t.double().requires_grad_(True) for t in (z, w_in, b_in, w_label, b_label)]
    zd, wi, bi, wl, bl = leaves
    e = emb(labels).view(B, NC, 1, 1)
    ct_in, ct_lab = nn.ConvTranspose2d(Kz, 256, 4, 1, 0).double(), nn.ConvTranspose2d(NC, 256, 4, 1, 0).double()
    pre = torch.cat([tF.conv_transpose2d(zd.view(B, Kz, 1, 1), wi, bi, ct_in.stride, ct_in.padding),
                     tF.conv_transpose2d(e, wl, bl, ct_lab.stride, ct_lab.padding)], dim=1)
    (pre * dpre.double()).sum().backward()
    _close(cr.stem_pre(z, labels, embed, w_in, b_in, w_label, b_label), pre.detach())
    got = cr.stem_backward(dpre, z, labels, embed, w_in, w_label)
    want = {"dz": zd.grad, "dlabel_embed": emb.weight.grad, "dw_in": wi.grad, "db_in": bi.grad, "dw_label": wl.grad,
            "db_label": bl.grad}
    for k in cr.GRADS:
        _close(got[k], want[k])
    absent = [c for c in range(NC) if c not in labels.tolist()]
    assert absent and bool((got["dlabel_embed"][absent] == 0).all())
    assert (got["abs_dw_in"] >= got["dw_in"].abs() * (1 - 1e-12)).all()
    assert (got["abs_dw_label"] >= got["dw_label"].abs() * (1 - 1e-12)).all()


def test_out_of_range_labels_in_the_references():
    """NaN rows in the label half of the bad samples only; dw_label / dlabel_embed are those of the batch
    without the bad samples, every other gradient that of the whole batch"""
    B, Kz, NC = cr.CONTRACT
    ins = cr.stem_inputs(B, Kz, NC)
    z, embed, w_in, b_in, w_label, b_label = ins
    clean = cr.label_patterns(B, NC)["per-tile"]
    bad = cr.with_bad_labels(clean, cr.CONTRACT_BAD, NC)
    assert bad[list(cr.CONTRACT_BAD)].tolist() == [-1, 3, 2 ** 32, 2 ** 32 + 1]
    assert cr.in_range(bad, NC).sum() == B - 4
    p0, p1 = cr.stem_pre(z, clean, *ins[1:]), cr.stem_pre(z, bad, *ins[1:])
    nan = torch.isnan(p1)
    assert nan[list(cr.CONTRACT_BAD), 256:].all() and int(nan.sum()) == 4 * 4096
    assert torch.equal(p1[~nan], p0[~nan])
    rows = cr.gather_rows(embed, bad)
    assert torch.isnan(rows[list(cr.CONTRACT_BAD)]).all() and torch.equal(rows[0], embed[bad[0]])
    dpre = cr.dpre_inputs(B)
    keep = [b for b in range(B) if b not in cr.CONTRACT_BAD]
    g1 = cr.stem_backward(dpre, z, bad, embed, w_in, w_label)
    g0 = cr.stem_backward(dpre, z, clean, embed, w_in, w_label)
    gk = cr.stem_backward(dpre[keep], z[keep], clean[keep], embed, w_in, w_label)
    for k in ("dw_label", "dlabel_embed", "abs_dw_label"):
        _close(g1[k], gk[k])
        assert normwise_err(g1[k], g0[k]) > 1e-3
    for k in ("dz", "dw_in", "db_in", "db_label", "abs_dw_in"):
        assert torch.equal(g1[k], g0[k]), k


@pytest.mark.parametrize("B,Kz,NC", [(1, 1, 1), (33, 65, 65), (65, 129, 130)])
def test_stem_slab_merges_to_the_plain_moments(B, Kz, NC):
    """stem_slab rows (unequal counts at B = 33: 512 and 16) merged by norm_refs.slab_moments: the per-channel
    n, sum, sum of squares of pre"""
    ins = cr.stem_inputs(B, Kz, NC)
    pre = cr.stem_pre(ins[0], _labels(B, NC) if NC > 1 else torch.zeros(B, dtype=torch.int64), *ins[1:]).float()
    slab = cr.stem_slab(pre, B)
    rows = (B + 31) // 32
    assert slab.shape == (2, rows, 256, 3) and slab.dtype == torch.float64
    assert slab[:, :, :, 0].unique().tolist() == sorted({16.0 * min(32, B - 32 * t) for t in range(rows)})
    x = pre.double().reshape(B, 2, 256, 16).permute(1, 2, 0, 3).reshape(2, 256, -1)
    for br in range(2):
        n, s, q = nr.slab_moments(slab[br])
        assert torch.equal(n, torch.full_like(n, 16.0 * B))
        _close(s, x[br].sum(dim=1))
        _close(q, (x[br] ** 2).sum(dim=1))
    _close(cr.stem_slab_abs(pre, B).sum(dim=1), x.abs().sum(dim=2))


@pytest.mark.parametrize("D", [3, 1024])
def test_scatter_rows_f32_against_index_add(D):
    NC, B = 7, 9
    _, grad = cr.row_inputs(B, NC, D)
    labels = cr.row_labels(B, NC)
    ok = cr.in_range(labels, NC)
    assert ok.tolist() == [True, True, True, False, True, False, True, False, False]
    got = cr.scatter_rows_f32(grad, labels, NC)
    ref = torch.zeros(NC, D, dtype=torch.float64).index_add_(0, labels[ok], grad.double()[ok])
    mag = torch.zeros(NC, D, dtype=torch.float64).index_add_(0, labels[ok], grad.double()[ok].abs())
    assert got.dtype == torch.float32
    assert ((got.double() - ref).abs() <= B * 2.0 ** -24 * mag).all()
    assert bool((got[[1, 2, 4, 5]] == 0).all()) and bool((got[[0, 3, 6]] != 0).any())
    assert torch.equal(got[0], grad[1]) and torch.equal(got[6], grad[4])      # one sample: the row itself
    assert torch.equal(got[3], (grad[0] + grad[2]) + grad[6])                 # three: in sample order


def test_noise_wgrad_reference():
    g, noise = cr.noise_inputs(3, 5, 96)
    ref, mag = cr.noise_wgrad(g, noise)
    want = torch.einsum("bcp,bp->c", g.double(), noise.double().reshape(3, 96))
    _close(ref, want)
    assert (mag >= ref.abs()).all() and ref.shape == (5,)
    assert not torch.equal(noise[0], noise[1])


def test_stem_module_is_the_composition():
    """cond_refs.Stem in float64 (eval: the running statistics) against stem_pre and a hand-written BN + GELU"""
    B, Kz, NC = 5, 8, 3
    m = cr.Stem(Kz, NC).double().eval()
    gen = torch.Generator().manual_seed(5)
    z, labels = torch.randn(B, Kz, generator=gen), torch.tensor([2, 0, 2, 1, 0])
    with torch.no_grad():
        y = m(z.double(), labels)
        pre = cr.stem_pre(z, labels, m.label_embed.weight.float(), m.input_conv[0].weight.float(),
                          m.input_conv[0].bias.float(), m.label_conv[0].weight.float(), m.label_conv[0].bias.float())
    assert set(m.state_dict()) >= {"label_embed.weight", "input_conv.0.weight", "label_conv.1.running_var"}
    ref = tF.gelu(pre / (1.0 + 1e-5) ** 0.5)           # fresh BatchNorm2d: mean 0, var 1, gamma 1, beta 0
    assert normwise_err(y, ref) <= 1e-6                  # the float32 copies of float64 parameters


# --------------------------------------------------------------------------- planted errors
def test_planted_dropped_sample_of_a_partial_tile_exceeds_the_bounds():
    """B = 37 (tile 1 holds 5 samples): the fifth left out of the slab sums, and of dw / db"""
    B, Kz, NC = 37, 70, 130
    ins = cr.stem_inputs(B, Kz, NC)
    labels = cr.label_patterns(B, NC)["per-tile"]
    pre = cr.stem_pre(ins[0], labels, *ins[1:]).float()
    ref, mag = cr.stem_slab(pre, B), cr.stem_slab_abs(pre, B)
    n = ref[..., 0]
    lim_mean = cr.mean_limit(mag, n)
    lim_m2 = cr.m2_limit(ref[..., 2], n, lim_mean)
    good, bad = slab32(pre, B).double(), slab32(pre, B, drop_last=True).double()
    assert ((good[..., 1] - ref[..., 1]).abs() <= lim_mean).all()
    assert ((good[..., 2] - ref[..., 2]).abs() <= lim_m2).all()
    assert torch.equal(bad[:, 0], good[:, 0])                                  # the full tile is untouched
    assert ((bad[:, 1, :, 1] - ref[:, 1, :, 1]).abs() > lim_mean[:, 1]).all()
    assert ((bad[:, 1, :, 2] - ref[:, 1, :, 2]).abs() > lim_m2[:, 1]).all()
    dpre = cr.dpre_inputs(B)
    z, embed, w_in, _, w_label, _ = ins
    rb = cr.stem_backward(dpre, z, labels, embed, w_in, w_label)
    assert all(_bwd_ok(backward32(dpre, z, labels, embed, w_in, w_label), rb, B).values())
    res = _bwd_ok(backward32(dpre, z, labels, embed, w_in, w_label, drop_last=True), rb, B)
    assert not (res["dw_in"] or res["db_in"] or res["dw_label"] or res["db_label"]), res


def test_planted_dropped_k64_term_exceeds_the_bound():
    B, Kz, NC = 33, 65, 65
    ins = cr.stem_inputs(B, Kz, NC)
    labels = cr.label_patterns(B, NC)["per-tile"]
    ref = cr.stem_pre(ins[0], labels, *ins[1:])
    good, bad = stem32(ins[0], labels, *ins[1:]), stem32(ins[0], labels, *ins[1:], drop_k=64)
    for br in range(2):
        half = slice(256 * br, 256 * br + 256)
        assert normwise_err(good[:, half], ref[:, half]) <= cr.TOL / 4
        assert normwise_err(bad[:, half], ref[:, half]) > 100 * cr.TOL


def test_planted_label_modulo_2_32_is_caught():
    """2^32 and 2^32 + 1 read as classes 0 and 1: no NaN row where the contract promises one, and those samples
    in dw_label / dlabel_embed"""
    B, Kz, NC = cr.CONTRACT
    ins = cr.stem_inputs(B, Kz, NC)
    z, embed, w_in, _, w_label, _ = ins
    labels = cr.with_bad_labels(cr.label_patterns(B, NC)["per-tile"], cr.CONTRACT_BAD, NC)
    wrapped = stem32(z, labels, *ins[1:], wrap=True)
    good = stem32(z, labels, *ins[1:])
    bad_rows = list(cr.CONTRACT_BAD)
    assert torch.isnan(good[bad_rows, 256:]).all() and not torch.isnan(good[bad_rows, :256]).any()
    assert not torch.isnan(wrapped[bad_rows[2:], 256:]).any()                  # the test asserts all NaN: it fails
    dpre = cr.dpre_inputs(B)
    rb = cr.stem_backward(dpre, z, labels, embed, w_in, w_label)
    assert all(_bwd_ok(backward32(dpre, z, labels, embed, w_in, w_label), rb, B).values())
    res = _bwd_ok(backward32(dpre, z, labels, embed, w_in, w_label, wrap=True), rb, B)
    assert not res["dw_label"] and not res["dlabel_embed"], res
    assert res["dz"] and res["dw_in"] and res["db_in"] and res["db_label"], res
    # the gather and the scatter likewise
    table, grad = cr.row_inputs(9, 7, 4)
    rl = cr.row_labels(9, 7)
    assert not torch.isnan(cr.gather_rows(table, rl & 0xFFFFFFFF)[7:]).any() and torch.isnan(cr.gather_rows(table, rl)[7:]).all()
    assert not torch.equal(cr.scatter_rows_f32(grad, rl & 0xFFFFFFFF, 7), cr.scatter_rows_f32(grad, rl, 7))


@pytest.mark.parametrize("D", [4, 1030])
def test_planted_reversed_sample_order_in_the_scatter_is_caught(D):
    _, grad = cr.row_inputs(9, 7, D)
    labels = cr.row_labels(9, 7)
    fwd = cr.scatter_rows_f32(grad, labels, 7)
    rev = cr.scatter_rows_f32(grad.flip(0), labels.flip(0), 7)
    assert not torch.equal(fwd, rev)                   # the GPU test asks for torch.equal
    assert torch.equal(fwd[[0, 6]], rev[[0, 6]])       # classes of one sample have no order


# --------------------------------------------------------------------------- inputs
def test_input_builders_are_fixed():
    for a, b in zip(cr.stem_inputs(3, 5, 2), cr.stem_inputs(3, 5, 2)):
        assert torch.equal(a, b) and a.dtype == torch.float32
    assert torch.equal(cr.dpre_inputs(3), cr.dpre_inputs(3))
    for B, NC in ((1, 1), (31, 3), (65, 130)):
        p, q = cr.label_patterns(B, NC), cr.label_patterns(B, NC)
        assert list(p) == list(q) and all(torch.equal(p[k], q[k]) and p[k].dtype == torch.int64 for k in p)
        assert all(cr.in_range(v, NC).all() for v in p.values())
    p = cr.label_patterns(65, 130)
    assert list(p) == ["one-class", "classes-left-out", "per-tile"]
    assert set(p["per-tile"][:32].tolist()) == {0} and 0 not in p["per-tile"][32:].tolist()
    assert set(p["per-tile"][32:64].tolist()) != set(p["per-tile"][64:].tolist())
    assert list(cr.label_patterns(1, 1)) == ["one-class"] and list(cr.label_patterns(31, 3)) == ["one-class", "classes-left-out"]
    for a, b in zip(cr.row_inputs(9, 7, 1030) + cr.noise_inputs(2, 3, 1028), cr.row_inputs(9, 7, 1030) + cr.noise_inputs(2, 3, 1028)):
        assert torch.equal(a, b) and a.dtype == torch.float32
    assert cr.bad_labels(3) == (-1, 3, 4294967296, 4294967297)


def _kappa(terms_abs, ref):
    """largest sum |term| of an element over the largest |ref|: the factor between u times the rounding depth
    and the normwise error a summation of that depth can make"""
    return float(terms_abs.max() / ref.abs().max())


@pytest.mark.parametrize("B,Kz,NC", cr.FWD_CASES)
def test_forward_inputs_leave_room_inside_the_bounds(B, Kz, NC):
    """a float32 fma chain sits a factor 4 inside the normwise bound on both branches; no element's reference
    is the residue of a cancellation (kappa <= 2); every slab row's M2 reference is well above 0, and a plain
    float32 evaluation of the slab sits inside its bounds"""
    ins = cr.stem_inputs(B, Kz, NC)
    z, embed, w_in, b_in, w_label, b_label = ins
    for name, labels in cr.label_patterns(B, NC).items():
        ref = cr.stem_pre(z, labels, *ins[1:])
        got = stem32(z, labels, *ins[1:])
        mag = cr.stem_pre(z.abs(), labels, embed.abs(), w_in.abs(), b_in.abs(), w_label.abs(), b_label.abs())
        for br in range(2):
            half = slice(256 * br, 256 * br + 256)
            e, k = normwise_err(got[:, half], ref[:, half]), _kappa(mag[:, half], ref[:, half])
            print(f"OBS pre ({B},{Kz},{NC}) {name} branch {br}: fp32 chain {e:.2e} kappa {k:.2f}")
            assert e <= cr.TOL / 4 and k <= 2.0
        slab, smag = cr.stem_slab(got, B), cr.stem_slab_abs(got, B)
        n = slab[..., 0]
        lm = cr.mean_limit(smag, n)
        l2 = cr.m2_limit(slab[..., 2], n, lm)
        s32 = slab32(got, B).double()
        assert (slab[..., 2] > 1e-3).all()
        assert ((s32[..., 1] - slab[..., 1]).abs() <= lm).all() and ((s32[..., 2] - slab[..., 2]).abs() <= l2).all()
        assert (l2 <= 1e-4 * slab[..., 2]).all()          # the relative bound stays a relative bound


@pytest.mark.parametrize("B,Kz,NC", cr.BWD_CASES)
def test_backward_inputs_leave_room_inside_the_bounds(B, Kz, NC):
    z, embed, w_in, _, w_label, _ = cr.stem_inputs(B, Kz, NC)
    dpre = cr.dpre_inputs(B)
    labels = list(cr.label_patterns(B, NC).values())[-1]
    ref = cr.stem_backward(dpre, z, labels, embed, w_in, w_label)
    got = backward32(dpre, z, labels, embed, w_in, w_label)
    mag = cr.stem_backward(dpre.abs(), z.abs(), labels, embed.abs(), w_in.abs(), w_label.abs())
    for k in cr.GRADS:
        if k.startswith("dw"):
            worst = float(((got[k].double() - ref[k]).abs() / cr.wgrad_limit(B, ref["abs_" + k]).clamp_min(1e-300)).max())
            print(f"OBS {k} ({B},{Kz},{NC}): fp32 chain diff / limit {worst:.2f}")
            assert worst <= 1.0
        else:
            e, kap = normwise_err(got[k], ref[k]), _kappa(mag[k], ref[k])
            print(f"OBS {k} ({B},{Kz},{NC}): fp32 {e:.2e} kappa {kap:.2f}")
            assert e <= cr.TOL / 4 and kap <= 2.0


@pytest.mark.parametrize("B,C,HW", cr.NOISE_CASES)
def test_noise_wgrad_inputs_leave_room_inside_the_bound(B, C, HW):
    """at most 2^13 products per channel, so an fp64 sum in any order is within 2^13 2^-53 sum |g n|; one fp32
    rounding of it within the bound; no channel's reference is near 0 against sum |g n|"""
    assert B * HW <= 2 ** 13
    g, noise = cr.noise_inputs(B, C, HW)
    ref, mag = cr.noise_wgrad(g, noise)
    assert (ref.abs() >= 0.25 * mag).all()
    got = ref.float().double()
    assert ((got - ref).abs() <= cr.noise_wgrad_limit(ref, mag)).all()
    # a float32 accumulation instead of the kernel's fp64 one fails it at the larger sizes
    if B * HW >= 2048:
        seq = torch.zeros(C)
        for p in (g * noise).permute(0, 2, 1).reshape(-1, C):
            seq = seq + p
        assert ((seq.double() - ref).abs() > cr.noise_wgrad_limit(ref, mag)).any()
