"""The adaptive-weight critic loss on the GPU: the kernels of csrc/aw_kernels.hip through the
ffc::aw_weights / ffc::aw_combine ops against the fixture recorded from the reference's aw_method in
float64 (tests/golden/aw_cases.npz) and the float64 restatement tests/aw_refs.py; alignment, empty
tensors, launch splits and run-to-run bitwise equality; aw_method.aw_loss on Discriminator32 with
set_sn_hip off and on; a graph capture of the op pair that replays a second case into another branch.

Bounds, with u = 2^-53, n the list's element count, and aw_refs' dots correctly rounded:
  rr, ff, rf   products of fp32 values are exact in fp64, so the error is summation alone:
               |err| <= n u sum |x_i y_i|
  rs, fs       per logit exp (2 ulp allowed on the device, 1 in numpy), 1 + e and the division on each
               side: 8 u relative; the mean over m logits adds m u: (8 + m) u relative
  w_r, w_f     a quotient of the dots and a square root: the dots' relative bounds added up (rf + ff +
               rr / 2, or rf + rr + ff / 2) plus 8 u for sqrt, the products, the quotient, the sum
  combine      |out - (w_r g_r + w_f g_f)| <= 4 * 2^-24 (|w_r g_r| + |w_f g_f|): one rounding of each
               weight to fp32, the products and the add, fused or not
Every test prints what it measured."""
import functools

import numpy as np
import pytest
import torch

import aw_refs as R
import fastfourierconvolution_amd as F
from fastfourierconvolution_amd import _autograd as ag

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
E24 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _cases():
    cs = R.load_cases()
    for c in cs:
        c["ref"] = R.aw_reference(c["a"], c["b"], c["real"], c["fake"], **c["kw"])
    return cs


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in arrays]


def _kw(c):
    k = c["kw"]
    return (k["alpha1"], k["alpha2"], k["delta"], k["epsilon"], k["normalized"])


def _run(g_real, g_fake, real, fake, kw):
    """the op pair on fresh outputs -> (stats, out) on the device"""
    stats = torch.ops.ffc.aw_weights(g_real, g_fake, real, fake, *kw)
    out = [torch.full_like(g, float("nan")) for g in g_real]
    torch.ops.ffc.aw_combine(g_real, g_fake, stats, out)
    return stats, out


def _check_stats(tag, stats, ref, m_real, m_fake):
    s = stats.cpu().numpy()
    want = ref["stats"]
    n = ref["n"]
    rr, ff, rf = want[0], want[1], want[2]
    bounds = [n * U * rr, n * U * ff, n * U * ref["abs_rf"], (8 + m_real) * U * want[3], (8 + m_fake) * U * want[4]]
    rel = {"rr": n * U, "ff": n * U, "rf": n * U * ref["abs_rf"] / abs(rf)}
    case = ref["case"]
    rel_wr = rel["rf"] + rel["rr"] + rel["ff"] / 2 if case == 3 else rel["rr"] / 2
    rel_wf = rel["rf"] + rel["ff"] + rel["rr"] / 2 if case == 1 else rel["ff"] / 2
    bounds += [(rel_wr + 8 * U) * abs(want[5]), (rel_wf + 8 * U) * abs(want[6]), 0.0]
    err = np.abs(s - want)
    print(f"  {tag}: case {int(s[7])}  " +
          "  ".join(f"{k} {e:.2e}/{b:.2e}" for k, e, b in zip(R.STATS, err, bounds)))
    assert int(s[7]) == ref["case"]
    assert np.all(err <= bounds), dict(zip(R.STATS, zip(err, bounds)))


def _check_combine(tag, out, g_real, g_fake, w_r, w_f, extra=0.0):
    worst = 0.0
    for o, a, b in zip(out, g_real, g_fake):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        mag = np.abs(w_r * a) + np.abs(w_f * b)
        err = np.abs(o.detach().cpu().numpy().astype(np.float64) - (w_r * a + w_f * b))
        bound = (4 * E24 + extra) * mag
        assert np.all(err <= bound), (tag, float(err.max()))
        if a.size:
            worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
    print(f"  {tag}: max |err| / (|w_r g_r| + |w_f g_f|) = {worst / E24:.3f} * 2^-24 (bound 4)")


# --------------------------------------------------------------------------- the fixture, all 10 cases
@pytest.mark.parametrize("k", range(10))
def test_stats_and_combine_against_fixture_and_refs(k):
    c = _cases()[k]
    ref = c["ref"]
    assert ref["case"] == c["case"]
    stats, out = _run(_dev(c["a"]), _dev(c["b"]), _dev([c["real"]])[0], _dev([c["fake"]])[0], _kw(c))
    _check_stats(f"normalized={c['kw']['normalized']} case {c['case']}", stats, ref, c["real"].size, c["fake"].size)
    _check_combine("against aw_refs", out, c["a"], c["b"], ref["w_r"], ref["w_f"])
    # the reference's own param.grad: fp64, within 4 n u of aw_refs (tests/test_aw_cpu.py)
    worst = 0.0
    for o, a, b, g in zip(out, c["a"], c["b"], c["grads"]):
        mag = np.abs(ref["w_r"] * a.astype(np.float64)) + np.abs(ref["w_f"] * b.astype(np.float64))
        err = np.abs(o.cpu().numpy().astype(np.float64) - g)
        assert np.all(err <= (4 * E24 + 4 * ref["n"] * U) * mag)
        worst = max(worst, float(err.max()))
    print(f"  against the reference's param.grad: max |err| = {worst:.2e}")
    # the loss expression of aw_method against the reference's returned loss
    h = c["hyper"]
    w = stats[5:7].to(torch.float32)
    loss = float(w[0] * torch.tensor(h["c_r"], device=DEV) + w[1] * torch.tensor(h["c_f"], device=DEV))
    assert abs(loss - c["loss"]) <= (4 * E24 + 4 * ref["n"] * U) * (abs(ref["w_r"] * h["c_r"]) + abs(ref["w_f"] * h["c_f"]))


# --------------------------------------------------------------------------- edge layout
@functools.lru_cache(maxsize=None)
def _dense():
    """a dense random list: two chunks and a ragged tail, small odd sizes, an empty tensor"""
    gen = torch.Generator().manual_seed(5)
    chunk = ag.rt.lib().ffc_aw_chunk()
    shapes = [(2 * chunk + 5,), (7,), (0,), (3, 5, 11), (chunk,), (1,)]
    a = [0.1 * torch.randn(s, generator=gen) for s in shapes]
    b = [0.3 * torch.randn(s, generator=gen) - 0.02 for s in shapes]
    real, fake = torch.randn(5, 1, generator=gen) - 1.0, torch.randn(5, 1, generator=gen)
    kw = (0.5, 0.75, 0.05, 0.05, True)
    ref = R.aw_reference(a, b, real, fake, *kw)
    return a, b, real, fake, kw, ref


def _offset_views(ts, off):
    """contiguous copies of ``ts`` that start ``off`` floats into one 16-byte aligned buffer each"""
    out = []
    for t in ts:
        buf = torch.empty(t.numel() + 8, device=DEV)
        v = buf[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and (v.numel() == 0 or v.data_ptr() % 16 == (4 * off) % 16)
        out.append(v)
    return out


def test_unaligned_views_and_empty_tensors():
    a, b, real, fake, kw, ref = _dense()
    real, fake = real.to(DEV), fake.to(DEV)
    base_s, base_o = _run(_dev([t.numpy() for t in a]), _dev([t.numpy() for t in b]), real, fake, kw)
    _check_stats("dense, aligned", base_s, ref, real.numel(), fake.numel())
    _check_combine("dense, aligned", base_o, a, b, ref["w_r"], ref["w_f"])
    assert base_o[2].numel() == 0
    for tag, oa, ob in (("both at +4 bytes", 1, 1), ("g_real aligned, g_fake at +4 bytes", 0, 1),
                        ("g_real at +12 bytes, g_fake aligned", 3, 0)):
        s, o = _run(_offset_views(a, oa), _offset_views(b, ob), real, fake, kw)
        assert torch.equal(s, base_s), tag
        assert all(torch.equal(x, y) for x, y in zip(o, base_o)), tag
        print(f"  {tag}: stats and outputs bitwise equal to the aligned run")
    # unaligned outputs alone take the 4-byte form of the combine
    stats = torch.ops.ffc.aw_weights(_dev([t.numpy() for t in a]), _dev([t.numpy() for t in b]), real, fake, *kw)
    out = _offset_views([torch.zeros_like(t) for t in a], 1)
    torch.ops.ffc.aw_combine(_dev([t.numpy() for t in a]), _dev([t.numpy() for t in b]), stats, out)
    assert all(torch.equal(x, y) for x, y in zip(out, base_o))
    # without the empty tensor the list gives the same stats: it is skipped, not a chunk
    keep = [i for i, t in enumerate(a) if t.numel()]
    s, _ = _run(_dev([a[i].numpy() for i in keep]), _dev([b[i].numpy() for i in keep]), real, fake, kw)
    assert torch.equal(s, base_s)


def test_combine_refuses_aliased_outputs():
    a, b, real, fake, kw, _ = _dense()
    ga, gb = _dev([t.numpy() for t in a]), _dev([t.numpy() for t in b])
    stats = torch.ops.ffc.aw_weights(ga, gb, real.to(DEV), fake.to(DEV), *kw)
    with pytest.raises(Exception, match="alias"):
        torch.ops.ffc.aw_combine(ga, gb, stats, list(ga))


# --------------------------------------------------------------------------- reproducibility
def test_bitwise_reproducible_and_independent_of_the_launch_split():
    """The 19-tensor fixture list takes two launches of A and C at the default 16 pairs per launch;
    _autograd.AW_JOBS_PER_LAUNCH forces 5 (four launches) and 1 (one per tensor).  The partials are
    indexed by global (tensor, chunk) position and merged in one launch, so every split is bitwise
    equal, as are two runs on fresh copies."""
    c = _cases()[0]
    real, fake = _dev([c["real"]])[0], _dev([c["fake"]])[0]
    base_s, base_o = _run(_dev(c["a"]), _dev(c["b"]), real, fake, _kw(c))
    old = ag.AW_JOBS_PER_LAUNCH
    try:
        for per in (0, 16, 5, 1):
            ag.AW_JOBS_PER_LAUNCH = per
            s, o = _run(_dev(c["a"]), _dev(c["b"]), real, fake, _kw(c))
            assert torch.equal(s, base_s), per
            assert all(torch.equal(x, y) for x, y in zip(o, base_o)), per
            print(f"  {per or 'default'} pairs per launch: bitwise equal")
    finally:
        ag.AW_JOBS_PER_LAUNCH = old


# --------------------------------------------------------------------------- the module, end to end
def _randomize(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.05 if p.dim() > 1 else 0.1))
    return model


@pytest.mark.parametrize("sn_hip", [False, True])
def test_aw_loss_on_discriminator32(sn_hip):
    from fastfourierconvolution_amd import training as T
    D = _randomize(F.Discriminator32(sn=True, mg=4), 1).to(DEV).train()
    if sn_hip:
        F.set_sn_hip(D)
    gen = torch.Generator().manual_seed(3)
    x_fake = torch.randn(4, 3, 32, 32, generator=gen).to(DEV)
    x_real = (torch.randn(4, 3, 32, 32, generator=gen) + 0.5).to(DEV)
    opt = torch.optim.SGD(D.parameters(), lr=0.1)
    out_fake, out_real = D(x_fake), D(x_real)
    L_r, L_f = T.hinge_loss_real(out_real), T.hinge_loss_fake(out_fake)
    params = [p for _, p in D.named_parameters()]
    g_r = [g.contiguous() for g in torch.autograd.grad(L_r, params, retain_graph=True)]
    g_f = [g.contiguous() for g in torch.autograd.grad(L_f, params, retain_graph=True)]
    # thresholds chosen around the scores this critic gives, away from them (the branch is discontinuous)
    rs = float(torch.sigmoid(out_real.detach().double()).mean())
    fs = float(torch.sigmoid(out_fake.detach().double()).mean())
    aw = F.aw_method(alpha1=rs - 0.2, alpha2=rs - 0.1, delta=fs - rs + 0.1)   # cases 3 / 4: rs above all three
    ref = R.aw_reference(g_r, g_f, out_real, out_fake, aw._alpha1, aw._alpha2, aw._delta, aw._epsilon, True)
    rr, ff, rf = ref["stats"][:3]
    print(f"  sn_hip={sn_hip}: rs {rs:.4f} fs {fs:.4f} rr {rr:.3e} ff {ff:.3e} rf {rf:.3e} case {ref['case']} "
          f"w_r {ref['w_r']:.4e} w_f {ref['w_f']:.4e}")
    assert ref["case"] in (3, 4) and abs(rf) >= 1e-3 * np.sqrt(rr * ff)
    for first in (True, False):   # freshly assigned .grad, then written in place
        before = [None if p.grad is None else p.grad.data_ptr() for p in params]
        loss = aw.aw_loss(L_r, L_f, opt, D, out_real, out_fake)
        torch.cuda.synchronize()
        assert all(b is None for b in before) if first else before == [p.grad.data_ptr() for p in params]
        _check_stats("last_stats", aw.last_stats, ref, out_real.numel(), out_fake.numel())
        _check_combine(f"param.grad ({'assigned' if first else 'in place'})", [p.grad for p in params],
                       [g.cpu().numpy() for g in g_r], [g.cpu().numpy() for g in g_f], ref["w_r"], ref["w_f"])
        lr, lf = float(L_r.detach()), float(L_f.detach())
        want = ref["w_r"] * lr + ref["w_f"] * lf
        mag = abs(ref["w_r"] * lr) + abs(ref["w_f"] * lf)
        print(f"  loss {float(loss.detach()):.7f} want {want:.7f}")
        assert loss.dtype == torch.float32 and loss.requires_grad and abs(float(loss.detach()) - want) <= 4 * E24 * mag
    D.extra = torch.nn.Parameter(torch.zeros(3, device=DEV))
    with pytest.raises(RuntimeError, match="extra receives no gradient"):
        aw.aw_loss(L_r, L_f, opt, D, out_real, out_fake)


def test_aw_discriminator_step_runs_and_moves_the_critic():
    from fastfourierconvolution_amd import training as T
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):   # the model constructors print their channel split
        G = F.FGenerator32(z_size=128, mg=4).to(DEV).train()
    D = F.set_sn_hip(_randomize(F.Discriminator32(sn=True, mg=4), 1).to(DEV).train())
    oG = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.0, 0.9))
    oD = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.0, 0.9))
    gen = torch.Generator().manual_seed(7)
    z, real = torch.randn(4, 128, generator=gen).to(DEV), torch.randn(4, 3, 32, 32, generator=gen).to(DEV)
    aw = F.aw_method()
    before = [p.detach().clone() for p in D.parameters()]
    loss = T.aw_discriminator_step(G, D, oG, oD, z, real, aw)
    stats = aw.last_stats.cpu().numpy()
    print(f"  loss {float(loss.detach()):.5f} stats {stats}")
    assert np.isfinite(stats).all() and stats[7] in (1, 2, 3, 4, 5) and torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in D.parameters())
    assert any(not torch.equal(p, q) for p, q in zip(D.parameters(), before))


# --------------------------------------------------------------------------- no host synchronisation
def test_graph_capture_replays_another_branch():
    """aw_weights + aw_combine + the loss expression captured once on one stream with case 1 of
    Algorithm 1 in the static buffers, then replayed with case 4 (another b, other logits): a host-side
    branch or a synchronisation would fail the capture or replay case 1's weights."""
    c0, c1 = _cases()[0], _cases()[3]
    assert (c0["case"], c1["case"]) == (1, 4) and _kw(c0) == _kw(c1)
    kw = _kw(c0)

    def loss_of(stats, L_r, L_f):
        w = stats[5:7].to(torch.float32)
        return w[0] * L_r + w[1] * L_f

    def inputs(c):
        h = c["hyper"]
        return (_dev(c["a"]), _dev(c["b"]), _dev([c["real"]])[0], _dev([c["fake"]])[0],
                torch.tensor(h["c_r"], device=DEV), torch.tensor(h["c_f"], device=DEV))

    eager = []
    for c in (c0, c1):
        a, b, real, fake, L_r, L_f = inputs(c)
        stats, out = _run(a, b, real, fake, kw)
        eager.append((stats, out, loss_of(stats, L_r, L_f)))
    assert int(eager[0][0][7]) == 1 and int(eager[1][0][7]) == 4
    sa, sb, sreal, sfake, sL_r, sL_f = inputs(c0)
    sout = [torch.zeros_like(t) for t in sa]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gstats = torch.ops.ffc.aw_weights(sa, sb, sreal, sfake, *kw)
        torch.ops.ffc.aw_combine(sa, sb, gstats, sout)
        gloss = loss_of(gstats, sL_r, sL_f)
    for k, c in ((0, c0), (1, c1), (0, c0)):
        for dst, src in zip([*sa, *sb, sreal, sfake, sL_r, sL_f], [x for part in inputs(c) for x in
                                                                    (part if isinstance(part, list) else [part])]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        stats, out, loss = eager[k]
        assert torch.equal(gstats, stats), (k, gstats, stats)
        assert all(torch.equal(x, y) for x, y in zip(sout, out)), k
        assert torch.equal(gloss, loss), k
        print(f"  replay of case {c['case']}: stats, outputs and loss bitwise equal to the eager run")


# --------------------------------------------------------------------------- opcheck
def test_opcheck():
    c = _cases()[2]
    a, b = _dev(c["a"]), _dev(c["b"])
    real, fake = _dev([c["real"]])[0], _dev([c["fake"]])[0]
    for op, args in ((torch.ops.ffc.aw_weights.default, (a, b, real, fake, *_kw(c))),
                     (torch.ops.ffc.aw_combine.default,
                      (a, b, torch.ops.ffc.aw_weights(a, b, real, fake, *_kw(c)), [torch.zeros_like(t) for t in a]))):
        res = torch.library.opcheck(op, args, None, raise_exception=False)
        bad = {k: v for k, v in res.items() if v != "SUCCESS"}
        assert not bad, f"{op}: {bad}"
