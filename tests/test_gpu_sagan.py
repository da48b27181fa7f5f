"""SAGANGenerator, SAGANDiscriminator, SAGANSpectralNorm and training.sagan_step on the GPU against the fixtures
recorded from the reference's classes (tests/golden/sagan/, B = 2 and 3) and against the float64 restatement
(tests/sagan_refs.py; B = 1 and the training iteration).  Weights: sagan_refs.fill(state_dict, 0).

Bounds, normwise: 1e-4 for outputs (the project's standing bound); for gradients the rule of DESIGN.md §7l from the
float32 restatement's figure for the same quantity, computed once per batch size: 1e-5 under 2.5e-6, four times the
figure otherwise.  A weight gradient's sum is compared on the scale ||g|| sqrt(n) (it cancels); gradients that are
zero in exact arithmetic (sagan_refs.is_zero_grad) absolutely, on the scale of the largest fully recorded gradient."""
import pytest
import torch

import sagan_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OUT_TOL = 1e-4


def _models(B, need_attention=True):
    import fastfourierconvolution_amd as F
    G = F.SAGANGenerator(B, 32, R.Z_DIM, 64)
    D = F.SAGANDiscriminator(B, 32, 64)
    R.fill(G.state_dict(), 0)
    R.fill(D.state_dict(), 0)
    G.need_attention = D.need_attention = need_attention
    return G.to(DEV).train(), D.to(DEV).train()


def _ref_sds(B):
    import fastfourierconvolution_amd as F
    return (R.cast(R.fill(F.SAGANGenerator(B, 32, R.Z_DIM, 64).state_dict(), 0), torch.float64),
            R.cast(R.fill(F.SAGANDiscriminator(B, 32, 64).state_dict(), 0), torch.float64))


@pytest.fixture(scope="module")
def gold():
    return {B: (R.load(B), R.record(B, torch.float32)) for B in (2, 3)}


def _close(what, a, ref, tol=OUT_TOL):
    e = R.nerr(a, ref)
    print(f"OBS {what} {e:.3e} (bound {tol:.1e})")
    assert tuple(a.shape) == tuple(ref.shape), (what, tuple(a.shape), tuple(ref.shape))
    assert e <= tol, (what, e)


def _state(model, prefix, g, scenario, keys=("weight_u", "weight_v", "running_mean", "running_var")):
    for k, v in model.state_dict().items():
        if k.endswith(keys):
            _close(f"{scenario}{prefix}{k}", v, g[f"{scenario}{prefix}{k}"])
        elif k.endswith("num_batches_tracked") and f"{scenario}{prefix}{k}" in g:
            assert int(v) == int(g[f"{scenario}{prefix}{k}"])


def _grads(model, g, f32, scenario):
    full = [g[k].double().norm() for k in g if k.startswith(scenario + "grad/") and "#" not in k]
    scale0 = float(max(full))
    seen = 0
    for name, p in model.named_parameters():
        key = f"{scenario}grad/{name}"
        if p.grad is None:
            assert key not in g and key + "#sum" not in g, name
            continue
        grad = p.grad.detach().cpu().double()
        if key in g:
            if R.is_zero_grad(key):
                e = R.nerr(grad, g[key], absolute=True) / scale0
                print(f"OBS {key} zero in exact arithmetic: {e:.3e} of the largest bias gradient")
                assert e <= 1e-5, (key, e)
            else:
                _close(key, grad, g[key], R.bound(R.nerr(f32[key], g[key])))
        else:
            flat = grad.reshape(-1)
            tol = R.bound(R.nerr(f32[key + "#every97"], g[key + "#every97"]))
            _close(key + "#every97", flat[::R.STRIDE], g[key + "#every97"], tol)
            _close(key + "#norm", flat.norm(), g[key + "#norm"], R.bound(R.nerr(f32[key + "#norm"], g[key + "#norm"])))
            s = abs(float(flat.sum()) - float(g[key + "#sum"])) / (float(g[key + "#norm"]) * flat.numel() ** 0.5)
            print(f"OBS {key}#sum {s:.3e}")
            assert s <= tol, (key, s)
        seen += 1
    assert seen == sum(1 for k in g if k.startswith(scenario + "grad/") and not k.endswith(("#norm", "#every97")))


@pytest.mark.parametrize("B", (2, 3))
def test_generator_scenario_matches_the_reference(gold, B):
    g, f32 = gold[B]
    G, D = _models(B)
    z = R.inputs(B)[0].float().to(DEV)
    img, p2 = G(z)
    out, p1 = D(img)
    assert img.shape == (B, 3, 32, 32) and p2.shape == (B, 256, 256) and out.shape == (B,) and p1.shape == (B, 16, 16)
    assert not p2.requires_grad and not p1.requires_grad
    _close("img", img, g["g/img"])
    _close("d_out", out, g["g/d_out"])
    _close("p1", p1, g["g/p1"])
    _close("p2 rows", p2[:, ::R.P2_ROWS], g["g/p2#rows"])
    _close("p2 column sums", p2.double().sum(1), g["g/p2#colsum"])
    _state(G, "G.", g, "g/")
    _state(D, "D.", g, "g/")
    loss = -out.mean()
    loss.backward()
    _close("g_loss", loss, g["g/g_loss"])
    _grads(G, g, f32, "g/")


@pytest.mark.parametrize("B", (2, 3))
def test_critic_scenario_matches_the_reference(gold, B):
    g, f32 = gold[B]
    G, D = _models(B)
    _, z_d, real = R.inputs(B)
    d_real, _ = D(real.float().to(DEV))
    with torch.no_grad():
        fake, _ = G(z_d.float().to(DEV))
    d_fake, _ = D(fake)
    _close("d_real", d_real, g["d/d_real"])
    _close("d_fake", d_fake, g["d/d_fake"])
    lr, lf = torch.relu(1.0 - d_real).mean(), torch.relu(1.0 + d_fake).mean()
    (lr + lf).backward()
    _close("d_loss_real", lr, g["d/d_loss_real"])
    _close("d_loss_fake", lf, g["d/d_loss_fake"])
    _state(D, "D.", g, "d/")        # two refreshes
    _grads(D, g, f32, "d/")         # the first call's rank-one term uses the second call's u, v, as the reference's


def test_batch_of_one_eval_mode_and_need_attention():
    for B in (1, 2, 3):
        gsd, dsd = _ref_sds(B)
        z = R.inputs(B)[0]
        G, D = _models(B)
        G.eval()
        zg = z.float().to(DEV)
        u0 = G.l2[0].module.weight_u.detach().clone()
        with torch.no_grad():
            u8 = G(zg)
        assert u8.dtype == torch.uint8 and u8.shape == (B, 3, 32, 32)
        assert not torch.equal(G.l2[0].module.weight_u, u0), "u must advance in eval mode"
        img, _, new = R.generator(gsd, z, training=False)
        _close("eval u", G.l2[0].module.weight_u, new["l2.0.module.weight_u"])
        x = 255 * (img * 0.5 + 0.5)
        near = (x - x.round()).abs() < 1e-4
        differ = u8.cpu() != R.quantize(img)
        print(f"OBS B={B} uint8: {int(differ.sum())} differ, {int(near.sum())} of {near.numel()} near a step")
        assert float(near.double().mean()) < 0.01 and not bool((differ & ~near).any())
        # second forward, float image, from the advanced state; then the critic at this batch size
        with torch.no_grad():
            f = G.forward_float(zg)
            out, p1 = D(f)
        img2, _, _ = R.generator(gsd, z, training=False)
        _close("forward_float", f, img2)
        ro, rp1, _ = R.discriminator(dsd, img2)
        assert out.dim() == (0 if B == 1 else 1) and tuple(out.shape) == tuple(ro.shape)
        _close("critic output", out, ro)
        _close("p1", p1, rp1)
    # need_attention = False: None in the matrix's place, the same bits
    G, D = _models(2)
    G2, D2 = _models(2, need_attention=False)
    z = R.inputs(2)[0].float().to(DEV)
    img, p2 = G(z)
    img2, none = G2(z)
    assert none is None and p2 is not None and torch.equal(img, img2)
    out, p1 = D(img)
    out2, none = D2(img2)
    assert none is None and p1 is not None and torch.equal(out, out2)


def _iteration(dtype, B):
    """trainer.py:93-168 (hinge) with SGD(lr = 1) in the restatement: D half on the fill state, then the G half on
    the updated critic -> (losses, D's gradients, G's gradients, D's u / v after, G's state after)"""
    z_g, z_d, real = (t.to(dtype) for t in R.inputs(B))
    gsd, dsd = (R.cast(sd, dtype) for sd in _ref_sds(B))
    d = R.leaves(dsd)
    with torch.no_grad():
        fake, _, gnew = R.generator(gsd, z_d)
    o_real, _, _ = R.discriminator(d, real)
    o_fake, _, _ = R.discriminator(d, fake)
    lr, lf = R.d_losses(o_real, o_fake)
    (lr + lf).backward()
    d_grads = {k: d[k].grad for k in R.trained(d) if d[k].grad is not None}
    cond_d = R.GAMMA_COND["attn1"]      # of the second recorded critic call; the first adds to the same sum
    d2 = {k: (v.detach() - d_grads[k] if k in d_grads else v.detach()) for k, v in d.items()}
    g = R.leaves(R.advance(gsd, gnew))
    img, _, gnew2 = R.generator(g, z_g)
    o, _, dnew = R.discriminator(d2, img)
    lg = R.g_loss(o)
    lg.backward()
    g_grads = {k: g[k].grad for k in R.trained(g)}
    conds = {"attn1": cond_d, "attn2": R.GAMMA_COND["attn2"]}
    return (lr.detach(), lf.detach(), lg.detach()), d_grads, g_grads, dnew, gnew2, conds


def _check_deltas(prefix, before, after, grads, grads32, conds):
    """parameter deltas under SGD(lr = 1) against the float64 gradients.  Bound: the gradient rule of §7l from the
    float32 restatement's figure for the same gradient, plus the rounding of p - g and of before - after, each
    at most half an ulp of p per element: 2^-23 ||p|| / ||g||.  A gradient that is zero in exact arithmetic
    (float64 leaves it below 1e-12 of the largest): absolutely, 1e-5 of the largest gradient's norm plus
    2^-23 ||p||.  A parameter the iteration does not reach keeps its bits.
    gamma's gradient is the inner product <dy, o> of the attention layer's output gradient and its unscaled output.
    dy is itself only good to the gradient rule's 1e-5 normwise, so by Cauchy-Schwarz <dy, o> is good to
    1e-5 ||dy|| ||o|| / |<dy, o>| relative: that condition number (sagan_refs.GAMMA_COND, from the float64 backward)
    times 1e-5 is gamma's bound where it is the larger one.  After D's SGD(lr = 1) step the sum cancels hard."""
    top = max(float(x.norm()) for x in grads.values() if x is not None)
    figs = {k: R.nerr(grads32[k], gr) for k, gr in grads.items() if gr is not None and float(gr.norm()) >= 1e-12 * top}
    for k, gr in grads.items():
        p0 = before[prefix + k]
        delta = (p0 - after[prefix + k]).cpu().double()
        if gr is None:
            assert torch.equal(p0, after[prefix + k]), k
        elif float(gr.norm()) < 1e-12 * top:
            e = float((delta - gr).norm())
            print(f"OBS step {prefix}{k} zero in exact arithmetic: {e:.3e} (largest gradient {top:.3e})")
            assert e <= 1e-5 * top + 2.0 ** -23 * float(p0.double().norm()), (k, e)
        else:
            tol = R.bound(figs[k])
            if k.endswith(".gamma"):
                cond = conds[k[:-len(".gamma")]]
                print(f"OBS {prefix}{k}: ||dy|| ||o|| / |<dy, o>| = {cond:.2f}, float32 figure {figs[k]:.2e}")
                tol = max(tol, 1e-5 * cond)
            tol += 2.0 ** -23 * float(p0.double().norm()) / float(gr.norm())
            _close("step " + prefix + k, delta, gr, tol)


def test_sagan_step_matches_the_restatement():
    from fastfourierconvolution_amd import training
    B = 2
    z_g, z_d, real = R.inputs(B)
    dev = lambda t: t.float().to(DEV)

    def run():
        G, D = _models(B, need_attention=False)
        before = {k: v.detach().clone() for m, n in ((G, "G."), (D, "D.")) for k, v in
                  ((n + k, p) for k, p in m.named_parameters())}
        oG = torch.optim.SGD([p for p in G.parameters() if p.requires_grad], lr=1.0)
        oD = torch.optim.SGD([p for p in D.parameters() if p.requires_grad], lr=1.0)
        losses = training.sagan_step(G, D, oG, oD, dev(z_d), dev(z_g), dev(real))
        after = {n + k: v.detach().clone() for m, n in ((G, "G."), (D, "D.")) for k, v in m.state_dict().items()}
        assert all(p.requires_grad == (not k.endswith(("weight_u", "weight_v"))) for k, p in D.named_parameters())
        return before, after, [l.detach().clone() for l in losses]

    before, after, losses = run()
    _, after2, losses2 = run()
    for k in after:
        assert torch.equal(after[k], after2[k]), f"two runs from the same state differ: {k}"
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2))

    _, d_grads32, g_grads32, _, _, _ = _iteration(torch.float32, B)
    want, d_grads, g_grads, dnew, gnew2, conds = _iteration(torch.float64, B)
    for got, ref, what in zip(losses, want, ("d_loss_real", "d_loss_fake", "g_loss")):
        _close(what, got, ref)
    _check_deltas("D.", before, after, d_grads, d_grads32, conds)
    _check_deltas("G.", before, after, g_grads, g_grads32, conds)
    for k, v in dnew.items():       # three refreshes of D
        _close("D." + k, after["D." + k], v)
    for k, v in gnew2.items():      # two refreshes of G, BN statistics updated in both halves
        if k.endswith("num_batches_tracked"):
            assert int(after["G." + k]) == 2
        else:
            _close("G." + k, after["G." + k], v)
    G, D = _models(B)
    with pytest.raises(NotImplementedError, match="double backward"):
        training.sagan_step(G, D, None, None, dev(z_d), dev(z_g), dev(real), adv_loss="wgan-gp")


def test_reference_checkpoint_keys_load_strictly_and_reproduce():
    import fastfourierconvolution_amd as F
    G, D = _models(2)
    z = R.inputs(2)[0].float().to(DEV)
    sdG = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}     # the reference's key set
    sdD = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    img, p2 = G(z)
    out, p1 = D(img)
    G2, D2 = F.SAGANGenerator(2, 32, R.Z_DIM, 64), F.SAGANDiscriminator(2, 32, 64)
    G2.load_state_dict(sdG, strict=True)
    D2.load_state_dict(sdD, strict=True)
    G2, D2 = G2.to(DEV).train(), D2.to(DEV).train()
    img2, p22 = G2(z)
    out2, p12 = D2(img2)
    assert torch.equal(img, img2) and torch.equal(p2, p22) and torch.equal(out, out2) and torch.equal(p1, p12)


def test_forwards_capture_into_a_graph_and_replay():
    G, D = _models(2)
    Ge, De = _models(2)
    z = R.inputs(2)[0].float().to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():     # warm-up: plans, packs
        Gw, Dw = _models(2)
        Dw(Gw(z)[0])
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        img, p2 = G(z)
        out, p1 = D(img)
    eager = []
    with torch.no_grad():
        for _ in range(3):
            i, _ = Ge(z)
            o, q = De(i)
            eager.append((i.clone(), o.clone(), q.clone()))
    # the capture itself does not run; each replay is one forward from where u, v stand
    for r in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(img, eager[r][0]) and torch.equal(out, eager[r][1]) and torch.equal(p1, eager[r][2]), r
    assert not torch.equal(eager[0][0], eager[1][0]), "u and v must advance between forwards"


def test_one_table_per_model_forward():
    from fastfourierconvolution_amd import _runtime as rt
    G, D = _models(2)
    z = R.inputs(2)[0].float().to(DEV)
    with torch.no_grad():
        img, _ = G(z)
        D(img)
        obs = rt.LaunchObserver()
        rt.set_observer(obs)
        try:
            D(img)
            nd = [w for l, _, _, w in obs.records if l == "sn_weight"]
            G(z)
            ng = [w for l, _, _, w in obs.records if l == "sn_weight"][len(nd):]
        finally:
            rt.set_observer(None)
    # what rt.observe sees is one record per ffc_sn_forward call, so this observes ONE table per model forward (a
    # table per layer would leave three records).  That one call is three launches by construction, not by
    # observation: a table of at most 16 jobs in training mode launches colsum, matvec and scale once each
    # (csrc/sn_kernels.hip, ffc_sn_forward).
    assert len(nd) == 1 and len(ng) == 1
