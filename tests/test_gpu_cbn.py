"""Conditional batch norm on the GPU: the kernels of csrc/cbn_kernels.hip against float64 at the shapes
where they change path, the label guard, the reference's fixtures (tests/golden/gen_golden_cbn.py), the
default / set_cond_bn rule, reproducibility of the embedding gradient, hipGraph replay with rewritten
labels, torch.library.opcheck of the two ops, and the four models of fgan_cond_complete.py with one
conditional G + D hinge step.

Bounds: kernels against float64 1e-5 normwise (the bound tests/test_gpu_train_kernels.py applies to
ffc_bn_bwd; kink-free inputs by its rule, constants from tests/train_refs.py); modules and models 1e-4
normwise in fp32.  Every test prints the errors it measured.

Observed maxima on the first MI355X run (normwise): kernels 2.5e-7 ((6, 8, 1) Sigmoid d table), the
reference's fixtures 4.7e-7 (cbn_conv3 gin.x), models 2.7e-6 (CondDiscriminator32 dx), the hinge step 3.9e-6 (loss_G).
"""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import cbn_refs as R
import train_refs as tr
from conftest import GOLDEN
from fixture_weights import input_array, make_state
from oracle.ffc_oracle import normwise_err, quantize_u8

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_K = 1e-5    # kernels against float64
TOL_M = 1e-4    # modules / models, fp32

with open(os.path.join(GOLDEN, "manifest_cbn.json")) as f:
    MANIFEST = json.load(f)
CASES = {c["name"]: c for c in MANIFEST["cases"]}


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _err(what, out, ref):
    out = out.detach().cpu().double().reshape(ref.shape)
    assert not torch.isnan(out).any(), what
    e = normwise_err(out, ref)
    print(f"  {what}: {e:.2e}")
    return e


# --------------------------------------------------------------------------- kernels through the C ABI
def _lib():
    from fastfourierconvolution_amd import _lib
    return _lib, _lib.load()


def _dev(inp, train):
    sc, sh = R.kernel_consts(inp, train)
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    d["scale0"], d["shift0"] = sc.to(DEV), sh.to(DEV)
    return d


def _item(L, d, y, act, noise, labels=None):
    B, C, HW = d["x"].shape
    lab = d["labels"] if labels is None else labels
    p = L.ptr
    return L.CbnApplyItem(p(d["x"]), p(y), B, C, HW, d["table"].shape[0], p(d["scale0"]), p(d["shift0"]),
                          p(d["table"]), p(lab), act, tr.SLOPE, p(d["noise_w"]) if noise else None,
                          p(d["noise"]) if noise else None)


def _apply(items):
    L, lib = _lib()
    arr = (L.CbnApplyItem * len(items))(*items)
    L.check(lib.ffc_cbn_act_apply_batch(arr, len(items), torch.cuda.current_stream().cuda_stream), "cbn apply")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", R.KERNEL_SHAPES)
@pytest.mark.parametrize("train", [True, False])
def test_forward_apply_matches_fp64(shape, train):
    """every activation code, with and without noise, out of place and in place"""
    L, _ = _lib()
    worst = 0.0
    for act in tr.ACTS:
        inp = R.kernel_inputs(shape, 3, train)
        d = _dev(inp, train)
        for noise in (False, True):
            ref = R.kernel_forward(inp, act, train, noise)
            y = torch.empty_like(d["x"])
            _apply([_item(L, d, y, act, noise)])
            worst = max(worst, _err(f"{shape} act={act} noise={noise}", y, ref))
            x2 = dict(d, x=d["x"].clone())
            _apply([_item(L, x2, x2["x"], act, noise)])
            assert torch.equal(x2["x"], y), "in place differs from out of place"
    assert worst <= TOL_K


@pytest.mark.parametrize("K", [1, 9])
def test_forward_k1_and_more_classes_than_samples(K):
    L, _ = _lib()
    inp = R.kernel_inputs((3, 5, 7), K, True)
    d = _dev(inp, True)
    y = torch.empty_like(d["x"])
    _apply([_item(L, d, y, 5, True)])
    assert _err(f"K={K}", y, R.kernel_forward(inp, 5, True, True)) <= TOL_K


def test_forward_batched_two_items():
    """bn_l and bn_g of one layer: two items of different C and HW (plane form + scalar form) in one launch"""
    L, _ = _lib()
    ia, ib = R.kernel_inputs((2, 4, 256), 3, True), R.kernel_inputs((2, 3, 7), 3, True, seed=1)
    da, db = _dev(ia, True), _dev(ib, True)
    ya, yb = torch.empty_like(da["x"]), torch.empty_like(db["x"])
    _apply([_item(L, da, ya, 2, True), _item(L, db, yb, 5, False)])
    assert _err("item 0", ya, R.kernel_forward(ia, 2, True, True)) <= TOL_K
    assert _err("item 1", yb, R.kernel_forward(ib, 5, True, False)) <= TOL_K


def _backward(d, act, train, labels=None):
    """sums, d table, dx through the C ABI"""
    L, lib = _lib()
    B, C, HW = d["x"].shape
    K = d["table"].shape[0]
    lab = d["labels"] if labels is None else labels
    st = torch.cuda.current_stream().cuda_stream
    p = L.ptr
    args = (p(d["x"]), p(d["dy"]), p(lab), p(d["table"]), B, C, HW, K, p(d["scale0"]), p(d["shift0"]), act, tr.SLOPE)
    sums = torch.empty(B, 2 * C, device=DEV)
    dtable = torch.empty(K, 2 * C, device=DEV)
    dx = torch.empty_like(d["x"])
    L.check(lib.ffc_cbn_bwd_sums(*args, p(sums), st), "sums")
    L.check(lib.ffc_embed_scatter_rows(p(sums), p(lab), B, K, 2 * C, p(dtable), st), "scatter")
    coef = None
    if train:
        coef = torch.empty(C, 2, device=DEV)
        L.check(lib.ffc_cbn_bwd_coeff(p(sums), p(lab), p(d["table"]), B, C, HW, K, p(coef), st), "coeff")
    L.check(lib.ffc_cbn_bwd_apply(*args, p(coef), p(dx), st), "apply")
    torch.cuda.synchronize()
    return sums, dtable, dx


@pytest.mark.parametrize("shape", R.KERNEL_SHAPES + [(2, 3, 1028)])
@pytest.mark.parametrize("train", [True, False])
def test_backward_matches_fp64(shape, train):
    """(2, 3, 1028): the workgroup-per-plane form of the sums (HW > 1024)"""
    worst = 0.0
    for act in tr.ACTS:
        for K in ((3,) if act else (1, 3, 70)):
            inp = R.kernel_inputs(shape, K, train)
            sums, dtable, dx = _backward(_dev(inp, train), act, train)
            rs, rt_, rdx = R.kernel_formulas(inp, act, train)
            worst = max(worst, _err(f"{shape} act={act} K={K} sums", sums, rs),
                        _err(f"{shape} act={act} K={K} dtable", dtable, rt_),
                        _err(f"{shape} act={act} K={K} dx", dx, rdx))
            absent = torch.ones(K, dtype=torch.bool)
            absent[inp["labels"]] = False
            assert torch.all(dtable.cpu()[absent] == 0), "absent classes must be exact zeros"
    assert worst <= TOL_K


def test_out_of_range_labels_are_guarded():
    """labels -1 and K beside valid ones: valid samples unchanged, bad samples NaN, the embedding gradient
    that of the valid samples alone.  The kernels never form an address from such a label."""
    L, _ = _lib()
    K = 3
    inp = R.kernel_inputs((6, 8, 16), K, True)
    d = _dev(inp, True)
    y = torch.empty_like(d["x"])
    _apply([_item(L, d, y, 5, True)])
    bad = d["labels"].clone()
    bad[1], bad[4] = -1, K
    yb = torch.empty_like(d["x"])
    _apply([_item(L, d, yb, 5, True, labels=bad)])
    ok = [0, 2, 3, 5]
    assert torch.equal(yb[ok], y[ok])
    assert torch.isnan(yb[[1, 4]]).all()
    sums, dtable, _ = _backward(d, 5, True)
    sums_b, dtable_b, _ = _backward(d, 5, True, labels=bad)
    assert torch.equal(sums_b[ok], sums[ok])
    ref = torch.zeros_like(dtable)
    for b in ok:   # sample order, as the scatter sums
        ref[int(d["labels"][b])] += sums[b]
    assert torch.equal(dtable_b, ref)


def test_embedding_gradient_is_reproducible():
    """bitwise identical over two runs; a permutation of the samples moves the rows only by the rounding
    of the fixed-order sums (bound: B ulps of the row's largest term); absent classes exact zeros"""
    K, shape = 7, (12, 6, 64)
    inp = R.kernel_inputs(shape, K, True)
    inp["labels"] = torch.tensor([0, 3, 3, 5, 0, 3, 5, 5, 0, 3, 6, 6])   # classes 1, 2, 4 absent (GELU: no kinks)
    d = _dev(inp, True)
    s1, t1, x1 = _backward(d, 5, True)
    s2, t2, x2 = _backward(d, 5, True)
    assert torch.equal(s1, s2) and torch.equal(t1, t2) and torch.equal(x1, x2)
    perm = torch.randperm(shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)
    dp = dict(d, x=d["x"][perm].contiguous(), dy=d["dy"][perm].contiguous(), labels=d["labels"][perm].contiguous())
    sp, tp, _ = _backward(dp, 5, True)
    assert torch.equal(sp, s1[perm]), "per-sample sums do not depend on the sample's position"
    bound = shape[0] * 2.0 ** -23 * s1.abs().max().item()
    print(f"  permuted rows differ by {(tp - t1).abs().max().item():.2e} (bound {bound:.2e})")
    assert (tp - t1).abs().max().item() <= bound
    absent = torch.ones(K, dtype=torch.bool)
    absent[inp["labels"]] = False
    assert absent.any() and torch.all(t1.cpu()[absent] == 0)


# --------------------------------------------------------------------------- ops
def test_opcheck():
    x = torch.randn(4, 6, 4, 4, device=DEV, requires_grad=True)
    labels = torch.tensor([2, 0, 2, 1], device=DEV)
    emb = torch.randn(3, 12, device=DEV, requires_grad=True)
    rm, rv = torch.zeros(6, device=DEV), torch.ones(6, device=DEV)
    nw = torch.randn(1, 6, 1, 1, device=DEV, requires_grad=True)
    nz = torch.randn(4, 1, 4, 4, device=DEV)
    for use_batch, act, noise in ((True, 5, True), (False, 2, False), (True, 0, False)):
        args = (x, labels, emb, rm, rv, use_batch, 1e-5, act, 0.1) + ((nw, nz) if noise else (None, None))
        torch.library.opcheck(torch.ops.ffc.cbn_act.default, args)
    _, sc, sh, _ = torch.ops.ffc.cbn_act(x.detach(), labels, emb.detach(), rm, rv, True, 1e-5, 5, 0.0, None, None)
    torch.library.opcheck(torch.ops.ffc.cbn_act_backward.default,
                          (x.detach(), torch.randn_like(x), labels, emb.detach(), sc, sh, True, 5, 0.0, True, True))


# --------------------------------------------------------------------------- fixtures of the reference
def _build(c, state=None):
    import fastfourierconvolution_amd as F
    kw = dict(c["ctor"])
    for k in ("norm_layer", "activation_layer"):
        if k in kw:
            kw[k] = F.ConditionalBatchNorm2d if kw[k] == "ConditionalBatchNorm2d" else getattr(nn, kw[k])
    mod = _quiet(getattr(F, c["kind"]), **kw)
    state = make_state(c["seed"], c["specs"]) if state is None else state
    mod.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return mod.to(DEV).train(c["mode"] == "train")


def _bias_aware_err(k, got, data):
    """a conv bias in front of batch statistics has an analytically vanishing gradient: its error is
    taken relative to the same conv's weight gradient (as in tests/test_cbn_cpu.py)"""
    want = torch.from_numpy(data[k]).double()
    if k.startswith("gpar.") and k.endswith(".bias"):
        e = (got.detach().cpu().double() - want).abs().max().item() / float(np.abs(data[k[:-4] + "weight"]).max())
        print(f"  {k}: {e:.2e} (of the weight gradient)")
        return e
    return _err(k, got, want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases(name):
    """forward, running buffers, input and parameter gradients; default mode (no set_cond_bn): the
    reference runs these"""
    c = CASES[name]
    data = np.load(os.path.join(GOLDEN, name + ".npz"))
    mod = _build(c)
    labels = torch.tensor(c["labels"], device=DEV).view(c["label_shape"])
    tin = {k: torch.from_numpy(input_array(c["seed"], k, s)).to(DEV).requires_grad_(True)
           for k, s in c["inputs"].items()}
    out = mod(tin["x"] if "x" in tin else (tin["x_l"], tin["x_g"]), labels)
    outs = {"out": out} if isinstance(out, torch.Tensor) else \
        {n: o for n, o in zip(("out_l", "out_g"), out) if isinstance(o, torch.Tensor)}
    loss = sum((o * torch.from_numpy(input_array(c["seed"] + 11, "cot:" + n, list(o.shape))).to(DEV)).sum()
               for n, o in outs.items())
    loss.backward()
    got = {"ref." + n: o for n, o in outs.items()}
    got.update({"gin." + k: t.grad for k, t in tin.items()})
    got.update({"gpar." + k: p.grad for k, p in mod.named_parameters()})
    got.update({"after." + k: v for k, v in mod.state_dict().items()})
    worst = 0.0
    for k in data.files:
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(data[k])
            continue
        assert got[k] is not None, k
        worst = max(worst, _bias_aware_err(k, got[k], data))
    assert worst <= TOL_M
    with torch.no_grad():   # the no-grad path (the fused inference kernels of the FFC part)
        mod = _build(c)
        x = {k: t.detach() for k, t in tin.items()}
        out2 = mod(x["x"] if "x" in x else (x["x_l"], x["x_g"]), labels)
    outs2 = {"out": out2} if isinstance(out2, torch.Tensor) else \
        {n: o for n, o in zip(("out_l", "out_g"), out2) if isinstance(o, torch.Tensor)}
    for n, o in outs2.items():
        assert _err("no_grad ref." + n, o, torch.from_numpy(data["ref." + n]).double()) <= TOL_M
    for k, v in mod.state_dict().items():
        if "after." + k in data.files and not k.endswith("num_batches_tracked"):
            assert _err("no_grad after." + k, v, torch.from_numpy(data["after." + k]).double()) <= TOL_M


def test_label_shapes_and_b1():
    import fastfourierconvolution_amd as F
    m = F.ConditionalBatchNorm2d(6, 3).to(DEV).eval()
    x = torch.randn(4, 6, 3, 3, device=DEV)
    y = torch.tensor([2, 0, 1, 1], device=DEV)
    a = m(x, y)
    assert torch.equal(a, m(x, y.view(4, 1))) and torch.equal(a, m(x, y.view(4, 1, 1)))
    with pytest.raises(IndexError):
        m(x[:1], y[:1].view(1, 1, 1))
    with pytest.raises(F._lib.FFCError):
        m(x, y.cpu())


# --------------------------------------------------------------------------- default / opt-in rule
SPECTRAL = dict(in_channels=32, out_channels=16, kernel_size=4, ratio_gin=0.25, ratio_gout=0.25, stride=2, padding=1,
                activation_layer="GELU", norm_layer="ConditionalBatchNorm2d", upsampling=True, num_classes=4)


def _spectral_case(mode="train"):
    import fastfourierconvolution_amd as F
    c = dict(kind="FFC_BN_ACT", ctor=SPECTRAL, mode=mode, seed=99)
    blk = _quiet(F.FFC_BN_ACT, **{**SPECTRAL, "activation_layer": nn.GELU, "norm_layer": F.ConditionalBatchNorm2d})
    from gen_golden import weight_specs
    specs = {}
    for nme, m in blk.named_modules():
        pre = nme + "." if nme else ""
        if isinstance(m, nn.Embedding):
            specs[pre + "weight"] = [list(m.weight.shape), "normal", 0.6, 0.4, "float32"]
        elif not list(m.children()) and m.state_dict():
            specs.update({pre + k: v for k, v in weight_specs(m).items() if k in m.state_dict()})
    c["specs"] = specs
    return c


def test_default_raises_and_opt_in_matches_fp64():
    """a label reaching a SpectralTransform: TypeError by default (the reference's); with set_cond_bn the
    layer runs (global branch: the fused Fourier unit on the 8x8 plane) and matches the float64 composition"""
    import fastfourierconvolution_amd as F
    c = _spectral_case()
    state = make_state(c["seed"], c["specs"])
    xl = torch.from_numpy(input_array(99, "x_l", [4, 24, 4, 4]))
    xg = torch.from_numpy(input_array(99, "x_g", [4, 8, 4, 4]))
    labels = torch.tensor([3, 1, 1, 0])
    nl, ng = torch.from_numpy(input_array(99, "nl", [4, 1, 8, 8])), torch.from_numpy(input_array(99, "ng", [4, 1, 8, 8]))
    wl, wg = torch.from_numpy(input_array(99, "wl", [1, 12, 1, 1])), torch.from_numpy(input_array(99, "wg", [1, 4, 1, 1]))
    for grad in (False, True):
        mod = _build(c, state)
        with pytest.raises(TypeError, match="SpectralTransform"):
            mod((xl.to(DEV), xg.to(DEV)), labels.to(DEV))
        F.set_cond_bn(mod)
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}
        sd = {k: v.double() if v.is_floating_point() else v.clone() for k, v in sd.items()}
        sd["nl.weight"], sd["ng.weight"] = wl.double(), wg.double()
        rl, rg = R.ffc_bn_act_cond((xl.double(), xg.double()), sd, "", SPECTRAL, labels, True,
                                   {"l": ("nl.weight", nl.double()), "g": ("ng.weight", ng.double())})
        nil, nig = F.NoiseInjection(12).to(DEV), F.NoiseInjection(4).to(DEV)
        with torch.no_grad():
            nil.weight.copy_(wl)
            nig.weight.copy_(wg)
        with torch.set_grad_enabled(grad):
            ol, og = mod.forward_noise((xl.to(DEV), xg.to(DEV)), (nil, nl.to(DEV)), (nig, ng.to(DEV)), labels.to(DEV))
        assert _err(f"grad={grad} out_l", ol, rl) <= TOL_M and _err(f"grad={grad} out_g", og, rg) <= TOL_M
        for k in ("bn_l.bn.running_mean", "bn_g.bn.running_var", "ffc.convg2g.fu.bn.running_var"):
            assert _err(k, mod.state_dict()[k], sd[k]) <= TOL_M


def test_hipgraph_replays_with_rewritten_labels():
    import fastfourierconvolution_amd as F
    c = _spectral_case("eval")
    mod = F.set_cond_bn(_build(c))
    xl, xg = torch.randn(4, 24, 4, 4, device=DEV), torch.randn(4, 8, 4, 4, device=DEV)
    labels = torch.tensor([0, 1, 2, 3], device=DEV)
    with torch.no_grad():
        mod((xl, xg), labels)   # plans, packed weights
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mod((xl, xg), labels)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ol, og = mod((xl, xg), labels)
        labels.copy_(torch.tensor([3, 3, 0, 1], device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        el, eg = mod((xl, xg), labels)
    assert torch.equal(ol, el) and torch.equal(og, eg)
    with torch.no_grad():
        fl, _ = mod((xl, xg), torch.tensor([0, 1, 2, 3], device=DEV))
    assert not torch.equal(fl, el), "the labels must matter"


# --------------------------------------------------------------------------- models
def _model_state(mod, seed):
    """deterministic float32 state for a model: gen_golden's per-layer distributions, embeddings N(0.6, 0.4)"""
    from gen_golden import weight_specs
    specs = {}
    for nme, m in mod.named_modules():
        pre = nme + "." if nme else ""
        if isinstance(m, nn.Embedding):
            specs[pre + "weight"] = [list(m.weight.shape), "normal", 0.6, 0.4, "float32"]
        elif hasattr(m, "weight_orig"):
            w = m.weight_orig
            specs[pre + "weight_orig"] = [list(w.shape), "normal", 0.0, w[0].numel() ** -0.5, "float32"]
            specs[pre + "weight_u"] = [list(m.weight_u.shape), "normal", 0.0, 1.0, "float32"]
            specs[pre + "weight_v"] = [list(m.weight_v.shape), "normal", 0.0, 1.0, "float32"]
            specs[pre + "bias"] = [list(m.bias.shape), "normal", 0.0, 0.1, "float32"]
        elif not list(m.children()) and m.state_dict():
            specs.update({pre + k: v for k, v in weight_specs(m).items() if k in m.state_dict()})
    assert set(specs) == set(mod.state_dict()), set(specs) ^ set(mod.state_dict())
    return make_state(seed, specs)


def _load(mod, state):
    mod.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return mod.to(DEV)


def _sd64(state):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}
    return {k: v.double() if v.is_floating_point() else v.clone() for k, v in sd.items()}


def _noises(B, mg, seed):
    return [(torch.from_numpy(input_array(seed, f"n{i}l", [B, 1, mg * 2 ** (i + 1), mg * 2 ** (i + 1)])),
             torch.from_numpy(input_array(seed, f"n{i}g", [B, 1, mg * 2 ** (i + 1), mg * 2 ** (i + 1)])))
            for i in range(3)]


@pytest.mark.parametrize("kind,mg,B", [("FCondGenerator32", 4, 4), ("FCondGeneratorSTL", 6, 2),
                                       ("FCondGeneratorSTL", 4, 4)])
def test_generators_match_fp64(kind, mg, B):
    """train with explicit noise, eval with the uint8 image; mg = 6: the 24 x 24 / 48 x 48 planes"""
    import fastfourierconvolution_amd as F
    K = 3
    G = _quiet(getattr(F, kind), 16, mg, K)
    state = _model_state(G, 5)
    G = _load(G, state)
    z = torch.from_numpy(input_array(5, "z", [B, 16]))
    labels = torch.tensor([2, 0, 2, 1][:B])
    stem = mg if kind == "FCondGeneratorSTL" else 4
    noises = _noises(B, stem, 5)
    sd = _sd64(state)
    G.train()
    with torch.no_grad():
        out = G(z.to(DEV), labels.to(DEV), [(a.to(DEV), b.to(DEV)) for a, b in noises])
    ref = R.cond_generator(z.double(), labels, sd, K, True, [(a.double(), b.double()) for a, b in noises],
                           stl_mg=mg if kind == "FCondGeneratorSTL" else None)
    assert tuple(out.shape) == (B, 3, 8 * stem, 8 * stem)
    assert _err(f"{kind} mg={mg} train", out, ref) <= TOL_M
    G.eval()
    with torch.no_grad():
        u8 = G(z.to(DEV), labels.to(DEV))
        fl = G.forward_float(z.to(DEV), labels.to(DEV))
    ref = R.cond_generator(z.double(), labels, sd, K, False, stl_mg=mg if kind == "FCondGeneratorSTL" else None)
    assert _err(f"{kind} mg={mg} eval", fl, ref) <= TOL_M
    assert u8.dtype == torch.uint8
    diff = (u8.cpu().int() - quantize_u8(ref).int()).abs()
    print(f"  uint8: max level difference {int(diff.max())}, share off {float((diff > 0).float().mean()):.2e}")
    assert int(diff.max()) <= 1 and float((diff > 0).float().mean()) <= 1e-3


@pytest.mark.parametrize("kind", ["CondDiscriminator32", "FCondDiscriminator32"])
def test_discriminators_match_fp64(kind):
    import fastfourierconvolution_amd as F
    K, B = 3, 4
    D = _quiet(getattr(F, kind), True, 4, K)
    state = _model_state(D, 6)
    D = _load(D, state).train()
    if hasattr(D, "gaus_noise"):
        D.gaus_noise.stddev = 0.0   # x + 0 * noise: the float64 composition has no noise
    x = torch.from_numpy(input_array(6, "x", [B, 3, 32, 32]))
    labels = torch.tensor([2, 0, 2, 1])
    sd = _sd64(state)
    xd = x.to(DEV).requires_grad_(True)
    out = D(xd, labels.to(DEV))
    out.sum().backward()
    x64 = x.double().requires_grad_(True)
    for k, v in sd.items():
        if v.is_floating_point() and not k.endswith(("running_mean", "running_var", "_u", "_v")):
            v.requires_grad_(True)
    ref = R.cond_discriminator(x64, labels, sd, True) if kind == "CondDiscriminator32" else \
        R.cond_fdiscriminator(x64, labels, sd, K, True)
    ref.sum().backward()
    assert _err(f"{kind} out", out, ref) <= TOL_M
    assert _err(f"{kind} dx", xd.grad, x64.grad) <= TOL_M
    assert _err(f"{kind} d label_embed", D.label_embed.weight.grad, sd["label_embed.weight"].grad) <= TOL_M
    if kind == "FCondDiscriminator32":
        for k in ("conv2.bn_l.embed.weight", "conv3.bn_g.embed.weight", "conv4.bn_l.embed.weight"):
            assert _err(k, dict(D.named_parameters())[k].grad, sd[k].grad) <= TOL_M


def test_conditional_hinge_step_matches_fp64():
    """one G step and one D step of the conditional pair (training.generator_step / discriminator_step with
    labels=): losses and layer-wise gradients against the float64 composition"""
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import training as T
    K, B = 3, 4
    G, D = _quiet(F.FCondGenerator32, 16, 4, K), _quiet(F.FCondDiscriminator32, True, 4, K)
    gs, ds = _model_state(G, 7), _model_state(D, 8)
    G, D = _load(G, gs).train(), _load(D, ds).train()
    D.gaus_noise.stddev = 0.0
    oG = torch.optim.SGD(G.parameters(), lr=0.0)
    oD = torch.optim.SGD(D.parameters(), lr=0.0)
    z = torch.from_numpy(input_array(7, "z", [B, 16]))
    real = torch.from_numpy(input_array(7, "real", [B, 3, 32, 32]))
    labels = torch.tensor([2, 0, 2, 1])
    noises = _noises(B, 4, 7)
    dn = [(a.to(DEV), b.to(DEV)) for a, b in noises]
    n64 = [(a.double(), b.double()) for a, b in noises]

    def ref_sd(state, grad):
        sd = _sd64(state)
        if grad:
            for k, v in sd.items():
                if v.is_floating_point() and not k.endswith(("running_mean", "running_var", "_u", "_v")):
                    v.requires_grad_(True)
        return sd

    # generator step
    loss = T.generator_step(G, D, oG, oD, z.to(DEV), dn, labels.to(DEV))
    gsd, dsd = ref_sd(gs, True), ref_sd(ds, False)
    fake = R.cond_generator(z.double(), labels, gsd, K, True, n64)
    rloss = -R.cond_fdiscriminator(fake, labels, dsd, K, True).mean()
    rloss.backward()
    worst = _err("loss_G", loss.reshape(()), rloss.detach())
    for k, p in G.named_parameters():
        if k.endswith(".bias") and ("input_conv.0" in k or "label_conv.0" in k):
            continue   # a bias in front of batch statistics: the gradient vanishes analytically
        if p.grad is None or gsd[k].grad is None:   # parameters no forward uses (the never-run lfu)
            assert p.grad is None and gsd[k].grad is None, k
            continue
        worst = max(worst, _err("G " + k, p.grad, gsd[k].grad))
    assert worst <= TOL_M
    # discriminator step: the models' buffers (running statistics, u / v) moved on; the references follow
    gs2 = {k: v.detach().cpu().numpy() for k, v in G.state_dict().items()}
    ds2 = {k: v.detach().cpu().numpy() for k, v in D.state_dict().items()}
    loss = T.discriminator_step(G, D, oG, oD, z.to(DEV), real.to(DEV), dn, labels.to(DEV))
    gsd, dsd = ref_sd(gs2, False), ref_sd(ds2, True)
    with torch.no_grad():
        fake = R.cond_generator(z.double(), labels, gsd, K, True, n64)
    o_fake = R.cond_fdiscriminator(fake, labels, dsd, K, True)
    o_real = R.cond_fdiscriminator(real.double(), labels, dsd, K, True)
    rloss = torch.relu(1.0 - o_real).mean() + torch.relu(1.0 + o_fake).mean()
    rloss.backward()
    worst = _err("loss_D", loss.reshape(()), rloss.detach())
    for k, p in D.named_parameters():
        if k.endswith(".bias") and ".ffc." in k:
            continue   # conv biases in front of the conditional norms' batch statistics
        if p.grad is None or dsd[k].grad is None:
            assert p.grad is None and dsd[k].grad is None, k
            continue
        worst = max(worst, _err("D " + k, p.grad, dsd[k].grad))
    assert worst <= TOL_M
