"""The kernel-level attention references, inputs and error measures of tests/attn_refs.py (core_ref,
core_bwd_ref, abi_case, shares), proven without a GPU for tests/test_gpu_attn_abi.py:

  - core_ref / core_bwd_ref against float64 autograd to 1e-12 (normwise; results that are zero in mathematics
    against their cancellation scale), and against attn_ref / attn_ref_backward through a projection;
  - the room: on every input of the GPU file the same operation in plain float32 (torch matmul, softmax,
    logsumexp, the gradients from the formulas), and the tile-by-tile float32 walk of the forward, stay within
    a quarter (attn_refs.ROOM) of every bound.  An input that misses is changed, never the bound.  Largest
    share reached: 0.199 (dq of 1x40x1x255); 0.18 on the directed inputs (dq of the negative offset); 0.009
    (L) and 0.005 (y) on the sampled rows of N = 65536, so that case keeps the common bound and needs no count
    of its chain of 2048 rescaled additions;
  - the directed inputs do what they claim, and their float32 scores equal the float64 scores;
  - nine float32 emulations with one planted defect each exceed the bound they are meant to trip (the
    smallest margin: L off by 1e-4 reaches 2.7 times the L bound; every other defect passes 1e4 times);
  - fma_f32 is fmaf, ties included.
Every test prints what it measured.
"""
import pytest
import torch

import attn_refs as R


def _fp32_all(c, defect=None):
    got = dict(R.fp32_forward(c, defect))
    got.update(R.fp32_backward(c, defect))
    return got


@pytest.mark.parametrize("name", ["1x8x1x1", "3x40x1x33", "2x64x6x6", "3x24x3x43", "offset", "late_max", "gamma_neg",
                                  "gamma_zero"])
def test_core_refs_match_autograd_fp64(name):
    c = R.abi_case(name)
    q, k, v, x = (c[n].double().requires_grad_(True) for n in "qkvx")
    gamma = torch.tensor(float(c["gamma"]), dtype=torch.float64, requires_grad=True)
    S = torch.bmm(q.transpose(1, 2), k)
    P = torch.softmax(S, -1)
    o = torch.bmm(v, P.transpose(1, 2))
    y = gamma * o + x
    (y * c["dy"].double()).sum().backward()
    f, w = c["fwd"], c["bwd"]
    errs = {"y": R.normwise(f["y"], y), "o": R.normwise(f["o"], o), "P": R.normwise(f["P"], P),
            "L": R.normwise(f["L"], torch.logsumexp(S, -1)), "S": R.normwise(f["S"], S),
            "P = exp(S - L)": R.normwise(torch.exp(f["S"] - f["L"][:, :, None]), P),
            "dv": R.normwise(w.dv, v.grad) if c["gamma"] else float(v.grad.abs().max()),
            "dgamma": abs(float(w.dgamma - gamma.grad)) / float(w.dgamma_scale),
            "D": R.normwise(w.D, (c["gamma"] * c["dy"].double() * o).sum(1)) if c["gamma"] else float(w.D.abs().max())}
    for n, ref, g, z in (("dq", w.dq, q.grad, w.dq_zero), ("dk", w.dk, k.grad, w.dk_zero)):
        errs[n] = float((ref - g).abs().max() / z.max().clamp_min(1e-300))
        assert bool((getattr(w, n + "_scale") <= z * (1 + 1e-12) + 1e-300).all()), "|dS| exceeds its own scale"
    assert bool(torch.equal(x.grad, c["dy"].double()))
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-12, errs


@pytest.mark.parametrize("name", ["b3_c16_6x6", "b2_c32_10x10", "mask"])
def test_core_refs_match_the_layer_refs_through_a_projection(name):
    c = R.case(name)
    r, g = c["ref"], c["grads"]
    B, C, H, W = c["x"].shape
    gamma = float(c["p"]["gamma"])
    y, L, o, P, S = R.core_ref(r["q"], r["k"], r["v"], c["x"], gamma)
    w = R.core_bwd_ref(c["dy"], r["q"], r["k"], r["v"], gamma)
    xf = c["x"].double().reshape(B, C, -1)
    errs = {"out": R.normwise(y, r["out"]), "attention": R.normwise(P, r["attention"]), "o": R.normwise(o, r["o"]),
            "gamma": R.normwise(w.dgamma, g["gamma"])}
    for n, dz in (("query_conv", w.dq), ("key_conv", w.dk), ("value_conv", w.dv)):
        errs[n + ".weight"] = R.normwise(torch.einsum("bmn,bcn->mc", dz, xf), g[n + ".weight"])
    errs["key_conv.bias.scale"] = R.normwise(w.dk.abs().sum((0, 2)), g["key_conv.bias.scale"])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-12, errs


@pytest.mark.parametrize("name", R.ABI_ALL)
def test_every_gpu_input_leaves_room_under_the_bounds(name):
    """proves the inputs, not the kernel: plain float32 reaches at most a quarter of each bound"""
    c = R.abi_case(name)
    S = c["fwd"]["S"]
    B, C, H, W = c["shape"]
    assert c["q"].shape == (B, C // 8, H * W) and c["v"].shape == (B, C, H * W) and c["q"].dtype == torch.float32
    if name in R.ABI_RANDOM or name == R.GRID_LIMIT:
        assert float(S.abs().max()) <= 11.5
        if H * W > 1:
            assert 1.0 <= float(S.std(unbiased=False)) <= 3.0
    floor = name in ("early_max", "late_max")
    plain = R.shares(c, _fp32_all(c), p_floor=floor)
    flash = R.shares(c, R.fp32_flash(c))
    print(name, f"max |S| {float(S.abs().max()):.1f}", "plain", {k: f"{v:.3f}" for k, v in plain.items()},
          "tiled", {k: f"{v:.3f}" for k, v in flash.items()})
    assert max(plain.values()) <= R.ROOM and max(flash.values()) <= R.ROOM, (plain, flash)
    if name == "gamma_zero":
        got = _fp32_all(c)
        assert torch.equal(got["y"], c["x"]) and all(float(got[k].abs().max()) == 0.0 for k in ("dq", "dk", "dv"))


def test_the_limit_input_leaves_room_on_its_sampled_rows():
    c = R.limit_case()
    assert c["shape"] == (1, 8, 256, 256) and c["rows"][:32].tolist() == list(range(32))
    assert c["rows"][32:64].tolist() == list(range(65504, 65536))
    got = R.limit_fp32(c)
    lim = R.TOL * (c["y"].abs() + c["y"].pow(2).mean().sqrt())
    sh = {"L": R.L_share(got["L"], c["L"]), "y": float(((got["y"].double() - c["y"]).abs() / lim).max())}
    print("N = 65536", sh)
    assert max(sh.values()) <= R.ROOM, sh


@pytest.mark.parametrize("name", R.EXACT_SCORES)
def test_directed_scores_are_exact_in_float32(name):
    c = R.abi_case(name)
    S = c["fwd"]["S"]
    assert torch.equal((c["q"].transpose(1, 2) @ c["k"]).double(), S), "float32 scores differ from float64"
    chain = torch.zeros(S.shape)
    for r in range(c["q"].shape[1]):                    # the kernel's k-ordered fmaf chain, one rounding a step
        chain = R.fma_f32(c["q"][:, r, :, None].expand(S.shape), c["k"][:, r, None, :].expand(S.shape), chain)
    assert torch.equal(chain.double(), S), "the fmaf chain over r differs from float64"
    print(name, f"scores in [{float(S.min()):.1f}, {float(S.max()):.1f}]")


def test_directed_inputs_do_what_they_claim():
    for name, lo, hi in (("offset", 96.0, 104.0), ("neg_offset", -104.0, -96.0)):
        S = R.abi_case(name)["fwd"]["S"]
        assert lo <= float(S.min()) and float(S.max()) <= hi and float(S.max() - S.min()) >= 4.0, name
    assert R.abi_case("neg_offset")["shape"][3] == 33
    early, late = R.abi_case("early_max")["fwd"]["S"], R.abi_case("late_max")["fwd"]["S"]
    N = early.shape[-1]
    assert N == 257 and bool((early[0, :, 1:] - early[0, :, :-1] == -0.5).all()) and bool((early[0, :, 0] == 0).all())
    assert torch.equal(late, early.flip(-1))
    assert float(torch.exp(early[0, 0, 175:] - early[0, 0].logsumexp(-1)).max()) < 2.0 ** -126   # float32 flushes
    c = R.abi_case("one_hot")
    S, perm = c["fwd"]["S"][0], R.one_hot_perm(129)
    assert sorted(perm.tolist()) == list(range(129))
    hit = torch.zeros(129, 129, dtype=torch.bool)
    hit[torch.arange(129), perm] = True
    assert bool((S[hit] == R.ONE_HOT_HIT).all()) and float(S[~hit].max()) == R.ONE_HOT_REST
    assert len({int(p) // 32 for p in perm[:32]}) > 1 and len({(int(p) % 32) // 4 % 2 for p in perm[:32]}) == 2
    assert float((c["fwd"]["o"] - c["v"].double()[:, :, perm]).abs().max()) <= 1e-15
    u = R.abi_case("uniform")["fwd"]
    assert float((u["P"] - 1 / 129).abs().max()) <= 1e-17 and float((u["L"] - torch.log(torch.tensor(129.0).double())).abs().max()) <= 1e-14
    assert R.abi_case("gamma_neg")["gamma"] < 0 and R.abi_case("gamma_zero")["gamma"] == 0.0
    assert float(R.abi_case("gamma_zero")["bwd"].dgamma.abs()) > 1.0


@pytest.mark.parametrize("defect", list(R.DEFECTS))
def test_a_planted_defect_exceeds_its_bound(defect):
    name, trips = R.DEFECTS[defect]
    c = R.abi_case(name)
    if defect in R.FLASH_DEFECTS:
        clean, got = R.shares(c, R.fp32_flash(c)), R.shares(c, R.fp32_flash(c, defect))
    else:
        clean, got = R.shares(c, _fp32_all(c)), R.shares(c, _fp32_all(c, defect))
    print(defect, "on", name, {k: f"{got[k]:.3g} (clean {clean[k]:.3f})" for k in trips})
    assert max(clean.values()) <= R.ROOM
    for k in trips:
        assert got[k] > 1.0, f"the {k} bound lets '{defect}' through"


def test_fma_f32_is_fmaf():
    one, u = torch.tensor([1.0]), 2.0 ** -24
    # 1 + u (1 + 2^-23): just above the tie between 1 and 1 + 2u -> rounds up; rounding the float64 sum
    # (1 + u exactly, a tie) a second time would give 1
    a = torch.tensor([1.0 + 2.0 ** -23])
    assert float(R.fma_f32(u, a, one)) == 1.0 + 2 * u
    assert float(R.fma_f32(u, one, one)) == 1.0                           # an exact tie goes to even
    assert float(R.fma_f32(-u, a, torch.tensor([1.0 + 2 * u]))) == 1.0    # just below the tie above 1
    gen = torch.Generator().manual_seed(7)
    g, a, x = 0.7, torch.randn(4096, generator=gen), torch.randn(4096, generator=gen)
    ref = (torch.tensor(g, dtype=torch.float32).double() * a.double() + x.double()).float()
    assert int((R.fma_f32(g, a, x) != ref).sum()) == 0                     # no tie among random operands
    assert torch.equal(R.fma_f32(0.0, a, x), x)
