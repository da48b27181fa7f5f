"""tests/convq_cases.py against the planner and against torch (no GPU): every case of the table plans under
the cfgs it lists, with the plan facts written next to it; its job satisfies every argument check of
ffc_convq_forward_split (restated below from csrc/convq_kernels.hip); the must-not-plan shapes do not
plan; the branch sets the table reaches equal the lists written out here (a case edited away fails
loudly); the integer builder is exact by its own condition; the references agree with
torch.nn.functional in float64."""
import pytest
import torch
import torch.nn.functional as F

import conv_refs as cr
import convq_cases as cc
from fastfourierconvolution_amd import _plan

ALL = sorted((n, cfg) for n, per in cc.FACTS.items() for cfg in per)


def _plan_of(name, cfg):
    c = cc.CASES[name]
    return c, _plan.plan_convq_job(c.B, c.M, cc.segs_of(c), cfg)


def test_every_case_has_facts_and_every_fact_a_case():
    assert set(cc.FACTS) == set(cc.CASES)
    assert all(per for per in cc.FACTS.values())
    assert _plan.CONVQ_CFGS == cc.CFGS and _plan.CONVQ_MAX_UNITS == cc.MAX_UNITS


@pytest.mark.parametrize("name,cfg", ALL)
def test_case_plans_with_the_expected_facts(name, cfg):
    c, q = _plan_of(name, cfg)
    assert q is not None and q.q, f"{name} does not plan under cfg {cfg}"
    NS, TR, TC, nrb, ncb, width = cc.FACTS[name][cfg]
    assert (q.NS, q.TR, q.TC, q.nrb, q.ncb) == (NS, TR, TC, nrb, ncb)
    assert tuple(cp // 16 for cp in q.cpad) == cc.chunks(c) and _plan.convq_chunks(q) == sum(cc.chunks(c))
    assert q.direct == [s[0] == "pw" for s in c.segs]
    u4 = max([2 * q.NS * pr * (pc // 4) for (pr, pc), d in zip(q.prc, q.direct) if not d])
    assert u4 == cc.units4(c, cc.FACTS[name][cfg]) <= cc.MAX_UNITS
    assert cc.stage_width(cfg, u4) == width
    tiles = _plan.build_patch_tiles([q])
    assert tiles.shape[0] == cc.ntiles(c, cfg, cc.FACTS[name][cfg])
    assert sorted(map(tuple, tiles[:, :3])) == sorted((0, m0, pb) for pb in range(q.npb) for m0 in range(0, c.M, 32 * q.mt))


def check_args(q, cfg, ntiles, ksplit=1, nslots=0):
    """every FFC_CHECK_ARG of ffc_convq_forward_split that depends on the plan (pointers and their alignment
    are the runtime's: ConvExec.job, test_gpu_convq_kernels.py), on the job struct ConvExec.base_job fills"""
    MT, NTW = cc.CFGS[cfg]
    assert ntiles > 0 and 0 <= cfg <= 3 and 1 <= ksplit <= 8
    assert ksplit == 1 or (nslots > 0 and nslots * ksplit == ntiles)
    assert q.B > 0 and q.M > 0 and len(q.phases) == 4 and (q.Sy, q.Sx) == (2, 2)
    assert 1 <= len(q.segs) <= 3 and q.Mpad % 128 == 0 and q.Mpad >= q.M
    assert q.NS * q.M * q.OH * q.OW * 4 < 0xFFFFFFFF
    assert min(q.NS, q.TR, q.TC, q.nrb, q.ncb) > 0 and q.NS * q.TR * q.TC <= 32 * NTW
    npix = 0
    for ph in q.phases:
        assert ph["Kpad"] % 16 == 0
    for i, sg in enumerate(q.segs):
        assert q.cpad[i] % 16 == 0 and q.cpad[i] >= sg.C and q.cc[i] == 16 and not sg.pool and not sg.gate
        assert all(ph["T"][i] == (1 if q.direct[i] else 4) for ph in q.phases)
        if q.direct[i]:
            assert q.mults[i] == (2, 2) and (sg.IH, sg.IW) == (q.OH, q.OW)
            continue
        PR, PC = q.prc[i][0], q.rowlen[i]
        qrow, qsample = q.qstride[i]
        assert PR > 0 and PC > 0 and PC % 4 == 0 and qrow >= PC and qsample >= PR * qrow
        assert q.vec4[i] and sg.IW % 4 == 0 and q.B * sg.C * sg.IH * sg.IW * 4 < 0x7FFFFFFF
        assert 2 * q.NS * PR * (PC // 4) <= 256
        npix = max(npix, q.NS * qsample)
    assert 3 * ((npix * 96 + 255) // 256 * 256 + 256) <= 160 * 1024


@pytest.mark.parametrize("name,cfg", ALL)
def test_case_passes_every_argument_check(name, cfg):
    c, q = _plan_of(name, cfg)
    check_args(q, cfg, _plan.build_patch_tiles([q]).shape[0])


@pytest.mark.parametrize("key", sorted(cc.KSPLITS))
def test_ksplit_ranges(key):
    name, forced = key
    c = cc.CASES[name]
    ks = min(forced, sum(cc.chunks(c)))
    assert cc.split_ranges(c, ks)[0] == cc.KSPLITS[key]
    assert sum(a + b for a, b in cc.KSPLITS[key]) == sum(cc.chunks(c))
    for cfg in cc.FACTS[name]:
        q = _plan_of(name, cfg)[1]
        tiles = _plan.build_patch_tiles([q], ksplit=ks)
        slots = _plan.convq_slot_tiles(tiles)
        assert tiles.shape[0] == cc.ntiles(c, cfg, cc.FACTS[name][cfg], ks) == slots.shape[0] * ks
        check_args(q, cfg, tiles.shape[0], ks, slots.shape[0])


@pytest.mark.parametrize("pair", sorted(cc.PAIRS))
def test_pairs_share_a_launch(pair):
    names, cfgs = cc.PAIRS[pair]
    for cfg in cfgs:
        qs = [_plan_of(n, cfg)[1] for n in names]
        assert all(q is not None for q in qs)
        u4 = max(cc.units4(cc.CASES[n], cc.FACTS[n][cfg]) for n in names)
        assert cc.stage_width(cfg, u4) == cc.PAIR_WIDTH[pair][cfg]
        tiles = _plan.build_patch_tiles(qs)
        assert tiles.shape[0] == sum(cc.ntiles(cc.CASES[n], cfg, cc.FACTS[n][cfg]) for n in names)
        a, b = (cc.CASES[n] for n in names)   # the two jobs differ in everything a tile hand-off depends on
        assert len(a.segs) != len(b.segs) and sum(cc.chunks(a)) != sum(cc.chunks(b)) and a.M != b.M
        assert a.segs[0][2:4] != b.segs[0][2:4]


@pytest.mark.parametrize("name", sorted(cc.NO_PLAN))
def test_must_not_plan(name):
    B, M, segs, reason = cc.NO_PLAN[name]
    for cfg in cc.NO_PLAN_CFGS.get(name, (0, 1, 2, 3)):
        assert _plan.plan_convq_job(B, M, [_plan.Seg(*s) for s in segs], cfg) is None, reason


def test_pointwise_off_the_output_resolution_is_refused():
    """a 1x1 that is not at the output resolution never reaches plan_convq_job's own test: plan_job, which it
    calls first, refuses the job for every kernel"""
    for cfg in range(4):
        with pytest.raises(ValueError):
            _plan.plan_convq_job(2, 40, [_plan.Seg(*cc.T(9, 4, 4)), _plan.Seg(*cc.P(6, 4, 4))], cfg)


def test_coverage_is_what_is_written_here():
    every = {0, 1, 2, 3}
    assert cc.coverage() == {
        # cfg 3 never has more than 128 units (NS TR TC <= 32), so its 4-pixel kernel is FFC_CONVQ_PX = 4 only
        "cfg_width": {(0, 2), (0, 4), (1, 2), (1, 4), (2, 2), (2, 4), (3, 1), (3, 2)},
        "cfg_persistent": every,
        "nst": {(0, 0), (1, 1), (0, 2), (1, 3), (0, 4), (1, 5), (1, 7)},
        "split_kinds": {"staged only", "direct only", "both", "starts mid-segment", "starts in a later segment"},
        "nrb>1": every, "ncb>1": every, "ragged B % NS": every, "ragged rows": every,
        "NS*TR*TC < 32*NTW": every, "NS*TR*TC == 32*NTW": every, "C < 8": every, "C % 16 != 0": every,
        "direct C % 16 != 0": every, "njobs=2": every,
    }
    for cfg, name in cc.PERSIST.items():
        assert list(cc.FACTS[name]) == [cfg]
        assert cc.ntiles(cc.CASES[name], cfg, cc.FACTS[name][cfg]) > cc.PERSIST_BOUND
    # waves without a valid pixel: the output_padding cases' last row block, phases py = 1
    for name, cfg in (("op25", 0), ("op12", 1), ("op12", 2), ("op12", 3)):
        n = cc.slab_row_counts(cc.CASES[name], cc.FACTS[name][cfg])
        assert n[-4:].tolist()[2:] == [0.0, 0.0] and n[-4] > 0 and n.sum() == 9 * (2 * cc.CASES[name].segs[0][2] + 1)


@pytest.mark.parametrize("name", ["ct3seg", "ks6", "ct33", "pers3", "op12"])
def test_integer_builder_is_exact(name):
    c = cc.CASES[name]
    B = min(c.B, cc.PERSIST_DISTINCT)
    segs = cc.segs_of(c)
    d = cc.integer(B, c.M, segs, seed=1, bias=True, addend=True)   # asserts S < 2^24 UNIT itself
    pre, _ = cc.job_ref(segs, d)
    assert torch.equal(pre.float().double(), pre)                        # the result is an fp32 number
    assert torch.equal((pre / cc.UNIT).round(), pre / cc.UNIT)           # and a multiple of UNIT
    for t in d["xs"] + d["ws"]:
        hi, mid, lo = (cr.bf16_to_f64(p) for p in cr.split_bf16_ref(t.numpy()))
        assert (hi != 0).all() and (mid != 0).all() and (lo == 0).all()


@pytest.mark.parametrize("builder", ["onehot_w", "onehot_x"])
def test_onehot_builders(builder):
    c = cc.CASES["ct3seg"]
    segs = cc.segs_of(c)
    d = cc.BUILDERS[builder](c.B, c.M, segs, seed=2)
    full = d["xs"] if builder == "onehot_w" else d["ws"]
    for t in full:   # all 24 significand bits in use, and the three pieces reconstruct the value
        a = t.numpy()
        pieces = [cr.bf16_to_f64(p) for p in cr.split_bf16_ref(a)]
        assert (pieces[0] + pieces[1] + pieces[2] == a.astype("float64")).all() and (pieces[2] != 0).mean() > 0.9
    assert any((t.view(torch.int32) == 0x3F7FFFFF).any() for t in full)
    pre, _ = cc.job_ref(segs, d)
    assert torch.equal(pre.float().double(), pre) and (pre != 0).any()
    S = cc.abs_sum_ref(segs, d)
    assert torch.equal(S, pre.abs())                                     # one term per output element


@pytest.mark.parametrize("name", ["ct3seg", "w68", "op12", "g1x4"])
def test_references_agree_with_torch(name):
    c = cc.CASES[name]
    segs = cc.segs_of(c)
    d = cc.normal(c.B, c.M, segs, seed=3, bias=True, addend=True)

    def torch_job(xs, ws, bias, addend):
        ref = 0
        for s, x, w in zip(segs, xs, ws):
            ref = ref + (F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1, output_padding=s.op)
                         if s.kind == "convT" else F.conv2d(x.double(), w.double()))
        return ref + bias.double()[None, :, None, None] + addend.double()
    pre, out = cc.job_ref(segs, d, cr.ACT["TANH"])
    want = torch_job(d["xs"], d["ws"], d["bias"], d["addend"])
    torch.testing.assert_close(pre, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(out, torch.tanh(want), rtol=1e-12, atol=1e-12)
    S = cc.abs_sum_ref(segs, d)
    torch.testing.assert_close(S, torch_job([x.abs() for x in d["xs"]], [w.abs() for w in d["ws"]], d["bias"].abs(),
                                            d["addend"].abs()), rtol=1e-12, atol=1e-12)
    assert (S >= pre.abs() * (1 - 1e-12)).all()
    n, mean, m2 = cc.slab_ref(pre)
    assert n == pre.numel() // c.M
    torch.testing.assert_close(mean, want.mean(dim=(0, 2, 3)), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(m2, ((want - want.mean(dim=(0, 2, 3), keepdim=True)) ** 2).sum(dim=(0, 2, 3)), rtol=1e-10, atol=1e-10)
    for cfg, f in cc.FACTS[name].items():   # the slab's count column adds up to the output's pixels
        assert cc.slab_row_counts(c, f).sum() == n
