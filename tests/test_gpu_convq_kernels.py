"""Kernel-level parity of ffc_convq_forward / ffc_convq_forward_split (csrc/convq_kernels.hip) against the
float64 references of tests/convq_cases.py (checked without a GPU in test_convq_cases_cpu.py), at the shapes
where the kernel or its host code changes path.  Jobs are built as test_gpu_convq.py builds them (ConvExec
and LaunchPlan with FFC_CONVQ_CFG / FFC_CONVQ_KSPLIT forced around construction and restored) and launched
through LaunchPlan.launch; lp.key, lp.cfg, lp.ksplit and lp.ntiles are asserted against the table.  No case
skips: a case that does not plan fails.

Every output and slab is prefilled with NaN and must come back NaN-free.  The kernel writes every slab row:
rows [pixel block * 4 + phase] for all ceil(B / NS) nrb ncb pixel blocks, {count, mean, M2, 0} per channel,
and {0, 0, 0, 0} where the phase has no valid pixel in the block; there is no row it is defined to leave.

Bound for normal inputs, per element: |out - ref| <= gamma S, S = sum |w| |x| + |bias| + |addend| (the same job
on absolute values), gamma from the arithmetic of ffc_internal.h:
  split3    x = hi + mid + lo exactly (24 significand bits = 8 + 8 + 8, truncating), |mid| < 2^-7 |x|,
            |lo| < 2^-14 |x|.  mfma_split3 adds six of the nine piece products; the dropped ones are
            |mid lo| + |lo mid| + |lo lo| < (2 2^-21 + 2^-28) |a b|:                      2^-20 + 2^-28
  MFMA      every piece product is exact in fp32; each of the 6 MFMAs of a 16-k step adds 16 of them to the
            accumulator.  One rounding of at most one ulp (2^-23: the rounding of the MFMA adder is not
            documented as to-nearest) is charged per accumulated product term, on partial sums bounded by S:
            6 Kpad terms, Kpad = 16 (4 staged chunks + direct chunks):                     6 Kpad 2^-23
  K split   ksplit - 1 additions of partial sums:                                          ksplit 2^-23
  epilogue  + bias, + addend, LeakyReLU's product with the fp32 slope:                      3 2^-23
so gamma = (6 Kpad + ksplit + 3) 2^-23 + 2^-20 + 2^-28 (1.8e-5 at Kpad 1600, 1.1e-6 + 4.6e-5 Kpad / 64 in
general).  Tanh / Sigmoid / GELU run as a second pass on the stored pre-activation: their Lipschitz constant
(1, 1/4, 1.13) times the bound above, plus the device function's own error, taken as 4 2^-23 max(1, |pre|)
absolute (GELU's 1 + erf cancels for negative arguments, so its error is absolute in |pre|), which is how
test_gpu_conv_kernels.py treats them under its normwise bound.  The project's normwise 1e-5 is asserted as
well.  Integer and one-hot inputs (convq_cases.py) must come back bit for bit.

Observed on the first MI355X run, cfg 0 / 1 / 2 / 3 (301 tests in 26 s: 5.5 s outside the four child
processes, about 5 s per child; no other test above 0.7 s):
  max |out - ref| / (gamma S)   6.9e-3  5.7e-3  6.3e-3  5.8e-3   (the bound charges a full rounding per product term)
  max normwise error            1.1e-6 under every cfg (ks33, K split 2, Tanh); bound 1e-5
  slab                          max |mean - ref| 1.7e-7, max relative variance error 2.4e-7
  integer / one-hot inputs      bit for bit under every cfg, K split and two-job launch, and in the children
  cfg 0..3 at ksplit 1          bit-identical on normal inputs (asserted: test_exact_cfgs_agree_bitwise_on_normal_inputs)

Case -> branch it is there for (convq_cases.CASES; every case under every cfg of FACTS)
  ch1 ch2 ch3 ch4 ch5 ch7   one staged segment of 1, 2, 3, 4, 5, 7 chunks (C 7, 20, 33, 64, 80, 100): the two
                   register slots and three LDS buffers of the staging pipeline, nst odd and even (npad rounds
                   up to whole rounds: padding periods that only meet barriers), C < 8 (channel half 1 loads
                   nothing), cfull false / true (ch4, ch5)
  seg2x1           two staged segments of one chunk: stage_setup and the compute side's segment change at
                   every chunk;  ct3seg: 2 + 1 staged chunks and a direct one
  st3d1 / stdrag   3 staged + 1 direct chunk;  a direct segment with C % 16 != 0 (masked channels)
  g1x4 g2x8 g3x4   inputs of 1, 2, 3 rows: phases that lose taps (zero-weight padded taps at the patch origin)
  g4x12 g5x20 g9x28   TC 12, 20, 28: the reciprocal division of q_geometry by non powers of two; H != W
  g12x4            tall input;  h24w8 / h22w8: nrb > 1, the last row block whole / ragged
  w68 w132         ncb > 1 (W 68 at TC 64 / 32, W 132 at TC 128), with a direct segment (w68)
  b5 b7 b11        ragged sample group at NS 2, 4 (4x4) and NS 8 (cfg 0 at 2x8)
  op12 op25        output_padding 1: PH differs per phase, and the last row block has rows of the py = 0
                   phases only: waves 2, 3 have no valid pixel, their slab rows are {0, 0, 0, 0}
  m1 .. m130       M < 32, M % 32 != 0, M % 64 != 0 under cfg 2, Mpad 256
  full70           every pixel block full (NS TR TC = 32 NTW, B % NS = 0): M-tiles 0 (and 32) take the
                   unmasked store path, the last one the masked path, in one launch
  pair             ct3seg + ct33 in one launch: nseg 3 / 1, 4 / 3 chunks, M 40 / 33, 8x8 / 16x16 outputs,
                   staging width by the larger job; post[j] (Tanh on one job), per-job slabs, ksplit 1, 2, 3
  ks6 ks33         K split 2, 3, 4, 8: convq_cases.KSPLITS lists every split's (staged, direct) chunks
  pers0 .. pers3   more than 4 x 256 tiles under their cfg: the tile-to-tile hand-off of the persistent loop;
                   also run with the tile table reversed (bitwise equal: no state survives a tile)
  rejections       every FFC_CHECK_ARG of ffc_convq_forward_split that one changed field can reach
  env children     FFC_CONVQ_PERSIST=0, FFC_CONVQ_PX=4, FFC_CONVQ_SLOTS11=3 | 4: the other template instances
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import conv_refs as cr
import convq_cases as cc
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAN = float("nan")
SLOPE = cr.SLOPE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -23
LIPSCHITZ = {0: 1.0, 1: 1.0, 2: 1.0, 3: 1.0, 4: 0.25, 5: 1.13}
_LIVE = []


def _mods():
    from fastfourierconvolution_amd import _lib, _plan, _runtime as rt
    return _lib, _plan, rt


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t):
    if t is None:
        return None
    _LIVE.append(t.to(DEV).contiguous())
    return _LIVE[-1]


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def gamma(case, ksplit=1):
    st, nd = cc.staged_direct(case)
    return (6 * 16 * (4 * sum(st) + nd) + ksplit + 3) * U + 2.0 ** -20 + 2.0 ** -28


@functools.lru_cache(maxsize=None)
def _inputs(name, builder, bias, addend, seed):
    """(segs, inputs, pre, S) of a case in float64, computed once; a persistent case's for its 7 distinct samples"""
    c = cc.CASES[name]
    segs = cc.segs_of(c)
    d = cc.BUILDERS[builder](min(c.B, cc.PERSIST_DISTINCT) if name in cc.PERSIST.values() else c.B, c.M, segs,
                             seed=seed, bias=bias, addend=addend)
    pre, _ = cc.job_ref(segs, d)
    return segs, d, pre, cc.abs_sum_ref(segs, d)


def _rep(t, B):
    """the batch of a persistent case: its distinct samples repeated"""
    return t if t is None or t.shape[0] == B else t.repeat(B // t.shape[0], *([1] * (t.dim() - 1)))


class Run:
    pass


def _launch(names, cfg, builder="normal", ksplit=1, acts=None, bias=False, addend=False, stats=False, seed=0,
            launch=True):
    """the cases as the jobs of one launch under (cfg, forced ksplit); -> Run(lp, jobs, per job: case, inputs,
    pre, S, out, slab)"""
    _lib, _plan, rt = _mods()
    acts = acts or [0] * len(names)
    env = {"FFC_CONVQ_CFG": str(cfg), "FFC_CONVQ_KSPLIT": str(ksplit)}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    r = Run()
    r.items, r.jobs, execs = [], [], []
    try:
        for name in names:
            c = cc.CASES[name]
            segs, d, pre, S = _inputs(name, builder, bias, addend, seed)
            bvec = _dev(d["bias"])
            wts = [(_dev(w), lay, w.shape[2], w.shape[3], bvec if i == 0 else None)
                   for i, (w, lay) in enumerate(zip(d["ws"], d["layouts"]))]
            execs.append(rt.ConvExec(c.B, c.M, segs, wts, DEV))
            assert execs[-1].launch_key == ("q", cfg), f"{name} has no convq plan under cfg {cfg}"
        lp = rt.LaunchPlan(execs, DEV)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    want_ks = min([ksplit] + [sum(cc.chunks(cc.CASES[n])) for n in names])
    assert lp.key == ("q", cfg) and lp.cfg == cfg and lp.ksplit == want_ks
    assert lp.ntiles == sum(cc.ntiles(cc.CASES[n], cfg, cc.FACTS[n][cfg], want_ks) for n in names)
    for j, (name, ex, act) in enumerate(zip(names, execs, acts)):
        c = cc.CASES[name]
        q = ex.plan
        assert (q.NS, q.TR, q.TC, q.nrb, q.ncb) == cc.FACTS[name][cfg][:5]
        segs, d, pre, S = _inputs(name, builder, bias, addend, seed)
        out = torch.full((c.B,) + tuple(pre.shape[1:]), NAN, device=DEV)
        assert lp.stat_rows(j) == q.npb * 4
        slab = torch.full((lp.stat_rows(j), c.M, 4), NAN, device=DEV) if stats else None
        xs = [(_dev(_rep(x, c.B)), None) for x in d["xs"]]
        r.jobs.append(ex.job(xs, out, act, SLOPE, _dev(_rep(d["addend"], c.B)), slab))
        r.items.append((name, c, act, pre, S, out, slab))
    r.lp, r.cfg, r.ksplit, r.execs = lp, cfg, want_ks, execs
    if launch:
        lp.launch(r.jobs, _stream())
        torch.cuda.synchronize()
    return r


MAXIMA = {}


def _check(r, what):
    """the elementwise and normwise bounds of every job of a launch, and its slab"""
    for name, c, act, pre, S, out, slab in r.items:
        assert not torch.isnan(out).any(), f"{what} {name}: unwritten (NaN) output elements"
        pre_d, S_d = pre.to(DEV), S.to(DEV)
        ref = cr.act64(pre_d, act, SLOPE)
        g = gamma(c, r.ksplit)
        bound = LIPSCHITZ[act] * g * S_d + (4 * U * pre_d.abs().clamp_min(1) if act >= 3 else 0)
        o = out.double().reshape((-1,) + tuple(pre.shape))       # (repeats, distinct samples, M, OH, OW)
        diff = (o - ref).abs()
        ratio = float((diff / bound).max())
        nerr = max(normwise_err(oo.cpu(), ref.cpu()) for oo in o[:: max(1, o.shape[0] - 1)])
        print(f"OBS convq {what} {name} cfg{r.cfg} ks{r.ksplit} act{act} ratio {ratio:.3e} normwise {nerr:.3e}")
        m = MAXIMA.setdefault(r.cfg, [0.0, 0.0])
        m[0], m[1] = max(m[0], ratio), max(m[1], nerr)
        assert (diff <= bound).all(), (what, name, ratio)
        assert nerr <= 1e-5, (what, name, nerr)
        if slab is not None:
            _check_slab(f"{what} {name} cfg{r.cfg}", slab, pre, c, cc.FACTS[name][r.cfg])


def _check_slab(what, slab, pre, c, facts):
    """every row written; the count column exactly; rows without a valid pixel all zero; the merged rows are the
    statistics of the pre-activation output (n exact, mean and variance at rtol 1e-5 / atol 1e-6)"""
    assert not torch.isnan(slab).any(), f"{what}: unwritten slab rows"
    s = slab.cpu()
    counts = cc.slab_row_counts(c, facts)
    assert torch.equal(s[..., 0].double(), counts[:, None].expand(-1, c.M)), what
    assert (s[..., 3] == 0).all() and (s[counts == 0] == 0).all(), what
    n, mean, var = cr.merge_slab(s)
    full = _rep(pre, c.B)
    n0, mean0, var0 = cr.channel_stats(full)
    assert torch.equal(n, torch.full_like(n, n0)), (what, n, n0)
    print(f"OBS convq_stats {what} mean {(mean - mean0).abs().max():.3e} var {((var - var0).abs() / var0).max():.3e}")
    torch.testing.assert_close(mean, mean0, rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} mean: {m}")
    torch.testing.assert_close(var, var0, rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} var: {m}")


def _cases(*names):
    return [(n, cfg) for n in names for cfg in sorted(cc.FACTS[n])]


# --------------------------------------------------------------------------- chunk pipeline, geometry, M
@pytest.mark.parametrize("name,cfg", _cases("ch1", "ch2", "ch3", "ch4", "ch5", "ch7", "seg2x1", "st3d1", "stdrag", "ct3seg"))
def test_chunk_pipeline(name, cfg):
    _check(_launch([name], cfg, seed=cfg + 1), "chunks")


@pytest.mark.parametrize("name,cfg", _cases("g1x4", "g2x8", "g3x4", "g4x12", "g5x20", "g12x4", "g9x28", "w68", "w132",
                                            "h24w8", "h22w8", "b5", "b7", "b11"))
def test_geometry(name, cfg):
    _check(_launch([name], cfg, bias=True, stats=True, seed=cfg + 2), "geometry")


@pytest.mark.parametrize("name,cfg", _cases("op12", "op25"))
def test_waves_without_a_valid_pixel_write_zero_rows(name, cfg):
    r = _launch([name], cfg, addend=True, stats=True, seed=3)
    _check(r, "empty waves")
    if (name, cfg) in (("op25", 0), ("op12", 1), ("op12", 2), ("op12", 3)):
        assert (r.items[0][6][-2:].cpu() == 0).all()


@pytest.mark.parametrize("name,cfg", _cases("m1", "m31", "m32", "m33", "m64", "m70", "m130", "full70"))
def test_output_channels(name, cfg):
    r = _launch([name], cfg, bias=True, stats=True, seed=4)
    if name == "full70":     # all pixels valid: the unmasked and the masked store path in one launch
        NS, TR, TC = cc.FACTS[name][cfg][:3]
        assert NS * TR * TC == 32 * cc.CFGS[cfg][1] and r.items[0][1].B % NS == 0 and 70 % (32 * cc.CFGS[cfg][0])
    _check(r, "M")


# --------------------------------------------------------------------------- epilogue
@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("bias,addend", [(True, False), (False, True), (True, True)])
def test_bias_addend(cfg, bias, addend):
    _check(_launch(["ct3seg"], cfg, bias=bias, addend=addend, seed=5), f"bias{int(bias)} addend{int(addend)}")


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4, 5])
def test_activations_with_slab(cfg, act):
    """the slab describes the pre-activation values under every activation"""
    assert sorted(cr.ACT.values()) == [0, 1, 2, 3, 4, 5]
    _check(_launch(["ct3seg"], cfg, acts=[act], bias=True, addend=True, stats=True, seed=6), "act")


# --------------------------------------------------------------------------- two jobs in one launch
@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("ksplit", [1, 2, 3])
@pytest.mark.parametrize("acts", [(0, 0), (2, 3), (3, 1)])
def test_two_jobs_in_one_launch(cfg, ksplit, acts):
    names = list(cc.PAIRS["pair"][0])
    r = _launch(names, cfg, ksplit=ksplit, acts=list(acts), bias=True, stats=True, seed=7)
    tiles = r.lp.tiles.cpu()
    assert set(tiles[:, 0].tolist()) == {0, 1}
    _check(r, f"pair acts{acts}")


# --------------------------------------------------------------------------- K split
@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("name,ksplit", sorted(cc.KSPLITS))
def test_ksplit(name, ksplit, cfg):
    """every split kind of convq_cases.KSPLITS with bias + addend + slab + activation; a second launch is
    bit-identical (nothing accumulates in the partial buffer)"""
    r = _launch([name], cfg, ksplit=ksplit, acts=[2 if ksplit % 2 else 3], bias=True, addend=True, stats=True, seed=8)
    assert r.ksplit == len(cc.KSPLITS[(name, ksplit)]) == min(ksplit, sum(cc.chunks(cc.CASES[name])))
    _check(r, "ksplit")
    first, slab1 = r.items[0][5].clone(), r.items[0][6].clone()
    r.lp.launch(r.jobs, _stream())
    torch.cuda.synchronize()
    assert torch.equal(r.items[0][5], first) and torch.equal(r.items[0][6], slab1)


# --------------------------------------------------------------------------- persistent loop
@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("builder", ["normal", "integer"])
def test_persistent_loop(cfg, builder):
    """more tiles than can be resident (4 workgroups of 512 threads per CU is a bound, not a measurement): every
    workgroup runs several tiles.  The same jobs with the tile table reversed give the same bits."""
    _lib, _plan, rt = _mods()
    name = cc.PERSIST[cfg]
    r = _launch([name], cfg, builder=builder, bias=True, addend=True, stats=builder == "normal", seed=9)
    assert r.lp.ntiles > 4 * torch.cuda.get_device_properties(DEV).multi_processor_count
    assert r.lp.ntiles > cc.PERSIST_BOUND
    out = r.items[0][5]
    if builder == "normal":
        _check(r, "persistent")
    else:
        pre = r.items[0][3]
        assert torch.equal(out.reshape((-1,) + tuple(pre.shape)), pre.float().to(DEV).expand(out.shape[0] // pre.shape[0], *pre.shape))
    first = out.clone()
    out.fill_(NAN)
    flipped = torch.flip(r.lp.tiles, [0]).contiguous()
    arr = (_lib.ConvPJob * 1)(*r.jobs)
    _lib.check(rt.lib().ffc_convq_forward(arr, 1, flipped.data_ptr(), r.lp.ntiles, cfg, _stream()), "ffc_convq_forward")
    torch.cuda.synchronize()
    assert torch.equal(out, first)


# --------------------------------------------------------------------------- exactness
EXACT = {"ct3seg": (["ct3seg"], 1), "pair": (list(cc.PAIRS["pair"][0]), 1), "ks6": (["ks6"], 3), "pers": (None, 1)}


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("builder", ["integer", "onehot_w", "onehot_x"])
@pytest.mark.parametrize("target", sorted(EXACT))
def test_exact_inputs_come_back_bitwise(target, builder, cfg):
    """integer inputs: every partial sum is exact in fp32 in any order; one-hot inputs: each output element is one
    operand with a full 24-bit significand times a power of two, so hi + mid + lo must rebuild it"""
    names, ksplit = EXACT[target]
    names = names or [cc.PERSIST[cfg]]
    extra = dict(bias=True, addend=True) if builder == "integer" else {}
    r = _launch(names, cfg, builder=builder, ksplit=ksplit, acts=[1 if builder == "integer" else 0] * len(names), seed=10, **extra)
    for name, c, act, pre, S, out, slab in r.items:
        ref = cr.act64(pre, act).float().to(DEV)
        assert torch.equal(ref.double().cpu(), cr.act64(pre, act))     # the reference is an fp32 number
        got = out.reshape((-1,) + tuple(pre.shape))
        assert torch.equal(got, ref.expand_as(got)), (name, int((got != ref).sum()))


@pytest.mark.parametrize("name", ["ct3seg", "ks6", "g9x28"])
def test_exact_cfgs_agree_bitwise_on_normal_inputs(name):
    """every cfg adds the same products of an output element in the same order (chunk by chunk, tap by tap, six
    MFMAs per 16-k step): without a K split the four configurations give the same bits"""
    outs = [_launch([name], cfg, bias=True, seed=11).items[0][5] for cfg in sorted(cc.FACTS[name])]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


# --------------------------------------------------------------------------- rejections
def _rejections():
    """name -> (edit of a copy of (job list, launch arguments)); every one fails an FFC_CHECK_ARG"""
    def job(f):
        return lambda jobs, a: f(jobs[0])

    def arg(**kw):
        return lambda jobs, a: a.update(kw)

    def seg(i, **kw):
        def f(j):
            for k, v in kw.items():
                setattr(j.seg[i], k, v(getattr(j.seg[i], k)) if callable(v) else v)
        return job(f)

    def field(**kw):
        def f(j):
            for k, v in kw.items():
                setattr(j, k, v(getattr(j, k)) if callable(v) else v)
        return job(f)
    one = {
        "ksplit 0": arg(ksplit=0), "ksplit 9": arg(ksplit=9), "njobs 0": arg(njobs=0), "njobs 3": arg(njobs=3),
        "cfg 4": arg(cfg=4), "cfg -1": arg(cfg=-1), "ntiles 0": arg(ntiles=0),
        "A3 null": field(A3=None), "A3 misaligned": field(A3=lambda p: p + 2),
        "nphase 3": field(nphase=3), "Mpad 64": field(Mpad=64), "Mpad 192": field(Mpad=192),
        "pooled": seg(0, pool=1), "gated": seg(1, gate=lambda p: 16),
        "IW % 4": seg(0, IW=6), "x misaligned": seg(0, x=lambda p: p + 4),
        "direct off the output resolution": seg(2, IH=4), "pixel block": field(NS=100), "PC % 4": seg(0, PC=6),
        "units": seg(0, PR=200), "LDS": seg(0, qsample=1 << 14), "Cpad": seg(0, Cpad=24), "out null": field(out=None),
    }
    split = {
        "part null": arg(part=None), "part misaligned": arg(part=lambda p: p + 4),
        "nslots": arg(nslots=lambda n: n + 1), "slots null": arg(slots=None),
    }
    return one, split


@pytest.mark.parametrize("ksplit", [1, 2])
def test_rejections_leave_the_output_alone(ksplit):
    _lib, _plan, rt = _mods()
    L = rt.lib()
    r = _launch(["ct3seg"], 0, ksplit=ksplit, seed=12, launch=False)
    out, lp = r.items[0][5], r.lp
    one, split = _rejections()
    for what, edit in (one if ksplit == 1 else split).items():
        jobs = [_lib.ConvPJob.from_buffer_copy(r.jobs[0]) for _ in range(3)]
        a = dict(njobs=1, ntiles=lp.ntiles, cfg=0, ksplit=lp.ksplit, nslots=lp.nslots,
                 tiles=lp.tiles.data_ptr(), slots=None if lp.slots is None else lp.slots.data_ptr(),
                 part=None if lp.part is None else lp.part.data_ptr())
        before = dict(a)
        edit(jobs, a)
        for k, v in list(a.items()):     # callables edit the valid value
            if callable(v):
                a[k] = v(before[k])
        arr = (_lib.ConvPJob * 3)(*jobs)
        rc = L.ffc_convq_forward_split(arr, a["njobs"], a["tiles"], a["ntiles"], a["slots"], a["nslots"], a["cfg"],
                                       a["ksplit"], a["part"], _stream())
        assert rc == -1, what        # FFC_E_INVALID
        assert b"ffc_convq_forward" in L.ffc_last_error(), what
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    lp.launch(r.jobs, _stream())     # the unedited job runs
    torch.cuda.synchronize()
    _check(r, "after rejections")


# --------------------------------------------------------------------------- env-selected instantiations
@pytest.mark.parametrize("setting", ["FFC_CONVQ_PERSIST=0", "FFC_CONVQ_PX=4", "FFC_CONVQ_SLOTS11=3", "FFC_CONVQ_SLOTS11=4"])
def test_env_selected_kernels_in_subprocess(setting):
    """the library reads these once per process: a fresh child runs the exactness and chunk-pipeline cases on
    the template instances the setting selects (one workgroup per tile; 4-pixel staging units everywhere,
    cfg 3 included; 3 / 4 staging register slots under cfg 3)"""
    k, v = setting.split("=")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "exact or chunk_pipeline"], cwd=ROOT, env=dict(os.environ, **{k: v}),
                       capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    last = r.stdout.splitlines()[-1]
    assert " passed" in last and "skipped" not in last and "failed" not in last, tail
