"""Kernel-level parity of the forward convolution family on the GPU -- the generic phase GEMM
(csrc/conv_kernels.hip), the LDS-patch kernel (convp_kernels.hip), the tiled 1x1 GEMM (pw_gemm.hip), the
small-M direct kernels (convt_smallm.hip) and the weight packers -- each called through the C ABI against
a float64 CPU reference of the same operation (tests/conv_refs.py, itself checked in
test_conv_refs_cpu.py), with the kernel, tile configuration and host branch forced from the test side and
asserted from the plan.

Every output and slab is prefilled with NaN and must come back NaN-free.  Every returned tensor is
compared normwise (oracle.ffc_oracle.normwise_err), bound 1e-5 (exact-fp32 and fp32-accurate split-bf16
kernels).  Slabs are merged in float64 and compared with the statistics of the pre-activation output: n
exact, mean and variance at rtol 1e-5 / atol 1e-6.  Packers are compared exactly.

Observed maxima on the first MI355X run (normwise error, bound 1e-5 each; statistics as max |mean - ref| /
max relative variance error; 357 tests of this module in 3.5 s, no case above 0.4 s):
  a. generic GEMM   cfg 0 / 1 / 2: 3.8e-07 each (exact fp32 products: the tile shape does not change the sums);
                    stats 1.5e-07 / 1.3e-07 under every cfg
  b. LDS patch      split    cfg 0..3: 3.3e-07 3.3e-07 3.7e-07 3.7e-07   stats <= 1.5e-07 / 2.6e-07
                    presplit cfg 0..3: 3.3e-07 3.3e-07 3.7e-07 3.7e-07   stats <= 1.5e-07 / 2.6e-07
                    f32      cfg 0..3: 3.8e-07 3.8e-07 3.0e-07 3.0e-07   stats <= 1.5e-07 / 2.1e-07
  c. 1x1 GEMM       cfg 0 / 1 / 2: 3.7e-07 each
  d. convt smallm   1.3e-06 (C 128 + 128, M 4)
  e. conv3x3 smallm 2.7e-06 (C 128 + 128, 33x132);  _tf 5.0e-06 (C 128 + 128 with noise: GELU by the A&S 7.1.26
                    erf, |error| <= 1.5e-7, on 256 channels), 6.8e-07 at C 5 + 4
  f. packers        exact

Case -> branch it is there for
  a. ffc_conv_forward, every case under tile cfg 0 (128 x 128), 1 (64 x 128) and 2 (32 x 256), the tile table
     from _plan.build_tiles(plans, cfg) (rt.USE_PATCH = False: ex.kind == "gemm")
  c3_36 / c3_130   Conv2d k3 s1 p1, C 7, 5x7, B 2: K = 63 (Kpad 64), 70 pixels; M 36 / 130
  ragged           the same conv at 11x13, M 130: 286 pixels.  For every cfg: M % BM != 0, pixels % BN != 0,
                   K % 16 != 0, more than one M-tile and more than one N-tile (asserted)
  c4s2             Conv2d k4 s2 p1, C 5, 9x7, M 40: K = 80 = Kpad (no K padding), 4x3 outputs
  ct3seg           ConvT k4 s2 p1, C 20 + 12 at 4x4, plus 1x1 C 8 at 8x8, B 3, M 40: 4 phases, three segments
  ct1x1            ConvT k4 s1 p0 on a 1x1 input, C 10, B 3, M 70: 16 one-tap phases of 3 pixels
  ctop             ConvT k3 s2 p1 output_padding 1, C 3, 5x7: phases of 1, 2, 2 and 4 taps
  ctdil / cdil     ConvT k4 s1 p0 dilation 2, C 2, 5x5;  Conv2d k3 p2 dilation 2, C 4, 7x9
  pool / gate      1x1 with pool (C 6, 4x4 from 8x8) / gate (C 12, 5x3): the on-load branches of load_b
  poolgate         1x1 pool + gate beside an ungated 1x1 segment in one job
  allpad           ConvT k1 s2 p0, C 3, 3x4: phases (0, 1), (1, 0), (1, 1) meet no tap -- their k-table is one
                   PAD_ENTRY and the kernel writes bias / addend only (plan_job does produce such phases)
  epilogue         ct3seg per cfg: bias + addend + slab (ffc_conv_stat_rows_per_tile rows per tile) under
                   act 0 / 1 / 2 / 5;  njobs = 2: c3_130 and ct3seg in one tile table, per cfg
  b. ffc_convp_forward, every case under cfg 0..3 (pick_patch_cfg forced to plan_patch_job(B, M, segs, cfg),
     rt.USE_CONVQ = False) x {split, f32 (FFC_CONVP_EXACT_F32), presplit (A3 from ffc_split_bf16)}; a cfg
     outside the listed set must plan None (the job then falls to the generic kernel; asserted, no launch)
  c3_6x8 {2, 3}    cc [4] (3x3 as 4x4 taps), vec4, NS 2 TR 6 TC 8;  c3_5x7 {2, 3}: the same, float staging
  c3_b7 {2, 3}     c3_6x8 at B 7: NS 5 / 2, ragged last sample group
  ct3 {2, 3}       ConvT k3 s1 p1, C 9, 6x8, M 17: tap offsets fall with k (sorted by the planner)
  c4s2pw {2, 3}    Conv2d k4 s2 p1 C 6 8x8 + 1x1 C 5 at 4x4: cc [4, 16]
  pw {2, 3}        1x1 only, C 17 + 3 at 7x3, B 3, M 130: float staging, five M-tiles
  wide {2, 3}      Conv2d k3, C 3, 3x260, B 1: nrb 3, ncb 2 (cfg 2) / 3 (cfg 3), TR 1
  ctdil {3}        ConvT k4 s1 p0 dilation 2: 16 dilated taps, only the smallest pixel block fits
  ct3seg {0, 1}    the 4-phase three-segment job;  ct_iw6 {1}: one segment, IW 6 (float staging; cfg 0 does not
                   fit the staging registers);  ctop {0, 1}: phases of 1 / 2 / 2 / 4 taps
  ct_b5 {0, 1}     ConvT k4 s2 p1 C 9 4x8 at B 5: NS 4 / 2, ragged last sample group
  ct_wide {0, 1}   ConvT k4 s2 p1 C 5 2x132, B 1: nrb 2, ncb 2 (cfg 0) / 3 (cfg 1)
                   (nrb > 1 or ncb > 1 forces NS = 1 in plan_patch_job, so no single shape has both split
                   planes and a ragged sample group: the two are separate cases per cfg)
  epilogue         ct3seg (cfg 0, 1) / c4s2pw (cfg 2, 3): bias + addend + slab (npb * 4 rows), act 0 / 1 / 2 / 5;
                   njobs = 2: c3_6x8 + c4s2pw in one launch (cfg 2)
  c. ffc_pw_forward cfg 0 / 1 / 2 on (B 3, M 40, C 17, 7x3), (B 5, M 200, C 64 + 48, 8x5),
     (B 1, M 130, C 64 + 64 + 32, 16x9); tiles == ffc_pw_tiles; a slab pointer is refused
  d. ffc_convt_k4s2_smallm (B, IH, IW) -> small / comb at M <= 3 (M = 4: comb 0) / VEC
  (2, 8, 8) (2, 3, 40)     0 / 2 / 1   16-row tiles; 3x40: two column tiles, ragged second
  (2, 5, 3) (2, 4, 33)     0 / 2 / 0   scalar staging; 4x33: two column tiles
  (1, 9, 4) (2, 12, 20) (1, 9, 36)   1 / 1 / 1   8-row tiles over 8 channel quarters
  (1, 17, 33) (1, 10, 3)   1 / 1 / 0
  (256, 9, 4) (256, 9, 3)  0 / 2 / 1, 0   the large grid with IH > 8 (C 3)
  (130, 9, 4) (130, 9, 3)  1 / 0 / 1, 0   8-row tiles, more than 256 workgroups: the serial combine at M <= 3
     each at M 1..4 with C0 / C1 from 1/0, 7/0, 9/8, 5/12, 17/0, 128/128 (the large-batch shapes: 3/0)
  e. ffc_conv3x3_smallm(_tf): H 1 / 31 / 32 / 33, W 4 / 64 / 68 / 132, M 1..4, C 1/0, 3/0, 5/4, 128/128;
     _tf on segment 0, 1, both, with and without noise (test_gpu_defer.py keeps its four ragged cases)
  f. ffc_split_bf16 n 1 / 7 / 8 / 257 (planes bit-exact, sum exact, nothing written past n);
     ffc_conv_pack on a generic, a cc = 4 patch and a convq plan; ffc_convq_pack_a3 with the fragment
     order inverted (conv_refs.unpack_a3)
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_refs as cr
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 1e-5
NAN = float("nan")
SLOPE = cr.SLOPE
TANH = cr.ACT["TANH"]
REACHED = set()     # branches the cases ran: ("gemm", cfg), ("patch", cfg), ("pw", cfg), ("smallm", small, comb, vec)


def _mods():
    import fastfourierconvolution_amd  # noqa: F401
    from fastfourierconvolution_amd import _lib, _plan, _runtime as rt
    return _lib, _plan, rt


def _L():
    return _mods()[2].lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(status, what):
    _mods()[0].check(status, what)


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


_LIVE = []


def _dev(t):
    """a device copy that stays alive until the test ends (the ABI takes raw pointers)"""
    if t is None:
        return None
    _LIVE.append(t.to(DEV).contiguous())
    return _LIVE[-1]


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def _err(family, what, out, ref):
    """print, then return, the normwise error of a returned tensor (which must hold no NaN)"""
    assert not torch.isnan(out).any(), f"{what}: unwritten (NaN) elements"
    e = normwise_err(out.detach().cpu().double().reshape(ref.shape), ref)
    print(f"OBS {family} {what} {e:.3e}")
    return e


def _check_slab(family, what, slab, pre):
    assert not torch.isnan(slab).any(), f"{what}: unwritten slab rows"
    n, mean, var = cr.merge_slab(slab.cpu())
    n0, mean0, var0 = cr.channel_stats(pre)
    assert torch.equal(n, torch.full_like(n, float(n0))), (what, n, n0)
    print(f"OBS {family}_stats {what} mean {(mean - mean0).abs().max():.3e} var {((var - var0).abs() / var0).max():.3e}")
    torch.testing.assert_close(mean, mean0, rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} mean: {m}")
    torch.testing.assert_close(var, var0, rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} var: {m}")


@contextlib.contextmanager
def _knobs(**kw):
    rt = _mods()[2]
    old = {k: getattr(rt, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(rt, k, v)
        yield rt
    finally:
        for k, v in old.items():
            setattr(rt, k, v)


@contextlib.contextmanager
def _force_patch_cfg(cfg):
    _plan = _mods()[1]
    old = _plan.pick_patch_cfg
    _plan.pick_patch_cfg = lambda B, M, segs, min_blocks=512: _plan.plan_patch_job(B, M, segs, cfg)
    try:
        yield
    finally:
        _plan.pick_patch_cfg = old


def _S(*a, **k):
    return _mods()[1].Seg(*a, **k)


def _jobs():
    """name -> (B, M, segs): every job shape of families a to c"""
    c3 = lambda h, w: [_S("conv", 7, h, w, 3, 1, 1)]   # noqa: E731
    ct = lambda C, h, w: _S("convT", C, h, w, 4, 2, 1)   # noqa: E731
    return {
        "c3_36": (2, 36, c3(5, 7)), "c3_130": (2, 130, c3(5, 7)), "ragged": (2, 130, c3(11, 13)),
        "c3_5x7": (2, 36, c3(5, 7)), "c3_6x8": (2, 36, c3(6, 8)), "c3_b7": (7, 36, c3(6, 8)),
        "c4s2": (2, 40, [_S("conv", 5, 9, 7, 4, 2, 1)]),
        "ct3seg": (3, 40, [ct(20, 4, 4), ct(12, 4, 4), _S("pw", 8, 8, 8)]),
        "ct1x1": (3, 70, [_S("convT", 10, 1, 1, 4, 1, 0)]),
        "ctop": (2, 36, [_S("convT", 3, 5, 7, 3, 2, 1, 1, 1)]),
        "ctdil": (2, 36, [_S("convT", 2, 5, 5, 4, 1, 0, 2)]),
        "cdil": (2, 36, [_S("conv", 4, 7, 9, 3, 1, 2, 2)]),
        "pool": (2, 36, [_S("pw", 6, 4, 4, pool=True)]),
        "gate": (3, 40, [_S("pw", 12, 5, 3, gate=True)]),
        "poolgate": (2, 40, [_S("pw", 6, 4, 4, pool=True, gate=True), _S("pw", 5, 4, 4)]),
        "allpad": (2, 36, [_S("convT", 3, 3, 4, 1, 2, 0)]),
        "ct3": (2, 17, [_S("convT", 9, 6, 8, 3, 1, 1)]),
        "c4s2pw": (2, 40, [_S("conv", 6, 8, 8, 4, 2, 1), _S("pw", 5, 4, 4)]),
        "pw": (3, 130, [_S("pw", 17, 7, 3), _S("pw", 3, 7, 3)]),
        "wide": (1, 36, [_S("conv", 3, 3, 260, 3, 1, 1)]),
        "ct_iw6": (3, 40, [ct(9, 5, 6)]), "ct_b5": (5, 40, [ct(9, 4, 8)]), "ct_wide": (1, 40, [ct(5, 2, 132)]),
        "pw40": (3, 40, [_S("pw", 17, 7, 3)]),
        "pw200": (5, 200, [_S("pw", 64, 8, 5), _S("pw", 48, 8, 5)]),
        "pw130": (1, 130, [_S("pw", 64, 16, 9), _S("pw", 64, 16, 9), _S("pw", 32, 16, 9)]),
    }


@functools.lru_cache(maxsize=None)
def _case(name, bias=False, addend=False):
    """(B, M, segs, inputs, float64 pre-activation reference), computed once per (case, extras)"""
    B, M, segs = _jobs()[name]
    OH, OW = _mods()[1].seg_out(segs[0])
    d = cr.job_inputs(B, M, segs, OH, OW, seed=sum(map(ord, name)), bias=bias, addend=addend)
    pre, _ = cr.conv_job_ref(segs, d["xs"], d["ws"], d["layouts"], d["gates"], d["bias"], d["addend"])
    return B, M, segs, d, pre


def _exec(name, bias=False, addend=False, pw_ok=False):
    """a ConvExec of the case under the knobs in force (plans and packs); -> (ex, case)"""
    rt = _mods()[2]
    c = _case(name, bias, addend)
    B, M, segs, d, _ = c
    wts = [(_dev(w), lay, w.shape[2], w.shape[3], _dev(d["bias"]) if i == 0 else None)
           for i, (w, lay) in enumerate(zip(d["ws"], d["layouts"]))]
    return rt.ConvExec(B, M, segs, wts, DEV, pw_ok=pw_ok), c


def _job(ex, c, act=0, slab=None):
    """(job struct, NaN-prefilled output)"""
    B, M, segs, d, pre = c
    out = _nan(tuple(pre.shape))
    inputs = [(_dev(x), _dev(g)) for x, g in zip(d["xs"], d["gates"])]
    return ex.job(inputs, out, act, SLOPE, _dev(d["addend"]), slab), out


# --------------------------------------------------------------------------- a. ffc_conv_forward
GEMM_CASES = {  # name -> (phases, set of K per phase)
    "c3_36": (1, {63}), "c3_130": (1, {63}), "ragged": (1, {63}), "c4s2": (1, {80}), "ct3seg": (4, {136}),
    "ct1x1": (16, {10}), "ctop": (4, {3, 6, 12}), "ctdil": (1, {32}), "cdil": (1, {36}), "pool": (1, {6}),
    "gate": (1, {12}), "poolgate": (1, {11}), "allpad": (4, {3, 1}),
}


def _gemm_tiles(plans, cfg):
    """tile table + the Python restatement of its size: per job, phase and pixel block of BN pixels one
    tile per BM output channels"""
    _lib, _plan, rt = _mods()
    BM, BN, rows = _plan.TILE_CFGS[cfg]
    assert (BM, BN) == {0: (128, 128), 1: (64, 128), 2: (32, 256)}[cfg]
    assert _L().ffc_conv_stat_rows_per_tile(cfg) == rows == {0: 2, 1: 2, 2: 4}[cfg]
    tiles, nslots = _plan.build_tiles(plans, cfg)
    want = [sum(-(-(p.B * ph.PH * ph.PW) // BN) for ph in p.phases) for p in plans]
    assert nslots == want
    assert tiles.shape[0] == sum(n * -(-p.M // BM) for n, p in zip(want, plans))
    return tiles, nslots, rows


def _gemm_launch(names, cfg, act=0, bias=False, addend=False, stats=False):
    """the cases as the jobs of one ffc_conv_forward launch under tile cfg; -> [(case, out, slab)]"""
    _lib, _plan, rt = _mods()
    with _knobs(USE_PATCH=False):
        made = [_exec(n, bias, addend) for n in names]
    for (ex, c), n in zip(made, names):
        assert ex.kind == "gemm" and isinstance(ex.plan, _plan.JobPlan)
        nph, Ks = GEMM_CASES[n]
        assert len(ex.plan.phases) == nph and {ph.K for ph in ex.plan.phases} == Ks, [ph.K for ph in ex.plan.phases]
    tiles, nslots, rows = _gemm_tiles([ex.plan for ex, _ in made], cfg)
    td = _dev(torch.from_numpy(tiles))
    res, jobs = [], []
    for (ex, c), ns in zip(made, nslots):
        slab = _nan((ns * rows, c[1], 4)) if stats else None
        job, out = _job(ex, c, act, slab)
        jobs.append(job)
        res.append((c, out, slab))
    arr = (_lib.ConvJob * len(jobs))(*jobs)
    _ok(_L().ffc_conv_forward(arr, len(jobs), td.data_ptr(), tiles.shape[0], cfg, _stream()), "ffc_conv_forward")
    torch.cuda.synchronize()
    REACHED.add(("gemm", cfg))
    return res, [ex.plan for ex, _ in made]


@pytest.mark.parametrize("cfg", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(GEMM_CASES))
def test_conv_gemm_matches_fp64(name, cfg):
    _lib, _plan, rt = _mods()
    res, plans = _gemm_launch([name], cfg)
    (c, out, _), pl = res[0], plans[0]
    BM, BN, _ = _plan.TILE_CFGS[cfg]
    if name == "ragged":     # every tile dimension ragged, several tiles along M and N, under every cfg
        npix = pl.B * pl.phases[0].PH * pl.phases[0].PW
        assert pl.M % BM and npix % BN and pl.phases[0].K % 16 and pl.M > BM and npix > BN
    if name == "allpad":     # phases without a tap: one PAD_ENTRY each
        assert sum(ph.entries == [_plan.PAD_ENTRY] for ph in pl.phases) == 3
    if name == "ct1x1":
        assert (pl.Sy, pl.Sx) == (4, 4) and all(ph.PH == ph.PW == 1 for ph in pl.phases)
    if name in ("pool", "gate", "poolgate"):   # the patch planners refuse them: only this kernel runs them
        assert _plan.plan_patch_job(pl.B, pl.M, pl.segs) is None and _plan.plan_convq_job(pl.B, pl.M, pl.segs, 0) is None
    assert _err("gemm", f"{name} cfg{cfg}", out, c[4]) <= TOL


@pytest.mark.parametrize("act", [0, 1, 2, 5])
@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_conv_gemm_epilogue(cfg, act):
    res, _ = _gemm_launch(["ct3seg"], cfg, act, bias=True, addend=True, stats=True)
    c, out, slab = res[0]
    assert _err("gemm", f"ct3seg cfg{cfg} epilogue act{act}", out, cr.act64(c[4], act, SLOPE)) <= TOL
    _check_slab("gemm", f"ct3seg cfg{cfg} act{act}", slab, c[4])


@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_conv_gemm_two_jobs_in_one_launch(cfg):
    res, plans = _gemm_launch(["c3_130", "ct3seg"], cfg, 2, stats=True)
    assert plans[0].M != plans[1].M and len(plans[0].phases) != len(plans[1].phases)
    for (c, out, slab), n in zip(res, ("c3_130", "ct3seg")):
        assert _err("gemm", f"njobs2 {n} cfg{cfg}", out, cr.act64(c[4], 2, SLOPE)) <= TOL
        _check_slab("gemm", f"njobs2 {n} cfg{cfg}", slab, c[4])


# --------------------------------------------------------------------------- b. ffc_convp_forward
PATCH_CASES = {  # name -> {cfg: (cc, vec4, NS, TR, TC, nrb, ncb)}; a cfg not listed must plan None
    "c3_6x8": {2: ([4], [True], 2, 6, 8, 1, 1), 3: ([4], [True], 2, 6, 8, 1, 1)},
    "c3_5x7": {2: ([4], [False], 2, 5, 7, 1, 1), 3: ([4], [False], 2, 5, 7, 1, 1)},
    "c3_b7": {2: ([4], [True], 5, 6, 8, 1, 1), 3: ([4], [True], 2, 6, 8, 1, 1)},
    "ct3": {2: ([4], [True], 2, 6, 8, 1, 1), 3: ([4], [True], 2, 6, 8, 1, 1)},
    "c4s2pw": {2: ([4, 16], [True, True], 2, 4, 4, 1, 1), 3: ([4, 16], [True, True], 2, 4, 4, 1, 1)},
    "pw": {2: ([16, 16], [False, False], 3, 7, 3, 1, 1), 3: ([16, 16], [False, False], 3, 7, 3, 1, 1)},
    "wide": {2: ([4], [True], 1, 1, 256, 3, 2), 3: ([4], [True], 1, 1, 128, 3, 3)},
    "ctdil": {3: ([4], [False], 1, 11, 11, 1, 1)},
    "ct3seg": {0: ([16] * 3, [True] * 3, 3, 4, 4, 1, 1), 1: ([16] * 3, [True] * 3, 3, 4, 4, 1, 1)},
    "ct_iw6": {1: ([16], [False], 2, 5, 6, 1, 1)},
    "ctop": {0: ([16], [False], 2, 5, 7, 1, 1), 1: ([16], [False], 1, 5, 7, 1, 1)},
    "ct_b5": {0: ([16], [True], 4, 4, 8, 1, 1), 1: ([16], [True], 2, 4, 8, 1, 1)},
    "ct_wide": {0: ([16], [True], 1, 1, 128, 2, 2), 1: ([16], [True], 1, 1, 64, 2, 3)},
}
ARITH = {"split": dict(CONV_ARITH="split", PRESPLIT_A=False), "f32": dict(CONV_ARITH="f32", PRESPLIT_A=False),
         "presplit": dict(CONV_ARITH="split", PRESPLIT_A=True)}


def _patch_block(B, M, segs, cfg):
    """plan_patch_job's pixel block restated: (NS, TR, TC, nrb, ncb) from the largest phase plane"""
    _plan = _mods()[1]
    base = _plan.plan_job(B, M, segs)
    NP = base.Sy * base.Sx
    npix = (4 // NP) * _plan.PATCH_CFGS[cfg][1] * 32
    PH, PW = max(p.PH for p in base.phases), max(p.PW for p in base.phases)
    TC = min(PW, npix)
    TR = min(PH, max(1, npix // TC))
    return max(1, min(B, npix // (TR * TC))), TR, TC, -(-PH // TR), -(-PW // TC)


def _patch_execs(names, cfg, arith, bias=False, addend=False):
    """ConvExecs on the LDS-patch kernel under cfg and the arithmetic variant, the plan asserted against
    PATCH_CASES; None when the cfg is expected to refuse the (single) case and does"""
    _lib, _plan, rt = _mods()
    made = []
    with _knobs(USE_PATCH=True, USE_CONVQ=False, **ARITH[arith]), _force_patch_cfg(cfg):
        for n in names:
            B, M, segs = _jobs()[n]
            want = PATCH_CASES[n].get(cfg)
            pl = _plan.plan_patch_job(B, M, segs, cfg)
            if want is None:
                assert pl is None, f"{n}: cfg {cfg} was expected to refuse this shape"
                ex, _ = _exec(n, bias, addend)
                assert ex.kind == "gemm"          # a refused job falls to the generic kernel
                return None
            ex, c = _exec(n, bias, addend)
            assert ex.kind == "patch" and ex.launch_key == ("patch", cfg) and not ex.plan.q
            p = ex.plan
            assert (p.cfg, p.cc, p.vec4, p.NS, p.TR, p.TC, p.nrb, p.ncb) == (cfg,) + want
            assert (p.NS, p.TR, p.TC, p.nrb, p.ncb) == _patch_block(B, M, segs, cfg)
            assert len(p.phases) == _plan.PATCH_CFGS[cfg][0]
            assert ex.use_a3 == (arith == "presplit") and (ex.A3 is not None) == ex.use_a3
            made.append((ex, c))
    return made


def _patch_launch(made, cfg, arith, act=0, stats=False):
    _lib, _plan, rt = _mods()
    tiles = _plan.build_patch_tiles([ex.plan for ex, _ in made])
    assert tiles.shape[0] == sum(ex.plan.npb * -(-ex.plan.M // 32) for ex, _ in made)
    td = _dev(torch.from_numpy(tiles))
    res, jobs = [], []
    for ex, c in made:
        slab = _nan((ex.plan.npb * 4, c[1], 4)) if stats else None
        job, out = _job(ex, c, act, slab)
        assert bool(job.A3) == (arith == "presplit")
        jobs.append(job)
        res.append((c, out, slab))
    arr = (_lib.ConvPJob * len(jobs))(*jobs)
    flag = _lib.CONVP_EXACT_F32 if arith == "f32" else 0
    _ok(_L().ffc_convp_forward(arr, len(jobs), td.data_ptr(), tiles.shape[0], cfg | flag, _stream()),
        "ffc_convp_forward")
    torch.cuda.synchronize()
    REACHED.add(("patch", cfg))
    return res


@pytest.mark.parametrize("arith", sorted(ARITH))
@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("name", sorted(PATCH_CASES))
def test_conv_patch_matches_fp64(name, cfg, arith):
    _lib, _plan, rt = _mods()
    made = _patch_execs([name], cfg, arith)
    if made is None:
        return
    p = made[0][0].plan
    if name == "ct3":        # a ConvTranspose2d's tap offsets fall with k: the planner sorts them
        offs = [o for _, o in _plan._taps(p.segs[0], 1, 0, 6, 6)]
        assert offs == sorted(offs, reverse=True) and len(offs) == 3
    if name == "pw":
        assert -(-p.M // 32) == 5
    if name in ("c3_b7", "ct_b5"):
        assert p.NS > 1 and p.B % p.NS
    if name in ("wide", "ct_wide"):
        assert p.nrb > 1 and p.ncb > 1
    if name == "ctop":
        assert [ph["T"] for ph in p.phases] == [[1], [2], [2], [4]]
    (c, out, _), = _patch_launch(made, cfg, arith)
    assert _err(f"patch_{arith}", f"{name} cfg{cfg}", out, c[4]) <= TOL


@pytest.mark.parametrize("arith", sorted(ARITH))
@pytest.mark.parametrize("act", [0, 1, 2, 5])
@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
def test_conv_patch_epilogue(cfg, act, arith):
    name = "ct3seg" if cfg < 2 else "c4s2pw"
    made = _patch_execs([name], cfg, arith, bias=True, addend=True)
    (c, out, slab), = _patch_launch(made, cfg, arith, act, stats=True)
    assert _err(f"patch_{arith}", f"{name} cfg{cfg} epilogue act{act}", out, cr.act64(c[4], act, SLOPE)) <= TOL
    _check_slab(f"patch_{arith}", f"{name} cfg{cfg} act{act}", slab, c[4])


@pytest.mark.parametrize("arith", sorted(ARITH))
def test_conv_patch_two_jobs_in_one_launch(arith):
    made = _patch_execs(["c3_6x8", "c4s2pw"], 2, arith)
    assert made[0][0].plan.M != made[1][0].plan.M and made[0][0].plan.cc != made[1][0].plan.cc
    for (c, out, slab), n in zip(_patch_launch(made, 2, arith, 2, stats=True), ("c3_6x8", "c4s2pw")):
        assert _err(f"patch_{arith}", f"njobs2 {n}", out, cr.act64(c[4], 2, SLOPE)) <= TOL
        _check_slab(f"patch_{arith}", f"njobs2 {n}", slab, c[4])


# --------------------------------------------------------------------------- c. ffc_pw_forward
PW_TILE = {0: (128, 128), 1: (64, 128), 2: (64, 64)}
PW_CASES = [("pw40", False, True, 0), ("pw200", True, True, 2), ("pw130", True, False, 1)]   # name, bias, addend, act


@pytest.mark.parametrize("cfg", [0, 1, 2])
@pytest.mark.parametrize("name,bias,addend,act", PW_CASES, ids=[c[0] for c in PW_CASES])
def test_pw_gemm_forced_cfg_matches_fp64(name, bias, addend, act, cfg):
    with _knobs(PW_KERNEL="pw"):
        ex, c = _exec(name, bias, addend, pw_ok=True)
    B, M, segs, d, pre = c
    assert ex.kind == "pw" and ex.launch_key[0] == "pw"
    Q = ex.plan.OH * ex.plan.OW
    BM, BN = PW_TILE[cfg]
    assert _L().ffc_pw_tiles(M, B, Q, cfg) == -(-M // BM) * -(-(B * Q) // BN)
    job, out = _job(ex, c, act)
    _ok(_L().ffc_pw_forward(ctypes.byref(job), cfg, _stream()), "ffc_pw_forward")
    torch.cuda.synchronize()
    REACHED.add(("pw", cfg))
    assert _err("pw", f"{name} cfg{cfg}", out, cr.act64(pre, act, SLOPE)) <= TOL


@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_pw_gemm_refuses_a_slab(cfg):
    with _knobs(PW_KERNEL="pw"):
        ex, c = _exec("pw40", pw_ok=True)
    slab = _nan((4, c[1], 4))
    job, out = _job(ex, c, 0, slab)
    assert _L().ffc_pw_forward(ctypes.byref(job), cfg, _stream()) != 0
    assert b"BN partials" in _L().ffc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(slab).all()


# --------------------------------------------------------------------------- d. ffc_convt_k4s2_smallm
def _ct_rule(B, IH, IW, M):
    """the host rule of ffc_convt_k4s2_smallm restated: (small, comb, vec)"""
    cdiv = lambda a, b: -(-a // b)   # noqa: E731
    small = B * cdiv(IH, 16) * cdiv(IW, 32) < 256 and IH > 8
    tr, nq = (8, 8) if small else (16, 4)
    grid = B * cdiv(IH, tr) * cdiv(IW, 32)
    qt = 16 * (tr // 2)
    comb = 0
    if M <= 3:
        if nq == 8 and qt == 64 and grid <= 256 and nq * 16 * M * qt * 4 <= 160 * 1024:
            comb = 1
        elif nq != 8 and (nq - 1) * 16 * M * qt * 4 <= 80 * 1024:
            comb = 2
    return int(small), comb, int(IW % 4 == 0)


CT_CHANNELS = [(1, 0), (7, 0), (9, 8), (5, 12), (17, 0), (128, 128)]
CT_SHAPES = [  # (B, IH, IW) -> (small, comb at M <= 3, vec); large batches run at C 3
    ((2, 8, 8), (0, 2, 1)), ((2, 3, 40), (0, 2, 1)), ((2, 5, 3), (0, 2, 0)), ((2, 4, 33), (0, 2, 0)),
    ((1, 9, 4), (1, 1, 1)), ((2, 12, 20), (1, 1, 1)), ((1, 9, 36), (1, 1, 1)), ((1, 17, 33), (1, 1, 0)),
    ((1, 10, 3), (1, 1, 0)), ((256, 9, 4), (0, 2, 1)), ((256, 9, 3), (0, 2, 0)), ((130, 9, 4), (1, 0, 1)),
    ((130, 9, 3), (1, 0, 0))]


def _ct_cases():
    out = []
    for si, ((B, IH, IW), want) in enumerate(CT_SHAPES):
        for M in (1, 2, 3, 4):
            C0, C1 = (3, 0) if B > 2 else CT_CHANNELS[(si + M) % 6]
            out.append((B, C0, C1, M, IH, IW, bool((si + M) % 2), (0, 2, TANH)[(si + M) % 3],
                        (want[0], want[1] if M <= 3 else 0, want[2])))
    return out


@functools.lru_cache(maxsize=None)
def _ct_inputs(B, C0, C1, M, IH, IW, bias):
    return cr.smallm_inputs(B, C0, C1, M, IH, IW, 4, True, seed=B + C0 + M + IH + IW, bias=bias)


def _ct_pack(d, C0, C1, M):
    n = _L().ffc_convt_smallm_pack_floats(C0, C1)
    assert n == (C0 + C1) * 64
    wp = _nan((n,))
    w0, w1 = _dev(d["w0"]), _dev(d["w1"])
    _ok(_L().ffc_convt_smallm_pack(_ptr(w0), C0, _ptr(w1), C1, M, _ptr(wp), _stream()), "ffc_convt_smallm_pack")
    return wp


@pytest.mark.parametrize("B,C0,C1,M,IH,IW,bias,act,want", _ct_cases(),
                         ids=[f"B{c[0]}_{c[4]}x{c[5]}_C{c[1]}+{c[2]}_M{c[3]}" for c in _ct_cases()])
def test_convt_k4s2_smallm_matches_fp64(B, C0, C1, M, IH, IW, bias, act, want):
    assert _ct_rule(B, IH, IW, M) == want
    d = _ct_inputs(B, C0, C1, M, IH, IW, bias)
    wp = _ct_pack(d, C0, C1, M)
    out = _nan((B, M, 2 * IH, 2 * IW))
    x0, x1, bv = _dev(d["x0"]), _dev(d["x1"]), _dev(d["bias"])
    _ok(_L().ffc_convt_k4s2_smallm(_ptr(x0), C0, _ptr(x1), C1, _ptr(wp), _ptr(bv), B, IH, IW, M, _ptr(out), act, SLOPE,
                                   _stream()), "ffc_convt_k4s2_smallm")
    torch.cuda.synchronize()
    REACHED.add(("smallm",) + want)
    # the pack on its own: [channel][tap][m 0..3], zero for m >= M
    w = torch.cat([d["w0"]] + ([d["w1"]] if C1 else []))                   # (C0 + C1, M, 4, 4)
    wantp = torch.zeros(C0 + C1, 16, 4)
    wantp[:, :, :M] = w.reshape(C0 + C1, M, 16).transpose(1, 2)
    assert torch.equal(wp.cpu().reshape(C0 + C1, 16, 4), wantp)
    ref = cr.convt_k4s2_ref(d["x0"], d["w0"], d["x1"], d["w1"], d["bias"], act, SLOPE)
    assert _err("convt_smallm", f"B{B} {IH}x{IW} C{C0}+{C1} M{M} {want}", out, ref) <= TOL


def test_convt_k4s2_smallm_rejections_leave_the_output_alone():
    L = _L()
    d = _ct_inputs(1, 128, 128, 4, 3, 4, False)
    wp = _ct_pack(d, 128, 128, 4)
    x = _dev(torch.cat([d["x0"], d["x1"], d["x0"]], dim=1))          # enough channels for any count below
    out = _nan((1 * 5 * 6 * 8 + 4,))
    run = lambda C0, C1, M, o: L.ffc_convt_k4s2_smallm(_ptr(x), C0, _ptr(x), C1, _ptr(wp), None, 1, 3, 4, M, o, 0,  # noqa: E731
                                                         SLOPE, _stream())
    assert run(129, 128, 4, _ptr(out)) != 0 and b"256" in L.ffc_last_error()
    assert run(128, 128, 5, _ptr(out)) != 0 and b"M" in L.ffc_last_error()
    assert run(128, 128, 4, _ptr(out) + 4) != 0 and b"aligned" in L.ffc_last_error()
    w0 = _dev(d["w0"])
    assert L.ffc_convt_smallm_pack(_ptr(w0), 128, None, 0, 5, _ptr(wp), _stream()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# --------------------------------------------------------------------------- e. ffc_conv3x3_smallm(_tf)
C3_CASES = [  # (B, C0, C1, M, H, W, bias, act)
    (2, 1, 0, 1, 1, 4, False, 0), (1, 3, 0, 2, 31, 64, True, TANH), (2, 5, 4, 3, 32, 68, True, 0),
    (1, 128, 128, 4, 33, 132, False, TANH), (2, 3, 0, 4, 33, 4, True, TANH), (1, 5, 4, 1, 32, 132, False, 0),
    (1, 1, 0, 3, 31, 68, True, TANH), (2, 3, 0, 2, 1, 64, False, 0), (1, 5, 4, 4, 1, 132, True, TANH),
    (1, 128, 128, 2, 32, 4, True, 0)]
C3_TF = [(w, n) for w in ("seg0", "seg1", "both") for n in (False, True)]


def _c3_run(d, B, C0, C1, M, H, W, act, tf0=None, tf1=None, out=None):
    _lib = _mods()[0]
    out = _nan((B, M, H, W)) if out is None else out
    x0, x1, w0, w1, bv = (_dev(d[k]) for k in ("x0", "x1", "w0", "w1", "bias"))

    def struct(t):
        if t is None:
            return None
        s = _lib.InTf(_ptr(_dev(t["scale"])), _ptr(_dev(t["shift"])), t["act"], t["act_param"], _ptr(_dev(t["noise_w"])),
                      _ptr(_dev(t["noise"])))
        _LIVE.append(s)
        return ctypes.byref(s)
    head = (_ptr(x0), C0, _ptr(w0), _ptr(x1), C1, _ptr(w1), _ptr(bv), B, H, W, M, _ptr(out), act, SLOPE)
    if tf0 is None and tf1 is None:
        rc = _L().ffc_conv3x3_smallm(*head, _stream())
    else:
        rc = _L().ffc_conv3x3_smallm_tf(*head, struct(tf0), struct(tf1), _stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("B,C0,C1,M,H,W,bias,act", C3_CASES)
def test_conv3x3_smallm_matches_fp64(B, C0, C1, M, H, W, bias, act):
    d = cr.smallm_inputs(B, C0, C1, M, H, W, 3, False, seed=C0 + M + H + W, bias=bias)
    assert (-(-H // 32), -(-W // 64)) == ({1: 1, 31: 1, 32: 1, 33: 2}[H], {4: 1, 64: 1, 68: 2, 132: 3}[W])   # 32-row tiles
    rc, out = _c3_run(d, B, C0, C1, M, H, W, act)
    _ok(rc, "ffc_conv3x3_smallm")
    ref = cr.conv3x3_ref(d["x0"], d["w0"], d["x1"], d["w1"], d["bias"], act, SLOPE)
    assert _err("conv3x3_smallm", f"B{B} {H}x{W} C{C0}+{C1} M{M}", out, ref) <= TOL


@pytest.mark.parametrize("which,noise", C3_TF)
@pytest.mark.parametrize("B,C0,C1,M,H,W", [(2, 5, 4, 3, 33, 68), (1, 128, 128, 4, 31, 132)])
def test_conv3x3_smallm_tf_matches_fp64(B, C0, C1, M, H, W, which, noise):
    d = cr.smallm_inputs(B, C0, C1, M, H, W, 3, False, seed=C0 + H + len(which) + noise, bias=True)
    gen = torch.Generator().manual_seed(17 + noise)
    tf0 = cr.tf_inputs(B, C0, H, W, cr.ACT["GELU"], noise, gen) if which in ("seg0", "both") else None
    tf1 = cr.tf_inputs(B, C1, H, W, cr.ACT["LEAKY_RELU"], noise, gen) if which in ("seg1", "both") else None
    rc, out = _c3_run(d, B, C0, C1, M, H, W, TANH, tf0, tf1)
    _ok(rc, "ffc_conv3x3_smallm_tf")
    ref = cr.conv3x3_ref(d["x0"], d["w0"], d["x1"], d["w1"], d["bias"], TANH, SLOPE, tf0, tf1)
    assert _err("conv3x3_smallm_tf", f"{H}x{W} C{C0}+{C1} {which} noise{int(noise)}", out, ref) <= TOL


def test_conv3x3_smallm_rejections_leave_the_output_alone():
    d = cr.smallm_inputs(1, 129, 128, 4, 2, 8, 3, False, seed=1)
    out = _nan((1, 4, 2, 8))
    assert _c3_run(d, 1, 129, 128, 4, 2, 8, 0, out=out)[0] != 0 and b"256" in _L().ffc_last_error()
    assert _c3_run(d, 1, 128, 128, 5, 2, 8, 0, out=out)[0] != 0 and b"M" in _L().ffc_last_error()
    assert _c3_run(d, 1, 128, 128, 4, 2, 6, 0, out=out)[0] != 0 and b"W % 4" in _L().ffc_last_error()
    assert torch.isnan(out).all()


# --------------------------------------------------------------------------- f. packers
@pytest.mark.parametrize("n", [1, 7, 8, 257])
def test_split_bf16_is_three_exact_pieces(n):
    """split_bf16_kernel truncates (u & 0xFFFF0000) three times; each remainder is exact in fp32 and the
    third has at most 8 significant bits, so nothing is lost: planes bit-equal to conv_refs.split_bf16_ref
    and hi + mid + lo == x in float64.  Elements n..stride of a plane are not written."""
    x = cr.split_inputs(n, seed=n)
    stride = (n + 8) // 8 * 8 + 8
    assert stride > n and stride % 8 == 0
    planes = torch.full((3 * stride,), -1, device=DEV, dtype=torch.int16)
    xd = _dev(torch.from_numpy(x))
    _ok(_L().ffc_split_bf16(_ptr(xd), n, _ptr(planes), stride, _stream()), "ffc_split_bf16")
    torch.cuda.synchronize()
    got = planes.cpu().numpy().view(np.uint16).reshape(3, stride)
    assert (got[:, n:] == 0xFFFF).all()
    for g, w in zip(got, cr.split_bf16_ref(x)):
        assert np.array_equal(g[:n], w)
    total = sum(cr.bf16_to_f64(g[:n]) for g in got)
    assert np.array_equal(total, x.astype(np.float64))


def _pack_direct(ex, c):
    """ffc_conv_pack into a NaN-prefilled buffer of exactly a_size floats -> (A numpy, bias numpy)"""
    _lib = _mods()[0]
    B, M, segs, d, _ = c
    A, bias = _nan((ex.plan.a_size,)), _nan((M,))
    n, pad = len(segs), _lib.MAX_SEG - len(segs)
    ws = [_dev(w) for w in d["ws"]]
    bs = [_dev(d["bias"])] + [None] * (n - 1)
    wp = (ctypes.c_void_p * _lib.MAX_SEG)(*[_ptr(w) for w in ws], *([None] * pad))
    lay = (ctypes.c_int * _lib.MAX_SEG)(*d["layouts"], *([0] * pad))
    kh = (ctypes.c_int * _lib.MAX_SEG)(*[w.shape[2] for w in ws], *([1] * pad))
    kw = (ctypes.c_int * _lib.MAX_SEG)(*[w.shape[3] for w in ws], *([1] * pad))
    bp = (ctypes.c_void_p * _lib.MAX_SEG)(*[_ptr(b) for b in bs], *([None] * pad))
    job = ex.pack_job()
    _ok(_L().ffc_conv_pack(ctypes.byref(job), wp, lay, kh, kw, bp, _ptr(A), _ptr(bias), _stream()), "ffc_conv_pack")
    torch.cuda.synchronize()
    return A.cpu().numpy(), bias.cpu().numpy()


@pytest.mark.parametrize("kind", ["gemm", "patch_cc4", "convq"])
def test_conv_pack_matches_the_ktab(kind):
    _lib, _plan, rt = _mods()
    if kind == "gemm":
        with _knobs(USE_PATCH=False):
            ex, c = _exec("ct3seg", bias=True)
        assert ex.kind == "gemm"
    elif kind == "patch_cc4":
        with _knobs(USE_CONVQ=False), _force_patch_cfg(2):
            ex, c = _exec("c4s2pw", bias=True)
        assert ex.kind == "patch" and ex.plan.cc == [4, 16] and not ex.plan.q
    else:
        with _knobs(USE_PATCH=True, USE_CONVQ=True, CONV_ARITH="split"):
            ex, c = _exec("ct3seg", bias=True)
        assert ex.kind == "patch" and ex.plan.q and ex.A3 is not None
    A, bias = _pack_direct(ex, c)
    want = cr.pack_ref(ex.plan, c[3]["ws"], c[3]["layouts"])
    assert not np.isnan(A).any() and np.array_equal(A, want)
    assert np.array_equal(bias, c[3]["bias"].numpy())
    for pi in range(len(ex.plan.phases)):      # rows M..Mpad and the padding columns are exactly 0
        kt_off, K, Kpad, a_off = cr.phase_table(ex.plan, pi)
        a = A[a_off: a_off + ex.plan.Mpad * Kpad].reshape(ex.plan.Mpad, Kpad)
        pad_cols = (ex.plan.ktab[kt_off: kt_off + Kpad, 0] & 15) == 15
        assert not a[ex.plan.M:].any() and not a[:, pad_cols].any() and a[:ex.plan.M][:, ~pad_cols].all()
    assert np.array_equal(ex.A.cpu().numpy()[:ex.plan.a_size], want)     # what the runtime packed itself
    if kind == "convq":   # ffc_convq_pack_a3: the fragment order inverted, each plane against the split
        planes = cr.unpack_a3(ex.plan, ex.A3.cpu().numpy()[:3 * ex.plan.a_size])
        for g, w in zip(planes, cr.split_bf16_ref(want)):
            assert np.array_equal(g, w)
        assert np.array_equal(sum(cr.bf16_to_f64(g) for g in planes), want.astype(np.float64))


# --------------------------------------------------------------------------- branch coverage
def test_every_branch_is_reached_by_a_case():
    """the case tables, run through the planners and the restated host rules here (no launch, no dependence
    on test order), reach every tile configuration and every small-M path; what the cases above recorded as
    run is a subset of it"""
    _lib, _plan, rt = _mods()
    planned = set()
    for name in GEMM_CASES:
        B, M, segs = _jobs()[name]
        pl = _plan.plan_job(B, M, segs)
        for cfg in _plan.TILE_CFGS:
            if _plan.build_tiles([pl], cfg)[0].shape[0] > 0:
                planned.add(("gemm", cfg))
    for name, cfgs in PATCH_CASES.items():
        B, M, segs = _jobs()[name]
        for cfg in _plan.PATCH_CFGS:
            pl = _plan.plan_patch_job(B, M, segs, cfg)
            assert (pl is not None) == (cfg in cfgs), (name, cfg)
            if pl is not None:
                planned.add(("patch", cfg))
    for name, *_ in PW_CASES:
        B, M, segs = _jobs()[name]
        for cfg in PW_TILE:
            if _L().ffc_pw_tiles(M, B, segs[0].IH * segs[0].IW, cfg) > 0:
                planned.add(("pw", cfg))
    for B, C0, C1, M, IH, IW, _, _, want in _ct_cases():
        assert _ct_rule(B, IH, IW, M) == want
        planned.add(("smallm",) + want)
    required = ({("gemm", c) for c in (0, 1, 2)} | {("patch", c) for c in (0, 1, 2, 3)} | {("pw", c) for c in (0, 1, 2)}
                | {("smallm", s, cb, v) for s, cb in ((0, 2), (0, 0), (1, 1), (1, 0)) for v in (0, 1)})
    assert required <= planned, required - planned
    assert REACHED <= planned, REACHED - planned
