"""What every Fourier-unit route computes, row by row of tests/fu_route_cases.py, against the float64 restatement
of tests/fu_route_refs.py: the outputs of three calls, the running statistics and num_batches_tracked of bn1,
the unit's BatchNorm and the local Fourier unit's after the third, and the route the call asked for (so a value
never passes on another path).  tests/test_gpu_fu_route.py pins which entry points a row launches; this module
pins what they are handed: the BatchNorm behind each descriptor, count_mult, the slab and its rows, who updates
which buffer and how often.

Per row (rt switches set as the route test sets them, state and input of fu_route_refs.from_row):
  route     rt.fu_route's answer in each of the three calls is the row's; st rows: conv1's kernel and the rows of
            bn1's slab too
  outputs   each call normwise <= 1e-5 (fp16 mix: 2e-3, the one-unit gate of test_gpu_sn_fp16.py), no NaN; the
            three bit-identical (train: batch statistics make the output independent of the buffers; eval: the
            buffers do not move)
  buffers   train: running_mean / running_var at rtol 1e-5, atol 1e-6 (the unit's BN under the fp16 mix: 2e-3
            and 2e-3 max|ref|), num_batches_tracked = 3; eval: every buffer bit-equal to what was loaded; lfu.bn
            bit-equal to what was loaded wherever the local Fourier unit does not run

Direct FourierUnitSN._run(t, in_relu=True, residual=True, in_fold=desc) -- the branch of fourier_unity.py that
takes a ready descriptor, which no caller in the package reaches (spectral() launches its route itself); desc is
a whole-slab fold of bn1 over t's own statistics in 2 to 4 rows:

  case                        | route                         | what _run does with desc
  (2, 8, 8, 8)                | fused, in_fold 'slab'         | folded as made, inside pass 0
  (2, 4, 4, 4)                | fused, no fold scratch        | desc.materialize(): reduce + finalize launch
  (2, 16, 16, 16), BN_CHFOLD  | staged, in_fold 'channels'    | re-made as a 'channels' descriptor, folded in the r2c
  (2, 16, 16, 16)             | staged, in_fold None          | desc.materialize() in front of the staged path

Rows by family and the switches they run under:
  fused    fu_* rows on csrc/fu_kernels.hip: fold scratch or not, split / whole-slab / no mix fold, FU_SPILL off,
           FU_SPLIT off, BN_FOLD off, eval, 24^2 and 48^2 (up 2) planes, B = 64
  staged   fu_* rows on csrc/fu2d_kernels.hip: spilled (r2c_mix or not), FU2D_SPILL off, FU2D_R2CMIX off, FU_COLS
           off, 32^2 / 64^2, eval with and without the column kernel, BN_CHFOLD with its two limits
  st       bn1 in front: slab fold, own launch (no scratch, BN_FOLD off, 65 rows), BN_FOLD_MAX raised, channel
           fold, momentum=None, eval behind a train-shaped route, up 2 (count_mult 4), pool, ST_PATH 'pw'
  lfu      run_lfu on the staged and on the fused path
  fp16     the f16 MFMA mix, train and eval

Observed on the first MI355X run (largest over the rows of a family; outputs normwise, running statistics as a
share of their bound; all 61 cases in 2.4 s):
  family | outputs                               | running statistics
  fused  | 1.83e-07 (fu_8x8_c8_nospill)          | 0.026 (fu_32_c8_B2_fused bn.running_var)
  staged | 2.40e-07 (fu_16_c16_eval_nocols)      | 0.028 (fu_16_c16 bn.running_var)
  st     | 1.88e-07 (st_8_c8_eval)               | 0.029 (st_16_up2_c8_fused bn1.running_var)
  lfu    | 1.13e-07 (st_8_c8_lfu_fused)          | 0.023 (st_16_c8_lfu bn1.running_var)
  fp16   | 7.30e-05 (fu_32_c16_fp16_eval)        | 0.014 (fu_32_c16_fp16 bn.running_var, of the 2e-3 bound)
  direct | 1.14e-07 (remade_by_channel)          | 0.026 (no_scratch_materialize fu.bn.running_var)
The buffer shares are those of float32 CPU torch (test_fu_route_refs_cpu.py: 0.029): three float32 roundings
of the stored buffer.  Every call of a row was bit-identical to its first, the BN_CHFOLD rows included.
"""
import contextlib
import io

import pytest
import torch

import fu_route_refs as fr
import spectral_refs as sr
from fu_route_cases import BY_ID, Row

pytestmark = pytest.mark.gpu

DEV = "cuda"
LIVE = [r.id for r in BY_ID.values() if r.raises is None]


def family(row):
    if row.id.startswith("direct_"):
        return "direct"
    if row.mix == "fp16":
        return "fp16"
    if row.lfu:
        return "lfu"
    return "st" if row.kind == "st" else row.route["path"]


def _module(row, state):
    import fastfourierconvolution_amd as F
    with contextlib.redirect_stdout(io.StringIO()):
        if row.kind == "fu":
            mod = F.FourierUnitSN(row.C, row.C)
        else:   # enable_lfu on in every st row (fu_route_refs): lfu.bn is there to be left alone
            mod = F.SpectralTransform(16, 2 * row.C, 2 if (row.pool or row.up == 2) else 1, 1, True, row.up == 2)
    mod.load_state_dict(state)
    mod = mod.to(DEV).train(row.train)
    if row.kind == "fu":
        mod.mix_precision = row.mix
    else:
        mod.run_lfu = row.lfu
        if row.momentum_none:
            mod.bn1.momentum = None
    return mod


def _spy(monkeypatch, rt, name, log):
    inner = getattr(rt, name)

    def spy(*a, **k):
        log.append((inner(*a, **k), a))
        return log[-1][0]
    monkeypatch.setattr(rt, name, spy)


def _compare(row, what, got, ref, loaded, touched):
    """the assertions on outputs and buffers; loaded: the state before the calls; touched(key): the BN of this
    buffer runs on batch statistics in this case"""
    s = fr.shares(row, got, ref)
    errs = [fr.normwise(a, r) for a, r in zip(got[0], ref[0])]
    bufs = {k: v for k, v in s.items() if k.endswith(("running_mean", "running_var")) and touched(k)}
    print(f"OBS {family(row)} {what}: out {max(errs):.3g} buffers {max(bufs.values(), default=0.0):.3g} "
          f"({max(bufs, key=bufs.get, default='-')})")
    bad = []    # every tensor out of bounds, not the first one: which ones a defect moves is what names it
    for i, a in enumerate(got[0]):
        assert a.shape == ref[0][i].shape
        if torch.isnan(a).any():
            bad.append((f"out{i}", "NaN"))
        elif s[f"out{i}"] > 1.0:
            bad.append((f"out{i}", f"normwise {errs[i]:.3g}"))
        if not torch.equal(a, got[0][0]):
            bad.append((f"out{i}", f"differs from call 0 by {fr.normwise(a, got[0][0]):.3g}"))
    for key, r in ref[1].items():
        a = got[1][key]
        if not touched(key):
            if not torch.equal(a, loaded[key]):
                bad.append((key, "changed"))
        elif key.endswith("num_batches_tracked"):
            if not int(a) == int(r) == fr.CALLS:
                bad.append((key, int(a)))
        elif not s[key] <= 1.0:
            rtol, atol = fr.buffer_tol(row, key, r)
            worst = (a.double() - r).abs().max().item()
            bad.append((key, f"{s[key]:.3g} of the bound (max |d| {worst:.3g}, rtol {rtol}, atol {atol:.3g})"))
    assert not bad, (what, bad)


@pytest.mark.parametrize("rid", LIVE)
def test_row_matches_the_restatement(rid, monkeypatch):
    from fastfourierconvolution_amd import _runtime as rt
    row = BY_ID[rid]
    for k, v in row.sw.items():
        monkeypatch.setattr(rt, k, v)
    state, x = fr.from_row(row)
    ref = fr.run(row, state, x)
    mod = _module(row, state)
    xd = x.to(DEV)
    routes, conv1s, firsts, outs = [], [], [], []
    _spy(monkeypatch, rt, "fu_route", routes)
    _spy(monkeypatch, rt, "st_conv1_route", conv1s)
    with torch.no_grad():
        for _ in range(fr.CALLS):
            firsts.append(len(routes))     # the main unit asks first (a local Fourier unit after it)
            outs.append(mod._run(xd, up=row.up) if row.kind == "fu" else mod.spectral(xd))
    torch.cuda.synchronize()
    assert len(routes) == fr.CALLS * (2 if row.lfu else 1)
    for i in firsts:
        route, args = routes[i]
        assert route._asdict() == row.route
        if row.kind == "st":
            assert args[-1].nrows == row.nrows and args[-1].count_mult == float(row.up * row.up)
    assert [c for c, _ in conv1s] == ([row.conv1] * fr.CALLS if row.kind == "st" else [])
    sd = mod.state_dict()
    got = ([o.cpu() for o in outs], {k: sd[k].cpu() for k in ref[1]})
    _compare(row, rid, got, ref, state, lambda k: row.train and (row.lfu or not k.startswith("lfu.")))


# (B, C, H), BN_CHFOLD, cuts of the slab, the route's (path, in_fold), desc.materialize() calls per _run
DIRECT = {
    "folded_as_made": ((2, 8, 8), False, (7, 64, 100), ("fused", "slab"), 0),
    "no_scratch_materialize": ((2, 4, 4), False, (5, 20), ("fused", None), 1),
    "remade_by_channel": ((2, 16, 16), True, (100,), ("staged", "channels"), 0),
    "staged_materialize": ((2, 16, 16), False, (100,), ("staged", None), 1),
}


@pytest.mark.parametrize("case", list(DIRECT))
def test_run_with_a_ready_descriptor(case, monkeypatch):
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import _runtime as rt
    (B, C, H), chfold, cuts, (path, in_fold), materialized = DIRECT[case]
    monkeypatch.setattr(rt, "BN_CHFOLD", chfold)
    row = Row("direct_" + case, "st", B, C, H)
    state, _ = fr.from_row(row, seed=4000 + 10 * H + int(chfold))
    t = torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(4500 + H))
    slab = sr.make_slab(t, cuts)
    nrows = slab.shape[0]
    assert 2 <= nrows <= 4 and int(sr.merge_slab(slab)[0][0]) == B * H * H
    ref = fr.run_from_t(C, state, t)

    bn1 = torch.nn.BatchNorm2d(C)
    bn1.load_state_dict({k[4:]: v for k, v in state.items() if k.startswith("bn1.")})
    with contextlib.redirect_stdout(io.StringIO()):
        fu = F.FourierUnitSN(C, C)
    fu.load_state_dict({k[3:]: v for k, v in state.items() if k.startswith("fu.")})
    bn1, fu = bn1.to(DEV).train(), fu.to(DEV).train()
    td, slabd = t.to(DEV), slab.to(DEV)

    routes, folds, mats, outs, keep = [], [], [], [], []
    _spy(monkeypatch, rt, "fu_route", routes)
    _spy(monkeypatch, rt, "make_bn_fold", folds)
    inner = rt.BnFoldDesc.materialize
    monkeypatch.setattr(rt.BnFoldDesc, "materialize", lambda self, stream: mats.append(self) or inner(self, stream))
    with torch.no_grad():
        for _ in range(fr.CALLS):
            desc = rt.make_bn_fold(bn1, C, slabd, nrows, 1.0, td.device, "slab")
            assert desc.kind == "slab"
            keep.append(desc)
            outs.append(fu._run(td, in_relu=True, residual=True, in_fold=desc))
    torch.cuda.synchronize()
    assert len(routes) == fr.CALLS
    for route, args in routes:
        assert (route.path, route.in_fold) == (path, in_fold)
        assert args[-1].ready == "slab" and args[-1].nrows == nrows
    assert len(mats) == materialized * fr.CALLS and all(any(m is d for d in keep) for m in mats)
    # bn1 again as a descriptor only where the route folds it by channel: over the same BN, slab and rows
    again = [(d, a) for d, a in folds if a[0] is bn1 and not any(d is k for k in keep)]
    assert len(again) == (fr.CALLS if in_fold == "channels" else 0)
    for d, a in again:
        assert d.kind == "channels" and a[2] is slabd and (a[1], a[3], a[4]) == (C, nrows, 1.0)
    got = ([o.cpu() for o in outs],
           {**{"bn1." + k: v.cpu() for k, v in bn1.state_dict().items() if k in fr.BN_BUFFERS},
            **{"fu." + k: v.cpu() for k, v in fu.state_dict().items() if k.split(".")[-1] in fr.BN_BUFFERS}})
    _compare(row, "direct " + case, got, ref, state, lambda k: True)
