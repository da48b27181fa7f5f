"""tests/fu_route_refs.py without a GPU:
A. the restatement of every non-refusal row equals, at one call, the two references the project already
   trusts: oracle.ffc_oracle.fourier_unit / spectral_transform (conv2 set to pass v through) and, for the rows
   that run the local Fourier unit, lfu_refs.spectral_transform_lfu -- outputs and BatchNorm buffers to float64
   round-off; and its state carries the package modules' state_dict keys and shapes;
B. the same restatement in float32 CPU torch stays within a quarter of every bound the GPU rows are held to
   (outputs, running statistics), three calls, one thread and the default thread count;
C. eight planted defects each exceed the bound on the tensor they are about, on at least one row, and on
   nothing they should not touch.
"""
import contextlib
import io

import pytest
import torch

import fu_route_refs as fr
import lfu_refs
from fu_route_cases import BY_ID, ROWS
from oracle import ffc_oracle as O

LIVE = [r for r in ROWS if r.raises is None]
IDS = [r.id for r in LIVE]
F64_TOL = 1e-12     # float64 round-off of FFTs and sums over <= 10^5 O(1) terms, normwise
CLEAN = 1e-6        # share of a bound below which a planted defect has not touched a tensor (float64 round-off)


def _reference(rid):
    row = BY_ID[rid]
    state, x = fr.from_row(row)
    return row, state, x, fr.run(row, state, x)


def test_rows_and_seeds():
    assert len(LIVE) == len(ROWS) - 2 and len(set(fr.SEEDS.values())) == len(ROWS)
    assert {r.mix for r in LIVE} == {"fp32", "fp16"}


@pytest.mark.parametrize("rid", IDS)
def test_state_is_the_package_modules(rid):
    """from_row's state loads into the drop-in module as it stands (strict keys, equal shapes)"""
    import fastfourierconvolution_amd as F
    row = BY_ID[rid]
    with contextlib.redirect_stdout(io.StringIO()):
        if row.kind == "fu":
            mod = F.FourierUnitSN(row.C, row.C)
        else:
            mod = F.SpectralTransform(16, 2 * row.C, 2 if (row.pool or row.up == 2) else 1, 1, True, row.up == 2)
    state, x = fr.from_row(row)
    want = mod.state_dict()
    assert list(state) == list(want)
    assert all(state[k].shape == want[k].shape and state[k].dtype == want[k].dtype for k in want)
    assert x.dtype == torch.float32 and tuple(x.shape) == fr.input_shape(row)
    for bn in fr.bn_names(row):      # visible affine and running statistics
        assert (state[bn + ".weight"] - 1).abs().max() > 1e-2 and state[bn + ".bias"].abs().max() > 1e-2
        assert state[bn + ".running_mean"].abs().max() > 1e-2 and (state[bn + ".running_var"] - 1).abs().max() > 1e-2


# --------------------------------------------------------------------------- A: against the oracle
@pytest.mark.parametrize("rid", IDS)
def test_restatement_equals_the_oracle(rid):
    row = BY_ID[rid]
    state, x = fr.from_row(row)
    (out,), bufs = fr.run(row, state, x, calls=1)
    sd = lfu_refs.to_double(state)
    xd = x.double()
    with torch.no_grad():
        if row.kind == "fu":
            s = xd.repeat_interleave(row.up, 2).repeat_interleave(row.up, 3)
            want = O.fourier_unit(s, sd, "", row.train)
        else:
            C = row.C
            sd["conv2.weight"] = torch.cat((torch.eye(C), torch.zeros(C, C))).double().reshape(2 * C, C, 1, 1)
            stride = 2 if (row.pool or row.up == 2) else 1
            if row.lfu:
                full = lfu_refs.spectral_transform_lfu(xd, sd, "", stride, row.up == 2, row.train)
            else:
                full = O.spectral_transform(xd, sd, "", stride, row.up == 2, row.train)
            want = full[:, :C]
            assert not full[:, C:].any()
    assert out.shape == want.shape == (row.B, row.C, row.H, row.H)
    assert fr.normwise(out, want) <= F64_TOL
    for key, got in bufs.items():
        bn = key.rsplit(".", 1)[0]
        ran = row.train and (row.lfu or not key.startswith("lfu."))
        if key.endswith("num_batches_tracked"):
            assert int(got) == int(sd[key]) == int(ran), key
        elif not ran:
            assert torch.equal(got, state[key].double()), key
        elif row.momentum_none and bn == "bn1":
            # the oracle's BatchNorm has the default momentum; the cumulative average's first step is the batch
            # statistic itself: undo the oracle's 0.9 / 0.1 mix
            stat = (sd[key] - 0.9 * state[key].double()) / 0.1
            assert fr.normwise(got, stat) <= 1e-10, key
        else:
            assert fr.normwise(got, sd[key]) <= F64_TOL, key


def test_cumulative_average_of_equal_batches_is_the_batch_statistic():
    """momentum=None over three calls on one input: the buffers end at the batch statistics whatever they held,
    and num_batches_tracked counts the calls (what the momentum_none rows' buffers are compared with)"""
    row, state, x, (outs, bufs) = _reference("st_8_c8_momentum_none")
    other = dict(state)
    other["bn1.running_mean"] = state["bn1.running_mean"] + 3.0
    _, bufs2 = fr.run(row, other, x)
    assert int(bufs["bn1.num_batches_tracked"]) == 3
    for k in ("bn1.running_mean", "bn1.running_var"):
        assert fr.normwise(bufs2[k], bufs[k]) <= F64_TOL
    assert fr.normwise(bufs2["fu.bn.running_mean"], bufs["fu.bn.running_mean"]) <= F64_TOL


def test_upsampled_bn1_counts_the_upsampled_samples():
    """running_var of bn1 behind the x2 upsample: the biased variance times n / (n - 1) with n = B H W at the
    upsampled size"""
    row, state, x, _ = _reference("st_16_up2_c16")
    _, bufs = fr.run(row, state, x, calls=1)
    mod = fr.build(row)
    mod.load_state_dict(state)
    with torch.no_grad():
        t = mod.conv1(mod.se_block(x.double()))
    var = t.var(dim=(0, 2, 3), unbiased=False)
    n = 4.0 * t.numel() / t.shape[1]
    want = 0.9 * state["bn1.running_var"].double() + 0.1 * var * n / (n - 1)
    assert fr.normwise(bufs["bn1.running_var"], want) <= F64_TOL


# --------------------------------------------------------------------------- B: the bound rule
def test_float32_cpu_torch_stays_within_a_quarter_of_every_bound():
    worst = {}
    default = torch.get_num_threads()
    try:
        for threads in sorted({1, default}):
            torch.set_num_threads(threads)
            for row in LIVE:
                state, x = fr.from_row(row)
                ref = fr.run(row, state, x)
                got = fr.run(row, state, x, dtype=torch.float32)
                for key, s in fr.shares(row, got, ref).items():
                    fam = ("out" if key.startswith("out") else "buffers") + (" fp16 rows" if row.mix == "fp16" else "")
                    if s >= worst.get(fam, (-1.0,))[0]:
                        worst[fam] = (s, row.id, key, threads)
    finally:
        torch.set_num_threads(default)
    for fam, (s, rid, key, threads) in sorted(worst.items()):
        print(f"OBS fp32-torch share {fam}: {s:.4f} ({rid} {key}, {threads} thread(s))")
    assert set(worst) == {"out", "buffers", "out fp16 rows", "buffers fp16 rows"}
    assert max(v[0] for v in worst.values()) <= fr.ROOM, worst


# --------------------------------------------------------------------------- C: planted defects
def _defect_shares(rid, defect):
    row, state, x, ref = _reference(rid)
    return fr.shares(row, fr.run(row, state, x, defect=defect), ref)


def _split(s, hit):
    """(the smallest share among the tensors named by `hit`, the largest among the others)"""
    named = [v for k, v in s.items() if hit(k)]
    rest = [v for k, v in s.items() if not hit(k)]
    assert named
    return min(named), max(rest, default=0.0)


UP2 = [r.id for r in LIVE if r.kind == "st" and r.up == 2]
ST_TRAIN = [r.id for r in LIVE if r.kind == "st" and r.train]
LFU = [r.id for r in LIVE if r.lfu]


def test_defect_row_sets():
    assert len(UP2) == 2 and len(LFU) == 2
    assert [r.id for r in LIVE if r.momentum_none] == ["st_8_c8_momentum_none", "st_16_c16_ch_momentum_none"]


@pytest.mark.parametrize("rid", UP2)
def test_defect_bn1_variance_over_the_input_count(rid):
    hit, rest = _split(_defect_shares(rid, "bn1_count"), lambda k: k == "bn1.running_var")
    assert hit > 1.0 and rest <= CLEAN, (hit, rest)     # bn1.running_var and nothing else


@pytest.mark.parametrize("rid", ["fu_8x8_c8", "fu_16_c16", "st_8_c8", "st_16_c8_lfu"])
def test_defect_unit_bn_updated_twice(rid):
    unit = "bn." if BY_ID[rid].kind == "fu" else "fu.bn."
    hit, rest = _split(_defect_shares(rid, "fu_bn_twice"), lambda k: k.startswith(unit))
    assert hit > 1.0 and rest <= CLEAN, (hit, rest)     # all three of its buffers


SKIP_ROWS = ("st_8_c8", "st_16_c8_lfu", "st_8_c8_lfu_fused", "st_16_up2_c16", "st_8_pool_c8_pw")


@pytest.mark.parametrize("rid,bn", [(rid, bn) for rid in SKIP_ROWS for bn in ("bn1", "fu.bn", "lfu.bn")
                                    if bn != "lfu.bn" or BY_ID[rid].lfu])
def test_defect_a_bn_never_updated(rid, bn):
    hit, rest = _split(_defect_shares(rid, "skip:" + bn), lambda k: k.startswith(bn + "."))
    assert hit > 1.0 and rest <= CLEAN, (hit, rest)


def test_defect_a_bn_never_updated_fu_rows():
    hit, rest = _split(_defect_shares("fu_16_c8_B2", "skip:fu.bn"), lambda k: k.startswith("bn."))
    assert hit > 1.0 and rest <= CLEAN, (hit, rest)


@pytest.mark.parametrize("rid", ["st_8_c8_momentum_none", "st_16_c16_ch_momentum_none"])
def test_defect_momentum_none_as_a_tenth(rid):
    s = _defect_shares(rid, "momentum_01")
    assert s["bn1.running_mean"] > 1.0 and s["bn1.running_var"] > 1.0, s
    assert max(v for k, v in s.items() if not k.startswith("bn1.running")) <= CLEAN


@pytest.mark.parametrize("rid", [r.id for r in LIVE if not r.train])
def test_defect_eval_on_batch_statistics(rid):
    s = _defect_shares(rid, "eval_batch_stats")
    assert min(s[f"out{i}"] for i in range(fr.CALLS)) > 1.0, s
    assert max(v for k, v in s.items() if not k.startswith("out")) == 0.0


@pytest.mark.parametrize("rid", [r.id for r in LIVE if r.kind == "st"])
def test_defect_residual_dropped(rid):
    s = _defect_shares(rid, "no_residual")
    assert min(s[f"out{i}"] for i in range(fr.CALLS)) > 1.0, s
    assert max(v for k, v in s.items() if not k.startswith("out")) <= CLEAN


@pytest.mark.parametrize("rid", LFU)
def test_defect_quadrants_in_the_wrong_order(rid):
    s = _defect_shares(rid, "lfu_order")
    assert min(s[f"out{i}"] for i in range(fr.CALLS)) > 1.0, s
    assert max(v for k, v in s.items() if k.startswith(("bn1.", "fu.bn."))) <= CLEAN


@pytest.mark.parametrize("rid", [r for r in ST_TRAIN if r not in LFU][:4])
def test_defect_idle_lfu_bn_bumped(rid):
    s = _defect_shares(rid, "lfu_bn_bump")
    assert s["lfu.bn.num_batches_tracked"] == float("inf")
    assert max(v for k, v in s.items() if k != "lfu.bn.num_batches_tracked") <= CLEAN
