"""The bounds and inputs of tests/test_gpu_aw_abi.py, proven without a GPU (tests/aw_refs.py).

1. aw_refs.restate, a restatement of csrc/aw_kernels.hip's arithmetic (the chunks, the strided per-thread sums and
   the fixed trees in fp64, the combine in fp32), stays under a quarter of every bound TOL * scale on the inputs
   the GPU file uses.  Two tolerances, each the smallest power of ten for which that holds: TOL_STAT = 1e-15 for
   the fp64 quantities (worst shares: per-chunk partials 0.19, rr 0.14, ff 0.13, rf 0.14, weights end to end
   0.04, rs / fs and the weights at their own stats exact; at 1e-16 the partials reach 1.9) and TOL_OUT = 1e-6
   for the fp32 combine (worst share 0.11; 1.1 at 1e-7).
2. Five planted defects exceed a bound or change the case on the input named beside each.
3. The tie inputs hit their ties exactly in float64 from the fp32 inputs.
Every test prints what it measured."""
import functools
import math

import numpy as np
import pytest

import aw_refs as A


@functools.lru_cache(maxsize=None)
def _inputs():
    """name -> (g_real, g_fake, real, fake, kw, the case, tie)"""
    out = {}
    for case, (kind, sign) in A.FIVE.items():
        for normalized in (True, False):
            a, b = A.make_list(A.NUMELS, sign, case)
            real, fake = A.logits_for(kind)
            out[f"case {case} normalized={normalized}"] = (a, b, real, fake, dict(A.KW, normalized=normalized), case, False)
    for name, (a, b, real, fake, kw, case, _) in A.tie_cases().items():
        out[name] = (a, b, real, fake, kw, case, True)
    a, b = A.make_list((A.EC + 1,) * 258, -1.0, 31)    # a partial 256 exists: the merge's second trip
    real, fake = A.logits_for("low")
    out["516 chunks"] = (a, b, real, fake, dict(A.KW), 1, False)
    return out


def _shares(name, defect=None):
    a, b, real, fake, kw, case, tie = _inputs()[name]
    r = A.restate(a, b, real, fake, defect=defect, **kw)
    try:
        sh, _ = A.abi_shares(a, b, real, fake, kw, r, tie=tie)
    except AssertionError as e:          # the case is not the reference's
        return {"case": float("inf")}, str(e)
    sh["case"] = 0.0 if int(r["stats"][7]) == case else float("inf")
    return sh, ""


def test_restatement_stays_under_a_quarter_of_every_bound():
    worst = {}
    for name in _inputs():
        sh, why = _shares(name)
        assert not why, (name, why)
        for k, v in sh.items():
            if v >= worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, name)
    print("OBS worst shares: " + "  ".join(f"{k} {v:.3f} ({n})" for k, (v, n) in sorted(worst.items())))
    assert all(v < 0.25 for v, _ in worst.values()), worst
    stat = max(v for k, (v, _) in worst.items() if k != "out")
    assert stat * 10 >= 0.25 and worst["out"][0] * 10 >= 0.25, "a TOL is not the smallest power of ten"
    assert A.TOL_OUT <= 1e-5


# defect -> (the input that catches it, the bound it exceeds)
PLANTED = {
    "drop_tail": ("case 1 normalized=True", "parts"),       # the scalar tail of a chunk dropped
    "drop_partial_256": ("516 chunks", "rr"),               # partial 256 dropped from the merge
    "rf_lt": ("rf == 0", "case"),                           # rf <= 0 read as rf < 0
    "rs_le": ("rs == alpha1", "case"),                      # rs <= alpha1 in place of <
    "wf_f32_early": ("case 1 normalized=True", "w_own"),    # w_f rounded to fp32 before the stats are written
}


@pytest.mark.parametrize("defect", list(PLANTED))
def test_planted_defect_exceeds_its_bound(defect):
    assert set(PLANTED) == set(A.AW_DEFECTS)
    name, key = PLANTED[defect]
    clean, _ = _shares(name)
    bad, why = _shares(name, defect)
    print(f"OBS {defect}: {key} on {name!r} {clean[key]:.3g} -> {bad[key]:.3g} {why}")
    assert clean[key] < 0.25 and bad[key] > 1.0, (defect, clean, bad)


def test_ties_are_exact_in_float64():
    t = A.tie_cases()
    a, b, real, fake, kw, case, _ = t["rs == alpha1"]
    rs = A.sigmoid_mean(real)
    assert rs == 0.5 == kw["alpha1"] and A.weights(1.0, 1.0, 1.0, rs, A.sigmoid_mean(fake), **kw)[2] == case == 5
    a, b, real, fake, kw, case, _ = t["rs == fs - delta"]
    rs, fs = A.sigmoid_mean(real), A.sigmoid_mean(fake)
    assert rs == 0.5 and fs == 0.75 and fs - kw["delta"] == rs and rs > kw["alpha1"] and rs > kw["alpha2"]
    assert 1.0 / (1.0 + math.exp(-100.0)) == 1.0
    assert A.weights(1.0, 1.0, 1.0, rs, fs, **kw)[2] == case == 5       # neither < nor > holds at the tie
    assert float(np.mean(1.0 / (1.0 + np.exp(-real.astype(np.float64))))) == 0.5
    assert float(np.mean(1.0 / (1.0 + np.exp(-fake.astype(np.float64))))) == 0.75
    a, b, real, fake, kw, case, _ = t["rf == 0"]
    parts = A.partials(a, b)
    assert (parts[:, 2] == 0.0).all() and (parts[:, 0].sum() > 0) and (parts[:, 1].sum() > 0)
    assert all(float(np.abs(x.astype(np.float64) * y.astype(np.float64)).sum()) == 0.0 for x, y in zip(a, b))
    assert A.restate(a, b, real, fake, **kw)["stats"][7] == case == 1
    print("OBS ties: rs = 0.5 = alpha1; rs = 0.5 = fs - delta = 0.75 - 0.25; rf = 0.0 on disjoint supports")


def test_restatement_matches_the_fixture_cases():
    """restate() against aw_reference on the recorded fixture: the same case and weights within the bounds"""
    for c in A.load_cases():
        r = A.restate(c["a"], c["b"], c["real"], c["fake"], **c["kw"])
        sh, e_case = A.abi_shares(c["a"], c["b"], c["real"], c["fake"], c["kw"], r)
        assert e_case == c["case"] == int(r["stats"][7])
        assert all(v < 0.25 for v in sh.values()), sh
