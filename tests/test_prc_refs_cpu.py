"""tests/prc_refs.py against the fixture recorded from the reference's own prc_features_to_metric
(tests/golden/metrics_prc.npz, gen_golden_prc.py), without a GPU: the direct-difference restatement reproduces the
fixture's counts exactly; on the fixture's inputs no row's decision margin is within 1000 x its bound, which is what
lets the GPU tests demand every flag; and the integer lattice holds rows that only `<=` decides."""
import functools
import os

import numpy as np
import pytest

import prc_refs as P
from conftest import ROOT

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "metrics_prc.npz"))
CASES = [("a", 3), ("a", 1), ("b", 3)]


@functools.lru_cache(maxsize=None)
def _ref(case, k):
    return P.prc(GOLD[f"{case}_f1"], GOLD[f"{case}_f2"], k)


def test_fixture_shapes_and_both_routes_of_the_reference_agree():
    assert GOLD["a_f1"].shape == (101, 130) and GOLD["a_f2"].shape == (90, 130)
    assert GOLD["b_f1"].shape == (65, 33) and GOLD["b_f2"].shape == (130, 33)
    assert all(GOLD[k].dtype == np.float32 for k in ("a_f1", "a_f2", "b_f1", "b_f2"))
    assert abs(float(GOLD["a_f1"].mean()) - 100.0) < 1.0   # the common offset
    for case, k in CASES:
        assert np.array_equal(GOLD[f"{case}_k{k}_0"], GOLD[f"{case}_k{k}_1"])


@pytest.mark.parametrize("case,k", CASES)
def test_restatement_reproduces_the_fixture_counts(case, k):
    n1, n2 = len(GOLD[f"{case}_f1"]), len(GOLD[f"{case}_f2"])
    ref = _ref(case, k)
    precision, recall, f_score = GOLD[f"{case}_k{k}_0"]
    assert ref["counts"] == [round(precision * n2), round(recall * n1)]
    # the reference's means are fp32
    assert abs(precision - ref["counts"][0] / n2) <= 2.0 ** -24 and abs(recall - ref["counts"][1] / n1) <= 2.0 ** -24
    assert abs(P.metric(ref, n1, n2)[2] - f_score) <= 1e-6
    if (case, k) == ("a", 3):
        assert ref["counts"] == [23, 14]
    if (case, k) == ("b", 3):
        assert ref["counts"] == [62, 6]


@pytest.mark.parametrize("case,k", CASES)
def test_no_fixture_row_is_decided_within_1000_bounds(case, k):
    ref = _ref(case, k)
    worst = min(float(np.min(np.abs(ref[f"margin_{s}"]) / ref[f"mbound_{s}"])) for s in (1, 2))
    rworst = min(float(np.min(P.lower(ref[f"radii2_{s}"]) / ref[f"rbound_{s}"])) for s in (1, 2))
    print(f"OBS prc fixture {case} k={k}: smallest |margin| / bound {worst:.3e}, smallest r2 / bound {rworst:.3e}, "
          f"smallest |margin| {min(np.abs(ref['margin_1']).min(), np.abs(ref['margin_2']).min()):.3e}, "
          f"largest bound {max(ref['mbound_1'].max(), ref['mbound_2'].max()):.3e}")
    assert worst > 1000.0


def test_lattice_has_rows_decided_by_equality_and_zero_radii():
    f1, f2 = P.lattice()
    assert np.array_equal(f1, np.round(f1)) and np.abs(f1).max() <= 4 and np.abs(f2).max() <= 4
    ref = P.prc(f1, f2, 3)
    r1 = P.lower(ref["radii2_1"])
    assert np.array_equal(r1, np.round(r1)), "lattice radii are integers"
    assert (r1 == 0).sum() >= 5 and (r1 > 0).any()
    tie_2 = (ref["margin_2"] == 0) & (ref["hit_2"] == 1)
    tie_1 = (ref["margin_1"] == 0) & (ref["hit_1"] == 1)
    print(f"OBS prc lattice: rows covered by equality only: {int(tie_2.sum())} of F2, {int(tie_1.sum())} of F1; "
          f"counts {ref['counts']}")
    assert tie_2.sum() + tie_1.sum() >= 1
    assert 0 < ref["counts"][0] < len(f2) and 0 < ref["counts"][1] < len(f1)
    # on the lattice a float64 direct difference is exact as well
    d = ((f2.astype(np.float64)[:, None, :] - f1.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    assert np.array_equal((d <= r1[None, :]).any(axis=1).astype(np.int64), ref["hit_2"])
