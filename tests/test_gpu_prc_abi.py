"""Kernel-level parity of csrc/prc_kernels.hip: ffc_prc called through the C ABI with raw pointers against the wide
direct-difference reference of tests/prc_refs.py, under the bounds derived there (per pair (D + 8) U sum (|a| + |b|)^2;
a radius the largest of its row; a coverage margin the largest of pair + radius bound).  Every buffer sits in a
NaN-filled allocation with 64 NaN elements behind it (abi_bufs.Buf; the int flag arrays live in fp32 buffers, whose
NaN fill is no 0 or 1): after a call every output element is finite and every guard element is still NaN; after a
rejection everything is still NaN.  Misaligned feature pointers start one float off 16-byte alignment.

Inputs -> what they are there for
  shapes    (N1, N2) (4, 4), (5, 63), (64, 65), (65, 130), (130, 64): fewer rows than one MFMA tile, a part-filled
            and a whole 64-row workgroup tile, a second tile of one row, a part-filled third; D 1, 3, 32, 33, 130
            (part of a 32-wide k chunk, one whole chunk, a second of one element, a ragged fifth); k 1, 3, 7 wherever
            N >= k + 1; features offset by +3 so that the norms cancel two digits
  strips    (2100, 1030) at D = 8: three column strips of 1024 for F1, the last of 52 columns in one part-filled
            tile; two for F2, the last of 6 columns
  fixtures  cases A and B of tests/golden/metrics_prc.npz: every row's margin is beyond 1000 x its bound
            (test_prc_refs_cpu.py), so every flag is demanded and the counts must be the reference's
  lattice   small integers with duplicated rows: radii, flags and counts exact, rows decided by d2 == r2, r2 = 0
"""
import functools
import os

import numpy as np
import pytest
import torch

import abi_bufs as B
import prc_refs as P
from abi_bufs import Buf
from conftest import ROOT

pytestmark = pytest.mark.gpu
F64 = torch.float64
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "metrics_prc.npz"))


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    B.end_of_test()


def _call(f1, f2, k, mis=False, **over):
    """-> (status, dict of the output Bufs)"""
    N1, N2 = len(f1), len(f2)
    nws = B.lib().ffc_prc_ws_bytes(N1, N2, k)
    o = dict(r1=Buf(N1, dtype=F64), r2=Buf(N2, dtype=F64), hit_2=Buf(N2), hit_1=Buf(N1), counts=Buf(2, dtype=F64),
             ws=Buf(max(nws // 8, N1 + N2 + 8), dtype=F64))
    a = dict(F1=Buf(f1.size, fill=f1, mis=mis).ptr(), N1=N1, F2=Buf(f2.size, fill=f2, mis=mis).ptr(), N2=N2,
             D=f1.shape[1], k=k, nws=nws, **{name: b.ptr() for name, b in o.items()})
    a.update(over)
    rc = B.lib().ffc_prc(a["F1"], a["N1"], a["F2"], a["N2"], a["D"], a["k"], a["r1"], a["r2"], a["hit_2"], a["hit_1"],
                         a["counts"], a["ws"], a["nws"], B.stream())
    return rc, o


def _flags(buf, what):
    bits = buf.get(what).view(torch.int32).numpy()
    assert np.isin(bits, (0, 1)).all(), f"{what}: a flag that is neither 0 nor 1"
    return bits.astype(np.int64)


def _read(o, N1, N2):
    """the outputs on the host, every element written and every guard element still NaN"""
    ws = o["ws"]
    torch.cuda.synchronize()
    data = ws.buf.cpu()
    assert bool(torch.isnan(data[:ws.off]).all()) and bool(torch.isnan(data[ws.off + ws.n:]).all()), "ws: wrote outside"
    assert bool(torch.isfinite(data[ws.off:ws.off + N1 + N2]).all()), "ws: norms"
    return dict(r1=o["r1"].get("radii2_1").numpy(), r2=o["r2"].get("radii2_2").numpy(), hit_2=_flags(o["hit_2"], "hit_2"),
                hit_1=_flags(o["hit_1"], "hit_1"), counts=o["counts"].get("counts").numpy())


def _run(f1, f2, k):
    """two aligned runs and one with both feature pointers one float off: bitwise equal; -> the first"""
    got = []
    for mis in (False, False, True):
        rc, o = _call(f1, f2, k, mis=mis)
        B.ok(rc, "ffc_prc")
        got.append(_read(o, len(f1), len(f2)))
    for other, what in ((got[1], "two runs differ"), (got[2], "misaligned feature pointers change the bits")):
        assert all(np.array_equal(got[0][key], other[key]) for key in got[0]), what
    return got[0]


def _check(got, ref, what, every_row=False):
    """radii within their bounds; every flag whose margin exceeds its bound; counts = the flag sums"""
    share = {}
    for s in (1, 2):
        err = np.abs(P.lower(P.lift(got[f"r{s}"]) - ref[f"radii2_{s}"]))
        share[f"r{s}"] = float(np.max(err / ref[f"rbound_{s}"]))
    decided = {s: np.abs(ref[f"margin_{s}"]) > ref[f"mbound_{s}"] for s in (1, 2)}
    n_dec, n_all = sum(int(d.sum()) for d in decided.values()), sum(d.size for d in decided.values())
    print(f"OBS {what}: r2_1 {share['r1']:.3f} r2_2 {share['r2']:.3f} of the bound; {n_dec} of {n_all} flags demanded; "
          f"counts {got['counts'].tolist()}")
    assert share["r1"] <= 1.0 and share["r2"] <= 1.0, share
    if every_row:
        assert n_dec == n_all, "a row of the fixture within its bound"
    assert n_dec >= 0.9 * n_all, "the inputs decide too few rows"
    for s in (1, 2):
        d = decided[s]
        assert np.array_equal(got[f"hit_{s}"][d], ref[f"hit_{s}"][d]), (what, s, np.flatnonzero(got[f"hit_{s}"] != ref[f"hit_{s}"]))
    assert got["counts"].tolist() == [float(got["hit_2"].sum()), float(got["hit_1"].sum())]
    if n_dec == n_all:
        assert got["counts"].tolist() == [float(c) for c in ref["counts"]]


def _features(n1, n2, d, seed):
    rng = np.random.default_rng(seed)
    f1 = (3.0 + rng.standard_normal((n1, d))).astype(np.float32)
    f2 = (3.1 + 0.9 * rng.standard_normal((n2, d))).astype(np.float32)
    return f1, f2


@functools.lru_cache(maxsize=None)
def _shape_case(n1, n2, d, k):
    f1, f2 = _features(n1, n2, d, 1000 * n1 + 10 * d + n2)
    return f1, f2, P.prc(f1, f2, k)


SHAPES = [(4, 4), (5, 63), (64, 65), (65, 130), (130, 64)]


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("D", [1, 3, 32, 33, 130])
@pytest.mark.parametrize("N1,N2", SHAPES)
def test_radii_flags_and_counts_match_the_wide_reference(N1, N2, D, k):
    if min(N1, N2) < k + 1:
        rc, o = _call(*_features(N1, N2, D, 1), k)
        B.rejected(rc, "ffc_prc", "N1, N2 >= neighborhood + 1")
        assert all(b.untouched() for b in o.values())
        return
    f1, f2, ref = _shape_case(N1, N2, D, k)
    _check(_run(f1, f2, k), ref, f"prc N=({N1}, {N2}) D={D} k={k}")


def test_three_column_strips_with_a_ragged_last_one():
    f1, f2 = _features(2100, 1030, 8, 5)
    _check(_run(f1, f2, 3), P.prc(f1, f2, 3), "prc N=(2100, 1030) D=8 k=3")


@pytest.mark.parametrize("case,k", [("a", 3), ("a", 1), ("b", 3)])
def test_fixture_rows_are_all_decided_as_the_reference_decides(case, k):
    f1, f2 = GOLD[f"{case}_f1"], GOLD[f"{case}_f2"]
    got = _run(f1, f2, k)
    _check(got, P.prc(f1, f2, k), f"prc fixture {case} k={k}", every_row=True)
    precision, recall, _ = GOLD[f"{case}_k{k}_0"]
    assert got["counts"].tolist() == [round(precision * len(f2)), round(recall * len(f1))]


@pytest.mark.parametrize("k", [1, 3])
def test_integer_lattice_is_exact(k):
    f1, f2 = P.lattice()
    ref = P.prc(f1, f2, k)
    got = _run(f1, f2, k)
    r1, r2 = P.lower(ref["radii2_1"]), P.lower(ref["radii2_2"])
    ties = int(((ref["margin_2"] == 0) & (ref["hit_2"] == 1)).sum() + ((ref["margin_1"] == 0) & (ref["hit_1"] == 1)).sum())
    print(f"OBS prc lattice k={k}: {ties} rows decided by d2 == r2, {int((r1 == 0).sum() + (r2 == 0).sum())} radii 0, "
          f"counts {got['counts'].tolist()}")
    assert ties >= 1 and (r1 == 0).any()
    assert np.array_equal(got["r1"], r1) and np.array_equal(got["r2"], r2)
    assert np.array_equal(got["hit_2"], ref["hit_2"]) and np.array_equal(got["hit_1"], ref["hit_1"])
    assert got["counts"].tolist() == [float(c) for c in ref["counts"]]


def test_rejections_write_nothing():
    f1, f2 = _features(9, 12, 5, 2)
    count = 0

    def no(word, k=3, **over):
        nonlocal count
        rc, o = _call(f1, f2, k, **over)
        B.rejected(rc, "ffc_prc", word)
        assert all(b.untouched() for b in o.values()), word
        count += 1

    no("F1 or F2 null", F1=None)
    no("F1 or F2 null", F2=None)
    no("not aligned to 4", F1=Buf(f1.size, fill=f1).ptr() + 2)
    no("not aligned to 4", F2=Buf(f2.size, fill=f2).ptr() + 1)
    no("radii2_1 or radii2_2 null", r1=None)
    no("radii2_1 or radii2_2 null", r2=None)
    no("not aligned to 8", r1=Buf(16, dtype=F64).ptr() + 4)
    no("hit_2 or hit_1 null", hit_2=None)
    no("hit_2 or hit_1 null", hit_1=None)
    no("not aligned to 4", hit_1=Buf(16).ptr() + 2)
    no("counts or ws null", counts=None)
    no("counts or ws null", ws=None)
    no("not aligned to 8", ws=Buf(256, dtype=F64).ptr() + 4)
    no("D out of range", D=0)
    no("D out of range", D=4097)
    no("neighborhood out of range", k=0)
    no("neighborhood out of range", k=8)
    no("N1, N2 >= neighborhood + 1", N1=3)
    no("N1, N2 >= neighborhood + 1", N2=3)
    no("N1, N2 >= neighborhood + 1", k=7, N1=7)
    no("too large", N1=64 * 65535 + 1)
    no("workspace too small", nws=B.lib().ffc_prc_ws_bytes(9, 12, 3) - 1)
    # the same operands are accepted as they are
    rc, o = _call(f1, f2, 3)
    B.ok(rc, "ffc_prc")
    _read(o, 9, 12)
    print(f"OBS {count} wrong calls refused with nothing written")


def test_workspace_replaces_the_three_matrices():
    ws = B.lib().ffc_prc_ws_bytes
    assert 0 < ws(50000, 50000, 3) < 128 * 2 ** 20   # the matrices it replaces are 20 GB each in fp64
    assert ws(3, 50, 3) == 0 and ws(50, 3, 3) == 0 and ws(50, 50, 0) == 0 and ws(50, 50, 8) == 0
    assert ws(64 * 65535 + 1, 50, 3) == 0
