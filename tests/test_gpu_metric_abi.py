"""Kernel-level parity of csrc/metric_kernels.hip: ffc_feat_moments_update, ffc_kid_sums and ffc_isc_sums called
through the C ABI with raw pointers against the wide references of tests/metric_refs.py (np.longdouble), under the
bounds derived there.  Outputs, states and workspaces sit in NaN-filled allocations with 64 NaN elements behind
them (abi_bufs.Buf): after a call every element in range is finite and every other one is still NaN; after a
rejection everything is still NaN.  Misaligned feature pointers start one float off 16-byte alignment.

Inputs -> what they are there for
  moments   D 1, 5, 16, 17, 40, 130 (below, at and above one 16-wide MFMA tile, one 64-wide workgroup tile and two
            of them with a part-filled third); three updates of B from 1, 3, 17, 70 (a first batch of one row, a
            part-filled k-step of 4, more than two 32-row chunks); features offset by +100 so that without the
            pivot the covariance would lose seven digits; small asymmetric integers, where every sum is exact
  KID       m 2, 17, 65 (one tile, a second tile of one row), D 3, 64, 130 (part of a 32-wide k chunk, whole
            chunks, a ragged fifth), tables that share rows between subsets in non-monotone order, degree 1 and 3
  ISC       (N, C, splits) (10, 2, 10), (23, 10, 10), (101, 1008, 10), (7, 5, 1); logits over +-40
"""
import numpy as np
import pytest
import torch

import abi_bufs as B
import metric_refs as R
from abi_bufs import Buf

pytestmark = pytest.mark.gpu
F64 = torch.float64


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    B.end_of_test()


def _share(err, bound):
    """largest |err| / bound (0 / 0 = 0)"""
    err, bound = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r))


def _report(what, sh):
    print(f"OBS {what} " + " ".join(f"{k} {v:.3f}" for k, v in sh.items()))
    bad = {k: v for k, v in sh.items() if not v <= 1.0}
    assert not bad, (what, bad)


def _ints(t):
    return B.keep(torch.as_tensor(t, dtype=torch.int64).contiguous().to(B.DEV))


# --------------------------------------------------------------------------- moments
def _state(D):
    n = B.lib().ffc_feat_moments_state_doubles(D)
    assert n == 1 + 2 * D + D * D
    return Buf(n, dtype=F64, fill=np.zeros(n))


def _update(state, x, mis=False):
    xb = Buf(x.size, fill=x, mis=mis)
    B.ok(B.lib().ffc_feat_moments_update(xb.ptr(), x.shape[0], x.shape[1], state.ptr(), B.stream()), "ffc_feat_moments_update")
    return xb


def _unpack(state, D):
    s = state.get("state").numpy()
    return s[0], s[1:1 + D].copy(), s[1 + D:1 + 2 * D].copy(), s[1 + 2 * D:].reshape(D, D).copy()


def _batches(D, sizes, seed):
    rng = np.random.default_rng(seed)
    scale = 0.5 + rng.random(D)
    return [(100.0 + scale * rng.standard_normal((b, D)) + 0.1 * np.arange(D)).astype(np.float32) for b in sizes]


@pytest.mark.parametrize("sizes", [(17, 1, 70), (1, 3, 70), (70, 3, 17)])
@pytest.mark.parametrize("D", [1, 5, 16, 17, 40, 130])
def test_moments_match_the_wide_reference(D, sizes):
    batches = _batches(D, sizes, 100 * D + sizes[0])
    runs = []
    for _ in range(2):
        st = _state(D)
        for k, x in enumerate(batches):
            _update(st, x, mis=(k + D) % 2 == 1)
        runs.append(_unpack(st, D))
    n, pivot, s1, S2 = runs[0]
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1])), "two runs differ"
    assert n == sum(sizes)
    assert np.array_equal(S2, S2.T), "S2 is not exactly symmetric"
    first = batches[0]
    piv_ref = R.column_mean(first)
    piv_bound = (first.shape[0] + 1) * R.U * np.abs(first.astype(np.float64)).sum(axis=0) / first.shape[0]
    ref = R.moments(batches, pivot)
    b1, b2 = R.moments_bounds(ref)
    _report(f"moments D={D} B={sizes}", dict(pivot=_share(R.lower(R.lift(pivot) - piv_ref), piv_bound),
                                           s1=_share(R.lower(R.lift(s1) - ref["s1"]), b1),
                                           S2=_share(R.lower(R.lift(S2) - ref["S2"]), b2)))


def test_moments_of_asymmetric_integers_are_exact():
    D = 130
    i, j = np.meshgrid(np.arange(7), np.arange(D), indexing="ij")
    x = (((3 * i + 5 * j + (i * j) % 4) % 9) - 3).astype(np.float32)   # rows 0..3 first: a column mean in quarters
    st = _state(D)
    _update(st, x[:4])
    _update(st, x[4:], mis=True)
    n, pivot, s1, S2 = _unpack(st, D)
    xd = x.astype(np.float64)
    p = xd[:4].mean(axis=0)
    d = xd - p
    assert n == 7 and np.array_equal(pivot, p) and np.array_equal(s1, d.sum(axis=0))
    want = d.T @ d   # multiples of 1/16 below 2^10: exact in any order
    assert not np.array_equal(want, want[::-1, ::-1]) and np.array_equal(S2, want), np.argwhere(S2 != want)[:8]


# --------------------------------------------------------------------------- KID
def _kid_inputs(m, D, subsets, seed):
    rng = np.random.default_rng(seed)
    n1, n2 = m + 5, m + 9
    f1 = rng.standard_normal((n1, D)).astype(np.float32)
    f2 = (0.3 + 1.2 * rng.standard_normal((n2, D))).astype(np.float32)
    idx1 = np.stack([rng.permutation(n1)[:m] for _ in range(subsets)]).astype(np.int64)
    idx2 = np.stack([rng.permutation(n2)[:m][::-1] for _ in range(subsets)]).astype(np.int64)
    return f1, f2, idx1, idx2


def _kid(f1, f2, i1, i2, deg, gam, c0, mis=False, **over):
    S, m = i1.shape
    a = dict(F1=Buf(f1.size, fill=f1, mis=mis).ptr(), N1=f1.shape[0], F2=Buf(f2.size, fill=f2).ptr(), N2=f2.shape[0],
             D=f1.shape[1], idx1=_ints(i1).data_ptr(), idx2=_ints(i2).data_ptr(), S=S, m=m, degree=deg, gamma=gam, coef0=c0)
    a.update(over)
    nws = B.lib().ffc_kid_ws_doubles(S, m)
    ws, sums = Buf(max(nws, 1), dtype=F64), Buf(6 * S, dtype=F64)
    a.setdefault("ws", ws.ptr())
    a.setdefault("nws", nws)
    a.setdefault("sums", sums.ptr())
    rc = B.lib().ffc_kid_sums(a["F1"], a["N1"], a["F2"], a["N2"], a["D"], a["idx1"], a["idx2"], a["S"], a["m"], a["degree"],
                              a["gamma"], a["coef0"], a["ws"], a["nws"], a["sums"], B.stream())
    return rc, ws, sums


@pytest.mark.parametrize("degree", [1, 3])
@pytest.mark.parametrize("subsets", [1, 3])
@pytest.mark.parametrize("D", [3, 64, 130])
@pytest.mark.parametrize("m", [2, 17, 65])
def test_kid_sums_match_the_wide_reference(m, D, subsets, degree):
    f1, f2, idx1, idx2 = _kid_inputs(m, D, subsets, 1000 * m + 10 * D + subsets)
    if subsets > 1 and m >= 17:
        assert len(np.intersect1d(idx1[0], idx1[1])) and np.any(np.diff(idx2[0]) < 0)
    gamma, coef0 = (1.0 / D, 1.0) if degree == 3 else (0.25, -0.5)
    got = []
    for rep in range(2):
        rc, ws, sums = _kid(f1, f2, idx1, idx2, degree, gamma, coef0, mis=(m + D) % 2 == 1)
        B.ok(rc, "ffc_kid_sums")
        got.append(sums.get("sums").numpy().reshape(subsets, 6))
        ws.get("ws")
    assert np.array_equal(got[0], got[1]), "two runs differ"
    ref, bounds = R.kid_sums(f1, f2, idx1, idx2, degree, gamma, coef0)
    err = R.lower(R.lift(got[0]) - ref)
    _report(f"kid m={m} D={D} subsets={subsets} degree={degree}",
            {name: _share(err[:, k], bounds[:, k]) for k, name in enumerate(("xx", "dxx", "yy", "dyy", "xy", "txy"))})


@pytest.mark.parametrize("which,value", [("idx1", None), ("idx2", -1)])
def test_kid_index_out_of_range_makes_only_its_subset_nan(which, value):
    f1, f2, idx1, idx2 = _kid_inputs(17, 64, 3, 5)
    rc, _, clean = _kid(f1, f2, idx1, idx2, 3, 1.0 / 64, 1.0)
    B.ok(rc, "ffc_kid_sums")
    clean = clean.get("sums").numpy().reshape(3, 6)
    bad = dict(idx1=idx1.copy(), idx2=idx2.copy())
    bad[which][1, 3] = (f1.shape[0] if which == "idx1" else f2.shape[0]) if value is None else value
    rc, _, sums = _kid(f1, f2, bad["idx1"], bad["idx2"], 3, 1.0 / 64, 1.0)
    B.ok(rc, "ffc_kid_sums")
    got = sums.raw().numpy().reshape(3, 6)
    assert np.isnan(got[1]).all(), got[1]
    assert np.array_equal(got[[0, 2]], clean[[0, 2]])


# --------------------------------------------------------------------------- ISC
def _isc(lg, pm, splits, mis=False, **over):
    N, C = lg.shape
    a = dict(logits=Buf(lg.size, fill=lg, mis=mis).ptr(), N=N, C=C, perm=_ints(pm).data_ptr(), splits=splits)
    a.update(over)
    nws = B.lib().ffc_isc_ws_doubles(N, C, splits)
    ws, out = Buf(max(nws, 1), dtype=F64), Buf(max(splits, 1) * (4 + C), dtype=F64)
    a.setdefault("ws", ws.ptr())
    a.setdefault("nws", nws)
    a.setdefault("out", out.ptr())
    rc = B.lib().ffc_isc_sums(a["logits"], a["N"], a["C"], a["perm"], a["splits"], a["ws"], a["nws"], a["out"], B.stream())
    return rc, ws, out


def _logits(N, C, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-40.0, 40.0, size=(N, C))
    x[::5] *= 0.04
    return x.astype(np.float32)


@pytest.mark.parametrize("N,C,splits", [(10, 2, 10), (23, 10, 10), (101, 1008, 10), (7, 5, 1)])
def test_isc_sums_match_the_wide_reference(N, C, splits):
    logits = _logits(N, C, N + C)
    perm = np.random.default_rng(3).permutation(N).astype(np.int64)
    got = []
    for rep in range(2):
        rc, ws, out = _isc(logits, perm, splits, mis=rep == 1)
        B.ok(rc, "ffc_isc_sums")
        got.append(out.get("out").numpy().reshape(splits, 4 + C))
    assert np.array_equal(got[0], got[1]), "two runs (aligned, one float off) differ"
    ref = R.isc_chunks(logits, perm, splits)
    assert [int(v) for v in got[0][:, 0]] == [(i + 1) * N // splits - i * N // splits for i in range(splits)] == \
        [c["n"] for c in ref]
    sh = dict(A=0.0, E=0.0, colsum=0.0, score=0.0)
    for g, c in zip(got[0], ref):
        sh["A"] = max(sh["A"], _share(g[1] - c["A"], (C + N + 16) * R.U * c["abs_plogp"]))
        sh["E"] = max(sh["E"], _share(g[2] - c["E"], c["bound"]))
        sh["colsum"] = max(sh["colsum"], _share(g[4:] - c["colsum"], (C + N + 16) * R.U * c["colsum"]))
        sh["score"] = max(sh["score"], _share(g[3] - c["score"], c["score"] * (np.expm1(c["bound"]) + 4 * R.U)))
    _report(f"isc N={N} C={C} splits={splits}", sh)


def test_isc_perm_out_of_range_makes_only_its_chunk_nan():
    logits = _logits(23, 10, 9)
    perm = np.arange(23, dtype=np.int64)[::-1].copy()
    rc, _, clean = _isc(logits, perm, 10)
    B.ok(rc, "ffc_isc_sums")
    clean = clean.get("out").numpy().reshape(10, 14)
    perm[5] = 23   # rows 4, 5 are chunk 2 (2 * 23 // 10 = 4, 3 * 23 // 10 = 6)
    rc, _, out = _isc(logits, perm, 10)
    B.ok(rc, "ffc_isc_sums")
    got = out.raw().numpy().reshape(10, 14)
    assert got[2, 0] == 2 and np.isnan(got[2, 1:]).all()
    keep = [i for i in range(10) if i != 2]
    assert np.array_equal(got[keep], clean[keep])


# --------------------------------------------------------------------------- rejections
def test_rejections_write_nothing():
    x = _batches(5, (3,), 1)[0]
    count = 0

    def fm(word, **over):
        nonlocal count
        st = Buf(36, dtype=F64)
        a = dict(X=Buf(x.size, fill=x).ptr(), B=3, D=5, state=st.ptr())
        a.update(over)
        B.rejected(B.lib().ffc_feat_moments_update(a["X"], a["B"], a["D"], a["state"], B.stream()), "ffc_feat_moments_update", word)
        assert st.untouched(), word
        count += 1

    fm("X null", X=None)
    fm("X null or not aligned", X=Buf(x.size, fill=x).ptr() + 2)
    fm("state null", state=None)
    fm("state null or not aligned", state=Buf(40, dtype=F64).ptr() + 4)
    fm("B >= 1", B=0)
    fm("D out of range", D=0)
    fm("D out of range", D=2049)
    assert B.lib().ffc_feat_moments_state_doubles(0) == 0 and B.lib().ffc_feat_moments_state_doubles(2049) == 0

    f1, f2, idx1, idx2 = _kid_inputs(17, 5, 2, 2)

    def kid(word, **over):
        nonlocal count
        rc, ws, sums = _kid(f1, f2, idx1, idx2, 3, 0.2, 1.0, **over)
        B.rejected(rc, "ffc_kid_sums", word)
        assert ws.untouched() and sums.untouched(), word
        count += 1

    kid("F1 or F2 null", F1=None)
    kid("F1 or F2 null", F2=None)
    kid("not aligned to 4", F1=Buf(f1.size, fill=f1).ptr() + 1)
    kid("idx1 or idx2 null", idx1=None)
    kid("idx1 or idx2 null", idx2=None)
    kid("not aligned to 8", idx2=_ints(np.zeros(40)).data_ptr() + 4)
    kid("ws or sums null", ws=None)
    kid("ws or sums null", sums=None)
    kid("N1, N2 >= 1", N1=0)
    kid("N1, N2 >= 1", N2=0)
    kid("D out of range", D=0)
    kid("D out of range", D=2049)
    kid("m < 2", m=1)
    kid("subsets out of range", S=0)
    kid("subsets out of range", S=65536)
    kid("degree >= 1", degree=0)
    kid("finite", gamma=float("nan"))
    kid("finite", coef0=float("inf"))
    kid("workspace too small", nws=B.lib().ffc_kid_ws_doubles(2, 17) - 1)

    logits, perm = _logits(23, 10, 1), np.arange(23, dtype=np.int64)

    def isc(word, splits=10, **over):
        nonlocal count
        rc, ws, out = _isc(logits, perm, splits, **over)
        B.rejected(rc, "ffc_isc_sums", word)
        assert ws.untouched() and out.untouched(), word
        count += 1

    isc("logits null", logits=None)
    isc("logits null or not aligned", logits=Buf(logits.size, fill=logits).ptr() + 2)
    isc("perm null", perm=None)
    isc("perm null or not aligned", perm=_ints(np.zeros(40)).data_ptr() + 4)
    isc("ws or out null", ws=None)
    isc("ws or out null", out=None)
    isc("C out of range", C=0)
    isc("C out of range", C=1025)
    isc("splits out of range", splits=0)
    isc("splits out of range", splits=65536)
    isc("N < splits", splits=24)
    isc("N too large", N=2 ** 31)
    isc("workspace too small", nws=B.lib().ffc_isc_ws_doubles(23, 10, 10) - 1)
    assert B.lib().ffc_isc_ws_doubles(5, 10, 10) == 0 and B.lib().ffc_isc_ws_doubles(23, 1025, 10) == 0
    # the same operands are accepted as they are
    rc, _, out = _isc(logits, perm, 10)
    B.ok(rc, "ffc_isc_sums")
    assert np.isfinite(out.get("out").numpy()).all()
    print(f"OBS {count} wrong calls refused with nothing written")
