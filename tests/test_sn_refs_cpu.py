"""The bounds and inputs of tests/test_gpu_sn_abi.py, proven without a GPU (tests/sn_refs.py).

1. The index maps the references use (elem_index, mk_index: the header's matrix view) agree with torch's
   reshape_weight_to_matrix on every case.
2. sn_f32 / sn_bwd_f32, a plain fp32 restatement of csrc/sn_kernels.hip's arithmetic, stay under a quarter of
   every bound TOL * scale on every input the GPU file uses.  TOL is the smallest power of ten for which that
   holds: at 1e-6 the worst shares are 0.28 (v', rank-one case) and 0.34 (dw_orig end to end, the same case),
   so TOL = 1e-5, the bound of tests/test_gpu_sn.py, where the measured worst shares are
       p 0.024   t 0.013   v' 0.028   u' 0.022 (1000x3)   sigma 0.015 (1x16385, eval)
       dw_orig at own (u, v, sigma) 0.016 (64x260)   dw_orig end to end 0.034   (the others at the rank-one case)
   and W is bit-equal to fl(w_orig / sigma) everywhere.
3. Eleven planted defects in the restatement exceed a bound on the case named beside each.
4. The inputs' conditions: the rank-one term's median share of dw / sigma is at least 0.1 on every case, and the
   scaled case's norms stay above normalize()'s 1e-12 at 2^-40.
Every test prints what it measured."""
import functools
import warnings

import numpy as np
import pytest
import torch

import sn_refs as R


@functools.lru_cache(maxsize=None)
def _cases():
    cs = {n: R.abi_case(n) for n in R.ABI_NAMES}
    cs["rank_one"] = R.rank_one_case()
    for e in (0, 40, -40):
        cs[f"scaled 2^{e}"] = R.scaled_case(e)
    return cs


def _all_shares(c, defect=None):
    """every share of every bound for the restatement on case c; W's entry is the count of inexact elements"""
    out = {}
    for training in (True, False):
        tag = "" if training else "eval "
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)     # a planted defect may divide by a zero sigma
            out.update(_one(c, training, tag, defect))
    return out


def _one(c, training, tag, defect):
    out = {}
    if True:
        r = R.sn_f32(c, training, defect if defect in R.SN_DEFECTS else None)
        out.update({tag + k: v for k, v in R.forward_shares(c, r, training).items()})
        out[tag + "w_inexact"] = R.w_exact(c, r["w"], r["sigma"])
        if training:
            d = R.sn_bwd_f32(c, r["u"], r["v"], r["sigma"], defect if defect in R.SN_BWD_DEFECTS else None)
            out.update(R.backward_shares(c, d, r["u"], r["v"], r["sigma"]))
    return out


def test_index_maps_are_torchs_matrix_view():
    for name, c in _cases().items():
        M, K, R_, si = c["M"], c["K"], c["R"], c["stride_i"]
        flat = torch.arange(M * K, dtype=torch.float64).reshape(c["shape"])
        want = R.to_matrix(flat, c["dim"]).numpy().astype(np.int64)
        idx = R.elem_index(M, K, R_, si)
        assert np.array_equal(idx, want), name
        m, k = R.mk_index(M, K, R_, si)
        assert np.array_equal(idx[m, k], np.arange(M * K)), name
        back = R.from_matrix(torch.from_numpy(want.astype(np.float64)), c["shape"], c["dim"])
        assert torch.equal(back, flat), name


def test_plain_fp32_stays_under_a_quarter_of_every_bound():
    worst = {}
    for name, c in _cases().items():
        for k, v in _all_shares(c).items():
            if k.endswith("w_inexact"):
                assert v == 0, (name, k, v)
            elif v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, name)
    print("OBS worst shares at TOL = %g: " % R.TOL + "  ".join(f"{k} {v:.3f} ({n})" for k, (v, n) in sorted(worst.items())))
    assert all(v < 0.25 for v, _ in worst.values()), worst
    assert R.TOL <= 1e-5
    tenth = max(v for v, _ in worst.values()) * 10
    print(f"OBS at TOL / 10 the worst share would be {tenth:.3f}")
    assert tenth >= 0.25, "TOL is not the smallest power of ten"


# defect -> (the case that catches it, the bound it exceeds)
PLANTED = {
    "mk_swapped": ("T5x7x3x3", "dw_own"),             # sn_mk with m and k swapped, dim 1, R = 9
    "col_ignores_stride_i": ("T19x65x3x3", "p"),      # sn_col without stride_i
    "chunk_last_unscaled": ("127x129", "w_inexact"),  # the last element of a chunk left equal to w_orig
    "drop_last_pa": ("65x256", "p"),                  # the last row chunk's pa dropped
    "psq_short": ("8x2052", "v"),                     # psq without the last column chunk (4 of 2052 columns)
    "drop_last_pb": ("8x2049", "t"),                  # pb of the last column chunk dropped
    "nv_twice": ("17x64", "sigma"),                   # nv applied twice
    "eval_refreshed_u": ("17x64", "eval sigma"),      # eval mode using the refreshed u
    "u_next_last_row": ("257x64", "dw_own"),          # u[m + 1] for the last row in the backward
    "pdot_short": ("257x64", "dw_own"),               # pdot without the last chunk (64 of 16448 elements)
    "coef_sigma_once": ("64x260", "dw_own"),          # coef divided by sigma once
}


def test_every_defect_is_planted():
    assert set(PLANTED) == set(R.SN_DEFECTS) | set(R.SN_BWD_DEFECTS) and len(PLANTED) == 11


@pytest.mark.parametrize("defect", list(PLANTED))
def test_planted_defect_exceeds_its_bound(defect):
    name, key = PLANTED[defect]
    c = _cases()[name]
    clean, bad = _all_shares(c)[key], _all_shares(c, defect)[key]
    over = lambda k, v: v > (0 if k.endswith("w_inexact") else 1)   # noqa: E731  (W's bound is exact equality)
    caught = [n for n, cc in _cases().items() if any(over(k, v) for k, v in _all_shares(cc, defect).items())]
    print(f"OBS {defect}: {key} on {name} {clean:.3g} -> {bad:.3g}; caught on {len(caught)} of {len(_cases())} cases")
    assert clean < 0.25 and over(key, bad), (defect, name, key, clean, bad)


def test_the_rank_one_term_shows_on_every_case():
    for name, c in _cases().items():
        if name.startswith("scaled"):      # forward only on the GPU
            continue
        print(f"OBS {name}: lambda {c['lam']:g}, median |c u v| / |dw / sigma| = {c['ratio']:.3f}")
        assert c["ratio"] >= 0.1, name


def test_scaled_inputs_keep_their_norms_above_eps():
    base = _cases()["scaled 2^0"]
    for e in (40, -40):
        c = _cases()[f"scaled 2^{e}"]
        assert torch.equal(c["w"], base["w"] * 2.0 ** e) and torch.equal(c["u"], base["u"]) and torch.equal(c["v"], base["v"])
        assert torch.equal(c["w"] * 2.0 ** -e, base["w"]), "the scaling is not exact"
        Wm = R.to_matrix(c["w"].double(), 0)
        p = Wm.t() @ c["u"].double()
        t = Wm @ (p / p.norm())
        print(f"OBS 2^{e}: ||Wm^T u|| {float(p.norm()):.3e}  ||Wm v|| {float(t.norm()):.3e}")
        assert float(p.norm()) > 4e-12 and float(t.norm()) > 4e-12
        r, r0 = R.sn_f32(c, True), R.sn_f32(base, True)
        assert np.array_equal(r["u"], r0["u"]) and np.array_equal(r["v"], r0["v"])
        assert float(r["sigma"][0]) == float(r0["sigma"][0]) * 2.0 ** e


def test_degenerate_shapes():
    """M = 1: u' = +-1 exactly; K = 1: v' = +-1 exactly; sigma = ||w|| within its bound"""
    for name in ("1x1", "1x4", "4x1"):
        c = _cases()[name]
        r = R.sn_f32(c, True)
        if c["M"] == 1:
            assert abs(float(r["u"][0])) == 1.0
        if c["K"] == 1:
            assert abs(float(r["v"][0])) == 1.0
        norm = float(c["w"].double().norm())
        assert abs(float(c["train"][3]) - norm) <= 1e-12 * norm
