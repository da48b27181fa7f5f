"""The plan key's switches (_runtime.PLAN_KNOBS / plan_knobs()): every switch is
registered, flipping any of them changes the key, and each keeps the default and the environment
parse it had when it was a hand-written `os.environ.get` expression (the expected values below are
literals worked out from those expressions)."""
import json
import os
import subprocess
import sys

import pytest

from fastfourierconvolution_amd import _plan
from fastfourierconvolution_amd import _runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 30 members of plan_knobs() before the registry (29 of _runtime and _plan.CONVQ_TCMAX), with the
# values a clean environment gives them
DEFAULTS = {
    "USE_PATCH": True, "PW_KERNEL": "pw", "CONV_ARITH": "split", "PRESPLIT_A": False, "USE_CONVQ": True,
    "CONVQ_FORCE": False, "USE_OUTER": True, "USE_SMALLM": True, "FORCE_FU2D": False, "FU_PATH": "auto",
    "FU_FUSED_MIN_BATCH": 64, "FU_COLS": True, "FU2D_SPILL": True, "OVERLAP_SPECTRAL": False, "BN_FOLD": True,
    "BN_FOLD_MAX": 4096, "FU_SPILL": True, "ST_PATH": "auto", "ST_SPLIT": True, "ST_SPLIT_MAX": 0, "SE_SUMS": True,
    "BN_CHFOLD": False, "BN_CHFOLD_LOADS": 16, "BN_CHFOLD_READS": 16384, "ST_SPLIT_MFMA": True, "FU2D_R2CMIX": True,
    "FU_SPLIT": True, "FU_KGROUPS": True, "BN_FOLD_SYNC": True,
}
TCMAX_DEFAULT = 0

# (variable, value) -> the attributes it decides
ENV_CASES = [
    ("FFC_BN_FOLD", "0", {"BN_FOLD": False}), ("FFC_BN_FOLD", "1", {"BN_FOLD": True}),
    ("FFC_BN_FOLD", "", {"BN_FOLD": True}), ("FFC_BN_FOLD", "00", {"BN_FOLD": True}),
    ("FFC_BN_FOLD_MAX", "100", {"BN_FOLD_MAX": 100}),
    ("FFC_SE_SUMS", "0", {"SE_SUMS": False}), ("FFC_SE_SUMS", "x9", {"SE_SUMS": True}),
    ("FFC_ST_SPLIT", "0", {"ST_SPLIT": False}), ("FFC_ST_SPLIT", "2", {"ST_SPLIT": True}),
    ("FFC_ST_SPLIT_MAX", "3", {"ST_SPLIT_MAX": 2}), ("FFC_ST_SPLIT_MAX", "8", {"ST_SPLIT_MAX": 8}),
    ("FFC_ST_SPLIT_MAX", "", {"ST_SPLIT_MAX": 0}), ("FFC_ST_SPLIT_MAX", "0", {"ST_SPLIT_MAX": 1}),
    ("FFC_ST_SPLIT_MAX", "1", {"ST_SPLIT_MAX": 1}), ("FFC_ST_SPLIT_MAX", "7", {"ST_SPLIT_MAX": 4}),
    ("FFC_ST_MFMA", "f32", {"ST_SPLIT_MFMA": False}), ("FFC_ST_MFMA", "split", {"ST_SPLIT_MFMA": True}),
    ("FFC_ST_MFMA", "x9", {"ST_SPLIT_MFMA": True}), ("FFC_ST_MFMA", "", {"ST_SPLIT_MFMA": True}),
    ("FFC_FU_SPILL", "0", {"FU_SPILL": False}), ("FFC_FU_SPILL", "1", {"FU_SPILL": True}),
    ("FFC_BN_FOLD_SYNC", "0", {"BN_FOLD_SYNC": False}), ("FFC_BN_FOLD_SYNC", "2", {"BN_FOLD_SYNC": True}),
    ("FFC_BN_CHFOLD", "1", {"BN_CHFOLD": True}), ("FFC_BN_CHFOLD", "0", {"BN_CHFOLD": False}),
    ("FFC_BN_CHFOLD", "2", {"BN_CHFOLD": False}), ("FFC_BN_CHFOLD", "", {"BN_CHFOLD": False}),
    ("FFC_BN_CHFOLD_LOADS", "4", {"BN_CHFOLD_LOADS": 4}), ("FFC_BN_CHFOLD_READS", "1024", {"BN_CHFOLD_READS": 1024}),
    ("FFC_FU_SPLIT", "00", {"FU_SPLIT": False}), ("FFC_FU_SPLIT", "0", {"FU_SPLIT": False}),
    ("FFC_FU_SPLIT", "1", {"FU_SPLIT": True}), ("FFC_FU_SPLIT", "", {"FU_SPLIT": True}),
    ("FFC_FU_SPLIT", "x9", {"FU_SPLIT": True}), ("FFC_FU_SPLIT", "split", {"FU_SPLIT": True}),
    ("FFC_PW_KERNEL", "gemm", {"PW_KERNEL": "gemm"}), ("FFC_PW_KERNEL", "patch", {"PW_KERNEL": "patch"}),
    ("FFC_PW_KERNEL", "", {"PW_KERNEL": ""}),
    ("FFC_CONV_ARITH", "f32", {"CONV_ARITH": "f32"}), ("FFC_CONV_ARITH", "split", {"CONV_ARITH": "split"}),
    ("FFC_CONVP_PRESPLIT", "1", {"PRESPLIT_A": True}), ("FFC_CONVP_PRESPLIT", "2", {"PRESPLIT_A": False}),
    ("FFC_CONVQ", "force", {"USE_CONVQ": True, "CONVQ_FORCE": True}),
    ("FFC_CONVQ", "1", {"USE_CONVQ": True, "CONVQ_FORCE": True}),
    ("FFC_CONVQ", "0", {"USE_CONVQ": False, "CONVQ_FORCE": False}),
    ("FFC_CONVQ", "auto", {"USE_CONVQ": True, "CONVQ_FORCE": False}),
    ("FFC_CONVQ", "", {"USE_CONVQ": True, "CONVQ_FORCE": False}),
    ("FFC_CONVQ", "x9", {"USE_CONVQ": True, "CONVQ_FORCE": False}),
    ("FFC_ST_PATH", "pw", {"ST_PATH": "pw"}), ("FFC_FU_PATH", "staged", {"FU_PATH": "staged"}),
    ("FFC_FU_PATH", "fused", {"FU_PATH": "fused"}),
    ("FFC_FU2D_SPILL", "0", {"FU2D_SPILL": False}), ("FFC_FU2D_SPILL", "1", {"FU2D_SPILL": True}),
    ("FFC_FU2D_R2CMIX", "0", {"FU2D_R2CMIX": False}), ("FFC_FU2D_R2CMIX", "2", {"FU2D_R2CMIX": True}),
    ("FFC_OVERLAP", "off", {"OVERLAP_SPECTRAL": False}), ("FFC_OVERLAP", "0", {"OVERLAP_SPECTRAL": False}),
    ("FFC_OVERLAP", "false", {"OVERLAP_SPECTRAL": False}), ("FFC_OVERLAP", "", {"OVERLAP_SPECTRAL": ""}),
    ("FFC_OVERLAP", "gemm-first", {"OVERLAP_SPECTRAL": "gemm-first"}),
    ("FFC_OVERLAP", "spectral-first", {"OVERLAP_SPECTRAL": "spectral-first"}),
]

# one child for all cases: it imports _runtime afresh under each environment (a reload re-runs the
# module's top level, which is where the switches are read)
CHILD = """
import importlib, json, os, sys
cases = json.loads(sys.argv[1])
from fastfourierconvolution_amd import _plan, _runtime as rt
snap = lambda: {**{n: getattr(rt, n) for n in rt.PLAN_KNOBS}, "CONVQ_TCMAX": _plan.CONVQ_TCMAX}
out = [snap()]
for var, val in cases:
    os.environ[var] = val
    importlib.reload(rt)
    out.append(snap())
    del os.environ[var]
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def child_values():
    env = {k: v for k, v in os.environ.items() if not k.startswith("FFC_")}
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps([c[:2] for c in ENV_CASES])], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _flipped(v):
    if isinstance(v, bool):
        return not v
    return v + 1 if isinstance(v, int) else str(v) + "_other"


def test_registry_holds_every_switch():
    assert set(DEFAULTS) <= set(rt.PLAN_KNOBS) and len(set(rt.PLAN_KNOBS)) == len(rt.PLAN_KNOBS)
    # every public upper-case scalar of the module is a switch: none may stay outside the key
    scalars = {n for n, v in vars(rt).items() if n.isupper() and not n.startswith("_")
               and isinstance(v, (bool, int, str))}
    assert scalars - {"PLAN_KNOBS"} <= set(rt.PLAN_KNOBS), scalars - set(rt.PLAN_KNOBS)
    assert len(rt.plan_knobs()) == len(rt.PLAN_KNOBS) + 1 and _plan.CONVQ_TCMAX in rt.plan_knobs()


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_flipping_a_switch_changes_the_key(monkeypatch, name):
    assert name in rt.PLAN_KNOBS
    base = rt.plan_knobs()
    with monkeypatch.context() as m:
        m.setattr(rt, name, _flipped(getattr(rt, name)))
        assert rt.plan_knobs() != base
    assert rt.plan_knobs() == base


def test_every_registered_switch_changes_the_key(monkeypatch):
    base = rt.plan_knobs()
    for name in rt.PLAN_KNOBS:
        with monkeypatch.context() as m:
            m.setattr(rt, name, _flipped(getattr(rt, name)))
            assert rt.plan_knobs() != base, name
        assert rt.plan_knobs() == base, name
    with monkeypatch.context() as m:
        m.setattr(_plan, "CONVQ_TCMAX", _plan.CONVQ_TCMAX + 8)
        assert rt.plan_knobs() != base
    assert rt.plan_knobs() == base


def test_plain_assignment_changes_the_key():
    """tests and tools assign the attributes directly (rt.USE_CONVQ = False)"""
    base, old = rt.plan_knobs(), rt.USE_CONVQ
    try:
        rt.USE_CONVQ = not old
        assert rt.plan_knobs() != base
    finally:
        rt.USE_CONVQ = old
    assert rt.plan_knobs() == base


def test_defaults_in_a_clean_environment(child_values):
    clean = child_values[0]
    assert {n: clean[n] for n in DEFAULTS} == DEFAULTS
    assert all(type(clean[n]) is type(DEFAULTS[n]) for n in DEFAULTS)
    assert clean["CONVQ_TCMAX"] == TCMAX_DEFAULT


@pytest.mark.parametrize("i", range(len(ENV_CASES)), ids=[f"{v}={x}" for v, x, _ in ENV_CASES])
def test_environment_parse(child_values, i):
    _, _, want = ENV_CASES[i]
    got = child_values[i + 1]
    expect = {**DEFAULTS, **want}   # and nothing else moves
    assert {n: got[n] for n in DEFAULTS} == expect
    assert all(type(got[n]) is type(expect[n]) for n in want)


def test_no_import_time_os_lookup_idiom():
    with open(rt.__file__) as f:
        assert '__import__("os")' not in f.read()
