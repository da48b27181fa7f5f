"""The library's environment readers (csrc/ffc_env.h: env_int, env_first, env_is) and what every
A/B knob of csrc/ makes of them, on the host: tests/native/env_readers_host.cpp includes the header
alone (no HIP) and is run once per value with every knob's variable set to it.

KNOBS holds, per knob, the expression at its call site (asserted to be in the source file, so the
table cannot drift from the code), the reader query behind it, the predicate the call site applies
and the result for each of VALUES.  The results are literals worked out by hand from the lambdas the
readers replaced (`e ? atoi(e) : d`, `e && e[0] == 'c'`, `e && std::string(e) == "w"`, ...): the
knobs' parses must stay what they were."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastfourierconvolution_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "native", "env_readers_host.cpp")

#          unset  empty                                garbage      more integers and words
VALUES = [None, "", "0", "1", "2", "split", "f32", "x9", "3", "4", "64", "old", "-7"]
T, F = True, False
ATOI = [0, 0, 0, 1, 2, 0, 0, 0, 3, 4, 64, 0, -7]    # `e ? atoi(e) : 0`
FIRST = [0, 0, 48, 49, 50, ord("s"), ord("f"), ord("x"), 51, 52, 54, ord("o"), ord("-")]   # first character
Q = "QSLOTS"                                        # convq's compiled-in default


def only(i, hit=T):
    return [hit if j == i else (not hit) for j in range(len(VALUES))]


# (variable, source file, call-site expression, query, predicate on the reader's value, results)
KNOBS = [
    ("FFC_FU_KGROUPS", "fu_kernels.hip", 'ffc::env_int("FFC_FU_KGROUPS", -1)', ("int", "-1"),
     lambda v: v == 2, only(4)),                                             # ffc_fu_kgroups: env != 2 -> off
    ("FFC_FU_MFMA", "fu_kernels.hip", "fu_mfma_env() == 's'", ("first",), lambda c: c == ord("s"), only(5)),
    ("FFC_FU_MFMA", "fu_kernels.hip", "fu_mfma_env() == 'f'", ("first",), lambda c: c == ord("f"), only(6)),
    ("FFC_FU_MFMA", "fu_kernels.hip", 'ffc::env_first("FFC_FU_MFMA")', ("first",), lambda c: c, FIRST),
    ("FFC_FU_SHUF", "fu_kernels.hip", """ffc::env_first("FFC_FU_SHUF") == '1'""", ("first",),
     lambda c: c == ord("1"), only(3)),
    ("FFC_FU_SPLIT", "fu_kernels.hip", """ffc::env_first("FFC_FU_SPLIT") != '0'""", ("first",),
     lambda c: c != ord("0"), only(2, F)),
    ("FFC_FU_MGROUPS", "fu_kernels.hip", 'ffc::env_int("FFC_FU_MGROUPS", 0)', ("int", "0"), lambda v: v, ATOI),
    ("FFC_CONVQ_PERSIST", "convq_kernels.hip", """ffc::env_first("FFC_CONVQ_PERSIST") == '0'""", ("first",),
     lambda c: c == ord("0"), only(2)),
    ("FFC_CONVQ_PX", "convq_kernels.hip", 'ffc::env_int("FFC_CONVQ_PX", 0)', ("int", "0"), lambda v: v, ATOI),
    ("FFC_CONVQ_SLOTS11", "convq_kernels.hip", 'ffc::env_int("FFC_CONVQ_SLOTS11", 0)', ("int", "0"),
     lambda n: n if n in (3, 4) else Q, [Q, Q, Q, Q, Q, Q, Q, Q, 3, 4, Q, Q, Q]),
    ("FFC_WGRAD_BK", "train_kernels.hip", 'ffc::env_int("FFC_WGRAD_BK", 0)', ("int", "0"), lambda v: v, ATOI),
    ("FFC_WGRAD_ARITH", "train_kernels.hip", 'ffc::env_is("FFC_WGRAD_ARITH", "f32")', ("is", "f32"),
     lambda v: v == 1, only(6)),
    ("FFC_WGRAD_KERNEL", "train_kernels.hip", 'ffc::env_is("FFC_WGRAD_KERNEL", "old")', ("is", "old"),
     lambda v: v == 1, only(11)),
    ("FFC_MIX_FILL", "fu2d_kernels.hip", 'ffc::env_int("FFC_MIX_FILL", 0)', ("int", "0"),
     lambda n: n if n > 0 else 512, [512, 512, 512, 1, 2, 512, 512, 512, 3, 4, 64, 512, 512]),
    ("FFC_HEAD_TR", "convt_smallm.hip", 'ffc::env_int("FFC_HEAD_TR", 32) == 64 ? 64 : 32', ("int", "32"),
     lambda v: 64 if v == 64 else 32, [32] * 10 + [64, 32, 32]),
    ("FFC_DENSE_VEC", "dense.hip", """ffc::env_first("FFC_DENSE_VEC") != '0'""", ("first",),
     lambda c: c != ord("0"), only(2, F)),
    ("FFC_BN_RED2_MIN", "bn_se_kernels.hip", 'std::max(1, ffc::env_int("FFC_BN_RED2_MIN", RED2_MIN_ROWS))',
     ("int", "1024"), lambda v: max(1, v), [1024, 1024, 1, 1, 2, 1, 1, 1, 3, 4, 64, 1, 1]),
]
# the readers themselves on a variable no knob uses
RAW = [
    (("int", "7"), [7, 7, 0, 1, 2, 0, 0, 0, 3, 4, 64, 0, -7]),
    (("first",), FIRST),
    (("is", "f32"), [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]),
    (("is", "f3"), [0] * len(VALUES)),   # whole words only
]
RAW_VAR = "FFC_TEST_ONLY_READER"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    out = str(tmp_path_factory.mktemp("env_readers") / "env_readers_host")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", CSRC, DRIVER, "-o", out], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _query(q, var):
    return [q[0], var, *q[1:]]


@pytest.fixture(scope="module")
def answers(exe):
    """answers[i]: the driver's numbers for every query of KNOBS then RAW, all variables = VALUES[i]"""
    args = [a for k in KNOBS for a in _query(k[3], k[0])] + [a for q, _ in RAW for a in _query(q, RAW_VAR)]
    names = {k[0] for k in KNOBS} | {RAW_VAR}
    out = []
    for val in VALUES:
        env = {k: v for k, v in os.environ.items() if k not in names}
        if val is not None:
            env.update({n: val for n in names})
        r = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=30)
        assert r.returncode == 0, (val, r.stderr[-1000:])
        out.append([int(x) for x in r.stdout.split()])
        assert len(out[-1]) == len(KNOBS) + len(RAW)
    return out


def test_value_list_covers_the_cases():
    assert VALUES[:8] == [None, "", "0", "1", "2", "split", "f32", "x9"]
    assert all(len(k[5]) == len(VALUES) for k in KNOBS) and all(len(w) == len(VALUES) for _, w in RAW)


@pytest.mark.parametrize("j", range(len(RAW)), ids=[" ".join(q) for q, _ in RAW])
def test_reader_values(answers, j):
    got = [a[len(KNOBS) + j] for a in answers]
    assert got == RAW[j][1], list(zip(VALUES, got, RAW[j][1]))


@pytest.mark.parametrize("j", range(len(KNOBS)), ids=[f"{k[0]}-{j}" for j, k in enumerate(KNOBS)])
def test_knob_table(answers, j):
    var, fname, site, _, pred, want = KNOBS[j]
    with open(os.path.join(CSRC, fname)) as f:
        assert site in f.read(), f"{fname} no longer reads {var} as `{site}`"
    got = [pred(a[j]) for a in answers]
    assert got == want, list(zip(VALUES, got, want))


def test_getenv_only_in_the_readers():
    """every other csrc file goes through ffc_env.h"""
    for fn in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, fn)) as f:
            if fn != "ffc_env.h":
                assert "getenv" not in f.read(), fn
