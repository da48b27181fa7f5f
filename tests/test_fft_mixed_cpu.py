"""The register FFTs of the fused Fourier unit (csrc/fft_reg.h: fft_reg, rfft_reg, irfft_reg) at the
3 * 2^k sizes of the mg = 6 models, compiled for the host (tests/native/fft_mixed_host.cpp includes
the kernels' own header with the device qualifiers defined away) and compared with numpy.fft in fp64.

N in {6, 12, 24, 48} (and 3, the half-size transform under rfft_reg<6>): forward and inverse complex
transforms, the real-input and real-output forms; a random input, a unit impulse at every index and
a constant.  N = 8 and 32 run through the same driver as a guard on the radix-2 path.  Bound: 1e-6
normwise (fp32 arithmetic with table twiddles: a few eps sqrt(log2 N))."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastfourierconvolution_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "native", "fft_mixed_host.cpp")
BOUND = 1e-6
MIXED = [6, 12, 24, 48]
POW2 = [8, 32]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc") \
        or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("fft_mixed") / "fft_mixed_host")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-I", CSRC, DRIVER, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _inputs(n, complex_, seed):
    """(count, n) test vectors: random, every unit impulse, a constant"""
    rng = np.random.default_rng(seed)
    vs = [rng.standard_normal(n) + (1j * rng.standard_normal(n) if complex_ else 0)]
    vs += [np.eye(n)[i] * (1 + (0.5j if complex_ else 0)) for i in range(n)]
    vs += [np.full(n, 0.75 - (0.25j if complex_ else 0))]
    return np.array(vs).astype(np.complex64 if complex_ else np.float32)


def _run(exe, kind, n, vecs):
    """vecs: (count, n) complex or real -> the driver's output rows as float64"""
    lines = [f"{kind} {n} {len(vecs)}"]
    for v in vecs:
        parts = np.concatenate([v.real, v.imag]) if np.iscomplexobj(v) else v
        lines.append(" ".join(repr(float(x)) for x in parts))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.array([[float(x) for x in ln.split()] for ln in r.stdout.strip().splitlines()])


def _err(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _check(got, want, what):
    errs = [_err(g, w) for g, w in zip(got, want)]
    print(f"{what}: max normwise err {max(errs):.3e}")
    assert max(errs) <= BOUND, (what, errs)


@pytest.mark.parametrize("inv", [False, True])
@pytest.mark.parametrize("n", [3] + MIXED + POW2)
def test_fft_reg_matches_numpy(exe, n, inv):
    x = _inputs(n, True, n)
    out = _run(exe, 1 if inv else 0, n, x)
    got = out[:, :n] + 1j * out[:, n:]
    x64 = x.astype(np.complex128)
    want = np.fft.ifft(x64, axis=-1) * n if inv else np.fft.fft(x64, axis=-1)   # the inverse is unnormalised
    _check(got, want, f"fft_reg<{n}, {inv}>")


@pytest.mark.parametrize("n", MIXED + POW2)
def test_rfft_reg_matches_numpy(exe, n):
    x = _inputs(n, False, 100 + n)
    p = n // 2 + 1
    out = _run(exe, 2, n, x)
    got = out[:, :p] + 1j * out[:, p:]
    _check(got, np.fft.rfft(x.astype(np.float64), axis=-1), f"rfft_reg<{n}>")
    assert np.all(out[:, p] == 0) and np.all(out[:, -1] == 0)   # Im X[0] = Im X[N/2] = 0 exactly


@pytest.mark.parametrize("n", MIXED + POW2)
def test_irfft_reg_matches_numpy(exe, n):
    """half spectra of real signals (and of impulses in the spectrum: one bin at a time); the imaginary
    parts of bins 0 and N/2 are ignored, as irfftn ignores them"""
    p = n // 2 + 1
    X = _inputs(p, True, 200 + n)
    got = _run(exe, 3, n, X)
    want = np.fft.irfft(X.astype(np.complex128), n=n, axis=-1) * n   # unnormalised
    _check(got, want, f"irfft_reg<{n}>")


@pytest.mark.parametrize("n", MIXED)
def test_rfft_then_irfft_round_trip(exe, n):
    x = _inputs(n, False, 300 + n)[:1]
    p = n // 2 + 1
    out = _run(exe, 2, n, x)
    spec = (out[:, :p] + 1j * out[:, p:]).astype(np.complex64)
    back = _run(exe, 3, n, spec) / n
    _check(back, x.astype(np.float64), f"round trip {n}")
