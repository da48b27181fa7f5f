"""Guarded device buffers for the tests that call the library through its C ABI with raw pointers
(tests/test_gpu_sn_abi.py, tests/test_gpu_aw_abi.py), after tests/test_gpu_attn_abi.py: every buffer sits in a
NaN-filled allocation with GUARD NaN elements behind it; a read-back asserts that every element in range is
finite and every other element is still NaN.  Device copies stay alive until the test ends."""
import pytest
import torch

DEV = torch.device("cuda", 0)
NAN = float("nan")
GUARD = 64
E_INVALID = -1
_LIVE = []


def keep(t):
    _LIVE.append(t)
    return t


def end_of_test():
    """the body of each file's autouse fixture, after the test: a device fault ends the file's run"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error after a kernel of this file: {e}", returncode=3)
    _LIVE.clear()


def lib():
    import fastfourierconvolution_amd  # noqa: F401  (registers torch.ops.ffc.*)
    from fastfourierconvolution_amd import _runtime as rt
    return rt.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(status, what):
    from fastfourierconvolution_amd._lib import check
    check(status, what)


def rejected(status, entry, word):
    msg = lib().ffc_last_error().decode()
    assert status == E_INVALID and entry in msg and word in msg, (status, msg, word)


class Buf:
    """n elements inside one NaN-filled allocation: four NaN elements in front (five with ``mis``: the data then
    starts one float off 16-byte alignment) and GUARD behind"""

    def __init__(self, n, mis=False, fill=None, dtype=torch.float32):
        assert not (mis and dtype != torch.float32)
        self.n, self.off, self.size = n, 5 if mis else 4, 4 if dtype == torch.float32 else 8
        self.buf = keep(torch.full((self.off + n + GUARD,), NAN, device=DEV, dtype=dtype))
        assert self.buf.data_ptr() % 16 == 0
        if fill is not None:
            self.buf[self.off:self.off + n] = torch.as_tensor(fill).to(DEV).reshape(-1).to(dtype)
        assert self.ptr() % 16 == (4 if mis else 0)

    def ptr(self, elems=0):
        return self.buf.data_ptr() + self.size * (self.off + elems)

    def raw(self):
        """the n elements on the CPU, unchecked"""
        torch.cuda.synchronize()
        return self.buf[self.off:self.off + self.n].cpu()

    def get(self, what):
        """the n elements on the CPU: each finite, every other element of the allocation still NaN"""
        torch.cuda.synchronize()
        data = self.buf.cpu()
        inside = data[self.off:self.off + self.n]
        assert bool(torch.isfinite(inside).all()), f"{what}: unwritten or non-finite elements in range"
        assert int(torch.isnan(data).sum()) == data.numel() - self.n, f"{what}: wrote outside its range"
        return inside.clone()

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.buf).all())
