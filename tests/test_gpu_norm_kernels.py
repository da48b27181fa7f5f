"""Kernel-level parity of the batch-norm forward path (csrc/bn_se_kernels.hip: slab reduce, finalize, BN +
activation (+ NoiseInjection) apply in its three host paths, the batched apply with plane sums, the SE gate
from those sums) and of the two caller streams (csrc/caller_kernels.hip: ffc_noise_inject,
ffc_quantize_u8) -- each called through the C ABI against a CPU reference of the same operation
(tests/norm_refs.py, itself checked in test_norm_refs_cpu.py), at the shapes where the host code or a
kernel's loop changes path.  tests/test_gpu_bn_reduce.py and test_gpu_se_sums.py stay as they are; this
file adds to them.

Every output is prefilled with NaN (the uint8 output with a sentinel byte) and must come back fully
written; after a rejection it must come back untouched.  Device copies stay alive until the test ends.
Only the three apply entry points, whose host code tests alignment, are ever handed a misaligned pointer.

Bounds (u = 2^-24, one fp32 rounding; every elementwise bound carries a factor 1 + 2^-20 for the second-order
terms and one fp32 denormal, 2^-149, absolutely)
  reduce      raw moments against the fp64 merge: rtol 1e-12 / atol 1e-8 (test_gpu_bn_reduce.py)
  finalize    scale, running_mean rtol 1e-6 / atol 1e-7; shift, running_var rtol 1e-5 / atol 1e-6
              (test_gpu_bn_reduce.py); the three entry points bit-identical to each other.
              The channel constant at mean 100 (variance 0, scale = gamma / sqrt(eps)): |shift - ref| <=
              k u (|beta| + |mean scale|), k = 7, the fp32 roundings of finalize_channel on the way to shift:
              (float)mu, (float)v, var + eps, sqrtf, 1 / sqrt, gamma * inv, and the final fmaf.
  apply       act 0 / 1: one correctly rounded fma (ReLU is exact): |got - ref| <= u |ref|;
              act 2: the fma and one multiply: 2u |ref|; Tanh / Sigmoid / GELU: normwise 1e-5.
  noise       y = fma(noise_w, noise, a), a the activation: |got - ref| <= e_a |a| + u |ref|, e_a the apply
              bound of a (u, 2u); Tanh / Sigmoid / GELU normwise 1e-5.  ffc_noise_inject: one fma, u |ref|.
  plane sums  against the fp64 chunk sums of the y the kernel returned: d u sum|y| over the chunk, d = 19, the
              depth of additions in bn_act_plane_batch_kernel: 2 (the float4's pair sums (x + y) + (z + w)),
              4 (ts += per float4 of the thread; the first adds to 0 exactly), 5 (half_wave_sum: four DPP
              steps and one permlane swap), 8 (the eight half sums in order; the first adds to 0 exactly):
              17 of the 19 round, so (1 + u)^17 - 1 < 19 u.  Against the reference's own sums: 1e-5 sum|y|.
  gates       normwise 1e-5 (TOL of test_gpu_spectral_kernels.py)
  quantize    torch.equal with the fp32 reference: the operation is exact

Observed maxima per family on the first MI355X run (177 tests in 3.0 s), as the largest |got - ref| / limit
of the family's bound unless a normwise error is named.  The single-fma families sit just under 1 by
construction: a correctly rounded result is off by up to half an ulp, which is u |ref| at a power of two.
  reduce      3.5e-04
  finalize    scale 0.12  shift 0.029  shift of the mean-100 channel 0.037  running_mean 0.12  running_var 0.0097;
              the three entry points bit-identical in every case
  apply       plane 0.94  vector 0.94  scalar 0.97 (act 0 / 1 / 2); Tanh / Sigmoid / GELU normwise <= 8.6e-08
              (with and without noise)
  noise       0.97      batch items 0.99 (non-plane items 0.81)
  plane sums  against the returned y 0.096; against the reference's sums 0.011
  gate sums   normwise 1.6e-07; chained: 5.6e-08 against fp64 and against ffc_se_gate
  inject      0.9996    quantize: 0 bytes differ at n = 4, 1004 and 8388612
Against the library of the parent commit only test_apply_batch_validates_every_item_before_the_first_launch
failed (all four cases: the valid first item had been written).

Case -> branch it is there for
  reduce      rows 1, 63 (one partly filled wave), 255 / 256 / 257 (RED_THREADS), 1023 (the 4 * RED_THREADS
              unrolled loop: r + 768 < nrows for threads 0..254, the tail loop for thread 255); 1024 (first
              two-level slab, S = 16 splits of 64 rows: exactly one unrolled round r + 48 < r_hi per lane and
              no tail), 1025 / 1087 (S = 16, splits of 64..68 rows: unrolled round + tail), 1088 (S = 17);
              C 1 / 15 / 17 / 33: a partly filled 16-channel group (cc = C - 1 clamp), 16: none;
              rows with n = 0 in a small and a two-level slab.  ffc_bn_reduce_ws_doubles > 0 from 1024 rows.
  finalize    ffc_bn_reduce_finalize (37-row slabs: bn_reduce_finalize_kernel; 1030 rows: bn_merge_kernel),
              ffc_bn_finalize from the moments that call wrote, ffc_bn_reduce_finalize_batch of one item:
              momentum 0.1 (bump inside the kernel), None at num_batches_tracked 0 / 3 (every block reads it,
              bn_bump_kernel after), update_running 0 with NULL running pointers and with given ones (left
              alone), gamma / beta / both NULL, count_mult 4, one row of n = 1 (nfull <= 1: biased running
              variance), the mean-100 channel, C 1 / 256 / 257 / 600 (bn_finalize_kernel: 1 / 1 / 2 / 3
              blocks, one bump); eval from the running statistics with moments NULL.
              batch: four packed items of different C (one C = 1: block-index prefix sums), small-large-small
              (a two-level item between packed ones), all large (the a.n == 0 return), n = 0 / 5 rejected.
  apply       plane (B, C, HW): (2, 3, 256) HW4 = 64 < 256 threads; (1, 2, 4096) one full chunk; (2, 2, 4100)
              two chunks, the second of one float4; (1, 5, 260).  vector: (4, 3, 9) channels change inside a
              float4; (3, 5, 36); (2, 2, 252) HW % 4 == 0 but < 256; (8, 300, 225): 528 blocks, and
              (32, 300, 225): total4 = 540000 > 2048 * 256, the grid-stride loop wraps.  scalar: (3, 5, 9)
              odd total; (1, 1, 1); (7, 301, 255) odd and past the grid cap; (2, 3, 256) with x and y one float
              off 16-byte alignment.  Every case in place and out of place (LeakyReLU); every activation on
              (2, 3, 256), (3, 5, 36), (3, 5, 9).
  noise       (3, 2, 4) one float4 per plane; (2, 5, 256); (2, 3, 4100) two chunks; B > 1 with a draw per
              sample; HW = 6, a misaligned noise, NULL noise_w rejected.
  batch       one call: plane + noise + plane_sum (in place), plane + plane_sum at HW 4100 (two chunks), plane
              without plane_sum, HW 36 (single-form path inside the batch); a batch of non-plane items only;
              a valid HW 36 item followed by an invalid one (plane_sum at HW 36, noise without noise_w, x NULL,
              noise at HW 6): rejected before anything is written.
  gate sums   HW 256 / 4100 / 16384 -> chunks 1 / 2 / 4; C 5 / 300 (more channels than threads); hidden 0 / 1 /
              300; chained ffc_bn_act_apply_batch -> ffc_se_gate_sums against ffc_se_gate and fp64; a wrong
              chunk count and NULL weights rejected.
  inject      (1, 1, 4) one float4; (3, 5, 36); (2, 33, 131072): n4 = 2162688 > 8192 * 256 (the loop wraps) and
              the noise of the second sample; HW = 6 and each NULL pointer rejected.
  quantize    n 4; the boundary set of norm_refs.quantize_inputs padded to a multiple of 4; 8192 * 256 * 4 + 4
              (past the grid cap); 64 sentinel bytes behind the output survive; n 6 / 0 rejected.
"""
import pytest
import torch

import norm_refs as nr
import spectral_refs as sr
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 1e-5
NAN = float("nan")
U = 2.0 ** -24
DENORMAL = 2.0 ** -149
SECOND_ORDER = 1.0 + 2.0 ** -20
K_SHIFT = 7           # fp32 roundings of finalize_channel on the way to shift (docstring)
D_SUM = 19            # depth of additions of one chunk sum (docstring)
MOM = float(torch.tensor(0.1, dtype=torch.float32))
EPS = nr.BN_EPS
SLOPE = nr.SLOPE32
SENTINEL = 0xA5


def _L():
    import fastfourierconvolution_amd  # noqa: F401  (registers torch.ops.ffc.*)
    from fastfourierconvolution_amd import _runtime as rt
    return rt.lib()


def _items():
    from fastfourierconvolution_amd import _lib
    return _lib.BnRfItem, _lib.BnApplyItem


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(status, what):
    from fastfourierconvolution_amd._lib import check
    check(status, what)


_LIVE = []


def _keep(t):
    _LIVE.append(t)
    return t


def _nan(shape, dtype=torch.float32):
    return _keep(torch.full(shape, NAN, device=DEV, dtype=dtype))


def _dev(t):
    """a device copy that stays alive until the test ends (the ABI takes raw pointers: a temporary freed
    before the launch could be handed to the next allocation)"""
    return None if t is None else _keep(t.to(DEV).contiguous())


def _i64(v):
    return _keep(torch.tensor([v], device=DEV, dtype=torch.int64))


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is launched from this file
        pytest.exit(f"HIP error after a kernel of this file: {e}", returncode=3)
    _LIVE.clear()


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in ts if t is not None)


def _err(family, what, out, ref):
    """print, then return, the normwise error of a returned tensor (which must hold no NaN)"""
    assert not torch.isnan(out).any(), f"{what}: unwritten (NaN) elements"
    e = normwise_err(out.detach().cpu().double().reshape(ref.shape), ref)
    print(f"OBS {family} {what} {e:.3e}")
    return e


def _within(family, what, got, ref, lim):
    """elementwise |got - ref| <= lim; prints the largest |got - ref| / lim"""
    assert not torch.isnan(got).any(), f"{what}: unwritten (NaN) elements"
    diff = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    worst = float((diff / lim).max())
    print(f"OBS {family} {what} max diff / limit {worst:.3e}")
    assert (diff <= lim).all(), (what, worst)


def _close(family, what, got, ref, rtol, atol):
    """torch.testing.assert_close after printing the largest |got - ref| / (atol + rtol |ref|)"""
    got = got.detach().cpu().double().reshape(ref.shape)
    assert not torch.isnan(got).any(), f"{what}: unwritten (NaN) elements"
    print(f"OBS {family} {what} max diff / limit {float(((got - ref).abs() / (atol + rtol * ref.abs())).max()):.3e}")
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


# --------------------------------------------------------------------------- reduce
ROWS = (1, 63, 255, 256, 257, 1023, 1024, 1025, 1087, 1088)
CHANNELS = (1, 15, 16, 17, 33)


def _reduce_both(slab, nrows, C, what):
    """ffc_bn_reduce and the moments ffc_bn_reduce_finalize writes, each against the fp64 merge"""
    L = _L()
    ref = torch.stack(nr.slab_moments(slab), dim=-1)
    ws = L.ffc_bn_reduce_ws_doubles(nrows, C)
    assert (ws > 0) == (nrows >= 1024)
    sd = _dev(slab)
    buf = _nan((3 * C + ws,), torch.float64)
    _ok(L.ffc_bn_reduce(_ptr(sd), nrows, C, _ptr(buf), _stream()), "ffc_bn_reduce")
    buf2, scale, shift = _nan((3 * C + ws,), torch.float64), _nan((C,)), _nan((C,))
    _ok(L.ffc_bn_reduce_finalize(_ptr(sd), nrows, C, _ptr(buf2), None, None, None, None, None, 0, MOM, EPS, 1.0,
                                 _ptr(scale), _ptr(shift), _stream()), "ffc_bn_reduce_finalize")
    torch.cuda.synchronize()
    _close("reduce", what + " ffc_bn_reduce", buf[:3 * C].view(C, 3), ref, 1e-12, 1e-8)
    _close("reduce", what + " ffc_bn_reduce_finalize", buf2[:3 * C].view(C, 3), ref, 1e-12, 1e-8)
    assert not torch.isnan(scale).any() and not torch.isnan(shift).any()


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("nrows", ROWS)
def test_reduce_matches_fp64_merge(nrows, C):
    _reduce_both(nr.slab_inputs(nrows, C), nrows, C, f"rows={nrows} C={C}")


@pytest.mark.parametrize("nrows", [300, 1100])
def test_reduce_ignores_rows_with_n_zero(nrows):
    zero = (0, 5, 64, 255, nrows - 1)
    slab = nr.slab_inputs(nrows, 17, zero_rows=zero)
    assert torch.equal(slab[list(zero)], torch.zeros(len(zero), 17, 4))
    _reduce_both(slab, nrows, 17, f"rows={nrows} C=17 zero rows")


# --------------------------------------------------------------------------- finalize
def _mean100(slab):
    """channel 0 constant at 100 in every row: M2 = 0, so the merged variance is exactly 0"""
    slab = slab.clone()
    slab[:, 0, 1] = 100.0
    slab[:, 0, 2] = 0.0
    return slab


def _one_sample(C):
    gen = torch.Generator().manual_seed(77)
    slab = torch.zeros(1, C, 4)
    slab[0, :, 0] = 1.0
    slab[0, :, 1] = torch.randn(C, generator=gen)
    return slab


# name: nrows, C, then keywords (defaults: momentum MOM, nbt 3, update, gamma, beta, running given, count_mult 1)
_FIN = {
    "train": (37, 33, {}),
    "train-large": (1030, 33, {}),
    "cumulative-nbt0": (37, 17, dict(momentum=None, nbt=0)),
    "cumulative-nbt3": (37, 17, dict(momentum=None)),
    "cumulative-nbt3-large": (1030, 17, dict(momentum=None)),
    "no-update-null-running": (37, 17, dict(update=False, running=False)),
    "no-update-null-running-large": (1030, 17, dict(update=False, running=False)),
    "no-update-given-running": (37, 17, dict(update=False)),
    "gamma-null": (37, 17, dict(gamma=False)),
    "beta-null": (37, 17, dict(beta=False)),
    "both-null": (37, 17, dict(gamma=False, beta=False)),
    "both-null-large": (1030, 17, dict(gamma=False, beta=False)),
    "count-mult-4": (37, 17, dict(count_mult=4.0)),
    "one-sample": (1, 17, dict(slab="one")),
    "one-sample-cumulative": (1, 5, dict(slab="one", momentum=None, nbt=0)),
    "mean-100": (37, 5, dict(slab="mean100")),
    "mean-100-large": (1030, 5, dict(slab="mean100")),
    "C1": (37, 1, {}),
    "C256": (5, 256, {}),
    "C257": (5, 257, {}),
    "C257-cumulative": (5, 257, dict(momentum=None)),
    "C600": (5, 600, {}),
    "C600-cumulative": (5, 600, dict(momentum=None)),
    "C600-large": (1030, 600, {}),
}


def _fin_inputs(nrows, C, kw, seed=0):
    kind = kw.get("slab")
    slab = _one_sample(C) if kind == "one" else nr.slab_inputs(nrows, C, seed)
    if kind == "mean100":
        slab = _mean100(slab)
    gamma, beta, rm, rv = nr.bn_params(C, seed)
    if not kw.get("gamma", True):
        gamma = None
    if not kw.get("beta", True):
        beta = None
    if not kw.get("running", True):
        rm = rv = None
    return dict(slab=slab, nrows=nrows, C=C, gamma=gamma, beta=beta, rm=rm, rv=rv, nbt=kw.get("nbt", 3),
                update=kw.get("update", True), momentum=kw.get("momentum", MOM), count_mult=kw.get("count_mult", 1.0),
                mean100=kind == "mean100")


def _fin_ref(d):
    return nr.finalize(*nr.slab_moments(d["slab"]), d["gamma"], d["beta"], EPS, d["momentum"], d["count_mult"], d["rm"],
                       d["rv"], d["nbt"], True, d["update"])


class _Fin:
    """device operands of one finalize call on the case d: its own running buffers, NaN outputs"""

    def __init__(self, d, slab=None):
        self.d = d
        C, nrows = d["C"], d["nrows"]
        self.slab = _dev(d["slab"]) if slab is None else slab
        self.gamma, self.beta = _dev(d["gamma"]), _dev(d["beta"])
        self.rm, self.rv = _dev(d["rm"]), _dev(d["rv"])
        self.nbt = _i64(d["nbt"]) if d["rm"] is not None else None
        self.buf = _nan((3 * C + _L().ffc_bn_reduce_ws_doubles(nrows, C),), torch.float64)
        self.scale, self.shift = _nan((C,)), _nan((C,))
        self.mom = -1.0 if d["momentum"] is None else d["momentum"]

    def tail(self):
        d = self.d
        return (int(d["update"]), self.mom, EPS, d["count_mult"], _ptr(self.scale), _ptr(self.shift))

    def running(self):
        return (_ptr(self.gamma), _ptr(self.beta), _ptr(self.rm), _ptr(self.rv), _ptr(self.nbt))

    def reduce_finalize(self):
        d = self.d
        return _L().ffc_bn_reduce_finalize(_ptr(self.slab), d["nrows"], d["C"], _ptr(self.buf), *self.running(),
                                           *self.tail(), _stream())

    def finalize(self, moments):
        return _L().ffc_bn_finalize(_ptr(moments), self.d["C"], *self.running(), 1, *self.tail(), _stream())

    def item(self):
        d = self.d
        return _items()[0](_ptr(self.slab), d["nrows"], d["C"], _ptr(self.buf), *self.running(), *self.tail())

    def outputs(self):
        return [t for t in (self.scale, self.shift, self.rm, self.rv, self.nbt) if t is not None]


def _fin_check(form, what, f, ref):
    """one call's outputs against norm_refs.finalize at the project's tolerances"""
    d = f.d
    sc, sh, rm, rv, nbt = ref
    fam = "finalize"
    _close(fam, f"{what} {form} scale", f.scale, sc, 1e-6, 1e-7)
    if d["mean100"]:
        # channel 0: the product mean * scale is of order 100 / sqrt(eps); K_SHIFT roundings lead to shift
        b0 = 0.0 if d["beta"] is None else abs(float(d["beta"][0]))
        mu = float(nr.slab_moments(d["slab"])[1][0] / nr.slab_moments(d["slab"])[0][0])
        assert mu == 100.0 and float(sc[0].abs()) > 100.0
        lim = K_SHIFT * U * (b0 + abs(mu * float(sc[0])))
        _within(fam, f"{what} {form} shift[mean 100]", f.shift[:1], sh[:1], torch.tensor([lim], dtype=torch.float64))
        _close(fam, f"{what} {form} shift", f.shift[1:], sh[1:], 1e-5, 1e-6)
    else:
        _close(fam, f"{what} {form} shift", f.shift, sh, 1e-5, 1e-6)
    if d["rm"] is None:
        return
    if d["update"]:
        _close(fam, f"{what} {form} running_mean", f.rm, rm, 1e-6, 1e-7)
        _close(fam, f"{what} {form} running_var", f.rv, rv, 1e-5, 1e-6)
        assert torch.isfinite(f.rv).all()
        assert int(f.nbt) == d["nbt"] + 1 == nbt, (what, form, int(f.nbt))      # one bump, however many blocks
    else:
        assert torch.equal(f.rm.cpu(), d["rm"]) and torch.equal(f.rv.cpu(), d["rv"]), (what, form)
        assert int(f.nbt) == d["nbt"] == nbt


@pytest.mark.parametrize("name", list(_FIN))
def test_finalize_forms_match_fp64_and_each_other(name):
    """ffc_bn_reduce_finalize, ffc_bn_finalize from the moments it wrote and ffc_bn_reduce_finalize_batch of one
    item: each against fp64, and bit-identical to each other (the explicit fmaf of finalize_channel)"""
    nrows, C, kw = _FIN[name]
    d = _fin_inputs(nrows, C, kw)
    assert (_L().ffc_bn_reduce_ws_doubles(nrows, C) > 0) == name.endswith("-large")
    ref = _fin_ref(d)
    rf = _Fin(d)
    _ok(rf.reduce_finalize(), "ffc_bn_reduce_finalize")
    torch.cuda.synchronize()
    assert not torch.isnan(rf.buf[:3 * C]).any()
    fin = _Fin(d, rf.slab)
    _ok(fin.finalize(rf.buf), "ffc_bn_finalize")
    bat = _Fin(d, rf.slab)
    arr = (_items()[0] * 1)(bat.item())
    _ok(_L().ffc_bn_reduce_finalize_batch(arr, 1, _stream()), "ffc_bn_reduce_finalize_batch")
    torch.cuda.synchronize()
    for form, f in (("reduce_finalize", rf), ("finalize", fin), ("batch", bat)):
        _fin_check(form, name, f, ref)
    for other in (fin, bat):
        for a, b in zip(rf.outputs(), other.outputs()):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("C", [5, 600])
@pytest.mark.parametrize("update", [0, 1])
@pytest.mark.parametrize("affine", [True, False])
def test_finalize_eval_uses_running_statistics(affine, update, C):
    """use_batch_stats = 0 with moments NULL: scale / shift from the running statistics, which stay as they were
    (as does num_batches_tracked) whatever update_running says"""
    gamma, beta, rm, rv = nr.bn_params(C)
    if not affine:
        gamma = beta = None
    sc, sh, _, _, _ = nr.finalize(None, None, None, gamma, beta, EPS, MOM, 1.0, rm, rv, 3, use_batch_stats=False)
    d_rm, d_rv, d_nbt = _dev(rm), _dev(rv), _i64(3)
    for mom in (MOM, -1.0):
        scale, shift = _nan((C,)), _nan((C,))
        _ok(_L().ffc_bn_finalize(None, C, _ptr(_dev(gamma)), _ptr(_dev(beta)), _ptr(d_rm), _ptr(d_rv), _ptr(d_nbt), 0,
                                 update, mom, EPS, 1.0, _ptr(scale), _ptr(shift), _stream()), "ffc_bn_finalize(eval)")
        torch.cuda.synchronize()
        what = f"eval C={C} affine={int(affine)} update={update} momentum={mom:.1f}"
        _close("finalize", what + " scale", scale, sc, 1e-6, 1e-7)
        _close("finalize", what + " shift", shift, sh, 1e-5, 1e-6)
        assert torch.equal(d_rm.cpu(), rm) and torch.equal(d_rv.cpu(), rv) and int(d_nbt) == 3


def test_finalize_rejections_write_nothing():
    L = _L()
    C = 5
    d = _fin_inputs(37, C, {})
    f = _Fin(d)
    mo = _keep(torch.ones(3 * C, device=DEV, dtype=torch.float64))
    run = f.running()
    calls = {
        "batch stats without moments": lambda: L.ffc_bn_finalize(None, C, *run, 1, *f.tail(), _stream()),
        "eval without running statistics": lambda: L.ffc_bn_finalize(_ptr(mo), C, run[0], run[1], None, None, run[4],
                                                                     0, 0, f.mom, EPS, 1.0, _ptr(f.scale), _ptr(f.shift),
                                                                     _stream()),
        "update without num_batches_tracked": lambda: L.ffc_bn_finalize(_ptr(mo), C, *run[:4], None, 1, *f.tail(),
                                                                        _stream()),
        "reduce_finalize: update without num_batches_tracked": lambda: L.ffc_bn_reduce_finalize(
            _ptr(f.slab), 37, C, _ptr(f.buf), *run[:4], None, *f.tail(), _stream()),
    }
    for what, call in calls.items():
        assert call() != 0, what
        assert L.ffc_last_error(), what
        assert _untouched(f.scale, f.shift, f.buf), what
        assert torch.equal(f.rm.cpu(), d["rm"]) and torch.equal(f.rv.cpu(), d["rv"]) and int(f.nbt) == 3, what
    Item = _items()[0]
    ok_item = f.item()
    bad = f.item()
    bad.num_batches_tracked = None
    for what, arr, n in (("n = 0", (Item * 1)(ok_item), 0), ("n = 5", (Item * 5)(*[ok_item] * 5), 5),
                         ("second item: update without num_batches_tracked", (Item * 2)(ok_item, bad), 2)):
        assert L.ffc_bn_reduce_finalize_batch(arr, n, _stream()) != 0, what
        assert _untouched(f.scale, f.shift, f.buf), what
        assert torch.equal(f.rm.cpu(), d["rm"]) and torch.equal(f.rv.cpu(), d["rv"]) and int(f.nbt) == 3, what


_BATCHES = {
    "four-small": [(37, 5, {}), (5, 1, dict(momentum=None)), (300, 33, dict(gamma=False)), (1, 17, dict(slab="one"))],
    "small-large-small": [(37, 5, {}), (1030, 17, dict(momentum=None)), (5, 33, dict(update=False, running=False))],
    "all-large": [(1024, 16, {}), (1030, 17, dict(momentum=None, nbt=0))],
}


@pytest.mark.parametrize("name", list(_BATCHES))
def test_finalize_batch_layouts(name):
    """every item of a batch against fp64 and bit-identical to its single ffc_bn_reduce_finalize call"""
    L = _L()
    specs = _BATCHES[name]
    large = [L.ffc_bn_reduce_ws_doubles(n, C) > 0 for n, C, _ in specs]
    assert large == {"four-small": [False] * 4, "small-large-small": [False, True, False],
                     "all-large": [True, True]}[name]
    ds = [_fin_inputs(n, C, kw, seed=i + 1) for i, (n, C, kw) in enumerate(specs)]
    single = [_Fin(d) for d in ds]
    for f in single:
        _ok(f.reduce_finalize(), "ffc_bn_reduce_finalize")
    batch = [_Fin(d, s.slab) for d, s in zip(ds, single)]
    arr = (_items()[0] * len(batch))(*[f.item() for f in batch])
    _ok(L.ffc_bn_reduce_finalize_batch(arr, len(batch), _stream()), "ffc_bn_reduce_finalize_batch")
    torch.cuda.synchronize()
    for i, (d, s, b) in enumerate(zip(ds, single, batch)):
        _fin_check("batch", f"{name}[{i}]", b, _fin_ref(d))
        for u, v in zip(s.outputs(), b.outputs()):
            assert torch.equal(u, v), (name, i)


# --------------------------------------------------------------------------- apply
GRID_CAP = 2048 * 256      # ffc_bn_act_apply: at most 2048 blocks of 256 threads


def _apply_path(B, C, HW, x_addr, y_addr):
    """the dispatch of ffc_bn_act_apply, restated"""
    total = B * C * HW
    vec = total % 4 == 0 and (x_addr | y_addr) % 16 == 0
    if vec and HW % 4 == 0 and HW >= 256:
        return "plane"
    return "vector" if vec else "scalar"


# (B, C, HW, misaligned, path)
APPLY_CASES = [
    (2, 3, 256, False, "plane"), (1, 2, 4096, False, "plane"), (2, 2, 4100, False, "plane"), (1, 5, 260, False, "plane"),
    (4, 3, 9, False, "vector"), (3, 5, 36, False, "vector"), (2, 2, 252, False, "vector"),
    (8, 300, 225, False, "vector"), (32, 300, 225, False, "vector"),
    (3, 5, 9, False, "scalar"), (1, 1, 1, False, "scalar"), (7, 301, 255, False, "scalar"),
    (2, 3, 256, True, "scalar"),
]
ACT_SHAPES = [(2, 3, 256, "plane"), (3, 5, 36, "vector"), (3, 5, 9, "scalar")]


def test_apply_cases_reach_every_path():
    """the case table run through the restated dispatch (no launch): all three kernels, the wrapping grid-stride
    loop of the vector and the scalar kernel, a chunk boundary of the plane kernel"""
    for B, C, HW, mis, path in APPLY_CASES:
        assert _apply_path(B, C, HW, 4 if mis else 0, 4 if mis else 0) == path, (B, C, HW, mis)
    for B, C, HW, path in ACT_SHAPES:
        assert _apply_path(B, C, HW, 0, 0) == path
    assert {c[4] for c in APPLY_CASES} == {p for *_, p in ACT_SHAPES} == {"plane", "vector", "scalar"}
    assert any(p == "vector" and B * C * HW // 4 > GRID_CAP for B, C, HW, _, p in APPLY_CASES)
    assert any(p == "scalar" and B * C * HW > GRID_CAP and (B * C * HW) % 2 for B, C, HW, _, p in APPLY_CASES)
    assert any(p == "scalar" and mis and _apply_path(B, C, HW, 0, 0) == "plane" for B, C, HW, mis, p in APPLY_CASES)
    assert any(p == "plane" and HW // 4 == 1025 for B, C, HW, _, p in APPLY_CASES)
    assert any(p == "plane" and HW // 4 < 256 for B, C, HW, _, p in APPLY_CASES)
    assert _L().ffc_plane_chunks(4096) == 1 and _L().ffc_plane_chunks(4100) == 2


def _guarded(total, misaligned, fill=NAN):
    """(buffer, view of `total` floats): four floats of guard in front (five when misaligned: the view then
    starts one float off 16-byte alignment) and eight behind"""
    off = 5 if misaligned else 4
    buf = _keep(torch.full((total + off + 8,), fill, device=DEV))
    view = buf[off:off + total]
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    return buf, view, off


def _guards_intact(buf, off, total):
    return bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + total:]).all())


def _act_limit(ref, act):
    """elementwise bound of act(fma(x, scale, shift)) for act 0 / 1 / 2 (docstring)"""
    return (1 if act < 2 else 2) * U * ref.abs() * SECOND_ORDER + DENORMAL


def _check_y(family, what, y, ref, act, a=None):
    """y against fp64: elementwise for act 0 / 1 / 2 (a: the activation's own value where noise was added on
    top), normwise for the transcendental activations"""
    if act > 2:
        assert _err(family, what, y, ref) <= TOL
        return
    lim = _act_limit(ref, act) if a is None else _act_limit(a, act) + U * ref.abs() * SECOND_ORDER
    _within(family, what, y, ref, lim)


def _run_apply(B, C, HW, act, inplace, misaligned, path):
    x, scale, shift = nr.apply_inputs(B, C, HW)
    ref = nr.bn_act_apply(x, scale, shift, act, SLOPE)
    total = x.numel()
    ybuf, y, off = _guarded(total, misaligned)
    if inplace:
        xin = y
    else:
        _, xin, _ = _guarded(total, misaligned, 0.0)
    xin.copy_(x.reshape(-1))
    assert _apply_path(B, C, HW, xin.data_ptr(), y.data_ptr()) == path
    _ok(_L().ffc_bn_act_apply(_ptr(xin), _ptr(y), B, C, HW, _ptr(_dev(scale)), _ptr(_dev(shift)), act, SLOPE, _stream()),
        "ffc_bn_act_apply")
    torch.cuda.synchronize()
    assert _guards_intact(ybuf, off, total), "wrote outside y"
    _check_y(f"apply_{path}", f"({B},{C},{HW}) act={act} inplace={int(inplace)} misaligned={int(misaligned)}", y, ref, act)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("B,C,HW,misaligned,path", APPLY_CASES)
def test_apply_matches_fp64(B, C, HW, misaligned, path, inplace):
    _run_apply(B, C, HW, 2, inplace, misaligned, path)


@pytest.mark.parametrize("act", range(6))
@pytest.mark.parametrize("B,C,HW,path", ACT_SHAPES)
def test_apply_every_activation(B, C, HW, path, act):
    _run_apply(B, C, HW, act, False, False, path)


# --------------------------------------------------------------------------- apply + noise
@pytest.mark.parametrize("act", [0, 2, 5])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("B,C,HW", [(3, 2, 4), (2, 5, 256), (2, 3, 4100)])
def test_noise_apply_matches_fp64(B, C, HW, inplace, act):
    x, scale, shift, nw, noise = nr.apply_inputs(B, C, HW, with_noise=True)
    assert B > 1 and not torch.equal(noise[0], noise[1])
    a = nr.bn_act_apply(x, scale, shift, act, SLOPE)
    ref = nr.bn_act_apply(x, scale, shift, act, SLOPE, nw, noise)
    ybuf, y, off = _guarded(x.numel(), False)
    xin = y if inplace else _dev(x).reshape(-1)
    if inplace:
        y.copy_(x.reshape(-1))
    _ok(_L().ffc_bn_act_noise_apply(_ptr(xin), _ptr(y), B, C, HW, _ptr(_dev(scale)), _ptr(_dev(shift)), act, SLOPE,
                                    _ptr(_dev(nw)), _ptr(_dev(noise)), _stream()), "ffc_bn_act_noise_apply")
    torch.cuda.synchronize()
    assert _guards_intact(ybuf, off, x.numel()), "wrote outside y"
    _check_y("noise", f"({B},{C},{HW}) act={act} inplace={int(inplace)}", y, ref, act, a)


def test_noise_apply_rejections_write_nothing():
    L = _L()
    B, C, HW = 2, 3, 8
    x, scale, shift, nw, noise = nr.apply_inputs(B, C, HW, with_noise=True)
    xd, sc, sh, nwd, nz = _dev(x), _dev(scale), _dev(shift), _dev(nw), _dev(noise)
    _, nz_off, _ = _guarded(B * HW, True, 0.0)
    y = _nan((B, C, HW))
    x6, y6 = _dev(torch.zeros(B, C, 6)), _nan((B, C, 6))
    calls = {
        "HW = 6": lambda: L.ffc_bn_act_noise_apply(_ptr(x6), _ptr(y6), B, C, 6, _ptr(sc), _ptr(sh), 0, SLOPE, _ptr(nwd),
                                                   _ptr(nz), _stream()),
        "misaligned noise": lambda: L.ffc_bn_act_noise_apply(_ptr(xd), _ptr(y), B, C, HW, _ptr(sc), _ptr(sh), 0, SLOPE,
                                                             _ptr(nwd), _ptr(nz_off), _stream()),
        "NULL noise_w": lambda: L.ffc_bn_act_noise_apply(_ptr(xd), _ptr(y), B, C, HW, _ptr(sc), _ptr(sh), 0, SLOPE, None,
                                                         _ptr(nz), _stream()),
    }
    for what, call in calls.items():
        assert call() != 0, what
        assert _untouched(y, y6), what


# --------------------------------------------------------------------------- batched apply, plane sums
class _ApplyOp:
    """device operands of one item of ffc_bn_act_apply_batch and its fp64 reference"""

    def __init__(self, B, C, HW, act, noise=False, psum=None, inplace=False, seed=0):
        self.B, self.C, self.HW, self.act = B, C, HW, act
        ins = nr.apply_inputs(B, C, HW, seed, with_noise=True)
        self.x, self.scale, self.shift = ins[:3]
        self.nw, self.noise = ins[3:] if noise else (None, None)
        self.a = nr.bn_act_apply(self.x, self.scale, self.shift, act, SLOPE)
        self.ref = nr.bn_act_apply(self.x, self.scale, self.shift, act, SLOPE, self.nw, self.noise)
        self.y = _nan((B, C, HW))
        self.xd = self.y if inplace else _dev(self.x)
        self.x_inplace = self.x if inplace else None
        self.dsc, self.dsh, self.dnw, self.dnz = _dev(self.scale), _dev(self.shift), _dev(self.nw), _dev(self.noise)
        self.psum = psum
        self.chunks = _L().ffc_plane_chunks(HW)

    def item(self, **over):
        if self.x_inplace is not None:
            self.y.copy_(self.x_inplace)
        f = dict(x=_ptr(self.xd), y=_ptr(self.y), B=self.B, C=self.C, HW=self.HW, scale=_ptr(self.dsc),
                 shift=_ptr(self.dsh), act=self.act, act_param=SLOPE, noise_w=_ptr(self.dnw), noise=_ptr(self.dnz),
                 plane_sum=_ptr(self.psum))
        f.update(over)
        return _items()[1](**f)

    def check(self, family, what):
        what = f"{what} ({self.B},{self.C},{self.HW}) act={self.act}"
        _check_y(family, what, self.y, self.ref, self.act, self.a if self.noise is not None else None)
        if self.psum is None:
            return
        got = self.psum.reshape(self.B, self.C, self.chunks)
        own = self.y.cpu().double()
        _within("plane_sum", what + " against the returned y", got, nr.plane_chunk_sums(own),
                D_SUM * U * nr.plane_chunk_sums(own.abs()) + DENORMAL)
        _within("plane_sum_ref", what + " against the reference's sums", got, nr.plane_chunk_sums(self.ref),
                TOL * nr.plane_chunk_sums(self.ref.abs()))


def _launch_batch(ops):
    arr = (_items()[1] * len(ops))(*[op.item() for op in ops])
    return _L().ffc_bn_act_apply_batch(arr, len(ops), _stream())


def test_apply_batch_and_plane_sums_match_fp64():
    L = _L()
    shapes = [(2, 3, 1024), (2, 2, 4100), (1, 5, 260), (3, 5, 36)]
    assert [_apply_path(*s, 0, 0) for s in shapes] == ["plane"] * 3 + ["vector"]
    n0, n1, n2 = (B * C * L.ffc_plane_chunks(HW) for B, C, HW in shapes[:3])
    assert (n0, n1, n2) == (6, 8, 5)
    sums = _nan((n0 + n2 + n1,))           # [item 0 | what item 2 would write, were it given one | item 1]
    ops = [_ApplyOp(*shapes[0], act=2, noise=True, psum=sums[:n0], inplace=True, seed=1),
           _ApplyOp(*shapes[1], act=1, psum=sums[n0 + n2:], seed=2),
           _ApplyOp(*shapes[2], act=5, seed=3),
           _ApplyOp(*shapes[3], act=2, seed=4)]
    _ok(_launch_batch(ops), "ffc_bn_act_apply_batch")
    torch.cuda.synchronize()
    for i, op in enumerate(ops):
        op.check("batch", f"item {i}")
    assert torch.isnan(sums[n0:n0 + n2]).all(), "the item without plane_sum wrote sums"


def test_apply_batch_of_non_plane_items_only():
    ops = [_ApplyOp(3, 5, 36, act=2, seed=5), _ApplyOp(3, 5, 9, act=1, inplace=True, seed=6),
           _ApplyOp(3, 2, 8, act=0, noise=True, seed=7)]
    assert [_apply_path(o.B, o.C, o.HW, 0, 0) for o in ops] == ["vector", "scalar", "vector"]
    _ok(_launch_batch(ops), "ffc_bn_act_apply_batch")
    torch.cuda.synchronize()
    for i, op in enumerate(ops):
        op.check("batch_nonplane", f"item {i}")


@pytest.mark.parametrize("bad", ["plane_sum at HW 36", "noise without noise_w", "x NULL", "noise at HW 6"])
def test_apply_batch_validates_every_item_before_the_first_launch(bad):
    """item 0 is a valid out-of-place HW = 36 tensor (a single-form path, launched from the item loop), item 1
    is invalid: the call is rejected and no output of either item is written"""
    psum = _nan((3 * 5,))
    first = _ApplyOp(3, 5, 36, act=2, seed=8)
    if bad == "plane_sum at HW 36":
        second = _ApplyOp(3, 5, 36, act=1, psum=psum, seed=9)
        over = {}
    elif bad == "noise without noise_w":
        second = _ApplyOp(2, 3, 1024, act=1, noise=True, psum=psum[:6], seed=9)
        over = dict(noise_w=None)
    elif bad == "x NULL":
        second = _ApplyOp(2, 3, 1024, act=1, psum=psum[:6], seed=9)
        over = dict(x=None)
    else:
        second = _ApplyOp(3, 5, 6, act=1, noise=True, seed=9)
        over = {}
    arr = (_items()[1] * 2)(first.item(), second.item(**over))
    rc = _L().ffc_bn_act_apply_batch(arr, 2, _stream())
    assert rc != 0 and _L().ffc_last_error()
    assert _untouched(second.y, psum), "the invalid item was written"
    assert _untouched(first.y), "the valid item before the invalid one was written: a half-applied batch"


# --------------------------------------------------------------------------- SE gate from plane sums
def _gate_sums(sums, B, C, HW, w1, w2, hidden, chunks=None):
    gate = _nan((B, C))
    rc = _L().ffc_se_gate_sums(_ptr(sums), _L().ffc_plane_chunks(HW) if chunks is None else chunks, B, C, HW, _ptr(w1),
                               _ptr(w2), hidden, _ptr(gate), _stream())
    torch.cuda.synchronize()
    return rc, gate


@pytest.mark.parametrize("B,C,H,W,hidden", [(2, 5, 16, 16, 1), (2, 5, 50, 82, 300), (2, 5, 128, 128, 0),
                                            (2, 300, 16, 16, 300), (2, 300, 50, 82, 0), (1, 300, 128, 128, 1),
                                            (3, 5, 16, 16, 0), (2, 300, 16, 16, 1), (1, 5, 128, 128, 300)])
def test_se_gate_sums_matches_fp64(B, C, H, W, hidden):
    HW = H * W
    chunks = _L().ffc_plane_chunks(HW)
    assert chunks == {256: 1, 4100: 2, 16384: 4}[HW]
    gen = torch.Generator().manual_seed(5000 + C + HW + hidden)
    x = torch.randn(B, C, H, W, generator=gen) + 0.5
    w1, w2 = sr.se_weights(x, 0, hidden, gen)
    sums = nr.plane_chunk_sums(x).float()                      # the fp64 chunk sums, rounded once
    assert sums.shape == (B, C, chunks)
    rc, gate = _gate_sums(_dev(sums), B, C, HW, _dev(w1), _dev(w2), hidden)
    _ok(rc, "ffc_se_gate_sums")
    assert _err("gate_sums", f"C={C} HW={HW} hidden={hidden}", gate, sr.se_gate(x, 0, w1, w2)) <= TOL


def test_apply_batch_plane_sums_feed_the_se_gate():
    """ffc_bn_act_apply_batch with plane_sum, then ffc_se_gate_sums: against ffc_se_gate on the same y and against
    fp64"""
    L = _L()
    B, C, H, W, hidden = 2, 6, 64, 68, 3
    HW = H * W
    chunks = L.ffc_plane_chunks(HW)
    assert chunks == 2 and W % 4 == 0
    psum = _nan((B * C * chunks,))
    op = _ApplyOp(B, C, HW, act=1, psum=psum, seed=10)
    w1, w2 = sr.se_weights(op.ref.reshape(B, C, H, W), 0, hidden, torch.Generator().manual_seed(6000))
    ref = sr.se_gate(op.ref.reshape(B, C, H, W), 0, w1, w2)
    _ok(_launch_batch([op]), "ffc_bn_act_apply_batch")
    d1, d2 = _dev(w1), _dev(w2)
    rc, gate = _gate_sums(psum, B, C, HW, d1, d2, hidden)
    _ok(rc, "ffc_se_gate_sums")
    direct = _nan((B, C))
    _ok(L.ffc_se_gate(_ptr(op.y), B, C, H, W, 0, _ptr(d1), _ptr(d2), hidden, _ptr(direct), _stream()), "ffc_se_gate")
    torch.cuda.synchronize()
    op.check("chain", "apply")
    errs = [_err("gate_chain", "sums against fp64", gate, ref), _err("gate_chain", "ffc_se_gate against fp64", direct, ref),
            _err("gate_chain", "sums against ffc_se_gate", gate, direct.cpu().double())]
    assert max(errs) <= TOL, errs


def test_se_gate_sums_rejections_write_nothing():
    B, C, HW, hidden = 2, 5, 4100, 2
    sums = _dev(torch.ones(B, C, 2))
    w = _dev(torch.ones(hidden * C))
    for what, kw in (("chunks != ffc_plane_chunks(HW)", dict(w1=w, w2=w, chunks=1)),
                     ("chunks != ffc_plane_chunks(HW)", dict(w1=w, w2=w, chunks=3)),
                     ("NULL w1", dict(w1=None, w2=w)), ("NULL w2", dict(w1=w, w2=None))):
        rc, gate = _gate_sums(sums, B, C, HW, hidden=hidden, **kw)
        assert rc != 0 and _untouched(gate), what


# --------------------------------------------------------------------------- ffc_noise_inject
INJECT_CAP = 8192 * 256    # caller_kernels.hip grid_for: at most 8192 blocks of 256 threads


@pytest.mark.parametrize("B,C,HW", [(1, 1, 4), (3, 5, 36), (2, 33, 131072)])
def test_noise_inject_matches_fp64(B, C, HW):
    assert (B * C * HW // 4 > INJECT_CAP) == (HW == 131072)
    gen = torch.Generator().manual_seed(7000 + HW)
    x = torch.randn(B, C, HW, generator=gen)
    w = torch.randn(C, generator=gen)
    noise = torch.randn(B, 1, HW, generator=gen)
    ref = nr.noise_inject(x, w, noise)
    obuf, out, off = _guarded(x.numel(), False)
    _ok(_L().ffc_noise_inject(_ptr(_dev(x)), _ptr(_dev(w)), _ptr(_dev(noise)), _ptr(out), B, C, HW, _stream()),
        "ffc_noise_inject")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, off, x.numel()), "wrote outside out"
    _within("noise_inject", f"({B},{C},{HW})", out, ref, U * ref.abs() * SECOND_ORDER + DENORMAL)


def test_noise_inject_rejections_write_nothing():
    L = _L()
    B, C = 2, 3
    x, x6 = _dev(torch.zeros(B, C, 8)), _dev(torch.zeros(B, C, 6))
    w, nz = _dev(torch.ones(C)), _dev(torch.ones(B, 1, 8))
    out = _nan((B, C, 8))
    assert L.ffc_noise_inject(_ptr(x6), _ptr(w), _ptr(nz), _ptr(out), B, C, 6, _stream()) != 0
    assert _untouched(out), "HW = 6"
    good = [_ptr(x), _ptr(w), _ptr(nz), _ptr(out)]
    for i, name in enumerate(("x", "weight", "noise", "out")):
        args = list(good)
        args[i] = None
        assert L.ffc_noise_inject(*args, B, C, 8, _stream()) != 0, name
        assert _untouched(out), name


# --------------------------------------------------------------------------- ffc_quantize_u8
def _quantize(x):
    n = x.numel()
    out = _keep(torch.full((n + 64,), SENTINEL, device=DEV, dtype=torch.uint8))
    rc = _L().ffc_quantize_u8(_ptr(_dev(x)), _ptr(out), n, _stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("kind", ["four", "boundaries", "past-grid-cap"])
def test_quantize_u8_is_exact(kind):
    edges = nr.quantize_inputs(1001)
    if kind == "four":
        x = edges[:4].clone()
    elif kind == "boundaries":
        x = torch.cat((edges, torch.zeros(3)))
    else:
        # random bytes everywhere (the elements one grid stride apart differ), the boundary set first and last
        n = INJECT_CAP * 4 + 4
        x = torch.rand(n, generator=torch.Generator().manual_seed(9)) * 2.0 - 1.0
        x[:1001] = edges
        x[-1001:] = edges.flip(0)
    n = x.numel()
    assert n % 4 == 0 and x.dtype == torch.float32 and x.abs().max() <= 1.0
    ref = nr.quantize_u8(x)
    assert torch.equal(ref, nr.quantize_u8_np(x))
    rc, out = _quantize(x)
    _ok(rc, "ffc_quantize_u8")
    got = out.cpu()
    print(f"OBS quantize n={n} bytes that differ {int((got[:n] != ref).sum())}")
    assert torch.equal(got[:n], ref)
    assert got[n:].eq(SENTINEL).all(), "wrote behind the output"


def test_quantize_u8_rejections_write_nothing():
    x = nr.quantize_inputs(1000)[:8]
    out = _keep(torch.full((72,), SENTINEL, device=DEV, dtype=torch.uint8))
    for n in (6, 0):
        assert _L().ffc_quantize_u8(_ptr(_dev(x)), _ptr(out), n, _stream()) != 0, n
        torch.cuda.synchronize()
        assert out.eq(SENTINEL).all(), n
