"""Kernel-level parity of csrc/cond_kernels.hip -- the conditional generator's stem (ffc_cond_stem_forward),
its four backward kernels (ffc_cond_stem_backward), the label-embedding row gather and scatter
(ffc_embed_gather_rows / ffc_embed_scatter_rows) -- and of ffc_noise_wgrad (csrc/caller_kernels.hip), each
called through the C ABI with raw pointers against a float64 CPU reference of the same operation
(tests/cond_refs.py, itself checked in test_cond_refs_cpu.py), at the shapes where a kernel's loop or the host
code changes path.  tests/test_gpu_cond.py stays as it is; this file adds to it.

Every output, slab and workspace is prefilled with NaN and must come back fully written; after a rejection it
must come back all NaN.  Device copies stay alive until the test ends.  Misaligned pointers (one float off,
inside a larger live allocation) go only to the entry points whose host code tests alignment: the backward's
dpre / w_in / w_label (rejected) and the gather's / scatter's table, out, grad, dtable (scalar path).  The
rejected oversize calls are given full-size buffers.

The label contract pinned down here: a label outside [0, num_classes) as an int64 -- -1, num_classes, and
2^32, 2^32 + 1, whose low 32 bits are valid classes -- forms no address: NaN row in the forward (label half
of that sample only), skipped in dw_label, in no scatter.

Bounds (u = 2^-24, one fp32 rounding; SECOND_ORDER = 1 + 2^-20 covers (1 + u)^k - 1 - k u)
  normwise    oracle.ffc_oracle.normwise_err <= 1e-5, the TOL of the other kernel-level files: pre (per branch),
              dbias, dz, dlabel_embed.
  slab n      exactly 16 nv, nv the tile's samples; the fourth float exactly 0 (the kernel writes
              make_float4(cnt, mean, q, 0.0f)).
  slab mean   against the fp64 mean of the pre the kernel returned: d u sum|x| / n, d = 21, recounted in
              cond_stem_kernel's epilogue: s takes 16 adds per lane of which the first (to 0) is exact: 15;
              xor_sum_channel adds 5 times; one divide.  15 + 5 + 1 = 21 (fewer in a partly filled tile).
  slab M2     a sum of non-negative terms: k u ref + n (mean bound)^2, k = 23: d = acc - mean rounds once, so
              d^2 carries 2; the fma chain q = fma(d, d, q) rounds 16 times (the first, fma(d, d, 0), rounds
              too); xor_sum_channel 5.  2 + 16 + 5 = 23.  sum (x - m')^2 = M2 + n (m' - m)^2 exactly for the
              kernel's mean m', hence the second term.
  dw          elementwise gamma_B sum_b |a g|, gamma_B = B u / (1 - B u): cond_stem_wgrad_kernel is a chain of
              one fma per sample (samples with a bad label are skipped: a shorter chain).
  scatter     torch.equal with the float32 sum in sample order; gather torch.equal (NaN positions apart).
  noise_wgrad u |ref| (1 + 2^-20) + 2^-40 sum|g n|: the kernel adds exact fp64 products in fp64 -- at most
              B HW <= 4100 < 2^13 of them per channel in these cases (per thread ceil(HW / 1024) B groups of
              4, then 6 shuffle steps and 3 adds), so any order is within 2^13 2^-53 sum|g n| -- and rounds
              once to fp32.

Case -> branch it is there for
  forward     (B, z_size, num_classes): (1, 1, 1) one sample, one k, nv = 1: 15 of 16 accumulator rows
              masked; (31, 63, 3) nv = 31 and K = 63, one short of the tile and of the chunk; (32, 64, 64)
              exactly one tile and one chunk on both branches; (33, 65, 65) two tiles, the second of one
              sample (bt = 1, slab rows (branch * 2 + 1) * 256 + c, counts 512 and 16), two chunks, the second
              of one k (the k < K guard and the OOB weight load at k = 65 .. 127); (65, 129, 130) three tiles
              and three chunks on both branches.  Each with a slab and with slab = NULL (bit-identical pre), and
              with the label patterns one-class, classes-left-out and (B >= 33) per-tile.
  contract    B = 40, NC = 3: bad labels -1, 3, 2^32, 2^32 + 1 at samples 2, 5, 35, 36 (both tiles), and at
              32, 33, 35, 36 (tile 1 only: tile 0's label slab row stays bit-equal).
  backward    (1, 1, 1); (3, 5, 2) a partly filled CS_DB group and 16-k grid row; (4, 16, 17) a full CS_DB group,
              16-k grid rows 1 and 2 (k = 16 alone in the second); (5, 64, 65); (6, 1024, 3) the 64 KB
              dynamic-LDS limit of cond_stem_dinput_kernel, two workgroups, the second of two samples;
              (37, 70, 130) ten dinput workgroups, dbias lanes over ten rounds.  One output at a time (the other
              five NULL and left NaN) at (3, 5, 2) and (37, 70, 130); bad labels at the contract shape.
              Rejected: z_size 1025, num_classes 1025, B 0, dpre / w_in / w_label one float off alignment,
              dlabel_embed without ws.
  rows        D 1 / 3 (scalar, one block), 4 (one float4), 1020 (255 float4: one thread idle), 1024 (exactly one
              vector block), 1028 (a second vector block of one float4), 1030 (scalar, five blocks, the last of
              6), 16384 (the critic's plane: 16 vector blocks); NC = 7, B = 1 and B = 9 (class 3 three times,
              four classes absent, the four bad labels); D % 4 == 0 also with table / out, grad / dtable one
              float off alignment (scalar path, bit-equal to the vector path).  64 NaN floats behind each
              output.  Rejected: gather B = 65536, scatter num_classes = 65536, D = 0, each NULL pointer.
  noise_wgrad (B, C, HW): (1, 1, 4) one float4; (3, 5, 96) the earlier case; (2, 3, 1024) HW / 4 = 256, every
              thread one step; (2, 3, 1028) thread 0 a second step; (1, 2, 4100) HW / 4 = 1025: five steps for
              thread 0, four for the rest; (2, 300, 36) more channels than threads, 9 float4.  HW = 6 and each
              NULL pointer rejected.
  wrapper     _autograd.cond_stem on cond_refs.Stem, train and eval, (33, 8, 3) and (65, 70, 70): the two- and
              three-row stem slab with unequal counts into ffc_bn_reduce_finalize_batch; TOL 1e-4 and the
              pre-BN bias treatment of test_gpu_cond.test_stem_vs_float64_torch.

Observed on the first MI355X run (61 tests in 4.7 s, every one passing; no kernel or wrapper had to change, so
none of them fails against the parent commit's library), as the largest |got - ref| / limit of the family's
bound unless a normwise error is named.  dw at B = 1 and noise_wgrad sit just under 1 by construction: a
correctly rounded result is off by up to half an ulp, which is u |ref| at a power of two.
  pre         normwise 5.8e-07 (the fp32 MFMA products at K <= 130: near sqrt(K) u, as supposed)
  slab        n and the padding exact; mean 0.15; M2 0.14
  dw_in       0.99 at (1, 1, 1), 0.17 at (37, 70, 130)      dw_label 0.99
  db_in       normwise 1.0e-07    db_label 1.1e-07    dz 1.5e-07 (K = 1024 included)    dlabel_embed 2.2e-07
  rows        gather and scatter bit-equal in every case, guards intact
  noise_wgrad 0.96 at (2, 300, 36), 0.66 at (1, 2, 4100)
  wrapper     4.2e-07 over outputs, running statistics and gradients (TOL 1e-4)
"""
import pytest
import torch

import cond_refs as cr
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = cr.TOL
WRAPPER_TOL = 1e-4
NAN = float("nan")
GUARD = 64            # NaN floats behind each gather / scatter output


def _L():
    import fastfourierconvolution_amd  # noqa: F401  (registers torch.ops.ffc.*)
    from fastfourierconvolution_amd import _runtime as rt
    return rt.lib()


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


def _nan(shape):
    return _keep(torch.full(shape, NAN, device=DEV, dtype=torch.float32))


def _dev(t):
    """a device copy that stays alive until the test ends (the ABI takes raw pointers: a temporary freed before
    the launch could be handed to the next allocation)"""
    return None if t is None else _keep(t.to(DEV).contiguous())


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
    print(f"OBS {family} {what} {e:.3e} (/ TOL {e / TOL:.3f})")
    return e


def _within(family, what, got, ref, lim):
    """elementwise |got - ref| <= lim; prints the largest |got - ref| / lim"""
    assert not torch.isnan(got).any(), f"{what}: unwritten (NaN) elements"
    diff = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    worst = float((diff / lim.clamp_min(1e-300)).max())
    print(f"OBS {family} {what} max diff / limit {worst:.3e}")
    assert (diff <= lim).all(), (what, worst)


def _offset(t, floats=1):
    """a device copy of t that starts `floats` floats past a 16-byte boundary, inside a larger live allocation"""
    buf = _keep(torch.zeros(t.numel() + 8, device=DEV))
    view = buf[floats:floats + t.numel()]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == 4 * floats
    return view


# --------------------------------------------------------------------------- stem forward
class _Fwd:
    """device operands of the stem's forward at one shape"""

    def __init__(self, B, Kz, NC):
        self.shape = (B, Kz, NC)
        self.host = cr.stem_inputs(B, Kz, NC)
        self.dev = [_dev(t) for t in self.host]
        self.rows = _L().ffc_cond_stem_slab_rows(B)
        assert self.rows == (B + cr.TILE - 1) // cr.TILE

    def run(self, labels, with_slab=True):
        B, Kz, NC = self.shape
        z, embed, w_in, b_in, w_label, b_label = self.dev
        out = _nan((B, 2 * cr.CH, 4, 4))
        slab = _nan((2, self.rows, cr.CH, 4)) if with_slab else None
        _ok(_L().ffc_cond_stem_forward(_ptr(z), _ptr(_dev(labels)), _ptr(embed), _ptr(w_in), _ptr(b_in), _ptr(w_label),
                                       _ptr(b_label), B, Kz, NC, _ptr(out), _ptr(slab), _stream()),
            "ffc_cond_stem_forward")
        torch.cuda.synchronize()
        return out.cpu(), None if slab is None else slab.cpu()

    def ref(self, labels):
        return cr.stem_pre(self.host[0], labels, *self.host[1:])


def _check_slab(what, slab, pre, B):
    """the kernel's slab against the fp64 statistics of the pre it returned"""
    assert not torch.isnan(slab).any(), f"{what}: unwritten slab rows"
    ref, mag = cr.stem_slab(pre, B), cr.stem_slab_abs(pre, B)
    n = ref[..., 0]
    assert torch.equal(slab[..., 0].double(), n), what
    assert bool((slab[..., 3] == 0).all()), what
    lim_mean = cr.mean_limit(mag, n)
    _within("slab_mean", what, slab[..., 1], ref[..., 1], lim_mean)
    _within("slab_m2", what, slab[..., 2], ref[..., 2], cr.m2_limit(ref[..., 2], n, lim_mean))


@pytest.mark.parametrize("B,Kz,NC", cr.FWD_CASES)
def test_stem_forward_matches_fp64(B, Kz, NC):
    f = _Fwd(B, Kz, NC)
    pats = cr.label_patterns(B, NC)
    assert len(pats) == (1 if NC == 1 else 3 if B > cr.TILE else 2)
    for name, labels in pats.items():
        what = f"({B},{Kz},{NC}) {name}"
        ref = f.ref(labels)
        pre, slab = f.run(labels)
        pre0, _ = f.run(labels, with_slab=False)
        assert not torch.isnan(pre0).any() and torch.equal(pre, pre0), f"{what}: pre differs without a slab"
        for br, branch in enumerate(("input", "label")):
            half = slice(cr.CH * br, cr.CH * (br + 1))
            assert _err("pre", f"{what} {branch}", pre[:, half], ref[:, half]) <= TOL
        _check_slab(what, slab, pre, B)


@pytest.mark.parametrize("where", ["both-tiles", "tile-1"])
def test_stem_forward_label_contract(where):
    """an out-of-range label: NaN in the label half of its sample, and nothing else moves by a bit"""
    B, Kz, NC = cr.CONTRACT
    bad_at = list(cr.CONTRACT_BAD if where == "both-tiles" else cr.CONTRACT_BAD_TILE1)
    f = _Fwd(B, Kz, NC)
    clean = cr.label_patterns(B, NC)["per-tile"]
    bad = cr.with_bad_labels(clean, bad_at, NC)
    assert bad[bad_at].tolist() == [-1, 3, 2 ** 32, 2 ** 32 + 1]
    pre0, slab0 = f.run(clean)
    pre1, slab1 = f.run(bad)
    assert not torch.isnan(pre0).any() and not torch.isnan(slab0).any()
    good_at = [b for b in range(B) if b not in bad_at]
    assert torch.isnan(pre1[bad_at, cr.CH:]).all(), "a bad label's row is not NaN"
    assert torch.equal(pre1[bad_at, :cr.CH], pre0[bad_at, :cr.CH]), "the input half of a bad sample moved"
    assert torch.equal(pre1[good_at], pre0[good_at]), "another sample moved"
    assert torch.equal(slab1[0], slab0[0]), "the input branch's slab moved"
    bad_tiles = sorted({b // cr.TILE for b in bad_at})
    assert bad_tiles == ([0, 1] if where == "both-tiles" else [1])
    for t in range(f.rows):
        if t in bad_tiles:
            assert torch.equal(slab1[1, t, :, 0], slab0[1, t, :, 0]) and torch.isnan(slab1[1, t, :, 1:3]).all(), t
        else:
            assert torch.equal(slab1[1, t], slab0[1, t]), f"label slab row of the clean tile {t} moved"
    pre2, _ = f.run(bad, with_slab=False)
    assert torch.equal(torch.isnan(pre2), torch.isnan(pre1)) and torch.equal(pre2.nan_to_num(), pre1.nan_to_num())


def test_stem_forward_rejections_write_nothing():
    L = _L()
    B, Kz, NC = 3, 5, 2
    f = _Fwd(B, Kz, NC)
    labels = _dev(cr.label_patterns(B, NC)["one-class"])
    out, slab = _nan((B, 2 * cr.CH, 4, 4)), _nan((2, 1, cr.CH, 4))
    good = [_ptr(t) for t in (f.dev[0], labels, *f.dev[1:])]
    for i, name in enumerate(("z", "labels", "label_embed", "w_in", "bias_in", "w_label", "bias_label")):
        args = list(good)
        args[i] = None
        assert L.ffc_cond_stem_forward(*args, B, Kz, NC, _ptr(out), _ptr(slab), _stream()) != 0, name
        assert L.ffc_last_error() and _untouched(out, slab), name
    for what, sizes in (("B = 0", (0, Kz, NC)), ("z_size = 0", (B, 0, NC)), ("num_classes = 0", (B, Kz, 0))):
        assert L.ffc_cond_stem_forward(*good, *sizes, _ptr(out), _ptr(slab), _stream()) != 0, what
        assert _untouched(out, slab), what
    assert L.ffc_cond_stem_forward(*good, B, Kz, NC, None, _ptr(slab), _stream()) != 0
    off = _nan((2 * cr.CH * 4 + 8,))[1:]
    assert L.ffc_cond_stem_forward(*good, B, Kz, NC, _ptr(out), _ptr(off), _stream()) != 0, "misaligned slab"
    assert _untouched(out, slab, off)


# --------------------------------------------------------------------------- stem backward
class _Bwd:
    """device operands of the stem's backward at one shape; run() -> dict of the outputs asked for (CPU) and
    the six NaN-prefilled device buffers"""

    def __init__(self, B, Kz, NC, labels):
        self.shape = (B, Kz, NC)
        z, embed, w_in, _, w_label, _ = cr.stem_inputs(B, Kz, NC)
        self.host = (cr.dpre_inputs(B), z, labels, embed, w_in, w_label)
        self.dev = [_dev(t) for t in self.host]
        self.shapes = {"dw_in": (Kz, cr.CH, 4, 4), "db_in": (cr.CH,), "dw_label": (NC, cr.CH, 4, 4),
                       "db_label": (cr.CH,), "dz": (B, Kz), "dlabel_embed": (NC, NC)}

    def ref(self):
        return cr.stem_backward(*self.host)

    def call(self, bufs, want, ws, dev=None, sizes=None):
        p = [_ptr(bufs[k]) if k in want else None for k in cr.GRADS]
        return _L().ffc_cond_stem_backward(*[_ptr(t) for t in (self.dev if dev is None else dev)],
                                           *(self.shape if sizes is None else sizes), *p, _ptr(ws), _stream())

    def buffers(self):
        B, _, NC = self.shape
        return {k: _nan(self.shapes[k]) for k in cr.GRADS}, _nan((B * NC,))

    def run(self, want=cr.GRADS):
        bufs, ws = self.buffers()
        _ok(self.call(bufs, want, ws), "ffc_cond_stem_backward")
        torch.cuda.synchronize()
        for k in cr.GRADS:
            if k not in want:
                assert torch.isnan(bufs[k]).all(), f"{k} written though its pointer was NULL"
        if "dlabel_embed" not in want:
            assert torch.isnan(ws).all(), "ws written without dlabel_embed"
        return {k: bufs[k].cpu() for k in want}


def _check_bwd(what, got, ref, B, labels, NC):
    for k in ("dw_in", "dw_label"):
        _within(k, what, got[k], ref[k], cr.wgrad_limit(B, ref["abs_" + k]))
    for k in ("db_in", "db_label", "dz", "dlabel_embed"):
        if float(ref[k].abs().max()) == 0.0:       # every sample dropped: exact zeros
            assert bool((got[k] == 0).all()), (what, k)
        else:
            assert _err(k, what, got[k], ref[k]) <= TOL, (what, k)
    absent = [c for c in range(NC) if c not in labels.tolist()]
    assert bool((got["dlabel_embed"][absent] == 0).all()), f"{what}: rows of absent classes are not exactly 0"


@pytest.mark.parametrize("B,Kz,NC", cr.BWD_CASES)
def test_stem_backward_matches_fp64(B, Kz, NC):
    for name, labels in cr.label_patterns(B, NC).items():
        if name == "one-class" and NC > 1:
            continue                                # the two richer patterns where there are any
        what = f"({B},{Kz},{NC}) {name}"
        b = _Bwd(B, Kz, NC, labels)
        got = b.run()
        _check_bwd(what, got, b.ref(), B, labels, NC)
        again = b.run()
        for k in cr.GRADS:
            assert torch.equal(got[k], again[k]), f"{what}: {k} differs between two runs"


@pytest.mark.parametrize("B,Kz,NC", [(3, 5, 2), (37, 70, 130)])
def test_stem_backward_one_output_at_a_time(B, Kz, NC):
    """each output alone, the other five NULL (and left NaN): bit-equal to the call that asks for all six"""
    labels = list(cr.label_patterns(B, NC).values())[-1]
    b = _Bwd(B, Kz, NC, labels)
    every = b.run()
    for k in cr.GRADS:
        alone = b.run(want=(k,))
        assert not torch.isnan(alone[k]).any(), k
        assert torch.equal(alone[k], every[k]), f"{k} alone differs from {k} among all six"


@pytest.mark.parametrize("where", ["both-tiles", "tile-1"])
def test_stem_backward_drops_bad_labels_from_the_label_path_only(where):
    B, Kz, NC = cr.CONTRACT
    bad_at = list(cr.CONTRACT_BAD if where == "both-tiles" else cr.CONTRACT_BAD_TILE1)
    clean = cr.label_patterns(B, NC)["per-tile"]
    bad = cr.with_bad_labels(clean, bad_at, NC)
    b0, b1 = _Bwd(B, Kz, NC, clean), _Bwd(B, Kz, NC, bad)
    g0, g1 = b0.run(), b1.run()
    _check_bwd(f"bad labels {where}", g1, b1.ref(), B, bad[cr.in_range(bad, NC)], NC)
    for k in ("dz", "dw_in", "db_in", "db_label"):
        assert torch.equal(g1[k], g0[k]), f"{k} moved with a bad label"
    assert not torch.equal(g1["dw_label"], g0["dw_label"])
    # every label bad: exact zeros on the label path, everything else as before
    none = torch.tensor(cr.bad_labels(NC) * (B // 4), dtype=torch.int64)
    b2 = _Bwd(B, Kz, NC, none)
    g2 = b2.run()
    assert bool((g2["dw_label"] == 0).all()) and bool((g2["dlabel_embed"] == 0).all())
    for k in ("dz", "dw_in", "db_in", "db_label"):
        assert torch.equal(g2[k], g0[k]), k


def test_stem_backward_rejections_write_nothing():
    """full-size buffers for the oversize calls: were a check missing, the launch would stay in bounds"""
    B = 2
    labels = torch.tensor([1, 0], dtype=torch.int64)
    for what, (Kz, NC) in (("z_size 1025", (1025, 3)), ("num_classes 1025", (3, 1025))):
        b = _Bwd(B, Kz, NC, labels)
        bufs, ws = b.buffers()
        assert b.call(bufs, cr.GRADS, ws) != 0, what
        assert _L().ffc_last_error() and _untouched(ws, *bufs.values()), what
        _LIVE.clear()
    b = _Bwd(B, 5, 3, labels)
    bufs, ws = b.buffers()
    assert b.call(bufs, cr.GRADS, ws, sizes=(0, 5, 3)) != 0, "B 0"
    assert _untouched(ws, *bufs.values()), "B 0"
    assert b.call(bufs, cr.GRADS, None) != 0, "dlabel_embed without ws"
    assert _untouched(ws, *bufs.values()), "dlabel_embed without ws"
    for i, name in ((0, "dpre"), (4, "w_in"), (5, "w_label")):
        dev = list(b.dev)
        dev[i] = _offset(b.dev[i])
        assert b.call(bufs, cr.GRADS, ws, dev=dev) != 0, f"{name} one float off alignment"
        assert _untouched(ws, *bufs.values()), name
    for i, name in enumerate(("dpre", "z", "labels", "label_embed", "w_in", "w_label")):
        dev = list(b.dev)
        dev[i] = None
        assert b.call(bufs, cr.GRADS, ws, dev=dev) != 0, f"{name} NULL"
        assert _untouched(ws, *bufs.values()), name
    # the same operands are accepted as they are
    _ok(b.call(bufs, cr.GRADS, ws), "ffc_cond_stem_backward")
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t).any()) for t in bufs.values())


# --------------------------------------------------------------------------- gather / scatter
def _guarded(total, misaligned):
    """(buffer, view of `total` floats): four NaN floats in front (five when misaligned: the view then starts
    one float off 16-byte alignment) and GUARD NaN floats behind"""
    off = 5 if misaligned else 4
    buf = _keep(torch.full((total + off + GUARD,), NAN, device=DEV))
    view = buf[off:off + total]
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    return buf, view, off


def _guards_intact(buf, off, total):
    return bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + total:]).all()) and \
        buf.numel() - off - total == GUARD


def _same_with_nans(got, ref):
    return torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got.nan_to_num(), ref.nan_to_num())


def _variants(D):
    """(input misaligned, output misaligned): the aligned call, and for D % 4 == 0 each side one float off"""
    return [(False, False)] + ([(True, False), (False, True), (True, True)] if D % 4 == 0 else [])


def _labels_for(B, NC):
    if B == 9:
        return [cr.row_labels(B, NC)]
    return [cr.row_labels(B, NC)] + [torch.tensor([v], dtype=torch.int64) for v in cr.bad_labels(NC)]


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("D", cr.ROW_D)
def test_embed_gather_rows_is_exact(D, B):
    NC = 7
    table, _ = cr.row_inputs(B, NC, D)
    first = None
    for labels in _labels_for(B, NC):
        ref = cr.gather_rows(table, labels)
        assert bool(torch.isnan(ref).any()) == bool((~cr.in_range(labels, NC)).any())
        dl = _dev(labels)
        for mis_in, mis_out in _variants(D):
            tab = _offset(table) if mis_in else _dev(table)
            obuf, out, off = _guarded(B * D, mis_out)
            _ok(_L().ffc_embed_gather_rows(_ptr(tab), _ptr(dl), B, NC, D, _ptr(out), _stream()), "ffc_embed_gather_rows")
            torch.cuda.synchronize()
            got = out.cpu().reshape(B, D)
            what = (D, B, labels.tolist(), mis_in, mis_out)
            assert _same_with_nans(got, ref), what
            assert _guards_intact(obuf, off, B * D), f"{what}: wrote outside out"
            first = got if first is None else first
    assert first is not None


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("D", cr.ROW_D)
def test_embed_scatter_rows_is_the_fp32_sum_in_sample_order(D, B):
    NC = 7
    _, grad = cr.row_inputs(B, NC, D)
    for labels in _labels_for(B, NC):
        ref = cr.scatter_rows_f32(grad, labels, NC)
        dl = _dev(labels)
        for mis_in, mis_out in _variants(D):
            g = _offset(grad) if mis_in else _dev(grad)
            obuf, out, off = _guarded(NC * D, mis_out)
            _ok(_L().ffc_embed_scatter_rows(_ptr(g), _ptr(dl), B, NC, D, _ptr(out), _stream()), "ffc_embed_scatter_rows")
            torch.cuda.synchronize()
            got = out.cpu().reshape(NC, D)
            what = (D, B, labels.tolist(), mis_in, mis_out)
            assert not torch.isnan(got).any(), f"{what}: unwritten rows"
            assert torch.equal(got, ref), what
            absent = [c for c in range(NC) if c not in labels.tolist()]
            assert bool((got[absent] == 0).all()), what
            assert _guards_intact(obuf, off, NC * D), f"{what}: wrote outside dtable"


def test_embed_rows_rejections_write_nothing():
    L = _L()
    NC, D = 7, 4
    big = 65536
    table, grad = cr.row_inputs(9, NC, D)
    tab, lab = _dev(table), _dev(torch.zeros(big, dtype=torch.int64))
    out = _nan((big * D,))                         # full size for B = 65536
    assert L.ffc_embed_gather_rows(_ptr(tab), _ptr(lab), big, NC, D, _ptr(out), _stream()) != 0, "gather B = 65536"
    assert L.ffc_last_error() and _untouched(out)
    _ok(L.ffc_embed_gather_rows(_ptr(tab), _ptr(lab), big - 1, NC, D, _ptr(out), _stream()), "gather B = 65535")
    torch.cuda.synchronize()
    assert torch.equal(out[:(big - 1) * D].cpu().reshape(-1, D), table[:1].expand(big - 1, D))
    assert torch.isnan(out[(big - 1) * D:]).all()
    g, l9 = _dev(grad), _dev(cr.row_labels(9, NC))
    dtable = _nan((big * D,))                      # full size for num_classes = 65536
    assert L.ffc_embed_scatter_rows(_ptr(g), _ptr(l9), 9, big, D, _ptr(dtable), _stream()) != 0, "scatter NC = 65536"
    assert _untouched(dtable)
    out9 = _nan((9 * D,))
    for what, args in (("D = 0", (9, NC, 0)), ("B = 0", (0, NC, D)), ("num_classes = 0", (9, 0, D))):
        assert L.ffc_embed_gather_rows(_ptr(tab), _ptr(l9), *args, _ptr(out9), _stream()) != 0, "gather " + what
        assert L.ffc_embed_scatter_rows(_ptr(g), _ptr(l9), *args, _ptr(dtable), _stream()) != 0, "scatter " + what
        assert _untouched(out9, dtable), what
    for i, name in enumerate(("table / grad", "labels", "out / dtable")):
        ga, sa = [_ptr(tab), _ptr(l9), _ptr(out9)], [_ptr(g), _ptr(l9), _ptr(dtable)]
        ga[i] = sa[i] = None
        assert L.ffc_embed_gather_rows(ga[0], ga[1], 9, NC, D, ga[2], _stream()) != 0, name
        assert L.ffc_embed_scatter_rows(sa[0], sa[1], 9, NC, D, sa[2], _stream()) != 0, name
        assert _untouched(out9, dtable), name


# --------------------------------------------------------------------------- ffc_noise_wgrad
@pytest.mark.parametrize("B,C,HW", cr.NOISE_CASES)
def test_noise_wgrad_matches_fp64(B, C, HW):
    assert B * HW <= 2 ** 13
    g, noise = cr.noise_inputs(B, C, HW)
    ref, mag = cr.noise_wgrad(g, noise)
    gd, nd = _dev(g), _dev(noise)
    outs = []
    for _ in range(2):
        buf = _nan((C + GUARD,))
        _ok(_L().ffc_noise_wgrad(_ptr(gd), _ptr(nd), B, C, HW, _ptr(buf), _stream()), "ffc_noise_wgrad")
        torch.cuda.synchronize()
        assert torch.isnan(buf[C:]).all(), "wrote behind dweight"
        outs.append(buf[:C].cpu())
    _within("noise_wgrad", f"({B},{C},{HW})", outs[0], ref, cr.noise_wgrad_limit(ref, mag))
    assert torch.equal(outs[0], outs[1]), "two runs differ"


def test_noise_wgrad_rejections_write_nothing():
    L = _L()
    B, C = 2, 3
    g, nz = _dev(torch.ones(B, C, 8)), _dev(torch.ones(B, 1, 8))
    dw = _nan((C,))
    assert L.ffc_noise_wgrad(_ptr(g), _ptr(nz), B, C, 6, _ptr(dw), _stream()) != 0
    assert L.ffc_last_error() and _untouched(dw), "HW = 6"
    good = [_ptr(g), _ptr(nz)]
    for i, name in enumerate(("dout", "noise")):
        args = list(good)
        args[i] = None
        assert L.ffc_noise_wgrad(*args, B, C, 8, _ptr(dw), _stream()) != 0, name
        assert _untouched(dw), name
    assert L.ffc_noise_wgrad(*good, B, C, 8, None, _stream()) != 0, "dweight"
    assert _untouched(dw)


# --------------------------------------------------------------------------- the wrapper over more than one tile
@pytest.mark.parametrize("B,z_size,nc", [(33, 8, 3), (65, 70, 70)])
def test_stem_wrapper_over_several_tiles_vs_float64_torch(B, z_size, nc):
    """_autograd.cond_stem forward, running statistics after one step and every gradient against cond_refs.Stem
    in float64, train and eval: the multi-row stem slab (rows of 512 and 16 elements at B = 33) through
    ffc_bn_reduce_finalize_batch.  Conv biases in front of a train-mode BatchNorm have the exact gradient 0;
    their residue is measured against the norm of the layer's weight gradient (test_gpu_cond.py's docstring)."""
    from fastfourierconvolution_amd import _autograd as ag
    assert _L().ffc_cond_stem_slab_rows(B) == (2 if B == 33 else 3)
    gen = torch.Generator().manual_seed(100 * B + z_size + nc)
    ref = cr.Stem(z_size, nc)
    with torch.no_grad():
        for bn in (ref.label_conv[1], ref.input_conv[1]):
            bn.weight.copy_(1 + 0.1 * torch.randn(256, generator=gen))
            bn.bias.copy_(0.1 * torch.randn(256, generator=gen))
            bn.running_mean.copy_(0.1 * torch.randn(256, generator=gen))
            bn.running_var.copy_(0.5 + torch.rand(256, generator=gen))
    for train in (True, False):
        for name, labels in cr.label_patterns(B, nc).items():
            mine = cr.Stem(z_size, nc)
            mine.load_state_dict(ref.state_dict())
            mine = mine.to(DEV).train(train)
            gold = cr.Stem(z_size, nc)
            gold.load_state_dict(ref.state_dict())
            gold = gold.double().train(train)
            z = torch.randn(B, z_size, generator=gen)
            cot = torch.randn(B, 512, 4, 4, generator=gen)
            zg, zr = z.to(DEV).requires_grad_(True), z.double().requires_grad_(True)
            y = ag.cond_stem(mine, zg, _dev(labels))
            (y * cot.to(DEV)).sum().backward()
            yr = gold(zr, labels)
            (yr * cot.double()).sum().backward()
            what = (B, z_size, nc, train, name)
            errs = {"y": normwise_err(y.detach().cpu(), yr.detach())}
            for (k, v), (_, r) in zip(mine.state_dict().items(), gold.state_dict().items()):
                if k.endswith(("running_mean", "running_var")):
                    errs[k] = normwise_err(v.cpu(), r)
                elif k.endswith("num_batches_tracked"):
                    assert int(v) == int(r), (what, k)
            errs["z"] = normwise_err(zg.grad.cpu(), zr.grad)
            pg = dict(gold.named_parameters())
            for k, p in mine.named_parameters():
                assert p.grad is not None, (what, k)
                if train and k.endswith("0.bias"):   # exact gradient 0
                    errs[k] = float(p.grad.double().norm()) / float(pg[k.replace("bias", "weight")].grad.norm())
                else:
                    errs[k] = normwise_err(p.grad.cpu(), pg[k].grad)
            print(f"OBS wrapper {what} max {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
            bad = {k: v for k, v in errs.items() if not v <= WRAPPER_TOL}
            assert not bad, (what, bad)
            absent = [c for c in range(nc) if c not in labels.tolist()]
            assert all(bool((mine.label_embed.weight.grad[c] == 0).all()) for c in absent), what
