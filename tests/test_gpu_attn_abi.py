"""Kernel-level parity of csrc/attn_kernels.hip: ffc_attn_forward, ffc_attn_matrix and ffc_attn_backward (the
forward, the matrix kernel, the two prep kernels, dk/dv in both template sizes and dq) called through the C ABI
with raw pointers against the float64 references of tests/attn_refs.py (core_ref, core_bwd_ref; themselves
proven in tests/test_attn_refs_cpu.py).  tests/test_gpu_attn_kernels.py, which goes through the layer, stays
as it is; this file adds to it.

Every output and the workspace (y, L, o, P, dq, dk, dv, dgamma, ws) is prefilled with NaN and has 64 NaN
floats behind it: after a call every element in range is finite and every other float, stride padding
included, is still NaN; after a rejection everything is still NaN.  The inputs' stride padding is NaN too, so
a read of it shows.  Misaligned pointers start one float into a larger live allocation.  Device copies stay
alive until the test ends.  The backward is given the o and L the forward produced on the GPU.

Bounds (attn_refs, TOL = 1e-5; test_attn_refs_cpu.py proves that plain float32 stays under a quarter of each
on every input used here and that nine planted defects exceed them)
  y, o, dq, dk, dv   elementwise |got - ref| <= TOL (|ref| + rms of ref over the sample's tensor)
  P                  the same with the rms of the row; floored at 2^-126 on the early / late maximum
  L                  |got - ref| <= TOL max(1, |ref|)
  dgamma             |got - ref| <= TOL sum |dy o|
  zero results       dq, dk at N = 1 and on the one-hot case against TOL times their cancellation scale
  ws                 Dn[b, i] = sum_c dy o and the per-chunk partials of dgamma against the float64 sums of
                     the o the GPU returned: TOL times the sum of |dy o| over the same terms
  bit equality       torch.equal: scalar path = vector path, o = NULL, batch independence, the backward run
                     twice, gamma = 0, the N = 1 identities, y = fmaf(gamma, o_gpu, x)

Case (B x C x H x W) -> the branch it is there for
  1x8x1x1      one key; d = 1; 24 of 32 value rows masked; 31 of 32 queries and keys padded
  2x24x1x31    d = 3 (half h = 1 of the last k-step is the zero row); one short of a tile
  1x32x32x1    CB = 1 full; exactly one tile, the vector path (N % 4 == 0)
  3x40x1x33    CB = 2 with 8 rows in the second block, d = 5; a second tile of one key; B = 3
  2x64x6x6     C = 64 full; one vector tile and a ragged tile of four keys
  1x56x127x1   d = 7; four waves, the last tile one short
  2x32x1x128   exactly one workgroup of four full waves, vector path throughout
  3x24x3x43    N = 129 = 3 x 43: a second workgroup of one wave with one query, three waves return early
  1x40x1x255   a prep chunk one short of full
  2x8x16x16    exactly one prep chunk per sample, vector path
  1x64x257x1   a second prep chunk of one query, a second dgamma partial per sample
  65535x8x1x1  B at the grid limit (forward, matrix, backward): P = 1, o = v, L = fl(q k), y = fmaf(gamma, v,
               x), dv = fl(gamma dy), dq = dk = 0
  1x8x256x256  N at the limit, forward only: y and L at the first tile, the last tile and 64 other queries
  forms        at 2x64x6x6 and 3x24x3x43: q, k, v in three allocations with bstride + 4; a stacked buffer with
               bstride + 1 (the odd stride turns the vector path off at N % 4 == 0); gbstride = bstride + 8 with
               dq, dk, dv in three allocations; one float off alignment for v (forward) and q, k, dy, L, ws
               (backward), one at a time; o = NULL.  All bit-equal to the plain call.
  directed     offset / neg_offset (scores at +-100 +- 4), early_max / late_max (scores 0 .. -128 at N = 257),
               one_hot (N = 129), uniform (q = 0), gamma = -1.3, gamma = 0: see attn_refs._directed_core
  rejections   C in 0, 4, 12, 72, -8; H, W, B = 0; B = 65536 with full-size buffers; strides one short; each
               pointer NULL; N above the limit through ffc_attn_supported / ffc_attn_ws_floats only
  wrappers     torch.ops.ffc.self_attn / self_attn_matrix / self_attn_bwd on a wrong C, L, o or gamma

Observed on the first MI355X run (30 tests in 4.5 s, every one passing, the slowest -- the wrappers' test, which
loads the operators -- 1.5 s; the N = 65536 forward with its copies and checks 5.9 ms; no kernel and no host
code of attn_kernels.hip had to change), as the largest share of each family's bound:
  y       0.087 (gamma = -1.3)                       L       0.016 (N = 65536; 0.015 at 3x24x3x43)
  o       0.21 (1x40x1x255); 0.88 on the sampled rows of N = 65536, where o is a mean of 65536 values of either
          sign and its bound takes the rms of the sampled rows
  P       0.28 (offset: L near 100 is known to half an ulp of 7.6e-6, and P = exp(S - L)); 0.11 on random shapes
  dq      0.25 (2x32x1x128)      dk 0.43 (offset; 0.37 at 1x64x257x1)      dv 0.55 (offset; 0.34 at 1x40x1x255)
  dgamma  0.004                  Dn 0.021 and partials 0.021 (both at 65535x8x1x1)
  zero    dq and dk exactly 0 at N = 1 (both cases) and on the one-hot case, where o == v[:, perm] bit for bit
  equal   every bit-equality held: nine calling forms and o = NULL at both shapes, the scalar path at N = 128
          and 256, sample 2 alone, three identical samples, the second backward, gamma = 0, the N = 1
          identities at B = 65535, and y = fmaf(gamma, o, x) on all 15 996 elements tried
"""
import pytest
import torch

import attn_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAN = float("nan")
GUARD = R.GUARD
E_INVALID = -1


def _L():
    import fastfourierconvolution_amd  # noqa: F401  (registers torch.ops.ffc.*)
    from fastfourierconvolution_amd import _runtime as rt
    return rt.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(status, what):
    from fastfourierconvolution_amd._lib import check
    check(status, what)


_LIVE = []


def _keep(t):
    _LIVE.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is launched from this file
        pytest.exit(f"HIP error after a kernel of this file: {e}", returncode=3)
    _LIVE.clear()


class _Buf:
    """B slabs of ``n`` floats at a batch stride of ``stride`` floats inside one NaN-filled allocation, four
    NaN floats in front (five with ``mis``: the slabs then start one float off 16-byte alignment) and GUARD
    behind"""

    def __init__(self, B, n, stride=None, mis=False, fill=None):
        self.B, self.n, self.stride = B, n, n if stride is None else stride
        assert self.stride >= n
        self.off = 5 if mis else 4
        self.total = (B - 1) * self.stride + n
        self.buf = _keep(torch.full((self.off + self.total + GUARD,), NAN, device=DEV, dtype=torch.float32))
        self.idx = (torch.arange(B, device=DEV)[:, None] * self.stride + torch.arange(n, device=DEV)[None, :]
                    + self.off).reshape(-1)
        assert self.buf.data_ptr() % 16 == 0
        if fill is not None:
            self.buf[self.idx] = fill.to(DEV).reshape(-1).float()

    def ptr(self, floats=0):
        return self.buf.data_ptr() + 4 * (self.off + floats)

    def get(self, what):
        """the slabs (B, n) on the CPU: every element finite, every other float of the allocation still NaN"""
        torch.cuda.synchronize()
        data = self.buf.cpu()
        inside = data[self.idx.cpu()]
        assert bool(torch.isfinite(inside).all()), f"{what}: unwritten or non-finite elements in range"
        assert int(torch.isnan(data).sum()) == data.numel() - inside.numel(), f"{what}: wrote outside its range"
        return inside.reshape(self.B, self.n)

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.buf).all())


class _Call:
    """device operands of one case in one calling form.
    layout: "stacked" (one qkv buffer) or "separate" (three allocations); pad: floats added to bstride;
    glayout / gpad: the same for dq, dk, dv; mis: names of the pointers placed one float off alignment"""

    def __init__(self, c, layout="stacked", pad=0, glayout="stacked", gpad=0, mis=()):
        self.c, self.mis = c, set(mis)
        B, C, H, W = c["shape"]
        self.B, self.C, self.H, self.W = B, C, H, W
        self.N, self.d = H * W, C // 8
        N, d = self.N, self.d
        self.M = (2 * d + C) * N
        self.bstride, self.gbstride = self.M + pad, self.M + pad + gpad
        if layout == "stacked":
            assert not self.mis & {"q", "k", "v"}
            qkv = _Buf(B, self.M, self.bstride, fill=torch.cat([c["q"], c["k"], c["v"]], 1))
            self.q, self.k, self.v = qkv.ptr(), qkv.ptr(d * N), qkv.ptr(2 * d * N)
        else:
            bufs = [_Buf(B, c[n].shape[1] * N, self.bstride, mis=n in self.mis, fill=c[n]) for n in "qkv"]
            self.q, self.k, self.v = (b.ptr() for b in bufs)
        self.glayout = glayout
        self.x = _Buf(B, C * N, fill=c["x"])
        self.dy = _Buf(B, C * N, fill=c["dy"], mis="dy" in self.mis)
        self.gamma = _keep(torch.full((1,), float(c["gamma"]), device=DEV))
        self.args = (B, C, H, W)

    # ---- forward
    def forward_buffers(self, with_o=True):
        B, C, N = self.B, self.C, self.N
        return _Buf(B, C * N), _Buf(B, N, mis="L" in self.mis), _Buf(B, C * N) if with_o else None

    def forward(self, with_o=True):
        """-> dict(y, L, o (CPU)); keeps the device L and o for the matrix call and the backward"""
        y, Lb, o = self.forward_buffers(with_o)
        _ok(_L().ffc_attn_forward(self.q, self.k, self.v, self.bstride, self.x.ptr(), self.gamma.data_ptr(), y.ptr(),
                                  Lb.ptr(), o.ptr() if o else None, *self.args, _stream()), "ffc_attn_forward")
        self.Ldev, self.odev = Lb, o
        B, C, N = self.B, self.C, self.N
        out = dict(y=y.get("y").reshape(B, C, N), L=Lb.get("L"))
        if o:
            out["o"] = o.get("o").reshape(B, C, N)
        return out

    def matrix(self):
        B, N = self.B, self.N
        P = _Buf(B, N * N)
        _ok(_L().ffc_attn_matrix(self.q, self.k, self.bstride, self.Ldev.ptr(), P.ptr(), *self.args, _stream()),
            "ffc_attn_matrix")
        return P.get("P").reshape(B, N, N)

    # ---- backward
    def backward_buffers(self):
        B, C, N, d = self.B, self.C, self.N, self.d
        if self.glayout == "stacked":
            g = _Buf(B, self.M, self.gbstride)
            gp = (g.ptr(), g.ptr(d * N), g.ptr(2 * d * N))
            gb = (g,)
        else:
            gb = tuple(_Buf(B, r * N, self.gbstride) for r in (d, d, C))
            gp = tuple(b.ptr() for b in gb)
        nws = _L().ffc_attn_ws_floats(*self.args)
        assert nws == B * N + B * ((N + 255) // 256) > 0
        return gb, gp, _Buf(1, 1), _Buf(1, nws, mis="ws" in self.mis)

    def backward(self):
        """after forward(): -> dict(dq, dk, dv, dgamma, Dn, part (CPU))"""
        B, C, N, d = self.B, self.C, self.N, self.d
        gb, gp, dgamma, ws = self.backward_buffers()
        _ok(_L().ffc_attn_backward(self.dy.ptr(), self.q, self.k, self.v, self.bstride, self.odev.ptr(), self.Ldev.ptr(),
                                   self.gamma.data_ptr(), *gp, self.gbstride, dgamma.ptr(), ws.ptr(), *self.args,
                                   _stream()), "ffc_attn_backward")
        if self.glayout == "stacked":
            g = gb[0].get("dqkv").reshape(B, 2 * d + C, N)
            out = dict(dq=g[:, :d], dk=g[:, d:2 * d], dv=g[:, 2 * d:])
        else:
            out = {n: b.get(n).reshape(B, -1, N) for n, b in zip(("dq", "dk", "dv"), gb)}
        w = ws.get("ws").reshape(-1)
        out.update(dgamma=dgamma.get("dgamma").reshape(()), Dn=w[:B * N].reshape(B, N), part=w[B * N:].reshape(B, -1))
        return out


def _report(what, sh):
    print(f"OBS {what} " + " ".join(f"{k} {v:.3f}" for k, v in sh.items()))
    bad = {k: v for k, v in sh.items() if not v <= 1.0}
    assert not bad, (what, bad)


def _ws_shares(c, o_gpu, got):
    """Dn and the partials against the float64 sums of dy o_gpu, as shares of TOL sum |dy o_gpu|"""
    t = c["dy"].double() * o_gpu.double()
    B, _, N = t.shape
    chunks = (N + 255) // 256
    pad = torch.zeros(B, chunks * 256 - N, dtype=torch.float64)
    Dn, aDn = t.sum(1), t.abs().sum(1)
    part = torch.cat([Dn, pad], 1).reshape(B, chunks, 256).sum(-1)
    apart = torch.cat([aDn, pad], 1).reshape(B, chunks, 256).sum(-1)
    return dict(Dn=R.scale_share(got["Dn"], Dn, aDn), part=R.scale_share(got["part"], part, apart))


def _all(call, p_floor=False):
    """forward, matrix and backward of one call, each measured -> the results"""
    c = call.c
    got = call.forward()
    got["P"] = call.matrix()
    got.update(call.backward())
    sh = R.shares(c, {k: got[k] for k in ("y", "L", "o", "P", "dq", "dk", "dv", "dgamma")}, p_floor=p_floor)
    sh.update(_ws_shares(c, got["o"], got))
    _report(c["name"], sh)
    return got


def _same(a, b, keys, what):
    for k in keys:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


FWD, BWD = ("y", "L", "o"), ("dq", "dk", "dv", "dgamma", "Dn", "part")


# --------------------------------------------------------------------------- every kernel against float64
@pytest.mark.parametrize("name", list(R.ABI_RANDOM))
def test_random_shapes_match_fp64(name):
    got = _all(_Call(R.abi_case(name)))
    if R.abi_case(name)["shape"][2:] == (1, 1):
        print(f"OBS {name} N = 1: dq {float(got['dq'].abs().max()):.1e} dk {float(got['dk'].abs().max()):.1e}")


@pytest.mark.parametrize("name", R.ABI_DIRECTED)
def test_directed_numerics_match_fp64(name):
    c = R.abi_case(name)
    got = _all(_Call(c), p_floor=name in ("early_max", "late_max"))
    if name == "one_hot":
        perm = R.one_hot_perm(c["shape"][2] * c["shape"][3])
        e = float((got["o"].double() - c["v"][:, :, perm].double()).abs().max())
        print(f"OBS one_hot max |o[:, i] - v[:, perm(i)]| {e:.2e}")
    if name == "gamma_zero":
        assert torch.equal(got["y"], c["x"]), "gamma = 0: y is not x bit for bit"
        for k in ("dq", "dk", "dv"):
            assert bool((got[k] == 0).all()), f"gamma = 0: {k} is not exactly zero"
        assert float(c["bwd"].dgamma_scale) > 1.0


def test_y_is_gamma_o_plus_x_exactly():
    """y == fmaf(gamma, o_gpu, x) bit for bit, in both template sizes and at a negative gamma"""
    for name in ("3x24x3x43", "2x64x6x6", "gamma_neg"):
        c = R.abi_case(name)
        got = _Call(c).forward()
        ref = R.fma_f32(c["gamma"], got["o"], c["x"])
        n = int((got["y"] != ref).sum())
        print(f"OBS fmaf {name}: {n} of {ref.numel()} elements differ")
        assert torch.equal(got["y"], ref), name


def test_batch_at_the_grid_limit():
    """B = 65535, one key: the results are identities"""
    c = R.abi_case(R.GRID_LIMIT)
    call = _Call(c)
    got = _all(call)
    g = torch.tensor(c["gamma"], dtype=torch.float32)
    assert bool((got["P"] == 1).all()), "P != 1"
    assert torch.equal(got["o"], c["v"]), "o != v"
    assert torch.equal(got["L"].reshape(-1), (c["q"] * c["k"]).reshape(-1)), "L != fl(q k)"
    assert torch.equal(got["y"], R.fma_f32(c["gamma"], c["v"], c["x"])), "y != fmaf(gamma, v, x)"
    exact = g.double() * c["dy"].double()
    assert bool(((got["dv"].double() - exact).abs() <= 2.0 ** -24 * exact.abs()).all()), "dv is not gamma dy to one rounding"
    print(f"OBS grid limit: dq max {float(got['dq'].abs().max()):.1e} dk max {float(got['dk'].abs().max()):.1e}")


def test_n_at_the_limit_forward():
    """N = 65536 (1 x 8 x 256 x 256), forward only: y and L at the first tile, the last tile and 64 other
    queries against float64 rows; no matrix and no backward at this N.  y's rms is taken over the sampled
    queries."""
    c = R.limit_case()
    call = _Call(dict(c, dy=c["x"]))
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    got = call.forward()
    end.record()
    torch.cuda.synchronize()
    rows = c["rows"]
    y, ref = got["y"][0][:, rows].double(), c["y"]
    lim = R.TOL * (ref.abs() + ref.pow(2).mean().sqrt())
    sh = dict(y=float(((y - ref).abs() / lim).max()), L=R.L_share(got["L"][0, rows], c["L"]),
              o=float(((got["o"][0][:, rows].double() - c["o"]).abs() / (R.TOL * (c["o"].abs() + c["o"].pow(2).mean().sqrt()))).max()))
    print(f"OBS N = 65536 forward, checks and copies included: {start.elapsed_time(end):.1f} ms")
    _report("1x8x256x256", sh)


# --------------------------------------------------------------------------- calling forms
@pytest.mark.parametrize("name", R.FORMS)
def test_calling_forms_are_bit_equal_to_the_plain_call(name):
    c = R.abi_case(name)
    plain = _Call(c)
    ref = _all(plain)
    forms = {
        "three allocations, bstride + 4": dict(layout="separate", pad=4),
        "stacked, bstride + 1": dict(pad=1),
        "gbstride = bstride + 8, three gradient allocations": dict(gpad=8, glayout="separate"),
        "v one float off": dict(layout="separate", mis=("v",)),
        "q one float off": dict(layout="separate", mis=("q",)),
        "k one float off": dict(layout="separate", mis=("k",)),
        "dy one float off": dict(mis=("dy",)),
        "L one float off": dict(mis=("L",)),
        "ws one float off": dict(mis=("ws",)),
    }
    for what, kw in forms.items():
        call = _Call(c, **kw)
        got = call.forward()
        got["P"] = call.matrix()
        got.update(call.backward())
        _same(got, ref, FWD + ("P",) + BWD, f"{name} {what}")
    call = _Call(c)
    no_o = call.forward(with_o=False)
    _same(no_o, ref, ("y", "L"), f"{name} o = NULL")
    print(f"OBS forms {name}: {len(forms)} forms and o = NULL bit-equal to the plain call")


def test_vector_and_scalar_paths_agree_at_n_multiple_of_4():
    """N = 128 and 256: the plain call takes the vector path; an odd stride or one pointer off alignment takes
    load_keys16's scalar path over the same elements in the same order"""
    for name in ("2x32x1x128", "2x8x16x16"):
        c = R.abi_case(name)
        call = _Call(c)
        ref = call.forward()
        ref.update(call.backward())
        for what, kw in (("bstride + 1", dict(pad=1)), ("v off", dict(layout="separate", mis=("v",))),
                         ("q off", dict(layout="separate", mis=("q",))), ("L off", dict(mis=("L",))),
                         ("ws off", dict(mis=("ws",))), ("dy off", dict(mis=("dy",)))):
            call = _Call(c, **kw)
            got = call.forward()
            got.update(call.backward())
            _same(got, ref, FWD + BWD, f"{name} {what}")
    print("OBS scalar path = vector path at N = 128 and 256")


# --------------------------------------------------------------------------- independence and determinism
def test_samples_are_independent_and_the_backward_is_deterministic():
    name = "3x24x3x43"
    c = R.abi_case(name)
    call = _Call(c)
    full = call.forward()
    full["P"] = call.matrix()
    full.update(call.backward())
    again = call.backward()
    _same(again, full, BWD, "the backward run twice")
    one = _Call(R.one_sample(name, 2))
    alone = one.forward()
    alone["P"] = one.matrix()
    alone.update(one.backward())
    for k in FWD + ("P", "dq", "dk", "dv", "Dn"):
        assert torch.equal(alone[k][0], full[k][2]), f"sample 2 alone differs in {k}"
    three = _Call(R.three_copies(name))
    same = three.forward()
    same["P"] = three.matrix()
    same.update(three.backward())
    for k in FWD + ("P", "dq", "dk", "dv", "Dn", "part"):
        assert torch.equal(same[k][0], same[k][1]) and torch.equal(same[k][0], same[k][2]), f"identical samples differ in {k}"
        if k != "part":
            assert torch.equal(same[k][0], full[k][0]), k
    print("OBS independence: sample 2 alone, three identical samples and the second backward are bit-equal")


# --------------------------------------------------------------------------- rejections
def _rejected(status, entry):
    msg = _L().ffc_last_error().decode()
    assert status == E_INVALID and entry in msg, (status, msg)


def test_rejections_write_nothing():
    L = _L()
    c = R.abi_case("2x64x6x6")
    call = _Call(c)
    fw = call.forward()
    assert set(fw) == set(FWD)
    B, C, H, W = call.args
    N, d = call.N, call.d
    y, Lb, o = call.forward_buffers()
    P = _Buf(B, N * N)
    gb, gp, dgamma, ws = call.backward_buffers()
    outs = (y, Lb, o, P, dgamma, ws) + gb
    g = call.gamma.data_ptr()

    def fwd(q=call.q, k=call.k, v=call.v, bs=call.bstride, x=call.x.ptr(), gamma=g, yp=y.ptr(), Lp=Lb.ptr(), shape=call.args):
        return L.ffc_attn_forward(q, k, v, bs, x, gamma, yp, Lp, o.ptr(), *shape, _stream())

    def mat(q=call.q, k=call.k, bs=call.bstride, Lp=call.Ldev.ptr(), Pp=P.ptr(), shape=call.args):
        return L.ffc_attn_matrix(q, k, bs, Lp, Pp, *shape, _stream())

    def bwd(shape=call.args, bs=call.bstride, gbs=call.gbstride, **kw):
        a = dict(dy=call.dy.ptr(), q=call.q, k=call.k, v=call.v, o=call.odev.ptr(), L=call.Ldev.ptr(), gamma=g, dq=gp[0],
                 dk=gp[1], dv=gp[2], dgamma=dgamma.ptr(), ws=ws.ptr())
        a.update(kw)
        return L.ffc_attn_backward(a["dy"], a["q"], a["k"], a["v"], bs, a["o"], a["L"], a["gamma"], a["dq"], a["dk"],
                                   a["dv"], gbs, a["dgamma"], a["ws"], *shape, _stream())

    def nothing_written(what):
        assert all(b.untouched() for b in outs), f"{what}: a rejected call wrote"

    shapes = [(B, Cx, H, W) for Cx in (0, 4, 12, 72, -8)] + [(B, C, 0, W), (B, C, H, 0), (0, C, H, W)]
    for shape in shapes:
        _rejected(fwd(shape=shape), "ffc_attn_forward")
        _rejected(mat(shape=shape), "ffc_attn_matrix")
        _rejected(bwd(shape=shape), "ffc_attn_backward")
        nothing_written(shape)
    M = (2 * d + C) * N
    _rejected(fwd(bs=M - 1), "ffc_attn_forward")
    _rejected(bwd(bs=M - 1), "ffc_attn_backward")
    _rejected(bwd(gbs=M - 1), "ffc_attn_backward")
    _rejected(mat(bs=d * N - 1), "ffc_attn_matrix")
    nothing_written("strides one short")
    for n in ("q", "k", "v", "x", "gamma", "yp", "Lp"):
        _rejected(fwd(**{n: None}), "ffc_attn_forward")
    for n in ("q", "k", "Lp", "Pp"):
        _rejected(mat(**{n: None}), "ffc_attn_matrix")
    for n in ("dy", "q", "k", "v", "o", "L", "gamma", "dq", "dk", "dv", "dgamma", "ws"):
        _rejected(bwd(**{n: None}), "ffc_attn_backward")
    nothing_written("NULL pointers")
    # the same operands are accepted as they are
    _ok(fwd(), "ffc_attn_forward")
    _ok(mat(), "ffc_attn_matrix")
    _ok(bwd(), "ffc_attn_backward")
    assert torch.equal(y.get("y").reshape(fw["y"].shape), fw["y"])
    P.get("P"), ws.get("ws"), dgamma.get("dgamma")
    print("OBS rejections: shapes, strides and NULL pointers refused with nothing written")


def test_batch_above_the_grid_limit_is_rejected_with_full_size_buffers():
    """B = 65536 at N = 1, every buffer sized for it: were the check missing, the launch would stay in bounds"""
    L = _L()
    big = 65536
    c = dict(R.abi_case(R.GRID_LIMIT))
    for k in ("q", "k", "v", "x", "dy"):
        c[k] = torch.cat([c[k], c[k][:1]], 0)
    c["shape"] = (big, 8, 1, 1)
    call = _Call(c)
    y, Lb, o = _Buf(big, 8), _Buf(big, 1), _Buf(big, 8)
    Lin, oin = _Buf(big, 1, fill=torch.zeros(big)), _Buf(big, 8, fill=c["v"])
    P, g, dgamma, ws = _Buf(big, 1), _Buf(big, 10), _Buf(1, 1), _Buf(1, 2 * big)
    assert L.ffc_attn_ws_floats(big, 8, 1, 1) == 0 and L.ffc_attn_ws_floats(big - 1, 8, 1, 1) == 2 * (big - 1)
    ga = call.gamma.data_ptr()
    _rejected(L.ffc_attn_forward(call.q, call.k, call.v, 10, call.x.ptr(), ga, y.ptr(), Lb.ptr(), o.ptr(), big, 8, 1, 1,
                                 _stream()), "ffc_attn_forward")
    _rejected(L.ffc_attn_matrix(call.q, call.k, 10, Lin.ptr(), P.ptr(), big, 8, 1, 1, _stream()), "ffc_attn_matrix")
    _rejected(L.ffc_attn_backward(call.dy.ptr(), call.q, call.k, call.v, 10, oin.ptr(), Lin.ptr(), ga, g.ptr(), g.ptr(1),
                                  g.ptr(2), 10, dgamma.ptr(), ws.ptr(), big, 8, 1, 1, _stream()), "ffc_attn_backward")
    assert all(b.untouched() for b in (y, Lb, o, P, g, dgamma, ws))


def test_n_above_the_limit_is_refused_by_the_shape_queries():
    """no device call with such an N"""
    L = _L()
    assert L.ffc_attn_supported(8, 256, 256) == 1 and L.ffc_attn_ws_floats(1, 8, 256, 256) == 65536 + 256
    for H, W in ((1, 65537), (65537, 1), (65536, 65536), (46341, 46341)):
        assert L.ffc_attn_supported(8, H, W) == 0, (H, W)
        assert L.ffc_attn_ws_floats(1, 8, H, W) == 0, (H, W)
    for name in R.ABI_ALL:
        assert L.ffc_attn_ws_floats(*R.abi_case(name)["shape"]) > 0, name


# --------------------------------------------------------------------------- the wrappers' argument checks
# These tests must never run against a library from before the checks were added to _autograd.py: without the
# checks each of these calls launches a kernel on a wrong stride or a short buffer, an out-of-bounds access on
# a machine that others share.  They belong to the commit that adds the checks and to its descendants only.
def test_wrappers_refuse_wrong_arguments_before_any_launch():
    import fastfourierconvolution_amd  # noqa: F401
    from fastfourierconvolution_amd._lib import FFCError
    ops = torch.ops.ffc
    B, C, H, W = 2, 16, 4, 4
    N, d = H * W, 2
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    x, qkv, gamma, L, o = z(B, C, H, W), z(B, 2 * d + C, H, W), z(1), z(B, N), z(B, C, N)
    y, L1, o1 = ops.self_attn(x, qkv, gamma, True)
    assert tuple(L1.shape) == (B, N) and tuple(o1.shape) == (B, C, N) and torch.equal(y, x)
    assert tuple(ops.self_attn_matrix(qkv, L, C).shape) == (B, N, N)
    dqkv, dgamma = ops.self_attn_bwd(x, qkv, o, L, gamma)
    assert tuple(dqkv.shape) == tuple(qkv.shape) and tuple(dgamma.shape) == (1,)
    with pytest.raises(RuntimeError, match=r"gamma.*\(2,\)"):
        ops.self_attn(x, qkv, z(2), True)
    for bad_C in (8, 24, 64):            # 2 (C // 8) + C != 20
        with pytest.raises(RuntimeError, match=r"\(2, 20, 4, 4\)"):
            ops.self_attn_matrix(qkv, L, bad_C)
    with pytest.raises(NotImplementedError, match="unsupported"):
        ops.self_attn_matrix(z(B, 15, H, W), L, 12)
    with pytest.raises(NotImplementedError, match="unsupported"):
        ops.self_attn_matrix(z(B, 0, H, W), L, 0)
    with pytest.raises(RuntimeError, match="4-D|B, 2d"):
        ops.self_attn_matrix(z(B, 2 * d + C, N), L, C)
    for bad_L in (z(B, N - 1), z(B * N), z(B, N, 1), z(B + 1, N)):
        with pytest.raises(RuntimeError, match=r"L must be \(2, 16\)"):
            ops.self_attn_matrix(qkv, bad_L, C)
        with pytest.raises(RuntimeError, match=r"L must be \(2, 16\)"):
            ops.self_attn_bwd(x, qkv, o, bad_L, gamma)
    with pytest.raises(FFCError, match="fp32"):
        ops.self_attn_matrix(qkv, L.double(), C)
    with pytest.raises(FFCError, match="no CPU fallback"):
        ops.self_attn_matrix(qkv, L.cpu(), C)
    for n, bad in (("L", L.double()), ("o", o.double()), ("gamma", gamma.double())):
        a = dict(o=o, L=L, gamma=gamma)
        a[n] = bad
        with pytest.raises(FFCError, match=n + ": fp32"):
            ops.self_attn_bwd(x, qkv, a["o"], a["L"], a["gamma"])
    with pytest.raises(FFCError, match="no CPU fallback"):
        ops.self_attn_bwd(x, qkv, o, L, gamma.cpu())
    with pytest.raises(RuntimeError, match=r"gamma.*\(3,\)"):
        ops.self_attn_bwd(x, qkv, o, L, z(3))
    with pytest.raises(RuntimeError, match="without save"):
        ops.self_attn_bwd(x, qkv, z(0), L, gamma)
    print("OBS wrappers: every wrong C, L, o and gamma refused before a launch")
