"""Kernel-level parity of csrc/sn_kernels.hip: ffc_sn_forward, ffc_sn_backward and ffc_sn_ws_bytes called through
the C ABI with raw pointers against the float64 references of tests/sn_refs.py, elementwise.
tests/test_gpu_sn.py, which goes through the ops with one normwise bound per tensor, stays as it is.

Every output and the workspace is prefilled with NaN and has 64 NaN floats behind it: after a call every element
in range is finite and every other float -- the gaps between job workspaces, the partials a mode does not write
(pa and psq in eval mode, pdot in the forward) and each job's padding included -- is still NaN; after a rejection
everything is still NaN.  Misaligned pointers start one float into a larger live allocation.  Device copies stay
alive until the test ends.

Bounds (sn_refs, TOL = 1e-5 times the float64 sum of the absolute terms of each quantity; test_sn_refs_cpu.py
proves that plain fp32 stays under a quarter of each on every input used here and that eleven planted defects
exceed them)
  p = Wm^T u    read back from the pa partials; scale sum_m |Wm| |u|
  t             the sum of the pb partials against Wm p at the p the GPU produced; scale sum_k |Wm| |p|
  u', v'        against float64 throughout; the scales above over the float64 norm
  sigma         scale sum |u'_m| |t_m|
  W             bit-equal to fl(w_orig / sigma) at the sigma the GPU returned: build.py compiles with -O3 and no
                fast-math flag, for which hipcc's documented default (-fhip-fp32-correctly-rounded-divide-sqrt) is a
                correctly rounded fp32 division; the device code of sn_scale_kernel holds the v_div_scale /
                v_div_fmas / v_div_fixup sequence and no bare reciprocal.  So equality, not a bound.
  dw_orig       at the GPU's own (u', v', sigma): scale |dw / sigma| + |c u_m v_k|; end to end:
                |dw / sigma| + |c| su_m sv_k with su, sv the scales of u', v' (sn_refs.backward_shares)
  bit equality  torch.equal: the second call, each calling form, any table order, table against single

Weights are N(0, 0.02), u and v normalised N(0, 1); the gradient is noise + lambda w_orig with lambda chosen so
that the rank-one term's median share is at least 0.1 (asserted in test_sn_refs_cpu.py).

Case (shape, dim) -> (M, K, R): what it is there for
  (5,7,3,3) 1 -> 7, 45, 9      the smallest dim-1 scalar form: sn_col / sn_mk with R != K
  (66,3,3,3) 1 -> 3, 594, 9    the baseline generators' 3x3 transposed head: M = 3, many runs of R
  (19,65,3,3) 1 -> 65, 171, 9  two row chunks; M K % 4 != 0: sn_bwd_apply's float4 crosses rows, then a scalar tail
  (8,20,2,2) 1 -> 20, 32, 4    the smallest dim-1 vector form
  17x64 16x65 65x256 64x260 257x64   edges of SN_RB, SN_RA, the 64- and 256-column colsum tiles, the thread stride
  1000x3 3x1000                the step loops over u and v with one chunk
  8x2048 8x2049 8x2052         one and two matvec column tiles, vector and scalar
  127x129 128x128 1x16385 4x4097     M K = 16383, 16384, 16385, 16388
  1x1 1x4 4x1                  u' or v' is +-1 exactly, sigma = ||w||
  forms      at (19,65,3,3), (8,20,2,2), 64x260: w_orig, w, dw, dw_orig one float off, one at a time (vec / evec
             off); u_save = v_save = NULL; the backward through u_save / v_save with u / v pointing at NaN
  workspace  permuted ws_off with 16-byte NaN gaps
  tables     all 21 jobs in one table (two SnTables), reversed, and each alone: bit-equal; a 17-job table whose
             17th job is invalid writes nothing
  directed   rank-one w_orig with u parallel to a; w_orig times 2^40 and 2^-40 (unit-variance weights: see
             sn_refs.scaled_case)
  rejections every message of sn_build and of the two entry points

Observed on the first MI355X run (this file and tests/test_gpu_aw_abi.py together: 51 tests in 3.3 s, every one
passing, the slowest -- the 258-chunk pair of the aw file -- 0.5 s; here 31 tests, the slowest 0.4 s, the first,
which loads the library), as the largest share of each bound:
  p 0.015 (4x4097)   t 0.011 (rank-one)   v' 0.018 (rank-one)   u' 0.071 (1000x3)   sigma 0.017 (8x2049, eval)
  dw_orig at own (u', v', sigma) 0.015 (8x2052)   dw_orig end to end 0.023 (rank-one)
  W        bit-equal to fl(w_orig / sigma) on every case, training and eval: the correctly rounded division held
  equal    every bit-equality held: the second call, the four misalignments with NULL saves and the redirect at the
           three shapes, permuted offsets, the 21-job table against its reverse and each job alone, the 2^+-40
           scalings; 36 wrong tables refused with nothing written
One defect was found and fixed in sn_kernels.hip: with R % 4 == 0 a w_orig off 16-byte alignment took
sn_matvec_kernel's one-column-per-lane loop, whose summation order is not the float4 form's, and sn_dot_kernel's
strided loop likewise, so u', sigma, W and dw_orig changed in their last bits with the alignment ((8,20,2,2): W
differed; 64x260: u' differed).  Both 4-byte forms now add in the float4 form's order.  Aligned tensors take the
code they took before.
"""
import pytest
import torch

import abi_bufs as B
import sn_refs as R
from abi_bufs import Buf

pytestmark = pytest.mark.gpu
NANBITS = int(torch.tensor(B.NAN).view(torch.int32))


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    B.end_of_test()


def _sizes(M, K):
    nra, ncb, nchunk = -(-M // R.RA), -(-K // R.CB), -(-(M * K) // R.EC)
    pdot = 8 * ncb
    pa = pdot + 8 * nchunk
    pb = pa + 4 * nra * K
    return dict(nra=nra, ncb=ncb, nchunk=nchunk, psq=0, pdot=pdot, pa=pa, pb=pb, end=pb + 4 * ncb * M,
                total=(pb + 4 * ncb * M + 15) & ~15)


class _Job:
    def __init__(self, c, mis=(), save=True):
        self.c = c
        n, M, K = c["M"] * c["K"], c["M"], c["K"]
        self.w_orig = Buf(n, fill=c["w"], mis="w_orig" in mis)
        self.u, self.v = Buf(M, fill=c["u"]), Buf(K, fill=c["v"])
        self.w, self.sigma = Buf(n, mis="w" in mis), Buf(1)
        self.us, self.vs = (Buf(M), Buf(K)) if save else (None, None)
        self.dw, self.dwo = Buf(n, fill=c["g"], mis="dw" in mis), Buf(n, mis="dw_orig" in mis)
        self.nan_u, self.nan_v = Buf(M), Buf(K)

    def outputs(self):
        return [b for b in (self.w, self.sigma, self.us, self.vs, self.dwo) if b is not None]


class _Table:
    """jobs of the cases ``cs`` in one table; workspaces placed in ``order`` with ``gap`` bytes between and behind"""

    def __init__(self, cs, mis=(), save=True, order=None, gap=0):
        from fastfourierconvolution_amd import _lib
        L = B.lib()
        self.cs, self.n = cs, len(cs)
        self.jobs = [_Job(c, mis, save) for c in cs]
        self.sz = [_sizes(c["M"], c["K"]) for c in cs]
        for c, s in zip(cs, self.sz):
            assert L.ffc_sn_ws_bytes(c["M"], c["K"]) == s["total"], c["name"]
        self.off, pos = [0] * self.n, 0
        for i in (order if order is not None else range(self.n)):
            self.off[i] = pos
            pos += self.sz[i]["total"] + gap
        self.ws_bytes = pos
        self.ws = Buf(pos // 4)
        self.written = torch.zeros(pos // 4, dtype=torch.bool)
        self.arr = (_lib.SnJob * self.n)()
        for a, j, c, off in zip(self.arr, self.jobs, cs, self.off):
            a.w_orig, a.u, a.v, a.w, a.sigma = j.w_orig.ptr(), j.u.ptr(), j.v.ptr(), j.w.ptr(), j.sigma.ptr()
            a.u_save, a.v_save = (j.us.ptr(), j.vs.ptr()) if save else (None, None)
            a.dw, a.dw_orig = j.dw.ptr(), j.dwo.ptr()
            a.M, a.K, a.R, a.stride_m, a.stride_i, a.ws_off = c["M"], c["K"], c["R"], c["stride_m"], c["stride_i"], off

    def _mark(self, i, *regions):
        s = self.sz[i]
        ends = dict(psq="pdot", pdot="pa", pa="pb", pb="end")
        for r in regions:
            self.written[(self.off[i] + s[r]) // 4:(self.off[i] + s[ends[r]]) // 4] = True

    def forward(self, training):
        B.ok(B.lib().ffc_sn_forward(self.arr, self.n, 1 if training else 0, self.ws.ptr(), self.ws_bytes, B.stream()),
             "ffc_sn_forward")
        for i in range(self.n):
            self._mark(i, *(("psq", "pa", "pb") if training else ("pb",)))
        return self

    def backward(self, redirect=False):
        """redirect: u / v point at NaN and the saved copies are given; otherwise u / v hold this call's vectors"""
        for a, j in zip(self.arr, self.jobs):
            a.u, a.v = (j.nan_u.ptr(), j.nan_v.ptr()) if redirect else (j.u.ptr(), j.v.ptr())
            a.u_save, a.v_save = (j.us.ptr(), j.vs.ptr()) if redirect else (None, None)
        B.ok(B.lib().ffc_sn_backward(self.arr, self.n, self.ws.ptr(), self.ws_bytes, B.stream()), "ffc_sn_backward")
        for i in range(self.n):
            self._mark(i, "pdot")
        return self

    def ws_words(self):
        """the workspace as int32 words: exactly the regions the calls so far must write differ from the prefill"""
        torch.cuda.synchronize()
        words = self.ws.buf.cpu().view(torch.int32)
        inside = words[self.ws.off:self.ws.off + self.ws.n]
        touched = inside != NANBITS
        assert torch.equal(touched, self.written), (
            f"workspace: {int((touched & ~self.written).sum())} words written outside the partials, "
            f"{int((~touched & self.written).sum())} words of the partials unwritten")
        assert int((words != NANBITS).sum()) == int(touched.sum()), "wrote in front of or behind the workspace"
        return inside

    def read(self, i, training, backward=False):
        """the results of job i on the CPU, every guard checked"""
        j, c, s = self.jobs[i], self.cs[i], self.sz[i]
        M, K = c["M"], c["K"]
        words = self.ws_words()
        out = dict(w=j.w.get("w").reshape(c["shape"]), u=j.u.get("u"), v=j.v.get("v"), sigma=j.sigma.get("sigma"))
        if j.us is not None:
            out.update(us=j.us.get("u_save"), vs=j.vs.get("v_save"))
        f = words.view(torch.float32)
        o = self.off[i] // 4
        pb = f[o + s["pb"] // 4:o + s["end"] // 4].reshape(s["ncb"], M)
        out["tb"] = pb.double().sum(0).float()
        if training:
            pa = f[o + s["pa"] // 4:o + s["pb"] // 4].reshape(s["nra"], K)
            out["p"] = pa.double().sum(0).float()
            psq = words[o:o + s["pdot"] // 4].clone().view(torch.float64)
            assert bool(torch.isfinite(pa).all() and torch.isfinite(pb).all() and torch.isfinite(psq).all())
        if backward:
            out["dw_orig"] = j.dwo.get("dw_orig").reshape(c["shape"])
            pdot = words[o + s["pdot"] // 4:o + s["pa"] // 4].clone().view(torch.float64)
            assert bool(torch.isfinite(pdot).all())
            out["pdot"] = pdot.clone()
        else:
            assert j.dwo.untouched()
        return out

    def nothing_written(self):
        return self.ws.untouched() and all(b.untouched() for j in self.jobs for b in j.outputs())


def _report(what, sh):
    print(f"OBS {what} " + " ".join(f"{k} {v:.3f}" for k, v in sh.items()))
    bad = {k: v for k, v in sh.items() if not v <= 1.0}
    assert not bad, (what, bad)


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


def _train_and_back(c, **kw):
    """training forward, checked; backward, checked -> (forward results, backward results)"""
    t = _Table([c], **{k: v for k, v in kw.items() if k != "redirect"})
    fw = t.forward(True).read(0, True)
    bw = t.backward(redirect=kw.get("redirect", False)).read(0, True, backward=True)
    return fw, bw


def _check_train(c, fw, bw):
    sh = R.forward_shares(c, fw, True)
    sh.update(R.backward_shares(c, bw["dw_orig"], fw["u"], fw["v"], fw["sigma"]))
    bad = R.w_exact(c, fw["w"], fw["sigma"])
    assert bad == 0, f"{c['name']}: {bad} elements of W are not fl(w_orig / sigma)"
    assert torch.equal(fw["us"], fw["u"]) and torch.equal(fw["vs"], fw["v"]), "the saved copies are not this call's u', v'"
    for k in ("w", "u", "v", "sigma", "us", "vs"):      # the backward writes none of the forward's outputs
        assert torch.equal(bw[k], fw[k]), k
    _report(c["name"], sh)


# --------------------------------------------------------------------------- every kernel against float64
@pytest.mark.parametrize("name", R.ABI_NAMES)
def test_case_matches_fp64(name):
    c = R.abi_case(name)
    fw, bw = _train_and_back(c)
    _check_train(c, fw, bw)
    fw2, bw2 = _train_and_back(c)
    _same(fw2, fw, "the forward run twice")
    _same(bw2, bw, "the backward run twice")
    ev = _Table([c]).forward(False).read(0, False)      # read() proves that pa and psq stayed NaN
    assert torch.equal(ev["u"], c["u"]) and torch.equal(ev["v"], c["v"]), "eval mode wrote u or v"
    assert torch.equal(ev["us"], c["u"]) and torch.equal(ev["vs"], c["v"]), "eval mode saves the stored vectors"
    assert R.w_exact(c, ev["w"], ev["sigma"]) == 0
    _report(name + " eval", R.forward_shares(c, ev, False))
    _same(_Table([c]).forward(False).read(0, False), ev, "the eval forward run twice")
    if c["M"] == 1:
        assert abs(float(fw["u"][0])) == 1.0
    if c["K"] == 1:
        assert abs(float(fw["v"][0])) == 1.0


# --------------------------------------------------------------------------- calling forms
@pytest.mark.parametrize("name", R.FORMS)
def test_calling_forms_are_bit_equal_to_the_plain_call(name):
    c = R.abi_case(name)
    fw, bw = _train_and_back(c)
    _check_train(c, fw, bw)
    ev = _Table([c]).forward(False).read(0, False)
    for which in ("w_orig", "w", "dw", "dw_orig"):
        f2, b2 = _train_and_back(c, mis=(which,))
        _same(f2, fw, f"{name} {which} one float off, forward")
        _same(b2, bw, f"{name} {which} one float off, backward")
        _same(_Table([c], mis=(which,)).forward(False).read(0, False), ev, f"{name} {which} one float off, eval")
    f2, b2 = _train_and_back(c, save=False)
    for k in f2:
        assert torch.equal(f2[k], fw[k]), f"{name} u_save = v_save = NULL: {k}"
    assert torch.equal(b2["dw_orig"], bw["dw_orig"])
    f2, b2 = _train_and_back(c, redirect=True)
    _same(f2, fw, f"{name} forward before the redirected backward")
    assert torch.equal(b2["dw_orig"], bw["dw_orig"]) and torch.equal(b2["pdot"], bw["pdot"]), "backward through u_save / v_save"
    print(f"OBS forms {name}: four misalignments (forward, eval, backward), NULL saves and the redirect bit-equal")


def test_w_orig_off_alignment_takes_the_scalar_rows_of_the_vector_case():
    """(8,20,2,2): R % 4 == 0, so only the alignment turns vec off; still within every bound"""
    c = R.abi_case("T8x20x2x2")
    fw, bw = _train_and_back(c, mis=("w_orig",))
    _check_train(c, fw, bw)


# --------------------------------------------------------------------------- workspace layout and tables
def _table_results(cs, **kw):
    t = _Table(cs, **kw)
    t.forward(True)
    fw = [t.read(i, True) for i in range(len(cs))]
    t.backward()
    bw = [t.read(i, True, backward=True) for i in range(len(cs))]
    return fw, bw


def test_permuted_workspace_offsets_with_gaps():
    names = ["T19x65x3x3", "8x2049", "1x1", "257x64", "T8x20x2x2"]
    cs = [R.abi_case(n) for n in names]
    fw, bw = _table_results(cs)
    fw2, bw2 = _table_results(cs, order=[3, 0, 4, 2, 1], gap=16)      # read() proves the gaps and the tail stay NaN
    for i, n in enumerate(names):
        _same(fw2[i], fw[i], f"{n} forward at a permuted ws_off")
        _same(bw2[i], bw[i], f"{n} backward at a permuted ws_off")
    print("OBS workspace: five jobs at permuted offsets with 16-byte gaps bit-equal, gaps and tail still NaN")


def test_tables_of_more_than_16_jobs():
    cs = [R.abi_case(n) for n in R.ABI_NAMES]
    assert len(cs) > R.MAX_JOBS
    fw, bw = _table_results(cs)
    rfw, rbw = _table_results(cs[::-1])
    for i, c in enumerate(cs):
        f1, b1 = _train_and_back(c)
        _same(fw[i], f1, f"{c['name']} in the table against alone, forward")
        _same(bw[i], b1, f"{c['name']} in the table against alone, backward")
        _same(rfw[len(cs) - 1 - i], f1, f"{c['name']} in the reversed table, forward")
        _same(rbw[len(cs) - 1 - i], b1, f"{c['name']} in the reversed table, backward")
    print(f"OBS tables: {len(cs)} jobs in one table, reversed and alone bit-equal, forward and backward")


def test_a_17th_invalid_job_rejects_the_whole_table_before_any_launch():
    L = B.lib()
    cs = [R.abi_case(n) for n in R.ABI_NAMES[:17]]
    for field, value, word in (("M", 0, "M, K must be positive"), ("w", None, "null tensor pointer")):
        t = _Table(cs)
        setattr(t.arr[16], field, value)
        B.rejected(L.ffc_sn_forward(t.arr, 17, 1, t.ws.ptr(), t.ws_bytes, B.stream()), "ffc_sn_forward", word)
        assert t.nothing_written(), "the first 16 jobs ran"
        for j, c in zip(t.jobs, cs):
            assert torch.equal(j.u.raw(), c["u"]) and torch.equal(j.v.raw(), c["v"])
    t = _Table(cs)
    t.arr[16].dw = None
    B.rejected(L.ffc_sn_backward(t.arr, 17, t.ws.ptr(), t.ws_bytes, B.stream()), "ffc_sn_backward", "null tensor pointer")
    assert t.nothing_written()


# --------------------------------------------------------------------------- directed
def test_rank_one_weight_is_at_its_fixed_point():
    c = R.rank_one_case()
    fw, bw = _train_and_back(c)
    _check_train(c, fw, bw)
    a, b = c["a"].double(), c["b"].double()
    na, nb = float(a.norm()), float(b.norm())
    sh = dict(sigma=R._share(fw["sigma"], na * nb, na * nb))
    su, sv = float(torch.sign(fw["u"][0].double() * a[0])), float(torch.sign(fw["v"][0].double() * b[0]))
    sh["u"] = R._share(fw["u"], su * a / na, a.abs() / na)
    sh["v"] = R._share(fw["v"], sv * b / nb, b.abs() / nb)
    _report("rank_one against ||a|| ||b||, a / ||a||, b / ||b||", sh)


def test_power_of_two_scaling_is_exact():
    base = _Table([R.scaled_case(0)]).forward(True).read(0, True)
    for e in (40, -40):
        got = _Table([R.scaled_case(e)]).forward(True).read(0, True)
        assert torch.equal(got["u"], base["u"]) and torch.equal(got["v"], base["v"]), f"2^{e}: u' or v' changed"
        assert float(got["sigma"][0]) == float(base["sigma"][0]) * 2.0 ** e, f"2^{e}: sigma"
        assert torch.equal(got["w"], base["w"]), f"2^{e}: W = w_orig / sigma changed"
    print(f"OBS scaling: u', v', W bit-equal and sigma scaled exactly at 2^40 and 2^-40 (sigma {float(base['sigma'][0]):.4f})")


# --------------------------------------------------------------------------- rejections
def test_rejections_write_nothing():
    L = B.lib()
    cT, c0 = R.abi_case("T19x65x3x3"), R.abi_case("64x260")
    count = 0

    def both(c, word, mutate=None, n=1, jobs=True, ws="ok", ws_bytes=None, fwd=True, bwd=True):
        nonlocal count
        t = _Table([c], gap=16)
        if mutate:
            mutate(t.arr[0], t)
        arr = t.arr if jobs else None
        wsp = dict(ok=t.ws.ptr(), null=None, eight=t.ws.ptr() + 8)[ws]
        nbytes = t.ws_bytes if ws_bytes is None else ws_bytes(t)
        if fwd:
            B.rejected(L.ffc_sn_forward(arr, n, 1, wsp, nbytes, B.stream()), "ffc_sn_forward", word)
            B.rejected(L.ffc_sn_forward(arr, n, 0, wsp, nbytes, B.stream()), "ffc_sn_forward", word)
        if bwd:
            B.rejected(L.ffc_sn_backward(arr, n, wsp, nbytes, B.stream()), "ffc_sn_backward", word)
        assert t.nothing_written(), word
        assert torch.equal(t.jobs[0].u.raw(), c["u"]) and torch.equal(t.jobs[0].v.raw(), c["v"]), word
        count += 1

    def put(**kw):
        def f(a, t):
            for k, v in kw.items():
                setattr(a, k, v(t) if callable(v) else v)
        return f

    both(c0, "n >= 1", n=0)
    both(c0, "n >= 1", n=-1)
    both(c0, "n >= 1", jobs=False)
    both(c0, "null workspace", ws="null")
    both(c0, "16-byte aligned", ws="eight")
    for c in (c0, cT):
        for field in ("M", "K"):
            for bad in (0, -1):
                both(c, "M, K must be positive", put(**{field: bad}))
    for field in ("w_orig", "u", "v", "sigma"):
        both(cT, "null tensor pointer", put(**{field: None}))
    both(cT, "null tensor pointer", put(w=None), bwd=False)
    both(cT, "null tensor pointer", put(dw=None), fwd=False)
    both(cT, "null tensor pointer", put(dw_orig=None), fwd=False)
    both(c0, "w must not be w_orig", put(w=lambda t: t.jobs[0].w_orig.ptr()), bwd=False)
    both(c0, "go together", put(u_save=None), bwd=False)
    both(c0, "go together", put(v_save=None), bwd=False)
    both(c0, "unsupported matrix view", put(stride_m=c0["K"] + 1))
    both(cT, "unsupported matrix view", put(stride_m=cT["R"] + 1))
    both(cT, "unsupported matrix view", put(R=10))                                  # 171 % 10 != 0
    both(cT, "unsupported matrix view", put(R=0))
    both(cT, "unsupported matrix view", put(stride_i=cT["stride_i"] + 1))
    both(cT, "unsupported matrix view", put(stride_i=0))
    both(c0, "workspace too small", put(ws_off=-16))
    both(c0, "workspace too small", put(ws_off=4))
    both(c0, "workspace too small", put(ws_off=8))
    both(c0, "workspace too small", put(ws_off=lambda t: t.ws_bytes + 16))
    both(c0, "workspace too small", ws_bytes=lambda t: t.sz[0]["total"] - 1)
    both(cT, "workspace too small", ws_bytes=lambda t: t.sz[0]["total"] - 1)
    # M K = 2^31: no workspace size, and the call is refused on small real buffers
    assert L.ffc_sn_ws_bytes(65536, 32768) == 0 and L.ffc_sn_ws_bytes(32768, 65535) > 0
    for M, K in ((0, 4), (4, 0), (-1, 4), (4, -1), (46341, 46341)):
        assert L.ffc_sn_ws_bytes(M, K) == 0, (M, K)
    both(c0, "M, K must be positive", put(M=65536, K=32768, R=32768, stride_m=32768))
    # the same operands are accepted as they are
    t = _Table([c0], gap=16)
    fw = t.forward(True).read(0, True)
    _same(fw, _Table([c0]).forward(True).read(0, True), "after the rejections")
    print(f"OBS rejections: {count} wrong tables refused by name with nothing written")
