"""Kernel-level parity of csrc/aw_kernels.hip: ffc_aw_weights, ffc_aw_combine and ffc_aw_ws_doubles called through
the C ABI with raw pointers against the float64 references of tests/aw_refs.py.  tests/test_gpu_aw.py, which goes
through the ops, stays as it is.

stats, the workspace and every out are prefilled with NaN and have 64 NaN elements behind them: after a call every
element in range is finite and every other one -- the doubles of ws behind 3 per chunk included -- is still NaN;
after a rejection everything is still NaN.  Misaligned pointers start one float into a larger live allocation.

Bounds (aw_refs.abi_shares; test_aw_refs_cpu.py proves that a restatement of the kernels' arithmetic stays under a
quarter of each on these inputs and that five planted defects exceed them)
  partials, rr, ff, rf   TOL_STAT = 1e-15 times the sum of |x y| over the same terms, against correctly rounded sums
  rs, fs                 TOL_STAT, scale 1
  w_r, w_f               against aw_refs.weights at the GPU's own stats (scale |w - eps| + |eps|) and, away from a
                         tie, end to end with the dots' own bounds carried along
  out                    TOL_OUT = 1e-6 times |w_r g_r| + |w_f g_f| against float32(w_r) g_r + float32(w_f) g_f
  bit equality           torch.equal: every launch split, every alignment, empty pairs, one tensor against its chunks

Inputs -> what they are there for
  five cases x two algorithms   the list of numel 0, 1, 3, 4, 5, 255, 256, 257, 16383, 16384, 16385, 32770; the case
                                driven by the logits and by g_fake = +-g_real + noise
  launch split                  jobs_per_launch 1, 2, 15, 16 and 0, -1, 17 (= 16); 40 small pairs at the default
  alignment                     g_real, g_fake, out one float off, one at a time and together
  empty pairs                   NULL pointers for numel = 0, first, last and interleaved; an all-empty list
  merge stride                  one pair of 257 x 16384 + 1 elements (258 chunks) against 258 tensors of one chunk
  logits                        n_real 1, 255, 256, 257 with another n_fake; logits at +-100
  ties                          rs = alpha1; rs = fs - delta; rf = 0 on disjoint supports
  rejections                    every message of the two entry points and of aw_collect.  "ws_doubles one short" is
                                one short of the 3 per chunk the kernels write: the entry point checks that, and the
                                one spare double of ffc_aw_ws_doubles (there so that the size is never 0) is neither
                                required nor touched

Observed on the first MI355X run (20 tests of the 51 the two ABI files ran in 3.3 s, every one passing, the slowest
the 258-chunk pair at 0.5 s; no line of aw_kernels.hip had to change), as the largest share of each bound:
  partials 0.21 and rr 0.17 (40 pairs)   ff 0.16 (258 chunks)   rf 0.17   rs 0.056 (logit counts)   fs 0
  weights at the GPU's own stats 0 (bit-equal to aw_refs.weights)   weights end to end 0.042   out 0.11
  equal    every bit-equality held: seven launch splits on 12 pairs and three on 40, four alignments, NULL empty
           pairs, 258 chunks against 258 tensors; the per-chunk partials were bit-equal to aw_refs.partials, the
           restated tree, on all ten case inputs; the three ties were exact (rs = 0.5, fs = 0.75, rf = 0.0);
           28 wrong calls refused with nothing written
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import abi_bufs as B
import aw_refs as A
from abi_bufs import Buf

pytestmark = pytest.mark.gpu
F64 = torch.float64


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    B.end_of_test()


def _kwargs(kw):
    return (kw["alpha1"], kw["alpha2"], kw["delta"], kw["epsilon"], 1 if kw["normalized"] else 0)


class _List:
    """device operands of one gradient list; mis: which of g_real, g_fake, out start one float off alignment;
    empty pairs get NULL pointers"""

    def __init__(self, a, b, real, fake, mis=()):
        self.a, self.b, self.n = a, b, len(a)
        self.gr = [Buf(x.size, fill=x, mis="g_real" in mis) for x in a]
        self.gf = [Buf(x.size, fill=x, mis="g_fake" in mis) for x in b]
        self.out = [Buf(x.size, mis="out" in mis) for x in a]
        arr = lambda bufs: (ctypes.c_void_p * self.n)(*[q.ptr() if q.n else None for q in bufs])   # noqa: E731
        self.pr, self.pf, self.po = arr(self.gr), arr(self.gf), arr(self.out)
        self.numel = (ctypes.c_longlong * self.n)(*[x.size for x in a])
        self.total = sum(-(-x.size // A.EC) for x in a)
        self.nws = B.lib().ffc_aw_ws_doubles(self.numel, self.n)
        assert self.nws == 3 * self.total + 1
        self.ws, self.stats = Buf(self.nws, dtype=F64), Buf(8, dtype=F64)
        self.real, self.fake = Buf(len(real), fill=real), Buf(len(fake), fill=fake)

    def weights(self, kw, per=0, **over):
        a = dict(pr=self.pr, pf=self.pf, numel=self.numel, n=self.n, real=self.real.ptr(), n_real=self.real.n,
                 fake=self.fake.ptr(), n_fake=self.fake.n, ws=self.ws.ptr(), nws=self.nws, stats=self.stats.ptr())
        a.update(over)
        return B.lib().ffc_aw_weights(a["pr"], a["pf"], a["numel"], a["n"], a["real"], a["n_real"], a["fake"], a["n_fake"],
                                      *_kwargs(kw), per, a["ws"], a["nws"], a["stats"], B.stream())

    def combine(self, per=0, **over):
        a = dict(pr=self.pr, pf=self.pf, po=self.po, numel=self.numel, n=self.n, stats=self.stats.ptr())
        a.update(over)
        return B.lib().ffc_aw_combine(a["pr"], a["pf"], a["po"], a["numel"], a["n"], a["stats"], per, B.stream())

    def parts(self):
        """the 3 per chunk partials; the doubles behind them and around ws still NaN"""
        torch.cuda.synchronize()
        data = self.ws.buf.cpu()
        inside = data[self.ws.off:self.ws.off + 3 * self.total]
        assert bool(torch.isfinite(inside).all()), "ws: a partial is unwritten"
        assert int(torch.isnan(data).sum()) == data.numel() - 3 * self.total, "ws: wrote behind 3 * total"
        return inside.numpy().reshape(-1, 3).copy()

    def run(self, kw, per=0):
        B.ok(self.weights(kw, per), "ffc_aw_weights")
        B.ok(self.combine(per), "ffc_aw_combine")
        return dict(parts=self.parts(), stats=self.stats.get("stats").numpy(), out=[o.get("out").numpy() for o in self.out])

    def nothing_written(self):
        return self.ws.untouched() and self.stats.untouched() and all(o.untouched() for o in self.out)


def _run(a, b, real, fake, kw, per=0, mis=()):
    return _List(a, b, real, fake, mis).run(kw, per)


def _equal(x, y, what):
    assert np.array_equal(x["stats"], y["stats"]), f"{what}: stats differ"
    assert len(x["out"]) == len(y["out"]) and all(np.array_equal(p.view(np.int32), q.view(np.int32))
                                                  for p, q in zip(x["out"], y["out"])), f"{what}: out differs"


def _report(what, sh):
    print(f"OBS {what} " + " ".join(f"{k} {v:.3f}" for k, v in sh.items()))
    bad = {k: v for k, v in sh.items() if not v <= 1.0}
    assert not bad, (what, bad)


# --------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("case", [1, 2, 3, 4, 5])
def test_five_cases_match_fp64(case, normalized):
    kind, sign = A.FIVE[case]
    a, b = A.make_list(A.NUMELS, sign, case)
    real, fake = A.logits_for(kind)
    kw = dict(A.KW, normalized=normalized)
    got = _run(a, b, real, fake, kw)
    sh, e_case = A.abi_shares(a, b, real, fake, kw, got)
    assert int(got["stats"][7]) == case == e_case
    same = int(np.array_equal(got["parts"], A.partials(a, b)))
    _report(f"case {case} normalized={normalized} (partials bit-equal to the restated tree: {same})", sh)


# --------------------------------------------------------------------------- launch split
def test_results_do_not_depend_on_the_launch_split():
    a, b = A.make_list(A.NUMELS, -1.0, 1)
    real, fake = A.logits_for("low")
    base = _run(a, b, real, fake, A.KW)
    for per in (1, 2, 15, 16, 0, -1, 17):
        got = _run(a, b, real, fake, A.KW, per=per)
        _equal(got, base, f"jobs_per_launch = {per}")
        assert np.array_equal(got["parts"], base["parts"])
    a, b = A.make_list([1 + 7 * (i % 5) + (A.EC if i == 33 else 0) for i in range(40)], 1.0, 2)
    base = _run(a, b, real, fake, A.KW)
    sh, _ = A.abi_shares(a, b, real, fake, A.KW, base)
    _report("40 pairs at the default", sh)
    for per in (1, 7, 16):
        _equal(_run(a, b, real, fake, A.KW, per=per), base, f"40 pairs, jobs_per_launch = {per}")
    print("OBS split: 1, 2, 15, 16, 0, -1, 17 bit-equal on 12 pairs; 40 pairs at the default, 1, 7, 16 bit-equal")


# --------------------------------------------------------------------------- alignment
def test_results_do_not_depend_on_the_alignment():
    a, b = A.make_list(A.NUMELS, -1.0, 3)
    real, fake = A.logits_for("high")
    base = _run(a, b, real, fake, A.KW)
    for mis in (("g_real",), ("g_fake",), ("out",), ("g_real", "g_fake", "out")):
        got = _run(a, b, real, fake, A.KW, mis=mis)
        _equal(got, base, f"{mis} one float off")
        assert np.array_equal(got["parts"], base["parts"]), mis
    print("OBS alignment: g_real, g_fake, out one float off, one at a time and together: bit-equal")


# --------------------------------------------------------------------------- empty pairs
def test_empty_pairs_with_null_pointers_are_skipped():
    a, b = A.make_list((0, 5, 0, 0, A.EC + 1, 257, 0), 1.0, 4)
    real, fake = A.logits_for("mid")
    got = _run(a, b, real, fake, A.KW)
    keep = [i for i, x in enumerate(a) if x.size]
    ref = _run([a[i] for i in keep], [b[i] for i in keep], real, fake, A.KW)
    assert np.array_equal(got["stats"], ref["stats"]) and np.array_equal(got["parts"], ref["parts"])
    assert all(np.array_equal(got["out"][i], ref["out"][k]) for k, i in enumerate(keep))
    sh, _ = A.abi_shares(a, b, real, fake, A.KW, got)
    _report("empty pairs first, last and interleaved", sh)


def test_a_list_of_only_empty_pairs():
    z = [np.zeros(0, dtype=np.float32)] * 3
    for kind in ("low", "high", "mid"):
        real, fake = A.logits_for(kind)
        t = _List(z, z, real, fake)
        assert t.nws == 1
        B.ok(t.weights(A.KW), "ffc_aw_weights")
        s = t.stats.get("stats").numpy()
        assert t.ws.untouched(), "ws written without a chunk"
        assert s[0] == 1e-4 and s[1] == 1e-4 and s[2] == 0.0
        w_r, w_f, case = A.weights(s[0], s[1], s[2], s[3], s[4], **A.KW)
        assert int(s[7]) == case and case in (1, 3, 5)
        assert abs(s[5] - w_r) <= A.TOL_STAT * (abs(w_r - 0.05) + 0.05) and abs(s[6] - w_f) <= A.TOL_STAT * (abs(w_f - 0.05) + 0.05)
        B.ok(t.combine(), "ffc_aw_combine")
        assert all(o.untouched() for o in t.out)
        print(f"OBS all-empty list, {kind}: case {case} w_r {s[5]:.6f} w_f {s[6]:.6f}")


# --------------------------------------------------------------------------- the merge's thread stride
def test_258_chunks_of_one_tensor_equal_258_tensors():
    n = 257 * A.EC + 1
    a, b = A.make_list((n,), -1.0, 5)
    real, fake = A.logits_for("low")
    one = _run(a, b, real, fake, A.KW)
    assert one["parts"].shape == (258, 3)
    sh, _ = A.abi_shares(a, b, real, fake, A.KW, one)
    _report("one pair of 258 chunks", sh)
    many = _run(A.chunks_of(a[0]), A.chunks_of(b[0]), real, fake, A.KW)
    assert np.array_equal(many["parts"], one["parts"]) and np.array_equal(many["stats"], one["stats"])
    assert np.array_equal(np.concatenate(many["out"]), one["out"][0])
    print("OBS merge: 258 chunks of one tensor bit-equal to 258 tensors of one chunk")


# --------------------------------------------------------------------------- logits
def test_logit_counts_and_saturated_logits():
    a, b = A.make_list((5, 257), 1.0, 6)
    rng = np.random.default_rng(7)
    worst = {}
    for n_real, n_fake in ((1, 3), (255, 256), (256, 1), (257, 255), (3, 257)):
        real = rng.standard_normal(n_real).astype(np.float32)
        fake = (rng.standard_normal(n_fake) + 1.0).astype(np.float32)
        got = _run(a, b, real, fake, A.KW)
        sh, _ = A.abi_shares(a, b, real, fake, A.KW, got, tie=True)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in sh.items()}
    for real, fake in (([100.0, -100.0, 100.0], [-100.0] * 5), ([-100.0] * 257, [100.0, 100.0])):
        real, fake = np.array(real, dtype=np.float32), np.array(fake, dtype=np.float32)
        got = _run(a, b, real, fake, A.KW)
        assert np.isfinite(got["stats"]).all()
        sh, _ = A.abi_shares(a, b, real, fake, A.KW, got)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in sh.items()}
        print(f"OBS logits +-100: rs {got['stats'][3]:.3e} fs {got['stats'][4]:.3e} case {int(got['stats'][7])}")
    _report("n_real, n_fake in 1, 3, 255, 256, 257 and logits at +-100", worst)


# --------------------------------------------------------------------------- ties
@pytest.mark.parametrize("name", list(A.tie_cases()))
def test_ties_in_the_case_selection(name):
    a, b, real, fake, kw, case, _ = A.tie_cases()[name]
    got = _run(a, b, real, fake, kw)
    s = got["stats"]
    if name == "rf == 0":
        assert s[2] == 0.0 and (got["parts"][:, 2] == 0.0).all()
    else:
        assert s[3] == 0.5 and s[4] == (0.75 if name == "rs == fs - delta" else 0.5), (s[3], s[4])
    assert int(s[7]) == case, f"{name}: case {int(s[7])}, expected {case}"
    sh, _ = A.abi_shares(a, b, real, fake, kw, got, tie=True)
    _report(f"tie {name}: case {int(s[7])}", sh)


# --------------------------------------------------------------------------- rejections
def test_rejections_write_nothing():
    a, b = A.make_list((5, 0, 257, A.EC + 3), 1.0, 8)
    real, fake = A.logits_for("low")
    count = 0

    def w(word, kw=A.KW, **over):
        nonlocal count
        t = _List(a, b, real, fake)
        B.rejected(t.weights(kw, **over), "ffc_aw_weights", word)
        assert t.nothing_written(), word
        count += 1

    def c(word, **over):
        nonlocal count
        t = _List(a, b, real, fake)
        B.ok(t.weights(A.KW), "ffc_aw_weights")
        over = {k: v(t) if callable(v) else v for k, v in over.items()}
        B.rejected(t.combine(**over), "ffc_aw_combine", word)
        assert all(o.untouched() for o in t.out), word
        for g, x in zip(t.gr + t.gf, a + b):
            assert np.array_equal(g.raw().numpy(), x), "a rejected call changed an input"
        count += 1

    def ptrs(t, which, i, value):
        arr = (ctypes.c_void_p * t.n)(*[q.ptr() if q.n else None for q in getattr(t, which)])
        arr[i] = value
        return arr

    probe = _List(a, b, real, fake)
    w("alpha1 < alpha2", kw=dict(A.KW, alpha1=0.75))
    w("alpha1 < alpha2", kw=dict(A.KW, alpha1=0.8))
    w("at least one element", n_real=0)
    w("at least one element", n_fake=0)
    w("at least one element", real=None)
    w("at least one element", fake=None)
    for k in ("pr", "pf", "numel"):
        w("n >= 1", **{k: None})
    w("n >= 1", n=0)
    w("null workspace or stats", ws=None)
    w("null workspace or stats", stats=None)
    w("null tensor pointer", pr=ptrs(probe, "gr", 2, None))
    w("null tensor pointer", pf=ptrs(probe, "gf", 0, None))
    w("negative numel", numel=(ctypes.c_longlong * 4)(5, -1, 257, A.EC + 3))
    w("workspace too small", nws=3 * probe.total - 1)
    for k in ("pr", "pf", "po", "numel"):
        c("n >= 1", **{k: None})
    c("n >= 1", n=0)
    c("null stats", stats=None)
    c("null tensor pointer", po=lambda t: ptrs(t, "out", 3, None))
    c("negative numel", numel=(ctypes.c_longlong * 4)(5, -1, 257, A.EC + 3))
    c("alias", po=lambda t: ptrs(t, "out", 0, t.gr[0].ptr()))                    # out == g_real
    c("alias", po=lambda t: ptrs(t, "out", 2, t.gf[2].ptr()))                    # out == g_fake
    # out overlapping g_real by one element, both inside one allocation: out = [0, n), g_real = [n - 1, 2n - 1)
    n = a[2].size
    both = Buf(2 * n - 1, fill=np.concatenate([np.full(n - 1, 7.0, dtype=np.float32), a[2]]))
    before = both.raw()
    t = _List(a, b, real, fake)
    B.ok(t.weights(A.KW), "ffc_aw_weights")
    B.rejected(t.combine(pr=ptrs(t, "gr", 2, both.ptr(n - 1)), po=ptrs(t, "out", 2, both.ptr())), "ffc_aw_combine", "alias")
    assert torch.equal(both.raw(), before) and all(o.untouched() for o in t.out)
    for g, x in zip(t.gr + t.gf, a + b):
        assert np.array_equal(g.raw().numpy(), x), "a rejected call changed an input"
    # the same operands are accepted as they are
    got = t.run(A.KW)
    sh, _ = A.abi_shares(a, b, real, fake, A.KW, got)
    _report(f"after {count + 1} rejections", sh)
    assert math.isfinite(sum(sh.values()))
