"""fp64 restatement of aw_method.aw_loss (layers/aw_loss.py:13-107) from the point where the two
gradient lists exist: the dots, the two scores, the case of Algorithm 1 (normalized) / Algorithm 2 and
the combined gradients.  The three dots are correctly rounded (math.fsum over products of values that
came from fp32, which are exact in fp64), so a test's bound on a kernel's sums is a bound on the
kernel alone."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATS = ("rr", "ff", "rf", "rs", "fs", "w_r", "w_f", "case")
U = 2.0 ** -53


def _np64(t):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def dots(g_real, g_fake):
    """-> (sum g_r^2, sum g_f^2, sum g_r g_f, sum |g_r g_f|, element count) over the lists"""
    a = np.concatenate([_np64(g).reshape(-1) for g in g_real]) if len(g_real) else np.zeros(0)
    b = np.concatenate([_np64(g).reshape(-1) for g in g_fake]) if len(g_fake) else np.zeros(0)
    assert a.shape == b.shape
    return (math.fsum((a * a).tolist()), math.fsum((b * b).tolist()), math.fsum((a * b).tolist()),
            math.fsum(np.abs(a * b).tolist()), a.size)


def weights(rdotr, fdotf, rdotf, rs, fs, alpha1, alpha2, delta, epsilon, normalized):
    """aw_loss.py:49-96 on rdotr / fdotf (the 1e-4 already added) -> (w_r, w_f, case 1..5)"""
    r_norm, f_norm = (math.sqrt(rdotr), math.sqrt(fdotf)) if normalized else (1.0, 1.0)
    one_r, one_f = 1.0 / r_norm, 1.0 / f_norm
    if rs < alpha1 or rs < (fs - delta):
        if rdotf <= 0:
            return one_r + epsilon, (-rdotf / (fdotf * r_norm)) + epsilon, 1
        return one_r + epsilon, epsilon, 2
    if rs > alpha2 and rs > (fs - delta):
        if rdotf <= 0:
            return (-rdotf / (rdotr * f_norm)) + epsilon, one_f + epsilon, 3
        return epsilon, one_f + epsilon, 4
    return one_r + epsilon, one_f + epsilon, 5


def aw_reference(g_real, g_fake, real_validity, fake_validity, alpha1=0.5, alpha2=0.75, delta=0.05, epsilon=0.05,
                 normalized=True):
    """-> dict: stats (8 fp64, the kernels' layout), grads (fp64 arrays), w_r, w_f, case, and for the
    tests' bounds abs_rf = sum |g_r g_f| and n = the element count"""
    rr, ff, rf, abs_rf, n = dots(g_real, g_fake)
    rr += 1e-4
    ff += 1e-4
    rs = float(np.mean(1.0 / (1.0 + np.exp(-_np64(real_validity)))))
    fs = float(np.mean(1.0 / (1.0 + np.exp(-_np64(fake_validity)))))
    w_r, w_f, case = weights(rr, ff, rf, rs, fs, alpha1, alpha2, delta, epsilon, normalized)
    grads = [w_r * _np64(a) + w_f * _np64(b) for a, b in zip(g_real, g_fake)]
    return dict(stats=np.array([rr, ff, rf, rs, fs, w_r, w_f, float(case)]), grads=grads, w_r=w_r, w_f=w_f,
                case=case, abs_rf=abs_rf, n=n)


# ---------------------------------------------------------------- the fixture (gen_golden_aw.py)
def load_cases():
    """-> list of dicts: a, b (fp32 arrays), real / fake logits, the hyper-parameters, c_r / c_f, the
    intended case and the reference's loss and param.grads (fp64)"""
    data = np.load(os.path.join(GOLDEN, "aw_cases.npz"))
    nt = int(data["ntensors"])
    cases = []
    for k in range(int(data["ncases"])):
        h = dict(zip(data["hyper_names"].tolist(), data[f"case{k}.hyper"].tolist()))
        bkey = "bpos" if h["cosine"] > 0 else "bneg"
        cases.append(dict(
            a=[data[f"a.{i}"] for i in range(nt)], b=[data[f"{bkey}.{i}"] for i in range(nt)],
            real=data[f"case{k}.real"], fake=data[f"case{k}.fake"], hyper=h,
            kw=dict(alpha1=h["alpha1"], alpha2=h["alpha2"], delta=h["delta"], epsilon=h["epsilon"],
                    normalized=bool(h["normalized"])),
            case=int(h["case"]), loss=float(data[f"case{k}.loss"]),
            grads=[data[f"case{k}.grad.{i}"] for i in range(nt)]))
    return cases


# ============================================================================ the C ABI tests
# (tests/test_aw_refs_cpu.py, tests/test_gpu_aw_abi.py): bounds of the form TOL * scale with scale the
# float64 sum of the absolute terms, and a restatement of csrc/aw_kernels.hip's arithmetic: its chunks,
# its strided per-thread sums and its fixed trees in fp64, the combine in fp32.
TOL_STAT = 1e-15   # the fp64 quantities: partials, totals, rs, fs, w_r, w_f   } the smallest powers of ten that keep
TOL_OUT = 1e-6     # the fp32 combine                                          } restate() under a quarter of the bound
EC, THREADS, MAX_JOBS = 16384, 256, 16
NUMELS = (0, 1, 3, 4, 5, 255, 256, 257, 16383, 16384, 16385, 32768 + 2)
KW = dict(alpha1=0.5, alpha2=0.75, delta=0.05, epsilon=0.05, normalized=True)
AW_DEFECTS = ("drop_tail", "drop_partial_256", "rf_lt", "rs_le", "wf_f32_early")


def _f32(t):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).reshape(-1)


def chunks_of(a):
    return [a[i:i + EC] for i in range(0, a.size, EC)]


def _tree(x):
    """sum of the leading axis (a power of two) by halving: lane i + lane i ^ off, as the xor shuffles"""
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        x = x[:h] + x[h:]
    return x[0]


def _block_sum(per_thread):
    """block_sum_f64: (256, ...) -> (...): each wave's xor tree, then (w0 + w1) + (w2 + w3)"""
    w = [_tree(per_thread[64 * i:64 * i + 64]) for i in range(4)]
    return (w[0] + w[1]) + (w[2] + w[3])


def _strided(terms):
    """(n, ...) -> (256, ...): thread t adds terms t, t + 256, ... in order"""
    n = terms.shape[0]
    rounds = -(-n // THREADS)
    pad = np.zeros((rounds * THREADS - n,) + terms.shape[1:])
    x = np.concatenate([terms, pad]).reshape((rounds, THREADS) + terms.shape[1:])
    acc = np.zeros((THREADS,) + terms.shape[1:])
    for r in range(rounds):
        acc = acc + x[r]
    return acc


def chunk_partial(a, b, defect=None):
    """aw_dots_kernel on one chunk (fp32 arrays of at most EC elements) -> [rr, ff, rf]"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    n4 = a.size // 4
    prod = np.stack([a * a, b * b, a * b], 1)              # exact
    q = prod[:4 * n4].reshape(n4, 4, 3)
    acc = _strided((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3]))
    if defect != "drop_tail":
        tail = np.zeros((THREADS, 3))
        tail[:a.size - 4 * n4] = prod[4 * n4:]
        acc = acc + tail
    return _block_sum(acc)


def partials(g_real, g_fake, defect=None):
    """(total chunks, 3): the workspace, pairs in list order, empty pairs skipped"""
    rows = [chunk_partial(x, y, defect) for a, b in zip(g_real, g_fake) for x, y in zip(chunks_of(_f32(a)), chunks_of(_f32(b)))]
    return np.array(rows).reshape(-1, 3)


def merge(parts, defect=None):
    """aw_weights_kernel's merge of the partials -> [rr, ff, rf], the 1e-4 not yet added"""
    if defect == "drop_partial_256":
        parts = np.delete(parts, 256, 0) if parts.shape[0] > 256 else parts
    return _block_sum(_strided(parts)) if parts.shape[0] else np.zeros(3)


def sigmoid_mean(x):
    x = _f32(x).astype(np.float64)
    return float(_block_sum(_strided(1.0 / (1.0 + np.exp(-x)))) / x.size)


def select(rr, ff, rf, rs, fs, alpha1, alpha2, delta, epsilon, normalized, defect=None):
    """thread 0 of aw_weights_kernel on rr / ff with the 1e-4 added -> (w_r, w_f, case)"""
    r_norm, f_norm = math.sqrt(rr), math.sqrt(ff)
    one_r, one_f = (1.0 / r_norm, 1.0 / f_norm) if normalized else (1.0, 1.0)
    neg = rf < 0.0 if defect == "rf_lt" else rf <= 0.0
    first = rs <= alpha1 if defect == "rs_le" else rs < alpha1
    if first or rs < fs - delta:
        if neg:
            return one_r + epsilon, (-rf / (ff * r_norm) if normalized else -rf / ff) + epsilon, 1
        return one_r + epsilon, epsilon, 2
    if rs > alpha2 and rs > fs - delta:
        if neg:
            return (-rf / (rr * f_norm) if normalized else -rf / rr) + epsilon, one_f + epsilon, 3
        return epsilon, one_f + epsilon, 4
    return one_r + epsilon, one_f + epsilon, 5


def combine_f32(a, b, w_r, w_f):
    """aw_combine_kernel: fmaf(wf, g_f, wr * g_r) with the weights rounded to fp32 once"""
    wr, wf = np.float32(w_r), np.float32(w_f)
    a, b = _f32(a), _f32(b)
    return (np.float64(wf) * b.astype(np.float64) + (wr * a).astype(np.float64)).astype(np.float32)


def restate(g_real, g_fake, real, fake, alpha1=0.5, alpha2=0.75, delta=0.05, epsilon=0.05, normalized=True, defect=None):
    """-> dict(parts, stats (8), out): what the two entry points leave"""
    parts = partials(g_real, g_fake, defect)
    rr, ff, rf = merge(parts, defect)
    rr, ff = rr + 1e-4, ff + 1e-4
    rs, fs = sigmoid_mean(real), sigmoid_mean(fake)
    w_r, w_f, case = select(rr, ff, rf, rs, fs, alpha1, alpha2, delta, epsilon, normalized, defect)
    if defect == "wf_f32_early":
        w_f = float(np.float32(w_f))
    return dict(parts=parts, stats=np.array([rr, ff, rf, rs, fs, w_r, w_f, float(case)]),
                out=[combine_f32(a, b, w_r, w_f) for a, b in zip(g_real, g_fake)])


def _fsum3(a, b):
    """correctly rounded [rr, ff, rf] of one chunk and their scales (a sum of squares is its own scale)"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    rr, ff = math.fsum((a * a).tolist()), math.fsum((b * b).tolist())
    return [rr, ff, math.fsum((a * b).tolist())], [rr, ff, float(np.abs(a * b).sum())]


def _sh(err, tol, scale):
    err, scale = np.asarray(err, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    if not np.isfinite(err).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(err == 0, 0.0, err / (tol * scale))
    return float(s.max()) if s.size else 0.0


def abi_shares(g_real, g_fake, real, fake, kw, got, tie=False):
    """shares of the bounds for got = dict(parts, stats, out).  partials and totals against correctly rounded
    sums (scale: the sum of |x y| over the same terms, plus the 1e-4 for rr and ff); rs, fs scale 1; the
    weights against weights() at got's own stats (scale |w - eps| + |eps|) and, away from a tie, end to end;
    out against float32(w_r) g_r + float32(w_f) g_f in float64 at got's weights.
    -> (shares, the end-to-end case)"""
    a = [_f32(x) for x in g_real]
    b = [_f32(x) for x in g_fake]
    ref, scale = [], []
    for x, y in zip(a, b):
        for cx, cy in zip(chunks_of(x), chunks_of(y)):
            r, s = _fsum3(cx, cy)
            ref.append(r)
            scale.append(s)
    ref, scale = np.array(ref).reshape(-1, 3), np.array(scale).reshape(-1, 3)
    sh = {"parts": _sh(np.abs(got["parts"] - ref), TOL_STAT, scale)}
    s = got["stats"]
    tot = np.array([math.fsum(ref[:, i].tolist()) for i in range(3)]) + [1e-4, 1e-4, 0.0]
    tscale = np.array([math.fsum(scale[:, i].tolist()) for i in range(3)]) + [1e-4, 1e-4, 0.0]
    for i, k in enumerate(("rr", "ff", "rf")):
        sh[k] = _sh(abs(s[i] - tot[i]), TOL_STAT, tscale[i])
    rs = float(np.mean(1.0 / (1.0 + np.exp(-_np64(real)))))
    fs = float(np.mean(1.0 / (1.0 + np.exp(-_np64(fake)))))
    sh["rs"], sh["fs"] = _sh(abs(s[3] - rs), TOL_STAT, 1.0), _sh(abs(s[4] - fs), TOL_STAT, 1.0)
    eps = kw["epsilon"]
    w_r, w_f, case = weights(s[0], s[1], s[2], s[3], s[4], **kw)
    assert int(s[7]) == case, f"case {int(s[7])} at the kernel's own stats, the reference takes {case}"
    sh["w_own"] = max(_sh(abs(s[5] - w_r), TOL_STAT, abs(w_r - eps) + abs(eps)),
                      _sh(abs(s[6] - w_f), TOL_STAT, abs(w_f - eps) + abs(eps)))
    e_r, e_f, e_case = weights(tot[0], tot[1], tot[2], rs, fs, **kw)
    if not tie:
        assert int(s[7]) == e_case, f"case {int(s[7])}, float64 throughout takes {e_case}"
        rel = TOL_STAT * (tscale / np.maximum(np.abs(tot), 1e-300))   # the dots' bounds carried into the weights
        amp = 1.0 + (rel[0] + rel[1] + rel[2]) / TOL_STAT
        sh["w_e2e"] = max(_sh(abs(s[5] - e_r), TOL_STAT, amp * (abs(e_r - eps) + abs(eps))),
                          _sh(abs(s[6] - e_f), TOL_STAT, amp * (abs(e_f - eps) + abs(eps))))
    wr, wf = float(np.float32(s[5])), float(np.float32(s[6]))
    worst = 0.0
    for o, x, y in zip(got["out"], a, b):
        x, y = x.astype(np.float64), y.astype(np.float64)
        worst = max(worst, _sh(np.abs(_np64(o).reshape(-1) - (wr * x + wf * y)), TOL_OUT, np.abs(wr * x) + np.abs(wf * y)))
    sh["out"] = worst
    return sh, e_case


# ---------------------------------------------------------------------------- inputs
def make_list(numels, sign, seed):
    """g_real ~ N(0, 0.1), g_fake = sign g_real + N(0, 0.03): rf takes the sign of ``sign``"""
    rng = np.random.default_rng(seed)
    a = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in numels]
    b = [(np.float32(sign) * x + (0.03 * rng.standard_normal(x.size)).astype(np.float32)).astype(np.float32) for x in a]
    return a, b


def logits_for(kind, n_real=5, n_fake=7, seed=0):
    """logits that put rs below alpha1 = 0.5 ("low": cases 1 / 2), above alpha2 = 0.75 and fs - delta ("high":
    3 / 4) or between ("mid": 5), well away from the thresholds"""
    rng = np.random.default_rng(100 + seed)
    centre = {"low": -1.5, "high": 2.5, "mid": 0.5}[kind]
    return ((centre + 0.1 * rng.standard_normal(n_real)).astype(np.float32),
            (0.1 * rng.standard_normal(n_fake)).astype(np.float32))


FIVE = {1: ("low", -1.0), 2: ("low", 1.0), 3: ("high", -1.0), 4: ("high", 1.0), 5: ("mid", 1.0)}


def tie_cases():
    """name -> (g_real, g_fake, real, fake, kw, the case, the planted defect that flips it)"""
    a, b = make_list((5, 257), 1.0, 9)
    z = np.zeros(8, dtype=np.float32)
    half = np.array([100.0] * 4 + [0.0] * 4, dtype=np.float32)    # sigmoid = 1 (exactly, in fp64) and 0.5: fs = 0.75
    da = [np.array([1.0, 2.0, 0.0, 0.0, 0.0], dtype=np.float32), np.zeros(257, dtype=np.float32)]
    db = [np.array([0.0, 0.0, 3.0, -1.0, 0.5], dtype=np.float32), np.ones(257, dtype=np.float32)]
    low = logits_for("low")
    return {
        "rs == alpha1": (a, b, z, z, dict(KW), 5, "rs_le"),                       # 0.5 < 0.5 is false; 0.5 > 0.75 is too
        "rs == fs - delta": (a, b, z, half, dict(KW, alpha1=0.25, alpha2=0.4, delta=0.25), 5, None),
        "rf == 0": (da, db, low[0], low[1], dict(KW), 1, "rf_lt"),
    }

