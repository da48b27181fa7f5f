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
