"""Restatements of the metric arithmetic (torch_fidelity metric_fid.py, metric_kid.py, metric_isc.py) that the tests
of csrc/metric_kernels.hip and fidelity.py compare against, with the bounds of those tests.

They run in np.longdouble where it carries at least 63 mantissa bits (x86: 64), so that the reference's own
rounding (2^-64 per operation) does not eat a bound stated in units of 2^-53.  Elsewhere the polynomial parts
(moments, Gram sums) run on fractions.Fraction, exactly; the Inception score, which needs exp and log, then stays in
float64 and its bound carries the reference's own share.

U = 2^-53.  Bounds (derived, not measured):
  moments   per entry of S2, N rows in all:  (N + 4) U sum_n |x_ni - p_i| |x_nj - p_j|
            the worst case of an N-term fp64 sum in any order (N - 1 roundings on a term's path), one rounding per
            product and one per pivoted factor; s1 alike with (N + 2) U sum_n |x_ni - p_i|
  KID       each of the six sums of a subset: (3 (D + 8) + m^2) U sum_ij (gamma sum_k |x_ik| |y_jk| + |c0|)^degree
            a D-term dot (D + small roundings) enters the kernel value `degree` <= 3 times, then an m^2-term sum
  ISC       on the exponent E before exp: (C + N + 16) U (sum |p log p| + n sum_c |q_c log q_c|)
"""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
WIDE = np.finfo(LD).nmant >= 63
U = 2.0 ** -53


def lift(a):
    """float array -> the wide type (exact)"""
    a = np.asarray(a)
    if WIDE:
        return a.astype(LD)
    return np.vectorize(Fraction, otypes=[object])(a.astype(np.float64))


def lower(a):
    """wide array -> float64 (one rounding)"""
    a = np.asarray(a)
    if a.dtype == object:
        return np.vectorize(float, otypes=[np.float64])(a)
    return a.astype(np.float64)


def _abs(a):
    return np.abs(a) if a.dtype != object else np.vectorize(abs, otypes=[object])(a)


# --------------------------------------------------------------------------- moments
def moments(batches, pivot):
    """wide {n, s1, S2, a1 = sum |x - p|, a2 = sum |x - p||x - p|^T} of the rows of ``batches`` around ``pivot``"""
    x = lift(np.concatenate([np.asarray(b, dtype=np.float32) for b in batches])) - lift(pivot)[None, :]
    ax = _abs(x)
    return dict(n=x.shape[0], s1=x.sum(axis=0), S2=x.T @ x, a1=ax.sum(axis=0), a2=ax.T @ ax)


def moments_bounds(m):
    """(bound of s1, bound of S2) as float64 arrays"""
    return (m["n"] + 2) * U * lower(m["a1"]), (m["n"] + 4) * U * lower(m["a2"])


def column_mean(batch):
    x = lift(np.asarray(batch, dtype=np.float32))
    return x.sum(axis=0) / x.shape[0]


def statistics(features):
    """wide (mu, sigma) = (mean, np.cov(rowvar=False)) of the rows"""
    x = lift(np.asarray(features, dtype=np.float32))
    n = x.shape[0]
    mu = x.sum(axis=0) / n
    d = x - mu[None, :]
    return mu, (d.T @ d) / (n - 1)


def statistics_from_state(n, pivot, s1, S2):
    """the formulas of FeatureStats.statistics on float64 arrays (numpy)"""
    d = s1 / n
    return pivot + d, (S2 - n * np.outer(d, d)) / (n - 1)


def repivot(n, pivot, s1, S2, new_pivot):
    """the identity FeatureStats.merge uses, on float64 numpy arrays"""
    delta = new_pivot - pivot
    d = s1 / n
    return s1 - n * delta, S2 - n * (np.outer(d, delta) + np.outer(delta, d)) + n * np.outer(delta, delta)


def fid_from_statistics(mu1, sigma1, mu2, sigma2):
    """metric_fid.py:38-40 on float64 numpy"""
    diff = mu1 - mu2
    tr = np.sum(np.sqrt(np.linalg.eigvals(sigma1.dot(sigma2)).astype("complex128")).real)
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr)


# --------------------------------------------------------------------------- KID
def _ipow(a, degree):
    out = a
    for _ in range(degree - 1):
        out = out * a
    return out


def kid_sums(f1, f2, idx1, idx2, degree, gamma, coef0):
    """wide (subsets, 6) [sum K_XX, sum diag K_XX, sum K_YY, sum diag K_YY, sum K_XY, trace K_XY] and the float64
    (subsets, 6) bounds"""
    g, c0 = lift(np.float64(gamma)), lift(np.float64(coef0))
    ag, ac0 = abs(float(gamma)), abs(float(coef0))
    S, m = idx1.shape
    D = f1.shape[1]
    sums, bounds = [], []
    for s in range(S):
        x, y = lift(f1[idx1[s]]), lift(f2[idx2[s]])
        ax, ay = np.abs(f1[idx1[s]].astype(np.float64)), np.abs(f2[idx2[s]].astype(np.float64))
        row, brow = [], []
        for a, b, aa, ab in ((x, x, ax, ax), (y, y, ay, ay), (x, y, ax, ay)):
            K = _ipow((a @ b.T) * g + c0, degree)
            scale = float(np.sum((ag * (aa @ ab.T) + ac0) ** degree))
            row += [K.sum(), np.trace(K)]
            brow += [(3 * (D + 8) + m * m) * U * scale] * 2
        sums.append(row)
        bounds.append(brow)
    return np.array(sums, dtype=object if not WIDE else LD), np.array(bounds, dtype=np.float64)


def mmd2(sums, m):
    """unbiased estimate (metric_kid.py:54-56) from the six sums, any array type"""
    return (sums[..., 0] - sums[..., 1] + sums[..., 2] - sums[..., 3]) / (m * (m - 1)) - 2 * sums[..., 4] / (m * m)


def mmd2_bound(bounds, m):
    return (bounds[..., 0] + bounds[..., 1] + bounds[..., 2] + bounds[..., 3]) / (m * (m - 1)) + 2 * bounds[..., 4] / (m * m)


def kid_tables(n1, n2, subsets, m, seed=2020):
    """the reference's subsets: RandomState(seed).choice per subset, input 1 first (metric_kid.py:117-123)"""
    rng = np.random.RandomState(seed)
    idx = np.empty((2, subsets, m), dtype=np.int64)
    for i in range(subsets):
        idx[0, i] = rng.choice(n1, m, replace=False)
        idx[1, i] = rng.choice(n2, m, replace=False)
    return idx[0], idx[1]


def kid_metric(f1, f2, subsets, m, degree=3, gamma=None, coef0=1.0, seed=2020):
    """float64 (mean, std, bound on either): std is 1-Lipschitz in the rms of the per-subset errors"""
    gamma = 1.0 / f1.shape[1] if gamma is None else gamma
    i1, i2 = kid_tables(len(f1), len(f2), subsets, m, seed)
    sums, bounds = kid_sums(f1, f2, i1, i2, degree, gamma, coef0)
    mm = lower(mmd2(sums, m))
    tol = float(np.max(mmd2_bound(bounds, m))) + (subsets + 4) * U * float(np.max(np.abs(mm)))
    return float(np.mean(mm)), float(np.std(mm)), tol


# --------------------------------------------------------------------------- ISC
def isc_perm(n, shuffle, seed=2020):
    return np.random.RandomState(seed).permutation(n).astype(np.int64) if shuffle else np.arange(n, dtype=np.int64)


def isc_chunks(logits, perm, splits):
    """per chunk: dict(n, A = sum p log p, colsum, E, score, bound) -- E and its bound in float64"""
    logits = np.asarray(logits, dtype=np.float32)
    N, C = logits.shape
    out = []
    for i in range(splits):
        rows = perm[i * N // splits:(i + 1) * N // splits]
        n = len(rows)
        # the same quantities as metric_isc.py:24-33, written so that a peaked row and a column whose mean
        # probability is near 1 keep their relative accuracy: the row's first maximum is left out of the
        # log-sum-exp (log1p of the rest), and log q comes from the complement t = sum (1 - p) where q > 1/2
        x = logits[rows].astype(LD if WIDE else np.float64)
        top = np.zeros(x.shape, dtype=bool)
        top[np.arange(n), x.argmax(axis=1)] = True
        d = x - x.max(axis=1, keepdims=True)
        rest = np.where(top, 0, np.exp(d)).sum(axis=1, keepdims=True)
        logp = d - np.log1p(rest)
        p = np.exp(logp)
        s = p.sum(axis=0)
        t = (-np.expm1(logp)).sum(axis=0)
        q = s / n
        logq = np.where(t / n < 0.5, np.log1p(-np.minimum(t / n, 0.5)), np.log(q))
        A = (p * logp).sum()
        cross = (s * logq).sum()
        sa = float(np.abs(p * logp).sum())
        sq = float(np.abs(q * logq).sum())
        E = float((A - cross) / n)
        out.append(dict(n=n, A=float(A), colsum=lower(s), E=E, score=math.exp(E), bound=(C + N + 16) * U * (sa + sq * n),
                        abs_plogp=sa))
    return out


def isc_metric(logits, splits, shuffle, seed=2020):
    """float64 (mean, std, bound on either): d exp(E) <= exp(E) expm1(bound), then mean / std over the chunks"""
    ch = isc_chunks(logits, isc_perm(len(logits), shuffle, seed), splits)
    sc = np.array([c["score"] for c in ch])
    tol = max(c["score"] * math.expm1(c["bound"]) for c in ch) + (splits + 4) * U * float(sc.max())
    return float(np.mean(sc)), float(np.std(sc)), tol
