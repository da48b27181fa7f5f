"""Restatement of the improved precision and recall (torch_fidelity metric_prc.py:57-66) that the tests of
csrc/prc_kernels.hip and fidelity.prc_features_to_metric compare against, with the bounds of those tests.

Squared distances by direct difference, d2(a, b) = sum_k (a_k - b_k)^2, in np.longdouble where it carries at least 63
mantissa bits (x86: 64), on fractions.Fraction elsewhere (metric_refs.lift).  features_1 is the REAL set.

U = 2^-53.  Bounds (derived, not measured) for a kernel that forms d2 = max(0, n_a + n_b - 2 g) in fp64 from the
row norms n and the dot product g, each a D-term fp64 sum in any order:
  pair      E_ab = (D + 8) U sum_k (|a_k| + |b_k|)^2:  n_a, n_b and g carry at most D U of sum a^2, sum b^2 and
            sum |a||b| (one rounding per product, D - 1 on a term's path), the two additions three more U of
            n_a + n_b + 2 |g| <= sum (|a| + |b|)^2; the clamp at 0 moves towards the true value
  radius    r2 of row j: max_i E_ji -- an order statistic is 1-Lipschitz in the sup norm of its inputs
  margin    of a row's coverage decision, m = min over the other set of (d2 - r2): max over the pairs of
            (E + the radius bound), a minimum being 1-Lipschitz too.  The row is covered iff m <= 0; a row with
            |m| above its bound has one possible flag
"""
import numpy as np

from metric_refs import U, lift, lower

CHUNK = 128


def d2_and_bound(a, b):
    """wide (Na, Nb) direct-difference squared distances and the float64 per-pair bound E"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    D = a.shape[1]
    wa, wb = lift(a), lift(b)
    aa, ab = np.abs(a.astype(np.float64)), np.abs(b.astype(np.float64))
    rows, bounds = [], []
    for at in range(0, len(a), CHUNK):
        diff = wa[at:at + CHUNK, None, :] - wb[None, :, :]
        rows.append((diff * diff).sum(axis=2))
        s = aa[at:at + CHUNK, None, :] + ab[None, :, :]
        bounds.append((D + 8) * U * (s * s).sum(axis=2))
    return np.concatenate(rows), np.concatenate(bounds)


def kth_smallest(d2, k1):
    """the k1-th smallest of every row (1-based), as kthvalue(k1) takes it"""
    return np.sort(d2, axis=1)[:, k1 - 1]


def prc(f1, f2, k):
    """dict of radii2_1, radii2_2 (wide), rbound_1, rbound_2, hit_2, hit_1 (int), margin_2, margin_1 (float64,
    min over the other set of d2 - r2) and mbound_2, mbound_1; counts = [sum hit_2, sum hit_1]"""
    d11, e11 = d2_and_bound(f1, f1)
    d22, e22 = d2_and_bound(f2, f2)
    d21, e21 = d2_and_bound(f2, f1)            # rows from F2, columns from F1
    r1, r2 = kth_smallest(d11, k + 1), kth_smallest(d22, k + 1)
    rb1, rb2 = e11.max(axis=1), e22.max(axis=1)
    m2 = (d21 - r1[None, :]).min(axis=1)       # F2[i] against the balls of F1
    m1 = (d21 - r2[:, None]).min(axis=0)       # F1[j] against the balls of F2
    hit_2, hit_1 = (m2 <= 0).astype(np.int64), (m1 <= 0).astype(np.int64)
    return dict(radii2_1=r1, radii2_2=r2, rbound_1=rb1, rbound_2=rb2, hit_2=hit_2, hit_1=hit_1,
                margin_2=lower(m2), margin_1=lower(m1), mbound_2=(e21 + rb1[None, :]).max(axis=1),
                mbound_1=(e21 + rb2[:, None]).max(axis=0), counts=[int(hit_2.sum()), int(hit_1.sum())])


def metric(ref, n1, n2):
    p, r = ref["counts"][0] / n2, ref["counts"][1] / n1
    return p, r, 2 * p * r / max(1e-5, p + r)


def lattice(n1=70, n2=67, d=5, seed=7):
    """small integers (F1 in [-4, 2], F2 in [-2, 4]: the sets overlap in part, so neither is covered whole) with rows
    duplicated within and across the sets: every product and sum is exact in fp64 in any order, so radii, flags
    and counts have one value.  Row 3 of F1 occurs five times (r2 = 0 at k = 3) and once in F2."""
    rng = np.random.RandomState(seed)
    f1 = rng.randint(-4, 3, size=(n1, d)).astype(np.float32)
    f2 = rng.randint(-2, 5, size=(n2, d)).astype(np.float32)
    f1[10:14] = f1[3]
    f1[n1 - 1] = f1[20]
    f2[5] = f1[3]
    f2[20:22] = f2[7]
    f2[n2 - 1] = f1[40]
    return f1, f2
