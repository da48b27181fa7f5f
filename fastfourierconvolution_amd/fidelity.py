"""The evaluation caller of the generators: how torch_fidelity drives a
generator when the reference scripts compute FID / IS (fgan_complete.py:416-418 wraps ``G`` in
``GenerativeModelModuleWrapper(G, z_size, z_type, 0)``).

The generator side is restated: sample noise, run the generator batch by batch, hand the fakes
on.  The feature extractor (Inception weights fetched by URL) stays out of scope and is the
caller's; the metric arithmetic that works on feature tensors runs on the device
(csrc/metric_kernels.hip).

  * ``random_normal``      torch_fidelity/noise.py:8-9      (numpy RandomState.randn -> float32)
  * ``GenerativeModelModuleWrapper``  torch_fidelity/generative_model_modulewrapper.py:10-68
                           (argument checks, eval mode, optional .cuda()).  torch_fidelity itself
                           passes the 2-D noise (B, z_size) through unchanged; ``FFCGenerator``
                           takes 4-D noise (B, nz, 1, 1) (models/ffc_generator.py:30), so this
                           wrapper has an explicit ``noise_4d`` argument (default: True exactly
                           for ``FFCGenerator`` instances) -- an extension, not reference behaviour
  * ``generate_batches``   torch_fidelity/utils.py:160-208 without the feature extractor: batches
                           of ``batch_size`` (default 64, defaults.py:5), RandomState(rng_seed)
                           (default 2020, defaults.py:56), ``torch.no_grad()``, the last batch ragged
  * ``FeatureStats``       metric_fid.py:21-29 (``fid_features_to_statistics``) as a streaming fp64
                           scatter matrix on the device; ``fid_statistics_to_metric`` metric_fid.py:32-46
  * ``kid_features_to_metric``  metric_kid.py:21-134 (polynomial kernel, ``mmd_est="unbiased"``)
  * ``isc_features_to_metric``  metric_isc.py:16-39
  * ``prc_features_to_metric``  metric_prc.py:57-94 (csrc/prc_kernels.hip); ``calculate_prc`` drives
                           a generator into it.  The reference's trainers do not pass ``prc=True``; this
                           completes the vendored evaluation surface
  * ``calculate_metrics``  metrics.py's driver for a generator as input 1, with the caller's extractor
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

__all__ = ["random_normal", "GenerativeModelModuleWrapper", "generate_batches", "FeatureStats",
           "fid_statistics_to_metric", "kid_features_to_metric", "isc_features_to_metric", "calculate_metrics",
           "mmd2_from_sums", "isc_from_chunk_sums", "prc_features_to_metric", "calculate_prc"]

DEFAULT_BATCH_SIZE = 64     # torch_fidelity/defaults.py:5
DEFAULT_RNG_SEED = 2020     # torch_fidelity/defaults.py:56


def random_normal(rng: np.random.RandomState, shape) -> torch.Tensor:
    """torch_fidelity/noise.py:8-9"""
    return torch.from_numpy(rng.randn(*shape)).float()


NOISE_SOURCES = {"normal": random_normal}


class GenerativeModelModuleWrapper(nn.Module):
    """torch_fidelity/generative_model_modulewrapper.py:10-68 for the FFC generators.  Raises
    ValueError where torch_fidelity's ``vassert`` raises.  Only the "normal" noise source is on the
    reference's path (fgan_complete.py passes ``args.z_type`` = "normal")."""

    def __init__(self, module, z_size, z_type="normal", num_classes=0, make_eval=True, cuda=None, noise_4d=None):
        super().__init__()
        if not isinstance(module, nn.Module):
            raise ValueError("Not an instance of torch.nn.Module")
        if type(z_size) is not int or z_size <= 0:
            raise ValueError("z_size must be a positive integer")
        if z_type not in NOISE_SOURCES:
            raise ValueError(f"z_type={z_type} not implemented")
        if type(num_classes) is not int or num_classes != 0:
            raise ValueError("the FFC generators are unconditional: num_classes must be 0")
        self.module = module
        if make_eval:
            self.module.eval()
        if cuda is not None:
            self.module = self.module.cuda() if cuda else self.module.cpu()
        self.z_size, self.z_type, self.num_classes = z_size, z_type, num_classes
        # FFCGenerator's first layer is a ConvTranspose2d on a 1x1 input: it takes (B, nz, 1, 1);
        # torch_fidelity proper would hand it the 2-D noise unchanged (noise_4d=False)
        if noise_4d is None:
            from .models import FFCGenerator
            noise_4d = isinstance(module, FFCGenerator)
        self._noise_4d = bool(noise_4d)

    def forward(self, z):
        if self._noise_4d and z.dim() == 2:
            z = z.reshape(z.shape[0], z.shape[1], 1, 1)
        return self.module(z)


def generate_batches(gen_model: GenerativeModelModuleWrapper, num_samples: int,
                     batch_size: int = DEFAULT_BATCH_SIZE, cuda: bool = True, rng_seed: int = DEFAULT_RNG_SEED):
    """Yield the generator's fakes batch by batch, as torch_fidelity/utils.py:160-208 feeds them
    to its feature extractor."""
    if not isinstance(gen_model, GenerativeModelModuleWrapper):
        raise ValueError("Input can only be a GenerativeModel instance")
    if batch_size > num_samples:
        batch_size = num_samples
    rng = np.random.RandomState(rng_seed)
    if cuda:
        gen_model.cuda()
    with torch.no_grad():
        for start in range(0, num_samples, batch_size):
            sz = min(start + batch_size, num_samples) - start
            noise = NOISE_SOURCES[gen_model.z_type](rng, (sz, gen_model.z_size))
            if cuda:
                noise = noise.cuda(non_blocking=True)
            yield gen_model(noise)


# --------------------------------------------------------------------------- metrics from features
KEY_METRIC_FID = "frechet_inception_distance"
KEY_METRIC_ISC_MEAN = "inception_score_mean"
KEY_METRIC_ISC_STD = "inception_score_std"
KEY_METRIC_KID_MEAN = "kernel_inception_distance_mean"
KEY_METRIC_KID_STD = "kernel_inception_distance_std"
KEY_METRIC_PRECISION = "precision"
KEY_METRIC_RECALL = "recall"
KEY_METRIC_F_SCORE = "f_score"


def _repivot(n, pivot, s1, S2, new_pivot):
    """(s1, S2) of the same rows around ``new_pivot``: with delta = new_pivot - pivot and d = s1 / n,
    s1' = s1 - n delta and S2' = S2 - n (d delta^T + delta d^T) + n delta delta^T"""
    delta = new_pivot - pivot
    cross = torch.outer(s1, delta)
    # cross + cross^T first: every term is then exactly symmetric, and so is the result
    return s1 - n * delta, S2 - (cross + cross.t()) + n * torch.outer(delta, delta)


class FeatureStats:
    """Streaming mean and covariance of feature rows (``fid_features_to_statistics``,
    metric_fid.py:21-29) in fp64 on the device: state = [n, pivot[D], s1[D], S2[D][D]] with
    s1 = sum (x - pivot), S2 = sum (x - pivot)(x - pivot)^T; the pivot is the first batch's column
    mean, so a large common offset of the features does not cancel the covariance away.
    ``update`` launches ffc::feat_moments_update and returns; only ``statistics`` synchronises."""

    def __init__(self, dim: int, device=None):
        from ._metrics import FM_MAX_D, state_doubles
        if type(dim) is not int or not 1 <= dim <= FM_MAX_D:
            raise ValueError(f"dim must be an integer in 1 .. {FM_MAX_D}")
        self.dim = dim
        self.state = torch.zeros(state_doubles(dim), dtype=torch.float64, device=device if device is not None else "cuda")

    # views into the state
    @property
    def n(self):
        return self.state[0:1]

    @property
    def pivot(self):
        return self.state[1:1 + self.dim]

    @property
    def s1(self):
        return self.state[1 + self.dim:1 + 2 * self.dim]

    @property
    def S2(self):
        return self.state[1 + 2 * self.dim:].view(self.dim, self.dim)

    def update(self, features: torch.Tensor) -> "FeatureStats":
        if features.dim() != 2 or features.shape[1] != self.dim:
            raise ValueError(f"features must be (B, {self.dim}), got {tuple(features.shape)}")
        if features.shape[0]:
            torch.ops.ffc.feat_moments_update(self.state, features)
        return self

    def merge(self, other: "FeatureStats") -> "FeatureStats":
        """add ``other``'s rows; fp64 torch ops on the device, no synchronisation.  An empty ``self`` takes
        ``other``'s pivot; otherwise ``other`` is re-pivoted to ``self``'s."""
        if not isinstance(other, FeatureStats) or other.dim != self.dim:
            raise ValueError("merge needs a FeatureStats of the same dim")
        pivot = torch.where(self.n == 0, other.pivot, self.pivot)
        s1, S2 = _repivot(other.n, other.pivot, other.s1, other.S2, pivot)
        self.pivot.copy_(pivot)
        self.s1.add_(s1)
        self.S2.add_(S2)
        self.n.add_(other.n)
        return self

    def all_reduce(self, group=None) -> "FeatureStats":
        """sum the states of all ranks of ``group``: rank 0's pivot is broadcast, every rank re-pivots to it,
        then [n, s1, S2] are all-reduced (the distributed.merge_moments pattern)"""
        import torch.distributed as dist
        pivot = self.pivot.clone()
        dist.broadcast(pivot, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        s1, S2 = _repivot(self.n, self.pivot, self.s1, self.S2, pivot)
        self.pivot.copy_(pivot)
        self.s1.copy_(s1)
        self.S2.copy_(S2)
        for part in (self.n, self.s1, self.S2):
            dist.all_reduce(part, op=dist.ReduceOp.SUM, group=group)
        return self

    def statistics(self) -> dict:
        """{"mu", "sigma"} as fp64 numpy arrays: sigma = (S2 - n d d^T) / (n - 1), d = s1 / n, which is
        ``np.cov(features, rowvar=False)``.  Synchronises."""
        n = float(self.n.item())
        if n < 2:
            raise ValueError("statistics() needs at least two feature rows")
        d = self.s1 / n
        sigma = (self.S2 - n * torch.outer(d, d)) / (n - 1.0)
        return {"mu": (self.pivot + d).cpu().numpy(), "sigma": sigma.cpu().numpy()}


def fid_statistics_to_metric(stat_1, stat_2) -> dict:
    """metric_fid.py:32-46 on the host (numpy, complex128 eigenvalues of sigma1 @ sigma2): one call per
    evaluation, and no fp64 eigen-solver exists on the device side of this library."""
    mu1, sigma1 = np.asarray(stat_1["mu"]), np.asarray(stat_1["sigma"])
    mu2, sigma2 = np.asarray(stat_2["mu"]), np.asarray(stat_2["sigma"])
    if not (mu1.ndim == 1 and mu1.shape == mu2.shape and mu1.dtype == mu2.dtype):
        raise ValueError("mu: two 1-D arrays of one shape and dtype")
    if not (sigma1.ndim == 2 and sigma1.shape == sigma2.shape and sigma1.dtype == sigma2.dtype):
        raise ValueError("sigma: two 2-D arrays of one shape and dtype")
    diff = mu1 - mu2
    tr_covmean = np.sum(np.sqrt(np.linalg.eigvals(sigma1.dot(sigma2)).astype("complex128")).real)
    return {KEY_METRIC_FID: float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean)}


def mmd2_from_sums(sums, m: int):
    """the unbiased MMD^2 estimate of metric_kid.py:21-60 from the six sums per subset of ffc::kid_sums,
    [sum K_XX, sum diag K_XX, sum K_YY, sum diag K_YY, sum K_XY, trace K_XY] (..., 6):
    (sum K_XX - diag + sum K_YY - diag) / (m (m - 1)) - 2 sum K_XY / m^2"""
    return (sums[..., 0] - sums[..., 1] + sums[..., 2] - sums[..., 3]) / (m * (m - 1)) - 2 * sums[..., 4] / (m * m)


def isc_from_chunk_sums(n, plogp, colsum):
    """the score of one chunk (metric_isc.py:28-34) from n rows, A = sum p log p and the column sums s_c of
    p (torch tensors): exp((A - sum_c s_c log(s_c / n)) / n)"""
    return torch.exp((plogp - torch.sum(torch.xlogy(colsum, colsum / n), dim=-1)) / n)


def kid_features_to_metric(features_1, features_2, kid_subsets=100, kid_subset_size=1000, kid_kernel_poly_degree=3,
                           kid_kernel_poly_gamma=None, kid_kernel_poly_coef0=1, rng_seed=DEFAULT_RNG_SEED,
                           kid_kernel="poly") -> dict:
    """metric_kid.py:96-134 with the polynomial kernel and ``mmd_est="unbiased"``: the subsets are the
    reference's (RandomState(rng_seed).choice per subset, input 1 first); ffc::kid_sums forms the three
    Gram matrices of every subset tile by tile and keeps six sums of each; MMD^2, mean and std are fp64
    on the device."""
    if kid_kernel == "rbf":
        raise NotImplementedError("kid_kernel='rbf' is not implemented (the reference's default is 'poly')")
    if kid_kernel != "poly":
        raise ValueError("Invalid KID kernel")
    if not (torch.is_tensor(features_1) and features_1.dim() == 2 and torch.is_tensor(features_2)
            and features_2.dim() == 2 and features_1.shape[1] == features_2.shape[1]):
        raise ValueError("features must be two 2-D tensors of one width")
    n1, n2, m = len(features_1), len(features_2), int(kid_subset_size)
    if not (n1 >= m and n2 >= m):
        raise ValueError(f"KID subset size {m} cannot be smaller than the number of samples "
                         f"(input_1: {n1}, input_2: {n2})")
    if m < 2 or kid_subsets < 1:
        raise ValueError("kid_subset_size >= 2 and kid_subsets >= 1")
    degree = int(kid_kernel_poly_degree)
    if degree != kid_kernel_poly_degree or degree < 1:
        raise ValueError("kid_kernel_poly_degree must be an integer >= 1")
    gamma = 1.0 / features_1.shape[1] if kid_kernel_poly_gamma is None else float(kid_kernel_poly_gamma)
    rng = np.random.RandomState(rng_seed)
    idx = np.empty((2, kid_subsets, m), dtype=np.int64)
    for i in range(kid_subsets):
        idx[0, i] = rng.choice(n1, m, replace=False)
        idx[1, i] = rng.choice(n2, m, replace=False)
    idx = torch.from_numpy(idx).to(features_1.device)
    sums = torch.ops.ffc.kid_sums(features_1, features_2, idx[0], idx[1], degree, gamma, float(kid_kernel_poly_coef0))
    mmds = mmd2_from_sums(sums, m)
    return {KEY_METRIC_KID_MEAN: float(mmds.mean().item()), KEY_METRIC_KID_STD: float(mmds.std(unbiased=False).item())}


def isc_features_to_metric(logits, splits=10, shuffle=True, rng_seed=DEFAULT_RNG_SEED) -> dict:
    """metric_isc.py:16-39: one pass of ffc::isc_sums over the logits.  ``N < splits`` raises ValueError
    (the reference returns NaN for its empty chunks)."""
    if not (torch.is_tensor(logits) and logits.dim() == 2):
        raise ValueError("logits must be a 2-D tensor")
    N = logits.shape[0]
    if type(splits) is not int or splits < 1:
        raise ValueError("splits must be a positive integer")
    if N < splits:
        raise ValueError(f"N = {N} rows cannot fill {splits} splits")
    perm = np.random.RandomState(rng_seed).permutation(N) if shuffle else np.arange(N)
    out = torch.ops.ffc.isc_sums(logits, torch.from_numpy(perm.astype(np.int64)).to(logits.device), splits)
    scores = out[:, 3]
    return {KEY_METRIC_ISC_MEAN: float(scores.mean().item()), KEY_METRIC_ISC_STD: float(scores.std(unbiased=False).item())}


PRC_MAX_NEIGHBORHOOD = 7


def prc_features_to_metric(features_1, features_2, prc_neighborhood=3, prc_batch_size=10000, save_cpu_ram=False) -> dict:
    """metric_prc.py:57-94: the improved precision and recall of Kynkaanniemi et al.  **Convention:
    ``features_1`` is the REAL set, ``features_2`` the GENERATED one** (metric_prc.py:70).  One call of ffc::prc:
    squared distances in fp64 on the device, no N x N matrix anywhere; precision = (samples of features_2 inside
    some k-NN ball of features_1) / N2, recall = (samples of features_1 inside some ball of features_2) / N1 from
    the exact integer counts, f_score = 2 p r / max(1e-5, p + r).  ``prc_batch_size`` and ``save_cpu_ram`` are
    accepted and ignored: both routes of the reference give one result, and neither of their matrices exists
    here.  ValueError where the reference asserts, for a neighborhood outside 1 .. 7 and for fewer than
    neighborhood + 1 rows (where the reference's kthvalue fails).  Features must be finite."""
    if not (torch.is_tensor(features_1) and features_1.dim() == 2 and torch.is_tensor(features_2)
            and features_2.dim() == 2 and features_1.shape[1] == features_2.shape[1]):
        raise ValueError("features must be two 2-D tensors of one width")
    k = prc_neighborhood
    if type(k) is not int or not 1 <= k <= PRC_MAX_NEIGHBORHOOD:
        raise ValueError(f"prc_neighborhood must be an integer in 1 .. {PRC_MAX_NEIGHBORHOOD}")
    n1, n2 = len(features_1), len(features_2)
    if min(n1, n2) < k + 1:
        raise ValueError(f"PRC neighborhood {k} needs at least {k + 1} samples (input_1: {n1}, input_2: {n2})")
    counts = torch.ops.ffc.prc(features_1, features_2, k)[4].cpu()
    precision, recall = float(counts[0]) / n2, float(counts[1]) / n1
    return {KEY_METRIC_PRECISION: precision, KEY_METRIC_RECALL: recall,
            KEY_METRIC_F_SCORE: 2 * precision * recall / max(1e-5, precision + recall)}


def calculate_prc(gen_model, feature_extractor, num_samples, real_features, batch_size=DEFAULT_BATCH_SIZE,
                  rng_seed=DEFAULT_RNG_SEED, prc_neighborhood=3) -> dict:
    """Precision and recall of a generator against ``real_features`` (N1, D), with the caller's feature
    extractor (torch_fidelity's default for PRC is VGG-16 ``fc2_relu``, D = 4096; its weights come by URL).
    ``feature_extractor(images_uint8) -> features_2d`` (or a tuple whose first entry they are, as
    ``calculate_metrics`` takes) is called on every batch of ``generate_batches``; then
    ``prc_features_to_metric(real_features, generated)``, that function's documented convention.

    The reference's own driver (metric_prc.py:104-112) puts input 1 first whatever it is: with a generator as
    input 1, as its trainers pass one to ``calculate_metrics``, what it reports as "precision" is this
    function's "recall" and the other way round."""
    if not (torch.is_tensor(real_features) and real_features.dim() == 2):
        raise ValueError("real_features must be a 2-D feature tensor")
    feats = []
    for images in generate_batches(gen_model, num_samples, batch_size, True, rng_seed):
        f = feature_extractor(images)
        if isinstance(f, (tuple, list)):
            f = f[0]
        feats.append(f.float().contiguous())
    return prc_features_to_metric(real_features, torch.cat(feats), prc_neighborhood=prc_neighborhood)


def _stats_of(input2, dim):
    if isinstance(input2, FeatureStats):
        return input2.statistics()
    if isinstance(input2, dict):
        return {"mu": np.asarray(input2["mu"]), "sigma": np.asarray(input2["sigma"])}
    return FeatureStats(dim, device=input2.device).update(input2).statistics()


def calculate_metrics(gen_model, feature_extractor, num_samples, input2=None, isc=True, fid=True, kid=False,
                      batch_size=DEFAULT_BATCH_SIZE, rng_seed=DEFAULT_RNG_SEED, **kid_kwargs) -> dict:
    """torch_fidelity.calculate_metrics for a generator as input 1 (fgan_complete.py:416-427), with the
    caller's feature extractor: **no Inception network is built here** (its weights come by URL).

    ``feature_extractor(images_uint8) -> (features_2d, logits_2d)`` is called on every batch of
    ``generate_batches``; the features stream into a ``FeatureStats``; features and logits are kept on
    the device only when KID or ISC needs them.  ``input2`` is a ``FeatureStats``, a {"mu", "sigma"}
    dict (what torch_fidelity caches) or a feature tensor (the only form KID accepts); ISC needs none.
    Returns the reference's keys; ``ppl`` and ``prc`` are not accepted."""
    for k in ("ppl", "prc"):
        if k in kid_kwargs:
            raise ValueError(f"{k} is not supported (its feature networks are out of scope)")
    bad = [k for k in kid_kwargs if not k.startswith("kid_")]
    if bad:
        raise TypeError(f"unexpected arguments {bad}")
    if not (isc or fid or kid):
        raise ValueError("At least one of 'isc', 'fid', 'kid' must be specified")
    if (fid or kid) and input2 is None:
        raise ValueError("fid and kid need input2")
    if kid and not torch.is_tensor(input2):
        raise ValueError("kid needs input2 as a feature tensor")
    stats, feats, logits = None, [], []
    for images in generate_batches(gen_model, num_samples, batch_size, True, rng_seed):
        f, lg = feature_extractor(images)
        if fid or kid:
            f = f.float().contiguous()
            if fid:
                if stats is None:
                    stats = FeatureStats(int(f.shape[1]), device=f.device)
                stats.update(f)
            if kid:
                feats.append(f)
        if isc:
            logits.append(lg.float())
    out = {}
    if isc:
        out.update(isc_features_to_metric(torch.cat(logits), rng_seed=rng_seed))
    if fid:
        out.update(fid_statistics_to_metric(stats.statistics(), _stats_of(input2, stats.dim)))
    if kid:
        out.update(kid_features_to_metric(torch.cat(feats), input2, rng_seed=rng_seed, **kid_kwargs))
    return out
