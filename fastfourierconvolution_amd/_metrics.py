"""Host side of ffc::feat_moments_update, ffc::kid_sums and ffc::isc_sums (csrc/metric_kernels.hip) and of ffc::prc
(csrc/prc_kernels.hip): argument checks, workspaces and the launches.  Nothing here synchronises."""
from __future__ import annotations

import torch

from . import _runtime as rt
from ._lib import check, ptr

FM_MAX_D = 2048     # the widest layer torch_fidelity reads features from
ISC_MAX_C = 1024
KID_SUMS = 6        # [sum K_XX, sum diag K_XX, sum K_YY, sum diag K_YY, sum K_XY, trace K_XY]
ISC_HEAD = 4        # [n_i, sum p log p, exponent, score] in front of the column sums
PRC_MAX_D = 4096    # VGG-16 fc2_relu, torch_fidelity's default layer for PRC
PRC_MAX_NEIGHBORHOOD = 7


def state_doubles(D: int) -> int:
    return 1 + 2 * D + D * D


def _features(t, name):
    t = rt.require(t, name)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name}: a non-empty 2-D tensor, got {tuple(t.shape)}")
    return t


def _index(t, name, dev):
    if t.dtype != torch.int64 or t.device != dev:
        raise ValueError(f"{name}: an int64 tensor on {dev}")
    return t.contiguous()


def feat_moments_update_impl(state, x):
    x = _features(x, "feat_moments_update: features")
    B, D = x.shape
    if D > FM_MAX_D:
        raise ValueError(f"feat_moments_update: D = {D} > {FM_MAX_D}")
    if state.dtype != torch.float64 or state.device != x.device or not state.is_contiguous() or \
            state.numel() != state_doubles(D):
        raise ValueError(f"feat_moments_update: state must be {state_doubles(D)} contiguous fp64 values on {x.device}")
    with rt.observe("feat_moments_update", bytes=4.0 * x.numel() + 16.0 * D * D):
        check(rt.lib().ffc_feat_moments_update(ptr(x), B, D, ptr(state), rt.stream_of(x)), "ffc_feat_moments_update")


def kid_sums_impl(f1, f2, idx1, idx2, degree, gamma, coef0):
    f1, f2 = _features(f1, "kid_sums: features_1"), _features(f2, "kid_sums: features_2")
    if f1.shape[1] != f2.shape[1] or f1.device != f2.device:
        raise ValueError("kid_sums: the two feature matrices need one width and one device")
    idx1, idx2 = _index(idx1, "kid_sums: idx1", f1.device), _index(idx2, "kid_sums: idx2", f1.device)
    if idx1.dim() != 2 or idx1.shape != idx2.shape:
        raise ValueError("kid_sums: two (subsets, m) index tables")
    S, m = idx1.shape
    L = rt.lib()
    nws = L.ffc_kid_ws_doubles(S, m)
    ws = torch.empty(max(nws, 1), device=f1.device, dtype=torch.float64)
    sums = torch.empty((S, KID_SUMS), device=f1.device, dtype=torch.float64)
    with rt.observe("kid_sums", flops=4.0 * S * m * m * f1.shape[1]):
        check(L.ffc_kid_sums(ptr(f1), f1.shape[0], ptr(f2), f2.shape[0], f1.shape[1], ptr(idx1), ptr(idx2), S, m,
                             int(degree), float(gamma), float(coef0), ptr(ws), nws, ptr(sums), rt.stream_of(f1)),
              "ffc_kid_sums")
    return sums


def prc_impl(f1, f2, neighborhood):
    """-> (radii2_1 (N1,), radii2_2 (N2,), hit_2 (N2,) int32, hit_1 (N1,) int32, counts (2,)) of ffc_prc"""
    f1, f2 = _features(f1, "prc: features_1"), _features(f2, "prc: features_2")
    if f1.shape[1] != f2.shape[1] or f1.device != f2.device:
        raise ValueError("prc: the two feature matrices need one width and one device")
    k = int(neighborhood)
    (N1, D), N2 = f1.shape, f2.shape[0]
    if not 1 <= k <= PRC_MAX_NEIGHBORHOOD:
        raise ValueError(f"prc: neighborhood = {k} out of range (1 .. {PRC_MAX_NEIGHBORHOOD})")
    if D > PRC_MAX_D:
        raise ValueError(f"prc: D = {D} > {PRC_MAX_D}")
    if min(N1, N2) < k + 1:
        raise ValueError(f"prc: N1 = {N1}, N2 = {N2} rows cannot hold {k + 1} neighbours")
    L = rt.lib()
    nws = L.ffc_prc_ws_bytes(N1, N2, k)
    if nws == 0:
        raise ValueError(f"prc: N1 = {N1} or N2 = {N2} too large")
    dev = f1.device
    ws = torch.empty(nws // 8, device=dev, dtype=torch.float64)
    r1, r2 = torch.empty(N1, device=dev, dtype=torch.float64), torch.empty(N2, device=dev, dtype=torch.float64)
    hit_2, hit_1 = torch.empty(N2, device=dev, dtype=torch.int32), torch.empty(N1, device=dev, dtype=torch.int32)
    counts = torch.empty(2, device=dev, dtype=torch.float64)
    with rt.observe("prc", flops=2.0 * D * (N1 * N1 + N2 * N2 + N1 * N2)):
        check(L.ffc_prc(ptr(f1), N1, ptr(f2), N2, D, k, ptr(r1), ptr(r2), ptr(hit_2), ptr(hit_1), ptr(counts), ptr(ws),
                        nws, rt.stream_of(f1)), "ffc_prc")
    return r1, r2, hit_2, hit_1, counts


def isc_sums_impl(logits, perm, splits):
    logits = _features(logits, "isc_sums: logits")
    N, C = logits.shape
    perm = _index(perm, "isc_sums: perm", logits.device)
    if perm.dim() != 1 or perm.numel() != N:
        raise ValueError("isc_sums: perm must have one entry per row")
    L = rt.lib()
    nws = L.ffc_isc_ws_doubles(N, C, int(splits))
    ws = torch.empty(max(nws, 1), device=logits.device, dtype=torch.float64)
    out = torch.empty((max(int(splits), 1), ISC_HEAD + C), device=logits.device, dtype=torch.float64)
    with rt.observe("isc_sums", bytes=4.0 * logits.numel()):
        check(L.ffc_isc_sums(ptr(logits), N, C, ptr(perm), int(splits), ptr(ws), nws, ptr(out), rt.stream_of(logits)),
              "ffc_isc_sums")
    return out
