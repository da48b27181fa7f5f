"""Execution layer between the drop-in modules and the C ABI.

Owns: plan caches, weight packing (re-packed only when a weight's version changes),
per-call buffers (allocated from PyTorch's caching allocator, so hipGraph capture via
torch.cuda.graph works), BatchNorm statistics (optionally all-reduced across ranks for
sharded train-mode batches) and the launches themselves.  Every launch goes to
``torch.cuda.current_stream()``.
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib, _plan
from ._lib import FFCError, check, ptr  # noqa: F401  (re-exported for the layers)

# --------------------------------------------------------------------------- device / stream


def require(t: torch.Tensor, name: str = "input") -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise FFCError(f"{name}: the FFC hot path runs only on a ROCm/HIP device (tensor is on {t.device}); "
                       "there is no CPU fallback")
    if t.dtype != torch.float32:
        raise FFCError(f"{name}: fp32 required (got {t.dtype})")
    return t.contiguous()


def stream_of(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def lib():
    return _lib.load()


def _env(var: str, default: str, parse=str):
    """value of a module-level switch: parse(the environment's ``var``, or ``default`` when unset).  The
    result is bound to a plain module attribute (tests and tools assign those); one a plan depends on is
    also named in PLAN_KNOBS below."""
    return parse(os.environ.get(var, default))


def _not0(s: str) -> bool:
    return s != "0"


# --------------------------------------------------------------------------- launch observer
class LaunchObserver:
    """Records HIP events around every library launch (on the launch stream) with a label and
    the launch's algorithmic work, for bench.py's live roofline measurement."""

    def __init__(self):
        self.records = []   # (label, start event, end event, work dict)

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for label, e0, e1, work in self.records:
            a = agg.setdefault(label, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "moved": 0.0})
            a["launches"] += 1
            a["ms"] += e0.elapsed_time(e1)
            a["flops"] += work.get("flops", 0.0)
            a["bytes"] += work.get("bytes", 0.0)
            a["moved"] += work.get("moved", work.get("bytes", 0.0))
        return agg


_OBS = {"obs": None}


def set_observer(obs):
    _OBS["obs"] = obs


class observe:
    """context manager around one launch"""

    def __init__(self, label, **work):
        self.label, self.work = label, work

    def __enter__(self):
        obs = _OBS["obs"]
        if obs is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        obs = _OBS["obs"]
        if obs is not None and exc[0] is None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            obs.records.append((self.label, self.e0, e1, self.work))
        return False


# --------------------------------------------------------------------------- SyncBN hook
_SYNC = {"group": None, "world1": False}


def set_sync_bn_group(group, even_world1: bool = False):
    """Route train-mode BN moments through torch.distributed.all_reduce (RCCL) over ``group``
    (None disables).  See fastfourierconvolution_amd.distributed.enable_sync_bn.
    ``even_world1``: keep the collective in a one-rank group (tests of the RCCL / hipGraph
    machinery on a one-GPU box); a one-rank group is otherwise skipped."""
    _SYNC["group"] = group
    _SYNC["world1"] = bool(even_world1)


def _sync_group():
    g = _SYNC["group"]
    if g is None:
        return None
    import torch.distributed as dist
    if not dist.is_initialized() or (dist.get_world_size(g) == 1 and not _SYNC["world1"]):
        return None
    return g


# --------------------------------------------------------------------------- batch norm
def bn_mode(bn: nn.BatchNorm2d):
    use_batch = bn.training or (bn.running_mean is None and bn.running_var is None)
    update = bn.training and bn.track_running_stats and bn.running_mean is not None
    return use_batch, update


def bn_momentum(bn: nn.BatchNorm2d) -> float:
    """the momentum as the library takes it: -1 for None (the cumulative average over num_batches_tracked)"""
    return -1.0 if bn.momentum is None else float(bn.momentum)


class BnArgs(NamedTuple):
    """an nn.BatchNorm2d as the C calls take it: ``args[1:]`` are the nine arguments before the outputs of
    ffc_bn_reduce_finalize and ffc_bn_finalize, and the same nine fields of ffc_bn_rf_item and ffc_bn_fold"""
    C: int
    gamma: Optional[int]
    beta: Optional[int]
    running_mean: Optional[int]
    running_var: Optional[int]
    num_batches_tracked: Optional[int]
    update: int
    momentum: float   # -1: None (the cumulative average)
    eps: float
    count_mult: float


def bn_args(bn: nn.BatchNorm2d, C: int, count_mult: float, fold: bool = False) -> BnArgs:
    """``bn`` over C channels as a BnArgs; RuntimeError when the module has another channel count.
    The running-statistics pointers are given wherever the module has the buffers: the separate
    finalize also reads them in eval mode.  ``fold`` (the record of an ffc_bn_fold, finalized inside
    its consumer kernel) gives them only when they are updated: a fold always runs on batch statistics
    and touches the buffers for nothing else, so its struct has carried them only then since the fold was
    written.  The two rules are two options of this one function on purpose; do not unify them."""
    if bn.num_features != C:
        raise RuntimeError(f"running_mean should contain {C} elements not {bn.num_features}")
    _, update = bn_mode(bn)
    stats = [None if t is None or (fold and not update) else ptr(t)
             for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    return BnArgs(C, ptr(bn.weight.detach()) if bn.weight is not None else None,
                  ptr(bn.bias.detach()) if bn.bias is not None else None, *stats, int(update),
                  bn_momentum(bn), float(bn.eps), float(count_mult))


def bn_finalize(a: BnArgs, moments, scale, shift, stream):
    """ffc_bn_finalize: (scale, shift) of ``a`` from the raw moments [C][3] {n, sum x, sum x^2}, or from
    the running statistics when ``moments`` is None"""
    check(lib().ffc_bn_finalize(ptr(moments), a.C, *a[1:6], int(moments is not None), *a[6:], ptr(scale), ptr(shift),
                                stream), "ffc_bn_finalize")


def _bn_reduce_synced(slab, nrows: int, C: int, device, stream, grp):
    """the slab's raw moments by ffc_bn_reduce, all-reduced over ``grp`` (SyncBN) -> (the buffer, its [C][3] view)"""
    from .distributed import merge_moments
    # [C][3] moments + the large-slab scratch behind them (ffc_bn_reduce_ws_doubles)
    mbuf = torch.empty(3 * C + lib().ffc_bn_reduce_ws_doubles(nrows, C), device=device, dtype=torch.float64)
    moments = mbuf[:3 * C].view(C, 3)
    check(lib().ffc_bn_reduce(ptr(slab), nrows, C, ptr(mbuf), stream), "ffc_bn_reduce")
    merge_moments(moments, group=grp)
    return mbuf, moments


def bn_scale_shift(bn: nn.BatchNorm2d, C: int, slab, nrows: int, count_mult: float, device, stream):
    """-> (scale, shift) fp32 device tensors of length C, nn.BatchNorm2d semantics."""
    a = bn_args(bn, C, count_mult)
    scale = torch.empty(C, device=device, dtype=torch.float32)
    shift = torch.empty(C, device=device, dtype=torch.float32)
    if not bn_mode(bn)[0]:
        bn_finalize(a, None, scale, shift, stream)
        return scale, shift
    grp = _sync_group()
    if grp is None:
        mbuf = torch.empty(3 * C + lib().ffc_bn_reduce_ws_doubles(nrows, C), device=device, dtype=torch.float64)
        with observe("bn_stats"):
            check(lib().ffc_bn_reduce_finalize(ptr(slab), nrows, C, ptr(mbuf), *a[1:], ptr(scale), ptr(shift), stream),
                  "ffc_bn_reduce_finalize")
    else:
        with observe("bn_stats"):
            _, moments = _bn_reduce_synced(slab, nrows, C, device, stream, grp)
            bn_finalize(a, moments, scale, shift, stream)
    return scale, shift


def _bn_finalize_batch(items, batch, device, stream):
    """single rank: the batch's reduce + finalize in one launch (ffc_bn_reduce_finalize_batch)"""
    from ._lib import BnRfItem
    arr = (BnRfItem * len(batch))()
    res, keep = {}, []
    for k, (bn, C, slab, nrows, cm) in enumerate(batch):
        a = bn_args(bn, C, cm)
        scale = torch.empty(C, device=device, dtype=torch.float32)
        shift = torch.empty(C, device=device, dtype=torch.float32)
        mbuf = torch.empty(3 * C + lib().ffc_bn_reduce_ws_doubles(nrows, C), device=device, dtype=torch.float64)
        keep.append(mbuf)
        arr[k] = BnRfItem(ptr(slab), nrows, C, ptr(mbuf), *a[1:], ptr(scale), ptr(shift))
        res[id(bn)] = (scale, shift)
    with observe("bn_stats"):
        check(lib().ffc_bn_reduce_finalize_batch(arr, len(batch), stream), "ffc_bn_reduce_finalize_batch")
    return [res[id(it[0])] if id(it[0]) in res else bn_scale_shift(it[0], it[1], it[2], it[3], it[4], device, stream)
            for it in items]


class ActApply(NamedTuple):
    """one tensor of bn_act_apply_batch: x <- act(scale * x + shift) (+ noise_w * noise), in place"""
    x: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    act: int
    param: float
    noise_w: Optional[torch.Tensor] = None
    noise: Optional[torch.Tensor] = None
    plane_sums: Optional[torch.Tensor] = None   # (B, C, ffc_plane_chunks(HW)): receives the chunk sums of y


def bn_act_apply_batch(items):
    """[ActApply] in one launch (ffc_bn_act_apply_batch; the l and g outputs of an FFC_BN_ACT, with
    fgan128's NoiseInjection)"""
    from ._lib import BnApplyItem
    arr = (BnApplyItem * len(items))()
    nbytes = 0.0
    for k, it in enumerate(items):
        B, C = it.x.shape[:2]
        HW = it.x.numel() // (B * C)
        arr[k] = BnApplyItem(ptr(it.x), ptr(it.x), B, C, HW, ptr(it.scale), ptr(it.shift), int(it.act),
                             float(it.param), ptr(it.noise_w), ptr(it.noise), ptr(it.plane_sums))
        nbytes += 8.0 * it.x.numel() + (4.0 * it.noise.numel() if it.noise is not None else 0.0)
    label = "bn_act_noise" if any(it.noise is not None for it in items) else "bn_act"
    with observe(label, bytes=nbytes):
        check(lib().ffc_bn_act_apply_batch(arr, len(items), stream_of(items[0].x)), "ffc_bn_act_apply_batch")


def bn_scale_shift_many(items, device, stream):
    """bn_scale_shift for several BNs whose slabs are ready together (an FFC layer's bn_l and bn_g,
    ffc_bn_act.py:80-83).  items: [(bn, C, slab, nrows, count_mult)] -> [(scale, shift)].  Under
    SyncBN their raw moments travel in ONE all-reduce (one collective per layer instead of one per
    BN: the per-rank step of strong scaling is latency-bound, each collective a round trip)."""
    grp = _sync_group()
    batch = [it for it in items if it[2] is not None and bn_mode(it[0])[0]]
    if len(batch) < 2 or len(batch) > 4:
        return [bn_scale_shift(bn, C, slab, nrows, cm, device, stream) for bn, C, slab, nrows, cm in items]
    if grp is None:
        return _bn_finalize_batch(items, batch, device, stream)
    from .distributed import merge_moments
    L = lib()
    recs = [bn_args(bn, C, cm) for bn, C, _, _, cm in batch]
    Cs = [it[1] for it in batch]
    # moments of every BN back to back ([sum C][3]); each reduce's scratch lies behind its own
    # moments (the later BNs' moments included: they are reduced afterwards, in stream order)
    offs = [3 * sum(Cs[:i]) for i in range(len(batch))]
    need = max(offs[i] + 3 * Cs[i] + L.ffc_bn_reduce_ws_doubles(batch[i][3], Cs[i]) for i in range(len(batch)))
    mbuf = torch.empty(need, device=device, dtype=torch.float64)
    with observe("bn_stats"):
        for (bn, C, slab, nrows, _), o in zip(batch, offs):
            check(L.ffc_bn_reduce(ptr(slab), nrows, C, ptr(mbuf[o:]), stream), "ffc_bn_reduce")
        tot = 3 * sum(Cs)
        merge_moments(mbuf[:tot].view(-1, 3), group=grp)
    res = {}
    for (bn, C, _, _, _), a, o in zip(batch, recs, offs):
        scale = torch.empty(C, device=device, dtype=torch.float32)
        shift = torch.empty(C, device=device, dtype=torch.float32)
        with observe("bn_stats"):
            bn_finalize(a, mbuf[o:], scale, shift, stream)
        res[id(bn)] = (scale, shift)
    return [res[id(it[0])] if id(it[0]) in res else bn_scale_shift(it[0], it[1], it[2], it[3], it[4], device, stream)
            for it in items]


# Train-mode BNs whose consumer kernel finalizes them in-kernel (ffc_bn_fold) instead of a
# separate ffc_bn_reduce_finalize launch: single rank only (SyncBN all-reduces the moments between
# the merge and the finalize).  FFC_BN_FOLD=0 restores the separate launch (A/B measurements).
BN_FOLD = _env("FFC_BN_FOLD", "1", _not0)
# slab rows x channels up to which the fold beats the separate launch (each consumer workgroup
# reads the whole slab; measured on MI355X, r02)
BN_FOLD_MAX = _env("FFC_BN_FOLD_MAX", "4096", int)
# the SE means of a layer's global input taken from the previous layer's BN-apply pass (plane sums
# written as it stores y) instead of a second read of y (FFC_SE_SUMS=0: se_mean_kernel)
SE_SUMS = _env("FFC_SE_SUMS", "1", _not0)


def plane_sums_for(x):
    """(sums, chunks) attached to x by the BN-apply pass that wrote it, if x is unchanged since"""
    at = getattr(x, "_ffc_plane_sums", None)
    if at is None or not SE_SUMS:
        return None
    sums, chunks, version = at
    return (sums, chunks) if x._version == version else None


# the fused ST prologue over several workgroups per sample at small batches (FFC_ST_SPLIT=0: one)
ST_SPLIT = _env("FFC_ST_SPLIT", "1", _not0)


def _pow2_floor(v: int) -> int:
    """the largest power of two <= max(v, 1) (the prologue split must divide conv1's tile count)"""
    v = max(int(v), 1)
    return 1 << (v.bit_length() - 1)


# cap, rounded to 2^k: 2 since the SE gate went thread-per-channel (B = 32: 0.1755 -> 0.1731 ms with 4
# instead of 8, profiles/r05/an; B = 64 0.2105 -> 0.2092 ms with 2 instead of 4, r05/av; r04 had
# measured them level)
# (FFC_ST_SPLIT_MAX fixes it for every batch).  Round 6: 4 at B <= 32 -- the per-rank batch of the
# 8-way strong split -- B = 32 0.1790 / 0.1798 -> 0.1771 / 0.1774 ms (8: 0.1774 / 0.1777), B = 64 level
# (profiles/r06/st)
ST_SPLIT_MAX = _env("FFC_ST_SPLIT_MAX", "", lambda s: _pow2_floor(s) if s else 0)   # 0: by batch (st_split_max)


def st_split_max(B: int) -> int:
    """the ST prologue's cap on workgroups per sample at batch B"""
    if ST_SPLIT_MAX:
        return ST_SPLIT_MAX
    return 4 if B <= 32 else 2
# ST prologue conv1 on the split-bf16 MFMA products (FFC_ST_MFMA=f32: the exact f32-input MFMA, A/B)
ST_SPLIT_MFMA = _env("FFC_ST_MFMA", "split", lambda s: s != "f32")
# the fused FU's pass 1 reads pass 0's mix output instead of recomputing it (FFC_FU_SPILL=0: recompute)
FU_SPILL = _env("FFC_FU_SPILL", "1", _not0)


class BnFoldDesc:
    """an ffc_bn_fold for ``bn`` over the partial rows ``slab`` plus the tensors it points at;
    scale / shift receive the folded affine (written by the consumer's workgroup 0)"""

    def __init__(self, bn: nn.BatchNorm2d, C: int, slab, nrows: int, count_mult: float, device, moments=None):
        a = bn_args(bn, C, count_mult, fold=True)
        self.slab = slab
        # SyncBN: the slab's raw moments, reduced and all-reduced over the ranks already ([C][3] fp64,
        # ffc_bn_fold.moments); the consumer finalizes from them
        self.moments = moments
        self.channel_only = False   # make_bn_fold(kind='channels'): too many rows for a whole-slab fold
        self.scale = torch.empty(C, device=device, dtype=torch.float32)
        self.shift = torch.empty(C, device=device, dtype=torch.float32)
        self.bn = bn
        self.struct = _lib.BnFold(ptr(slab), int(nrows), int(C), *a[1:], ptr(self.scale), ptr(self.shift), ptr(moments))

    @property
    def kind(self) -> str:
        """the bn_fold_kind this descriptor was made for"""
        return "moments" if self.moments is not None else "channels" if self.channel_only else "slab"

    def materialize(self, stream):
        """(scale, shift) by the separate reduce + finalize launch: for a ready descriptor handed to a
        Fourier unit whose route does not fold it (FourierUnitSN._run(in_fold=))"""
        if self.moments is not None:   # SyncBN: only the finalize is left (the moments are merged)
            bn_finalize(bn_args(self.bn, self.struct.C, self.struct.count_mult), self.moments, self.scale, self.shift,
                        stream)
            return self.scale, self.shift
        return bn_scale_shift(self.bn, self.struct.C, self.slab, self.struct.nrows, self.struct.count_mult,
                              self.scale.device, stream)


def bn_fold_kind(nrows: int, C: int, use_batch: bool, momentum_none: bool, lanes: Optional[int] = None,
                 consumers: int = 1) -> Optional[str]:
    """How a BN over ``nrows`` slab rows of C channels can be finalized inside its consumer kernel, from the
    switches, the sync group and the row limits alone (no tensor, no launch); None: by its own launch
    (bn_scale_shift).  Batch statistics only.
      lanes None: the whole-slab fold (every consumer workgroup merges all rows) -> 'slab', within
                  BN_FOLD_MAX rows x channels
      lanes = n:  the per-channel fold (n lanes merge one channel's rows) -> 'channels': BN_CHFOLD on,
                  momentum not None (the per-channel leaders cannot read num_batches_tracked while another
                  bumps it), at most BN_CHFOLD_LOADS rows per lane and BN_CHFOLD_READS slab rows read per
                  channel over its ``consumers`` workgroups (at fgan128's B = 512 every 64^2 C2R plane
                  workgroup re-read 1024 rows: C2R 798 -> 1046 us per step, r05l)
    SyncBN -> 'moments' for both, no row gating: the slab's raw moments are reduced and
    all-reduced first (make_bn_fold) and every consumer reads 3 doubles per channel."""
    if not (BN_FOLD and use_batch) or (lanes is not None and (not BN_CHFOLD or momentum_none)):
        return None
    if _sync_group() is not None:
        return "moments" if BN_FOLD_SYNC else None
    if lanes is None:   # every consumer workgroup merges all rows: only small slabs pay
        return "slab" if nrows * C <= BN_FOLD_MAX else None
    if -(-nrows // lanes) > BN_CHFOLD_LOADS or nrows * max(1, consumers) > BN_CHFOLD_READS:
        return None
    return "channels"


def make_bn_fold(bn: nn.BatchNorm2d, C: int, slab, nrows: int, count_mult: float, device, kind: str) -> BnFoldDesc:
    """the BnFoldDesc of a fold bn_fold_kind allowed.  'moments': ffc_bn_reduce and the all-reduce over the
    sync group (RCCL) run here, and the consumer's workgroups finalize from the merged moments, so the
    separate ffc_bn_finalize launch of the N > 1 path goes away"""
    if kind != "moments":
        d = BnFoldDesc(bn, C, slab, nrows, count_mult, device)
        d.channel_only = kind == "channels"
        return d
    bn_args(bn, C, count_mult)   # a module of another channel count is refused before anything is launched
    with observe("bn_stats"):
        mbuf, _ = _bn_reduce_synced(slab, nrows, C, device, torch.cuda.current_stream(device).cuda_stream,
                                    _sync_group())
    return BnFoldDesc(bn, C, slab, nrows, count_mult, device, moments=mbuf)


# SyncBN: reduce + all-reduce the moments, then finalize inside the consumer (ffc_bn_fold.moments)
# instead of a separate ffc_bn_finalize launch (FFC_BN_FOLD_SYNC=0: the old path, A/B)
BN_FOLD_SYNC = _env("FFC_BN_FOLD_SYNC", "1", _not0)


# Per-channel in-kernel folds (ffc::bn_fold_channels): consumers whose workgroups / waves need only
# one or a few channels (the staged Fourier unit's r2c / c2r, the fused FU's split pass 1) merge just
# those channels' slab rows -- cheap at any channel count, so the limit is the rows a lane merges.
# FFC_BN_CHFOLD=0 restores the separate finalize launches (A/B); FFC_BN_CHFOLD_LOADS: max slab rows
# per lane.
# Off by default since round 6 (FFC_BN_CHFOLD=1 turns it on): the same fold placed inside
# ffc_fu2d_r2c_mix was reproduced non-deterministic in round 6 (T of whole channels
# wrong in co-resident workgroups, 39 of 40 repeated forwards) and its mechanism is not isolated, so
# the single-rank path finalizes these BNs by their own launch (B = 32: +3 %, B = 256: neutral, r05c)
BN_CHFOLD = _env("FFC_BN_CHFOLD", "0", lambda s: s == "1")
BN_CHFOLD_LOADS = _env("FFC_BN_CHFOLD_LOADS", "16", int)
BN_CHFOLD_READS = _env("FFC_BN_CHFOLD_READS", "16384", int)
# mirrors fu_kernels.hip fu_split_on(): FFC_FU_SPLIT=0 runs the fused FU's pass 1 as one workgroup per
# sample, which folds a mix BN over its whole slab (bn_fold_block) -- a channel-only fold descriptor
# (the split pass 1's) must not reach it
FU_SPLIT = _env("FFC_FU_SPLIT", "1", lambda s: s[:1] != "0")
# fused FU pass 0 over two bin groups per sample where the library takes them (ffc_fu_kgroups, round
# 6; off unless FFC_FU_KGROUPS=2, which the library reads too -- measured neutral to slower);
# FU_KGROUPS = False keeps one workgroup per sample even then
FU_KGROUPS = True


def act_code(mod: nn.Module):
    """activation module -> (FFC_ACT_* code, parameter).  layers/ffc/ffc_bn_act.py:63-67."""
    if isinstance(mod, nn.Identity):
        return 0, 0.0
    if isinstance(mod, nn.LeakyReLU):
        return 2, float(mod.negative_slope)
    if isinstance(mod, nn.ReLU):
        return 1, 0.0
    if isinstance(mod, nn.Tanh):
        return 3, 0.0
    if isinstance(mod, nn.Sigmoid):
        return 4, 0.0
    if isinstance(mod, nn.GELU) and getattr(mod, "approximate", "none") == "none":
        return 5, 0.0
    raise NotImplementedError(f"activation {type(mod).__name__} has no fused HIP epilogue")


def bn_act_apply(x, scale, shift, act, param, out=None):
    B, C = x.shape[:2]
    HW = x.numel() // (B * C)
    out = x if out is None else out
    with observe("bn_act", bytes=8.0 * x.numel()):
        check(lib().ffc_bn_act_apply(ptr(x), ptr(out), B, C, HW, ptr(scale), ptr(shift), act, float(param),
                                     stream_of(x)), "ffc_bn_act_apply")
    return out


def bn_act_noise_apply(x, scale, shift, act, param, noise_mod, noise=None):
    """x <- act(x*scale + shift) + noise_mod.weight[c] * noise[b] in one pass (noise drawn with normal_()
    as layers/noise_injection.py:26-28 does when not given)"""
    B, C, H, W = x.shape
    if noise is None:
        noise = x.new_empty(B, 1, H, W).normal_()
    noise = require(noise, "noise")
    if tuple(noise.shape) != (B, 1, H, W):
        raise RuntimeError(f"noise must be {(B, 1, H, W)}, got {tuple(noise.shape)}")
    w = require(noise_mod.weight.detach(), "NoiseInjection.weight")
    if w.numel() != C:
        raise RuntimeError(f"NoiseInjection has {w.numel()} channels, tensor has {C}")
    with observe("bn_act_noise", bytes=8.0 * x.numel() + 4.0 * noise.numel()):
        check(lib().ffc_bn_act_noise_apply(ptr(x), ptr(x), B, C, H * W, ptr(scale), ptr(shift), act, float(param),
                                           ptr(w), ptr(noise), stream_of(x)), "ffc_bn_act_noise_apply")
    return x


class PendingAct:
    """A branch output whose BN + activation (+ NoiseInjection) has not been applied yet: the consumer
    applies it while staging its operand (ffc_in_tf), so the separate read + write pass of the whole
    tensor disappears.  ``materialize()`` runs that pass instead (for consumers without the option).
    The noise is drawn when the pending value is created, in the order the eager path draws it."""

    def __init__(self, raw, scale, shift, act, param, noise_mod=None, noise=None):
        B, C, H, W = raw.shape
        self.raw, self.scale, self.shift, self.act, self.param = raw, scale, shift, int(act), float(param)
        self.noise_w = self.noise = None
        if noise_mod is not None:
            if noise is None:
                noise = raw.new_empty(B, 1, H, W).normal_()
            noise = require(noise, "noise")
            if tuple(noise.shape) != (B, 1, H, W):
                raise RuntimeError(f"noise must be {(B, 1, H, W)}, got {tuple(noise.shape)}")
            w = require(noise_mod.weight.detach(), "NoiseInjection.weight")
            if w.numel() != C:
                raise RuntimeError(f"NoiseInjection has {w.numel()} channels, tensor has {C}")
            self.noise_w, self.noise = w, noise
        self.shape = raw.shape

    @classmethod
    def from_tensors(cls, raw, scale, shift, act, param, noise_w=None, noise=None):
        """a PendingAct from its tensors (the outputs / inputs of the deferred ffc::ffc_bn_act op)"""
        p = cls(raw, scale, shift, act, param)
        p.noise_w, p.noise = noise_w, noise
        return p

    def struct(self):
        from ._lib import InTf
        return InTf(ptr(self.scale), ptr(self.shift), self.act, self.param, ptr(self.noise_w), ptr(self.noise))

    def materialize(self):
        x = self.raw
        if self.noise is not None:
            with observe("bn_act_noise", bytes=8.0 * x.numel() + 4.0 * self.noise.numel()):
                B, C, H, W = x.shape
                check(lib().ffc_bn_act_noise_apply(ptr(x), ptr(x), B, C, H * W, ptr(self.scale), ptr(self.shift),
                                                   self.act, self.param, ptr(self.noise_w), ptr(self.noise),
                                                   stream_of(x)), "ffc_bn_act_noise_apply")
            return x
        return bn_act_apply(x, self.scale, self.shift, self.act, self.param)


def materialize(x):
    """PendingAct -> tensor (other values unchanged); tuples element-wise"""
    if type(x) is tuple:
        return tuple(materialize(v) for v in x)
    return x.materialize() if isinstance(x, PendingAct) else x


# --------------------------------------------------------------------------- packed-weight keys
# Packed forms of weights (GEMM A panels, transposed mix / conv1 / Linear weights) are cached by
# (pointer, version, epoch).  The custom ops (ops.py) are functional: the weights arrive as op
# arguments, and one op's plan cache serves every module with the same structure.  Pointer +
# version alone would then hit stale packs when a freed model's weight memory is reused by a new
# model's weight at the same version count, so each weight tensor OBJECT (the view's base for
# views) gets an epoch the first time an op sees it; a new object at a recycled address gets a
# new epoch and is re-packed.
_EPOCH = {"next": 1, "by_id": {}, "by_ptr": {}}
_EPOCH_LOCK = __import__("threading").Lock()


def note_tensors(ts):
    """register the weight tensors an op was called with (see weight_key)"""
    import weakref
    with _EPOCH_LOCK:
        by_id, by_ptr = _EPOCH["by_id"], _EPOCH["by_ptr"]
        for t in ts:
            if t is None or not isinstance(t, torch.Tensor):
                continue
            a = t._base if t._base is not None else t
            e = by_id.get(id(a))
            if e is None or e[0]() is not a:
                k = id(a)
                e = (weakref.ref(a, lambda _r, k=k: _EPOCH["by_id"].pop(k, None)), _EPOCH["next"])
                _EPOCH["next"] += 1
                by_id[k] = e
            by_ptr[t.data_ptr()] = (e[0], e[1])


def weight_key(t):
    """cache key of a weight's packed form: (pointer, version, epoch of the live tensor object noted at
    that pointer; 0 when none is alive there)"""
    if t is None:
        return None
    p = t.data_ptr()
    e = _EPOCH["by_ptr"].get(p)
    a = e[0]() if e is not None else None
    return p, t._version, e[1] if a is not None and a.data_ptr() == p else 0


def _wkey(ts):
    return tuple(weight_key(t) for t in ts)


class StreamPool:
    """Objects that own device buffers (layer templates with their plan caches, packed weights and
    split-K partials; the conv_layer plan cache) handed to ONE caller at a time.

    Concurrent callers -- nn.DataParallel-style threads, each on its own stream (SURVEY.md §8b
    "Threading", /root/reference/train_cond.py:66-68) -- get different objects, and the pool's lock
    covers only the check-out and the return, never the launches.  An object's previous holder may
    have been another thread whose kernels are still queued on ITS stream and read or write the
    object's buffers, so a caller that takes an object last used by another thread makes its current
    stream wait for that stream first.  One thread alone never records or waits on anything (graph
    capture and the timed loops are unaffected)."""

    def __init__(self, factory):
        import threading
        self._factory = factory
        self._free, self._all = [], []
        self._lock = threading.Lock()
        self._last = {}   # id(object) -> (thread id, stream) of its previous holder

    def take(self):
        import threading
        me = threading.get_ident()
        with self._lock:
            obj = self._free.pop() if self._free else None
        if obj is None:
            obj = self._factory()   # built outside the lock (only this caller can see it)
            with self._lock:
                self._all.append(obj)
        last = self._last.get(id(obj))
        if last is not None and last[0] != me:
            cur = torch.cuda.current_stream()
            if torch.cuda.is_current_stream_capturing():
                # a wait on an event recorded outside the capture invalidates it, and so does a host
                # synchronise from the capturing thread (measured r06d): nothing is done
                # here -- graphs.capture_step synchronises the device before it captures, so the
                # previous holder's kernels have retired
                pass
            else:
                cur.wait_stream(last[1])
        return obj

    def give(self, obj):
        import threading
        if torch.cuda.is_initialized():
            self._last[id(obj)] = (threading.get_ident(), torch.cuda.current_stream())
        with self._lock:
            self._free.append(obj)

    @property
    def instances(self) -> int:
        return len(self._all)

    def first(self):
        """an object of the pool for read-only inspection (built if none exists yet)"""
        with self._lock:
            if self._all:
                return self._all[0]
        obj = self.take()
        self.give(obj)
        return obj

    class _Hold:
        def __init__(self, pool):
            self.pool = pool

        def __enter__(self):
            self.obj = self.pool.take()
            return self.obj

        def __exit__(self, *exc):
            self.pool.give(self.obj)
            return False

    def hold(self):
        """``with pool.hold() as obj:`` -- obj held exclusively for the block"""
        return StreamPool._Hold(self)


class PackCache:
    """Forms derived from weights (packed, transposed, concatenated).  An entry lives in a slot and holds
    the weight_key of the sources it was built from; sources with another key (a new version, or a new
    tensor object: another epoch) re-build into the same slot, so nothing stale stays behind.  The slot is
    (tag, the sources' pointers): an updated weight, and a new tensor at a freed one's address, replace
    the old entry, while other models' weights get slots of their own.  A caller whose source is a fresh
    tensor every step, possibly at a new address (W / sigma on the training path), names the slot itself
    (``slot``: its job key).  Slots are FIFO-bounded by ``cap``."""

    def __init__(self, cap: int = 16):
        self.cap, self.d = cap, {}

    def get(self, tag, sources, build, slot=None):
        key = _wkey(sources)
        slot = (tag, slot if slot is not None else tuple(None if k is None else k[0] for k in key))
        hit = self.d.get(slot)
        if hit is None or hit[0] != key:
            if hit is None and len(self.d) >= self.cap:
                self.d.pop(next(iter(self.d)))
            hit = self.d[slot] = (key, build())
        return hit[1]


def packs_of(cache: dict) -> PackCache:
    """the PackCache kept inside a plan cache (a layer's executor cache, the conv_layer op's)"""
    p = cache.get("packs")
    if p is None:
        p = cache["packs"] = PackCache(64)
    return p


# --------------------------------------------------------------------------- convolution jobs


# The module-level switches plans and templates depend on, by name: every switch of this module, with
# or without an environment variable (tests/test_knobs_cpu.py checks that none is missing).
PLAN_KNOBS = ("USE_PATCH", "PW_KERNEL", "CONV_ARITH", "PRESPLIT_A", "USE_CONVQ", "CONVQ_FORCE", "USE_OUTER",
              "USE_SMALLM", "FORCE_FU2D", "FU_PATH", "FU_FUSED_MIN_BATCH", "FU_COLS", "FU2D_SPILL", "OVERLAP_SPECTRAL",
              "BN_FOLD", "BN_FOLD_MAX", "FU_SPILL", "ST_PATH", "ST_SPLIT", "ST_SPLIT_MAX", "SE_SUMS", "BN_CHFOLD",
              "BN_CHFOLD_LOADS", "BN_CHFOLD_READS", "ST_SPLIT_MFMA", "FU2D_R2CMIX", "FU_SPLIT", "FU_KGROUPS",
              "BN_FOLD_SYNC")


def plan_knobs():
    """the current values of PLAN_KNOBS and _plan.CONVQ_TCMAX (tests and A/B runs flip them): part of every
    plan cache key, so a changed switch never meets a plan made under another setting"""
    g = globals()
    return tuple(g[n] for n in PLAN_KNOBS) + (_plan.CONVQ_TCMAX,)


def algorithmic_flops(plan) -> float:
    """exact multiply-adds x2 of the job: every (output pixel, in-bounds tap, channel) triple"""
    total = 0
    phases = plan.phases
    for pi, ph in enumerate(phases):
        if isinstance(ph, dict):
            ent = plan.ktab[ph["kt_off"]: ph["kt_off"] + ph["K"]]
            PH, PW = ph["PH"], ph["PW"]
        else:
            ent = plan.ktab[plan.kt_off[pi]: plan.kt_off[pi] + ph.K]
            PH, PW = ph.PH, ph.PW
        for sx, oy, ox, _ in ent:
            seg = sx & 15
            if seg == 15:
                continue
            sg = plan.segs[seg]
            my_, mx_ = plan.mults[seg]
            ny = sum(1 for m in range(PH) if 0 <= m * my_ + oy < sg.IH)
            nx = sum(1 for m in range(PW) if 0 <= m * mx_ + ox < sg.IW)
            total += ny * nx
    return 2.0 * total * plan.B * plan.M


USE_PATCH = True   # LDS-patch kernel where it applies (tests flip this to cover the generic kernel)
# 1x1-only jobs of the training path: "pw" = ffc_pw_forward (tiled GEMM), "patch" / "gemm" = the
# conv kernels (A/B measurements, tests)
PW_KERNEL = _env("FFC_PW_KERNEL", "pw")


def pick_pw_cfg(B, M, Q):
    """largest ffc_pw_forward tile that still gives >= 512 workgroups (2 per CU), else the smallest"""
    cands = (0, 1, 2) if M > 64 else (1, 2)
    for c in cands:
        if lib().ffc_pw_tiles(M, B, Q, c) >= 512:
            return c
    return 2
# LDS-patch conv products: "split" = fp32-accurate split-bf16 MFMA (three exact bf16 pieces per
# operand, six piece products), "f32" = v_mfma_f32_32x32x2_f32 (A/B measurements, tests)
CONV_ARITH = _env("FFC_CONV_ARITH", "split")
PRESPLIT_A = _env("FFC_CONVP_PRESPLIT", "0", lambda s: s == "1")   # A/B knob: A3 planes (off: measured neutral / -1 %)
# stride-2 transposed-conv jobs on ffc_convq_forward (operands split once while staged, warp-specialised,
# persistent workgroups) under the split-bf16 products: taken wherever it plans ("auto" / "1" / "force");
# "0" never (convp for everything, A/B measurements).  Until r02 it lost to convp on large grids; the
# persistent grid (r03) reversed that (tools/convq_probe.py)
USE_CONVQ = _env("FFC_CONVQ", "auto", _not0)
CONVQ_FORCE = _env("FFC_CONVQ", "auto", lambda s: s in ("1", "force"))
USE_OUTER = True   # inference: ConvT on a 1x1 input as one outer-product GEMM (conv_route, _FFCExec._outer_rewrite)
USE_SMALLM = True  # direct VALU kernels for <= 4 output channels (conv_route 'convT' / 'full' / 'conv3' / 'convT3')
FORCE_FU2D = False  # large-plane FU stages even where the fused per-sample FU applies (tests)
# SpectralTransform prologue: "auto" = the fused per-sample kernel where the sample fits in LDS
# (st_prologue.hip), else SE gate + gated 1x1 GEMM (st_pw.hip); "pw" forces the latter (A/B runs)
ST_PATH = _env("FFC_ST_PATH", "auto")
# Fourier-unit path where both apply: the fused one-workgroup-per-sample kernel fills the chip only
# with B >= ~CUs/4 samples; smaller batches run the staged kernels, which spread every sample over
# many workgroups.  "auto" | "fused" | "staged".  The threshold was 128 until the fused mix ran on
# pre-split weights (r05ad); gen64 B = 64 then measured 0.2161 -> 0.2147 ms fused (r05af)
FU_PATH = _env("FFC_FU_PATH", "auto")
FU_FUSED_MIN_BATCH = 64
FU_COLS = True      # staged FU: inverse column FFT fused into mix pass 1, rows-only C2R (H in 32..128)
# staged FU, batch-statistics BN: pass 0 spills the raw Y and the whole-plane C2R applies BN + ReLU on
# load (no second mix); FFC_FU2D_SPILL=0 keeps the two-pass mix
FU2D_SPILL = _env("FFC_FU2D_SPILL", "1", _not0)
# staged FU with the spill on small t planes (h in {8, 16}, C in {16, 32}): the R2C inside mix pass 0
# (ffc_fu2d_r2c_mix: one launch instead of two); FFC_FU2D_R2CMIX=0 keeps the separate R2C
FU2D_R2CMIX = _env("FFC_FU2D_R2CMIX", "1", _not0)
# Run SpectralTransform's kernels on a side stream beside the local-branch GEMM of the same FFC
# layer ("gemm-first" / "spectral-first": which is issued first).  Off by default: measured on
# MI355X (B=256 generator) 10-18 % slower than one launch pairing the local and global GEMMs,
# because the FU / ST kernels' LDS footprint cannot co-reside with the GEMM workgroups and the
# separate GEMM launches lose the heavy/light tile pairing.
OVERLAP_SPECTRAL = _env("FFC_OVERLAP", "off", lambda s: False if s in ("0", "off", "false") else s)

_SIDE = {}


def side_stream(device):
    """one side stream per device (created once, outside any graph capture of later steps)"""
    key = str(device)
    s = _SIDE.get(key)
    if s is None:
        s = _SIDE[key] = torch.cuda.Stream(device=device)
    return s


class ConvWeight(NamedTuple):
    """one segment's weight: layout 0 = (M, C, kh, kw) (nn.Conv2d), 1 = (C, M, kh, kw) (nn.ConvTranspose2d)"""
    w: torch.Tensor
    layout: int
    kh: int
    kw: int
    bias: Optional[torch.Tensor]


def conv_weights(weights):
    """-> [ConvWeight]; callers outside the package may pass plain (w, layout, kh, kw, bias) tuples"""
    return [w if isinstance(w, ConvWeight) else ConvWeight(*w) for w in weights]


# ----- the route of a convolution job: a direct kernel, or the implicit-GEMM kernels
class RouteCaps:
    """channel caps of the direct kernels: their argument checks refuse more, so conv_route never sends it
    (constants of the kernels, not switches: tests/test_route_cpu.py compares them with the sources)"""
    CONVT_SMALLM_CMAX = 256   # CT_CMAX in csrc/convt_smallm.hip (ffc_convt_k4s2_smallm: both segments' channels)
    CONV3_SMALLM_CMAX = 256   # CMAX3 in csrc/convt_smallm.hip (ffc_conv3x3_smallm: both segments' channels)
    DENSE_KMAX = 256          # DN_KMAX in csrc/dense.hip (ffc_dense_forward: the A tile's K staged in LDS)
    CONVT3_SMALLM_CMAX = 256  # CT3_CMAX in csrc/convt3_smallm.hip (ffc_convt3x3_smallm and its data gradient)


INFER_ROUTES = frozenset(("convT", "full", "conv3", "dense", "convT3"))
# _autograd.conv_forward has never sent a job to the 3x3 kernel (its 3x3 jobs run on the implicit-GEMM
# kernels); that answer is kept
TRAIN_ROUTES = frozenset(("convT", "full", "dense", "convT3"))


def conv_route(segs, weights, M, has_addend, has_bn, accept, training=False):
    """The kernel for out = act(sum_s conv_s(x_s)) with M output channels and ConvWeight ``weights``, among
    the routes the caller accepts.  Looks at shapes only (no tensor data, no device).
    -> None: the implicit-GEMM kernels, or
      'convT'  <= 4 output channels, ConvTranspose2d k4 s2 p1 (the generator's last layer): ffc_convt_k4s2_smallm
      'full'   <= 4 output channels, Conv2d onto a 1x1 output (FFCDiscriminator's last layer): ffc_conv_full_smallm
      'conv3'  <= 4 output channels, Conv2d k3 s1 p1 on rows of 4n pixels (the fgan128 head): ffc_conv3x3_smallm
      'convT3' <= 4 output channels, one ConvTranspose2d k3 s1 p1 segment on rows of any width (the head of the
               baseline generators): ffc_convt3x3_smallm; its data gradient is ffc_convt3x3_smallm_dgrad
      'dense'  ConvTranspose2d(k, s=1, p=0) on a 1x1 input (the generators' first layer), a plain GEMM
               out (B, M k k) = x (B, C) . W (C, M k k): ffc_dense_forward
    No direct kernel adds an addend, collects BN partials, pools or gates its input, or takes two biases.
    ``training`` marks the two points where the callers' launchers differ (below)."""
    if has_addend or has_bn or M is None or not segs or any(sg.pool or sg.gate for sg in segs):
        return None
    layouts = {w.layout for w in weights}
    C = sum(sg.C for sg in segs)
    one_plane = all((sg.IH, sg.IW) == (segs[0].IH, segs[0].IW) for sg in segs)
    route = None
    if USE_SMALLM and M <= 4 and len(segs) <= 2 and sum(w.bias is not None for w in weights) <= 1:
        if all(sg.kind == "convT" and (sg.k, sg.s, sg.p, sg.d, sg.op) == (4, 2, 1, 1, 0) for sg in segs):
            if one_plane and layouts == {1} and C <= RouteCaps.CONVT_SMALLM_CMAX:
                route = "convT"
        elif all(sg.kind == "conv" and sg.k == sg.IH == sg.IW and sg.p == 0 and sg.d == 1 for sg in segs):
            # segments of two plane sizes: the kernel takes them (K0, K1) and the training path sends them;
            # the inference executor never did (one kernel size per layer: it cannot meet them).  Both kept
            if layouts == {0} and (one_plane or training):
                route = "full"
        elif all(sg.kind == "conv" and (sg.k, sg.s, sg.p, sg.d) == (3, 1, 1, 1) for sg in segs):
            if one_plane and segs[0].IW % 4 == 0 and C <= RouteCaps.CONV3_SMALLM_CMAX:
                route = "conv3"
        elif len(segs) == 1 and segs[0].kind == "convT" and \
                (segs[0].k, segs[0].s, segs[0].p, segs[0].d, segs[0].op) == (3, 1, 1, 1, 0):
            if layouts == {1} and C <= RouteCaps.CONVT3_SMALLM_CMAX:
                route = "convT3"
    sg = segs[0]
    if route is None and len(segs) == 1 and sg.kind == "convT" and layouts == {1} and C <= RouteCaps.DENSE_KMAX and \
            (sg.IH, sg.IW, sg.s, sg.p, sg.d, sg.op) == (1, 1, 1, 0, 1, 0):
        # inference repeats the bias over the k x k taps (_FFCExec._outer_rewrite) and honours USE_OUTER;
        # the training launcher passes W as it is, so it takes bias-free jobs only, and it never looked
        # at USE_OUTER (a switch of the inference executor's rewrite): each caller's answer is kept
        if (weights[0].bias is None) if training else USE_OUTER:
            route = "dense"
    return route if route in accept else None


# ----- the route of a Fourier unit: which kernels run it, and who finalizes which BatchNorm
class InBn(NamedTuple):
    """the BatchNorm in front of a Fourier unit (SpectralTransform.bn1) as fu_route looks at it"""
    nrows: int              # rows of its statistics slab
    count_mult: float
    use_batch: bool
    momentum_none: bool
    consumers_other: bool = False   # something beside the Fourier unit reads it (run_lfu: the LFU gather)
    ready: Optional[str] = None     # BnFoldDesc.kind of a descriptor the caller built already (_run(in_fold=))


class FuRoute(NamedTuple):
    """what one FourierUnitSN call launches (fu_route).  Fields a path does not have are None / False."""
    path: str                   # 'fused' (csrc/fu_kernels.hip, a workgroup per sample) | 'staged' (csrc/fu2d_kernels.hip)
    stats: bool                 # the unit's own BN runs on batch statistics: a pass 0 fills its slab
    in_fold: Optional[str]      # the input BN folded into the first kernel, as a make_bn_fold kind: 'slab' |
    #                             'channels' | 'moments'; None: scale / shift come from their own launch
    kgroups: int = 1                   # fused pass 0: bin groups per sample
    spill: bool = False                # pass 0 keeps its mix output Y for the last kernel
    mix3: bool = False                 # fused: the mix weight's pre-split bf16 pieces (C % 8 == 0)
    mix_fold: Optional[str] = None     # fused: the unit's BN folded into pass 1: 'split' (per channel) | 'slab'
    split_lanes: Optional[int] = None  # fused: the lanes per channel the split pass 1's fold was asked for
    r2c_mix: bool = False              # staged: the R2C inside mix pass 0 (ffc_fu2d_r2c_mix)
    mix1: Optional[str] = None         # staged: mix pass 1, 'cols' (inverse column FFT fused in) | 'plain'; None: spilled
    c2r: Optional[str] = None          # staged: 'fold' | 'bn' (BN on load, folded / given) | 'rows' | 'plain'
    bn_kind: Optional[str] = None      # the make_bn_fold kind behind mix_fold / c2r == 'fold'


def fu_route(B, C, H, W, up, mix_precision, use_batch, momentum_none, in_bn: Optional[InBn] = None) -> FuRoute:
    """The launches of a Fourier unit over (B, C, H, W) planes (``up``: the x2 upsample folded into its loads)
    whose BN has ``use_batch`` / ``momentum_none``, behind the BatchNorm ``in_bn`` (or none).  Looks at shapes,
    the switches of this module, the sync group and the library's host-side capability queries; allocates
    and launches nothing.  Raises NotImplementedError for a plane neither path runs."""
    L = lib()
    fused = L.ffc_fu_supported(C, H, W, up) == 1 and not FORCE_FU2D
    staged_ok = bool(L.ffc_fu2d_supported(C, H, W, up))
    f16 = mix_precision == "fp16"
    if f16:
        if not (staged_ok and C in (16, 32, 64)):
            raise NotImplementedError(f"fp16 mix: staged FU with C in {{16, 32, 64}} only; got C={C}, {H}x{W}")
        fused = False
    if fused and staged_ok and (FU_PATH == "staged" or (FU_PATH == "auto" and B < FU_FUSED_MIN_BATCH)):
        fused = False
    if not fused and not staged_ok:
        raise NotImplementedError(f"Fourier unit supports H,W in {{4,8,16,32}}, square 24x24, or 48x48 as "
                                  f"the x2-upsampled output of a SpectralTransform (up = 2), with "
                                  f"16*C*H*(W/2+1) <= 160 KiB (fused), "
                                  f"or square H=W in {{16,32,64,128}} with 2C <= 128 (staged); "
                                  f"got C={C}, {H}x{W}")
    # the fused kernel's planes hold the in-kernel BN fold's scratch (csrc/bn_common.h)
    fold_ok = 16 * C * H * (W // 2 + 1) >= 8 * 3 * 512 // 4
    # the input BN as its producer would fold it: over the whole slab, else channel by channel (the staged
    # r2c's fold); with a second consumer it is finalized by its own launch
    k1 = None
    if in_bn is not None and in_bn.ready is not None:
        k1 = in_bn.ready
    elif in_bn is not None and in_bn.use_batch and not in_bn.consumers_other:
        k1 = (bn_fold_kind(in_bn.nrows, C, True, in_bn.momentum_none) or
              bn_fold_kind(in_bn.nrows, C, True, in_bn.momentum_none, lanes=64))
    if fused:
        # pass 0 folds over the whole slab only (a channel fold is not taken: its own launch), and only the
        # moments fold does without the scratch in the planes; no pass 0 in eval mode, so nothing folds
        in_fold = k1 if use_batch and (k1 == "moments" or (k1 == "slab" and fold_ok)) else None
        mix3 = L.ffc_fu_mix3_elems(C) != 0
        kg, mix_fold, lanes, kind = 1, None, None, None
        if use_batch:
            # two bin groups per sample where the library takes them (ffc_fu_kgroups); slab rows = B x groups
            kg = L.ffc_fu_kgroups(B, C, H, W) if (FU_KGROUPS and FU_SPILL and mix3) else 1
            rows = L.ffc_fu_slab_rows(B, C, H, W, kg)
            if FU_SPLIT and FU_SPILL and H == W and H in (8, 16, 32) and C % (64 // H) == 0:
                # the split pass 1 (one wave per 64 / H channels) folds its 2 * 64 / H channels itself
                lanes = 64 // (2 * 64 // H)
                kind = bn_fold_kind(rows, 2 * C, True, momentum_none, lanes=lanes)
                mix_fold = "split" if kind else None
            if mix_fold is None and fold_ok:
                kind = bn_fold_kind(rows, 2 * C, True, momentum_none)
                mix_fold = "slab" if kind else None
        return FuRoute("fused", use_batch, in_fold, kgroups=kg, spill=bool(use_batch and FU_SPILL), mix3=mix3,
                       mix_fold=mix_fold, split_lanes=lanes, bn_kind=kind)
    # staged: the r2c folds channel by channel, one plane workgroup per (sample, channel): a whole-slab
    # answer is asked again as a channel fold over B consumers, where the fused path above refuses the
    # channel fold outright (each answer as the two paths gave it); moments merged over the ranks are
    # finalized per channel, which needs a momentum
    if k1 == "moments":
        in_fold = None if in_bn.momentum_none else "moments"
    else:
        in_fold = bn_fold_kind(in_bn.nrows, C, True, in_bn.momentum_none, lanes=64, consumers=B) if k1 else None
    spill = bool(use_batch and FU2D_SPILL)
    r2c_mix = bool(spill and FU2D_R2CMIX and not f16 and L.ffc_fu2d_r2c_mix_supported(C, H, W, up))
    if spill:   # the unit's BN finalized inside the C2R (two channels per plane) where the rows allow
        kind = bn_fold_kind(L.ffc_fu2d_slab_rows(B, C, H, W), 2 * C, True, momentum_none, lanes=64, consumers=B)
        return FuRoute("staged", True, in_fold, spill=True, r2c_mix=r2c_mix, c2r="fold" if kind else "bn", bn_kind=kind)
    cols = bool(FU_COLS and L.ffc_fu2d_cols_supported(C, H, W, up, int(f16)))
    return FuRoute("staged", use_batch, in_fold, mix1="cols" if cols else "plain", c2r="rows" if cols else "plain")


def st_conv1_route(B, Cin, H, W, pool, hid, c) -> str:
    """SpectralTransform's conv1 over a (B, Cin, H, W) input (``pool``: behind the 2x2 average pool; ``hid``:
    the SE block's hidden width; c output channels):
      'prologue'  one fused launch, [pool] -> SE gate -> conv1 -> BN partials, where a sample fits in LDS
      'pw_gate'   SE gate, then conv1 with the gate folded into the per-sample weights (csrc/st_pw.hip)
      'gemm'      SE gate, then the implicit-GEMM kernels (the pooled input, or channels over st_pw's LDS)"""
    L = lib()
    if ST_PATH != "pw" and L.ffc_st_prologue_lds_bytes(Cin, H, W, int(pool), hid, c) > 0:
        return "prologue"
    return "pw_gate" if not pool and L.ffc_pw_gate_lds_bytes(Cin, c) > 0 else "gemm"


def smallm_forward(route, segs, weights, xs, M, B, act, stream, packs=None, pack_slot=None, tfs=None):
    """launch the direct kernel of a 'convT' / 'full' / 'conv3' / 'convT3' job (conv_route) -> out.
    packs, pack_slot: the PackCache (and its slot, see there) for the convT kernel's packed weights;
    tfs: per input, the PendingAct whose
    BN + activation (+ noise) the 3x3 kernel applies as it stages that input (or None)"""
    L = lib()
    dev = xs[0].device
    x1 = xs[1] if len(xs) > 1 else None
    w0, w1 = weights[0].w, (weights[1].w if len(weights) > 1 else None)
    bias = next((w.bias for w in weights if w.bias is not None), None)
    C0, C1 = segs[0].C, (segs[1].C if x1 is not None else 0)
    IH, IW = segs[0].IH, segs[0].IW
    a, ap = act[0], float(act[1])
    if route == "full":
        out = torch.empty((B, M, 1, 1), device=dev, dtype=torch.float32)
        K0 = C0 * segs[0].k * segs[0].k
        K1 = C1 * segs[1].k * segs[1].k if x1 is not None else 0
        with observe("conv_full_smallm", flops=2.0 * B * M * (K0 + K1)):
            check(L.ffc_conv_full_smallm(ptr(xs[0]), K0, ptr(w0), ptr(x1), K1, ptr(w1), ptr(bias), B, M, ptr(out),
                                         a, ap, stream), "ffc_conv_full_smallm")
        return out
    if route == "convT":
        def pack():   # [C0 + C1][16 taps][4] by a HIP kernel
            wp = torch.empty(L.ffc_convt_smallm_pack_floats(C0, C1), device=dev, dtype=torch.float32)
            check(L.ffc_convt_smallm_pack(ptr(w0), C0, ptr(w1), C1, M, ptr(wp), stream), "ffc_convt_smallm_pack")
            return wp
        wp = packs.get("ctpack", [w0, w1], pack, slot=pack_slot)
        out = torch.empty((B, M, 2 * IH, 2 * IW), device=dev, dtype=torch.float32)
        with observe("convt_smallm", flops=2.0 * B * M * (C0 + C1) * 4 * (2 * IH) * (2 * IW)):
            check(L.ffc_convt_k4s2_smallm(ptr(xs[0]), C0, ptr(x1), C1, ptr(wp), ptr(bias), B, IH, IW, M, ptr(out),
                                          a, ap, stream), "ffc_convt_k4s2_smallm")
        return out
    out = torch.empty((B, M, IH, IW), device=dev, dtype=torch.float32)
    if route == "convT3":   # the raw (C, M, 3, 3) weight as it stands: nothing to pack
        with observe("convt3_smallm", flops=2.0 * B * M * C0 * 9 * IH * IW):
            check(L.ffc_convt3x3_smallm(ptr(xs[0]), C0, ptr(w0), ptr(bias), B, IH, IW, M, ptr(out), a, ap, stream),
                  "ffc_convt3x3_smallm")
        return out
    head = (ptr(xs[0]), C0, ptr(w0), ptr(x1), C1, ptr(w1), ptr(bias), B, IH, IW, M, ptr(out), a, ap)
    with observe("conv3_smallm", flops=2.0 * B * M * (C0 + C1) * 9 * IH * IW):
        if tfs is not None and any(t is not None for t in tfs):
            st = [t.struct() if t is not None else None for t in tfs] + [None]
            check(L.ffc_conv3x3_smallm_tf(*head, None if st[0] is None else ctypes.byref(st[0]),
                                          None if st[1] is None else ctypes.byref(st[1]), stream),
                  "ffc_conv3x3_smallm_tf")
        else:
            check(L.ffc_conv3x3_smallm(*head, stream), "ffc_conv3x3_smallm")
    return out


def convt3_dgrad(dpre, w, x_shape, stream):
    """data gradient of a 'convT3' job: dx (B, C, H, W) from dpre (B, M, H, W) and the raw weight (C, M, 3, 3)"""
    B, C, H, W = x_shape
    M = dpre.shape[1]
    dx = torch.empty((B, C, H, W), device=dpre.device, dtype=torch.float32)
    with observe("convt3_dgrad", flops=2.0 * B * M * C * 9 * H * W):
        check(lib().ffc_convt3x3_smallm_dgrad(ptr(dpre), ptr(w), B, C, H, W, M, ptr(dx), stream),
              "ffc_convt3x3_smallm_dgrad")
    return dx


def dense_forward(x, Wt, bias, B, K, N, N0, out0, out1, act, stream):
    """ffc_dense_forward: act(x (B, K) . Wt (K, N) + bias), columns [0, N0) to out0 and the rest to out1"""
    with observe("dense", flops=2.0 * B * K * N):
        check(lib().ffc_dense_forward(ptr(x), ptr(Wt), ptr(bias), B, K, N, N0, ptr(out0), ptr(out1), act[0],
                                      float(act[1]), stream), "ffc_dense_forward")


class ConvExec:
    """One planned + packed job: output = sum of segment convolutions of fixed shapes.

    kind 'patch' -> ffc_convp_forward (LDS input patch, all phases per workgroup),
    kind 'gemm'  -> ffc_conv_forward (generic phase GEMM with gathered B)."""

    def __init__(self, B, M, segs, weights, device, pw_ok=False, convq_cfg=None):
        weights = conv_weights(weights)
        pw_only = all(sg.kind == "pw" and not sg.pool and not sg.gate for sg in segs)
        pp = (_plan.pick_patch_cfg(B, M, segs, 128 if CONV_ARITH == "split" else 512)
              if USE_PATCH and not (pw_only and PW_KERNEL == "gemm") else None)
        if USE_PATCH and USE_CONVQ and CONV_ARITH == "split" and not pw_only and convq_cfg is not None:
            pp = _plan.plan_convq_job(B, M, segs, convq_cfg) or pp   # the launch group's common cfg
        elif USE_PATCH and USE_CONVQ and CONV_ARITH == "split" and not pw_only:
            # persistent convq (r03) measured faster than convp on every timed stride-2 shape, large
            # grids included (profiles/r03/r03g_probe_fgan128_*.log); convp stays for what it cannot plan
            pp = _plan.pick_convq_cfg(B, M, segs) or pp
        if pw_ok and pw_only and PW_KERNEL == "pw":
            self.kind, self.plan = "pw", _plan.plan_job(B, M, segs)
            self.launch_key = ("pw", pick_pw_cfg(B, M, self.plan.OH * self.plan.OW))
        elif pp is not None:
            self.kind, self.plan = "patch", pp
            self.launch_key = ("q" if pp.q else "patch", pp.cfg)
        else:
            self.kind, self.plan = "gemm", _plan.plan_job(B, M, segs)
            self.launch_key = ("gemm",)
        self.device = device
        self.ktab = torch.from_numpy(self.plan.ktab.copy()).to(device)
        # + tail padding: the patch kernel loads all 4 tap groups of a chunk, used or not
        self.a_floats = max(1, self.plan.a_size) + 256
        # split-bf16 patch conv: A pre-split into three exact bf16 planes (ffc_split_bf16) after every
        # pack, so the kernel loads the pieces instead of splitting each chunk's A in registers
        self.a3_stride = -(-self.a_floats // 8) * 8
        self.use_a3 = self.kind == "patch" and CONV_ARITH == "split" and (PRESPLIT_A or self.plan.q)
        self.has_bias = any(w.bias is not None for w in weights)
        self.M = M
        # packed buffers per weight identity: modules of one structure share this plan,
        # and alternating them must neither re-pack every call nor overwrite a buffer in use
        self._slots = {}   # identity -> (key, A, A3, bias)
        self._packed = None
        self.A = self.A3 = self.bias = None
        self.flops = algorithmic_flops(self.plan)
        self.ensure_packed(weights)

    PACK_SLOTS = 4   # distinct weight sets kept packed per plan

    def _new_buffers(self):
        A = torch.zeros(self.a_floats, device=self.device, dtype=torch.float32)
        A3 = torch.zeros(3 * self.a3_stride, device=self.device, dtype=torch.int16) if self.use_a3 else None
        bias = torch.empty(self.M, device=self.device, dtype=torch.float32) if self.has_bias else None
        return A, A3, bias

    def check_launch(self, inputs, out, addend=None):
        """host-side launch guard: the tensors must have exactly the extents this plan was made for.
        The C ABI takes raw pointers and cannot check them, so a plan reused for another shape (a
        cache-key collision: DESIGN.md §10b) would write past ``out`` instead of failing."""
        pl = self.plan
        want = (pl.B, pl.M, pl.OH, pl.OW)

        def fits(t, n):   # (B, ...) fp32, dense, exactly n elements (a view such as (B, M, k, k) for
            return (t.dim() >= 1 and t.shape[0] == pl.B and t.numel() == n and t.is_contiguous()   # (B, M k k, 1, 1)
                    and t.dtype == torch.float32)
        n_out = pl.B * pl.M * pl.OH * pl.OW
        if not fits(out, n_out):
            raise FFCError(f"conv launch guard: output {tuple(out.shape)} ({out.dtype}, contiguous="
                           f"{out.is_contiguous()}) does not match the plan's {want}")
        if addend is not None and not fits(addend, n_out):
            raise FFCError(f"conv launch guard: addend {tuple(addend.shape)} does not match the plan's {want}")
        if len(inputs) != len(pl.segs):
            raise FFCError(f"conv launch guard: {len(inputs)} inputs for {len(pl.segs)} segments")
        for i, ((x, gate), sg) in enumerate(zip(inputs, pl.segs)):
            n_in = pl.B * sg.C * sg.IH * sg.IW * (4 if sg.pool else 1)   # pooled: the 2x2-pool input
            if not fits(x, n_in):
                raise FFCError(f"conv launch guard: segment {i} input {tuple(x.shape)} (contiguous="
                               f"{x.is_contiguous()}) does not match the plan's ({pl.B}, {sg.C}, "
                               f"{sg.IH * (2 if sg.pool else 1)}, {sg.IW * (2 if sg.pool else 1)})")
            if gate is not None and gate.numel() != pl.B * sg.C:
                raise FFCError(f"conv launch guard: segment {i} gate has {gate.numel()} values, "
                               f"the plan needs {pl.B * sg.C}")

    def pack_job(self):
        """ffc_conv_job describing the packed-weight layout (used by ffc_conv_pack for both kinds)"""
        pl = self.plan
        job = _lib.ConvJob()
        job.nseg = len(pl.segs)
        job.nphase = len(pl.phases)
        job.B, job.M, job.Mpad, job.OH, job.OW, job.Sy, job.Sx = pl.B, pl.M, pl.Mpad, pl.OH, pl.OW, pl.Sy, pl.Sx
        for i, (sg, (my, mx)) in enumerate(zip(pl.segs, pl.mults)):
            sgs = job.seg[i]
            sgs.C, sgs.IH, sgs.IW, sgs.mult_y, sgs.mult_x, sgs.pool = sg.C, sg.IH, sg.IW, my, mx, int(sg.pool)
        for i, ph in enumerate(pl.phases):
            p = job.ph[i]
            if isinstance(ph, dict):
                p.py, p.px, p.PH, p.PW, p.K, p.Kpad = ph["py"], ph["px"], ph["PH"], ph["PW"], ph["K"], ph["Kpad"]
                p.a_off, p.kt_off = ph["a_off"], ph["kt_off"]
            else:
                p.py, p.px, p.PH, p.PW, p.K, p.Kpad = ph.py, ph.px, ph.PH, ph.PW, ph.K, ph.Kpad
                p.a_off, p.kt_off = pl.a_off[i], pl.kt_off[i]
        job.A = self.A.data_ptr()
        job.ktab = self.ktab.data_ptr()
        job.bias = self.bias.data_ptr() if self.bias is not None else None
        return job

    def base_job(self):
        if self.kind in ("gemm", "pw"):
            return self.pack_job()
        pl = self.plan
        job = _lib.ConvPJob()
        job.nseg = len(pl.segs)
        job.nphase = len(pl.phases)
        job.B, job.M, job.Mpad, job.OH, job.OW, job.Sy, job.Sx = pl.B, pl.M, pl.Mpad, pl.OH, pl.OW, pl.Sy, pl.Sx
        job.NS, job.TR, job.TC, job.nrb, job.ncb = pl.NS, pl.TR, pl.TC, pl.nrb, pl.ncb
        for i, sg in enumerate(pl.segs):
            s = job.seg[i]
            s.C, s.Cpad, s.IH, s.IW = sg.C, pl.cpad[i], sg.IH, sg.IW
            s.mult_y, s.mult_x = pl.mults[i]
            s.org_y, s.org_x = pl.org[i]
            s.PR, s.PC = pl.prc[i][0], pl.rowlen[i]
            s.pool = int(sg.pool)
            s.vec4 = int(pl.vec4[i])
            s.cc = pl.cc[i]
            s.direct = int(pl.direct[i]) if pl.q else 0
            if pl.q:
                s.qrow, s.qsample = pl.qstride[i]
        for i, ph in enumerate(pl.phases):
            p = job.ph[i]
            p.py, p.px, p.PH, p.PW, p.Kpad, p.a_off = ph["py"], ph["px"], ph["PH"], ph["PW"], ph["Kpad"], ph["a_off"]
            for si in range(len(pl.segs)):
                p.T[si], p.kseg[si], p.tap_h[si] = ph["T"][si], ph["kseg"][si], ph["tap_h"][si]
                for t in range(min(ph["T"][si], 8)):
                    p.tap[si][t] = int(pl.taptab[ph["tap_base"][si] + t])
        job.A = self.A.data_ptr()
        job.bias = self.bias.data_ptr() if self.bias is not None else None
        if self.A3 is not None:
            job.A3, job.a3_stride = self.A3.data_ptr(), self.a3_stride
        return job

    def ensure_packed(self, weights):
        weights = conv_weights(weights)
        key = _wkey([w.w for w in weights] + [w.bias for w in weights])
        if key == self._packed:
            return
        # identity = the weight objects (pointer, epoch) without their versions: an updated weight
        # re-packs into its own slot, another model's weights get a slot of their own
        ident = tuple(None if k is None else (k[0], k[2]) for k in key)
        slot = self._slots.pop(ident, None)
        if slot is not None and slot[0] == key:
            self._slots[ident] = slot
            _, self.A, self.A3, self.bias = slot
            self._packed = key
            return
        if slot is not None:
            bufs = slot[1:]
        elif len(self._slots) >= self.PACK_SLOTS:
            bufs = self._slots.pop(next(iter(self._slots)))[1:]   # oldest slot's buffers
        else:
            bufs = self._new_buffers()
        self.A, self.A3, self.bias = bufs
        self._slots[ident] = (key,) + tuple(bufs)
        n = len(weights)
        job = self.pack_job()
        wp = (ctypes.c_void_p * _lib.MAX_SEG)(*[w.w.data_ptr() for w in weights], *([None] * (_lib.MAX_SEG - n)))
        lay = (ctypes.c_int * _lib.MAX_SEG)(*[w.layout for w in weights], *([0] * (_lib.MAX_SEG - n)))
        kh = (ctypes.c_int * _lib.MAX_SEG)(*[w.kh for w in weights], *([1] * (_lib.MAX_SEG - n)))
        kw = (ctypes.c_int * _lib.MAX_SEG)(*[w.kw for w in weights], *([1] * (_lib.MAX_SEG - n)))
        bp = (ctypes.c_void_p * _lib.MAX_SEG)(*[ptr(w.bias) for w in weights], *([None] * (_lib.MAX_SEG - n)))
        check(lib().ffc_conv_pack(ctypes.byref(job), wp, lay, kh, kw, bp, self.A.data_ptr(),
                                  ptr(self.bias), torch.cuda.current_stream(self.device).cuda_stream),
              "ffc_conv_pack")
        if self.A3 is not None and self.plan.q:
            # fragment-ordered split planes (one coalesced 1 KiB load per A fragment piece)
            check(lib().ffc_convq_pack_a3(ctypes.byref(self.base_job()), self.A.data_ptr(), self.A3.data_ptr(),
                                          torch.cuda.current_stream(self.device).cuda_stream), "ffc_convq_pack_a3")
        elif self.A3 is not None:
            check(lib().ffc_split_bf16(self.A.data_ptr(), self.A.numel(), self.A3.data_ptr(), self.a3_stride,
                                       torch.cuda.current_stream(self.device).cuda_stream), "ffc_split_bf16")
        self._packed = key

    def job(self, inputs, out, act=0, act_param=0.0, addend=None, stats=None):
        self.check_launch(inputs, out, addend)
        job = self.base_job()
        for i, (x, gate) in enumerate(inputs):
            if self.kind == "patch" and self.plan.vec4[i] and x.data_ptr() % 16:
                raise FFCError("patch conv: input segment is not 16-byte aligned")
            job.seg[i].x = x.data_ptr()
            job.seg[i].gate = ptr(gate)
        job.out = out.data_ptr()
        job.addend = ptr(addend)
        job.stats = ptr(stats)
        job.act = act
        job.act_param = act_param
        return job


class LaunchPlan:
    """tile table for a set of jobs of the same kind launched together"""

    def __init__(self, execs, device):
        kinds = {e.launch_key for e in execs}
        if len(kinds) != 1:
            raise ValueError("jobs of one launch must share a kernel configuration")
        self.key = kinds.pop()
        if self.key[0] == "pw":
            self.cfg = self.key[1]
            self._rows = [0 for _ in execs]
            self.ntiles = sum(lib().ffc_pw_tiles(e.plan.M, e.plan.B, e.plan.OH * e.plan.OW, self.cfg) for e in execs)
            self.tiles = None
            return
        self.ksplit, self.part, self.slots, self.nslots = 1, None, None, 0
        if self.key[0] in ("patch", "q"):
            self.cfg = self.key[1]
            if self.key[0] == "q":   # one K split for the launch's jobs (small batches: fill the CUs)
                self.ksplit = _plan.pick_convq_ksplit_group([e.plan for e in execs])
            tiles = _plan.build_patch_tiles([e.plan for e in execs], ksplit=self.ksplit)
            self._rows = [e.plan.npb * 4 for e in execs]
            if self.ksplit > 1:   # partial fragments, added by the reduce launch of ffc_convq_forward_split
                slots = _plan.convq_slot_tiles(tiles)
                self.nslots = slots.shape[0]
                n = lib().ffc_convq_split_floats(self.cfg, self.nslots, self.ksplit)
                if n <= 0:
                    raise RuntimeError("ffc_convq_split_floats: bad configuration")
                self.part = torch.empty(n, device=device, dtype=torch.float32)
                self.slots = torch.from_numpy(slots).to(device)
        else:
            self.cfg = _plan.pick_tile_cfg([e.plan.M for e in execs])
            tiles, nslots = _plan.build_tiles([e.plan for e in execs], self.cfg)
            while tiles.shape[0] < 256 and self.cfg == 0:   # too few tiles to fill 256 CUs: halve BM
                self.cfg = 1
                tiles, nslots = _plan.build_tiles([e.plan for e in execs], self.cfg)
            rpt = _plan.TILE_CFGS[self.cfg][2]
            self._rows = [n * rpt for n in nslots]
        self.ntiles = tiles.shape[0]
        self.tiles = torch.from_numpy(tiles).to(device)

    def stat_rows(self, j):
        return self._rows[j]

    def launch(self, jobs, stream, flops=0.0):
        L = lib()
        with observe("conv_gemm", flops=flops):
            if self.key[0] == "pw":
                for jb in jobs:
                    check(L.ffc_pw_forward(ctypes.byref(jb), self.cfg, stream), "ffc_pw_forward")
            elif self.key[0] == "q":
                arr = (_lib.ConvPJob * len(jobs))(*jobs)
                if self.ksplit > 1:
                    check(L.ffc_convq_forward_split(arr, len(jobs), self.tiles.data_ptr(), self.ntiles,
                                                    self.slots.data_ptr(), self.nslots, self.cfg, self.ksplit,
                                                    self.part.data_ptr(), stream),
                          "ffc_convq_forward_split")
                else:
                    check(L.ffc_convq_forward(arr, len(jobs), self.tiles.data_ptr(), self.ntiles, self.cfg, stream),
                          "ffc_convq_forward")
            elif self.key[0] == "patch":
                arr = (_lib.ConvPJob * len(jobs))(*jobs)
                cfg = self.cfg | (_lib.CONVP_EXACT_F32 if CONV_ARITH == "f32" else 0)
                check(L.ffc_convp_forward(arr, len(jobs), self.tiles.data_ptr(), self.ntiles, cfg, stream),
                      "ffc_convp_forward")
            else:
                arr = (_lib.ConvJob * len(jobs))(*jobs)
                check(L.ffc_conv_forward(arr, len(jobs), self.tiles.data_ptr(), self.ntiles, self.cfg, stream),
                      "ffc_conv_forward")


def cached_conv(cache, key, B, M, segs, weights, device, pw_ok=False):
    """-> (ConvExec, LaunchPlan) of a one-job launch kept in ``cache`` under ``key`` (made on a miss), its
    weights re-packed where they changed"""
    hit = cache.get(key)
    if hit is None:
        ex = ConvExec(B, M, list(segs), weights, device, pw_ok=pw_ok)
        hit = cache[key] = (ex, LaunchPlan([ex], device))
    hit[0].ensure_packed(weights)
    return hit


def sn_refresh(mod):
    """Run a module's torch.nn.utils.spectral_norm pre-hook (W <- W_orig / sigma, with one power
    iteration in training mode) at the point where the reference's forward would call the module
    (layers/snffc/snffc.py:23-33); the HIP path reads module.weight without calling the module.
    By default the power iteration stays host-driven PyTorch, as in the reference; a
    module switched on by set_sn_hip runs it, sigma and the division on the ffc::sn_weight op, written
    straight into the persistent tensor."""
    hooks = getattr(mod, "_forward_pre_hooks", None)
    if not hooks:
        return
    if mod.__dict__.get("sn_hip") and _sn_refresh_hip(mod):
        return
    from torch.nn.utils.spectral_norm import SpectralNorm
    for h in hooks.values():
        if isinstance(h, SpectralNorm):
            h(mod, None)
            # keep the normalised weight in one persistent tensor updated in place: its version
            # changes every refresh, so the packed-weight caches (keyed by pointer + version) repack
            w = getattr(mod, h.name)
            buf = mod.__dict__.get("_ffc_sn_" + h.name)
            if buf is None or buf.shape != w.shape or buf.device != w.device:
                buf = w.detach().clone()
                mod.__dict__["_ffc_sn_" + h.name] = buf
            else:
                buf.copy_(w.detach())
            setattr(mod, h.name, buf)


def _sn_refresh_hip(mod):
    """sn_refresh on the HIP path: no autograd, W lands in the persistent tensor (its version moves, so
    the packed-weight caches repack).  False when the module has no SpectralNorm hook"""
    from . import _autograd as ag
    h = ag.sn_hook(mod)
    if h is None:
        return False
    w_orig = getattr(mod, h.name + "_orig").detach()
    buf = mod.__dict__.get("_ffc_sn_" + h.name)
    if buf is None or buf.shape != w_orig.shape or buf.device != w_orig.device or not buf.is_contiguous():
        buf = torch.empty(w_orig.shape, device=w_orig.device, dtype=w_orig.dtype)
        mod.__dict__["_ffc_sn_" + h.name] = buf
    sigma = torch.empty(1, device=w_orig.device, dtype=torch.float32)
    with torch.no_grad():
        torch.ops.ffc.sn_weight([w_orig.contiguous()], [getattr(mod, h.name + "_u")], [getattr(mod, h.name + "_v")],
                                [buf], sigma, sigma.new_empty(0), [int(h.dim)], bool(mod.training))
    setattr(mod, h.name, buf)
    return True


_SN_BATCHED = set()   # ids of the modules a model forward has refreshed in its own table (sn_batch)


class sn_batch:
    """``with sn_batch(mods):`` refreshes the spectral-norm weights of those of ``mods`` that are switched
    to the HIP path (set_sn_hip) in ONE table -- three launches forward, two backward, whatever the
    number of layers -- and turns their per-layer sn_refresh_train calls inside the block into no-ops:
    one power iteration per layer and forward call, as the reference's module calls do (power
    iterations do not depend on activations, so refreshing up front changes no result).  Modules
    without the switch are left to their per-layer refresh."""

    def __init__(self, mods):
        self.mods = mods
        self.ids = ()

    def __enter__(self):
        from . import _autograd as ag
        pairs = [(m, ag.sn_hook(m)) for m in self.mods if m.__dict__.get("sn_hip") and id(m) not in _SN_BATCHED]
        pairs = [(m, h) for m, h in pairs if h is not None]
        if pairs:
            ag.sn_weights([m for m, _ in pairs], [h for _, h in pairs])
            self.ids = tuple(id(m) for m, _ in pairs)
            _SN_BATCHED.update(self.ids)
        return self

    def __exit__(self, *exc):
        _SN_BATCHED.difference_update(self.ids)
        return False


def sn_refresh_train(mod):
    """training path: run the spectral_norm pre-hooks so ``mod.weight`` = weight_orig / sigma is a
    differentiable function of weight_orig (the reference calls the module, which does the same).
    With set_sn_hip: the ffc::sn_weight op with a table of one, or nothing when the model refreshed
    this module in its own table at the top of the forward (sn_batch)"""
    hooks = getattr(mod, "_forward_pre_hooks", None)
    if not hooks:
        return
    if mod.__dict__.get("sn_hip"):
        if id(mod) in _SN_BATCHED:
            return
        from . import _autograd as ag
        h = ag.sn_hook(mod)
        if h is not None:
            ag.sn_weights([mod], [h])
            return
    from torch.nn.utils.spectral_norm import SpectralNorm
    for h in hooks.values():
        if isinstance(h, SpectralNorm):
            h(mod, None)


def conv_weight(mod):
    """ConvWeight of an nn.Conv2d (layout 0) / nn.ConvTranspose2d (layout 1)."""
    w = mod.weight.detach()
    kh, kw = w.shape[2], w.shape[3]
    b = mod.bias.detach() if mod.bias is not None else None
    return ConvWeight(require(w, "weight"), 1 if isinstance(mod, nn.ConvTranspose2d) else 0, kh, kw,
                      require(b, "bias") if b is not None else None)


def _square(v, what):
    if isinstance(v, (tuple, list)):
        if len(set(v)) != 1:
            raise NotImplementedError(f"non-square {what} {v}")
        return int(v[0])
    return int(v)


def conv_seg(mod, x: torch.Tensor):
    """Seg for an nn.Conv2d / nn.ConvTranspose2d applied to x."""
    if mod.groups != 1:
        raise NotImplementedError("grouped convolutions are not on the FFC hot path (groups=1 in every caller)")
    if getattr(mod, "padding_mode", "zeros") != "zeros":
        raise NotImplementedError("only zero padding")
    if isinstance(mod.padding, str):
        raise NotImplementedError("string padding")
    B, C, H, W = x.shape
    if C != mod.in_channels:
        raise RuntimeError(f"expected input with {mod.in_channels} channels, got {C}")
    k = _square(mod.kernel_size, "kernel")
    s = _square(mod.stride, "stride")
    p = _square(mod.padding, "padding")
    d = _square(mod.dilation, "dilation")
    if isinstance(mod, nn.ConvTranspose2d):
        op = _square(mod.output_padding, "output_padding")
        return _plan.Seg("convT", C, H, W, k, s, p, d, op)
    return _plan.Seg("conv", C, H, W, k, s, p, d)
