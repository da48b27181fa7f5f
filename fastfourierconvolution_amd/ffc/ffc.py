"""Drop-in ``FFC`` (reference: layers/ffc/ffc.py:10-99) and the shared HIP executor that
FFCTranspose (ffc_transpose.py) and FFC_BN_ACT (ffc_bn_act.py) also use.

The module forwards go through the custom ops of ops.py (``ffc::ffc_bn_act`` for inference, the
per-op training ops under autograd); _FFCExec is the executor those ops run.

Each output branch is ONE implicit-GEMM launch (both branches share it):
  out_l = convl2l(x_l) + convg2l(x_g)                      segments: conv, conv
  out_g = convl2g(x_l) + conv2(v),  v = s + fu(s)          segments: conv, 1x1 at output res
with the FFC_BN_ACT activation fused into the epilogue (or BN partials, then one
BN+activation pass when norm_layer is BatchNorm2d).  ``nn.Identity`` sub-convs keep the
reference semantics: they return their input (usually the int 0 of the tuple protocol).
"""
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from .. import _autograd as ag
from .. import _plan
from .. import _runtime as rt
from .. import ops
from .spectral_transform import SpectralTransform


class Branch(NamedTuple):
    """one output branch of a layer: out = act(BN(sum_s conv_s(inputs[s]) + addends))"""
    name: str          # "l" | "g"
    segs: list         # _plan.Seg per convolution
    weights: list      # rt.ConvWeight per convolution
    inputs: list       # input tensor per convolution
    addends: list      # tensors passed through nn.Identity sub-convs
    act: tuple         # (code, parameter)
    bn: Optional[nn.Module]
    M: Optional[int]   # output channels (None: no convolution)


@dataclass(slots=True)
class _Job:
    """a branch planned on the implicit-GEMM kernels (its segments possibly in the outer-product form)"""
    branch: Branch
    key: tuple         # of ``ex`` in the layer's cache
    ex: rt.ConvExec
    segs: list
    weights: list
    M: int
    out: torch.Tensor
    addend: Optional[torch.Tensor]


class _Dense(NamedTuple):
    """an outer-product branch for ffc_dense_forward: weight (N, C, 1, 1) with its bias repeated over the taps"""
    weight: rt.ConvWeight   # derived by _outer_rewrite from ...
    source: rt.ConvWeight   # ... the module's own weight and bias (what the launch's pack is keyed on)
    x: torch.Tensor
    out: torch.Tensor
    act: tuple
    N: int


class _Post(NamedTuple):
    """an output that still needs its BN and / or activation (+ noise) pass"""
    name: str
    out: torch.Tensor
    act: tuple
    bn: Optional[nn.Module]
    slab: Optional[torch.Tensor]   # BN partials from the GEMM epilogue
    nrows: int


def _is_conv(mod):
    return isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d))


def _no_conditional():
    # the reference passes y into SpectralTransform / FourierUnitSN, whose BatchNorm2d.forward()
    # takes no label (fourier_unity.py:46-47), or into nn.Identity.forward (one argument)
    raise TypeError("FFC: the conditional (y) path is not supported (the reference raises in "
                    "FourierUnitSN, fourier_unity.py:46-47)")


def layer_call(mod, ffc, x, y, act_l=(0, 0.0), act_g=(0, 0.0), bn_l=None, bn_g=None, noise=None, defer=False):
    """forward of FFC_BN_ACT / FFC / FFCTranspose ``mod`` whose FFC part is ``ffc``: the training ops
    when autograd needs them, else the fused ffc::ffc_bn_act op"""
    if y is not None and ffc.ratio_gout != 0:
        _no_conditional()
    x_l, x_g = x if type(x) is tuple else (x, 0)
    if ag.wants_grad(mod, x_l, x_g):
        x_l, x_g = rt.materialize(x_l), rt.materialize(x_g)
        return ffc._run_train(x_l, x_g, None, act_l, act_g, bn_l, bn_g, noise)
    return ops.layer_forward(mod, x, noise, defer)


class _FFCExec:
    """mixin: fused execution of an FFC / FFCTranspose layer (run by the ffc::ffc_bn_act op)"""

    def _ffc_cache(self):
        c = self.__dict__.get("_exec_cache")
        if c is None:
            c = self.__dict__["_exec_cache"] = {}
        return c

    def _branch(self, parts):
        """parts: list of (module, input) whose outputs are summed.  -> (segments, weights, inputs, addends)"""
        segs, weights, inputs, addends = [], [], [], []
        for mod, inp in parts:
            if _is_conv(mod):
                if not isinstance(inp, torch.Tensor):
                    raise TypeError(f"{type(mod).__name__} got {type(inp).__name__} input")
                rt.sn_refresh(mod)
                segs.append(rt.conv_seg(mod, inp))
                weights.append(rt.conv_weight(mod))
                inputs.append(inp)
            elif isinstance(mod, nn.Identity):
                if isinstance(inp, torch.Tensor):
                    addends.append(inp)       # Identity passes a tensor through
            else:
                raise NotImplementedError(f"{type(mod).__name__} in an FFC branch")
        return segs, weights, inputs, addends

    def _g_branch(self, x_l, spectral_v, act_g, bn_g):
        """the global output branch convl2g(x_l) + conv2(v) as one job; spectral_v() -> v = s + fu(s), the
        SpectralTransform up to its conv2 (None without one).  It is called after convl2g's weight is
        taken, where the one-stream path has always run the spectral chain."""
        segs, w, inp, add = self._branch([(self.convl2g, x_l)])
        M = self.convl2g.out_channels if _is_conv(self.convl2g) else None
        if spectral_v is not None:
            v, conv2 = spectral_v(), self.convg2g.conv2
            rt.sn_refresh(conv2)
            segs.append(_plan.Seg("pw", v.shape[1], v.shape[2], v.shape[3]))
            w.append(rt.conv_weight(conv2))
            inp.append(v)
            M = conv2.out_channels if M is None else M
        return Branch("g", segs, w, inp, add, act_g, bn_g, M)

    def _run(self, x, y=None, act_l=(0, 0.0), act_g=(0, 0.0), bn_l=None, bn_g=None, noise=None, defer=False):
        """noise: optional {"l"|"g": (NoiseInjection, noise tensor or None)} applied after the branch's
        BN + activation in the same pass (FFC_BN_ACT followed by the fgan128 NoiseInjection).
        defer: return rt.PendingAct outputs instead of running that pass (the consumer applies it).
        Inputs may be PendingAct: a consumer that cannot apply them materializes them first."""
        x_l, x_g = x if type(x) is tuple else (x, 0)
        if isinstance(x_l, rt.PendingAct) or isinstance(x_g, rt.PendingAct):
            out = self._run_pending(x_l, x_g, y, act_l, act_g, bn_l, bn_g, noise)
            if out is not None:
                return out
            x_l, x_g = rt.materialize(x_l), rt.materialize(x_g)
        if ag.wants_grad(self, x_l, x_g):
            return self._run_train(x_l, x_g, y, act_l, act_g, bn_l, bn_g, noise)
        if isinstance(x_l, torch.Tensor):
            x_l = rt.require(x_l, "x_l")
        if isinstance(x_g, torch.Tensor):
            x_g = rt.require(x_g, "x_g")
        ref = x_l if isinstance(x_l, torch.Tensor) else x_g
        if not isinstance(ref, torch.Tensor):
            raise TypeError("FFC input has no tensor branch")
        B, dev = ref.shape[0], ref.device
        stream = rt.stream_of(ref)
        branches = []
        if self.ratio_gout != 1:
            segs, w, inp, add = self._branch([(self.convl2l, x_l), (self.convg2l, x_g)])
            M = next((m.out_channels for m in (self.convl2l, self.convg2l) if _is_conv(m)), None)
            branches.append(Branch("l", segs, w, inp, add, act_l, bn_l, M))
        if self.ratio_gout == 0:
            return self._launch_branches(branches, B, dev, stream, noise, defer)
        st = self.convg2g
        if not isinstance(st, (nn.Identity, SpectralTransform)):
            raise NotImplementedError(type(st).__name__)
        spectral = isinstance(st, SpectralTransform)
        if rt.OVERLAP_SPECTRAL and spectral and y is None and isinstance(x_g, torch.Tensor) and branches and \
                branches[0].segs:
            # The local branch does not depend on the spectral chain: its GEMM runs on the main stream
            # while SpectralTransform's latency-bound kernels run on a side stream (fork / join by
            # events, hipGraph-capturable); then the global-branch GEMM consumes v.
            main = torch.cuda.current_stream(dev)
            side = rt.side_stream(dev)
            side.wait_stream(main)
            if rt.OVERLAP_SPECTRAL == "spectral-first":
                with torch.cuda.stream(side):
                    v = st.spectral(x_g)
                out_l, _ = self._launch_branches(branches, B, dev, stream, noise)
            else:
                out_l, _ = self._launch_branches(branches, B, dev, stream, noise)
                with torch.cuda.stream(side):
                    v = st.spectral(x_g)
            main.wait_stream(side)
            v.record_stream(main)
            _, out_g = self._launch_branches([self._g_branch(x_l, lambda: v, act_g, bn_g)], B, dev, stream, noise)
            return out_l, out_g

        def spectral_v():
            if y is not None:
                _no_conditional()
            if not isinstance(x_g, torch.Tensor):
                raise TypeError("spectral branch needs a tensor x_g")
            return st.spectral(x_g)
        branches.append(self._g_branch(x_l, spectral_v if spectral else None, act_g, bn_g))
        return self._launch_branches(branches, B, dev, stream, noise, defer)

    def _run_pending(self, x_l, x_g, y, act_l, act_g, bn_l, bn_g, noise):
        """Inputs with deferred BN + activation (+ noise): the direct 3x3 head (fgan128 conv7: local output
        only, no BN, both inputs convs) reads them through ffc_in_tf.  -> (out_l, 0) or None (not fusable)"""
        if y is not None or noise or bn_l is not None or self.ratio_gout != 0 or ag.wants_grad(self, x_l, x_g):
            return None
        parts = [(self.convl2l, x_l), (self.convg2l, x_g)]
        if not all(isinstance(m, nn.Conv2d) and isinstance(t, (torch.Tensor, rt.PendingAct)) for m, t in parts):
            return None
        raw = [t.raw if isinstance(t, rt.PendingAct) else rt.require(t, "x") for _, t in parts]
        segs, w, inp, _ = self._branch([(m, r) for (m, _), r in zip(parts, raw)])
        M = self.convl2l.out_channels
        if rt.conv_route(segs, w, M, False, False, frozenset(("conv3",))) != "conv3":
            return None
        tfs = [t if isinstance(t, rt.PendingAct) else None for _, t in parts]
        return rt.smallm_forward("conv3", segs, w, inp, M, raw[0].shape[0], act_l, rt.stream_of(raw[0]), tfs=tfs), 0

    def _run_train(self, x_l, x_g, y, act_l, act_g, bn_l, bn_g, noise):
        """training path (autograd recording): the layer's local convs and ST conv2 as one
        _ConvLayerFn (both output branches; their data gradients w.r.t. x_l in one adjoint launch),
        SpectralTransform through its per-op Functions, BN + activation as _BNActFn
        (include/ffc_amd.h "training path")."""
        if y is not None:
            _no_conditional()
        for t, n in ((x_l, "x_l"), (x_g, "x_g")):
            if isinstance(t, torch.Tensor):
                rt.require(t, n)
        ref = x_l if isinstance(x_l, torch.Tensor) else x_g
        if not isinstance(ref, torch.Tensor):
            raise TypeError("FFC input has no tensor branch")
        B = ref.shape[0]
        inputs, idx, outs, edges, names = [], {}, [], [], []

        def inp(t):
            if id(t) not in idx:
                idx[id(t)] = len(inputs)
                inputs.append(t.contiguous())
            return idx[id(t)]

        def branch(parts, extra=None):
            convs = []
            for mod, t in parts:
                if _is_conv(mod):
                    if not isinstance(t, torch.Tensor):
                        raise TypeError(f"{type(mod).__name__} got {type(t).__name__} input")
                    convs.append((mod, t))
                elif isinstance(t, torch.Tensor):
                    raise NotImplementedError("identity pass-through of a tensor on the training path")
            return convs + ([extra] if extra else [])

        for name, parts, extra, act, bn in (
                ("l", [(self.convl2l, x_l), (self.convg2l, x_g)], None, act_l, bn_l),
                ("g", [(self.convl2g, x_l)], "st", act_g, bn_g)):
            if (name == "l" and self.ratio_gout == 1) or (name == "g" and self.ratio_gout == 0):
                continue
            ex = None
            if extra and isinstance(self.convg2g, SpectralTransform) and isinstance(x_g, torch.Tensor):
                v = ag.spectral_v(self.convg2g, x_g)
                ex = (self.convg2g.conv2, v, _plan.Seg("pw", v.shape[1], v.shape[2], v.shape[3]))
            elif extra and not isinstance(self.convg2g, nn.Identity):
                raise NotImplementedError(type(self.convg2g).__name__)
            convs = branch(parts)
            if not convs and ex is None:
                continue
            j = len(outs)
            M = (convs[0][0] if convs else ex[0]).out_channels
            outs.append((M,) + (tuple(act) if bn is None else (0, 0.0)))
            for mod, t in convs:
                edges.append((j, inp(t), rt.conv_seg(mod, t), mod))
            if ex is not None:
                edges.append((j, inp(ex[1]), ex[2], ex[0]))
            names.append((name, act, bn))
        res = {"l": 0, "g": 0}
        if outs:
            ys = ag.conv_layer(B, outs, edges, inputs)
            for (name, act, bn), yv in zip(names, ys):
                res[name] = ag.bn_act(bn, yv, act) if bn is not None else yv
        for name, (mod, n) in (noise or {}).items():   # fgan128's NoiseInjection after FFC_BN_ACT
            if isinstance(res[name], torch.Tensor):
                res[name] = ag.noise_inject(mod, res[name], n)
        return res["l"], res["g"]

    def _launch_branches(self, branches, B, dev, stream, noise=None, defer=False):
        """route, plan / pack and launch the GEMM(s) of the given branches (one launch per kernel kind),
        then BN statistics and BN+activation passes (defer: PendingAct outputs instead of those
        passes).  -> (out_l, out_g)"""
        outs = {"l": 0, "g": 0}
        if any(len(br.addends) > 1 for br in branches):
            raise NotImplementedError("more than one identity pass-through in a branch")
        routes = [rt.conv_route(br.segs, br.weights, br.M, bool(br.addends), br.bn is not None, rt.INFER_ROUTES)
                  for br in branches]
        jobs, post = self._plan_branches(branches, routes, B, dev, stream, outs)
        self._launch_jobs(jobs, dev, stream, post)
        self._finish(post, outs, noise or {}, defer, dev, stream)
        return outs["l"], outs["g"]

    def _plan_branches(self, branches, routes, B, dev, stream, outs):
        """per branch, in order: its pass-through copy, its direct kernel (launched here), or its plan,
        packed weights and output on the implicit-GEMM kernels.  -> (jobs, post)"""
        cache = self._ffc_cache()
        jobs, post, dense = [], [], []
        for br, route in zip(branches, routes):
            addend = br.addends[0] if br.addends else None
            if not br.segs:
                # no convolution: the branch is its pass-through (or the int 0)
                if addend is not None:
                    outs[br.name] = addend.clone()
                    post.append(_Post(br.name, outs[br.name], br.act, br.bn, None, 0))
                continue
            if route in ("convT", "full", "conv3", "convT3"):
                outs[br.name] = rt.smallm_forward(route, br.segs, br.weights, br.inputs, br.M, B, br.act, stream,
                                                  rt.packs_of(cache))
                continue
            segs, w, M, out_shape = br.segs, br.weights, br.M, None
            rw = self._outer_rewrite(segs, w, M) if addend is None and br.bn is None else None
            if rw is not None:
                segs, w, M, chw = rw
                out_shape = (B,) + chw
                if route == "dense":
                    # a plain GEMM: batched with the other branch's into one dense launch below
                    outs[br.name] = torch.empty(out_shape, device=dev, dtype=torch.float32)
                    dense.append(_Dense(w[0], br.weights[0], br.inputs[0], outs[br.name], br.act, M))
                    continue
            key = (br.name, B, tuple(segs), str(dev))
            ex = cache.get(key)
            if ex is None:
                ex = cache[key] = rt.ConvExec(B, M, segs, w, dev)
            ex.ensure_packed(w)
            pl = ex.plan
            out = torch.empty(out_shape or (B, pl.M, pl.OH, pl.OW), device=dev, dtype=torch.float32)
            if addend is not None and tuple(addend.shape) != tuple(out.shape):
                raise RuntimeError(f"shape mismatch adding pass-through {tuple(addend.shape)} to {tuple(out.shape)}")
            outs[br.name] = out
            jobs.append(_Job(br, key, ex, segs, w, M, out, addend))
        if dense:
            self._launch_dense(dense, B, stream)
        # the layer's convq jobs share one launch, so one configuration: when they picked different
        # ones (untuned shapes), rebuild them on the costliest job's (cached: happens once)
        qjobs = [jb for jb in jobs if jb.ex.launch_key[0] == "q"]
        if len({jb.ex.launch_key for jb in qjobs}) > 1:
            # the decision is cached per layer shape, including "this job cannot take that cfg" (it
            # stays on its own kernel): nothing is re-planned or re-packed on later forwards
            rkey = ("rebuild",) + tuple(jb.key for jb in qjobs)
            dec = cache.get(rkey)
            if dec is None:
                cfg = max((jb.ex.plan for jb in qjobs), key=_plan.convq_cost).cfg
                dec = {}
                for i, jb in enumerate(qjobs):
                    ex2 = rt.ConvExec(B, jb.M, jb.segs, jb.weights, dev, convq_cfg=cfg)
                    if ex2.launch_key[0] == "q":
                        cache[jb.key] = dec[i] = ex2
                cache[rkey] = dec
            for i, ex2 in dec.items():
                ex2.ensure_packed(qjobs[i].weights)
                qjobs[i].ex = ex2
        return jobs, post

    def _launch_jobs(self, jobs, dev, stream, post):
        """one launch per kernel configuration; a job with a BN gets its slab of partials and a post item"""
        cache = self._ffc_cache()
        groups = {}
        for jb in jobs:
            groups.setdefault(jb.ex.launch_key, []).append(jb)
        for gjobs in groups.values():
            lkey = ("launch",) + tuple(id(jb.ex) for jb in gjobs)
            lp = cache.get(lkey)
            if lp is None:
                lp = cache[lkey] = rt.LaunchPlan([jb.ex for jb in gjobs], dev)
            structs = []
            for ji, jb in enumerate(gjobs):
                act, bn = jb.branch.act, jb.branch.bn
                slab = None
                if bn is not None and rt.bn_mode(bn)[0]:
                    slab = torch.empty((lp.stat_rows(ji), jb.ex.plan.M, 4), device=dev, dtype=torch.float32)
                fused_act = act if bn is None else (0, 0.0)
                structs.append(jb.ex.job([(x, None) for x in jb.branch.inputs], jb.out, fused_act[0], fused_act[1],
                                         jb.addend, slab))
                if bn is not None:
                    post.append(_Post(jb.branch.name, jb.out, act, bn, slab, lp.stat_rows(ji)))
            lp.launch(structs, stream, flops=sum(jb.ex.flops for jb in gjobs))

    def _finish(self, post, outs, noise, defer, dev, stream):
        """BN scale / shift of the post items, then their BN + activation (+ noise) passes as one launch
        (defer: rt.PendingAct outputs instead); a NoiseInjection without such a pass runs on its own"""
        done = set()
        applies = []
        # the layer's slab-backed BNs (bn_l, bn_g) finalized together: one SyncBN all-reduce for both
        slab_bns = [(it.bn, it.out.shape[1], it.slab, it.nrows, 1.0) for it in post
                    if it.bn is not None and it.slab is not None]
        ss = dict(zip((id(it[0]) for it in slab_bns), rt.bn_scale_shift_many(slab_bns, dev, stream)))
        for it in post:
            out, (act, param) = it.out, it.act
            C = out.shape[1]
            nz = noise.get(it.name)
            if it.bn is not None:
                if it.slab is not None:
                    sc, sh = ss[id(it.bn)]
                elif rt.bn_mode(it.bn)[0]:
                    sc, sh = self._bn_from_tensor(it.bn, out, stream)
                else:
                    sc, sh = rt.bn_scale_shift(it.bn, C, None, it.nrows, 1.0, dev, stream)
            else:
                if act == 0 and nz is None:
                    continue
                sc = torch.ones(C, device=dev, dtype=torch.float32)
                sh = torch.zeros(C, device=dev, dtype=torch.float32)
            if defer:
                outs[it.name] = rt.PendingAct(out, sc, sh, act, param, *(nz if nz is not None else (None, None)))
                done.add(it.name)
                continue
            # the global output's plane sums for the next layer's SE gate (large planes, where the
            # SpectralTransform reads y twice otherwise: spectral_transform.py pw path)
            HW = out.shape[2] * out.shape[3]
            ps = None
            if it.name == "g" and rt.SE_SUMS and HW % 4 == 0 and HW >= 256:
                chunks = rt.lib().ffc_plane_chunks(HW)
                ps = torch.empty((out.shape[0], out.shape[1], chunks), device=dev, dtype=torch.float32)
            if nz is not None and HW % 4 == 0:
                # the noise drawn here, in branch order, as the single pass does; applied below
                p = rt.PendingAct(out, sc, sh, act, param, *nz)
                applies.append(rt.ActApply(out, sc, sh, act, param, p.noise_w, p.noise, ps))
                done.add(it.name)
            else:
                applies.append(rt.ActApply(out, sc, sh, act, param, plane_sums=ps))
            if ps is not None:
                out._ffc_plane_sums = (ps, chunks, out._version)
        if applies:   # the layer's BN + activation (+ noise) passes in one launch
            rt.bn_act_apply_batch(applies)
        for name, (mod, n) in noise.items():   # branches without a BN/activation pass of their own
            if name not in done and isinstance(outs[name], torch.Tensor):
                outs[name] = mod(outs[name], n)

    def _outer_rewrite(self, segs, w, M):
        """ConvTranspose2d(k, s=1, p=0) on a 1x1 input (the generator's first layer, ffc0:
        ffc_transpose.py:79-86 on z of shape (B, nz, 1, 1)) is an outer product: out[b, m, y, x] =
        sum_c z[b, c] W[c, m, y, x].  As ONE GEMM with M' = M*k*k "channels" at 1x1 (the output
        (B, M, k, k) has the memory layout of (B, M*k*k, 1, 1)) it fills the GPU with tiles instead
        of 16 tiny per-phase GEMMs: on ffc_dense_forward where rt.conv_route says 'dense', as 1x1
        segments of an implicit-GEMM job otherwise (several segments, or more channels than the dense
        kernel stages).  -> (segments, weights, M', output shape) or None."""
        if M is None or not segs or not rt.USE_OUTER:
            return None
        k = segs[0].k
        for sg in segs:
            if (sg.kind, sg.IH, sg.IW, sg.s, sg.p, sg.d, sg.op, sg.k) != ("convT", 1, 1, 1, 0, 1, 0, k):
                return None
        packs = rt.packs_of(self._ffc_cache())
        segs2, w2 = [], []
        for sg, wt in zip(segs, w):
            def build(sg=sg, wt=wt):
                wr = wt.w.permute(1, 2, 3, 0).reshape(M * k * k, sg.C, 1, 1).contiguous()   # (C,M,k,k) -> (M k k, C)
                br = wt.bias.repeat_interleave(k * k).contiguous() if wt.bias is not None else None
                rt.note_tensors([wr, br])   # the launch's packed-weight key is taken from these
                return wr, br
            wr, br = packs.get("outer", [wt.w, wt.bias], build)
            segs2.append(_plan.Seg("pw", sg.C, 1, 1))
            w2.append(rt.ConvWeight(wr, 0, 1, 1, br))
        return segs2, w2, M * k * k, (M, k, k)

    def _launch_dense(self, dense, B, stream):
        """outer-product branches (ConvT on a 1x1 input) as ffc_dense_forward launches; two branches with
        the same input and activation share one launch (their weights concatenated along N, cached)"""
        packs = rt.packs_of(self._ffc_cache())
        groups = []
        for d in dense:
            for g in groups:
                if len(g) == 1 and g[0].x.data_ptr() == d.x.data_ptr() and g[0].act == d.act:
                    g.append(d)
                    break
            else:
                groups.append([d])
        for g in groups:
            wts = [d.weight for d in g]

            def build(wts=wts):
                Wt = torch.cat([wt.w.reshape(wt.w.shape[0], -1).t() for wt in wts], dim=1).contiguous()
                if all(wt.bias is None for wt in wts):
                    return Wt, None
                return Wt, torch.cat([wt.bias if wt.bias is not None else torch.zeros(wt.w.shape[0], device=Wt.device)
                                      for wt in wts]).contiguous()
            Wt, bias = packs.get("dense", [t for d in g for t in (d.source.w, d.source.bias)], build)
            K, N = Wt.shape
            rt.dense_forward(g[0].x, Wt, bias, B, K, N, g[0].N, g[0].out, g[1].out if len(g) > 1 else None,
                             g[0].act, stream)

    def _bn_from_tensor(self, bn, out, stream):
        """batch statistics of a pass-through branch (no GEMM epilogue to collect them)"""
        B, C = out.shape[:2]
        ex = self._ffc_cache().get(("bnstats", tuple(out.shape), str(out.device)))
        if ex is None:
            seg = _plan.Seg("pw", C, out.shape[2], out.shape[3])
            eye = nn.Conv2d(C, C, 1, bias=False).to(out.device)
            with torch.no_grad():
                eye.weight.zero_()
                eye.weight[:, :, 0, 0] = torch.eye(C, device=out.device)
            ex = (rt.ConvExec(B, C, [seg], [rt.conv_weight(eye)], out.device), eye)
            self._ffc_cache()[("bnstats", tuple(out.shape), str(out.device))] = ex
        cexec, _ = ex
        lp = rt.LaunchPlan([cexec], out.device)
        slab = torch.empty((lp.stat_rows(0), C, 4), device=out.device, dtype=torch.float32)
        tmp = torch.empty_like(out)
        lp.launch([cexec.job([(out, None)], tmp, stats=slab)], stream)
        return rt.bn_scale_shift(bn, C, slab, lp.stat_rows(0), 1.0, out.device, stream)


class FFC(_FFCExec, nn.Module):
    def __init__(self, in_channels: int, out_channels: int, kernel_size: int,
                 ratio_gin: float, ratio_gout: float, stride: int = 1, padding: int = 0,
                 dilation: int = 1, groups: int = 1, bias: bool = False, enable_lfu: bool = True,
                 attention: bool = False, num_classes: int = 1):
        super().__init__()
        assert stride == 1 or stride == 2, "Stride should be 1 or 2."
        self._ffc_ctor = ["FFC", dict(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size,
                                      ratio_gin=ratio_gin, ratio_gout=ratio_gout, stride=stride, padding=padding,
                                      dilation=dilation, groups=groups, bias=bias, enable_lfu=enable_lfu,
                                      num_classes=num_classes)]
        self.stride = stride
        in_cg = int(in_channels * ratio_gin)
        in_cl = in_channels - in_cg
        out_cg = int(out_channels * ratio_gout)
        out_cl = out_channels - out_cg
        print("in_cl, in_cg, out_cl, out_cg")   # the reference prints at construction (ffc.py:38-39)
        print(in_cl, in_cg, out_cl, out_cg)
        self.ratio_gin = ratio_gin
        self.ratio_gout = ratio_gout
        module = nn.Identity if (in_cl == 0 or out_cl == 0) else nn.Conv2d
        self.convl2l = module(in_cl, out_cl, kernel_size, stride, padding, dilation, groups, bias)
        module = nn.Identity if (in_cl == 0 or out_cg == 0) else nn.Conv2d
        self.convl2g = module(in_cl, out_cg, kernel_size, stride, padding, dilation, groups, bias)
        module = nn.Identity if (in_cg == 0 or out_cl == 0) else nn.Conv2d
        self.convg2l = module(in_cg, out_cl, kernel_size, stride, padding, dilation, groups, bias)
        module = nn.Identity if in_cg == 0 or out_cg == 0 else SpectralTransform
        self.convg2g = module(in_cg, out_cg, stride, 1 if groups == 1 else groups // 2, enable_lfu, False,
                              num_classes)

    def forward(self, x, y=None):
        return layer_call(self, self, x, y)
