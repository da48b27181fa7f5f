"""FusedAdamW / FusedAdam: torch.optim.AdamW / Adam whose ``step()`` is one pass of csrc/optim_kernels.hip per
param group (``ffc::optim_step``: 1 + ceil(n / 64) launches for n parameters with a gradient), with the step count
and an optional linear LR decay kept on the device, so a captured training iteration follows the reference's
schedule (fgan128_complete.py:625-629, 715-716):

    optG = FusedAdamW(G.parameters(), lr=2e-4, betas=(0.5, 0.999), decay_steps=num_total_steps)
    ...
    optG.step()          # lr_eff = lr * max(0, 1 - s / decay_steps), computed on the device
    optG.lr_step()       # s <- s + 1: LambdaLR(optG, lambda s: 1 - s / num_total_steps).step(), capturable

The update is torch's ``_single_tensor_adam`` (amsgrad = maximize = False) element for element; include/ffc_amd.h
says which scalar is rounded where.  The classes subclass torch's, so ``param_groups``, ``zero_grad``,
``add_param_group`` and a host ``LambdaLR`` (with ``decay_steps=None``, in eager mode) work as before, and the state
dict interchanges with torch's.  Limits: fp32 parameters on one GPU; no amsgrad, maximize, sparse gradients or
tensor ``lr``; one step count per param group -- a parameter whose ``.grad`` is None on some steps shares its group's
count where torch keeps one per parameter.  ``step()`` and ``lr_step()`` never synchronise; ``get_last_lr()``,
``state_dict()`` and ``load_state_dict()`` read or write the device counts and do."""
import torch

from . import _autograd as ag

__all__ = ["FusedAdamW", "FusedAdam"]

TICKS_KEY = "ffc_lr_ticks"   # the schedule count s of a group in the state dict: a group key torch carries and ignores


class _Fused:
    """the HIP step under torch.optim.Adam's param groups and state layout"""

    def _ffc_init(self, decay_steps, amsgrad, maximize):
        if amsgrad or maximize:
            raise NotImplementedError(f"{type(self).__name__}: amsgrad and maximize are not implemented")
        if decay_steps is not None and (int(decay_steps) != decay_steps or decay_steps < 1):
            raise ValueError(f"{type(self).__name__}: decay_steps must be a positive integer or None")
        self.decay_steps = None if decay_steps is None else int(decay_steps)
        self._ffc_state = None   # (groups, 4) int64 on the GPU: [t, s, scalars] per param group

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        name = type(self).__name__
        group = self.param_groups[-1]
        if group.get("amsgrad") or group.get("maximize"):
            raise NotImplementedError(f"{name}: amsgrad and maximize are not implemented")
        if isinstance(group["lr"], torch.Tensor):
            raise NotImplementedError(f"{name}: a tensor lr is not implemented")
        devices = {p.device for g in self.param_groups for p in g["params"]}
        for p in group["params"]:
            if not p.is_cuda or p.dtype != torch.float32:
                raise NotImplementedError(f"{name}: fp32 parameters on the GPU only ({p.dtype} on {p.device})")
            if not p.is_contiguous():
                raise NotImplementedError(f"{name}: contiguous parameters only")
        if len(devices) > 1:
            raise NotImplementedError(f"{name}: the parameters must share one device")
        row = torch.zeros((1, ag.OPTIM_STATE), dtype=torch.int64, device=devices.pop())
        self._ffc_state = row if getattr(self, "_ffc_state", None) is None else torch.cat([self._ffc_state, row])

    def _mode(self, group):
        return ag.OPTIM_ADAMW if group.get("decoupled_weight_decay", self._decoupled) else ag.OPTIM_ADAM

    @torch.no_grad()
    def step(self, closure=None):
        """one ffc::optim_step per param group over the parameters that have a gradient; no host sync"""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for k, group in enumerate(self.param_groups):
            params, grads, ms, vs = [], [], [], []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise NotImplementedError(f"{type(self).__name__}: sparse gradients are not implemented")
                st = self.state[p]
                if not st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                params.append(p)
                grads.append(g if g.is_contiguous() else g.contiguous())
                ms.append(st["exp_avg"])
                vs.append(st["exp_avg_sq"])
            if not params:
                continue
            beta1, beta2 = group["betas"]
            torch.ops.ffc.optim_step(params, grads, ms, vs, self._ffc_state[k], float(group["lr"]), float(beta1),
                                     float(beta2), float(group["eps"]), float(group["weight_decay"]),
                                     self.decay_steps or 0, self._mode(group))
        return loss

    def lr_step(self):
        """scheduler.step() of LambdaLR(self, lambda s: 1 - s / decay_steps) on the device: one ffc::optim_tick for
        all groups, capturable.  Without decay_steps the count advances and changes nothing."""
        torch.ops.ffc.optim_tick(self._ffc_state)

    def reset_lr_schedule(self, count=0):
        """s <- count in every group, in place on the device (a captured graph keeps following it); no host sync"""
        self._ffc_state[:, 1] = int(count)

    def get_last_lr(self):
        """the lr the next step() applies, per group, from the device's schedule count: synchronises"""
        s = self._ffc_state[:, 1].tolist()
        T = self.decay_steps
        return [float(g["lr"]) * (max(0.0, 1 - k / T) if T else 1.0) for g, k in zip(self.param_groups, s)]

    def state_dict(self):
        """torch's layout: per parameter ``step`` (the group's count, a CPU fp32 scalar as torch's), ``exp_avg``,
        ``exp_avg_sq``; the schedule count as the group key 'ffc_lr_ticks'.  Synchronises."""
        sd = super().state_dict()
        counts = self._ffc_state[:, :2].tolist()
        for group, (t, s) in zip(sd["param_groups"], counts):
            group[TICKS_KEY] = int(s)
            for i in group["params"]:
                if i in sd["state"]:
                    sd["state"][i] = dict(sd["state"][i], step=torch.tensor(float(t), dtype=torch.float32))
        return sd

    def load_state_dict(self, state_dict):
        """a FusedAdam(W) or torch.optim.Adam(W) state dict; the parameters of one group must share one ``step``"""
        super().load_state_dict(state_dict)
        counts = []
        for group in self.param_groups:
            steps = {float(self.state[p].pop("step")) for p in group["params"] if "step" in self.state.get(p, {})}
            if len(steps) > 1:
                raise NotImplementedError(f"{type(self).__name__}: one step count per param group "
                                          f"(the state dict holds {sorted(steps)})")
            counts.append([int(steps.pop()) if steps else 0, int(group.pop(TICKS_KEY, 0)), 0, 0])
        self._ffc_state.copy_(torch.tensor(counts, dtype=torch.int64))


class FusedAdamW(_Fused, torch.optim.AdamW):
    """torch.optim.AdamW on libffc_amd.so; ``decay_steps=T``: lr * max(0, 1 - s / T) with s advanced by lr_step()"""
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, decay_steps=None):
        self._ffc_init(decay_steps, amsgrad, maximize)
        torch.optim.AdamW.__init__(self, params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class FusedAdam(_Fused, torch.optim.Adam):
    """torch.optim.Adam (L2 weight decay added to the gradient) on libffc_amd.so; ``decay_steps`` as FusedAdamW"""
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 maximize=False, decay_steps=None):
        self._ffc_init(decay_steps, amsgrad, maximize)
        torch.optim.Adam.__init__(self, params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
