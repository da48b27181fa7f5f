"""aw_method (layers/aw_loss.py): the adaptive-weight critic loss, with its weights kept on the device.

The reference runs two backward passes into ``param.grad``, clones and concatenates every gradient
twice, reads three dot products and two scores back to the host and branches there.  Here the two
gradient lists come from ``torch.autograd.grad`` and go through two ops on csrc/aw_kernels.hip:
``ffc::aw_weights`` (the dots, the scores and the case of Algorithm 1 / 2, into an fp64 stats vector
on the device) and ``ffc::aw_combine`` (w_r * g_real + w_f * g_fake into ``param.grad``).  Nothing
synchronises with the host, so the step can be captured into a graph."""
import torch

__all__ = ["aw_method"]


class aw_method():
    def __init__(self, alpha1=0.5, alpha2=0.75, delta=0.05, epsilon=0.05, normalized_aw=True):
        assert alpha1 < alpha2
        self._alpha1 = alpha1
        self._alpha2 = alpha2
        self._delta = delta
        self._epsilon = epsilon
        self._normalized_aw = normalized_aw
        self.last_stats = None   # [rr, ff, rf, rs, fs, w_r, w_f, case] of the last call: fp64, on the device

    def aw_loss(self, Dloss_real, Dloss_fake, Dis_opt, Dis_Net, real_validity, fake_validity):
        """aw_loss.py:13-107.  On return every ``param.grad`` of ``Dis_Net`` holds
        w_r * dDloss_real/dparam + w_f * dDloss_fake/dparam (written in place where a matching ``.grad``
        exists), ``self.last_stats`` the device stats; returns w_r * Dloss_real + w_f * Dloss_fake.
        ``Dis_opt`` is taken for the reference's signature: no ``zero_grad`` is needed."""
        named = list(Dis_Net.named_parameters())
        if not named:
            raise ValueError("aw_loss: Dis_Net has no parameters")
        for name, p in named:
            if not p.is_cuda or p.dtype != torch.float32:
                raise NotImplementedError(f"aw_loss: fp32 parameters on the GPU only ({name}: {p.dtype} on {p.device})")
        params = [p for _, p in named]
        g_real = torch.autograd.grad(Dloss_real, params, retain_graph=True, allow_unused=True)
        g_fake = torch.autograd.grad(Dloss_fake, params, retain_graph=True, allow_unused=True)
        for (name, _), gr, gf in zip(named, g_real, g_fake):
            if gr is None or gf is None:   # the reference fails here too, on None.clone()
                raise RuntimeError(f"aw_loss: parameter {name} receives no gradient from "
                                   f"{'Dloss_real' if gr is None else 'Dloss_fake'}")
        g_real = [g.contiguous() for g in g_real]
        g_fake = [g.contiguous() for g in g_fake]
        stats = torch.ops.ffc.aw_weights(g_real, g_fake, real_validity.detach(), fake_validity.detach(),
                                         float(self._alpha1), float(self._alpha2), float(self._delta),
                                         float(self._epsilon), bool(self._normalized_aw))
        out = []
        for p in params:
            g = p.grad
            if g is None or g.shape != p.shape or g.dtype != p.dtype or g.device != p.device or \
                    not g.is_contiguous():
                g = torch.empty(p.shape, dtype=p.dtype, device=p.device)
            out.append(g)
        torch.ops.ffc.aw_combine(g_real, g_fake, stats, out)
        for p, g in zip(params, out):
            if p.grad is not g:
                p.grad = g
        self.last_stats = stats
        w = stats[5:7].to(Dloss_real.dtype)   # the reference's Python floats take the losses' dtype
        return w[0] * Dloss_real + w[1] * Dloss_fake
