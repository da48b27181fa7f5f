"""The fgan128 training iteration (fgan128_complete.py:666-703) over the HIP layers: the reference's
hinge losses and its generator / discriminator updates, restated as functions so a caller (or a
hipGraph capture, bench.py --workload fgan128train) can run the same step the reference's loop runs.

Every convolution, Fourier unit, BatchNorm, activation, NoiseInjection and Linear of G and D runs
on libffc_amd.so (forward and backward); the hinge losses (a few ops on a (B, 1) tensor), the
spectral-norm power iteration (torch.nn.utils.spectral_norm's own hook, on the GPU) and the
optimizer are torch's, as in the reference.  Every step function takes any optimizer: optim.FusedAdamW /
FusedAdam run the update on libffc_amd.so too, with the reference's LR decay inside a captured iteration."""
import torch
import torch.nn.functional as tF


def hinge_loss_dis(fake, real):
    """fgan128_complete.py:566-572"""
    assert fake.dim() == 2 and fake.shape[1] == 1 and real.shape == fake.shape, f"{fake.shape} {real.shape}"
    return tF.relu(1.0 - real).mean() + tF.relu(1.0 + fake).mean()


def hinge_loss_real(real):
    """fgan128_complete.py:574-576: the real half of hinge_loss_dis"""
    return tF.relu(1.0 - real).mean()


def hinge_loss_fake(fake):
    """fgan128_complete.py:578-579: the fake half of hinge_loss_dis"""
    return tF.relu(1.0 + fake).mean()


def hinge_loss_gen(fake):
    """fgan128_complete.py:581-585"""
    assert fake.dim() == 2 and fake.shape[1] == 1, f"{fake.shape}"
    return -fake.mean()


def generator_step(G, D, optim_G, optim_D, z, noises=None, labels=None):
    """fgan128_complete.py:680-690: G trainable, D frozen; loss_G = hinge_loss_gen(D(G(z))), backward
    through D into G, optim_G.step().  ``noises``: explicit NoiseInjection noise (FGenerator.forward);
    None draws it on the GPU as the reference does.  ``labels`` (B,) int64 on the GPU: the conditional
    step of fgan128_cond_complete.py:296-308 over FCondGenerator / FCondDiscriminator,
    loss_G = hinge_loss_gen(D(G(z, labels), labels))."""
    G.requires_grad_(True)
    D.requires_grad_(False)
    optim_D.zero_grad()
    optim_G.zero_grad()
    if labels is None:
        fake = G(z) if noises is None else G(z, noises)   # the baseline generators take z alone
        loss_G = hinge_loss_gen(D(fake))
    else:
        fake = G(z, labels, noises)
        loss_G = hinge_loss_gen(D(fake, labels))
    loss_G.backward()
    optim_G.step()
    return loss_G


def discriminator_step(G, D, optim_G, optim_D, z, real, noises=None, labels=None):
    """fgan128_complete.py:692-703 (one of num_dis_updates): G frozen (its forward takes the
    no-grad inference path), loss_D = hinge_loss_dis(D(G(z)), D(real)) in the reference's call order,
    backward into D, optim_D.step().  ``labels``: the conditional step of
    fgan128_cond_complete.py:311-324, the real batch's labels on both critic calls."""
    G.requires_grad_(False)
    D.requires_grad_(True)
    optim_D.zero_grad()
    optim_G.zero_grad()
    if labels is None:
        fake = G(z) if noises is None else G(z, noises)   # the baseline generators take z alone
        output_dg = D(fake)
        output_dreal = D(real)
    else:
        fake = G(z, labels, noises)
        output_dg = D(fake, labels)
        output_dreal = D(real, labels)
    loss_D = hinge_loss_dis(output_dg, output_dreal)
    loss_D.backward()
    optim_D.step()
    return loss_D


def aw_discriminator_step(G, D, optim_G, optim_D, z, real, aw, noises=None, labels=None):
    """discriminator_step with the adaptive-weight loss (layers/aw_loss.py) in place of hinge_loss_dis:
    the same two critic calls, then ``aw.aw_loss`` (an aw_loss.aw_method) over the two hinge halves, which
    takes both gradients through the one retained graph and leaves w_r * g_real + w_f * g_fake in
    D's ``.grad``s, then optim_D.step().  Under set_sn_hip SpectralNormWeight.backward runs once per
    gradient pass on the tensors it saved; the two passes share nothing they write."""
    G.requires_grad_(False)
    D.requires_grad_(True)
    optim_G.zero_grad()
    if labels is None:
        fake = G(z) if noises is None else G(z, noises)
        output_dg = D(fake)
        output_dreal = D(real)
    else:
        fake = G(z, labels, noises)
        output_dg = D(fake, labels)
        output_dreal = D(real, labels)
    loss_D = aw.aw_loss(hinge_loss_real(output_dreal), hinge_loss_fake(output_dg), optim_D, D, output_dreal,
                        output_dg)
    optim_D.step()
    return loss_D


def train_iteration(G, D, optim_G, optim_D, z_g, z_d, real, num_dis_updates=1, labels=None):
    """one iteration of the reference's loop body (:680-703) without its logging / LR schedule:
    a generator update, then ``num_dis_updates`` discriminator updates (z_d: one z per update)"""
    loss_G = generator_step(G, D, optim_G, optim_D, z_g, labels=labels)
    zs = z_d if isinstance(z_d, (list, tuple)) else [z_d]
    assert len(zs) == num_dis_updates
    loss_D = None
    for z in zs:
        loss_D = discriminator_step(G, D, optim_G, optim_D, z, real, labels=labels)
    return loss_G, loss_D


def sagan_step(G, D, optim_G, optim_D, z_d, z_g, real, adv_loss='hinge'):
    """benchmark_models/sagan/trainer.py:93-168 with ``adv_loss = 'hinge'``, over sagan.SAGANGenerator /
    SAGANDiscriminator, in the reference's call order: both models in train mode;
    D half: d_loss_real = relu(1 - D(real)).mean(), d_loss_fake = relu(1 + D(G(z_d))).mean(), both optimizers'
    gradients reset, (d_loss_real + d_loss_fake).backward(), optim_D.step();
    G half: g_loss = -D(G(z_g)).mean() on the updated critic, gradients reset, backward, optim_G.step().
    -> (d_loss_real, d_loss_fake, g_loss), on the device.

    One call runs D's spectral-norm wrappers three times and G's twice, so u and v advance that often, and G's
    BatchNorm running statistics update in both halves, as in the reference.  Two things are not computed because
    the reference throws them away: the D half runs G without recording its graph (the gradients d_loss.backward()
    would leave in G are reset at :166 before anything reads them), and the G half does not accumulate the
    critic's parameter gradients (they are reset at :125 of the next iteration); after the call D's ``.grad``s are
    unset where the reference would hold those of g_loss.

    ``adv_loss = 'wgan-gp'`` (the reference's default) raises NotImplementedError: its gradient penalty
    differentiates a gradient of D, a double backward the custom ops do not have.  Takes torch's optimizers or
    optim.FusedAdam (the reference: Adam, lr 1e-4 for G and 4e-4 for D, betas (0.0, 0.9), over the parameters
    that require a gradient)."""
    if adv_loss == 'wgan-gp':
        raise NotImplementedError("sagan_step: adv_loss = 'wgan-gp' needs the gradient penalty, a double backward "
                                  "through every layer of D that the custom ops do not have; use 'hinge'")
    if adv_loss != 'hinge':
        raise NotImplementedError(f"sagan_step: adv_loss = {adv_loss!r} ('hinge' only)")
    D.train()
    G.train()
    d_out_real, _ = D(real)
    d_loss_real = tF.relu(1.0 - d_out_real).mean()
    with torch.no_grad():
        fake_images, _ = G(z_d)
    d_out_fake, _ = D(fake_images)
    d_loss_fake = tF.relu(1.0 + d_out_fake).mean()
    d_loss = d_loss_real + d_loss_fake
    optim_D.zero_grad()
    optim_G.zero_grad()
    d_loss.backward()
    optim_D.step()

    fake_images, _ = G(z_g)
    trained = [p for p in D.parameters() if p.requires_grad]
    for p in trained:
        p.requires_grad_(False)
    try:
        g_out_fake, _ = D(fake_images)
    finally:
        for p in trained:
            p.requires_grad_(True)
    g_loss_fake = -g_out_fake.mean()
    optim_D.zero_grad()
    optim_G.zero_grad()
    g_loss_fake.backward()
    optim_G.step()
    return d_loss_real, d_loss_fake, g_loss_fake
