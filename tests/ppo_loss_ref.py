"""Plain PyTorch restatement of RLlib 2.4's PPO loss for the 2-vs-2 policies (test infrastructure): the yardstick of hh_ppo_loss
(include/hh_learner.h) and of hhmarl_2d_amd.learner.ppo_loss.  `ray` is not a dependency of this repository, so, as with GAE
(oracle/gae_ref.py), every line names the ray function it restates; dtype-generic (the dtype of `logits`): float64 is the reference,
float32 measures what the format itself costs.

Where ray decides something that the issue text leaves open, this file follows ray:
  * the KL term and mean_kl exist only when kl_coeff > 0 (`if self.config["kl_coeff"] > 0.0`), mean_kl is 0.0 otherwise;
  * reduce_mean_valid is `torch.sum(t[mask]) / num_valid` for a recurrent model (Fight1 / Fight2: ModelV2.__call__ returns the dummy
    state_in as the state, so `if state:` holds) and `torch.mean` otherwise."""
import torch

SPLITS = {4: (13, 9, 2, 2), 3: (13, 9, 2)}


def categorical_logp(inputs, a):
    """TorchCategorical.logp: torch.distributions.Categorical(logits=inputs).log_prob(a)"""
    return torch.distributions.Categorical(logits=inputs).log_prob(a)


def categorical_entropy(inputs):
    """TorchCategorical.entropy (ray/rllib/models/torch/torch_action_dist.py)"""
    a0 = inputs - torch.max(inputs, dim=1, keepdim=True)[0]
    ea0 = torch.exp(a0)
    z0 = torch.sum(ea0, dim=1, keepdim=True)
    p0 = ea0 / z0
    return torch.sum(p0 * (torch.log(z0) - a0), dim=1)


def categorical_kl(inputs, other):
    """TorchCategorical.kl: KL(self || other)"""
    a0 = inputs - torch.max(inputs, dim=1, keepdim=True)[0]
    a1 = other - torch.max(other, dim=1, keepdim=True)[0]
    ea0, ea1 = torch.exp(a0), torch.exp(a1)
    z0, z1 = torch.sum(ea0, dim=1, keepdim=True), torch.sum(ea1, dim=1, keepdim=True)
    p0 = ea0 / z0
    return torch.sum(p0 * (a0 - torch.log(z0) - a1 + torch.log(z1)), dim=1)


def ppo_loss(logits, vf, old_logits, actions, old_logp, adv, target, mask, *, n_comp, clip_param, vf_clip_param, vf_loss_coeff,
             entropy_coeff, kl_coeff):
    """PPOTorchPolicy.loss (ray/rllib/algorithms/ppo/ppo_torch_policy.py).  logits [R, >= 26 | 24] and vf [R] in the working dtype (may
    require grad); old_logits [R, >= 26 | 24], actions integer [R, 4], old_logp / adv / target [R]; mask bool [R] or None.
    -> (total_loss, dict of the statistics ray reports: mean_policy_loss, mean_vf_loss, mean_kl, mean_entropy, n_valid)"""
    dt = logits.dtype
    splits = SPLITS[n_comp]
    n_out = sum(splits)
    cur = logits[:, :n_out].split(splits, dim=1)                  # TorchMultiCategorical.__init__: torch.split(inputs, input_lens, dim=1)
    prev = old_logits[:, :n_out].to(dt).split(splits, dim=1)
    a = actions.long()
    # TorchMultiCategorical.logp / entropy / kl: torch.stack over the components, summed over dim 1
    logp = torch.stack([categorical_logp(c, a[:, i]) for i, c in enumerate(cur)], dim=1).sum(dim=1)
    entropy = torch.stack([categorical_entropy(c) for c in cur], dim=1).sum(dim=1)
    if mask is not None:                                           # RNN case
        num_valid = torch.sum(mask)
        reduce_mean_valid = lambda t: torch.sum(t[mask]) / num_valid
    else:
        num_valid = torch.tensor(logits.shape[0])
        reduce_mean_valid = torch.mean
    logp_ratio = torch.exp(logp - old_logp.to(dt))
    if kl_coeff > 0.0:
        action_kl = torch.stack([categorical_kl(p, c) for p, c in zip(prev, cur)], dim=1).sum(dim=1)   # prev_action_dist.kl(curr_action_dist)
        mean_kl_loss = reduce_mean_valid(action_kl)
    else:
        mean_kl_loss = torch.tensor(0.0, dtype=dt, device=logits.device)
    mean_entropy = reduce_mean_valid(entropy)
    A = adv.to(dt)
    surrogate_loss = torch.min(A * logp_ratio, A * torch.clamp(logp_ratio, 1 - clip_param, 1 + clip_param))
    vf_loss = torch.pow(vf - target.to(dt), 2.0)
    vf_loss_clipped = torch.clamp(vf_loss, 0, vf_clip_param)
    mean_vf_loss = reduce_mean_valid(vf_loss_clipped)
    total_loss = reduce_mean_valid(-surrogate_loss + vf_loss_coeff * vf_loss_clipped - entropy_coeff * entropy)
    if kl_coeff > 0.0:
        total_loss = total_loss + kl_coeff * mean_kl_loss
    stats = {"total_loss": total_loss, "mean_policy_loss": reduce_mean_valid(-surrogate_loss), "mean_vf_loss": mean_vf_loss,
             "mean_kl": mean_kl_loss, "mean_entropy": mean_entropy, "n_valid": num_valid}
    aux = {"ratio": logp_ratio.detach(), "vf_sq": vf_loss.detach()}
    return total_loss, stats, aux


def make_inputs(R, n_comp, ld, masked, seed, clip_param=0.25, vf_clip_param=10.0):
    """Seeded inputs (float32 / int8 / bool CPU tensors) that reach every branch of the loss: the learner's logits are the sampler's plus
    a perturbation whose scale varies by row (ratios from ~1 to far outside [1 - clip, 1 + clip], both sides), advantages of both signs,
    value errors on both sides of sqrt(vf_clip_param).  Rows within the issue's exclusion bands of a kink are rare by construction
    (the ratio and the squared value error are continuous variables with densities of order 1 there): near_kink() counts them."""
    g = torch.Generator().manual_seed(int(seed) * 1000003 + R * 7 + n_comp * 3 + ld + (1 if masked else 0))
    n_out = sum(SPLITS[n_comp])
    old = torch.zeros((R, 32))
    old[:, :n_out] = torch.randn((R, n_out), generator=g) * 1.5
    scale = torch.rand((R, 1), generator=g) ** 2 * 0.8
    logits = torch.randn((R, ld), generator=g)                   # the columns beyond n_out hold junk on purpose
    logits[:, :n_out] = old[:, :n_out] + scale * torch.randn((R, n_out), generator=g)
    actions = torch.zeros((R, 4), dtype=torch.int8)
    for i, w in enumerate(SPLITS[n_comp]):
        actions[:, i] = torch.randint(0, w, (R,), generator=g).to(torch.int8)
    lo = 0
    old_logp = torch.zeros(R)
    for i, w in enumerate(SPLITS[n_comp]):
        old_logp += torch.log_softmax(old[:, lo:lo + w].double(), dim=1).gather(1, actions[:, i:i + 1].long()).squeeze(1).float()
        lo += w
    adv = torch.randn(R, generator=g)
    vf = torch.randn(R, generator=g) * 2.0
    target = vf + torch.randn(R, generator=g) * (vf_clip_param ** 0.5)
    mask = (torch.rand(R, generator=g) < 0.8) if masked else None
    if masked:
        mask[0] = True
    return dict(logits=logits, vf=vf, old_logits=old, actions=actions, old_logp=old_logp, adv=adv, target=target, mask=mask)


def near_kink(aux, clip_param, vf_clip_param):
    """rows whose gradient the issue lets a comparison leave out: |ratio - (1 +- clip)| < 1e-4 or |(vf - target)^2 - vf_clip_param| < 1e-3"""
    r, s = aux["ratio"], aux["vf_sq"]
    return ((r - (1 - clip_param)).abs() < 1e-4) | ((r - (1 + clip_param)).abs() < 1e-4) | ((s - vf_clip_param).abs() < 1e-3)


def reference(inp, dtype, **kw):
    """the restatement and its autograd gradients on make_inputs' tensors in `dtype` -> (stats as a list of 6 floats in the order of
    hh_ppo_loss's, d_logits [R, ld], d_vf [R], aux)"""
    logits = inp["logits"].detach().to(dtype).clone().requires_grad_(True)
    vf = inp["vf"].detach().to(dtype).clone().requires_grad_(True)
    total, st, aux = ppo_loss(logits, vf, inp["old_logits"], inp["actions"], inp["old_logp"], inp["adv"], inp["target"], inp["mask"], **kw)
    total.backward()
    order = ("total_loss", "mean_policy_loss", "mean_vf_loss", "mean_kl", "mean_entropy", "n_valid")
    return [float(st[k].detach()) if torch.is_tensor(st[k]) else float(st[k]) for k in order], logits.grad, vf.grad, aux
