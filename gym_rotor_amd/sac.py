"""The critic half of a SAC update on the device: the soft target values of a minibatch in one launch (`sac_target`: qr_sac_target)
and, on live modules, the whole critic update (`sac_critic_loss`: `sac_target`, then `td3.twinq_grad`).  The replay buffer, the
twin-Q regression and the Polyak step are td3.py's (`ReplayBuffer`, `twinq_grad`, `soft_update`): SAC's critic has TD3's form.

Replaces, per minibatch of `SAC.train` (algos/sac/sac.py:123-170, the non-CTDE branch without the spectral-norm term): the index
clones, `actor.sample` on obs_next (two heads, the clamp, rsample, tanh, the log-probability with its tanh correction), the target
critic's two passes, min, the entropy term and the Bellman line, two mse_loss and the autograd backward pass.  The actor half, alpha's
own update and the optimiser group of twelve tensors are not here (twelve tensors: two `optim.DeviceAdamW` groups of six).
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import _lib
from .policy import ActorParams, QCriticParams
from .td3 import ReplayBuffer, _critic_update_state, _target, twinq_grad


def sac_target(actor: Optional[ActorParams], critic_target: QCriticParams, buffer_or_tensors, k: int = 0,
               index: Optional[torch.Tensor] = None, *, discount: float = 0.99, alpha: Union[float, torch.Tensor] = 0.2,
               noise: Optional[torch.Tensor] = None, action_next: Optional[torch.Tensor] = None, logp_next: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, action_out: Optional[torch.Tensor] = None,
               logp_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SAC's target values of one minibatch in one launch (qr_sac_target; sac.py:135-153), j the minibatch position, i = index[j]:
        mean, ls = actor(obs_next[i]);  ls = clamp(ls, -20, 2);  a'_j = tanh(mean + exp(ls) * noise[j])
        logp_j = sum_f [ -noise[j]^2 / 2 - ls - log sqrt(2 pi) - log(1 - a'^2 + 1e-6) ]
        y[j] = rwd[i] + discount * (1 - done[i]) * (min(Q1, Q2)(obs_next[i], a'_j) - alpha * logp_j)
    actor: `ActorParams.from_sac_module(module)` — the LIVE actor, SAC has no target actor — in one of the three sizes of the rollout,
    or None with action_next [B, A] and logp_next [B] float32, used as they are.  buffer_or_tensors: a `ReplayBuffer` (agent k's
    tensors) or a dict with obs_next [rows, D], rwd, done (float32, `rows` elements, one stride).  noise: float32 [B, A]
    standard-normal draws by minibatch position (rsample's), None: zeros.  alpha: a Python float, or a float32 tensor of one element
    on the device that the kernel reads (no host synchronisation).  index: int64 [B], None: all rows in order.  action_out [B, A],
    logp_out [B]: optional outputs a' and logp.  Returns y float32 [B] (`out` given: written in place)."""
    what = "sac_target"

    def own(B, A, dev):   # what follows _target's check of noise and action_next; the keywords of sac_target_args that are SAC's
        x = action_out
        if x is not None and (x.dtype != torch.float32 or x.device != dev or tuple(x.shape) != (B, A) or not x.is_contiguous()):
            raise ValueError(f"{what}: action_out must be a contiguous float32 [{B}, {A}] tensor on {dev}")
        for name, x in (("logp_next", logp_next), ("logp_out", logp_out)):
            if x is not None and (x.dtype != torch.float32 or x.device != dev or x.numel() != B or not x.is_contiguous()):
                raise ValueError(f"{what}: {name} must be a contiguous float32 [{B}] tensor on {dev}")
        a, alpha_dev = alpha, None
        if isinstance(a, torch.Tensor):
            if a.dtype != torch.float32 or a.device != dev or a.numel() != 1:
                raise ValueError(f"{what}: alpha must be a Python float or a float32 tensor of one element on {dev}")
            alpha_dev, a = a, 0.0
        elif not 0.0 <= float(a) < float("inf"):
            raise ValueError(f"{what}: alpha must be finite and >= 0, got {a}")
        if not 0.0 <= float(discount) < float("inf"):
            raise ValueError(f"{what}: discount must be finite and >= 0, got {discount}")
        return dict(logp_next=logp_next, alpha_dev=alpha_dev, action_out=action_out, logp_out=logp_out, discount=discount, alpha=a)

    A = critic_target.dims[1]
    return _target(what, "qr_sac_target", _lib.sac_target_args, actor,
                   (_lib.ACTOR_TANH_SAMPLE, True, "the actor must be of MLP_Actor_SAC's form: the tanh-of-sample rule with a log_std head"),
                   f"without an actor, action_next [B, {A}] and logp_next [B] are required" if action_next is None or logp_next is None else None,
                   critic_target, buffer_or_tensors, k, index, noise, action_next, out, own)


def sac_critic_loss(critic_module, critic_target_module, actor_module, buffer: ReplayBuffer, k: int = 0, index: Optional[torch.Tensor] = None, *,
                    discount: float = 0.99, alpha: Union[float, torch.Tensor] = 0.2, noise: Optional[torch.Tensor] = None,
                    stats: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> torch.Tensor:
    """The critic update of SAC.train, as the reference writes it, without autograd: `sac_target` on the LIVE `actor_module`
    (attributes fc1, fc2, mean_linear, log_std_linear) and the target critic, then `twinq_grad` on the live `critic_module` (attributes
    fc1 .. fc6 — its tensors are read in place) for agent k of `buffer`; writes the gradients into
    `critic_module.fc{1..6}.{weight,bias}.grad` in place, as `loss.backward()` after `zero_grad()` leaves them.  noise: the [B, A]
    standard-normal draws of the sample (rsample in the reference), None: zeros.  alpha: a float, or the device tensor of automatic
    entropy tuning.  Returns stats (stats[0] = the loss).  From the second call on with an unchanged B nothing is allocated: y, the
    workspace and stats are cached on the buffer.  The optimiser step follows on these .grad tensors (two `optim.DeviceAdamW` groups
    of six tensors, or torch's), then `soft_update(critic_module, critic_target_module, tau)`."""
    if not isinstance(buffer, ReplayBuffer):
        raise ValueError("sac_critic_loss: buffer must be a ReplayBuffer")
    A = buffer.action_dims[k]
    grads, critic, (y, workspace, own_stats) = _critic_update_state(critic_module, buffer, k, index, max_workgroups, ("sac",))
    sac_target(ActorParams.from_sac_module(actor_module), QCriticParams.from_module(critic_target_module, A), buffer, k, index,
               discount=discount, alpha=alpha, noise=noise, out=y)
    _, stats = twinq_grad(critic, buffer.obs[k], buffer.act[k], y, index, grads=grads, stats=own_stats if stats is None else stats,
                          workspace=workspace, max_workgroups=max_workgroups)
    return stats
