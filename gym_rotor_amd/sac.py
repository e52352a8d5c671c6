"""The critic half of a SAC update on the device: the soft target values of a minibatch in one launch (`sac_target`: qr_sac_target)
and, on live modules, the whole critic update (`sac_critic_loss`: `sac_target`, then `td3.twinq_grad`).  The replay buffer, the
twin-Q regression and the Polyak step are td3.py's (`ReplayBuffer`, `twinq_grad`, `soft_update`): SAC's critic has TD3's form.

Replaces, per minibatch of `SAC.train` (algos/sac/sac.py:123-170, the non-CTDE branch without the spectral-norm term): the index
clones, `actor.sample` on obs_next (two heads, the clamp, rsample, tanh, the log-probability with its tanh correction), the target
critic's two passes, min, the entropy term and the Bellman line, two mse_loss and the autograd backward pass.  The actor half, alpha's
own update and the optimiser group of twelve tensors are not here (twelve tensors: two `optim.DeviceAdamW` groups of six).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Union

import torch

from . import _lib
from .policy import ActorParams, PPO_ACTOR_DIMS, QCriticParams
from .td3 import ReplayBuffer, _agent_tensors, _check_index, _column, _rows, twinq_grad, twinq_workspace_bytes


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
    t = _agent_tensors(buffer_or_tensors, k)
    dev = critic_target.device
    D, A, H = critic_target.dims
    rows = _rows(t.get("obs_next"), D, dev, what, "obs_next")
    rs, ds = _column(t.get("rwd"), rows, dev, what, "rwd"), _column(t.get("done"), rows, dev, what, "done")
    _check_index(index, dev, what)
    B = rows if index is None else index.numel()
    if actor is not None:
        if actor.dims not in PPO_ACTOR_DIMS:
            raise ValueError(f"{what}: actor sizes {actor.dims} are not among {PPO_ACTOR_DIMS} (obs, hidden, action)")
        if actor.squash != _lib.ACTOR_TANH_SAMPLE or actor.log_std_w is None or actor.log_std_b is None:
            raise ValueError(f"{what}: the actor must be of MLP_Actor_SAC's form: the tanh-of-sample rule with a log_std head")
        if (actor.dims[0], actor.dims[2]) != (D, A):
            raise ValueError(f"{what}: the actor maps {actor.dims[0]} -> {actor.dims[2]}, the critic reads {D} + {A}")
        Da, Ha, Aa = actor.dims
        ashapes = {"fc1_w": (Ha, Da), "fc1_b": (Ha,), "fc2_w": (Ha, Ha), "fc2_b": (Ha,), "mean_w": (Aa, Ha), "mean_b": (Aa,),
                   "log_std_w": (Aa, Ha), "log_std_b": (Aa,)}
        for n, shp in ashapes.items():   # (log_std is not read: whatever it holds is not checked)
            w = getattr(actor, n)
            if tuple(w.shape) != shp or w.dtype != torch.float32 or w.device != dev or not w.is_contiguous():
                raise ValueError(f"{what}: actor tensor {n} must be a contiguous float32 {shp} tensor on {dev}")
    elif action_next is None or logp_next is None:
        raise ValueError(f"{what}: without an actor, action_next [B, {A}] and logp_next [B] are required")
    for name, x in (("noise", noise), ("action_next", action_next), ("action_out", action_out)):
        if x is not None and (x.dtype != torch.float32 or x.device != dev or tuple(x.shape) != (B, A) or not x.is_contiguous()):
            raise ValueError(f"{what}: {name} must be a contiguous float32 [{B}, {A}] tensor on {dev}")
    for name, x in (("logp_next", logp_next), ("logp_out", logp_out)):
        if x is not None and (x.dtype != torch.float32 or x.device != dev or x.numel() != B or not x.is_contiguous()):
            raise ValueError(f"{what}: {name} must be a contiguous float32 [{B}] tensor on {dev}")
    alpha_dev = None
    if isinstance(alpha, torch.Tensor):
        if alpha.dtype != torch.float32 or alpha.device != dev or alpha.numel() != 1:
            raise ValueError(f"{what}: alpha must be a Python float or a float32 tensor of one element on {dev}")
        alpha_dev, alpha = alpha, 0.0
    elif not 0.0 <= float(alpha) < float("inf"):
        raise ValueError(f"{what}: alpha must be finite and >= 0, got {alpha}")
    if not 0.0 <= float(discount) < float("inf"):
        raise ValueError(f"{what}: discount must be finite and >= 0, got {discount}")
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.device != dev or out.numel() != B or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous float32 [{B}] tensor on {dev}")
    if dev.type != "cuda":
        raise RuntimeError("gym_rotor_amd ops run on the GPU only (no CPU kernel exists)")
    if B == 0:
        return out
    b = _lib.transitions(obs_next=t["obs_next"], reward=t["rwd"], done=t["done"], index=index, batch=B, rows=rows, reward_stride=rs, done_stride=ds)
    g = _lib.sac_target_args(eps=noise, action_next=action_next, logp_next=logp_next, alpha_dev=alpha_dev, y=out, action_out=action_out,
                             logp_out=logp_out, discount=discount, alpha=alpha)
    q = critic_target.as_c()
    if actor is not None:
        p = actor.as_c()
        p.log_std = None
    with torch.cuda.device(dev):
        rc = _lib.load().qr_sac_target(C.byref(p) if actor is not None else None, C.byref(q), C.byref(b), C.byref(g),
                                       torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "qr_sac_target")
    return out


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
    layers = [getattr(critic_module, f"fc{j}") for j in range(1, 7)]
    grads = {}
    for n, p in zip(_lib.TWINQ_GRAD_NAMES, (t for l in layers for t in (l.weight, l.bias))):
        if p.grad is None or not p.grad.is_contiguous():
            p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
        grads[n] = p.grad
    critic = QCriticParams.from_module(critic_module, A)
    B = buffer.capacity if index is None else index.numel()
    key = ("sac", k, B, int(max_workgroups))
    hit = buffer._cache.get(key)
    if hit is None:
        dev = critic.device
        need = twinq_workspace_bytes(critic.dims, B, max_workgroups) // 8 if B else 0
        hit = buffer._cache[key] = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(need, dtype=torch.float64, device=dev),
                                    torch.empty(4, dtype=torch.float32, device=dev))
    y, workspace, own_stats = hit
    sac_target(ActorParams.from_sac_module(actor_module), QCriticParams.from_module(critic_target_module, A), buffer, k, index,
               discount=discount, alpha=alpha, noise=noise, out=y)
    _, stats = twinq_grad(critic, buffer.obs[k], buffer.act[k], y, index, grads=grads, stats=own_stats if stats is None else stats,
                          workspace=workspace, max_workgroups=max_workgroups)
    return stats
