"""Both halves of a SAC update on the device.  The critic half: the soft target values of a minibatch in one launch (`sac_target`: qr_sac_target)
and, on live modules, the whole critic update (`sac_critic_loss`: `sac_target`, then `td3.twinq_grad`).  The replay buffer, the
twin-Q regression and the Polyak step are td3.py's (`ReplayBuffer`, `twinq_grad`, `soft_update`): SAC's critic has TD3's form.

Replaces, per minibatch of `SAC.train` (algos/sac/sac.py:123-170, the non-CTDE branch without the spectral-norm term): the index
clones, `actor.sample` on obs_next (two heads, the clamp, rsample, tanh, the log-probability with its tanh correction), the target
critic's two passes, min, the entropy term and the Bellman line, two mse_loss and the autograd backward pass.

The actor half (`sac_actor_grad`: qr_sac_actor_grad; on live modules `sac_actor_loss`) replaces, per minibatch (sac.py:182-211 with
algos/policy_regularization.py): the index clones, four `actor.sample` passes, two critic passes, min, the three smoothness terms and
autograd through all of it — and leaves d alpha_loss / d log_alpha beside the gradients.  The optimiser steps stay the caller's: no
updater class is built here.

The critic half also exists for ONE centralized (CTDE) twin critic over the two agents of a Decoupled buffer (sac.py:136-144, 156-157):
`sac_target_ctde` (qr_ctde_sac_target) and, on live modules, `sac_critic_loss_ctde`; the regression is `td3.twinq_grad_ctde`.
So does agent k's actor half under that critic (sac.py:175-203): `sac_actor_grad_ctde` (qr_ctde_sac_actor_grad) and, on live modules,
`sac_actor_loss_ctde`, which replaces both actors' samples, two `torch.cat`, both critics, min, the second sample of agent k, the three
regulariser samples and autograd through all of it.
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import _checks as ck
from . import _lib
from .policy import PPO_ACTOR_DIMS, ActorParams, QCriticParams, _grad_outputs, module_grads
from .td3 import ReplayBuffer, _critic_update_state, _ctde_actor_launch, _ctde_actors_c, _target, _target_ctde, twinq_grad, twinq_grad_ctde


_EPS = ("eps", "eps_reg", "eps_next", "eps_pert")   # sac_actor_grad's four [B, A] draws


def _entropy_terms(what: str, alpha, target_entropy, alpha_grad, A: int, dev):
    """(alpha, alpha_dev, target_entropy) of a SAC actor launch, checked, and the check of alpha_grad; target_entropy None: -A."""
    a, alpha_dev = ck.alpha(what, alpha, dev)
    te = -float(A) if target_entropy is None else float(target_entropy)
    if not -float("inf") < te < float("inf"):
        raise ValueError(f"{what}: target_entropy must be finite, got {target_entropy}")
    ck.scalar(what, "alpha_grad", alpha_grad, torch.float32, dev)
    return a, alpha_dev, te


def _actor_grads(what: str, m, log_alpha) -> dict:
    """The live SAC actor's eight .grad tensors by name, and log_alpha's where it is given, made where there is none."""
    params = [t for l in (m.fc1, m.fc2, m.mean_linear, m.log_std_linear) for t in (l.weight, l.bias)]
    if log_alpha is not None:
        if log_alpha.numel() != 1:
            raise ValueError(f"{what}: log_alpha must have one element")
        params.append(log_alpha)
    return module_grads(_lib.SAC_ACTOR_GRAD_NAMES, params)


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
        ck.tensor(what, "action_out", action_out, torch.float32, (B, A), dev, True)
        ck.flat(what, "logp_next", logp_next, torch.float32, B, dev, True)
        ck.flat(what, "logp_out", logp_out, torch.float32, B, dev, True)
        a, alpha_dev = ck.alpha(what, alpha, dev)
        ck.nonneg(what, ("discount",), discount)
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
    workspace and stats are cached on the buffer.  The optimiser step follows on these .grad tensors (one `optim.PolyakAdamW` group
    of all twelve tensors, which can carry the soft update, or torch's and `soft_update(critic_module, critic_target_module, tau)`)."""
    if not isinstance(buffer, ReplayBuffer):
        raise ValueError("sac_critic_loss: buffer must be a ReplayBuffer")
    A = buffer.action_dims[k]
    grads, critic, (y, workspace, own_stats) = _critic_update_state(critic_module, buffer, k, index, max_workgroups, ("sac",))
    sac_target(ActorParams.from_sac_module(actor_module), QCriticParams.from_module(critic_target_module, A), buffer, k, index,
               discount=discount, alpha=alpha, noise=noise, out=y)
    _, stats = twinq_grad(critic, buffer.obs[k], buffer.act[k], y, index, grads=grads, stats=own_stats if stats is None else stats,
                          workspace=workspace, max_workgroups=max_workgroups)
    return stats


def sac_target_ctde(actors, critic_target: QCriticParams, buffer_or_tensors, k: int = 0, index: Optional[torch.Tensor] = None, *,
                    discount: float = 0.99, alpha: Union[float, torch.Tensor] = 0.2, noise=None, noise_logp: Optional[torch.Tensor] = None,
                    action_next=None, logp_next: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, action_out=None,
                    logp_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SAC's target values for the centralized (CTDE) twin critic of two agents in one launch (qr_ctde_sac_target; sac.py:136-153), j the
    minibatch position, i = index[j], m = 0, 1:
        mean_m, ls_m = actors[m](obs_next_m[i]);  ls_m = clamp(ls_m, -20, 2);  a'_m = tanh(mean_m + exp(ls_m) * noise[m][j])
        logp_j = sum_f [ -e^2 / 2 - ls_k - log sqrt(2 pi) - log(1 - tanh(mean_k + exp(ls_k) e)^2 + 1e-6) ],  e = noise_logp[j]
        y[j] = rwd_k[i] + discount * (1 - done_k[i]) * (min(Q1, Q2)([obs_next_0[i] | obs_next_1[i] | a'_0 | a'_1]) - alpha * logp_j)
    The reference samples agent k a second time for the log-probability: noise_logp [B, A_k] is that draw; None: noise[k], one sample
    (the same tensor for both gives the same bits).  actors: the pair of `ActorParams.from_sac_module` — the LIVE actors — of the sizes
    (15,16,4) and (3,4,1), or None with action_next = (a'_0, a'_1) and logp_next [B] used as they are, for any widths whose sum the
    critic reads.  critic_target, buffer_or_tensors, noise, index, out: `td3.td3_target_ctde`'s; alpha: `sac_target`'s.  action_out: a
    pair of optional outputs [B, A_m]; logp_out [B]: optional."""
    what = "sac_target_ctde"

    def own(B, ad, dev, supplied):
        outs = ck.pair_of(what, "action_out", action_out, B, ad, dev)
        ck.tensor(what, "noise_logp", noise_logp, torch.float32, (B, ad[k]), dev, True)
        ck.flat(what, "logp_next", logp_next, torch.float32, B, dev, True)
        ck.flat(what, "logp_out", logp_out, torch.float32, B, dev, True)
        if supplied and logp_next is None:
            raise ValueError(f"{what}: without actors, logp_next [B] is required")
        a, alpha_dev = ck.alpha(what, alpha, dev)
        ck.nonneg(what, ("discount",), discount)
        return dict(eps_logp=noise_logp, logp_next=logp_next, alpha_dev=alpha_dev, action_out=outs, logp_out=logp_out, discount=discount, alpha=a,
                    agent=k)

    return _target_ctde(what, "qr_ctde_sac_target", _lib.ctde_sac_target_args, actors,
                        (_lib.ACTOR_TANH_SAMPLE, True, "the actors must be of MLP_Actor_SAC's form: the tanh-of-sample rule with a log_std head"),
                        critic_target, buffer_or_tensors, k, index, noise, action_next, out, own)


def sac_critic_loss_ctde(critic_module, critic_target_module, actor_modules, buffer: ReplayBuffer, k: int = 0, index: Optional[torch.Tensor] = None, *,
                         discount: float = 0.99, alpha: Union[float, torch.Tensor] = 0.2, noise=None, noise_logp: Optional[torch.Tensor] = None,
                         stats: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> torch.Tensor:
    """`sac_critic_loss` for the centralized (CTDE) critic of a two-agent `buffer`, for agent k's reward and done: `sac_target_ctde` on
    the two LIVE `actor_modules` and the target critic, then `td3.twinq_grad_ctde` on the live `critic_module` (MLP_Critic_CTDE:
    fc1 .. fc6 over [obs_0 | obs_1 | act_0 | act_1]); fills `critic_module.fc{1..6}.{weight,bias}.grad` in place.  noise: the pair of
    rsample draws, noise_logp: the draw of the reference's second sample of agent k (None: noise[k]).  Returns stats (stats[0] = the
    loss).  y, the workspace and stats are cached on the buffer under a key of their own: from the second call on with an unchanged B
    nothing is allocated.  The optimiser step stays the caller's."""
    if not isinstance(buffer, ReplayBuffer):
        raise ValueError("sac_critic_loss_ctde: buffer must be a ReplayBuffer")
    A = sum(buffer.action_dims)
    grads, critic, (y, workspace, own_stats) = _critic_update_state(critic_module, buffer, k, index, max_workgroups, ("sac_ctde",), action_dim=A)
    sac_target_ctde([ActorParams.from_sac_module(m) for m in actor_modules], QCriticParams.from_module(critic_target_module, A), buffer, k, index,
                    discount=discount, alpha=alpha, noise=noise, noise_logp=noise_logp, out=y)
    _, stats = twinq_grad_ctde(critic, buffer.obs, buffer.act, y, index, grads=grads, stats=own_stats if stats is None else stats,
                               workspace=workspace, max_workgroups=max_workgroups)
    return stats


def sac_actor_workspace_bytes(actor_dims, critic_hidden: int, batch: int, max_workgroups: int = 0) -> int:
    """Bytes of workspace one `sac_actor_grad` call needs (qr_sac_actor_workspace_bytes); actor_dims = (obs_dim, hidden, action_dim)."""
    return _lib.workspace_bytes("qr_sac_actor_workspace_bytes", *actor_dims, critic_hidden, batch, max_workgroups)


def sac_actor_grad(actor: ActorParams, critic: QCriticParams, obs: torch.Tensor, obs_next: Optional[torch.Tensor] = None,
                   index: Optional[torch.Tensor] = None, *, alpha: Union[float, torch.Tensor] = 0.2, lam_T: float = 0.4, lam_S: float = 0.3,
                   lam_M: float = 0.6, max_action: float = 1.0, eps: Optional[torch.Tensor] = None, eps_reg: Optional[torch.Tensor] = None,
                   eps_next: Optional[torch.Tensor] = None, eps_pert: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                   nominal: Optional[torch.Tensor] = None, alpha_grad: Optional[torch.Tensor] = None, target_entropy: Optional[float] = None,
                   grads: Optional[dict] = None, stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                   max_workgroups: int = 0):
    """SAC's actor loss and its gradients (qr_sac_actor_grad; sac.py:182-211 without the spectral-norm term, with
    algos/policy_regularization.py), c = clamp to +-max_action, i = index[j], sample = MLP_Actor_SAC.sample with the given draws:
        (a, logp) = sample(obs[i], eps[j]);   L0 = mean_j (alpha logp_j - min(Q1, Q2)(obs[i], a_j))
        r = c(sample(obs[i], eps_reg[j]).a);  rn = c(sample(obs_next[i], eps_next[j]).a);  rp = c(sample(obs[i] + noise, eps_pert[j]).a)
        loss = L0 + lam_T mse(r, rn) + lam_S mse(r, rp) + lam_M mse(r, nominal)
    — no autograd, no copies of the minibatch's rows.  actor: `ActorParams.from_sac_module(module)` in one of the three sizes of the
    rollout; critic: the twin critic, both networks are read.  obs, obs_next [rows, D] contiguous float32 (obs_next: needed when
    lam_T != 0); the four eps: float32 [B, A] standard-normal draws by minibatch position (rsample's), None: zeros; noise [D]: ONE row,
    needed when lam_S != 0; nominal [A]: needed when lam_M != 0; index int64 [B], None: all rows in order.  alpha: a Python float, or a
    float32 tensor of one element on the device that the kernels read (no host synchronisation); it is a constant of this loss.
    alpha_grad: an optional float32 tensor of one element that receives d alpha_loss / d log_alpha = -(target_entropy + mean_j logp_j);
    target_entropy: None is -A.
    Returns (grads, stats): grads = {name: float32 tensor} for fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, log_std_w, log_std_b —
    `grads` given: overwritten in place — and stats float32 [6] = loss, the mean of min(Q1, Q2), the mean logp of the loss pass, the
    weighted sum of the three smoothness terms, the share of the loss pass's raw log_std components outside [-20, 2], the share of
    rows that took Q2."""
    what = "sac_actor_grad"
    dev = critic.device
    D, A, H = critic.dims
    shapes = ck.actor(what, actor, PPO_ACTOR_DIMS, D, A, dev, _lib.ACTOR_TANH_SAMPLE, True,
                      "the actor must be of MLP_Actor_SAC's form: the tanh-of-sample rule with a log_std head")
    ck.nonneg(what, ck.LAMS, lam_T, lam_S, lam_M, max_action)
    a, alpha_dev, te = _entropy_terms(what, alpha, target_entropy, alpha_grad, A, dev)
    rows = ck.rows(what, "obs", obs, D, dev)
    if lam_T != 0 and ck.rows(what, "obs_next", obs_next, D, dev) != rows:
        raise ValueError(f"{what}: obs_next must have obs's {rows} rows")
    if (lam_S != 0 and noise is None) or (lam_M != 0 and nominal is None):
        raise ValueError(f"{what}: noise [{D}] is required when lam_S != 0, nominal [{A}] when lam_M != 0")
    ck.flat(what, "noise", noise, torch.float32, D, dev, True)
    ck.flat(what, "nominal", nominal, torch.float32, A, dev, True)
    B = ck.index(what, index, dev, rows)
    ck.named(what, "{}", dict(eps=eps, eps_reg=eps_reg, eps_next=eps_next, eps_pert=eps_pert), dict.fromkeys(_EPS, (B, A)), dev, optional=True)
    grads, stats, workspace = _grad_outputs(what, shapes, dev, B, grads, stats, workspace,
                                            lambda: sac_actor_workspace_bytes(actor.dims, H, B, max_workgroups), size_given=False,
                                            n_stats=_lib.SAC_ACTOR_STATS)
    if workspace is None:
        if alpha_grad is not None:
            alpha_grad.zero_()
        return grads, stats
    b = _lib.transitions(obs=obs, obs_next=obs_next if lam_T != 0 else None, index=index, batch=B, rows=rows)
    g = _lib.sac_actor_grad_args(grads, stats, workspace, eps=eps, eps_reg=eps_reg, eps_next=eps_next, eps_pert=eps_pert,
                                 noise=noise if lam_S != 0 else None, nominal=nominal if lam_M != 0 else None, alpha_dev=alpha_dev,
                                 alpha_grad=alpha_grad, alpha=a, target_entropy=te, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M,
                                 max_action=max_action, max_workgroups=max_workgroups)
    _lib.launch(dev, "qr_sac_actor_grad", actor.as_c(), critic.as_c(), b, g)
    return grads, stats


def sac_actor_loss(actor_module, critic_module, buffer: ReplayBuffer, k: int = 0, index: Optional[torch.Tensor] = None, *,
                   log_alpha: Optional[torch.Tensor] = None, target_entropy: Optional[float] = None, alpha: Union[float, torch.Tensor] = 0.2,
                   lam_T: float = 0.4, lam_S: float = 0.3, lam_M: float = 0.6, max_action: float = 1.0, eps: Optional[torch.Tensor] = None,
                   eps_reg: Optional[torch.Tensor] = None, eps_next: Optional[torch.Tensor] = None, eps_pert: Optional[torch.Tensor] = None,
                   noise: Optional[torch.Tensor] = None, nominal: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                   max_workgroups: int = 0) -> torch.Tensor:
    """The actor update of SAC.train, as the reference writes it, without autograd: `sac_actor_grad` on the live `actor_module`
    (attributes fc1, fc2, mean_linear, log_std_linear) and `critic_module` (fc1 .. fc6) for agent k of `buffer`; writes the gradients
    into the eight `.grad` tensors of the actor in place, as `loss.backward()` after `zero_grad()` leaves them.  log_alpha: the
    one-element parameter of automatic entropy tuning; given, its `.grad` receives d alpha_loss / d log_alpha =
    -(target_entropy + mean logp) (target_entropy: None is -A).  alpha: a float, or the device tensor exp(log_alpha) — it is read, not
    formed here.  The four eps: the [B, A] draws of the four samples (rsample's), None: zeros; noise: policy_regularization's ONE [D]
    row; nominal: its [A] hover action.  Returns stats [6] (stats[0] = the loss).  From the second call on with an unchanged B nothing
    is allocated: the workspace and stats are cached on the buffer.
    The optimiser steps stay the caller's: the actor's eight tensors are one `optim.DeviceAdamW` group, log_alpha is a group of one,
    and `torch.exp(log_alpha, out=alpha)` feeds the next `sac_target` and `sac_actor_loss`."""
    if not isinstance(buffer, ReplayBuffer):
        raise ValueError("sac_actor_loss: buffer must be a ReplayBuffer")
    grads = _actor_grads("sac_actor_loss", actor_module, log_alpha)
    actor = ActorParams.from_sac_module(actor_module)
    critic = QCriticParams.from_module(critic_module, buffer.action_dims[k])
    workspace, own_stats = buffer._actor_scratch("sac_actor", k, index, max_workgroups, critic.device,
                                                 lambda B: sac_actor_workspace_bytes(actor.dims, critic.dims[2], B, max_workgroups),
                                                 _lib.SAC_ACTOR_STATS)
    _, stats = sac_actor_grad(actor, critic, buffer.obs[k], buffer.obs_next[k], index, alpha=alpha, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M,
                              max_action=max_action, eps=eps, eps_reg=eps_reg, eps_next=eps_next, eps_pert=eps_pert, noise=noise,
                              nominal=nominal, alpha_grad=None if log_alpha is None else log_alpha.grad, target_entropy=target_entropy,
                              grads=grads, stats=own_stats if stats is None else stats, workspace=workspace, max_workgroups=max_workgroups)
    return stats


def sac_actor_workspace_bytes_ctde(k: int, critic_hidden: int, batch: int, max_workgroups: int = 0) -> int:
    """Bytes of workspace one `sac_actor_grad_ctde` call needs for agent k (qr_ctde_sac_actor_workspace_bytes): `sac_actor_workspace_bytes`'
    figure for td3.CTDE_ACTOR_DIMS[k]."""
    return _lib.workspace_bytes("qr_ctde_sac_actor_workspace_bytes", k, critic_hidden, batch, max_workgroups)


def sac_actor_grad_ctde(actors, critic: QCriticParams, obs, obs_next=None, index: Optional[torch.Tensor] = None, *, k: int = 0,
                        action_other: Optional[torch.Tensor] = None, alpha: Union[float, torch.Tensor] = 0.2, lam_T: float = 0.4,
                        lam_S: float = 0.3, lam_M: float = 0.6, max_action: float = 1.0, eps: Optional[torch.Tensor] = None,
                        eps_logp: Optional[torch.Tensor] = None, eps_other: Optional[torch.Tensor] = None, eps_reg: Optional[torch.Tensor] = None,
                        eps_next: Optional[torch.Tensor] = None, eps_pert: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                        nominal: Optional[torch.Tensor] = None, alpha_grad: Optional[torch.Tensor] = None, target_entropy: Optional[float] = None,
                        grads: Optional[dict] = None, stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                        max_workgroups: int = 0):
    """Agent k's SAC actor loss under the centralized (CTDE) twin critic of two agents and its gradients (qr_ctde_sac_actor_grad;
    sac.py:175-203 without the spectral-norm term, with algos/policy_regularization.py), i = index[j], sample and c as `sac_actor_grad`'s:
        a_k = sample(pi_k, obs[k][i], eps[j]).a;   a_o = sample(pi_o, obs[o][i], eps_other[j]).a      (o = 1 - k; no clamp)
        logp_j = sample(pi_k, obs[k][i], eps_logp[j]).logp                                            (a SECOND sample of agent k)
        L0 = mean_j (alpha logp_j - min(Q1, Q2)([obs[0][i] | obs[1][i] | a_0 | a_1]))
        loss_k = L0 + lam_T mse(r, rn) + lam_S mse(r, rp) + lam_M mse(r, nominal)                     (r, rn, rp: agent k's, `sac_actor_grad`'s)
    — no autograd, nothing concatenated.  eps_logp None: ONE sample, logp and a_k both from eps (eps_logp given as zeros is not that
    form: it is a second sample at the mean).  actors: the pair of `ActorParams.from_sac_module` of the sizes td3.CTDE_ACTOR_DIMS; the
    other agent's runs forward only inside the kernel and gets NO gradient (the reference leaves one in its .grad, which that agent
    zeroes before reading).  Or actors[1 - k] None with action_other float32 [B, A_other] by minibatch position, used as it is: then
    eps_other is not read and the other agent's widths are free as long as all four add up to the critic's.  obs, obs_next: pairs of
    contiguous float32 [rows, D_m]; obs_next[k] is needed when lam_T != 0, obs_next[1 - k] never.  eps, eps_logp, eps_reg, eps_next,
    eps_pert [B, A_k], eps_other [B, A_other]: float32 draws by minibatch position, None: zeros.  noise [D_k], nominal [A_k], alpha,
    alpha_grad, target_entropy (None: -A_k), index, grads, stats, workspace, max_workgroups and the return value (grads of agent k's
    eight tensors, stats [6]): `sac_actor_grad`'s; stats[2] and alpha_grad come from the sample that carries logp."""
    what = "sac_actor_grad_ctde"
    dev = critic.device
    form = (_lib.ACTOR_TANH_SAMPLE, True, "the actors must be of MLP_Actor_SAC's form: the tanh-of-sample rule with a log_std head")
    shapes, B, rows, od, ad, nxt = _ctde_actor_launch(what, actors, critic, obs, obs_next, index, k, action_other, lam_T, lam_S, lam_M, max_action,
                                                      noise, nominal, form)
    a, alpha_dev, te = _entropy_terms(what, alpha, target_entropy, alpha_grad, ad[k], dev)
    own, other = (B, ad[k]), (B, ad[1 - k])
    ck.named(what, "{}", dict(eps=eps, eps_logp=eps_logp, eps_other=eps_other, eps_reg=eps_reg, eps_next=eps_next, eps_pert=eps_pert),
             dict(eps=own, eps_logp=own, eps_other=other, eps_reg=own, eps_next=own, eps_pert=own), dev, optional=True)
    grads, stats, workspace = _grad_outputs(what, shapes, dev, B, grads, stats, workspace,
                                            lambda: sac_actor_workspace_bytes_ctde(k, critic.dims[2], B, max_workgroups), size_given=False,
                                            n_stats=_lib.SAC_ACTOR_STATS)
    if workspace is None:
        if alpha_grad is not None:
            alpha_grad.zero_()
        return grads, stats
    b = _lib.ctde_transitions(obs=obs, obs_next=(nxt, None) if k == 0 else (None, nxt), index=index, batch=B, rows=rows, obs_dims=od, action_dims=ad)
    g = _lib.ctde_sac_actor_grad_args(grads, stats, workspace, agent=k, action_other=action_other, eps_logp=eps_logp,
                                      eps_other=eps_other if action_other is None else None, eps=eps, eps_reg=eps_reg, eps_next=eps_next,
                                      eps_pert=eps_pert, noise=noise if lam_S != 0 else None, nominal=nominal if lam_M != 0 else None,
                                      alpha_dev=alpha_dev, alpha_grad=alpha_grad, alpha=a, target_entropy=te, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M,
                                      max_action=max_action, max_workgroups=max_workgroups)
    _lib.launch(dev, "qr_ctde_sac_actor_grad", *_ctde_actors_c(actors, log_std=True), critic.as_c(), b, g)
    return grads, stats


def sac_actor_loss_ctde(actor_modules, critic_module, buffer: ReplayBuffer, k: int = 0, index: Optional[torch.Tensor] = None, *,
                        log_alpha: Optional[torch.Tensor] = None, target_entropy: Optional[float] = None, alpha: Union[float, torch.Tensor] = 0.2,
                        lam_T: float = 0.4, lam_S: float = 0.3, lam_M: float = 0.6, max_action: float = 1.0, eps: Optional[torch.Tensor] = None,
                        eps_logp: Optional[torch.Tensor] = None, eps_other: Optional[torch.Tensor] = None, eps_reg: Optional[torch.Tensor] = None,
                        eps_next: Optional[torch.Tensor] = None, eps_pert: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                        nominal: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> torch.Tensor:
    """`sac_actor_loss` for agent k of a two-agent `buffer` under the centralized (CTDE) twin critic: `sac_actor_grad_ctde` on the two live
    actors (attributes fc1, fc2, mean_linear, log_std_linear) and `critic_module` (MLP_Critic_CTDE, fc1 .. fc6); fills agent k's eight
    `.grad` tensors in place, as `loss.backward()` after `zero_grad()` leaves them, and `log_alpha.grad` when log_alpha is given.  Of
    `actor_modules[1 - k]` only the eight tensors' data are read: no attribute of it is set, neither its tensors nor its .grad are
    touched.  The draws, noise, nominal: `sac_actor_grad_ctde`'s.  Returns stats [6] (stats[0] = the loss).  The workspace and stats are
    cached on the buffer under a key of their own: from the second call on with an unchanged B nothing is allocated.  The optimiser
    steps stay the caller's."""
    what = "sac_actor_loss_ctde"
    if not isinstance(buffer, ReplayBuffer) or buffer.n_agents != 2:
        raise ValueError(f"{what}: buffer must be a two-agent ReplayBuffer")
    if k not in (0, 1):
        raise ValueError(f"{what}: k must be 0 or 1 (two agents), got {k}")
    actor_modules = tuple(actor_modules)
    if len(actor_modules) != 2:
        raise ValueError(f"{what}: actor_modules must be the pair of both agents' actors")
    grads = _actor_grads(what, actor_modules[k], log_alpha)
    actors = [ActorParams.from_sac_module(a) for a in actor_modules]
    critic = QCriticParams.from_module(critic_module, sum(buffer.action_dims))
    workspace, own_stats = buffer._actor_scratch("sac_actor_ctde", k, index, max_workgroups, critic.device,
                                                 lambda B: sac_actor_workspace_bytes_ctde(k, critic.dims[2], B, max_workgroups),
                                                 _lib.SAC_ACTOR_STATS)
    _, stats = sac_actor_grad_ctde(actors, critic, buffer.obs, buffer.obs_next, index, k=k, alpha=alpha, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M,
                                   max_action=max_action, eps=eps, eps_logp=eps_logp, eps_other=eps_other, eps_reg=eps_reg, eps_next=eps_next,
                                   eps_pert=eps_pert, noise=noise, nominal=nominal, alpha_grad=None if log_alpha is None else log_alpha.grad,
                                   target_entropy=target_entropy, grads=grads, stats=own_stats if stats is None else stats, workspace=workspace,
                                   max_workgroups=max_workgroups)
    return stats
