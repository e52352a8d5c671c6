"""What the tests of qr_adamw_polyak_step / PolyakAdamW and of Td3Updater / SacUpdater compare against.

The optimiser: optim_ref's float64 step with, after it, the soft-update line target = tau * p + (1 - tau) * target on the NEW
parameters and exp_out = exp(the new parameter) for a one-entry group (include/quadrotor_hip.h, qr_adamw_polyak_step).

The iterations: one training iteration of TD3.train (algos/td3/td3.py:111-211) and of SAC.train (algos/sac/sac.py:123-221) for ONE
agent with its own critic, restated with torch autograd on tensors of a chosen dtype — float64 is the yardstick, float32 gives the
size of torch's own rounding error for the bar.  The losses are written out here from the reference's lines; the optimiser steps
are torch's own clip_grad_norm_ over ALL of a network's tensors (the twin critic's twelve under one coefficient), AdamW and
CosineAnnealingWarmRestarts, in the reference's call order.  The draws are inputs, by the names the updaters keep them under."""
import math

import numpy as np
import torch

from optim_ref import adamw_step_f64

LOG_SIG_MAX, LOG_SIG_MIN, EPSILON = 2.0, -20.0, 1e-6
T0, ETA_MIN = 1_000_000, 1e-5


def polyak_f64(p, target, tau):
    return [tau * np.asarray(a, dtype=np.float64) + (1.0 - tau) * np.asarray(t, dtype=np.float64) for a, t in zip(p, target)]


def polyak_step_f64(p, g, m, v, t_prev, targets=None, *, tau=0.005, exp_out=False, **hyper):
    """One qr_adamw_polyak_step group in float64.  targets: None, or per tensor an array or None.  Returns (p, m, v, targets, exp_out
    value or None, info)."""
    p, m, v, info = adamw_step_f64(p, g, m, v, t_prev, **hyper)
    out = None
    if targets is not None:
        out = [None if t is None else tau * a + (1.0 - tau) * np.asarray(t, dtype=np.float64) for a, t in zip(p, targets)]
    e = None
    if exp_out:
        assert sum(a.size for a in p) == 1
        e = math.exp(float(p[0].reshape(-1)[0]))
    return p, m, v, out, e, info


def run_polyak_f64(p, grad_sets, targets, polyak_steps=None, *, tau=0.005, **hyper):
    """k steps from zero moments; the soft update follows step j when polyak_steps is None or holds j.  Returns (p, m, v, targets, infos)."""
    p = [np.asarray(a, dtype=np.float64) for a in p]
    tg = [None if t is None else np.asarray(t, dtype=np.float64) for t in targets]
    m, v, infos = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p], []
    for j, g in enumerate(grad_sets):
        on = polyak_steps is None or j in polyak_steps
        p, m, v, new, _, info = polyak_step_f64(p, g, m, v, j, tg if on else None, tau=tau, **hyper)
        tg = new if on else tg
        infos.append(info)
    return p, m, v, tg, infos


# -- the networks, as lists of tensors in torch.nn.Linear layout --------------------------------------------------------------------------
def _mlp(ws, x):
    """Linear, relu, Linear, relu, Linear over ws = [w1, b1, w2, b2, w3, b3]."""
    x = torch.relu(x @ ws[0].T + ws[1])
    x = torch.relu(x @ ws[2].T + ws[3])
    return x @ ws[4].T + ws[5]


def td3_actor(ws, obs):
    return torch.tanh(_mlp(ws, obs))


def twin_q(ws, obs, act):
    sa = torch.cat([obs, act], dim=1)
    return _mlp(ws[:6], sa), _mlp(ws[6:], sa)


def sac_sample(ws, obs, eps):
    """MLP_Actor_SAC.sample with rsample's draw given: (action, log_prob [B, 1])."""
    h = torch.relu(torch.relu(obs @ ws[0].T + ws[1]) @ ws[2].T + ws[3])
    mean, log_std = h @ ws[4].T + ws[5], torch.clamp(h @ ws[6].T + ws[7], LOG_SIG_MIN, LOG_SIG_MAX)
    std = log_std.exp()
    x_t = mean + std * eps
    action = torch.tanh(x_t)
    log_prob = -((x_t - mean) ** 2) / (2 * std ** 2) - log_std - math.log(math.sqrt(2 * math.pi))
    log_prob = log_prob - torch.log((1 - action.pow(2)) + EPSILON)
    return action, log_prob.sum(1, keepdim=True)


def _mse(a, b):
    return ((a - b) ** 2).mean()


def _regularized(loss, act, act_next, act_pert, nominal, hp):
    """algos/policy_regularization.py: temporal, spatial and magnitude terms on the clamped actions."""
    c = lambda a: a.clamp(-hp["max_action"], hp["max_action"])
    act = c(act)
    return loss + hp["lam_T"] * _mse(act, c(act_next)) + hp["lam_S"] * _mse(act, c(act_pert)) + hp["lam_M"] * _mse(act, nominal.expand_as(act))


class Net:
    """A network's tensors as Parameters of one dtype with torch's AdamW, the scheduler and the clip over ALL of them."""

    def __init__(self, arrays, dtype, lr, max_norm, schedule=True):
        self.ws = [torch.nn.Parameter(torch.as_tensor(np.asarray(a)).to(dtype).clone()) for a in arrays]
        # betas, eps and weight_decay as the C-ABI holds them, float32 (DeviceAdamW's documented deviation: beta2 = 0.999 is
        # 0.99900001287...), so that the kernel, this restatement and its float32 run compute with the same values
        f32 = lambda x: float(np.float32(x))
        self.opt = torch.optim.AdamW(self.ws, lr=lr, betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(1e-2))
        self.sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(self.opt, T_0=T0, eta_min=ETA_MIN) if schedule else None
        self.max_norm = max_norm

    def step(self, loss):
        """zero_grad, backward, clip_grad_norm_, step, scheduler.  Returns the gradients' norms: (joint, [per tensor])."""
        self.opt.zero_grad()
        loss.backward()
        per = [float(w.grad.double().pow(2).sum()) for w in self.ws]
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.ws, self.max_norm)
        self.opt.step()
        if self.sched is not None:
            self.sched.step()
        return math.sqrt(sum(per)), per

    def arrays(self):
        return [w.detach().double().numpy() for w in self.ws]

    def moments(self):
        return ([self.opt.state[w]["exp_avg"].double().numpy() for w in self.ws], [self.opt.state[w]["exp_avg_sq"].double().numpy() for w in self.ws])


def _soft(net_ws, target_ws, tau):
    with torch.no_grad():
        for p, t in zip(net_ws, target_ws):
            t.copy_(tau * p + (1 - tau) * t)


def _batch(batch, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in batch.items()}


def td3_iteration(dtype, actor, critic, actor_t, critic_t, batch, noise, nominal, hp, update=True):
    """One TD3.train call from fresh optimisers.  actor / critic / targets: lists of arrays; batch: obs, act, rwd, obs_next, done of the
    minibatch rows; noise: {"smooth" [B, A], "reg" [D]}.  Returns a dict of float64 arrays and the critic gradient's norms."""
    b, nz = _batch(batch, dtype), _batch(noise, dtype)
    nom = torch.as_tensor(np.asarray(nominal)).to(dtype)
    A, C = Net(actor, dtype, hp["lr_a"], hp["grad_max_norm"]), Net(critic, dtype, hp["lr_c"], hp["grad_max_norm"])
    At = [torch.as_tensor(np.asarray(a)).to(dtype).clone() for a in actor_t]
    Ct = [torch.as_tensor(np.asarray(a)).to(dtype).clone() for a in critic_t]
    rwd, done = b["rwd"].reshape(-1, 1), b["done"].reshape(-1, 1)
    with torch.no_grad():
        a_next = td3_actor(At, b["obs_next"])
        smooth = (nz["smooth"] * hp["target_noise"]).clamp(-hp["noise_clip"], hp["noise_clip"])
        a_next = (a_next + smooth).clamp(-hp["max_action"], hp["max_action"])
        y = rwd + hp["discount"] * (1 - done) * torch.min(*twin_q(Ct, b["obs_next"], a_next))
    q1, q2 = twin_q(C.ws, b["obs"], b["act"])
    joint, per = C.step(_mse(q1, y) + _mse(q2, y))
    if update:
        act = td3_actor(A.ws, b["obs"]).clamp(-hp["max_action"], hp["max_action"])
        loss = -twin_q(C.ws, b["obs"], act)[0].mean()
        loss = _regularized(loss, td3_actor(A.ws, b["obs"]), td3_actor(A.ws, b["obs_next"]), td3_actor(A.ws, b["obs"] + nz["reg"].reshape(1, -1)), nom, hp)
        A.step(loss)
        _soft(C.ws, Ct, hp["tau"])
        _soft(A.ws, At, hp["tau"])
    return dict(actor=A.arrays(), critic=C.arrays(), actor_t=[t.double().numpy() for t in At], critic_t=[t.double().numpy() for t in Ct],
                critic_m=C.moments(), actor_m=A.moments() if update else None, joint_norm=joint,
                half_norms=(math.sqrt(sum(per[:6])), math.sqrt(sum(per[6:]))))


def sac_iteration(dtype, actor, critic, critic_t, batch, noise, nominal, hp, alpha, log_alpha, update=True):
    """One SAC.train call from fresh optimisers with automatic entropy tuning.  noise: {"next", "eps", "eps_reg", "eps_next", "eps_pert"
    [B, A], "reg" [D]}; alpha: the temperature in use; log_alpha: the parameter's value.  Returns as td3_iteration, with log_alpha and
    alpha after the step."""
    b, nz = _batch(batch, dtype), _batch(noise, dtype)
    nom = torch.as_tensor(np.asarray(nominal)).to(dtype)
    A, C = Net(actor, dtype, hp["lr_a"], hp["grad_max_norm"]), Net(critic, dtype, hp["lr_c"], hp["grad_max_norm"])
    L = Net([np.asarray([log_alpha])], dtype, hp["lr_a"], None, schedule=False)
    Ct = [torch.as_tensor(np.asarray(a)).to(dtype).clone() for a in critic_t]
    rwd, done = b["rwd"].reshape(-1, 1), b["done"].reshape(-1, 1)
    n_act = b["act"].shape[1]
    target_entropy = -float(n_act) if hp.get("target_entropy") is None else hp["target_entropy"]
    with torch.no_grad():
        a_next, logp_next = sac_sample(A.ws, b["obs_next"], nz["next"])
        y = rwd + hp["discount"] * (1 - done) * (torch.min(*twin_q(Ct, b["obs_next"], a_next)) - alpha * logp_next)
    q1, q2 = twin_q(C.ws, b["obs"], b["act"])
    joint, per = C.step(_mse(q1, y) + _mse(q2, y))
    act, logp = sac_sample(A.ws, b["obs"], nz["eps"])
    loss = -(torch.min(*twin_q(C.ws, b["obs"], act)) - alpha * logp).mean()
    loss = _regularized(loss, sac_sample(A.ws, b["obs"], nz["eps_reg"])[0], sac_sample(A.ws, b["obs_next"], nz["eps_next"])[0],
                        sac_sample(A.ws, b["obs"] + nz["reg"].reshape(1, -1), nz["eps_pert"])[0], nom, hp)
    A.step(loss)
    L.step(-(L.ws[0] * (target_entropy + logp).detach()).mean())
    if update:
        _soft(C.ws, Ct, hp["tau"])
    la = float(L.ws[0].detach().double())
    return dict(actor=A.arrays(), critic=C.arrays(), critic_t=[t.double().numpy() for t in Ct], critic_m=C.moments(), actor_m=A.moments(),
                log_alpha=la, alpha=math.exp(la), joint_norm=joint, half_norms=(math.sqrt(sum(per[:6])), math.sqrt(sum(per[6:]))))
