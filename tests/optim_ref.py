"""The float64 restatement of one optimiser step as include/quadrotor_hip.h states it for qr_adamw_step: clip_grad_norm_, AdamW
(amsgrad = False, maximize = False) and CosineAnnealingWarmRestarts stepped after the optimiser.  NumPy only; the yardstick it is
checked against is torch's own three pieces on double tensors (tests/test_optim_host.py)."""
import math

import numpy as np


def schedule(t_prev: int, lr: float, t0: int, eta_min: float) -> float:
    """The rate of the optimiser step that follows t_prev steps: eta(t_prev) of CosineAnnealingWarmRestarts(T_0 = t0, eta_min)."""
    if t0 == 0:
        return lr
    return eta_min + (lr - eta_min) * (1.0 + math.cos(math.pi * (t_prev % t0) / t0)) / 2.0


def adamw_step_f64(p, g, m, v, t_prev, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=-1.0, t0=0, eta_min=0.0):
    """One step for one group.  p, g, m, v: lists of arrays (any shapes, one per tensor; m, v in the tensors' shapes); t_prev: steps
    taken so far.  Returns (p, m, v, info) as new float64 arrays, info = dict(total_norm, clip_coef, lr_t, t)."""
    p, g, m, v = ([np.asarray(a, dtype=np.float64) for a in x] for x in (p, g, m, v))
    t = int(t_prev) + 1
    total_norm = math.sqrt(sum(float((a * a).sum()) for a in g))
    lr_t = schedule(t - 1, lr, t0, eta_min)
    clip = 1.0
    if max_norm >= 0:
        clip = max_norm / (total_norm + 1e-6)
        clip = 1.0 if clip > 1.0 else clip            # (NaN stays NaN)
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    po, mo, vo = [], [], []
    with np.errstate(invalid="ignore"):
        for pk, gk, mk, vk in zip(p, g, m, v):
            gk = clip * gk
            pk = pk * (1.0 - lr_t * weight_decay)
            mk = b1 * mk + (1.0 - b1) * gk
            vk = b2 * vk + (1.0 - b2) * gk * gk
            pk = pk - (lr_t / bc1) * mk / (np.sqrt(vk) / math.sqrt(bc2) + eps)
            po.append(pk); mo.append(mk); vo.append(vk)
    return po, mo, vo, dict(total_norm=total_norm, clip_coef=clip, lr_t=lr_t, t=t)


def run_f64(p, grad_sets, **hyper):
    """k steps from zero moments and step 0.  Returns (p, m, v, [info per step])."""
    p = [np.asarray(a, dtype=np.float64) for a in p]
    m, v, infos = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p], []
    for t_prev, g in enumerate(grad_sets):
        p, m, v, info = adamw_step_f64(p, g, m, v, t_prev, **hyper)
        infos.append(info)
    return p, m, v, infos


def run_torch(p, grad_sets, dtype, device="cpu", *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=-1.0, t0=0, eta_min=0.0,
              **adamw_kw):
    """The same k steps with torch's own clip_grad_norm_, AdamW and CosineAnnealingWarmRestarts on tensors of `dtype`, in the
    reference's call order (ppo.py:185-190).  Returns (p, m, v, [total_norm per step]) as float64 NumPy."""
    import torch
    params = [torch.nn.Parameter(torch.as_tensor(np.asarray(a)).to(dtype).to(device).clone()) for a in p]
    opt = torch.optim.AdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **adamw_kw)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=t0, eta_min=eta_min) if t0 > 0 else None
    norms = []
    for g in grad_sets:
        for q, gk in zip(params, g):
            q.grad = torch.as_tensor(np.asarray(gk)).to(dtype).to(device).reshape(q.shape).clone()
        if max_norm >= 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
        if sched is not None:
            sched.step()
    out = lambda ts: [t.detach().double().cpu().numpy() for t in ts]
    return out(params), out([opt.state[q]["exp_avg"] for q in params]), out([opt.state[q]["exp_avg_sq"] for q in params]), norms
