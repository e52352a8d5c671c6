#!/usr/bin/env python3
"""One epoch of a PPO update on one horizon — shuffle, then per minibatch the actor's and the critic's loss and gradients and both
optimiser steps — three ways on the same build, storage and initial weights:

  (a) the loop as it had to be written before `DeviceAdamW`: `actor_loss` + `critic_loss` (the gradient launches), then per network
      torch's `clip_grad_norm_`, `AdamW.step()` and `CosineAnnealingWarmRestarts.step()`; with torch's default AdamW and, where this
      torch accepts them on the device, with foreach=True and fused=True;
  (b) `PpoUpdater.update` with K_epochs = 1 (the same gradient launches, one `qr_adamw_step` launch per minibatch for both networks);
  (c) one optimiser step of both networks alone: `DeviceAdamW.step_all` against torch's three calls per network (default AdamW);
  and the gradient launches of an epoch alone, for the share of (b) that is still theirs.

    python tools/ppo_update_bench.py [--envs 65536] [--horizon 32] [--minibatches 32] [--reps 20]

Coupled (actor 23 -> 16 -> 16 -> 4, critic 23 -> 62 -> 62 -> 1), the reference's hyperparameters.  HIP events around each path with a
synchronise behind it, warm-up, median / min / max of --reps.  Prints ONE JSON line."""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch.optim.lr_scheduler import CosineAnnealingWarmRestarts  # noqa: E402

from gym_rotor_amd import (ActorParams, CriticParams, DeviceAdamW, PpoUpdater, QuadVecEnv, RolloutStorage, actor_loss, critic_loss,  # noqa: E402
                           minibatch_slices)

p = argparse.ArgumentParser()
p.add_argument("--envs", type=int, default=65536)
p.add_argument("--horizon", type=int, default=32)
p.add_argument("--minibatches", type=int, default=32)
p.add_argument("--reps", type=int, default=20)
p.add_argument("--warmup", type=int, default=3)
a = p.parse_args()
dev = torch.device("cuda", 0)
MAX_NORM, T0, ETA_MIN, LR_A, LR_C, L2 = 100.0, 1_000_000, 1e-5, 3e-4, 2e-4, 1e-4
CO = dict(clip=0.2, lam_T=0.4, lam_S=0.3, lam_M=0.6, max_action=1.0)
ENTROPY = 1e-2 * 0.99


class Actor(torch.nn.Module):  # the shape of the reference's MLP_Actor_PPO (attributes fc1, fc2, mean_linear, log_std)
    def __init__(self, D=23, H=16, A=4):
        super().__init__()
        self.fc1, self.fc2, self.mean_linear = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, A)
        self.log_std = torch.nn.Parameter(torch.ones(1, A) * -0.5)


class Critic(torch.nn.Module):  # the shape of the reference's MLP_Critic (attributes fc1, fc2, fc3)
    def __init__(self, D=23, H=62):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, 1)


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def main():
    N, T = a.envs, a.horizon
    torch.manual_seed(0)
    env = QuadVecEnv("coupled", N, device=dev, auto_reset=True, seed=0)
    env.reset("train")
    env.get_norm_error_state()
    st = RolloutStorage(env, T)
    actor0, critic0 = Actor().to(dev), Critic().to(dev)
    for _ in range(3):   # (episodes of every age, not one horizon after a common reset)
        st.collect(env, [ActorParams.from_module(actor0)])
    nv = st.compute_values([CriticParams.from_module(critic0)])
    adv, _, stats = st.compute_gae(0.99, 0.9, next_value=nv)
    adv = RolloutStorage.normalize(adv, stats)
    noise, nominal = torch.randn(23, device=dev) * 0.05, RolloutStorage.nominal_action(env, 0)
    rows = T * N
    mb = (rows + a.minibatches - 1) // a.minibatches
    slices = minibatch_slices(rows, mb)
    a_stats, c_stats = torch.zeros(4, device=dev), torch.zeros(4, device=dev)

    def gradients(actor, critic, perm, sl):
        actor_loss(actor, st, 0, adv, perm[sl], entropy_coef=ENTROPY, noise=noise, nominal=nominal, stats=a_stats, **CO)
        critic_loss(critic, st, 0, perm[sl], l2_reg=L2, stats=c_stats)

    def torch_optims(actor, critic, **kw):
        out = []
        for m, lr in ((actor, LR_A), (critic, LR_C)):
            opt = torch.optim.AdamW(m.parameters(), lr=lr, **kw)
            out.append((list(m.parameters()), opt, CosineAnnealingWarmRestarts(opt, T_0=T0, eta_min=ETA_MIN)))
        return out

    def torch_step(optims):
        for params, opt, sched in optims:
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
            sched.step()

    result = {"workload": "one epoch of a PPO update, Coupled: shuffle + per minibatch actor and critic gradients + both optimiser steps",
              "envs": N, "horizon": T, "minibatches": len(slices), "rows_per_minibatch": mb, "reps": a.reps}

    # the gradient launches of an epoch alone
    actor, critic = copy.deepcopy(actor0), copy.deepcopy(critic0)

    def grads_only():
        perm = torch.randperm(rows, device=dev)
        for sl in slices:
            gradients(actor, critic, perm, sl)

    result["gradient_launches_epoch"] = timed(grads_only)

    # (a) torch's optimiser path
    result["a_torch_epoch"] = {}
    for label, kw in (("default", {}), ("foreach", dict(foreach=True)), ("fused", dict(fused=True))):
        actor, critic = copy.deepcopy(actor0), copy.deepcopy(critic0)
        try:
            optims = torch_optims(actor, critic, **kw)
            gradients(actor, critic, torch.arange(rows, device=dev), slices[0])
            torch_step(optims)
            torch.cuda.synchronize()
        except Exception as e:   # this torch does not take the flag on this device
            result["a_torch_epoch"][label] = {"unavailable": f"{type(e).__name__}: {e}"[:200]}
            continue

        def torch_epoch():
            perm = torch.randperm(rows, device=dev)
            for sl in slices:
                gradients(actor, critic, perm, sl)
                torch_step(optims)

        result["a_torch_epoch"][label] = timed(torch_epoch)

    # (b) PpoUpdater
    actor, critic = copy.deepcopy(actor0), copy.deepcopy(critic0)
    hyper = dict(max_norm=MAX_NORM, t0=T0, eta_min=ETA_MIN)
    oa, oc = DeviceAdamW(actor.parameters(), lr=LR_A, **hyper), DeviceAdamW(critic.parameters(), lr=LR_C, **hyper)
    up = PpoUpdater([actor], [critic], [oa], [oc], K_epochs=1, actor_batch_size=mb, critic_batch_size=mb, entropy_coef=ENTROPY,
                    entropy_coef_decay=1.0, l2_reg=L2, noise=[noise], nominal=[nominal], **CO)
    result["b_updater_epoch"] = timed(lambda: up.update(st, adv))

    # (c) one optimiser step of both networks alone, from the gradients of one minibatch
    n_steps = len(slices)
    actor, critic = copy.deepcopy(actor0), copy.deepcopy(critic0)
    gradients(actor, critic, torch.arange(rows, device=dev), slices[0])
    oa, oc = DeviceAdamW(actor.parameters(), lr=LR_A, **hyper), DeviceAdamW(critic.parameters(), lr=LR_C, **hyper)
    both = [oa, oc]

    def device_steps():
        for _ in range(n_steps):
            DeviceAdamW.step_all(both)

    result["c_device_steps"] = dict(timed(device_steps), steps=n_steps)
    actor, critic = copy.deepcopy(actor0), copy.deepcopy(critic0)
    gradients(actor, critic, torch.arange(rows, device=dev), slices[0])
    optims = torch_optims(actor, critic)

    def torch_steps():
        for _ in range(n_steps):
            torch_step(optims)

    result["c_torch_steps"] = dict(timed(torch_steps), steps=n_steps)

    g, b = result["gradient_launches_epoch"]["median_us"], result["b_updater_epoch"]["median_us"]
    a_def = result["a_torch_epoch"]["default"]["median_us"]
    result["ratios"] = {
        "a_default_over_b": round(a_def / b, 2),
        "optimiser_share_of_a_default": round((a_def - g) / a_def, 3),
        "gradient_share_of_b": round(g / b, 3),
        "c_torch_over_device_step": round(result["c_torch_steps"]["median_us"] / result["c_device_steps"]["median_us"], 2),
        "device_step_us": round(result["c_device_steps"]["median_us"] / n_steps, 2),
        "torch_step_us": round(result["c_torch_steps"]["median_us"] / n_steps, 2)}
    print(json.dumps(result))


main()
