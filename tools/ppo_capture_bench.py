#!/usr/bin/env python3
"""One whole PPO update (K_epochs epochs of the reference's minibatches of 128) on one horizon, three ways on the same build, storage and
initial weights, the arms alternating call by call:

  (a) `PpoUpdater.update` with its defaults (shuffle_source = noise_source = "torch": the update as it was before the device sources);
  (b) the same eager loop with shuffle_source = noise_source = "device";
  (c) the callable of `PpoUpdater.capture`: K_epochs replays of one recorded epoch.

and `shuffle` alone against `torch.randperm` at n = 2 097 152.

    python tools/ppo_capture_bench.py [--envs 4096] [--horizon 32] [--batch 128] [--epochs 2] [--reps 20] [--out profiles/ppo_capture_bench.json]

Coupled (actor 23 -> 16 -> 16 -> 4, critic 23 -> 62 -> 62 -> 1), the reference's hyperparameters.  HIP events around one update with a
synchronise behind it, warm-up, median / min / max of --reps.  Prints ONE JSON line and writes it to --out."""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gym_rotor_amd import ActorParams, CriticParams, DeviceAdamW, PpoUpdater, QuadVecEnv, RolloutStorage, shuffle  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--envs", type=int, default=4096)
p.add_argument("--horizon", type=int, default=32)
p.add_argument("--batch", type=int, default=128)
p.add_argument("--epochs", type=int, default=2)
p.add_argument("--reps", type=int, default=20)
p.add_argument("--warmup", type=int, default=2)
p.add_argument("--out", default="profiles/ppo_capture_bench.json")
a = p.parse_args()
dev = torch.device("cuda", 0)
HYPER = dict(max_norm=100.0, t0=1_000_000, eta_min=1e-5)
CO = dict(clip=0.2, lam_T=0.4, lam_S=0.3, lam_M=0.6, max_action=1.0)


class Actor(torch.nn.Module):  # the shape of the reference's MLP_Actor_PPO (attributes fc1, fc2, mean_linear, log_std)
    def __init__(self, D=23, H=16, A=4):
        super().__init__()
        self.fc1, self.fc2, self.mean_linear = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, A)
        self.log_std = torch.nn.Parameter(torch.ones(1, A) * -0.5)


class Critic(torch.nn.Module):  # the shape of the reference's MLP_Critic (attributes fc1, fc2, fc3)
    def __init__(self, D=23, H=62):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, 1)


def one(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternating(arms: dict) -> dict:
    """Warm-up, then --reps rounds with every arm once per round, in order."""
    for _ in range(a.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in arms}
    for _ in range(a.reps):
        for name, fn in arms.items():
            us[name].append(one(fn))
    return {name: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for name, v in us.items()}


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

    def updater(**kw):
        actor, critic = copy.deepcopy(actor0), copy.deepcopy(critic0)
        oa, oc = DeviceAdamW(actor.parameters(), lr=3e-4, **HYPER), DeviceAdamW(critic.parameters(), lr=2e-4, **HYPER)
        return PpoUpdater([actor], [critic], [oa], [oc], K_epochs=a.epochs, actor_batch_size=a.batch, critic_batch_size=a.batch, nominal=[nominal],
                          **CO, **kw)

    up_a, up_b, up_c = updater(noise=[noise]), updater(shuffle_source="device", noise_source="device"), updater(shuffle_source="device", noise_source="device")
    up_c.update(st, adv)
    replay = up_c.capture(st, adv)
    result = {"workload": "one PPO update, Coupled: per epoch a shuffle, then per minibatch the noise row, actor and critic gradients, both optimiser steps",
              "envs": N, "horizon": T, "rows": T * N, "batch": a.batch, "epochs": a.epochs, "minibatches_per_update": a.epochs * -(-T * N // a.batch),
              "reps": a.reps}
    result.update(alternating({"a_torch_sources_eager": lambda: up_a.update(st, adv), "b_device_sources_eager": lambda: up_b.update(st, adv),
                               "c_captured": replay}))
    am, cm = result["a_torch_sources_eager"], result["c_captured"]
    result["c_median_below_a_min"] = bool(cm["median_us"] < am["min_us"])
    result["a_median_over_c_median"] = round(am["median_us"] / cm["median_us"], 2)

    n = 2_097_152
    out = torch.zeros(n, dtype=torch.int64, device=dev)
    draws = iter(range(10 ** 9))
    result["shuffle_alone"] = dict(alternating({"qr_shuffle": lambda: shuffle(out, n=n, seed=1, draw=next(draws), stream=0),
                                                "torch_randperm": lambda: torch.randperm(n, device=dev)}), n=n)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


main()
