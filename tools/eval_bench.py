#!/usr/bin/env python3
"""Times QuadVecEnv.evaluate (qr_evaluate_actor: eval_policy for every env in one launch) against what the library offered before
it: rollout_actor(deterministic=True, n_steps=T) with auto-reset off — [T, N] rows of observations, actions, log-probabilities,
rewards and dones — reduced to eval_policy's per-episode figures by a torch scan on the GPU.

Both wrappers at --envs (65 536) envs and T = 1000 steps (eval_max_steps), with two actors:
  trained-like  zero weights and the mean bias that gives hover thrust, from rest at the goal: every episode runs all T steps;
  random        the reference's initial actor (random_actors), from the eval reset distribution: episodes crash early.
Prints one JSON line per (kind, actor) with us per launch and per 65 536-env step (launch time / T), the mean episode length and
the speed-up, and checks that both paths give the same lengths.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_rotor_amd import QuadVecEnv, random_actors  # noqa: E402
from gym_rotor_amd.constants import QuadConstants  # noqa: E402


def scan(ro, framework, T, x_lim=1.0):
    """eval_policy's accounting over the rollout's rows, in torch on the device (what a caller without evaluate() writes)."""
    done = ro["terminated"].any(-1)                                      # [T, N]
    any_d = done.any(0)
    first = torch.where(any_d, done.int().argmax(0), torch.full_like(any_d, T - 1, dtype=torch.long))
    alive = torch.arange(T, device=done.device)[:, None] <= first[None, :]
    ex = ro["obs0"][..., 0:3].double() * x_lim
    eb1 = (ro["obs1"][..., 0] if framework == "MODUL" else ro["obs0"][..., 18]).double() * math.pi
    b = (-ex.norm(dim=-1) - eb1.abs() + 2.0).clamp(0.0, 2.0) * 0.5
    ret = (ro["reward"].double() * alive[..., None]).sum(0)
    bench = (b * alive).sum(0)
    return ret, bench, first + 1


def hover_actors(kind):
    c = QuadConstants()
    hover = c.m_nominal * c.g / 4
    maxf = c.c_tw_nominal * hover
    avrg = (c.min_force + maxf) / 2
    actors = random_actors(kind, "cuda")
    for a in actors:
        for t in (a.fc1_w, a.fc1_b, a.fc2_w, a.fc2_b, a.mean_w, a.mean_b):
            t.zero_()
    actors[0].mean_b[0] = math.atanh((hover - avrg) / (maxf - avrg))
    return actors


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) * 1e3)
    return float(np.median(times))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=65536)
    p.add_argument("--steps", type=int, default=1000)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--kinds", default="coupled,decoupled")
    a = p.parse_args()
    N, T = a.envs, a.steps
    for kind in a.kinds.split(","):
        for actor_name in ("trained-like", "random"):
            env = QuadVecEnv(kind, N, device="cuda", seed=1992, autotune=False)
            if actor_name == "trained-like":
                actors = hover_actors(kind)
                s = np.zeros((N, 18))
                s[:, 6:15] = np.eye(3).reshape(-1, order="F")
                env.set_state(s, integ=np.zeros((N, 8)))
            else:
                actors = random_actors(kind, "cuda", generator=torch.Generator("cuda").manual_seed(0))
                env.reset("eval")
            obs = [o.clone() for o in env.get_norm_error_state()]
            sd = env.state_dict()
            fw = env.framework

            def run_eval():
                env.load_state_dict(sd)
                return env.evaluate(actors, max_steps=T, obs=obs)

            def run_rollout():
                env.load_state_dict(sd)
                ro = env.rollout_actor(actors, T, obs=obs, deterministic=True)
                return scan(ro, fw, T)

            got = run_eval()
            _, _, want_len = run_rollout()
            torch.cuda.synchronize()
            same = bool(torch.equal(got["length"].long(), want_len))
            mean_len = float(got["length"].double().mean())
            del got, want_len
            t_eval = timed(run_eval, a.reps)
            t_ro = timed(run_rollout, a.reps)
            print(json.dumps({"kind": kind, "actor": actor_name, "envs": N, "max_steps": T, "mean_length": round(mean_len, 1),
                              "evaluate_us": round(t_eval, 1), "evaluate_us_per_step": round(t_eval / T, 3),
                              "rollout_scan_us": round(t_ro, 1), "rollout_scan_us_per_step": round(t_ro / T, 3),
                              "speedup": round(t_ro / t_eval, 2), "same_lengths": same}), flush=True)
            del env
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
