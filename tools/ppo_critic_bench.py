#!/usr/bin/env python3
"""The critic half of a PPO update on one horizon: `RolloutStorage.critic_grad` (ppo_critic_kernel + ppo_critic_reduce_kernel: one
launch and a small reduction per minibatch, reading the storage in place) against the path it replaces — the reference's eager torch
code (ppo.py:193-210): shuffled index clones of the observation rows and the TD targets, the module forwards, `.pow(2).mean()` plus
the three L2 terms, autograd backwards — on the SAME rows, which come from a real `collect`.

    python tools/ppo_critic_bench.py [--envs 65536] [--horizon 32] [--minibatches 32] [--reps 20] [--max-workgroups 0]

Coupled (23 -> 62 -> 62 -> 1).  Two rows: ONE minibatch of all T * N rows, and --minibatches shuffled minibatches of T * N / that many
rows (one epoch).  HIP events around each path, warm-up, median of --reps.  The optimiser step is in neither path.  Prints ONE JSON
line: both times and their ratio per row, and the worst gradient difference between the two paths."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gym_rotor_amd import ActorParams, CriticParams, QuadVecEnv, RolloutStorage  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--envs", type=int, default=65536)
p.add_argument("--horizon", type=int, default=32)
p.add_argument("--minibatches", type=int, default=32)
p.add_argument("--reps", type=int, default=20)
p.add_argument("--warmup", type=int, default=3)
p.add_argument("--max-workgroups", type=int, default=0)
a = p.parse_args()
dev = torch.device("cuda", 0)
L2 = 1e-4


class Critic(torch.nn.Module):  # the shape of the reference's MLP_Critic (attributes fc1, fc2, fc3)
    def __init__(self, D=23, H=62):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, 1)

    def forward(self, x):
        return self.fc3(torch.tanh(self.fc2(torch.tanh(self.fc1(x)))))


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms) * 1e3, min(ms) * 1e3


def main():
    N, T = a.envs, a.horizon
    torch.manual_seed(0)
    env = QuadVecEnv("coupled", N, device=dev, auto_reset=True, seed=0)
    env.reset("train")
    env.get_norm_error_state()
    st = RolloutStorage(env, T)
    actor = ActorParams.random(23, 16, 4, device=dev)
    m = Critic().to(dev)
    params = CriticParams.from_module(m)
    for _ in range(3):   # (episodes of every age, not one horizon after a common reset)
        st.collect(env, [actor])
    nv = st.compute_values([params])
    st.compute_gae(0.99, 0.9, next_value=nv, want_stats=False)
    ps = (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias)
    rows = []
    for n_mb in (1, a.minibatches):
        perm = torch.randperm(T * N, device=dev)
        mb = (T * N + n_mb - 1) // n_mb
        seen = {}

        def kernel_path():
            for i in range(n_mb):
                seen["kernel"], _ = st.critic_grad(0, params, perm[i * mb:(i + 1) * mb], l2_reg=L2, max_workgroups=a.max_workgroups)

        def torch_path():
            b_obs, b_tgt = st.obs[0][:T].reshape(T * N, -1)[perm].clone(), st.td_target.reshape(T * N, 1)[perm].clone()
            for i in range(n_mb):
                sl = slice(i * mb, (i + 1) * mb)
                loss = (m(b_obs[sl]) - b_tgt[sl]).pow(2).mean()
                for name, param in m.named_parameters():
                    if "weight" in name:
                        loss = loss + param.pow(2).sum() * L2
                m.zero_grad()
                loss.backward()
            seen["torch"] = [q.grad.reshape(-1).clone() for q in ps]

        t_torch = timed(torch_path)
        t_kernel = timed(kernel_path)
        diff = max(float((g.reshape(-1) - t).abs().max()) for g, t in zip(seen["kernel"].values(), seen["torch"]))   # the last minibatch
        rows.append({"minibatches": n_mb, "rows_per_minibatch": mb, "critic_grad_us": round(t_kernel[0], 1), "critic_grad_us_min": round(t_kernel[1], 1),
                     "torch_eager_us": round(t_torch[0], 1), "torch_eager_us_min": round(t_torch[1], 1),
                     "torch_over_kernel": round(t_torch[0] / t_kernel[0], 2), "max_abs_grad_diff_between_paths": diff})
    print(json.dumps({"workload": "PPO critic loss + gradients, Coupled 23->62->62->1: critic_grad against eager torch autograd with index clones",
                      "envs": N, "horizon": T, "reps": a.reps, "l2_reg": L2, "max_workgroups": a.max_workgroups, "rows": rows}))


main()
