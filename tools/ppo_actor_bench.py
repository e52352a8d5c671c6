#!/usr/bin/env python3
"""The actor half of a PPO update on one horizon: `RolloutStorage.actor_grad` (ppo_actor_kernel + ppo_reduce_kernel: one launch and a
small reduction per minibatch, reading the storage in place) against the path it replaces — the reference's eager torch code
(ppo.py:154-186 + policy_regularization.py): shuffled index clones of the `sample()` tensors, three passes through the module,
Normal / ratio / clipped surrogate / entropy, autograd backwards — on the SAME rows, which come from a real `collect`.

    python tools/ppo_actor_bench.py [--envs 65536] [--horizon 32] [--minibatches 32] [--reps 20]

Coupled (23 -> 16 -> 16 -> 4).  Two rows: ONE minibatch of all T * N rows, and --minibatches shuffled minibatches of T * N / that many
rows (one epoch).  HIP events around each path, warm-up, median of --reps.  The optimiser step is in neither path.  Prints ONE JSON
line: both times and their ratio per row, and the worst gradient difference between the two paths."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gym_rotor_amd import ActorParams, QuadVecEnv, RolloutStorage  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--envs", type=int, default=65536)
p.add_argument("--horizon", type=int, default=32)
p.add_argument("--minibatches", type=int, default=32)
p.add_argument("--reps", type=int, default=20)
p.add_argument("--warmup", type=int, default=3)
a = p.parse_args()
dev = torch.device("cuda", 0)
CO = dict(clip=0.2, entropy_coef=0.01, lam_T=0.4, lam_S=0.3, lam_M=0.6, max_action=1.0)


class Actor(torch.nn.Module):  # the shape of the reference's MLP_Actor_PPO (attributes fc1, fc2, mean_linear, log_std)
    def __init__(self, D=23, H=16, A=4):
        super().__init__()
        self.fc1, self.fc2, self.mean_linear = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, A)
        self.log_std = torch.nn.Parameter(torch.full((1, A), -0.5))

    def forward(self, x):
        return torch.tanh(self.mean_linear(torch.relu(self.fc2(torch.relu(self.fc1(x))))))


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
    m = Actor().to(dev)
    params = ActorParams.from_module(m)
    for _ in range(3):   # (episodes of every age, not one horizon after a common reset)
        st.collect(env, [params])
    adv = torch.randn(T, N, 1, device=dev)
    noise = torch.randn(23, device=dev) * 0.05
    nominal = RolloutStorage.nominal_action(env, 0)
    ps = (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.mean_linear.weight, m.mean_linear.bias, m.log_std)
    mse = torch.nn.functional.mse_loss
    rows = []
    for n_mb in (1, a.minibatches):
        perm = torch.randperm(T * N, device=dev)
        mb = (T * N + n_mb - 1) // n_mb
        seen = {}

        def kernel_path():
            for i in range(n_mb):
                seen["kernel"], _ = st.actor_grad(0, params, adv, perm[i * mb:(i + 1) * mb], noise=noise, nominal=nominal, **CO)

        def torch_path():
            obs, act, _, obs_next, _, logp = st.sample()
            b_obs, b_act, b_next, b_adv, b_logp = (t[perm].clone() for t in (obs[0], act[0], obs_next[0], adv.reshape(-1, 1), logp[0]))
            for i in range(n_mb):
                sl = slice(i * mb, (i + 1) * mb)
                dist = torch.distributions.Normal(m(b_obs[sl]), m.log_std.expand(b_obs[sl].shape[0], -1).exp())
                ratio = torch.exp(dist.log_prob(b_act[sl]).sum(1, keepdim=True) - b_logp[sl].sum(1, keepdim=True))
                s1, s2 = ratio * b_adv[sl], torch.clamp(ratio, 1 - CO["clip"], 1 + CO["clip"]) * b_adv[sl]
                loss = -(torch.min(s1, s2) + CO["entropy_coef"] * dist.entropy().sum(1, keepdim=True)).mean()
                a0 = m(b_obs[sl]).clamp(-1, 1)
                loss = loss + CO["lam_T"] * mse(a0, m(b_next[sl]).clamp(-1, 1)) + CO["lam_S"] * mse(a0, m(b_obs[sl] + noise).clamp(-1, 1)) \
                    + CO["lam_M"] * mse(a0, nominal.expand_as(a0))
                m.zero_grad()
                loss.backward()
            seen["torch"] = [q.grad.reshape(-1).clone() for q in ps]

        t_torch = timed(torch_path)
        t_kernel = timed(kernel_path)
        diff = max(float((g.reshape(-1) - t).abs().max()) for g, t in zip(seen["kernel"].values(), seen["torch"]))   # the last minibatch
        rows.append({"minibatches": n_mb, "rows_per_minibatch": mb, "actor_grad_us": round(t_kernel[0], 1), "actor_grad_us_min": round(t_kernel[1], 1),
                     "torch_eager_us": round(t_torch[0], 1), "torch_eager_us_min": round(t_torch[1], 1),
                     "torch_over_kernel": round(t_torch[0] / t_kernel[0], 2), "max_abs_grad_diff_between_paths": diff})
    print(json.dumps({"workload": "PPO actor loss + gradients, Coupled 23->16->16->4: actor_grad against eager torch autograd with index clones",
                      "envs": N, "horizon": T, "reps": a.reps, "coefficients": CO, "rows": rows}))


main()
