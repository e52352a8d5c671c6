#!/usr/bin/env python
"""The critic half of a SAC update on one minibatch: `sac_critic_loss` (sac_target_kernel, then twinq_kernel + twinq_reduce_kernel)
against the same update written in eager torch as the reference writes it (index clones, MLP_Actor_SAC.sample on obs_next, cat, the
target critic's two passes, min, the entropy term, the Bellman line, two mse_loss, autograd), Coupled 23 + 4 -> 62.  The eager path
draws its own noise (rsample), the device path is given one: the timing is what is compared, and the gradients only loosely (both
use the same minibatch, not the same draws — see tests/test_gpu_sac_critic.py for the numbers).

    python tools/sac_critic_bench.py [--batches 256 65536 2097152] [--reps 20]

HIP events around one call, median of --reps with min .. max, everything in one session."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Actor(torch.nn.Module):   # the reference's MLP_Actor_SAC
    def __init__(self, D=23, H=16, A=4):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(D, H), torch.nn.Linear(H, H)
        self.mean_linear, self.log_std_linear = torch.nn.Linear(H, A), torch.nn.Linear(H, A)

    def sample(self, x):
        x = torch.relu(self.fc2(torch.relu(self.fc1(x))))
        mean, log_std = self.mean_linear(x), torch.clamp(self.log_std_linear(x), min=-20, max=2)
        normal = torch.distributions.Normal(mean, log_std.exp())
        x_t = normal.rsample()
        action = torch.tanh(x_t)
        log_prob = normal.log_prob(x_t)
        log_prob -= torch.log((1 - action.pow(2)) + 1e-6)
        return action, log_prob.sum(1, keepdim=True), torch.tanh(mean)


class Critic(torch.nn.Module):   # the reference's MLP_Critic (TD3's, which SAC uses)
    def __init__(self, D=27, H=62):
        super().__init__()
        for k, (i, o) in enumerate(((D, H), (H, H), (H, 1)) * 2, 1):
            setattr(self, f"fc{k}", torch.nn.Linear(i, o))

    def forward(self, s, a):
        sa = torch.cat([s, a], 1)
        q1 = self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(sa)))))
        q2 = self.fc6(torch.relu(self.fc5(torch.relu(self.fc4(sa)))))
        return q1, q2


def eager(critic, critic_t, actor, buf, idx, discount=0.99, alpha=0.2):
    obs, act, rwd, nxt, done = buf.obs[0][idx], buf.act[0][idx], buf.rwd[0][idx][:, None], buf.obs_next[0][idx], buf.done[0][idx][:, None]
    with torch.no_grad():
        a, logp, _ = actor.sample(nxt)
        y = rwd + discount * (1 - done) * (torch.min(*critic_t(nxt, a)) - alpha * logp)
    q1, q2 = critic(obs, act)
    loss = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
    critic.zero_grad()
    loss.backward()
    return loss


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 65536, 2097152])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from gym_rotor_amd import ReplayBuffer, sac_critic_loss
    torch.manual_seed(0)
    critic, critic_t, actor = Critic().cuda(), Critic().cuda(), Actor().cuda()
    twin = Critic().cuda()
    twin.load_state_dict(critic.state_dict())
    for B in args.batches:
        rows = max(B, 1 << 20)
        buf = ReplayBuffer(rows, [23], [4], "cuda")
        g = torch.Generator(device="cuda").manual_seed(B)
        buf.obs[0].copy_(torch.rand(rows, 23, device="cuda", generator=g) * 2 - 1)
        buf.obs_next[0].copy_(torch.rand(rows, 23, device="cuda", generator=g) * 2 - 1)
        buf.act[0].copy_(torch.rand(rows, 4, device="cuda", generator=g) * 2 - 1)
        buf.rwd[0].copy_(torch.randn(rows, device="cuda", generator=g))
        buf.done[0].copy_((torch.rand(rows, device="cuda", generator=g) < 0.05).float())
        buf.count, buf.current_size = 0, rows
        idx = buf.sample(B, g)
        eps = torch.randn(B, 4, device="cuda", generator=g)
        dev = timed(lambda: sac_critic_loss(critic, critic_t, actor, buf, 0, idx, discount=0.99, alpha=0.2, noise=eps), args.reps)
        ref = timed(lambda: eager(twin, critic_t, actor, buf, idx), args.reps)
        print(f"B = {B}: sac_critic_loss {dev[0]:.3f} ms ({dev[1]:.3f} .. {dev[2]:.3f}); eager torch {ref[0]:.3f} ms ({ref[1]:.3f} .. {ref[2]:.3f}); "
              f"ratio {ref[0] / dev[0]:.1f}", flush=True)


if __name__ == "__main__":
    main()
