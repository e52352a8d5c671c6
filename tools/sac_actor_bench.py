#!/usr/bin/env python
"""The actor half of a SAC update on one minibatch: `sac_actor_loss` (sac_actor_kernel + sac_actor_reduce_kernel) against the same
update written in eager torch as the reference writes it (index clones, four MLP_Actor_SAC.sample passes, the critic's two passes, min,
the three smoothness terms of policy_regularization, autograd), Coupled 23 + 4 -> 62, and beside both `td3_actor_loss` on the same
buffer.  The eager path draws its own noise (rsample), the device path is given its four draws: the timing is what is compared (see
tests/test_gpu_sac_actor.py for the numbers).

    python tools/sac_actor_bench.py [--batches 256 65536 2097152] [--reps 20]

HIP events around one call, median of --reps with min .. max, everything in one session.  No ratio is promised."""
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


def eager(critic, actor, buf, idx, noise_row, nominal, alpha=0.2, lam=(0.4, 0.3, 0.6), max_action=1.0):
    obs, nxt = buf.obs[0][idx], buf.obs_next[0][idx]
    a, logp, _ = actor.sample(obs)
    loss = -(torch.min(*critic(obs, a)) - alpha * logp).mean()
    r = actor.sample(obs)[0].clamp(-max_action, max_action)
    rn = actor.sample(nxt)[0].clamp(-max_action, max_action)
    rp = actor.sample(obs + noise_row)[0].clamp(-max_action, max_action)
    mse = torch.nn.functional.mse_loss
    loss = loss + lam[0] * mse(r, rn) + lam[1] * mse(r, rp) + lam[2] * mse(r, nominal.expand_as(r))
    actor.zero_grad()
    loss.backward()
    return loss


class Td3Actor(torch.nn.Module):   # the reference's MLP_Actor_TD3
    def __init__(self, D=23, H=16, A=4):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, A)


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
    from gym_rotor_amd import ReplayBuffer, sac_actor_loss, td3_actor_loss
    torch.manual_seed(0)
    critic, actor, td3 = Critic().cuda(), Actor().cuda(), Td3Actor().cuda()
    twin = Actor().cuda()
    twin.load_state_dict(actor.state_dict())
    for B in args.batches:
        rows = max(B, 1 << 20)
        buf = ReplayBuffer(rows, [23], [4], "cuda")
        g = torch.Generator(device="cuda").manual_seed(B)
        buf.obs[0].copy_(torch.rand(rows, 23, device="cuda", generator=g) * 2 - 1)
        buf.obs_next[0].copy_(torch.rand(rows, 23, device="cuda", generator=g) * 2 - 1)
        buf.count, buf.current_size = 0, rows
        idx = buf.sample(B, g)
        eps = [torch.randn(B, 4, device="cuda", generator=g) for _ in range(4)]
        noise_row = torch.randn(23, device="cuda", generator=g) * 0.05
        nominal = torch.tensor([-0.2, 0.0, 0.0, 0.0], device="cuda")
        kw = dict(noise=noise_row, nominal=nominal)
        dev = timed(lambda: sac_actor_loss(actor, critic, buf, 0, idx, alpha=0.2, eps=eps[0], eps_reg=eps[1], eps_next=eps[2], eps_pert=eps[3], **kw),
                    args.reps)
        tdev = timed(lambda: td3_actor_loss(td3, critic, buf, 0, idx, **kw), args.reps)
        ref = timed(lambda: eager(critic, twin, buf, idx, noise_row, nominal), args.reps)
        print(f"B = {B}: sac_actor_loss {dev[0]:.3f} ms ({dev[1]:.3f} .. {dev[2]:.3f}); td3_actor_loss {tdev[0]:.3f} ms ({tdev[1]:.3f} .. {tdev[2]:.3f}); "
              f"eager torch {ref[0]:.3f} ms ({ref[1]:.3f} .. {ref[2]:.3f}); eager / device {ref[0] / dev[0]:.1f}", flush=True)


if __name__ == "__main__":
    main()
