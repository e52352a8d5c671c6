#!/usr/bin/env python
"""The critic half of a TD3 update on one minibatch: `td3_critic_loss` (td3_target_kernel, then twinq_kernel + twinq_reduce_kernel)
against the same update written in eager torch (index clones, the target actor, clamps, cat, two twin-critic passes, min, the
Bellman line, two mse_loss, autograd), Coupled 23 + 4 -> 62, the same eps for both paths.

    python tools/td3_critic_bench.py [--batches 256 65536 2097152] [--reps 20]

HIP events around one call, median of --reps with min .. max; the worst gradient difference between the two paths; and the MFMA time
of the twin-Q kernel by arithmetic (1008 v_mfma_f32_16x16x4_f32 of 32 clocks per tile and network, 2.4 GHz)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Actor(torch.nn.Module):   # the reference's MLP_Actor_TD3
    def __init__(self, D=23, H=16, A=4):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, A)

    def forward(self, x):
        return torch.tanh(self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(x))))))


class Critic(torch.nn.Module):   # the reference's MLP_Critic (TD3)
    def __init__(self, D=27, H=62):
        super().__init__()
        for k, (i, o) in enumerate(((D, H), (H, H), (H, 1)) * 2, 1):
            setattr(self, f"fc{k}", torch.nn.Linear(i, o))

    def forward(self, s, a):
        sa = torch.cat([s, a], 1)
        q1 = self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(sa)))))
        q2 = self.fc6(torch.relu(self.fc5(torch.relu(self.fc4(sa)))))
        return q1, q2


def eager(critic, critic_t, actor_t, buf, idx, eps, discount=0.99, target_noise=0.2, noise_clip=0.5, max_action=1.0):
    obs, act, rwd, nxt, done = buf.obs[0][idx], buf.act[0][idx], buf.rwd[0][idx][:, None], buf.obs_next[0][idx], buf.done[0][idx][:, None]
    with torch.no_grad():
        a = (actor_t(nxt) + (eps * target_noise).clamp(-noise_clip, noise_clip)).clamp(-max_action, max_action)
        y = rwd + discount * (1 - done) * torch.min(*critic_t(nxt, a))
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
    from gym_rotor_amd import ReplayBuffer, td3_critic_loss
    torch.manual_seed(0)
    critic, critic_t, actor_t = Critic().cuda(), Critic().cuda(), Actor().cuda()
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
        dev = timed(lambda: td3_critic_loss(critic, critic_t, actor_t, buf, 0, idx, noise=eps), args.reps)
        ref = timed(lambda: eager(twin, critic_t, actor_t, buf, idx, eps), args.reps)
        diff = max(float((p.grad - q.grad).abs().max()) for p, q in zip(critic.parameters(), twin.parameters()))
        gmax = max(float(q.grad.abs().max()) for q in twin.parameters())
        tiles = (B + 63) // 64
        per_wave = -(-tiles // min(tiles, 512))
        mfma_ms = per_wave * 1008 * 32 / 2.4e9 * 1e3
        print(f"B = {B}: td3_critic_loss {dev[0]:.3f} ms ({dev[1]:.3f} .. {dev[2]:.3f}); eager torch {ref[0]:.3f} ms ({ref[1]:.3f} .. {ref[2]:.3f}); "
              f"ratio {ref[0] / dev[0]:.1f}; worst gradient difference {diff:.2e} (largest gradient entry {gmax:.2e}); twin-Q MFMA time by "
              f"arithmetic {mfma_ms:.4f} ms ({per_wave} tile(s) per wave)", flush=True)


if __name__ == "__main__":
    main()
