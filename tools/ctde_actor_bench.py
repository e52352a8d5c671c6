#!/usr/bin/env python
"""The actor half of a TD3 update for agent k under the centralized (CTDE) twin critic of the Decoupled env, 15 + 3 / 4 + 1 -> 62, on one
minibatch: `td3_actor_loss_ctde` (ctde_dpg_actor_kernel + dpg_reduce_kernel) against
  eager      the reference's CTDE branch in eager torch (index clones, both actors, two cat, Q1, three more passes of agent k's actor
             in policy_regularization, autograd), the same noise row;
  one agent  as a yardstick, the one-agent `td3_actor_loss` of agent k's actor with a critic of its own widths at the same B: what the
             second actor's pass and the two further row sources cost on top.

    python tools/ctde_actor_bench.py [--batches 256 65536 2097152] [--reps 20]

HIP events around one call, median of --reps with min .. max, k = 0 and k = 1; and the worst gradient difference of the device path to
eager torch."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OD, AD, H = (15, 3), (4, 1), 62
DIMS = ((15, 16, 4), (3, 4, 1))
LAM = (0.4, 0.3, 0.6)


class Td3Actor(torch.nn.Module):   # the reference's MLP_Actor_TD3
    def __init__(self, D, Hh, A):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(D, Hh), torch.nn.Linear(Hh, Hh), torch.nn.Linear(Hh, A)

    def forward(self, x):
        return torch.tanh(self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(x))))))


class Critic(torch.nn.Module):   # the reference's MLP_Critic_CTDE (and, with one agent's widths, MLP_Critic)
    def __init__(self, D=sum(OD) + sum(AD)):
        super().__init__()
        for k, (i, o) in enumerate(((D, H), (H, H), (H, 1)) * 2, 1):
            setattr(self, f"fc{k}", torch.nn.Linear(i, o))

    def Q1(self, s, a):
        sa = torch.cat([torch.cat(s, 1), torch.cat(a, 1)], 1)
        return self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(sa)))))


def eager(actors, critic, buf, k, idx, noise, nominal, max_action=1.0):
    """td3.py:180-200 with policy_regularization.py, agent k."""
    mse = torch.nn.functional.mse_loss
    obs_n = [o[idx] for o in buf.obs]
    nxt = buf.obs_next[k][idx]
    act_n = [actors[i](obs_n[i]).clamp(-max_action, max_action) for i in (0, 1)]
    loss = -critic.Q1(obs_n, act_n).mean()
    a = actors[k](obs_n[k]).clamp(-max_action, max_action)
    loss = (loss + LAM[0] * mse(a, actors[k](nxt).clamp(-max_action, max_action))
            + LAM[1] * mse(a, actors[k](obs_n[k] + noise[None, :]).clamp(-max_action, max_action)) + LAM[2] * mse(a, nominal[None, :].expand_as(a)))
    actors[k].zero_grad()
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
    from gym_rotor_amd import ReplayBuffer, td3_actor_loss, td3_actor_loss_ctde
    torch.manual_seed(0)
    critic = Critic().cuda()
    for B in args.batches:
        rows = max(B, 1 << 20)
        buf = ReplayBuffer(rows, OD, AD, "cuda")
        g = torch.Generator(device="cuda").manual_seed(B)
        for m in (0, 1):
            buf.obs[m].copy_(torch.rand(rows, OD[m], device="cuda", generator=g) * 2 - 1)
            buf.obs_next[m].copy_(torch.rand(rows, OD[m], device="cuda", generator=g) * 2 - 1)
        buf.count, buf.current_size = 0, rows
        idx = buf.sample(B, g)
        for k in (0, 1):
            dev_a, ref_a, one_a = ([Td3Actor(*d).cuda() for d in DIMS] for _ in range(3))
            for m in (0, 1):
                ref_a[m].load_state_dict(dev_a[m].state_dict()), one_a[m].load_state_dict(dev_a[m].state_dict())
            one_c = Critic(OD[k] + AD[k]).cuda()
            one_buf = ReplayBuffer(rows, [OD[k]], [AD[k]], "cuda")
            one_buf.obs[0], one_buf.obs_next[0] = buf.obs[k], buf.obs_next[k]
            one_buf.count, one_buf.current_size = 0, rows
            noise = 0.05 * torch.randn(OD[k], device="cuda", generator=g)
            nominal = torch.tensor([-0.3, 0.0, 0.0, 0.0][:AD[k]] if k == 0 else [0.0], device="cuda")
            kw = dict(lam_T=LAM[0], lam_S=LAM[1], lam_M=LAM[2], noise=noise, nominal=nominal)
            dev = timed(lambda: td3_actor_loss_ctde(dev_a, critic, buf, k, idx, **kw), args.reps)
            ref = timed(lambda: eager(ref_a, critic, buf, k, idx, noise, nominal), args.reps)
            one = timed(lambda: td3_actor_loss(one_a[k], one_c, one_buf, 0, idx, **kw), args.reps)
            diff = max(float((p.grad - q.grad).abs().max()) for p, q in zip(dev_a[k].parameters(), ref_a[k].parameters()))
            gmax = max(float(q.grad.abs().max()) for q in ref_a[k].parameters())
            print(f"B = {B}, k = {k}: td3_actor_loss_ctde {dev[0]:.3f} ms ({dev[1]:.3f} .. {dev[2]:.3f}); eager torch {ref[0]:.3f} ms "
                  f"({ref[1]:.3f} .. {ref[2]:.3f}), ratio {ref[0] / dev[0]:.1f}; one-agent td3_actor_loss {one[0]:.3f} ms ({one[1]:.3f} .. {one[2]:.3f}), "
                  f"ctde / one-agent {dev[0] / one[0]:.3f}; worst gradient difference to eager {diff:.2e} (largest gradient entry {gmax:.2e})", flush=True)


if __name__ == "__main__":
    main()
