#!/usr/bin/env python
"""The actor half of a TD3 update on one minibatch: `td3_actor_loss` (dpg_actor_kernel + dpg_reduce_kernel) against the same update
written in eager torch (index clones, three actor passes, the Q1 pass, three mse_loss, autograd), Coupled 23 + 4 -> 62, the same noise
row for both paths; and `soft_update` of an actor's and a twin critic's 18 tensors in one launch against the reference's loop of
eighteen copy_ lines.

    python tools/td3_actor_bench.py [--batches 256 65536 2097152] [--reps 20]

HIP events around one call, median of --reps with min .. max; the worst gradient difference between the two paths."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from td3_critic_bench import Actor, Critic, timed  # noqa: E402

LAM_T, LAM_S, LAM_M, MAX_ACTION, TAU = 0.4, 0.3, 0.6, 1.0, 0.005


def eager(actor, critic, buf, idx, noise, nominal):
    obs, nxt = buf.obs[0][idx], buf.obs_next[0][idx]
    act = actor(obs).clamp(-MAX_ACTION, MAX_ACTION)
    sa = torch.cat([obs, act], 1)
    loss = -critic.fc3(torch.relu(critic.fc2(torch.relu(critic.fc1(sa))))).mean()   # MLP_Critic.Q1
    mse = torch.nn.functional.mse_loss
    a, a_next = actor(obs).clamp(-MAX_ACTION, MAX_ACTION), actor(nxt).clamp(-MAX_ACTION, MAX_ACTION)   # policy_regularization
    a_pert = actor(obs + noise[None, :]).clamp(-MAX_ACTION, MAX_ACTION)
    loss = loss + LAM_T * mse(a, a_next) + LAM_S * mse(a, a_pert) + LAM_M * mse(a, nominal[None, :].expand_as(a))
    actor.zero_grad()
    loss.backward()
    return loss


def eager_soft(pairs):
    for p, t in pairs:
        t.data.copy_(TAU * p.data + (1 - TAU) * t.data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 65536, 2097152])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from gym_rotor_amd import ReplayBuffer, soft_update, td3_actor_loss
    torch.manual_seed(0)
    actor, critic, twin = Actor().cuda(), Critic().cuda(), Actor().cuda()
    twin.load_state_dict(actor.state_dict())
    g = torch.Generator(device="cuda").manual_seed(1)
    noise, nominal = 0.05 * torch.randn(23, device="cuda", generator=g), torch.tensor([-0.3, 0.0, 0.0, 0.0], device="cuda")
    for B in args.batches:
        rows = max(B, 1 << 20)
        buf = ReplayBuffer(rows, [23], [4], "cuda")
        buf.obs[0].copy_(torch.rand(rows, 23, device="cuda", generator=g) * 2 - 1)
        buf.obs_next[0].copy_(torch.rand(rows, 23, device="cuda", generator=g) * 2 - 1)
        buf.count, buf.current_size = 0, rows
        idx = buf.sample(B, g)
        kw = dict(lam_T=LAM_T, lam_S=LAM_S, lam_M=LAM_M, max_action=MAX_ACTION, noise=noise, nominal=nominal)
        dev = timed(lambda: td3_actor_loss(actor, critic, buf, 0, idx, **kw), args.reps)
        ref = timed(lambda: eager(twin, critic, buf, idx, noise, nominal), args.reps)
        diff = max(float((p.grad - q.grad).abs().max()) for p, q in zip(actor.parameters(), twin.parameters()))
        gmax = max(float(q.grad.abs().max()) for q in twin.parameters())
        print(f"B = {B}: td3_actor_loss {dev[0]:.3f} ms ({dev[1]:.3f} .. {dev[2]:.3f}); eager torch {ref[0]:.3f} ms ({ref[1]:.3f} .. {ref[2]:.3f}); "
              f"ratio {ref[0] / dev[0]:.1f}; worst gradient difference {diff:.2e} (largest gradient entry {gmax:.2e})", flush=True)
    critic_t, actor_t = Critic().cuda(), Actor().cuda()
    c2, a2 = Critic().cuda(), Actor().cuda()
    c2.load_state_dict(critic_t.state_dict())
    a2.load_state_dict(actor_t.state_dict())
    pairs = list(zip(list(critic.parameters()) + list(actor.parameters()), list(c2.parameters()) + list(a2.parameters())))
    dev = timed(lambda: soft_update([critic, actor], [critic_t, actor_t], TAU), args.reps)
    ref = timed(lambda: eager_soft(pairs), args.reps)
    same = all(torch.equal(p.data, q.data) for p, q in zip(list(critic_t.parameters()) + list(actor_t.parameters()), (t for _, t in pairs)))
    print(f"soft_update, 18 tensors: one launch {dev[0]:.3f} ms ({dev[1]:.3f} .. {dev[2]:.3f}); the reference's loop {ref[0]:.3f} ms "
          f"({ref[1]:.3f} .. {ref[2]:.3f}); ratio {ref[0] / dev[0]:.1f}; targets bit-equal after {3 + args.reps} updates each: {same}", flush=True)


if __name__ == "__main__":
    main()
