#!/usr/bin/env python
"""The critic half of a TD3 and of a SAC update with the centralized (CTDE) twin critic of the Decoupled env, 15 + 3 / 4 + 1 -> 62, on one
minibatch: `td3_critic_loss_ctde` / `sac_critic_loss_ctde` (one target launch, then ctde_twinq_kernel + twinq_reduce_kernel) against
  eager   the reference's CTDE branch in eager torch (index clones, both actors, cat, two twin-critic passes, min, the Bellman line, two
          mse_loss, autograd), the same draws;
  concat  what a user had before: the one-agent `twinq_grad` fed torch-concatenated rows, and the one-agent targets in their no-actor
          form fed the concatenated obs_next and the actions of both actors evaluated in eager torch — copies included.

    python tools/ctde_critic_bench.py [--batches 256 65536 2097152] [--reps 20]

HIP events around one call, median of --reps with min .. max; and the worst gradient difference of the device path to eager torch."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OD, AD, H = (15, 3), (4, 1), 62
DIMS = ((15, 16, 4), (3, 4, 1))


class Td3Actor(torch.nn.Module):   # the reference's MLP_Actor_TD3
    def __init__(self, D, Hh, A):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(D, Hh), torch.nn.Linear(Hh, Hh), torch.nn.Linear(Hh, A)

    def forward(self, x):
        return torch.tanh(self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(x))))))


class SacActor(torch.nn.Module):   # the reference's MLP_Actor_SAC, rsample's draw supplied
    def __init__(self, D, Hh, A):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(D, Hh), torch.nn.Linear(Hh, Hh)
        self.mean_linear, self.log_std_linear = torch.nn.Linear(Hh, A), torch.nn.Linear(Hh, A)

    def sample(self, x, eps):
        h = torch.relu(self.fc2(torch.relu(self.fc1(x))))
        mean, log_std = self.mean_linear(h), torch.clamp(self.log_std_linear(h), min=-20, max=2)
        std = log_std.exp()
        x_t = mean + std * eps
        a = torch.tanh(x_t)
        logp = torch.distributions.Normal(mean, std).log_prob(x_t) - torch.log((1 - a.pow(2)) + 1e-6)
        return a, logp.sum(1, keepdim=True)


class Critic(torch.nn.Module):   # the reference's MLP_Critic_CTDE
    def __init__(self, D=sum(OD) + sum(AD)):
        super().__init__()
        for k, (i, o) in enumerate(((D, H), (H, H), (H, 1)) * 2, 1):
            setattr(self, f"fc{k}", torch.nn.Linear(i, o))

    def forward(self, s, a):
        sa = torch.cat([torch.cat(s, 1), torch.cat(a, 1)], 1)
        q1 = self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(sa)))))
        q2 = self.fc6(torch.relu(self.fc5(torch.relu(self.fc4(sa)))))
        return q1, q2


def regress(critic, obs_n, act_n, y):
    q1, q2 = critic(obs_n, act_n)
    loss = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
    critic.zero_grad()
    loss.backward()
    return loss


def gather(buf, idx, k):
    return ([o[idx] for o in buf.obs], [a[idx] for a in buf.act], buf.rwd[k][idx][:, None], [o[idx] for o in buf.obs_next], buf.done[k][idx][:, None])


def eager_td3(critic, critic_t, actors_t, buf, k, idx, eps, discount=0.99, target_noise=0.2, noise_clip=0.5, max_action=1.0):
    obs_n, act_n, rwd, nxt_n, done = gather(buf, idx, k)
    with torch.no_grad():
        a_n = [(actors_t[i](nxt_n[i]) + (eps[i] * target_noise).clamp(-noise_clip, noise_clip)).clamp(-max_action, max_action) for i in (0, 1)]
        y = rwd + discount * (1 - done) * torch.min(*critic_t(nxt_n, a_n))
    return regress(critic, obs_n, act_n, y)


def eager_sac(critic, critic_t, actors, buf, k, idx, eps, elp, discount=0.99, alpha=0.2):
    obs_n, act_n, rwd, nxt_n, done = gather(buf, idx, k)
    with torch.no_grad():
        a_n = [actors[i].sample(nxt_n[i], eps[i])[0] for i in (0, 1)]
        logp = actors[k].sample(nxt_n[k], elp)[1]
        y = rwd + discount * (1 - done) * (torch.min(*critic_t(nxt_n, a_n)) - alpha * logp)
    return regress(critic, obs_n, act_n, y)


def concat(sac, live, critic, critic_t, actors, buf, k, idx, eps, elp, ws):
    """The workaround: concatenated copies of the whole minibatch, eager actors, the one-agent launches."""
    from gym_rotor_amd import QCriticParams, sac_target, td3_target, twinq_grad
    with torch.no_grad():
        nxt = [o[idx] for o in buf.obs_next]
        one = {"obs_next": torch.cat(nxt, 1), "rwd": buf.rwd[k][idx], "done": buf.done[k][idx]}
        if sac:
            a_n = torch.cat([actors[i].sample(nxt[i], eps[i])[0] for i in (0, 1)], 1)
            logp = actors[k].sample(nxt[k], elp)[1][:, 0].contiguous()
            y = sac_target(None, QCriticParams.from_module(critic_t, 5), one, 0, None, action_next=a_n, logp_next=logp, out=ws["y"])
        else:
            a_n = torch.cat([(actors[i](nxt[i]) + (eps[i] * 0.2).clamp(-0.5, 0.5)).clamp(-1.0, 1.0) for i in (0, 1)], 1)
            y = td3_target(None, QCriticParams.from_module(critic_t, 5), one, 0, None, action_next=a_n, out=ws["y"])
        obs, act = torch.cat([o[idx] for o in buf.obs], 1), torch.cat([a[idx] for a in buf.act], 1)
    return twinq_grad(QCriticParams.from_module(live, 5), obs, act, y, None, grads=ws["grads"], stats=ws["stats"], workspace=ws["workspace"])


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
    from gym_rotor_amd import ReplayBuffer, sac_critic_loss_ctde, td3_critic_loss_ctde
    from gym_rotor_amd.td3 import twinq_workspace_bytes
    torch.manual_seed(0)
    critic_t = Critic().cuda()
    td3_actors, sac_actors = [Td3Actor(*d).cuda() for d in DIMS], [SacActor(*d).cuda() for d in DIMS]
    k = 1
    for B in args.batches:
        rows = max(B, 1 << 20)
        buf = ReplayBuffer(rows, OD, AD, "cuda")
        g = torch.Generator(device="cuda").manual_seed(B)
        for m in (0, 1):
            buf.obs[m].copy_(torch.rand(rows, OD[m], device="cuda", generator=g) * 2 - 1)
            buf.obs_next[m].copy_(torch.rand(rows, OD[m], device="cuda", generator=g) * 2 - 1)
            buf.act[m].copy_(torch.rand(rows, AD[m], device="cuda", generator=g) * 2 - 1)
            buf.rwd[m].copy_(torch.randn(rows, device="cuda", generator=g))
            buf.done[m].copy_((torch.rand(rows, device="cuda", generator=g) < 0.05).float())
        buf.count, buf.current_size = 0, rows
        idx = buf.sample(B, g)
        eps = [torch.randn(B, a, device="cuda", generator=g) for a in AD]
        elp = torch.randn(B, AD[k], device="cuda", generator=g)
        for sac in (False, True):
            dev_c, ref_c, cat_c = Critic().cuda(), Critic().cuda(), Critic().cuda()
            ref_c.load_state_dict(dev_c.state_dict()), cat_c.load_state_dict(dev_c.state_dict())
            ws = {"y": torch.empty(B, device="cuda"), "stats": torch.empty(4, device="cuda"),
                  "grads": {f"fc{j}_{x}": torch.empty_like(getattr(getattr(cat_c, f"fc{j}"), "weight" if x == "w" else "bias")) for j in range(1, 7) for x in "wb"},
                  "workspace": torch.empty(twinq_workspace_bytes((18, 5, H), B) // 8, dtype=torch.float64, device="cuda")}
            if sac:
                dev = timed(lambda: sac_critic_loss_ctde(dev_c, critic_t, sac_actors, buf, k, idx, noise=eps, noise_logp=elp), args.reps)
                ref = timed(lambda: eager_sac(ref_c, critic_t, sac_actors, buf, k, idx, eps, elp), args.reps)
            else:
                dev = timed(lambda: td3_critic_loss_ctde(dev_c, critic_t, td3_actors, buf, k, idx, noise=eps), args.reps)
                ref = timed(lambda: eager_td3(ref_c, critic_t, td3_actors, buf, k, idx, eps), args.reps)
            cat = timed(lambda: concat(sac, cat_c, None, critic_t, sac_actors if sac else td3_actors, buf, k, idx, eps, elp, ws), args.reps)
            diff = max(float((p.grad - q.grad).abs().max()) for p, q in zip(dev_c.parameters(), ref_c.parameters()))
            dcat = max(float((p.grad - ws["grads"][n]).abs().max()) for (n, _), p in zip(ws["grads"].items(), dev_c.parameters()))
            gmax = max(float(q.grad.abs().max()) for q in ref_c.parameters())
            name = "sac_critic_loss_ctde" if sac else "td3_critic_loss_ctde"
            print(f"B = {B}: {name} {dev[0]:.3f} ms ({dev[1]:.3f} .. {dev[2]:.3f}); eager torch {ref[0]:.3f} ms ({ref[1]:.3f} .. {ref[2]:.3f}), "
                  f"ratio {ref[0] / dev[0]:.1f}; concatenation workaround {cat[0]:.3f} ms ({cat[1]:.3f} .. {cat[2]:.3f}), ratio {cat[0] / dev[0]:.2f}; "
                  f"worst gradient difference to eager {diff:.2e}, to the workaround {dcat:.2e} (largest gradient entry {gmax:.2e})", flush=True)


if __name__ == "__main__":
    main()
