#!/usr/bin/env python
"""The actor half of a SAC update for agent k under the centralized (CTDE) twin critic of the Decoupled env, 15 + 3 / 4 + 1 -> 62, on one
minibatch: `sac_actor_loss_ctde` (ctde_sac_actor_kernel + sac_actor_reduce_kernel) against
  eager      the reference's CTDE branch in eager torch (index clones, both actors' samples, two cat, both critics, min, the second
             sample of agent k, three more samples in policy_regularization, autograd, alpha's loss), the same draws and noise row;
  one agent  as a yardstick, the one-agent `sac_actor_loss` of agent k's actor with a critic of its own widths at the same B: what the
             second actor's pass, the second sample and the two further row sources cost on top.

    python tools/sac_ctde_actor_bench.py [--batches 256 65536 2097152] [--reps 20]

HIP events around one call, median of --reps with min .. max, k = 0 and k = 1; and the worst gradient difference of the device path to
eager torch."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OD, AD, H = (15, 3), (4, 1), 62
DIMS = ((15, 16, 4), (3, 4, 1))
LAM = (0.4, 0.3, 0.6)
ALPHA = 0.2


class SacActor(torch.nn.Module):   # the reference's MLP_Actor_SAC, sample() with the draw supplied
    def __init__(self, D, Hh, A):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(D, Hh), torch.nn.Linear(Hh, Hh)
        self.mean_linear, self.log_std_linear = torch.nn.Linear(Hh, A), torch.nn.Linear(Hh, A)

    def sample(self, x, eps):
        h = torch.relu(self.fc2(torch.relu(self.fc1(x))))
        mean, ls = self.mean_linear(h), torch.clamp(self.log_std_linear(h), -20.0, 2.0)
        a = torch.tanh(mean + ls.exp() * eps)
        lp = -0.5 * eps * eps - ls - 0.5 * math.log(2 * math.pi) - torch.log((1 - a.pow(2)) + 1e-6)
        return a, lp.sum(1, keepdim=True)


class Critic(torch.nn.Module):   # the reference's MLP_Critic_CTDE (and, with one agent's widths, MLP_Critic)
    def __init__(self, D=sum(OD) + sum(AD)):
        super().__init__()
        for k, (i, o) in enumerate(((D, H), (H, H), (H, 1)) * 2, 1):
            setattr(self, f"fc{k}", torch.nn.Linear(i, o))

    def forward(self, s, a):
        sa = torch.cat([torch.cat(s, 1), torch.cat(a, 1)], 1)
        return (self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(sa))))), self.fc6(torch.relu(self.fc5(torch.relu(self.fc4(sa))))))


def eager(actors, critic, log_alpha, buf, k, idx, e, noise, nominal, max_action=1.0):
    """sac.py:175-211 with policy_regularization.py, agent k."""
    mse = torch.nn.functional.mse_loss
    obs_n = [o[idx] for o in buf.obs]
    nxt = buf.obs_next[k][idx]
    act_n = [actors[i].sample(obs_n[i], e["eps" if i == k else "eps_other"])[0] for i in (0, 1)]
    logp = actors[k].sample(obs_n[k], e["eps_logp"])[1]
    loss = -(torch.min(*critic(obs_n, act_n)) - ALPHA * logp).mean()
    r = actors[k].sample(obs_n[k], e["eps_reg"])[0].clamp(-max_action, max_action)
    rn = actors[k].sample(nxt, e["eps_next"])[0].clamp(-max_action, max_action)
    rp = actors[k].sample(obs_n[k] + noise[None, :], e["eps_pert"])[0].clamp(-max_action, max_action)
    loss = loss + LAM[0] * mse(r, rn) + LAM[1] * mse(r, rp) + LAM[2] * mse(r, nominal[None, :].expand_as(r))
    actors[k].zero_grad()
    loss.backward()
    alpha_loss = -(log_alpha * (-float(AD[k]) + logp).detach()).mean()
    log_alpha.grad = None
    alpha_loss.backward()
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


def own(m):
    return [t for l in (m.fc1, m.fc2, m.mean_linear, m.log_std_linear) for t in (l.weight, l.bias)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 65536, 2097152])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from gym_rotor_amd import ReplayBuffer, sac_actor_loss, sac_actor_loss_ctde
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
            dev_a, ref_a, one_a = ([SacActor(*d).cuda() for d in DIMS] for _ in range(3))
            for m in (0, 1):
                ref_a[m].load_state_dict(dev_a[m].state_dict()), one_a[m].load_state_dict(dev_a[m].state_dict())
            one_c = Critic(OD[k] + AD[k]).cuda()
            one_buf = ReplayBuffer(rows, [OD[k]], [AD[k]], "cuda")
            one_buf.obs[0], one_buf.obs_next[0] = buf.obs[k], buf.obs_next[k]
            one_buf.count, one_buf.current_size = 0, rows
            noise = 0.05 * torch.randn(OD[k], device="cuda", generator=g)
            nominal = torch.tensor([-0.3, 0.0, 0.0, 0.0][:AD[k]] if k == 0 else [0.0], device="cuda")
            e = {n: torch.randn(B, AD[1 - k] if n == "eps_other" else AD[k], device="cuda", generator=g)
                 for n in ("eps", "eps_other", "eps_logp", "eps_reg", "eps_next", "eps_pert")}
            la_dev, la_ref, la_one = (torch.zeros(1, device="cuda", requires_grad=True) for _ in range(3))
            kw = dict(alpha=ALPHA, lam_T=LAM[0], lam_S=LAM[1], lam_M=LAM[2], noise=noise, nominal=nominal)
            one_e = {n: e[n] for n in ("eps", "eps_reg", "eps_next", "eps_pert")}
            dev = timed(lambda: sac_actor_loss_ctde(dev_a, critic, buf, k, idx, log_alpha=la_dev, **e, **kw), args.reps)
            ref = timed(lambda: eager(ref_a, critic, la_ref, buf, k, idx, e, noise, nominal), args.reps)
            one = timed(lambda: sac_actor_loss(one_a[k], one_c, one_buf, 0, idx, log_alpha=la_one, **one_e, **kw), args.reps)
            diff = max(float((p.grad - q.grad).abs().max()) for p, q in zip(own(dev_a[k]) + [la_dev], own(ref_a[k]) + [la_ref]))
            gmax = max(float(q.grad.abs().max()) for q in own(ref_a[k]))
            print(f"B = {B}, k = {k}: sac_actor_loss_ctde {dev[0]:.3f} ms ({dev[1]:.3f} .. {dev[2]:.3f}); eager torch {ref[0]:.3f} ms "
                  f"({ref[1]:.3f} .. {ref[2]:.3f}), ratio {ref[0] / dev[0]:.1f}; one-agent sac_actor_loss {one[0]:.3f} ms ({one[1]:.3f} .. {one[2]:.3f}), "
                  f"ctde / one-agent {dev[0] / one[0]:.3f}; worst gradient difference to eager {diff:.2e} (largest gradient entry {gmax:.2e})", flush=True)


if __name__ == "__main__":
    main()
