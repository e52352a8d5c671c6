#!/usr/bin/env python3
"""One TD3 / SAC training iteration on one MI355X, three ways, HIP events, median of 20 with min .. max, the arms alternated in
one process:

  (a) the parent's path: the loss calls, the twin critic stepped as two `DeviceAdamW` groups of six, the actor's group, `soft_update`
      calls, and for SAC a one-entry group for log_alpha plus `torch.exp` for alpha;
  (b) `Td3Updater.update(buffer, 1)` / `SacUpdater.update(buffer, 1)`;
  (c) one replay of `capture(buffer)`, divided by its iterations.

    python tools/offpolicy_update_bench.py [--out FILE]

policy_update_freq = 1, so that every iteration is an update iteration and the three arms do the same work; B = 256 and 65 536;
modes single and ctde.  Nothing is asserted; the table goes to stdout and to --out."""
import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gym_rotor_amd as G  # noqa: E402

DIMS = {"single": ([23], [4], [(23, 16, 4)]), "ctde": ([15, 3], [4, 1], [(15, 16, 4), (3, 4, 1)])}
H = 62


class Twin(torch.nn.Module):
    def __init__(self, din):
        super().__init__()
        for k, (i, o) in enumerate(((din, H), (H, H), (H, 1)) * 2, 1):
            setattr(self, f"fc{k}", torch.nn.Linear(i, o))


class Actor(torch.nn.Module):
    def __init__(self, D, Hh, A, sac):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(D, Hh), torch.nn.Linear(Hh, Hh)
        if sac:
            self.mean_linear, self.log_std_linear = torch.nn.Linear(Hh, A), torch.nn.Linear(Hh, A)
        else:
            self.fc3 = torch.nn.Linear(Hh, A)


def plist(m, names):
    return [t for n in names for t in (getattr(m, n).weight, getattr(m, n).bias)]


def setup(algo, mode, B):
    od, ad, adims = DIMS[mode]
    torch.manual_seed(0)
    cap = max(2 * B, 1024)
    buf = G.ReplayBuffer(cap, od, ad, "cuda", seed=1)
    for k in range(len(od)):
        buf.obs[k].normal_(); buf.obs_next[k].normal_(); buf.act[k].uniform_(-1, 1); buf.rwd[k].uniform_()
    buf.count, buf.current_size = 0, cap
    buf.use_device_state()   # (from the ints above)
    actors = [Actor(*d, algo == "sac").cuda() for d in adims]
    din = [sum(od) + sum(ad)] * len(od) if mode == "ctde" else [od[0] + ad[0]]
    critics = [Twin(d).cuda() for d in din]
    nominal = [torch.zeros(a, device="cuda") for a in ad]
    return buf, (actors, critics, copy.deepcopy(actors), copy.deepcopy(critics), nominal)


def make_updater(algo, mode, mods, B):
    actors, critics, actors_t, critics_t, nominal = mods
    kw = dict(mode=mode, policy_update_freq=1, batch_size=B, nominal=nominal)
    if algo == "td3":
        return G.Td3Updater(actors, critics, actors_t, critics_t, **kw)
    return G.SacUpdater(actors, critics, critics_t, automatic_entropy_tuning=True, **kw)


def parent_path(algo, mode, mods, buf, B, layout):
    """Arm (a) as a callable doing one iteration for every agent."""
    actors, critics, actors_t, critics_t, nominal = mods
    n = len(actors)
    hy = dict(max_norm=100.0, t0=1_000_000, eta_min=1e-5)
    an = ("fc1", "fc2", "fc3") if algo == "td3" else ("fc1", "fc2", "mean_linear", "log_std_linear")
    q1 = [G.DeviceAdamW(plist(c, ("fc1", "fc2", "fc3")), lr=2e-4, **hy) for c in critics]
    q2 = [G.DeviceAdamW(plist(c, ("fc4", "fc5", "fc6")), lr=2e-4, **hy) for c in critics]
    ao = [G.DeviceAdamW(plist(a, an), lr=3e-4, **hy) for a in actors]
    idx = [torch.zeros(B, dtype=torch.int64, device="cuda") for _ in range(n)]
    noise = [{k: (tuple(torch.zeros_like(x) for x in t) if isinstance(t, tuple) else torch.zeros_like(t)) for k, t in layout[j].items()} for j in range(n)]
    if algo == "sac":
        la = [torch.zeros(1, device="cuda", requires_grad=True) for _ in range(n)]
        al = [torch.full((1,), 0.05, device="cuda") for _ in range(n)]
        lo = [G.DeviceAdamW([x], lr=3e-4) for x in la]

    def run():
        for k in range(n):
            buf.sample_index(B, out=idx[k])
            nz = noise[k]
            for name, t in nz.items():
                for x in (t if isinstance(t, tuple) else (t,)):
                    x.normal_(0.0, 0.05 if name == "reg" else 1.0)
            reg = dict(noise=nz["reg"], nominal=nominal[k])
            if algo == "td3":
                if mode == "ctde":
                    G.td3_critic_loss_ctde(critics[k], critics_t[k], actors_t, buf, k, idx[k], noise=nz["smooth"])
                else:
                    G.td3_critic_loss(critics[k], critics_t[k], actors_t[k], buf, k, idx[k], noise=nz["smooth"])
                G.DeviceAdamW.step_all([q1[k], q2[k]])
                if mode == "ctde":
                    G.td3_actor_loss_ctde(actors, critics[k], buf, k, idx[k], **reg)
                else:
                    G.td3_actor_loss(actors[k], critics[k], buf, k, idx[k], **reg)
                ao[k].step()
                G.soft_update([critics[k], actors[k]], [critics_t[k], actors_t[k]], 0.005)
            else:
                e = dict(log_alpha=la[k], alpha=al[k], eps=nz["eps"], eps_reg=nz["eps_reg"], eps_next=nz["eps_next"], eps_pert=nz["eps_pert"])
                if mode == "ctde":
                    G.sac_critic_loss_ctde(critics[k], critics_t[k], actors, buf, k, idx[k], alpha=al[k], noise=nz["next"], noise_logp=nz["noise_logp"])
                else:
                    G.sac_critic_loss(critics[k], critics_t[k], actors[k], buf, k, idx[k], alpha=al[k], noise=nz["next"])
                G.DeviceAdamW.step_all([q1[k], q2[k]])
                if mode == "ctde":
                    G.sac_actor_loss_ctde(actors, critics[k], buf, k, idx[k], eps_logp=nz["eps_logp"], eps_other=nz["eps_other"], **e, **reg)
                else:
                    G.sac_actor_loss(actors[k], critics[k], buf, k, idx[k], **e, **reg)
                G.DeviceAdamW.step_all([ao[k], lo[k]])
                torch.exp(la[k].data, out=al[k])
                G.soft_update(critics[k], critics_t[k], 0.005)
    return run


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-capture", action="store_true")
    args = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}; one iteration (all agents), us: median of 20 (min .. max); arms alternated"]
    for algo in ("td3", "sac"):
        for mode in ("single", "ctde"):
            for B in (256, 65536):
                buf_b, mods_b = setup(algo, mode, B)
                up = make_updater(algo, mode, mods_b, B)
                up.update(buf_b, 1)
                buf_a, mods_a = setup(algo, mode, B)
                arm_a = parent_path(algo, mode, mods_a, buf_a, B, up.noise)
                arms = {"a": arm_a, "b": lambda: up.update(buf_b, 1)}
                if not args.no_capture:
                    buf_c, mods_c = setup(algo, mode, B)
                    up_c = make_updater(algo, mode, mods_c, B)
                    up_c.update(buf_c, 1)
                    arms["c"] = up_c.capture(buf_c)
                for fn in arms.values():
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                t = {k: [] for k in arms}
                for _ in range(20):
                    for k, fn in arms.items():
                        t[k].append(timed(fn))
                cells = "  ".join(f"({k}) {statistics.median(v):8.1f} ({min(v):.1f} .. {max(v):.1f})" for k, v in t.items())
                lines.append(f"{algo} {mode:6s} B={B:6d}  {cells}")
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
