#!/usr/bin/env python
"""What PPO's advantages cost per collected horizon with the reference's time-limit done rule: three arms alternated call by call in one
process,
    (a) what a user had to write for the same result before qr_gae_rule: the rule's done flags patched in torch, `compute_gae` on them
        (with its torch per-agent sums for Decoupled), `RolloutStorage.normalize`,
    (b) `compute_gae(time_limit="solved", normalized=True)` (qr_gae_rule: three launches behind one C call),
    (c) plain `compute_gae` plus `normalize`: each agent's own flag — the cost of the rule alone is (a) - (c),
at tools/replay_bench.py's shape (T = 32, N = 16 384), Coupled and Decoupled.

    python tools/gae_bench.py [--horizon 32] [--envs 16384] [--reps 20] [--json PATH]

HIP events around one call, median of --reps with min .. max.  Condition, printed with its numbers: (b)'s median lies below (a)'s
minimum.  After the timing the results of (a) and (b) are compared.
Arm (a) has to be repeatable, so besides the patch it times one clone of the own flags and one copy of the patched flags into the
storage (0.5 MB / 1 MB each at this shape): two small copies a user who patches a fresh horizon once would partly avoid, so (a) / (b)
is slightly flattering to (b); (a) - (c) carries them too."""
import argparse
import json
import math
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from replay_bench import KINDS, once, storage  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gae_bench.py measures on the GPU; there is none")
    from gym_rotor_amd import RolloutStorage, TimeLimitRule
    T, N = args.horizon, args.envs
    dev = torch.device("cuda", torch.cuda.current_device())
    fmt = lambda t: f"{t[0]:.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "gae": []}
    rule = TimeLimitRule()
    for kind, (od, ad) in KINDS.items():
        s = storage(od, ad, T, N, seed=3)
        na = len(od)
        s.done &= torch.rand(T, N, na, device="cuda") < 0.1       # about 3 % per agent and 3 % truncated: episodes of ~15 steps
        s.truncated &= torch.rand(T, N, device="cuda") < 0.1
        s.final_obs[0][:, ::3, :3] *= 0.02     # a third of the envs near the tolerance: both outcomes are dense
        if na > 1:
            s.final_obs[1][:, ::3, 0] *= 0.01
        s.reward[:, ::5] = -1.0
        env = types.SimpleNamespace(kind=kind, num_envs=N, auto_reset=True, obs_rows=True, n_agents=na, obs_dims=list(od), action_dim=sum(ad),
                                    device=dev, x_lim=1.0)
        stores = [RolloutStorage(env, T, action_dims=list(ad)) for _ in range(3)]
        value = torch.randn(T + 1, N, na, device="cuda")
        next_value = torch.randn(T, N, na, device="cuda")
        for st in stores:
            for dst, src in zip(st.final_obs, s.final_obs):
                dst.copy_(src)
            st.reward.copy_(s.reward), st.done.copy_(s.done), st.truncated.copy_(s.truncated), st.value.copy_(value)
        sa, sb, sc = stores
        own_done = sa.done.clone()
        out = {}

        def arm_a():
            eff = own_done.clone()
            for k in range(na):
                nxt = sa.final_obs[k]
                err = nxt[..., :3].double() * rule.x_lim if k == 0 else nxt[..., :1].double() * math.pi
                solved = (err.abs() <= (rule.pos_tol if k == 0 else rule.rot_tol)).all(-1) & (sa.reward[..., k] != -1.0)
                eff[..., k] = torch.where(sa.truncated, solved, own_done[..., k])
            sa.done.copy_(eff)
            adv, _, stats = sa.compute_gae(0.99, 0.9, next_value=next_value)
            out["a"] = (eff, RolloutStorage.normalize(adv, stats))

        def arm_b():
            sb.compute_gae(0.99, 0.9, next_value=next_value, time_limit="solved", normalized=True)
            out["b"] = sb.advantage_normalized

        def arm_c():
            adv, _, stats = sc.compute_gae(0.99, 0.9, next_value=next_value)
            out["c"] = RolloutStorage.normalize(adv, stats)

        arms = (arm_a, arm_b, arm_c)
        for _ in range(3):
            for f in arms:
                f()
        torch.cuda.synchronize()
        ms = ([], [], [])
        for _ in range(args.reps):
            for m, f in zip(ms, arms):
                m.append(once(f))
        a, b, c = [(statistics.median(m), min(m), max(m)) for m in ms]
        sb.compute_gae(0.99, 0.9, next_value=next_value, time_limit="solved", normalized=True, done_eff=True)
        torch.cuda.synchronize()
        same = torch.equal(sa.advantage, sb.advantage) and torch.equal(sa.td_target, sb.td_target) and torch.equal(out["a"][0], sb.done_eff)
        gap = float((out["a"][1] - sb.advantage_normalized).abs().max())
        moved = int((sb.done_eff != own_done).sum())
        ok = b[0] < a[1]
        print(f"{kind} T = {T} N = {N} ({T * N} transitions, {int(sb.truncated.sum())} at the time limit, the rule moved {moved} flags):\n"
              f"  (a) torch patch + compute_gae + normalize                 {fmt(a)}\n"
              f"  (b) compute_gae(time_limit='solved', normalized=True)     {fmt(b)}\n"
              f"  (c) compute_gae + normalize (own flags)                   {fmt(c)}\n"
              f"  median of (b) below (a)'s minimum: {ok} (a / b {a[0] / b[0]:.1f}, c / b {c[0] / b[0]:.1f}; the patch alone costs (a) - (c) = {a[0] - c[0]:.4f} ms)\n"
              f"  advantages, td targets and effective flags of (a) and (b) equal bit for bit: {same}; normalised advantages differ by at most {gap:.3e}",
              flush=True)
        results["gae"].append({"kind": kind, "T": T, "N": N, "torch_ms": a, "rule_ms": b, "own_ms": c, "below_torch_min": bool(ok), "equal": bool(same),
                               "normalized_gap": gap, "flags_moved": moved})
        if not same:
            raise SystemExit("the torch composition and qr_gae_rule left different advantages")
        del s, stores, sa, sb, sc
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
