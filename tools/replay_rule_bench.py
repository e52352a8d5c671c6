#!/usr/bin/env python
"""What the time-limit "solved" done rule costs inside the append launch: three arms alternated call by call in one process,
    (a) `ReplayBuffer.append` followed by the torch patch of `done` a user had to write before (time-limit rows -> solved and not crashed),
    (b) `ReplayBuffer.append(storage, time_limit="solved")` (qr_replay_add_rule, one launch),
    (c) `ReplayBuffer.append(storage)` (qr_replay_add), the floor,
at tools/replay_bench.py's append shapes.

    python tools/replay_rule_bench.py [--capacity 1000000] [--horizon 32] [--envs 16384] [--reps 20] [--json PATH]

HIP events around one call, median of --reps with min .. max.  Two conditions are printed with their numbers: (b) is not slower than (a);
(b) lies within (c)'s min .. max plus the time of the bytes the rule reads on top (truncated, reward and 3 + 1 observation words per
transition) at the bandwidth the plain append reached (--gbps, by default the figures of profiles/r24/replay_bench.txt).  After the
timing, (a) and (b) are compared bit for bit."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from replay_bench import KINDS, once, storage  # noqa: E402

APPEND_GBPS = {"coupled": 2659.0, "decoupled": 2248.0}   # profiles/r24/replay_bench.txt


def rule_bytes(obs_dims, n):
    """What the done segment reads on top, per transition and agent: the truncated byte, the reward word, and ex (3 words) or eb1 (1)."""
    return n * sum(1 + 4 + 4 * (3 if k == 0 else 1) for k in range(len(obs_dims)))


def patch_done(buf, s, start, rule):
    """The rule in torch on the rows an append just wrote: what a caller of the plain append had to add."""
    n = s.T * s.N
    lim = s.truncated.reshape(n)
    first = min(n, buf.capacity - start)
    for k in range(buf.n_agents):
        fin = s.final_obs[k].reshape(n, -1)      # (a time-limit row was re-sampled: its obs_next is final_obs)
        err = fin[:, :3].double() * rule.x_lim if k == 0 else fin[:, :1].double() * math.pi
        solved = (err.abs() <= (rule.pos_tol if k == 0 else rule.rot_tol)).all(-1) & (s.reward[..., k].reshape(n) != -1.0)
        done = torch.where(lim, solved, s.done[..., k].reshape(n)).to(torch.float32)
        buf.done[k][start:start + first].copy_(done[:first])
        if n > first:
            buf.done[k][:n - first].copy_(done[first:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gbps", type=float, nargs=2, default=None, metavar=("COUPLED", "DECOUPLED"))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("replay_rule_bench.py measures on the GPU; there is none")
    from gym_rotor_amd import ReplayBuffer
    gbps = dict(zip(KINDS, args.gbps)) if args.gbps else APPEND_GBPS
    T, N = args.horizon, args.envs
    n = T * N
    start = args.capacity - n // 2   # the append wraps in its middle
    fmt = lambda t: f"{t[0]:.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "append": []}
    for kind, (od, ad) in KINDS.items():
        s = storage(od, ad, T, N, seed=3)
        s.final_obs[0][:, ::3, :3] *= 0.02     # a third of the envs near the tolerance: both outcomes are dense
        if len(od) > 1:
            s.final_obs[1][:, ::3, 0] *= 0.01
        s.reward[:, ::5] = -1.0
        bufs = [ReplayBuffer(args.capacity, od, ad, "cuda") for _ in range(3)]
        rule = bufs[0].time_limit_rule

        def place(b):
            b.count, b.current_size = start, args.capacity

        def arm_a():
            place(bufs[0])
            bufs[0].append(s)
            patch_done(bufs[0], s, start, rule)

        def arm_b():
            place(bufs[1])
            bufs[1].append(s, time_limit="solved")

        def arm_c():
            place(bufs[2])
            bufs[2].append(s)

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
        torch.cuda.synchronize()
        same = all(torch.equal(bufs[0].tensors(k)[name].view(torch.int32), t.view(torch.int32)) for k in range(bufs[1].n_agents)
                   for name, t in bufs[1].tensors(k).items())
        changed = sum(int((bufs[1].done[k] != bufs[2].done[k]).sum()) for k in range(len(od)))
        extra = rule_bytes(od, n)
        extra_ms = extra / (gbps[kind] * 1e9) * 1e3
        ok_a, ok_c = b[0] <= a[0], b[0] <= c[2] + extra_ms
        print(f"{kind} T = {T} N = {N} ({n} transitions) at count {start} of {args.capacity}:\n"
              f"  (a) append + torch patch of done  {fmt(a)}\n  (b) append(time_limit='solved')     {fmt(b)}\n  (c) append                          {fmt(c)}\n"
              f"  (b) not slower than (a): {ok_a} (ratio a / b {a[0] / b[0]:.2f});  the rule reads {extra / 1e6:.1f} MB on top = {extra_ms:.4f} ms at "
              f"{gbps[kind]:.0f} GB/s, so the bound is (c)'s max + that = {c[2] + extra_ms:.4f} ms: (b) within it: {ok_c} (b - c medians "
              f"{1e3 * (b[0] - c[0]):+.1f} us)\n  (a) and (b) left equal buffers bit for bit: {same}; done rows the rule changed: {changed}", flush=True)
        results["append"].append({"kind": kind, "T": T, "N": N, "patch_ms": a, "rule_ms": b, "plain_ms": c, "extra_bytes": extra, "extra_ms": extra_ms,
                                  "not_slower_than_patch": bool(ok_a), "within_floor_plus_extra": bool(ok_c), "equal": bool(same), "changed": changed})
        if not same:
            raise SystemExit("the patched append and append(time_limit='solved') left different buffers")
        del bufs, s
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
