#!/usr/bin/env python
"""The data side of a TD3 / SAC iteration: `ReplayBuffer.sample_index` (qr_replay_sample) against `ReplayBuffer.sample` (torch.randperm of
the whole buffer), and `ReplayBuffer.append` (qr_replay_add, one launch) against `ReplayBuffer.add` (torch copies), alternated call by call
in one process.

    python tools/replay_bench.py [--capacity 1000000] [--batches 256 65536] [--horizon 32] [--envs 16384] [--reps 20] [--json PATH]

HIP events around one call, median of --reps with min .. max.  The append's bandwidth is the bytes it must move (each source word read once,
each buffer word written once, the flag bytes once) over its time, as a share of 8 TB/s.  After the timing the appended buffers are compared
bit for bit at the timed shape."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KINDS = {"coupled": ((23,), (4,)), "decoupled": ((15, 3), (4, 1))}
PEAK = 8.0e12   # bytes / s, the figure the README prices bandwidth against


def storage(obs_dims, action_dims, T, N, seed):
    """What add / append read of a RolloutStorage, filled directly: about 30 % of done and truncated set."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    na = len(obs_dims)
    s = types.SimpleNamespace(T=T, N=N, n_agents=na, action_dims=list(action_dims))
    s.obs = [torch.randn(T + 1, N, d, device="cuda", generator=g) for d in obs_dims]
    s.final_obs = [torch.randn(T, N, d, device="cuda", generator=g) for d in obs_dims]
    s.act_all = torch.randn(T, N, sum(action_dims), device="cuda", generator=g)
    s.act = list(torch.split(s.act_all, list(action_dims), dim=-1))
    s.reward = torch.randn(T, N, na, device="cuda", generator=g)
    s.done = torch.rand(T, N, na, device="cuda", generator=g) < 0.3
    s.truncated = torch.rand(T, N, device="cuda", generator=g) < 0.3
    s.reset_mask = lambda: s.done.any(-1) | s.truncated
    return s


def append_bytes(obs_dims, action_dims, n):
    words = sum(2 * d + a + 1 for d, a in zip(obs_dims, action_dims))     # read: obs, one of obs[t + 1] / final_obs, act, rwd
    flags = len(obs_dims) + 1                                             # done per agent and truncated, one byte each
    written = sum(2 * d + a + 2 for d, a in zip(obs_dims, action_dims))   # obs, obs_next, act, rwd, done
    return n * (4 * words + flags + 4 * written)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(new, old, reps):
    """[(median, min, max)] of new and old in ms, one call of each per repetition, after three warm-up rounds."""
    for _ in range(3):
        new(), old()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        ms[0].append(once(new))
        ms[1].append(once(old))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 65536])
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("replay_bench.py measures on the GPU; there is none")
    from gym_rotor_amd import ReplayBuffer
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "sample": [], "append": []}
    fmt = lambda t: f"{t[0]:.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"

    buf = ReplayBuffer(args.capacity, [1], [1], "cuda", seed=1)   # the sampler reads the fill level alone
    buf.count, buf.current_size = 0, args.capacity
    for B in args.batches:
        out = torch.empty(B, dtype=torch.int64, device="cuda")
        new, old = alternate(lambda: buf.sample_index(B, out=out), lambda: buf.sample(B), args.reps)
        distinct = int(torch.unique(out).numel())
        print(f"sample  n = {args.capacity} B = {B}: sample_index {fmt(new)}; sample (randperm) {fmt(old)}; ratio {old[0] / new[0]:.1f}; "
              f"distinct {distinct} of {B}, max {int(out.max())}", flush=True)
        results["sample"].append({"n": args.capacity, "B": B, "sample_index_ms": new, "sample_ms": old, "distinct": distinct})
    del buf

    T, N = args.horizon, args.envs
    n = T * N
    start = args.capacity - n // 2   # the append wraps in its middle
    for kind, (od, ad) in KINDS.items():
        s = storage(od, ad, T, N, seed=3)
        got, want = ReplayBuffer(args.capacity, od, ad, "cuda"), ReplayBuffer(args.capacity, od, ad, "cuda")

        def run(b, method):
            b.count, b.current_size = start, args.capacity
            method(s)

        new, old = alternate(lambda: run(got, got.append), lambda: run(want, want.add), args.reps)
        torch.cuda.synchronize()
        same = all(torch.equal(got.tensors(k)[name].view(torch.int32), t.view(torch.int32)) for k in range(got.n_agents)
                   for name, t in want.tensors(k).items())
        nbytes = append_bytes(od, ad, n)
        gbs = nbytes / (new[0] * 1e-3) / 1e9
        print(f"append  {kind} T = {T} N = {N} ({n} transitions, {nbytes / 1e6:.1f} MB to move) at count {start} of {args.capacity}: "
              f"append {fmt(new)}; add {fmt(old)}; ratio {old[0] / new[0]:.2f}; append {gbs:.0f} GB/s = {100 * gbs * 1e9 / PEAK:.1f} % of 8 TB/s; "
              f"add {nbytes / (old[0] * 1e-3) / 1e9:.0f} GB/s of the same bytes; buffers equal bit for bit: {same}", flush=True)
        results["append"].append({"kind": kind, "T": T, "N": N, "bytes": nbytes, "append_ms": new, "add_ms": old, "append_GBps": gbs,
                                  "share_of_8TBps": gbs * 1e9 / PEAK, "equal": bool(same)})
        if not same:
            raise SystemExit("append and add left different buffers")
        del got, want, s
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
