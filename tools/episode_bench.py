#!/usr/bin/env python
"""What the training curve costs per collected horizon: three arms alternated call by call in one process,
    (a) `EpisodeTracker.update_torch` — the loop over t of torch ops a user had to write before,
    (b) `EpisodeTracker.update` without dense outputs (qr_episode_scan: two launches behind one C call),
    (c) `EpisodeTracker.update` with the four dense outputs,
at tools/replay_bench.py's append shape (T = 32, N = 16 384), Coupled and Decoupled.

    python tools/episode_bench.py [--horizon 32] [--envs 16384] [--reps 20] [--json PATH]

HIP events around one call, median of --reps with min .. max.  Condition, printed with its numbers: the medians of (b) and (c) lie
below (a)'s minimum.  (b) is also set against the time its bytes — reward, done and truncated over T x N, the carries read and
written — would take at the bandwidth the replay append reached (--gbps, by default the figures of profiles/r24/replay_bench.txt).
After the timing the three trackers, which saw the same horizons, are compared."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from replay_bench import KINDS, once, storage  # noqa: E402

APPEND_GBPS = {"coupled": 2659.0, "decoupled": 2248.0}   # profiles/r24/replay_bench.txt


def scan_bytes(na, T, N):
    """What (b) has to move: reward (4 na), done (na) and truncated (1) per transition; the carries (8 na + 4 per env) in and out."""
    return T * N * (4 * na + na + 1) + 2 * N * (8 * na + 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gbps", type=float, nargs=2, default=None, metavar=("COUPLED", "DECOUPLED"))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("episode_bench.py measures on the GPU; there is none")
    from gym_rotor_amd import EpisodeTracker
    from gym_rotor_amd import _lib
    gbps = dict(zip(KINDS, args.gbps)) if args.gbps else APPEND_GBPS
    T, N = args.horizon, args.envs
    fmt = lambda t: f"{t[0]:.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "scan": []}
    for kind, (od, ad) in KINDS.items():
        s = storage(od, ad, T, N, seed=3)
        s.device = torch.device("cuda", torch.cuda.current_device())
        s.done &= torch.rand(T, N, len(od), device="cuda") < 0.1       # about 3 % per agent and 3 % truncated: episodes of ~15 steps
        s.truncated &= torch.rand(T, N, device="cuda") < 0.1
        s.final_obs[0][:, ::3, :3] *= 0.02     # a third of the envs near the tolerance: both outcomes are dense
        if len(od) > 1:
            s.final_obs[1][:, ::3, 0] *= 0.01
        s.reward[:, ::5] = -1.0
        twin, plain, dense = EpisodeTracker(s, dense=True), EpisodeTracker(s), EpisodeTracker(s, dense=True)
        arms = (lambda: twin.update_torch(s), lambda: plain.update(s), lambda: dense.update(s))
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
        same = all(torch.equal(getattr(twin, n), getattr(dense, n)) for n in ("run_return", "run_length", "ep_return", "ep_length", "ep_flags", "ep_final_error"))
        same = same and torch.equal(plain.run_return, dense.run_return) and torch.equal(plain.total, dense.total)
        count = float(dense.last[_lib.EP_COUNT])
        close = bool(torch.allclose(twin.total, dense.total, rtol=1e-12, atol=0.0))
        nbytes = scan_bytes(len(od), T, N)
        floor_ms = nbytes / (gbps[kind] * 1e9) * 1e3
        ok = b[0] < a[1] and c[0] < a[1]
        print(f"{kind} T = {T} N = {N} ({T * N} transitions, {int(count)} episodes ended in the last horizon):\n"
              f"  (a) update_torch                 {fmt(a)}\n  (b) update                       {fmt(b)}\n  (c) update, dense outputs        {fmt(c)}\n"
              f"  medians of (b) and (c) below (a)'s minimum: {ok} (a / b {a[0] / b[0]:.1f}, a / c {a[0] / c[0]:.1f})\n"
              f"  (b) moves {nbytes / 1e6:.2f} MB = {floor_ms:.4f} ms at {gbps[kind]:.0f} GB/s (the append's bandwidth): (b) is {b[0] / floor_ms:.1f} times that "
              f"({nbytes / b[0] / 1e6:.0f} GB/s)\n"
              f"  carries and dense rows of (a) and (c), carries and totals of (b) and (c) equal bit for bit: {same}; totals of (a) and (c) within 1e-12: {close}",
              flush=True)
        results["scan"].append({"kind": kind, "T": T, "N": N, "torch_ms": a, "scan_ms": b, "dense_ms": c, "bytes": nbytes, "floor_ms": floor_ms,
                                "below_torch_min": bool(ok), "equal": bool(same), "totals_close": close, "episodes": count})
        if not same:
            raise SystemExit("update_torch and update left different carries or dense rows")
        del s, twin, plain, dense
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
