#!/usr/bin/env python3
"""What the library's noise source (qr_noise_fill, noise_source="device") is worth to a TD3 / SAC iteration on one MI355X: HIP events,
median of 20 with min .. max, the two arms alternated call by call in one process:

  (a) noise_source="torch": one `normal_` launch per noise tensor (the parent's path);
  (b) noise_source="device": ONE `noise_fill` launch per agent.

    python tools/noise_bench.py [--out FILE]

TD3 single and SAC ctde, B = 256 and 65 536, `update(buffer, 1)` and one `capture` replay, policy_update_freq = 1.  The kernel launches
of one eager iteration are counted with torch.profiler (all launches, and those that draw noise).  Last, the fill of one
[2 097 152, 4] tensor against `normal_` and against the time its 32 MB take at a given write rate (--write-gbs, the rate
profiles/r24/replay_bench.txt reached).  Nothing is asserted; the table goes to stdout and to --out."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gym_rotor_amd as G  # noqa: E402
from offpolicy_update_bench import setup, timed  # noqa: E402


def make_updater(algo, mode, mods, B, source):
    actors, critics, actors_t, critics_t, nominal = mods
    kw = dict(mode=mode, policy_update_freq=1, batch_size=B, nominal=nominal, noise_source=source, noise_seed=11)
    if algo == "td3":
        return G.Td3Updater(actors, critics, actors_t, critics_t, **kw)
    return G.SacUpdater(actors, critics, critics_t, automatic_entropy_tuning=True, **kw)


def count_launches(fn):
    """(all kernel launches, those that draw noise) of one call, from torch.profiler's device events; None where it gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    except Exception as exc:   # (a build of torch without the tracer)
        print(f"# launch count unavailable: {exc!r}")
        return None
    noise = [n for n in names if "noise_fill" in n or "normal" in n.lower() or "distribution" in n.lower()]
    return (len(names), len(noise)) if names else None


def stats(v):
    return f"{statistics.median(v):8.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--write-gbs", type=float, default=None, help="HBM write rate to price the 32 MB fill against")
    args = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}; one iteration (all agents), us: median of 20 (min .. max); arms alternated call by call",
             "# (a) noise_source='torch'  (b) noise_source='device'; launches: all kernels of one eager iteration / those that draw noise"]
    misses = []
    for algo, mode in (("td3", "single"), ("sac", "ctde")):
        for B in (256, 65536):
            ups, bufs = {}, {}
            for arm, source in (("a", "torch"), ("b", "device")):
                bufs[arm], mods = setup(algo, mode, B)
                ups[arm] = make_updater(algo, mode, mods, B, source)
                ups[arm].update(bufs[arm], 1)
            counts = {arm: count_launches(lambda arm=arm: ups[arm].update(bufs[arm], 1)) for arm in ups}
            eager = {arm: (lambda arm=arm: ups[arm].update(bufs[arm], 1)) for arm in ups}
            graph = {arm: ups[arm].capture(bufs[arm]) for arm in ups}
            for what, arms in (("update ", eager), ("replay ", graph)):
                for fn in arms.values():
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                t = {k: [] for k in arms}
                for _ in range(20):
                    for k, fn in arms.items():
                        t[k].append(timed(fn))
                ok = statistics.median(t["b"]) <= max(t["a"])
                if not ok:
                    misses.append(f"{algo} {mode} B={B} {what.strip()}")
                cnt = "  ".join(f"({k}) launches {c[0]} / {c[1]}" if c else f"({k}) launches n/a" for k, c in counts.items()) if what == "update " else ""
                lines.append(f"{algo} {mode:6s} B={B:6d} {what} (a) {stats(t['a'])}  (b) {stats(t['b'])}  b.median <= a.max: {'yes' if ok else 'NO'}  {cnt}")
                print(lines[-1], flush=True)
    lines.append("condition (b's median does not exceed a's max) " + ("holds at every point" if not misses else "MISSED at: " + "; ".join(misses)))
    print(lines[-1], flush=True)

    big = torch.empty(2_097_152, 4, device="cuda")
    arms = {"normal_": lambda: big.normal_(), "noise_fill normal": lambda: G.noise_fill([big], seed=1, draw=0, streams=[0]),
            "noise_fill uniform": lambda: G.noise_fill([big], seed=1, draw=0, streams=[0], kind="uniform"), "zero_ (write only)": lambda: big.zero_()}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(20):
        for k, fn in arms.items():
            t[k].append(timed(fn))
    mb = big.numel() * 4 / 1e6
    for k, v in t.items():
        lines.append(f"[2097152, 4] float32 ({mb:.1f} MB) {k:20s} {stats(v)} us  = {mb / 1e3 / (statistics.median(v) * 1e-6):7.0f} GB/s written")
        print(lines[-1], flush=True)
    if args.write_gbs:
        lines.append(f"the same bytes at {args.write_gbs:.0f} GB/s: {mb / 1e3 / args.write_gbs * 1e6:.1f} us")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
