#!/usr/bin/env python3
"""The critic's values for one PPO horizon: `RolloutStorage.compute_values` (critic_kernel: one launch per critic and mode) against
the path it replaces — the torch module on all T+1 observation rows, then `next_values(module)` (nonzero() gather of the reset
rows, the module on them, scatter) — on the SAME rows, which come from a real `collect`.

    python tools/critic_bench.py [--envs 65536] [--horizon 32] [--reps 20]

HIP events around each path, warm-up, median of --reps.  Prints ONE JSON line: per row (Coupled MONO critic 23->62->62->1;
Decoupled with two CTDE critics 18->62->62->1) both times and their ratio, the share of next-value tiles that held a reset (and
so were evaluated), the worst difference between the two paths, and two yardsticks for the kernel path: its bytes at 8 TB/s, and
its MFMA instructions at 32 clocks each spread over the device's SIMDs (one matrix pipe per SIMD, whatever waves are resident)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gym_rotor_amd import CriticParams, QuadVecEnv, RolloutStorage, random_actors  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--envs", type=int, default=65536)
p.add_argument("--horizon", type=int, default=32)
p.add_argument("--reps", type=int, default=20)
p.add_argument("--warmup", type=int, default=3)
a = p.parse_args()
dev = torch.device("cuda", 0)
HBM_BYTES_PER_S, MFMA_CLOCKS, MFMA_PER_TILE = 8e12, 32, 4 * 4 * 6 + 4 * 4 * 16


class Critic(torch.nn.Module):  # the shape of the reference's MLP_Critic / MLP_Critic_CTDE (attributes fc1, fc2, fc3)
    def __init__(self, din, hidden=62):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(din, hidden), torch.nn.Linear(hidden, hidden), torch.nn.Linear(hidden, 1)

    def forward(self, x):
        return self.fc3(torch.tanh(self.fc2(torch.tanh(self.fc1(x)))))


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms) * 1e3, min(ms) * 1e3


def row(kind, ctde):
    N, T = a.envs, a.horizon
    torch.manual_seed(0)
    env = QuadVecEnv(kind, N, device=dev, auto_reset=True, seed=0)
    env.reset("train")
    env.get_norm_error_state()
    st = RolloutStorage(env, T)
    actors = random_actors(kind, dev, generator=torch.Generator(dev).manual_seed(1), log_std=-0.5)
    for _ in range(3):   # (episodes of every age, not one horizon after a common reset)
        st.collect(env, actors)
    D = [o.shape[-1] for o in st.obs]
    inputs = [(0, 1)] * 2 if ctde else [(k,) for k in range(len(D))]
    mods = [Critic(sum(D[j] for j in i)).to(dev) for i in inputs]
    params = [CriticParams.from_module(m, i) for m, i in zip(mods, inputs)]

    def module(rows):   # per-agent rows [n, D_k] -> [n, n_agents]
        with torch.no_grad():
            return torch.cat([m(torch.cat([rows[j] for j in i], 1) if len(i) > 1 else rows[i[0]]) for m, i in zip(mods, inputs)], 1)

    out = {}

    def kernel_path():
        out["kernel"] = st.compute_values(params)

    def torch_path():
        st.value.copy_(module([o.reshape((T + 1) * N, -1) for o in st.obs]).reshape(T + 1, N, st.n_agents))
        out["torch"] = st.next_values(module)

    t_torch = timed(torch_path)
    v_torch = st.value.clone()
    t_kernel = timed(kernel_path)
    diff = max(float((st.value - v_torch).abs().max()), float((out["kernel"] - out["torch"]).abs().max()))

    mask = st.reset_mask().reshape(-1)
    pad = (-mask.numel()) % 64
    tiles_next = (mask.numel() + pad) // 64
    hit = int(torch.nn.functional.pad(mask, (0, pad)).view(-1, 64).any(1).sum())
    tiles_values = ((T + 1) * N + 63) // 64
    din = params[0].dims[0]
    n_crit = len(params)
    rows_read = (T + 1) * N + 64 * hit
    bytes_moved = n_crit * (rows_read * din * 4 + (T + 1) * N * 4 + T * N * (st.n_agents + 1 + 4 + 4))
    prop = torch.cuda.get_device_properties(dev)
    khz = getattr(prop, "clock_rate", 2400000)
    simds, hz = prop.multi_processor_count * 4, khz * 1e3
    mfma = n_crit * (tiles_values + hit) * MFMA_PER_TILE
    return {"kind": kind, "critics": [f"{c.dims[0]}->{c.dims[1]}->{c.dims[1]}->1" for c in params], "envs": N, "horizon": T,
            "compute_values_us": round(t_kernel[0], 1), "compute_values_us_min": round(t_kernel[1], 1),
            "torch_module_us": round(t_torch[0], 1), "torch_module_us_min": round(t_torch[1], 1),
            "torch_over_kernel": round(t_torch[0] / t_kernel[0], 2),
            "reset_share": round(float(mask.float().mean()), 5), "next_value_tiles": tiles_next, "next_value_tiles_evaluated": hit,
            "next_value_tiles_evaluated_share": round(hit / tiles_next, 4),
            "max_abs_diff_between_paths": diff,
            "yardstick_bytes_us": round(bytes_moved / HBM_BYTES_PER_S * 1e6, 1),
            "yardstick_mfma_us": round(mfma * MFMA_CLOCKS / simds / hz * 1e6, 1), "mfma_instructions": mfma, "simds": simds,
            "clock_mhz": khz / 1e3}


print(json.dumps({"workload": "critic values of one PPO horizon: compute_values against torch module + next_values(module)",
                  "reps": a.reps, "rows": [row("coupled", False), row("decoupled", True)]}))
