"""Batched policy evaluation: the reference's `Learner.eval_policy` (main.py:270-404) as one launch.

The reference evaluates `--num_eval` (10) episodes one after the other on a fresh eval env: per episode the deterministic actor
flies from `reset(env_type='eval')` until the first `any(done_n)` or `eval_max_steps` (5 s), and it reports the mean episode reward
per agent, the mean benchmark reward (utils/utils.py:42-47) and per-agent success flags (main.py:366-373).  Here every episode is an
env of one QuadVecEnv and all of them run in ONE qr_evaluate_actor launch (`QuadVecEnv.evaluate`): thousands of evaluation
episodes for about the cost of one collection launch, which turns the reference's 10-episode model-selection signal into a
measurement.

    res = evaluate_policy("decoupled", actors, num_episodes=4096, traj_mode=1)
    res.summary()   # {"eval_reward": [..], "benchmark_reward": .., "success_rate": [..], "mean_length": .., "terminated_fraction": ..}
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from .vec_env import QuadVecEnv


@dataclass
class EvalResult:
    """Per-episode results of an evaluation (the tensors `QuadVecEnv.evaluate` returns)."""
    episode_return: torch.Tensor   # [N, n_agents] float64
    benchmark: torch.Tensor        # [N] float64
    length: torch.Tensor           # [N] int32
    terminated: torch.Tensor       # [N] bool
    success: torch.Tensor          # [N, n_agents] bool
    final_error: Optional[torch.Tensor] = None   # [N, 4] float32

    @classmethod
    def from_dict(cls, d: dict) -> "EvalResult":
        return cls(d["episode_return"], d["benchmark"], d["length"], d["terminated"], d["success"], d.get("final_error"))

    def sums(self) -> torch.Tensor:
        """float64 [2 n_agents + 4]: sum of the returns per agent, of the benchmark, of the lengths, the number of terminated
        episodes, the number of episodes, then the success counts per agent — what summary() needs, and what a sharded
        evaluation all-reduces."""
        parts = [self.episode_return.double().sum(0), self.benchmark.double().sum().reshape(1), self.length.double().sum().reshape(1),
                 self.terminated.double().sum().reshape(1), torch.tensor([float(self.length.numel())], dtype=torch.float64,
                                                                         device=self.length.device),
                 self.success.double().sum(0)]
        return torch.cat(parts)

    def summary(self, group=None) -> dict:
        """eval_policy's figures over these episodes: `eval_reward` (mean episode reward per agent) and `benchmark_reward` (mean
        benchmark reward), rounded to 4 decimals as main.py:392-393 prints them, plus the success rate per agent, the mean
        length and the fraction of episodes that ended by done.  When torch.distributed is initialised the sums are all-reduced
        over `group` first (like RolloutStorage.normalize), so every rank of a sharded evaluation gets the global figures."""
        import torch.distributed as dist
        s = self.sums()
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(s, group=group)
        s = s.cpu().tolist()
        g = self.episode_return.shape[1]
        n = s[g + 3]
        return {"eval_reward": [round(s[k] / n, 4) for k in range(g)],
                "benchmark_reward": round(s[g] / n, 4),
                "success_rate": [s[g + 4 + k] / n for k in range(g)],
                "mean_length": s[g + 1] / n,
                "terminated_fraction": s[g + 2] / n,
                "episodes": int(n)}


def evaluate_policy(kind: str, actors: Sequence, num_episodes: int, traj_mode: Optional[int] = 0, seed: int = 1992,
                    eval_seconds: float = 5.0, device="cuda", substeps: int = 1, layout: str = "mixed", env_offset: int = 0,
                    max_action: float = 1.0) -> EvalResult:
    """eval_policy in one call: a QuadVecEnv of `num_episodes` envs with the trajectory generator of `traj_mode` fused into the
    step, reset(env_type='eval', seed) (the reference's fixed eval seed 1992), mark_traj_start + the first get_desired and the
    first observation (main.py:305-309), then every episode in one `evaluate` launch of round(eval_seconds / dt) steps at most.
    `actors`: one `policy.ActorParams` per agent (coupled: 1, decoupled: 2).  `env_offset`: the global id of this shard's first
    episode (shard_range), so that a sharded evaluation draws the same episodes as a single-device one."""
    if kind == "quad":
        raise ValueError("evaluate_policy needs kind 'coupled' or 'decoupled' (Quad-v0 has no actor)")
    env = QuadVecEnv(kind, int(num_episodes), device=device, seed=seed, substeps=substeps, layout=layout, goal_mode=traj_mode,
                     env_offset=env_offset, autotune=False)
    env.reset("eval", seed=seed)
    if traj_mode is not None:
        env.get_desired(store_goal=True)
    obs = env.get_norm_error_state()
    out = env.evaluate(actors, max_steps=int(round(eval_seconds / env.dt)), obs=obs, max_action=max_action)
    return EvalResult.from_dict(out)
