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


def _prepare_episodes(kind, num_envs, traj_mode, seed, **env_kw):
    """(env, obs): `num_envs` evaluation episodes at their start as eval_policy prepares them (main.py:305-309) — reset(env_type=
    'eval', seed), with a fused generator mark_traj_start + the first get_desired(store_goal=True), the first observation."""
    env = QuadVecEnv(kind, int(num_envs), seed=seed, goal_mode=traj_mode, autotune=False, **env_kw)
    env.reset("eval", seed=seed)
    if traj_mode is not None:
        env.get_desired(store_goal=True)
    return env, env.get_norm_error_state()


def _tile_episodes(src: QuadVecEnv, src_obs, env: QuadVecEnv, P: int, obs: Optional[list] = None) -> list:
    """Copy the prepared episodes of `src` (E envs: state, parameters, integrators, goal, generator state, episode index) into every
    one of the P policies' blocks of `env` (P * Epad envs); returns `src_obs` tiled the same way, zeros in the padding rows.
    `obs`: the rows an earlier call returned for the same `src_obs` — they are returned as they are and nothing is allocated."""
    from .policy import population_tile
    E = src.num_envs
    if src._goal is not None:   # (the goal buffer of a stateless generator mode exists from get_desired(store_goal=True) on)
        env._ensure_goal()
    for name in ("_pos_vel", "_att_rate", "_integ", "_params", "_goal", "_traj"):   # SoA [fields, N]
        if getattr(src, name) is not None:
            population_tile(getattr(src, name), P, E, getattr(env, name), env_dim=1)
    population_tile(src._episode, P, E, env._episode)
    if obs is not None:
        return obs
    return [population_tile(o, P, E, torch.zeros(env.num_envs, o.shape[1], dtype=o.dtype, device=o.device)) for o in src_obs]


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
    env, obs = _prepare_episodes(kind, num_episodes, traj_mode, seed, device=device, substeps=substeps, layout=layout, env_offset=env_offset)
    out = env.evaluate(actors, max_steps=int(round(eval_seconds / env.dt)), obs=obs, max_action=max_action)
    return EvalResult.from_dict(out)


@dataclass
class PopulationResult:
    """Per-episode results of a population evaluation.  `flat` holds the per-env tensors of `QuadVecEnv.evaluate_population`
    ([N, ...], N = P * Epad, padding rows included); the attributes below are their [P, E, ...] VIEWS with the padding sliced
    off.  `result[p]` is the `EvalResult` of policy p."""
    flat: dict
    n_policies: int
    envs_per_policy: int

    def _view(self, key):
        from .policy import population_view
        t = self.flat.get(key)
        return None if t is None else population_view(t, self.n_policies, self.envs_per_policy)

    episode_return = property(lambda self: self._view("episode_return"))   # [P, E, n_agents] float64
    benchmark = property(lambda self: self._view("benchmark"))             # [P, E] float64
    length = property(lambda self: self._view("length"))                   # [P, E] int32
    terminated = property(lambda self: self._view("terminated"))           # [P, E] bool
    success = property(lambda self: self._view("success"))                 # [P, E, n_agents] bool
    final_error = property(lambda self: self._view("final_error"))         # [P, E, 4] float32

    def __len__(self) -> int:
        return self.n_policies

    def __getitem__(self, p: int) -> EvalResult:
        fe = self.final_error
        return EvalResult(self.episode_return[p], self.benchmark[p], self.length[p], self.terminated[p], self.success[p],
                          None if fe is None else fe[p])

    def per_policy(self) -> dict:
        """The means over each policy's E episodes (float64, unrounded; one [P, E] torch reduction each): episode_return
        [P, n_agents] (summary()'s eval_reward), benchmark [P] (benchmark_reward), success [P, n_agents] (success_rate), length [P]
        (mean_length), terminated [P] (terminated_fraction)."""
        return {"episode_return": self.episode_return.double().mean(1), "benchmark": self.benchmark.double().mean(1),
                "success": self.success.double().mean(1), "length": self.length.double().mean(1),
                "terminated": self.terminated.double().mean(1)}

    def best(self, key: str = "benchmark") -> int:
        """Index of the policy with the largest per_policy()[key] (summed over the agents where there are two; the first one on
        a tie)."""
        v = self.per_policy()[key]
        if v.dim() > 1:
            v = v.sum(1)
        return int(torch.argmax(v))


def evaluate_population(kind: str, population, episodes_per_policy: int, traj_mode: Optional[int] = 0, seed: int = 1992,
                        eval_seconds: float = 5.0, common_episodes: bool = True, device="cuda", substeps: int = 1,
                        layout: str = "mixed", env_offset: int = 0, max_action: float = 1.0) -> PopulationResult:
    """`evaluate_policy` for the P policies of a `policy.ActorPopulation` in ONE launch (`QuadVecEnv.evaluate_population`): policy
    p flies E = `episodes_per_policy` episodes on its own block of an env of P * roundup(E, 64) envs.

    common_episodes=True (common random numbers): the E episodes are prepared ONCE on an E-env env exactly as evaluate_policy
    prepares them — reset(env_type='eval', seed), mark_traj_start + get_desired(store_goal=True) with a fused generator, the first
    observation — and that state (state, parameters, integrators, goal, generator state, observation rows) is copied into every
    policy's block.  Policy p's results are then those of evaluate_policy(kind, population[p], E, ...), episode by episode, and
    two policies are compared on the same episodes: a paired comparison.
    common_episodes=False: the big env is reset as a whole, so every episode of every policy has its own draws.

    Sharding is by slicing the population: each rank evaluates `population.select(slice)` (with the same seed and, for common
    episodes, the same env_offset) and keeps its own PopulationResult; there is nothing to reduce across ranks until the caller
    compares per_policy() figures."""
    from .policy import population_layout
    if kind == "quad":
        raise ValueError("evaluate_population needs kind 'coupled' or 'decoupled' (Quad-v0 has no actor)")
    P, E = len(population), int(episodes_per_policy)
    _, n = population_layout(P, E)
    env_kw = dict(device=device, substeps=substeps, layout=layout, env_offset=env_offset)
    if common_episodes:
        src, src_obs = _prepare_episodes(kind, E, traj_mode, seed, **env_kw)
        env = QuadVecEnv(kind, n, seed=seed, goal_mode=traj_mode, autotune=False, **env_kw)
        obs = _tile_episodes(src, src_obs, env, P)
    else:
        env, obs = _prepare_episodes(kind, n, traj_mode, seed, **env_kw)
    out = env.evaluate_population(population, E, max_steps=int(round(eval_seconds / env.dt)), obs=obs, max_action=max_action)
    return PopulationResult(out, P, E)
