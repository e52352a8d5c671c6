"""The collection half of the reference's PPO loop (main.py:140-181 up to `PPO.train`'s advantages, ppo.py:128-147) as one host
object: `PpoCollector`, the PPO counterpart of `offpolicy.OffPolicyCollector`.  It owns a `RolloutStorage` and — on request — an
`EpisodeTracker`, and `collect` chains the launches the library already has: one horizon with the actors inside the step kernel
(qr_rollout_actor), the critics over it (qr_critic_values, qr_critic_next_values), and the advantages over the done flag the
reference stores at the time limit, with their statistics and their normalisation (qr_gae_rule).  Its output feeds
`PpoUpdater.update(storage, advantage)` as it is.
"""
from __future__ import annotations

from typing import Optional

from .episodes import EpisodeTracker
from .rollout import RolloutStorage
from .td3 import TIME_LIMITS, TimeLimitRule


class PpoCollector:
    """One horizon of T env-steps per `collect` call: a host object with no kernel of its own.

    env: a Coupled or Decoupled `QuadVecEnv` with auto_reset=True (and max_episode_steps set, or no transition is ever at the time
    limit).  gamma, lam: ppo.py's discount and GAE lambda.  time_limit: "solved" — the default, the reference's: at the time limit the
    done flag PPO reads is main.py:169-173's "solved and not crashed" — or "own", each agent's own flag, what a bare
    `compute_gae()` uses.  rule: the `TimeLimitRule`; None: the reference's tolerances with the env's x_lim.
    track_episodes=True: the collector owns `episodes`, an `EpisodeTracker` with the same rule, and every `collect` ends with
    `episodes.update(storage)`; False: `episodes` is None.

    `collect(actors, critics)` returns (storage, normalised advantages [T, N, n_agents]) and synchronises nothing.  On one rank the
    advantages are `storage.advantage_normalized`, written by the same C call that computed them.  When torch.distributed is
    initialised the statistics have to be summed over the ranks first: the call then leaves the normalisation out and the collector
    returns `RolloutStorage.normalize(advantage, stats)`, the all-reduced path (3 doubles per agent)."""

    def __init__(self, env, horizon: int, *, gamma: float = 0.99, lam: float = 0.9, time_limit: str = "solved",
                 rule: Optional[TimeLimitRule] = None, track_episodes: bool = False):
        what = "PpoCollector"
        if time_limit not in TIME_LIMITS:
            raise ValueError(f"{what}: time_limit must be one of {TIME_LIMITS}, got {time_limit!r}")
        self.T = int(horizon)
        if self.T < 1:
            raise ValueError(f"{what}: horizon must be >= 1")
        self.gamma, self.lam = float(gamma), float(lam)
        if not (0.0 <= self.gamma < float("inf") and 0.0 <= self.lam < float("inf")):
            raise ValueError(f"{what}: gamma and lam must be finite and >= 0, got {gamma}, {lam}")
        if not getattr(env, "auto_reset", False):
            raise ValueError(f"{what} needs an env with auto_reset=True: a horizon runs through episode ends")
        if env.n_agents not in (1, 2):
            raise ValueError(f"{what}: one or two agents, got {env.n_agents}")
        if time_limit == "solved" and env.obs_dims[0] < 3:
            raise ValueError(f"{what}: time_limit='solved' reads ex, the first three words of agent 0's observation")
        if rule is None:
            rule = TimeLimitRule(x_lim=float(env.x_lim))
        self.rule = TimeLimitRule(*rule).check(what)
        self.env, self.time_limit = env, time_limit
        self.storage = RolloutStorage(env, self.T)
        self.episodes = EpisodeTracker(self.storage, rule=self.rule) if track_episodes else None

    def collect(self, actors, critics, **kw):
        """One horizon into `storage`, its values, its advantages.  actors: one `ActorParams` per agent; critics: one `CriticParams`
        per agent; kw goes to `RolloutStorage.collect` (noise, noise_seed, max_action).  Returns (storage, normalised advantages)."""
        import torch.distributed as dist
        st = self.storage
        st.collect(self.env, actors, **kw)
        next_value = st.compute_values(critics)
        sharded = dist.is_available() and dist.is_initialized()
        adv, _, stats = st.compute_gae(self.gamma, self.lam, next_value=next_value, time_limit=self.time_limit, rule=self.rule,
                                       normalized=not sharded)
        if self.episodes is not None:
            self.episodes.update(st)
        return st, (RolloutStorage.normalize(adv, stats) if sharded else st.advantage_normalized)
