"""On-device rollout storage + GAE.

Batched replacement of the reference's PPO data path: `ReplayBuffer` (NumPy arrays of
`T_horizon` rows per agent: obs, act, rwd, obs_next, done, logprob; algos/replay_buffer.py:15-39)
and the Python GAE loop + advantage normalisation in `PPO.train` (algos/ppo/ppo.py:134-147).
Transitions of N envs stay on the GPU as `[T, N, ...]` tensors; `QuadVecEnv.step(..., out=slot)`
writes observation / reward / done rows straight into them; GAE is one HIP launch
(`qr_gae`: reverse scan over T per (env, agent) column), and so are the critic's values between the two
(`qr_critic_values`, `qr_critic_next_values`: `compute_values`), and so is the actor's loss with its gradients per minibatch
(`qr_ppo_actor_grad`: `actor_grad`), and so is the critic's loss with its gradients per minibatch (`qr_ppo_critic_grad`:
`critic_grad`); the optimiser step that follows is `optim.DeviceAdamW` (`qr_adamw_step`).  Normalisation statistics can be
all-reduced over the env shards (RCCL when launched under torchrun; gloo in the CPU tests).
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import _checks as ck
from . import _lib
from .td3 import TIME_LIMITS, TimeLimitRule


def gae_rule_workspace_numel(n_envs: int, n_agents: int) -> int:
    """float64 elements of workspace `gae_rule` needs for its stats: 2 * n_agents per 64-column workgroup."""
    return max(1, (int(n_envs) * int(n_agents) + 63) // 64) * 2 * int(n_agents)


def gae_rule(reward, done, value, advantage, td_target, *, gamma: float = 0.99, lam: float = 0.9, next_value=None, truncated=None, term_obs=None,
             rule=None, done_eff=None, stats=None, normalized=None, workspace=None, norm_eps: float = _lib.GAE_NORM_EPS):
    """ppo.py:134-146 over the done flag the reference stores, in one C call (qr_gae_rule; up to three launches, no synchronisation).

    reward [T, N, n_agents] float32, done [T, N, n_agents] bool, value [T + 1, N, n_agents] float32 (row T: the bootstrap; [T, ...] will
    do with next_value), next_value None or [T, N, n_agents] float32: as `RolloutStorage` holds them and as qr_gae reads them.
    advantage, td_target [T, N, n_agents] float32: written.  rule: None — each agent's own flag — or a `TimeLimitRule`
    (x_lim, pos_tol, rot_tol): on transitions whose `truncated` [T, N] is set the flag is main.py:169-173's, "the error in obs_next
    is within tolerance and the reward is not -1", read from term_obs — per agent the [T, N, D_k] rows that hold obs_next on those
    transitions (`storage.final_obs`, or `[o[1:] for o in storage.obs]`).  done_eff [T, N, n_agents] bool or uint8: optional, the flag
    the scan used.  stats float64 [n_agents, 3]: optional, per agent sum, sum of squares and count of its advantages
    (`RolloutStorage.normalize`'s input).  normalized [T, N, n_agents] float32: optional, (adv - mean) / (std + norm_eps) with torch's
    unbiased std; needs stats and T * N >= 2.  workspace: float64, `gae_rule_workspace_numel(N, n_agents)` elements (None with stats:
    made here).  Every check raises ValueError before a launch.  Returns (advantage, td_target, stats)."""
    what = "gae_rule"
    if not isinstance(reward, torch.Tensor) or reward.dim() != 3 or reward.dtype != torch.float32 or not reward.is_contiguous():
        raise ValueError(f"{what}: reward must be a contiguous float32 [T, N, n_agents] tensor")
    T, N, na = reward.shape
    dev = reward.device
    if na not in (1, 2) or T < 1:
        raise ValueError(f"{what}: one or two agents and T >= 1, got reward of shape {tuple(reward.shape)}")
    f32, flag = torch.float32, (torch.bool, torch.uint8)
    ck.tensor(what, "done", done, flag, (T, N, na), dev)
    if next_value is None:
        ck.tensor(what, "value", value, f32, (T + 1, N, na), dev)
    else:
        if not isinstance(value, torch.Tensor) or value.dim() != 3 or value.shape[0] not in (T, T + 1):
            raise ValueError(f"{what}: value must be [{T} or {T + 1}, {N}, {na}]")
        ck.tensor(what, "value", value, f32, (value.shape[0], N, na), dev)
        ck.tensor(what, "next_value", next_value, f32, (T, N, na), dev)
    ck.tensor(what, "advantage", advantage, f32, (T, N, na), dev)
    ck.tensor(what, "td_target", td_target, f32, (T, N, na), dev)
    if rule is not None:
        rule = TimeLimitRule(*rule).check(what)
        if truncated is None or term_obs is None:
            raise ValueError(f"{what}: the time-limit rule needs truncated and term_obs, the rows that hold obs_next at the time limit")
        ck.tensor(what, "truncated", truncated, flag, (T, N), dev)
        term_obs = [term_obs] if isinstance(term_obs, torch.Tensor) else list(term_obs)
        if len(term_obs) != na:
            raise ValueError(f"{what}: term_obs is one [T, N, D_k] tensor per agent ({na}), got {len(term_obs)}")
        for k, f in enumerate(term_obs):
            if not isinstance(f, torch.Tensor) or f.dim() != 3 or f.shape[-1] < (3 if k == 0 else 1):
                raise ValueError(f"{what}: term_obs[{k}] must be [T, N, D] with D >= {3 if k == 0 else 1} (ex is three words, eb1 one)")
            ck.tensor(what, f"term_obs[{k}]", f, f32, (T, N, f.shape[-1]), dev)
    else:
        truncated = term_obs = None
    ck.tensor(what, "done_eff", done_eff, flag, (T, N, na), dev, True)
    if normalized is not None:
        ck.tensor(what, "normalized", normalized, f32, (T, N, na), dev)
        if stats is None:
            raise ValueError(f"{what}: normalized needs stats")
        if T * N < 2:
            raise ValueError(f"{what}: normalized needs at least two transitions per agent (the unbiased std), got {T} x {N}")
        ck.nonneg(what, ("norm_eps",), norm_eps)
    if stats is not None:
        ck.tensor(what, "stats", stats, torch.float64, (na, 3), dev)
        ck.workspace(what, workspace, gae_rule_workspace_numel(N, na), dev)
    ck.require_gpu(dev)
    if stats is not None and workspace is None:
        workspace = torch.empty(gae_rule_workspace_numel(N, na), dtype=torch.float64, device=dev)
    e = _lib.gae_rule_args(reward, done, truncated, term_obs, value, next_value, advantage, td_target, done_eff, stats, normalized,
                           workspace if stats is not None else None, n_steps=T, n_envs=N, n_agents=na, gamma=gamma, lam=lam, rule=rule,
                           norm_eps=norm_eps)
    _lib.launch(dev, "qr_gae_rule", e)
    return advantage, td_target, stats


class RolloutStorage:
    """[T(+1), N, ...] buffers for one PPO horizon of a QuadVecEnv.

    obs[k]      [T+1, N, D_k]   observation of agent k BEFORE step t; row T = after the last step.
                               With same-step auto-reset the row after an episode's last step holds the
                               NEW episode's first observation, so obs[t+1] is NOT the reference's
                               obs_next of that transition (main.py:163-178 stores the true next
                               observation and ppo.py:128-138 evaluates the critic on it).  (1 - done)
                               hides the difference only for the agent that terminated: a time-limit
                               truncation (done = 0) and — MODUL — the agent that did NOT terminate when
                               the other one ended the episode both bootstrap from V(obs_next).
    final_obs[k] [T, N, D_k]    (final_obs=True) the terminal observation of every env that was re-sampled
                               in step t, written by the step kernel (QrStepOut.final_obs*); rows of envs
                               that did not reset are meaningless.  `next_values(critic)` builds the
                               reference's V(obs_next) from it: value[t+1] everywhere except on reset
                               rows, where the critic is evaluated on final_obs.
    act[k]      [T, N, A_k]     logprob[k] [T, N, A_k]  (per-dimension log-probs, ppo.py buffer)
    reward      [T, N, n_agents]   done [T, N, n_agents] (bool)   truncated [T, N] (bool)
    value       [T+1, N, n_agents] critic outputs, row T = bootstrap
    """

    def __init__(self, env, horizon: int, action_dims: Optional[List[int]] = None, final_obs: Optional[bool] = None):
        self.T, self.N, self.device = int(horizon), env.num_envs, env.device
        self.n_agents = env.n_agents
        f32 = dict(dtype=torch.float32, device=self.device)
        if action_dims is None:
            action_dims = [env.action_dim] if env.n_agents == 1 else [4, 1]  # main.py:161: agents' actions concatenated
        if sum(action_dims) != env.action_dim:
            raise ValueError("action_dims must sum to the env's action dimension")
        self.action_dims = list(action_dims)
        T, N = self.T, self.N
        self.obs = [torch.zeros(T + 1, N, d, **f32) for d in env.obs_dims]
        if final_obs is None:  # needed (and possible) exactly when the env re-samples inside the step
            final_obs = bool(env.auto_reset) and (env.kind != "quad" or env.obs_rows)
        if final_obs and not env.auto_reset:
            raise ValueError("final_obs needs an env with auto_reset=True")
        self.final_obs = [torch.zeros(T, N, d, **f32) for d in env.obs_dims] if final_obs else None
        # agents' actions / log-probs concatenated along the last axis (main.py:161), which is the row
        # layout qr_rollout_actor writes; act[k] / logprob[k] are per-agent views into them
        self.act_all = torch.zeros(T, N, env.action_dim, **f32)
        self.logprob_all = torch.zeros(T, N, env.action_dim, **f32)
        self.act = list(torch.split(self.act_all, self.action_dims, dim=-1))
        self.logprob = list(torch.split(self.logprob_all, self.action_dims, dim=-1))
        self.reward = torch.zeros(T, N, self.n_agents, **f32)
        self.done = torch.zeros(T, N, self.n_agents, dtype=torch.bool, device=self.device)
        self.truncated = torch.zeros(T, N, dtype=torch.bool, device=self.device)
        self.value = torch.zeros(T + 1, N, self.n_agents, **f32)
        self.advantage = torch.zeros(T, N, self.n_agents, **f32)
        self.td_target = torch.zeros(T, N, self.n_agents, **f32)
        self.env_x_lim = getattr(env, "x_lim", None)   # the default x_lim of compute_gae(time_limit="solved")
        self.gae_stats = self._gae_workspace = self.advantage_normalized = self.done_eff = None   # compute_gae's, made at first use
        _lib.load()   # a missing library is reported here, not at the first launch
        self._ppo_workspace = {}   # (agent, B, max_workgroups) -> workspace of actor_grad
        self._critic_workspace = {}   # (agent, B, max_workgroups) -> workspace of critic_grad

    def set_initial_obs(self, obs):
        obs = [obs] if isinstance(obs, torch.Tensor) else list(obs)
        for k, o in enumerate(obs):
            self.obs[k][0].copy_(o)

    def slot(self, t: int) -> dict:
        """Output slices for `env.step(actions, out=storage.slot(t))`: the step kernel writes the
        next observation (row t+1), reward, done and truncated of step t directly into the storage."""
        out = {"obs0": self.obs[0][t + 1], "reward": self.reward[t], "terminated": self.done[t], "truncated": self.truncated[t]}
        if len(self.obs) > 1:
            out["obs1"] = self.obs[1][t + 1]
        if self.final_obs is not None:
            for k, f in enumerate(self.final_obs):
                out[f"final_obs{k}"] = f[t]
        return out

    def horizon(self) -> dict:
        """Output tensors of one whole horizon for `env.rollout_actor(actors, T, out=storage.horizon())`."""
        out = {"obs0": self.obs[0][1:], "action": self.act_all, "logprob": self.logprob_all, "reward": self.reward,
               "terminated": self.done, "truncated": self.truncated}
        if len(self.obs) > 1:
            out["obs1"] = self.obs[1][1:]
        if self.final_obs is not None:
            for k, f in enumerate(self.final_obs):
                out[f"final_obs{k}"] = f
        return out

    def reset_mask(self) -> torch.Tensor:
        """[T, N] bool: the env was re-sampled at the end of step t (an agent terminated or the time limit hit)."""
        return self.done.any(-1) | self.truncated

    def next_values(self, critic) -> torch.Tensor:
        """The reference's V(obs_next) for every transition, [T, N, n_agents]: value[t+1] (which must already
        hold V(obs[t+1]), row T = the bootstrap row) except where the env was re-sampled in step t — there
        `critic` is evaluated on the terminal observation rows.  critic(list of per-agent [n, D_k] rows) ->
        [n, n_agents].  Pass the result to compute_gae(next_value=...)."""
        nv = self.value[1:].clone()
        if self.final_obs is None:
            return nv
        idx = self.reset_mask().nonzero(as_tuple=True)
        if idx[0].numel():
            rows = [f[idx] for f in self.final_obs]
            nv[idx] = critic(rows).reshape(-1, self.n_agents).to(nv.dtype)
        return nv

    def compute_values(self, critics) -> torch.Tensor:
        """The critic over the whole horizon on the device: fills `value` with V(obs[t]) for all T+1 rows and returns the
        reference's V(obs_next), [T, N, n_agents], ready for compute_gae(next_value=...) — what `next_values(module)` gives after
        the module has filled `value`, without the module, the gather of reset rows or its host synchronisation.
        critics: one `CriticParams` per agent (`CriticParams.from_module(module, inputs=...)`).  One launch per critic for the
        values (qr_critic_values) and, with final_obs, one for the next values (qr_critic_next_values); without final_obs the
        result is the view value[1:]."""
        from .policy import CriticParams, critic_next_values, critic_values
        critics = [critics] if isinstance(critics, CriticParams) else list(critics)
        if len(critics) != self.n_agents:
            raise ValueError(f"compute_values needs one CriticParams per agent ({self.n_agents}), got {len(critics)}")
        for k, c in enumerate(critics):
            critic_values(c, self.obs, self.value[..., k])
        if self.final_obs is None:
            return self.value[1:]
        next_value = torch.empty(self.T, self.N, self.n_agents, dtype=torch.float32, device=self.device)
        for k, c in enumerate(critics):
            critic_next_values(c, self.final_obs, self.done, self.truncated, self.value[..., k], next_value[..., k])
        return next_value

    def actor_grad(self, k: int, actor, advantage: torch.Tensor, index: Optional[torch.Tensor] = None, **coeffs):
        """PPO's actor loss and its gradients for agent k on the minibatch `index` (int64 rows of the flat [T * N] transitions; None:
        all of them) in one launch that reads this storage in place (`policy.ppo_actor_grad`): obs[k], the agent's columns of
        the shared action / logprob rows, final_obs / done / truncated for the reference's obs_next.  advantage: [T, N, n_agents]
        (agent k's column is taken) or [T, N].  coeffs: clip, entropy_coef, lam_T, lam_S, lam_M, noise, nominal, max_action, grads,
        stats, max_workgroups, entropy_coef_dev (a float32 device word read instead of entropy_coef).  The workspace is kept per (agent, B, max_workgroups).  Returns (grads, stats)."""
        from .policy import ppo_actor_grad, ppo_workspace_bytes
        k = int(k)
        if not 0 <= k < self.n_agents:
            raise ValueError(f"agent {k} of {self.n_agents}")
        adv = advantage[..., k] if advantage.dim() == 3 else advantage
        B = self.T * self.N if index is None else index.numel()
        mw = int(coeffs.get("max_workgroups", 0))
        key = (k, B, mw)
        if B and key not in self._ppo_workspace:
            self._ppo_workspace[key] = torch.empty(ppo_workspace_bytes(actor.dims, B, mw) // 8, dtype=torch.float64, device=self.device)
        fin = {} if self.final_obs is None else dict(final_obs=self.final_obs[k], done=self.done, truncated=self.truncated)
        return ppo_actor_grad(actor, self.obs[k], self.act_all, self.logprob_all, adv, index, col_offset=sum(self.action_dims[:k]),
                              workspace=self._ppo_workspace.get(key), **fin, **coeffs)

    def critic_grad(self, k: int, critic, index: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None, **coeffs):
        """PPO's critic loss and its gradients for agent k's critic on the minibatch `index` (int64 rows of the flat [T * N]
        transitions; None: all of them) in one launch that reads this storage in place (`policy.ppo_critic_grad`): the observation
        rows `critic.inputs` names (rows past T * N, the bootstrap row among them, are never read) and `target`, by default
        td_target[..., k] as compute_gae left it; a given target is [T, N, n_agents] (agent k's column is taken) or [T, N].
        coeffs: l2_reg, grads, stats, max_workgroups.  The workspace is kept per (agent, B, max_workgroups).
        Returns (grads, stats)."""
        from .policy import ppo_critic_grad, ppo_critic_workspace_bytes
        k = int(k)
        if not 0 <= k < self.n_agents:
            raise ValueError(f"agent {k} of {self.n_agents}")
        if target is None:
            target = self.td_target
        if tuple(target.shape[:2]) != (self.T, self.N) or target.dim() not in (2, 3):
            raise ValueError(f"critic_grad: target must be [{self.T}, {self.N}, n_agents] or [{self.T}, {self.N}], got {tuple(target.shape)}")
        tgt = target[..., k] if target.dim() == 3 else target
        B = self.T * self.N if index is None else index.numel()
        mw = int(coeffs.get("max_workgroups", 0))
        key = (k, B, mw)
        need = ppo_critic_workspace_bytes(critic.dims, B, mw) // 8 if B else 0
        if B and (key not in self._critic_workspace or self._critic_workspace[key].numel() < need):   # (a second, wider critic of one agent)
            self._critic_workspace[key] = torch.empty(need, dtype=torch.float64, device=self.device)
        return ppo_critic_grad(critic, self.obs, tgt, index, workspace=self._critic_workspace.get(key), **coeffs)

    @staticmethod
    def nominal_action(env, k: int, max_action: float = 1.0, device=None) -> torch.Tensor:
        """The nominal action of the magnitude term (policy_regularization.py:30-46), float32 [A_k]: the hover thrust mapped into
        [-max_action, max_action] followed by zero moments (MONO, and MODUL agent 0); zero for MODUL agent 1 (the yaw moment)."""
        import numpy as np
        if env.n_agents == 2 and int(k) == 1:
            vals = [0.0]
        else:
            f = float(np.interp(4.0 * env.hover_force, [4.0 * env.min_force, 4.0 * env.max_force], [-max_action, max_action]))
            vals = [f, 0.0, 0.0, 0.0]
        return torch.tensor(vals, dtype=torch.float32, device=env.device if device is None else device)

    def collect(self, env, actors, **kw) -> dict:
        """One horizon with the actor(s) inside the step kernel (qr_rollout_actor): obs row 0 is the
        env's current observation, everything else is written by the single launch."""
        cur = env._last_obs
        if cur is None:
            raise ValueError("no current observation: call env.get_norm_error_state() or env.step() first")
        self.set_initial_obs(cur)
        return env.rollout_actor(actors, self.T, obs=[o[0] for o in self.obs], out=self.horizon(), **kw)

    def insert(self, t: int, act=None, logprob=None, value=None):
        """Learner-side quantities of step t (actions taken, their log-probs, V(obs[t]))."""
        for dst, src in ((self.act, act), (self.logprob, logprob)):
            if src is not None:
                src = [src] if isinstance(src, torch.Tensor) else list(src)
                for k, s in enumerate(src):
                    dst[k][t].copy_(s)
        if value is not None:
            self.value[t].copy_(value.reshape(self.N, self.n_agents))

    def compute_gae(self, gamma: float = 0.99, lam: float = 0.9, last_value: Optional[torch.Tensor] = None,
                    next_value: Optional[torch.Tensor] = None, want_stats: bool = True, *, time_limit: str = "own",
                    rule: Optional[TimeLimitRule] = None, normalized: bool = False, done_eff: bool = False):
        """ppo.py:134-146 for every (env, agent) column in one launch.  `last_value` fills the
        bootstrap row value[T]; `next_value` ([T,N,n_agents]) overrides Vnext_t = value[t+1] — with an
        auto-resetting env pass `next_values(critic)`: value[t+1] is V of the NEW episode's first
        observation on reset rows, which is not what the reference bootstraps from (see the class
        docstring).  The recursion itself is the reference's: masked by `done` only.
        Returns (advantage, td_target[, (sum, sumsq, count) per agent as float64 [n_agents, 3]]).

        With the keyword-only arguments at their defaults that is all (qr_gae).  Any other value goes through ONE call of qr_gae_rule
        (`gae_rule`) and returns (advantage, td_target, stats), stats being the kept tensor `gae_stats` (None with want_stats=False and
        normalized=False):
        time_limit="solved": `done` is, on the transitions whose `truncated` is set, the flag the reference stores there
            (main.py:169-173, 176-177: "solved and not crashed", read from final_obs, or from obs[t + 1] in a storage without it) in
            both places ppo.py:134-146 reads it — a solved episode is not bootstrapped and cuts the recursion, an env that crashed
            on its last step is bootstrapped and does not.  rule: the three numbers; None: TimeLimitRule(x_lim=the env's).
            With time_limit="own" a given rule is checked and has NO effect on the flags (the call still goes through qr_gae_rule):
            the rule's numbers are read at the time limit only, and "own" keeps each agent's flag there.
        normalized=True: `advantage_normalized` holds (adv - mean) / (std + 1e-4) per agent, what `normalize(advantage, stats)`
            gives on one rank, from the same call.
        done_eff=True: `done_eff` ([T, N, n_agents] bool) holds the flag the scan used.
        Both tensors are made at first use and kept; every check is made before the launch."""
        if time_limit != "own" or rule is not None or normalized or done_eff:
            return self._compute_gae_rule(gamma, lam, last_value, next_value, want_stats, time_limit, rule, normalized, done_eff)
        if last_value is not None:
            self.value[self.T].copy_(last_value.reshape(self.N, self.n_agents))
        M = self.N * self.n_agents
        grid = (M + 63) // 64
        partials = torch.zeros(grid, 2, dtype=torch.float64, device=self.device) if want_stats else None
        nv = None if next_value is None else next_value.contiguous()
        if nv is not None and (tuple(nv.shape) != (self.T, self.N, self.n_agents) or nv.dtype != torch.float32 or nv.device != self.device):
            raise ValueError(f"next_value must be float32 [{self.T}, {self.N}, {self.n_agents}] on {self.device}")
        # (launched on the storage's device, whatever the caller's current device is)
        _lib.launch(self.device, "qr_gae", self.reward.data_ptr(), self.done.data_ptr(), self.value.data_ptr(), _lib.ptr(nv), self.T, M, float(gamma),
                    float(lam), self.advantage.data_ptr(), self.td_target.data_ptr(), _lib.ptr(partials))
        if not want_stats:
            return self.advantage, self.td_target
        if self.n_agents == 1:
            tot = partials.sum(0, keepdim=True)
        else:  # columns interleave agents: recompute per-agent sums from the advantages (small)
            a64 = self.advantage.double()
            tot = torch.stack([a64.sum((0, 1)), (a64 * a64).sum((0, 1))], 1)
        cnt = torch.full((self.n_agents, 1), float(self.T * self.N), dtype=torch.float64, device=self.device)
        return self.advantage, self.td_target, torch.cat([tot, cnt], 1)

    def _compute_gae_rule(self, gamma, lam, last_value, next_value, want_stats, time_limit, rule, normalized, done_eff):
        """compute_gae's path through qr_gae_rule: the checks, the kept tensors, one call."""
        what = "compute_gae"
        if time_limit not in TIME_LIMITS:
            raise ValueError(f"time_limit must be one of {TIME_LIMITS}, got {time_limit!r}")
        if rule is None:
            rule = TimeLimitRule() if self.env_x_lim is None else TimeLimitRule(x_lim=float(self.env_x_lim))
        rule = TimeLimitRule(*rule).check(what)
        truncated = term_obs = None
        if time_limit == "solved":
            if self.truncated is None:
                raise ValueError("time_limit='solved' needs the storage's truncated flags: they mark the transitions at the time limit")
            if self.obs[0].shape[-1] < 3:
                raise ValueError("time_limit='solved' reads ex, the first three words of agent 0's observation")
            truncated = self.truncated
            term_obs = self.final_obs if self.final_obs is not None else [o[1:] for o in self.obs]
        else:
            rule = None
        T, N, na, dev = self.T, self.N, self.n_agents, self.reward.device
        if last_value is not None and last_value.numel() != N * na:
            raise ValueError(f"last_value must hold {N} x {na} values")
        nv = None if next_value is None else next_value.contiguous()
        if nv is not None and (tuple(nv.shape) != (T, N, na) or nv.dtype != torch.float32 or nv.device != dev):
            raise ValueError(f"next_value must be float32 [{T}, {N}, {na}] on {dev}")
        if normalized and T * N < 2:
            raise ValueError(f"{what}: normalized=True needs at least two transitions per agent, got {T} x {N}")
        ck.require_gpu(dev)
        stats = want_stats or normalized
        if stats and self.gae_stats is None:
            self.gae_stats = torch.zeros(na, 3, dtype=torch.float64, device=dev)
            self._gae_workspace = torch.zeros(gae_rule_workspace_numel(N, na), dtype=torch.float64, device=dev)
        if normalized and self.advantage_normalized is None:
            self.advantage_normalized = torch.zeros(T, N, na, dtype=torch.float32, device=dev)
        if done_eff and self.done_eff is None:
            self.done_eff = torch.zeros(T, N, na, dtype=torch.bool, device=dev)
        if last_value is not None:
            self.value[T].copy_(last_value.reshape(N, na))
        return gae_rule(self.reward, self.done, self.value, self.advantage, self.td_target, gamma=gamma, lam=lam, next_value=nv,
                        truncated=truncated, term_obs=term_obs, rule=rule, done_eff=self.done_eff if done_eff else None,
                        stats=self.gae_stats if stats else None, normalized=self.advantage_normalized if normalized else None,
                        workspace=self._gae_workspace if stats else None)

    @staticmethod
    def normalize(advantage: torch.Tensor, stats: torch.Tensor, group=None) -> torch.Tensor:
        """(adv - mean) / (std + 1e-4) with torch's unbiased std (ppo.py:147), per agent, over ALL
        envs of all ranks when torch.distributed is initialised (stats are all-reduced: 3 doubles
        per agent over RCCL/gloo — the only collective of the data path, and optional)."""
        import torch.distributed as dist
        st = stats.clone()
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(st, group=group)
        s1, s2, n = st[:, 0], st[:, 1], st[:, 2]
        mean = s1 / n
        var = (s2 - n * mean * mean) / (n - 1.0)
        std = var.clamp_min(0).sqrt()
        return ((advantage.double() - mean) / (std + 1e-4)).float()

    def sample(self):
        """The reference's `ReplayBuffer.sample()` for PPO (replay_buffer.py:41-57): per-agent
        lists of [T*N, ...] float tensors (obs, act, rwd, obs_next, done, logprob), time-major."""
        T, N = self.T, self.N
        flat = lambda x: x.reshape(T * N, -1)
        obs = [flat(o[:-1]) for o in self.obs]
        obs_next = [o[1:].clone() for o in self.obs]
        if self.final_obs is not None:  # the true next observation of transitions that ended an episode
            idx = self.reset_mask().nonzero(as_tuple=True)
            for k, f in enumerate(self.final_obs):
                obs_next[k][idx] = f[idx]
        obs_next = [flat(o) for o in obs_next]
        act = [flat(a) for a in self.act]
        logp = [flat(l) for l in self.logprob]
        rwd = [flat(self.reward[..., k:k + 1]) for k in range(self.n_agents)]
        done = [flat(self.done[..., k:k + 1].float()) for k in range(self.n_agents)]
        return obs, act, rwd, obs_next, done, logp
