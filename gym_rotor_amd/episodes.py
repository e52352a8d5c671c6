"""The training curve on the device: `episode_scan` turns the [T, N, ...] rows a collected horizon has left in a `RolloutStorage` into
"which episodes finished, how long they were, what they returned, how they ended and how close to the goal" — what the reference's
loop prints and logs as it goes (main.py:132-137, 180, 212-235) — in ONE C call of two launches (qr_episode_scan), and `EpisodeTracker`
owns the tensors that call needs across horizons.

Per env two carries live on the device: the running return per agent (float64) and the running length.  An episode ends in step t
when any agent's done or truncated is set (`RolloutStorage.reset_mask`'s rule); its record is the return per agent, the length, a
flag byte (bit g: agent g's done, bit 7: truncated, bits 4 and 5: agent 0 / 1 "solved" at the time limit, main.py:169-173 with
`TimeLimitRule`'s numbers) and the final error ex = final_obs0[0:3] * x_lim, eb1 = final_obs1[0] * pi.  Statistics over the episodes
of a call go to `last`, accumulated ones to `total` (include/quadrotor_hip.h: the QR_EP_* indices, `_lib.EP_INDEX` here).

Deliberate deviation, the one `QrEvalOut.episode_return` documents: the reference rounds its running return to 4 decimals at every
step; here the float32 rewards are summed in float64 and never rounded (at most 0.5e-4 per step of the episode apart).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _checks as ck
from . import _lib
from .td3 import TimeLimitRule

K, KT = _lib.EP_FIELDS, _lib.EP_TOTAL_FIELDS
DENSE_NAMES = ("ep_return", "ep_length", "ep_flags", "ep_final_error")


def episode_workspace_numel(n_envs: int) -> int:
    """float64 elements of workspace `episode_scan` needs for n_envs envs: one vector of QR_EP_FIELDS per 64-env workgroup."""
    return max(1, (int(n_envs) + 63) // 64) * K


def _check(what, reward, done, truncated, run_return, run_length, last, total, final_obs, dense, workspace):
    """Every shape, dtype and device check of `episode_scan`; returns (T, N, n_agents, final_obs as a list or None)."""
    if not isinstance(reward, torch.Tensor) or reward.dim() != 3 or reward.dtype != torch.float32 or not reward.is_contiguous():
        raise ValueError(f"{what}: reward must be a contiguous float32 [T, N, n_agents] tensor")
    T, N, na = reward.shape
    dev = reward.device
    if na not in (1, 2) or T < 1:
        raise ValueError(f"{what}: one or two agents and T >= 1, got reward of shape {tuple(reward.shape)}")
    ck.tensor(what, "done", done, torch.bool, (T, N, na), dev)
    ck.tensor(what, "truncated", truncated, torch.bool, (T, N), dev)
    ck.tensor(what, "run_return", run_return, torch.float64, (N, na), dev)
    ck.tensor(what, "run_length", run_length, torch.int32, (N,), dev)
    ck.tensor(what, "last", last, torch.float64, (K,), dev)
    ck.tensor(what, "total", total, torch.float64, (KT,), dev)
    if final_obs is not None:
        final_obs = [final_obs] if isinstance(final_obs, torch.Tensor) else list(final_obs)
        if len(final_obs) != na:
            raise ValueError(f"{what}: final_obs is one [T, N, D_k] tensor per agent ({na}), got {len(final_obs)}")
        for k, f in enumerate(final_obs):
            if not isinstance(f, torch.Tensor) or f.dim() != 3 or f.shape[-1] < (3 if k == 0 else 1):
                raise ValueError(f"{what}: final_obs[{k}] must be [T, N, D] with D >= {3 if k == 0 else 1} (ex is three words, eb1 one)")
            ck.tensor(what, f"final_obs[{k}]", f, torch.float32, (T, N, f.shape[-1]), dev)
    shapes = ((torch.float64, (T, N, na)), (torch.int32, (T, N)), (torch.uint8, (T, N)), (torch.float32, (T, N, 4)))
    for name, x, (dtype, shape) in zip(DENSE_NAMES, dense, shapes):
        ck.tensor(what, name, x, dtype, shape, dev, True)
    if dense[3] is not None and final_obs is None:
        raise ValueError(f"{what}: ep_final_error needs final_obs")
    ck.workspace(what, workspace, episode_workspace_numel(N), dev)
    return T, N, na, final_obs


def episode_scan(reward, done, truncated, run_return, run_length, last, total, *, final_obs=None, x_lim: Optional[float] = None,
                 rule: TimeLimitRule = TimeLimitRule(), record: bool = True, ep_return=None, ep_length=None, ep_flags=None, ep_final_error=None,
                 workspace=None) -> torch.Tensor:
    """One horizon's rows into per-episode records and statistics, in one C call (qr_episode_scan; two launches, no synchronisation).

    reward [T, N, n_agents] float32, done [T, N, n_agents] bool, truncated [T, N] bool: as `RolloutStorage` holds them.  run_return
    [N, n_agents] float64 and run_length [N] int32: the carries, read and advanced in place.  last float64 [QR_EP_FIELDS]: this
    call's statistics, written; total float64 [QR_EP_TOTAL_FIELDS]: accumulated in place (start it from `_lib.episode_empty()`).
    final_obs: None, or per agent the [T, N, D_k] terminal observations (`RolloutStorage.final_obs`) — without it the final error
    and the solved bits are zero.  x_lim: the env's position limit; None: rule.x_lim.  rule: pos_tol and rot_tol of the "solved" bits.
    record=False (the warm-up, main.py:218): carries and dense rows as ever, `last` empty, `total` unchanged but for steps_seen.
    ep_return [T, N, n_agents] float64, ep_length [T, N] int32, ep_flags [T, N] uint8, ep_final_error [T, N, 4] float32: optional
    dense rows, zero where no episode ended.  workspace: float64, `episode_workspace_numel(N)` elements (None: made here).
    Every check raises ValueError before a launch.  Returns `last`."""
    what = "episode_scan"
    rule = TimeLimitRule(*rule)
    rule = rule._replace(x_lim=rule.x_lim if x_lim is None else x_lim).check(what)
    dense = (ep_return, ep_length, ep_flags, ep_final_error)
    T, N, na, final_obs = _check(what, reward, done, truncated, run_return, run_length, last, total, final_obs, dense, workspace)
    dev = reward.device
    ck.require_gpu(dev)
    if workspace is None:
        workspace = torch.empty(episode_workspace_numel(N), dtype=torch.float64, device=dev)
    e = _lib.episode_scan_args(reward, done, truncated, final_obs, run_return, run_length, dense, last, total, workspace, n_steps=T, n_envs=N,
                               n_agents=na, x_lim=rule.x_lim, pos_tol=rule.pos_tol, rot_tol=rule.rot_tol, record=record)
    _lib.launch(dev, "qr_episode_scan", e)
    return last


def summarize(vec, n_agents: int) -> dict:
    """The dict `EpisodeTracker.summary` returns, from a `last` or `total` vector on the host (a sequence of floats)."""
    v = [float(x) for x in vec]
    n = v[_lib.EP_COUNT]
    nan = float("nan")
    g = range(n_agents)

    def per(k):
        return [v[k + a] / n if n else nan for a in g]
    mean = per(_lib.EP_RETURN_SUM)
    std = [math.sqrt(max(v[_lib.EP_RETURN_SQ + a] / n - mean[a] ** 2, 0.0)) if n else nan for a in g]
    out = {"episodes": int(n), "return_mean": mean, "return_std": std,
           "return_min": [v[_lib.EP_RETURN_MIN + a] if n else nan for a in g], "return_max": [v[_lib.EP_RETURN_MAX + a] if n else nan for a in g],
           "length_mean": v[_lib.EP_LENGTH_SUM] / n if n else nan, "length_max": int(v[_lib.EP_LENGTH_MAX]),
           "terminated_rate": per(_lib.EP_DONE), "truncated_rate": v[_lib.EP_TRUNCATED] / n if n else nan, "solved_rate": per(_lib.EP_SOLVED),
           "final_ex_mean": v[_lib.EP_EX_SUM] / n if n else nan, "final_eb1_mean": v[_lib.EP_EB1_SUM] / n if n else nan}
    if len(v) > _lib.EP_STEPS_SEEN:
        out["steps_seen"] = int(v[_lib.EP_STEPS_SEEN])
    return out


class EpisodeTracker:
    """The tensors `episode_scan` needs across horizons, made once: the carries `run_return` [N, n_agents] float64 and `run_length` [N]
    int32, `last` and `total`, the workspace and, with dense=True, the four dense tensors (`ep_return`, `ep_length`, `ep_flags`,
    `ep_final_error`; made at the first update when only the env is given, since they need the horizon's T).

    env_or_storage: a `QuadVecEnv` or a `RolloutStorage` (read: the env count, the agents, the device).  rule: the `TimeLimitRule`
    behind the solved bits and the scale of ex; None: the reference's tolerances with x_lim = the env's (1.0 for a storage).
    `update(storage)` after every collected horizon is the whole use: PPO calls it behind `storage.collect`, `OffPolicyCollector`
    (track_episodes=True) behind its append.  Nothing synchronises until `summary` or `episodes`."""

    def __init__(self, env_or_storage, *, rule: Optional[TimeLimitRule] = None, dense: bool = False):
        src = env_or_storage
        self.N = int(src.N if hasattr(src, "N") else src.num_envs)
        self.n_agents, self.device = int(src.n_agents), torch.device(src.device)
        if self.n_agents not in (1, 2) or self.N < 1:
            raise ValueError(f"EpisodeTracker: one or two agents and at least one env, got {self.n_agents} and {self.N}")
        if rule is None:
            rule = TimeLimitRule(x_lim=float(getattr(src, "x_lim", 1.0)))
        self.rule = TimeLimitRule(*rule).check("EpisodeTracker")
        dev = self.device
        self.run_return = torch.zeros(self.N, self.n_agents, dtype=torch.float64, device=dev)
        self.run_length = torch.zeros(self.N, dtype=torch.int32, device=dev)
        dev = self.device = self.run_return.device   # ("cuda" names the current device: keep what the tensors say)
        self._empty = torch.tensor(_lib.episode_empty(), dtype=torch.float64).to(dev)
        self.last, self.total = self._empty[:K].clone(), self._empty.clone()
        self.workspace = torch.zeros(episode_workspace_numel(self.N), dtype=torch.float64, device=dev)
        self.dense, self.T, self.T_last = bool(dense), None, None
        self.ep_return = self.ep_length = self.ep_flags = self.ep_final_error = None
        if self.dense and hasattr(src, "T"):
            self._make_dense(int(src.T), getattr(src, "final_obs", None) is not None)

    def _make_dense(self, T: int, final: bool) -> None:
        dev, N = self.device, self.N
        self.T = T
        self.ep_return = torch.zeros(T, N, self.n_agents, dtype=torch.float64, device=dev)
        self.ep_length = torch.zeros(T, N, dtype=torch.int32, device=dev)
        self.ep_flags = torch.zeros(T, N, dtype=torch.uint8, device=dev)
        self.ep_final_error = torch.zeros(T, N, 4, dtype=torch.float32, device=dev)
        self._dense_final = final

    def _dense_for(self, storage):
        """The dense tensors of an update over this storage (all None without dense=True)."""
        what = "EpisodeTracker.update"
        if storage.N != self.N or storage.n_agents != self.n_agents or storage.reward.device != self.device:
            raise ValueError(f"{what}: the storage has {storage.N} envs and {storage.n_agents} agent(s) on {storage.reward.device}; the tracker "
                             f"{self.N} and {self.n_agents} on {self.device}")
        if not self.dense:
            return (None, None, None, None)
        if self.T is None:
            self._make_dense(int(storage.T), storage.final_obs is not None)
        if storage.T != self.T:
            raise ValueError(f"{what}: the dense rows were made for a horizon of {self.T} steps, the storage has {storage.T}")
        return (self.ep_return, self.ep_length, self.ep_flags, self.ep_final_error if storage.final_obs is not None else None)

    def update(self, storage, record: bool = True) -> torch.Tensor:
        """Scan the horizon `storage` holds: one C call, nothing allocated, nothing synchronised.  Returns `last` (on the device)."""
        dense = self._dense_for(storage)
        self.T_last = int(storage.T)
        return episode_scan(storage.reward, storage.done, storage.truncated, self.run_return, self.run_length, self.last, self.total,
                            final_obs=storage.final_obs, rule=self.rule, record=record, workspace=self.workspace,
                            **dict(zip(DENSE_NAMES, dense)))

    def reset(self) -> None:
        """Clear the carries and `total` (and `last`)."""
        self.run_return.zero_()
        self.run_length.zero_()
        self.total.copy_(self._empty)
        self.last.copy_(self._empty[:K])

    def summary(self, which: str = "last") -> dict:
        """Synchronises.  episodes; return_mean / return_std / return_min / return_max per agent; length_mean, length_max;
        terminated_rate per agent, truncated_rate, solved_rate per agent; final_ex_mean (of max |ex|), final_eb1_mean; steps_seen
        (env-steps per env scanned since creation or reset).  Means and rates are NaN over no episodes."""
        if which not in ("last", "total"):
            raise ValueError(f"EpisodeTracker.summary: which must be 'last' or 'total', got {which!r}")
        out = summarize((self.last if which == "last" else self.total).tolist(), self.n_agents)
        out["steps_seen"] = int(self.total[_lib.EP_STEPS_SEEN].item())
        return out

    def episodes(self, storage_t0: int = 0) -> dict:
        """The episodes that finished in the last update, in (t, n) order — the order the reference would have logged them in (needs
        dense=True; synchronises).  timestep: int64, storage_t0 + steps_seen - T + t + 1, the reference's total_timesteps of the
        episode's last step when the tracker has seen every horizon (storage_t0: env-steps flown before its first); env, length,
        returns [E, n_agents] float64, flags (uint8: `_lib.EP_FLAG_*`), final_error [E, 4] float32 — `log_step`'s and the print
        line's content."""
        if not self.dense or self.T is None or self.T_last is None:
            raise ValueError("EpisodeTracker.episodes needs dense=True and an update")
        t, n = self.ep_length.nonzero(as_tuple=True)
        first = int(storage_t0) + int(self.total[_lib.EP_STEPS_SEEN].item()) - self.T
        return {"timestep": t + (first + 1), "env": n, "length": self.ep_length[t, n], "returns": self.ep_return[t, n],
                "flags": self.ep_flags[t, n], "final_error": self.ep_final_error[t, n]}

    def update_torch(self, storage, record: bool = True) -> torch.Tensor:
        """`update` in plain torch, a loop over t: the twin the GPU tests compare against and the arm the timing compares against, as
        `ReplayBuffer.add` is for `append`.  Carries and dense rows equal `update`'s bit for bit; the float64 sums are taken in
        torch's order.  Works on CPU tensors too."""
        dense = self._dense_for(storage)
        self.T_last = int(storage.T)
        T, N, na, rule = int(storage.T), self.N, self.n_agents, self.rule
        dev = self.device
        if self.dense:
            ep_ret, ep_len, ep_flg, ep_err = self.ep_return, self.ep_length, self.ep_flags, self.ep_final_error
        else:
            ep_ret = torch.zeros(T, N, na, dtype=torch.float64, device=dev)
            ep_len = torch.zeros(T, N, dtype=torch.int32, device=dev)
            ep_flg = torch.zeros(T, N, dtype=torch.uint8, device=dev)
            ep_err = torch.zeros(T, N, 4, dtype=torch.float32, device=dev)
        errd = torch.zeros(T, N, 2, dtype=torch.float64, device=dev)   # max |ex| and |eb1| in double
        final = storage.final_obs
        for t in range(T):
            self.run_return += storage.reward[t].double()
            self.run_length += 1
            limit = storage.truncated[t]
            ended = storage.done[t].any(-1) | limit
            flags = torch.zeros(N, dtype=torch.int32, device=dev)
            for g in range(na):
                flags |= storage.done[t, :, g].to(torch.int32) << g
            flags |= limit.to(torch.int32) << 7
            err = torch.zeros(N, 4, dtype=torch.float64, device=dev)
            if final is not None:
                err[:, :3] = final[0][t, :, :3].double() * rule.x_lim
                solved = [(err[:, :3].abs() <= rule.pos_tol).all(-1) & (storage.reward[t, :, 0] != -1.0)]
                if na == 2:
                    err[:, 3] = final[1][t, :, 0].double() * math.pi
                    solved.append((err[:, 3].abs() <= rule.rot_tol) & (storage.reward[t, :, 1] != -1.0))
                for g in range(na):
                    flags |= (limit & solved[g]).to(torch.int32) << (4 + g)
            zero = torch.zeros((), dtype=torch.float64, device=dev)
            ep_ret[t] = torch.where(ended[:, None], self.run_return, zero)
            ep_len[t] = torch.where(ended, self.run_length, torch.zeros((), dtype=torch.int32, device=dev))
            ep_flg[t] = torch.where(ended, flags, torch.zeros((), dtype=torch.int32, device=dev)).to(torch.uint8)
            err = torch.where(ended[:, None], err, zero)
            if ep_err is not None and final is not None:
                ep_err[t] = err.float()
            errd[t, :, 0], errd[t, :, 1] = err[:, :3].abs().amax(-1), err[:, 3].abs()
            self.run_return.masked_fill_(ended[:, None], 0.0)
            self.run_length.masked_fill_(ended, 0)
        vec = self._empty[:K].clone()
        if record:
            m, ep_flg = ep_len > 0, ep_flg.to(torch.int32)
            md = m.double()
            vec[_lib.EP_COUNT] = md.sum()
            inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
            for g in range(na):
                r = ep_ret[..., g]
                vec[_lib.EP_RETURN_SUM + g], vec[_lib.EP_RETURN_SQ + g] = r.sum(), (r * r).sum()
                vec[_lib.EP_RETURN_MIN + g], vec[_lib.EP_RETURN_MAX + g] = torch.where(m, r, inf).min(), torch.where(m, r, -inf).max()
                vec[_lib.EP_DONE + g] = ((ep_flg >> g) & 1).double().sum()
                vec[_lib.EP_SOLVED + g] = ((ep_flg >> (4 + g)) & 1).double().sum()
            vec[_lib.EP_LENGTH_SUM], vec[_lib.EP_LENGTH_MAX] = ep_len.double().sum(), ep_len.max().double()
            vec[_lib.EP_TRUNCATED] = ((ep_flg >> 7) & 1).double().sum()
            vec[_lib.EP_EX_SUM], vec[_lib.EP_EB1_SUM] = errd[..., 0].sum(), errd[..., 1].sum()
            tot = self.total[:K]
            kmin, kmax = list(_lib.EP_MIN_FIELDS), list(_lib.EP_MAX_FIELDS)
            ksum = [k for k in range(K) if k not in kmin + kmax]
            tot[ksum] = tot[ksum] + vec[ksum]
            tot[kmin] = torch.minimum(tot[kmin], vec[kmin])
            tot[kmax] = torch.maximum(tot[kmax], vec[kmax])
        self.last.copy_(vec)
        self.total[_lib.EP_STEPS_SEEN] += T
        return self.last
