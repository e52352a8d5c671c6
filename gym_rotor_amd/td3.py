"""A TD3 update on the device: the replay buffer as flat device tensors (`ReplayBuffer`), the target values of a minibatch in one
launch (`td3_target`: qr_twinq_target), the twin-Q loss and its twelve gradients in two (`twinq_grad`: qr_twinq_grad), both on live
modules (`td3_critic_loss`); the actor's loss -mean Q1(s, pi(s)) with its smoothness terms and its six gradients in two launches
(`dpg_actor_grad`: qr_dpg_actor_grad; on live modules `td3_actor_loss`), and the soft target update of all tensors in one
(`soft_update`: qr_soft_update).

Replaces, per minibatch of `TD3.train` (algos/td3/td3.py:111-211): the index clones, the actor-target forward pass, randn_like's two
clamps, two twin-critic forward passes, min, the Bellman line, two mse_loss and the autograd backward pass; and every
policy_update_freq-th iteration three actor passes, the Q1 pass, the backward pass through the critic and three times through the
actor, and eighteen copy_ lines.  The optimiser group of twelve tensors is `optim.PolyakAdamW` (one clip over all twelve, as
the reference's; `optim.DeviceAdamW` takes eight tensors), and the whole loop is `offpolicy.Td3Updater`.

The critic half also exists for ONE centralized (CTDE) twin critic over the two agents of a Decoupled buffer (td3.py:124-137, 157-158):
`td3_target_ctde` (qr_ctde_twinq_target), `twinq_grad_ctde` (qr_ctde_twinq_grad) and `td3_critic_loss_ctde` on live modules.  The
critic's row [obs_0 | obs_1 | act_0 | act_1] is formed inside the kernels from the agents' tensors; nothing is concatenated.
So does agent k's actor half under that critic (td3.py:180-196): `dpg_actor_grad_ctde` (qr_ctde_dpg_actor_grad) and, on live modules,
`td3_actor_loss_ctde` — the other agent's actor runs forward only inside the kernel (or its action is supplied), and only agent k's
six gradients are produced.  A written-out CTDE iteration is `td3_critic_loss_ctde`, optimiser, `td3_actor_loss_ctde`, optimiser,
`soft_update`, with no autograd in it.

The data side matches: `ReplayBuffer.append` writes a whole horizon into the ring in one launch (`replay_add`: qr_replay_add), and
`ReplayBuffer.sample_index` draws a minibatch's distinct rows in O(B) (`replay_sample`: qr_replay_sample) — a keyed permutation of
[0, current_size) in integers, not a permutation of the whole buffer.  `use_device_state()` moves the three counters into device
memory, so an iteration that appends and samples can be captured in a graph once and replayed.  `append(storage, time_limit="solved")`
stores the reference's done at the episode time limit (main.py:169-173: "solved and not crashed") in the same single launch
(qr_replay_add_rule); the default, "own", stores each agent's own flag.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

import torch

from . import _checks as ck
from . import _lib
from .policy import ActorParams, PPO_ACTOR_DIMS, QCriticParams, _grad_outputs, module_grads


TIME_LIMITS = ("own", "solved")   # what `done` holds on a transition at the episode time limit: the agent's own flag / main.py:169-173


class TimeLimitRule(NamedTuple):
    """The numbers of the reference's time-limit rule (main.py:169-173): done = all |ex| <= pos_tol (ex = obs_next_0[0:3] * x_lim) for
    agent 0, |eb1| <= rot_tol (eb1 = obs_next_1[0] * pi) for Decoupled's agent 1, and the reward is not the crash reward -1."""
    x_lim: float = 1.0      # the env's position limit (QuadVecEnv.x_lim)
    pos_tol: float = 0.03   # [m]
    rot_tol: float = 0.03   # [rad]

    def check(self, what: str) -> "TimeLimitRule":
        x, p, r = (float(v) for v in self)
        if not (math.isfinite(x) and x > 0.0 and math.isfinite(p) and p >= 0.0 and math.isfinite(r) and r >= 0.0):
            raise ValueError(f"{what}: the time-limit rule needs a finite x_lim > 0 and finite tolerances >= 0, got {tuple(self)}")
        return TimeLimitRule(x, p, r)


class ReplayBuffer:
    """The reference's `ReplayBuffer` (algos/replay_buffer.py) for TD3 / SAC as flat device tensors per agent k:
        obs[k], obs_next[k] [capacity, D_k]   act[k] [capacity, A_k]   rwd[k], done[k] [capacity] float32 (done: 0.0 / 1.0)
    `count` (the next row to write) and `current_size` follow the reference's ring rule, one transition at a time:
    count = (count + 1) % capacity, current_size = min(current_size + 1, capacity).
    seed: the 64-bit key of `sample_index`'s draws (`seed(s)` changes it); `draw` counts them.
    time_limit_rule: the numbers `add` / `append` use with time_limit="solved" (set x_lim to the env's)."""

    def __init__(self, capacity: int, obs_dims: Sequence[int], action_dims: Sequence[int], device, seed: int = 0):
        self.capacity = int(capacity)
        self.obs_dims, self.action_dims = [int(d) for d in obs_dims], [int(a) for a in action_dims]
        if self.capacity < 1 or len(self.obs_dims) != len(self.action_dims) or not self.obs_dims:
            raise ValueError("ReplayBuffer needs capacity >= 1 and one obs_dim and one action_dim per agent")
        self.device = torch.device(device)
        f32 = dict(dtype=torch.float32, device=self.device)
        n = self.capacity
        self.obs = [torch.zeros(n, d, **f32) for d in self.obs_dims]
        self.obs_next = [torch.zeros(n, d, **f32) for d in self.obs_dims]
        self.act = [torch.zeros(n, a, **f32) for a in self.action_dims]
        self.rwd = [torch.zeros(n, **f32) for _ in self.obs_dims]
        self.done = [torch.zeros(n, **f32) for _ in self.obs_dims]
        self.count, self.current_size = 0, 0
        self.draw = 0          # minibatches drawn by sample_index: with the seed, the key of the next one
        self.seed(seed)
        self.time_limit_rule = TimeLimitRule()
        self.state = None      # use_device_state(): int64 [3] = (count, current_size, draw) on the device
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)   # qr_replay_sample raises it if a walk hits its cap (it cannot)
        self._cache = {}   # (agent, B, max_workgroups) -> y, workspace, stats of td3_critic_loss; ("actor", ...) -> td3_actor_loss's

    @property
    def n_agents(self) -> int:
        return len(self.obs_dims)

    def _scratch(self, key: tuple, make):
        """The tensors a `*_loss` wrapper keeps between calls, from the cache under `key`; made by `make()` at first use."""
        hit = self._cache.get(key)
        if hit is None:
            hit = self._cache[key] = make()
        return hit

    def _actor_scratch(self, tag: str, k: int, index, max_workgroups: int, dev, workspace_bytes, n_stats: int = 4):
        """(workspace, stats [n_stats]) of an actor-loss wrapper under (tag, k, B, max_workgroups); workspace_bytes(B): the size query."""
        B = self.capacity if index is None else index.numel()
        return self._scratch((tag, k, B, int(max_workgroups)), lambda: (
            torch.empty(workspace_bytes(B) // 8 if B else 0, dtype=torch.float64, device=dev), torch.empty(n_stats, dtype=torch.float32, device=dev)))

    def _check_storage(self, storage, time_limit: str) -> Optional[TimeLimitRule]:
        """add's and append's checks, before anything is written; the rule's numbers for time_limit "solved", None for "own"."""
        T, N = storage.T, storage.N
        n = T * N
        if time_limit not in TIME_LIMITS:
            raise ValueError(f"time_limit must be one of {TIME_LIMITS}, got {time_limit!r}")
        if n > self.capacity:
            raise ValueError(f"a horizon of {T} x {N} = {n} transitions does not fit a buffer of {self.capacity}")
        if storage.n_agents != self.n_agents or [o.shape[-1] for o in storage.obs] != self.obs_dims or list(storage.action_dims) != self.action_dims:
            raise ValueError("the storage's agents, observation widths or action widths differ from the buffer's")
        if time_limit == "own":
            return None
        if storage.truncated is None:
            raise ValueError("time_limit='solved' needs the storage's truncated flags: they mark the transitions at the time limit")
        if self.obs_dims[0] < 3:
            raise ValueError("time_limit='solved' reads ex, the first three words of agent 0's observation")
        return TimeLimitRule(*self.time_limit_rule).check("ReplayBuffer")

    def add(self, storage, time_limit: str = "own") -> None:
        """Append one collected `RolloutStorage` horizon: its T * N transitions in (t, n) order — what T * N calls of the reference's
        store_transition leave, wrapping at capacity.  obs_next is the reference's: final_obs where the env was re-sampled in the
        step (any agent's done, or truncated: qr_critic_next_values' rule), obs[t + 1] elsewhere; done is agent k's own flag.
        time_limit="solved": on transitions whose `truncated` is set, done is the reference's main.py:169-173 instead — agent 0: all
        |obs_next_0[0:3] * x_lim| <= pos_tol, agent 1: |obs_next_1[0] * pi| <= rot_tol, compared in float64, and reward != -1
        (`time_limit_rule` holds the three numbers).  Plain torch copies, once per horizon."""
        rule = self._check_storage(storage, time_limit)
        T, N = storage.T, storage.N
        n = T * N
        reset = storage.reset_mask().reshape(n, 1) if storage.final_obs is not None else None
        first = min(n, self.capacity - self.count)   # rows [count, count + first), then rows [0, n - first)
        for k in range(self.n_agents):
            nxt = storage.obs[k][1:].reshape(n, -1)
            if reset is not None:
                nxt = torch.where(reset, storage.final_obs[k].reshape(n, -1), nxt)
            done = storage.done[..., k].reshape(n)
            if rule is not None:
                err = nxt[:, :3].double() * rule.x_lim if k == 0 else nxt[:, :1].double() * math.pi
                solved = (err.abs() <= (rule.pos_tol if k == 0 else rule.rot_tol)).all(-1) & (storage.reward[..., k].reshape(n) != -1.0)
                done = torch.where(storage.truncated.reshape(n), solved, done)
            cols = ((self.obs[k], storage.obs[k][:-1].reshape(n, -1)), (self.obs_next[k], nxt), (self.act[k], storage.act[k].reshape(n, -1)),
                    (self.rwd[k], storage.reward[..., k].reshape(n)), (self.done[k], done.to(torch.float32)))
            for dst, src in cols:
                dst[self.count:self.count + first].copy_(src[:first])
                if n > first:
                    dst[:n - first].copy_(src[first:])
        self.count = (self.count + n) % self.capacity
        self.current_size = min(self.current_size + n, self.capacity)
        if self.state is not None:   # the device counters follow: one copy, enqueued
            self.state.copy_(torch.tensor([self.count, self.current_size, self.draw], dtype=torch.int64), non_blocking=True)

    def seed(self, seed: int) -> None:
        """The 64-bit key of `sample_index`.  `draw` keeps counting, so no (seed, draw) pair comes twice."""
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"ReplayBuffer: seed must lie in [0, 2^64), got {seed}")
        self._seed = seed

    def use_device_state(self) -> torch.Tensor:
        """Keep (count, current_size, draw) in an int64 [3] device tensor as well: from here on `append` and `sample_index` read them
        there and advance them there with a one-thread launch, so both can be captured in a `torch.cuda.graph` and every replay
        appends at the advanced position and draws a fresh minibatch.  The host's ints keep advancing by the same rule with every
        eager call (nothing is synchronised) — capturing counts as one — while replays of a graph advance the tensor only:
        `pull_device_state()` reads it back.
        `add` refreshes the tensor from the host's ints.  Returns the tensor."""
        if self.state is None:
            self.state = torch.tensor([self.count, self.current_size, self.draw], dtype=torch.int64).to(self.device)
        return self.state

    def pull_device_state(self) -> None:
        """Set the host's ints from the device counters (synchronises): after replays of a captured graph."""
        if self.state is None:
            raise ValueError("ReplayBuffer: no device state (use_device_state() was not called)")
        self.count, self.current_size, self.draw = (int(v) for v in self.state.tolist())

    def append(self, storage, time_limit: str = "own") -> None:
        """`add` in ONE launch (qr_replay_add; time_limit="solved": qr_replay_add_rule): the same T * N transitions into the same ring rows
        with the same obs_next and done rule, bit for bit, for all agents and all five tensors, without a temporary."""
        rule = self._check_storage(storage, time_limit)
        n = storage.T * storage.N
        replay_add([self.tensors(k) for k in range(self.n_agents)], storage.obs, storage.final_obs, storage.act_all, storage.reward, storage.done,
                   storage.truncated, self.count, state=self.state, time_limit_rule=rule)
        self.count = (self.count + n) % self.capacity
        self.current_size = min(self.current_size + n, self.capacity)

    def sample_index(self, batch_size: int, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int64 [batch_size] pairwise distinct rows below current_size in one O(batch_size) launch (qr_replay_sample): the images of
        0 .. batch_size - 1 under the permutation of [0, current_size) keyed by (seed, draw); draw then advances.  out: an int64
        [batch_size] tensor on the buffer's device, written in place — a steady-state call then allocates nothing."""
        out = replay_sample(self.current_size, batch_size, self._seed, self.draw, out, device=self.status.device, state=self.state, status=self.status)
        self.draw += 1
        return out

    def sample(self, batch_size: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """int64 [batch_size] rows below current_size, without replacement (np.random.choice(current_size, batch_size, replace=False))."""
        batch_size = int(batch_size)
        if not 1 <= batch_size <= self.current_size:
            raise ValueError(f"cannot sample {batch_size} of {self.current_size} transitions without replacement")
        return torch.randperm(self.current_size, device=self.device, generator=generator)[:batch_size]

    def tensors(self, k: int) -> dict:
        """Agent k's five tensors, as `td3_target` / `twinq_grad` take them."""
        return {"obs": self.obs[k], "act": self.act[k], "rwd": self.rwd[k], "obs_next": self.obs_next[k], "done": self.done[k]}


def replay_add(tensors, obs, final_obs, action: torch.Tensor, reward: torch.Tensor, done: torch.Tensor, truncated: Optional[torch.Tensor],
               count: int, *, state: Optional[torch.Tensor] = None, time_limit_rule: Optional[TimeLimitRule] = None) -> None:
    """One collected horizon into the ring of a flat transition buffer in one launch (qr_replay_add).  tensors: per agent (one or two)
    a dict with obs, obs_next [capacity, D_k], act [capacity, A_k], rwd, done [capacity], contiguous float32 (`ReplayBuffer.tensors(k)`),
    written in place.  The horizon as `RolloutStorage` holds it: obs a list of [T + 1, N, D_k]; final_obs a list of [T, N, D_k] or None;
    action [T, N, sum A_k], the agents' columns side by side; reward [T, N, n_agents] float32; done [T, N, n_agents] and truncated
    [T, N] (or None) bool.  Transition j = t * N + n goes to row (count + j) % capacity; obs_next is final_obs[t, n] where it is given and
    any agent's done or truncated is set, obs[t + 1, n] elsewhere; done is agent k's own flag as 0.0 / 1.0.  The caller advances its
    counters: count = (count + T * N) % capacity, current_size = min(current_size + T * N, capacity).  state: the int64 [3] device
    counters (count, current_size, draw), read on the device instead of `count` and advanced there behind the launch.
    time_limit_rule: None, or a `TimeLimitRule` (x_lim, pos_tol, rot_tol): the same launch through qr_replay_add_rule, whose done on a
    transition with truncated set is the reference's main.py:169-173 — the agent's error in the stored obs_next is within tolerance and
    its reward is not -1 — and the own flag elsewhere.  Needs truncated and an agent 0 observation of at least three words."""
    what = "replay_add"
    if time_limit_rule is not None:
        time_limit_rule = TimeLimitRule(*time_limit_rule).check(what)
        if truncated is None:
            raise ValueError(f"{what}: the time-limit rule needs truncated")
    tensors = [dict(t) for t in tensors]
    obs = [obs] if isinstance(obs, torch.Tensor) else list(obs)
    if final_obs is not None:
        final_obs = [final_obs] if isinstance(final_obs, torch.Tensor) else list(final_obs)
    na = len(tensors)
    if na not in (1, 2) or len(obs) != na or (final_obs is not None and len(final_obs) != na):
        raise ValueError(f"{what}: one or two agents, with one obs (and final_obs) tensor per agent; got {na} buffers, {len(obs)} obs")
    b0 = tensors[0].get("obs")
    if b0 is None or b0.dim() != 2:
        raise ValueError(f"{what}: agent 0's buffer obs must be a contiguous float32 [capacity, D] tensor")
    dev, capacity = b0.device, b0.shape[0]
    if action is None or action.dim() != 3 or obs[0] is None or obs[0].dim() != 3:
        raise ValueError(f"{what}: action must be [T, N, A] and obs[k] [T + 1, N, D_k]")
    T, N, row = action.shape
    od, ad = [], []
    for k, t in enumerate(tensors):
        a = t.get("act")
        if a is None or a.dim() != 2 or t.get("obs") is None or t["obs"].dim() != 2:
            raise ValueError(f"{what}: agent {k}'s buffer obs and act must be contiguous float32 [capacity, width] tensors")
        od.append(t["obs"].shape[1])
        ad.append(a.shape[1])
    if sum(ad) != row or min(od + ad) < 1 or max(od + ad) > _lib.REPLAY_MAX_WIDTH:
        raise ValueError(f"{what}: the buffers' action widths {ad} must add up to the action row's {row}; widths lie in 1..{_lib.REPLAY_MAX_WIDTH}")
    if time_limit_rule is not None and od[0] < 3:
        raise ValueError(f"{what}: the time-limit rule reads the first three words of agent 0's observation, which has {od[0]}")
    if T < 1 or N < 1 or T * N > capacity:
        raise ValueError(f"{what}: a horizon of {T} x {N} = {T * N} transitions does not fit a buffer of {capacity}")
    f32 = torch.float32
    for k, t in enumerate(tensors):
        for name, shape in (("obs", (capacity, od[k])), ("obs_next", (capacity, od[k])), ("act", (capacity, ad[k])), ("rwd", (capacity,)), ("done", (capacity,))):
            ck.tensor(what, f"agent {k}'s buffer {name}", t.get(name), f32, shape, dev)
        ck.tensor(what, f"obs[{k}]", obs[k], f32, (T + 1, N, od[k]), dev)
        if final_obs is not None:
            ck.tensor(what, f"final_obs[{k}]", final_obs[k], f32, (T, N, od[k]), dev)
    ck.tensor(what, "action", action, f32, (T, N, row), dev)
    ck.tensor(what, "reward", reward, f32, (T, N, na), dev)
    ck.tensor(what, "done", done, torch.bool, (T, N, na), dev)
    ck.tensor(what, "truncated", truncated, torch.bool, (T, N), dev, True)
    ck.state(what, state, dev)
    count = int(count)
    if state is None and not 0 <= count < capacity:
        raise ValueError(f"{what}: count must lie in [0, {capacity}), got {count}")
    ck.require_gpu(dev)
    r = _lib.replay_add_args(tensors, obs, final_obs, action, reward, done, truncated, state=state, count=count if state is None else 0,
                             capacity=capacity, n_steps=T, n_envs=N, obs_dims=od, action_dims=ad,
                             col_offsets=[sum(ad[:k]) for k in range(na)], action_row=row)
    if time_limit_rule is None:
        _lib.launch(dev, "qr_replay_add", r)
    else:
        _lib.launch(dev, "qr_replay_add_rule", _lib.replay_add_rule_args(r, **time_limit_rule._asdict()))


def replay_sample(n: int, batch_size: int, seed: int, draw: int, out: Optional[torch.Tensor] = None, *, device=None,
                  state: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [batch_size] pairwise distinct rows in [0, n), 1 <= batch_size <= n < 2^31, in one O(batch_size) launch (qr_replay_sample):
    index[j] is the image of j under the permutation of [0, n) keyed by the 64-bit (seed, draw) — a six-round Feistel network over
    Philox4x32-10, cycle-walked into [0, n); integers only, so tests/replay_ref.py gives the same indices on the CPU.  Use a (seed, draw)
    pair once: draw counts the calls.  out: written in place (None: made on `device`, by default the current GPU).  state: the int64 [3]
    device counters; n = state[1] and draw = state[2] are then read on the device, and state[2] advances behind the launch.  status: an
    int32 [1] device tensor that the launch sets to 1 should a walk reach its cap (it cannot), or None."""
    what = "replay_sample"
    n, B, seed, draw = int(n), int(batch_size), int(seed), int(draw)
    if n >= 2 ** 31:
        raise ValueError(f"{what}: n must be below 2^31, got {n}")
    if not 1 <= B <= n:
        raise ValueError(f"cannot sample {B} of {n} transitions without replacement")
    if not 0 <= seed < 2 ** 64 or not 0 <= draw < 2 ** 64:
        raise ValueError(f"{what}: seed and draw must lie in [0, 2^64)")
    dev = torch.device("cuda" if out is None else out.device) if device is None else torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    ck.tensor(what, "out", out, torch.int64, (B,), dev, True)
    ck.state(what, state, dev)
    ck.scalar(what, "status", status, torch.int32, dev)
    ck.require_gpu(dev)
    if out is None:
        out = torch.empty(B, dtype=torch.int64, device=dev)
    _lib.launch(dev, "qr_replay_sample", _lib.replay_sample_args(out, status, state, n=n, batch=B, seed=seed, draw=draw))
    return out


def _agent_tensors(buffer_or_tensors, k: int) -> dict:
    return buffer_or_tensors.tensors(k) if isinstance(buffer_or_tensors, ReplayBuffer) else dict(buffer_or_tensors)


def _target(what: str, entry: str, make_args, actor: Optional[ActorParams], form: tuple, missing: Optional[str], critic_target: QCriticParams,
            buffer_or_tensors, k: int, index, noise, action_next, out, own) -> torch.Tensor:
    """What `td3_target` and `sac.sac_target` do alike: the transitions, the actor (`form`: _checks.actor's last three arguments) or,
    without one, `missing` (the message when a supplied tensor is), noise, action_next, the caller's `own(B, A, dev)` checks —
    which return its own keywords of `make_args` — out, and the launch of `entry`."""
    t = _agent_tensors(buffer_or_tensors, k)
    dev = critic_target.device
    D, A, H = critic_target.dims
    rows = ck.rows(what, "obs_next", t.get("obs_next"), D, dev)
    rs, ds = ck.column(what, "rwd", t.get("rwd"), rows, dev), ck.column(what, "done", t.get("done"), rows, dev)
    B = ck.index(what, index, dev, rows)
    if actor is not None:
        ck.actor(what, actor, PPO_ACTOR_DIMS, D, A, dev, *form)
    elif missing is not None:
        raise ValueError(f"{what}: {missing}")
    ck.tensor(what, "noise", noise, torch.float32, (B, A), dev, True)
    ck.tensor(what, "action_next", action_next, torch.float32, (B, A), dev, True)
    kw = own(B, A, dev)
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    else:
        ck.flat(what, "out", out, torch.float32, B, dev)
    ck.require_gpu(dev)
    if B == 0:
        return out
    b = _lib.transitions(obs_next=t["obs_next"], reward=t["rwd"], done=t["done"], index=index, batch=B, rows=rows, reward_stride=rs, done_stride=ds)
    g = make_args(eps=noise, action_next=action_next, y=out, **kw)
    p = None
    if actor is not None:
        p = actor.as_c()
        p.log_std = None
    _lib.launch(dev, entry, p, critic_target.as_c(), b, g)
    return out


def td3_target(actor_target: Optional[ActorParams], critic_target: QCriticParams, buffer_or_tensors, k: int = 0,
               index: Optional[torch.Tensor] = None, *, discount: float = 0.99, target_noise: float = 0.2, noise_clip: float = 0.5,
               max_action: float = 1.0, noise: Optional[torch.Tensor] = None, action_next: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """TD3's target values of one minibatch in one launch (qr_twinq_target; td3.py:139-154), j the minibatch position, i = index[j]:
        a'_j = clamp(actor_target(obs_next[i]) + clamp(target_noise * noise[j], +-noise_clip), +-max_action)
        y[j] = rwd[i] + discount * (1 - done[i]) * min(Q1, Q2)(obs_next[i], a'_j)
    actor_target: `ActorParams.from_td3_module(module, 0.0)` (the tanh-of-mean form in one of the three sizes of the rollout; its
    log_std is not read), or None with action_next [B, A] float32: a'_j = action_next[j] as it is.  buffer_or_tensors: a
    `ReplayBuffer` (agent k's tensors) or a dict with obs_next [rows, D], rwd, done (float32, `rows` elements, one stride).
    noise: float32 [B, A] standard-normal draws by minibatch position, None: no smoothing noise.  index: int64 [B], None: all rows
    in order.  Returns y float32 [B] (`out` given: written in place)."""
    A = critic_target.dims[1]
    return _target("td3_target", "qr_twinq_target", _lib.td3_target_args, actor_target,
                   (_lib.ACTOR_TANH_MEAN, False, "the target actor must be of MLP_Actor_TD3's form: the tanh-of-mean rule, no log_std head"),
                   f"without a target actor, action_next [B, {A}] is required" if action_next is None else None, critic_target, buffer_or_tensors,
                   k, index, noise, action_next, out,
                   lambda B, A, dev: dict(discount=discount, target_noise=target_noise, noise_clip=noise_clip, max_action=max_action))


CTDE_ACTOR_DIMS = ((15, 16, 4), (3, 4, 1))   # the Decoupled wrapper's two actors: what the centralized target kernels hold


def _ctde_actors_c(actors, log_std: bool = False) -> list:
    """The pair's QrActor structs for a centralized launch, None where an agent's actor is not given; their log_std, which these
    launches do not read, is null unless `log_std`."""
    p = [None if a is None else a.as_c() for a in actors]
    for c in p:
        if c is not None and not log_std:
            c.log_std = None
    return p


def _td3_actor(m) -> ActorParams:
    """MLP_Actor_TD3's six tensors (fc3 the mean head) as the TD3 launches take them: no log_std, which they do not read."""
    return ActorParams(*(t.data for l in (m.fc1, m.fc2, m.fc3) for t in (l.weight, l.bias)), None)


def _ctde_tensors(what: str, buffer_or_tensors, critic: QCriticParams, k: int):
    """Both agents' tensors of a two-agent `ReplayBuffer` (or a pair of dicts with obs, obs_next, act and, for agent k, rwd and done),
    their observation and action widths — which must add up to the centralized critic's — and the common row count."""
    if k not in (0, 1):
        raise ValueError(f"{what}: k must be 0 or 1 (two agents), got {k}")
    if isinstance(buffer_or_tensors, ReplayBuffer):
        if buffer_or_tensors.n_agents != 2:
            raise ValueError(f"{what}: buffer must hold two agents, it holds {buffer_or_tensors.n_agents}")
        t = [buffer_or_tensors.tensors(m) for m in range(2)]
    else:
        t = [dict(x) for x in buffer_or_tensors]
        if len(t) != 2:
            raise ValueError(f"{what}: buffer must be a two-agent ReplayBuffer or a pair of per-agent dicts")
    dev = critic.device
    for m in range(2):
        for name in ("obs_next", "act"):
            x = t[m].get(name)
            if x is None or x.dim() != 2 or x.shape[1] < 1:
                raise ValueError(f"{what}: agent {m}'s {name} must be a float32 [rows, width] tensor on {dev}")
    od, ad = [t[m]["obs_next"].shape[1] for m in range(2)], [t[m]["act"].shape[1] for m in range(2)]
    D, A, _ = critic.dims
    if sum(od) != D or sum(ad) != A:
        raise ValueError(f"{what}: the buffer's widths {od[0]}+{od[1]} / {ad[0]}+{ad[1]} do not add up to the critic's {D} / {A}")
    rows = ck.rows(what, "agent 0's obs_next", t[0]["obs_next"], od[0], dev)
    if ck.rows(what, "agent 1's obs_next", t[1]["obs_next"], od[1], dev) != rows:
        raise ValueError(f"{what}: agent 1's obs_next must have agent 0's {rows} rows")
    return t, od, ad, rows


def _target_ctde(what: str, entry: str, make_args, actors, form: tuple, critic_target: QCriticParams, buffer_or_tensors, k: int, index, noise,
                 action_next, out, own) -> torch.Tensor:
    """`_target` for the centralized critic of two agents, shared by `td3_target_ctde` and `sac.sac_target_ctde`: both agents'
    transitions, both actors (`form`: _checks.actor's last three arguments) or neither, the pairs noise and action_next, the caller's
    `own(B, widths, dev, supplied)` checks — which return its own keywords of `make_args` — out, and the launch of `entry`."""
    t, od, ad, rows = _ctde_tensors(what, buffer_or_tensors, critic_target, k)
    dev = critic_target.device
    rs, ds = ck.column(what, "rwd", t[k].get("rwd"), rows, dev), ck.column(what, "done", t[k].get("done"), rows, dev)
    B = ck.index(what, index, dev, rows)
    actors = (None, None) if actors is None else tuple(actors)
    if len(actors) != 2 or (actors[0] is None) != (actors[1] is None):
        raise ValueError(f"{what}: actors must be a pair of both agents' actors, or None for both")
    supplied = actors[0] is None
    for m in range(2):
        if not supplied:
            ck.actor(what, actors[m], PPO_ACTOR_DIMS, od[m], ad[m], dev, *form)
            if actors[m].dims != CTDE_ACTOR_DIMS[m]:
                raise ValueError(f"{what}: actor {m} must have the sizes {CTDE_ACTOR_DIMS[m]} (obs, hidden, action), got {actors[m].dims}")
    noise = ck.pair_of(what, "noise", noise, B, ad, dev)
    action_next = ck.pair_of(what, "action_next", action_next, B, ad, dev)
    if supplied and (action_next[0] is None or action_next[1] is None):
        raise ValueError(f"{what}: without actors, action_next ([B, {ad[0]}], [B, {ad[1]}]) is required")
    kw = own(B, ad, dev, supplied)
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    else:
        ck.flat(what, "out", out, torch.float32, B, dev)
    ck.require_gpu(dev)
    if B == 0:
        return out
    b = _lib.ctde_transitions(obs_next=(t[0]["obs_next"], t[1]["obs_next"]), reward=t[k]["rwd"], done=t[k]["done"], index=index, batch=B, rows=rows,
                              obs_dims=od, action_dims=ad, reward_stride=rs, done_stride=ds)
    g = make_args(eps=noise, action_next=action_next, y=out, **kw)
    _lib.launch(dev, entry, *_ctde_actors_c(actors), critic_target.as_c(), b, g)
    return out


def td3_target_ctde(actor_targets, critic_target: QCriticParams, buffer_or_tensors, k: int = 0, index: Optional[torch.Tensor] = None, *,
                    discount: float = 0.99, target_noise: float = 0.2, noise_clip: float = 0.5, max_action: float = 1.0, noise=None,
                    action_next=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """TD3's target values for the centralized (CTDE) twin critic of two agents in one launch (qr_ctde_twinq_target; td3.py:124-154),
    j the minibatch position, i = index[j], m = 0, 1:
        a'_m = clamp(actor_targets[m](obs_next_m[i]) + clamp(target_noise * noise[m][j], +-noise_clip), +-max_action)
        y[j] = rwd_k[i] + discount * (1 - done_k[i]) * min(Q1, Q2)([obs_next_0[i] | obs_next_1[i] | a'_0 | a'_1])
    critic_target: `QCriticParams.from_module(MLP_Critic_CTDE, action_dim=sum(action_dims))`.  actor_targets: the pair of
    `ActorParams.from_td3_module` of the sizes (15,16,4) and (3,4,1), or None with action_next = (a'_0 [B, A_0], a'_1 [B, A_1]) used as
    they are, for any widths whose sum the critic reads.  buffer_or_tensors: a two-agent `ReplayBuffer`, or a pair of dicts with
    obs_next, act (its width is read) and, for agent k, rwd and done.  noise: a pair of float32 [B, A_m] standard-normal draws (either
    may be None) or None.  No concatenated copy of the rows is made.  Returns y float32 [B] (`out` given: written in place)."""
    return _target_ctde("td3_target_ctde", "qr_ctde_twinq_target", _lib.ctde_td3_target_args, actor_targets,
                        (_lib.ACTOR_TANH_MEAN, False, "the target actors must be of MLP_Actor_TD3's form: the tanh-of-mean rule, no log_std head"),
                        critic_target, buffer_or_tensors, k, index, noise, action_next, out,
                        lambda B, ad, dev, supplied: dict(discount=discount, target_noise=target_noise, noise_clip=noise_clip, max_action=max_action))


def twinq_grad_ctde(critic: QCriticParams, obs, action, y: torch.Tensor, index: Optional[torch.Tensor] = None, *, grads: Optional[dict] = None,
                    stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, max_workgroups: int = 0):
    """`twinq_grad` for the centralized (CTDE) critic (qr_ctde_twinq_grad): the row [obs[0][i] | obs[1][i] | action[0][i] | action[1][i]]
    is formed inside the kernel from the two agents' tensors — no concatenated copy.  obs: a pair of contiguous float32 [rows, D_m];
    action: a pair of float32 [rows, A_m] whose rows lie one row stride apart (all columns are read); the widths must add up to the
    critic's.  y, index, grads, stats, workspace, max_workgroups and the return value: `twinq_grad`'s, as are the bits where the
    concatenated rows are given to it at the same grid."""
    what = "twinq_grad_ctde"
    dev = critic.device
    D, A, H = critic.dims
    obs, action = tuple(obs), tuple(action)
    if len(obs) != 2 or len(action) != 2:
        raise ValueError(f"{what}: obs and action must be pairs, one tensor per agent")
    for m in range(2):
        if obs[m] is None or obs[m].dim() != 2 or obs[m].shape[1] < 1:
            raise ValueError(f"{what}: obs[{m}] must be a contiguous float32 [rows, width] tensor on {dev}")
    rows = ck.rows(what, "obs[0]", obs[0], obs[0].shape[1], dev)
    if ck.rows(what, "obs[1]", obs[1], obs[1].shape[1], dev) != rows:
        raise ValueError(f"{what}: obs[1] must have obs[0]'s {rows} rows")
    strides = [ck.strided_rows(what, f"action[{m}]", a, rows, 1, dev, wider=True) for m, a in enumerate(action)]
    od, ad = [o.shape[1] for o in obs], [a.shape[1] for a in action]
    if sum(od) != D or sum(ad) != A:
        raise ValueError(f"{what}: the widths of obs {od[0]}+{od[1]} / action {ad[0]}+{ad[1]} do not add up to the critic's {D} / {A}")
    B = ck.index(what, index, dev, rows)
    ck.flat(what, "y", y, torch.float32, B, dev)
    grads, stats, workspace = _grad_outputs(what, critic.shapes, dev, B, grads, stats, workspace,
                                            lambda: twinq_workspace_bytes(critic.dims, B, max_workgroups))
    if workspace is None:
        return grads, stats
    b = _lib.ctde_transitions(obs=obs, action=action, index=index, batch=B, rows=rows, obs_dims=od, action_dims=ad, row_strides=strides)
    _lib.launch(dev, "qr_ctde_twinq_grad", critic.as_c(), b, _lib.twinq_grad_args(grads, stats, y, workspace, max_workgroups))
    return grads, stats


def twinq_workspace_bytes(dims, batch: int, max_workgroups: int = 0) -> int:
    """Bytes of workspace one `twinq_grad` call needs (qr_twinq_workspace_bytes); dims = (obs_dim, action_dim, hidden width)."""
    return _lib.workspace_bytes("qr_twinq_workspace_bytes", int(dims[0]) + int(dims[1]), dims[2], batch, max_workgroups)


def twinq_grad(critic: QCriticParams, obs: torch.Tensor, action: torch.Tensor, y: torch.Tensor, index: Optional[torch.Tensor] = None, *,
               grads: Optional[dict] = None, stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
               max_workgroups: int = 0):
    """The twin-Q regression against a given target and its gradients (qr_twinq_grad; td3.py:157-167 without the equivariant term,
    and SAC's critic loss): loss = mean_j (Q1(obs[i], action[i]) - y[j])^2 + mean_j (Q2(obs[i], action[i]) - y[j])^2, i = index[j] —
    no autograd, no copies of the minibatch's rows.  obs [rows, D] contiguous float32; action float32 [rows, >= A] whose rows lie one
    row stride apart (the critic reads the leading A columns: pass a per-agent view of wider rows as it is); y float32 [B] by
    minibatch position; index int64 [B], None: all rows in order.
    Returns (grads, stats): grads = {name: float32 tensor} for fc1_w .. fc6_b — `grads` given: overwritten in place — and stats
    float32 [4] = loss, the Q1 mse, the Q2 mse, the mean of y."""
    what = "twinq_grad"
    dev = critic.device
    D, A, H = critic.dims
    rows = ck.rows(what, "obs", obs, D, dev)
    row_stride = ck.strided_rows(what, "action", action, rows, A, dev, wider=True)
    B = ck.index(what, index, dev, rows)
    ck.flat(what, "y", y, torch.float32, B, dev)
    grads, stats, workspace = _grad_outputs(what, critic.shapes, dev, B, grads, stats, workspace,
                                            lambda: twinq_workspace_bytes(critic.dims, B, max_workgroups))
    if workspace is None:
        return grads, stats
    b = _lib.transitions(obs=obs, action=action, index=index, batch=B, rows=rows, row_stride=row_stride)
    _lib.launch(dev, "qr_twinq_grad", critic.as_c(), b, _lib.twinq_grad_args(grads, stats, y, workspace, max_workgroups))
    return grads, stats


def _critic_update_state(critic_module, buffer: ReplayBuffer, k: int, index, max_workgroups: int, tag: tuple = (), action_dim: Optional[int] = None):
    """For `td3_critic_loss`, `sac.sac_critic_loss` and their centralized forms: the live twin critic's twelve .grad tensors by name (made
    where there is none), its `QCriticParams` (action_dim: agent k's, or what the centralized form gives), and (y, workspace, stats)
    from the buffer's cache under tag + (k, B, max_workgroups)."""
    layers = [getattr(critic_module, f"fc{j}") for j in range(1, 7)]
    grads = module_grads(_lib.TWINQ_GRAD_NAMES, (t for l in layers for t in (l.weight, l.bias)))
    critic = QCriticParams.from_module(critic_module, buffer.action_dims[k] if action_dim is None else action_dim)
    B = buffer.capacity if index is None else index.numel()
    dev = critic.device

    def make():
        need = twinq_workspace_bytes(critic.dims, B, max_workgroups) // 8 if B else 0
        return (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(need, dtype=torch.float64, device=dev),
                torch.empty(4, dtype=torch.float32, device=dev))
    return grads, critic, buffer._scratch(tag + (k, B, int(max_workgroups)), make)


def td3_critic_loss(critic_module, critic_target_module, actor_target_module, buffer: ReplayBuffer, k: int = 0,
                    index: Optional[torch.Tensor] = None, *, discount: float = 0.99, target_noise: float = 0.2, noise_clip: float = 0.5,
                    max_action: float = 1.0, noise: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                    max_workgroups: int = 0) -> torch.Tensor:
    """The critic update of TD3.train, as the reference writes it, without autograd: `td3_target` on the target modules, then
    `twinq_grad` on the live `critic_module` (attributes fc1 .. fc6 — its tensors are read in place) for agent k of `buffer`; writes
    the gradients into `critic_module.fc{1..6}.{weight,bias}.grad` in place, as `loss.backward()` after `zero_grad()` leaves them.
    The defaults are the reference's (args_parse.py:44-58).  noise: the [B, A] standard-normal draws of the target policy smoothing
    (torch.randn_like in the reference), None: none.  Returns stats (stats[0] = the loss).  From the second call on with an unchanged
    B nothing is allocated: y, the workspace and stats are cached on the buffer.  The optimiser step follows on these .grad tensors:
    one `optim.PolyakAdamW` group of all twelve tensors, or torch's."""
    A = buffer.action_dims[k]
    grads, critic, (y, workspace, own_stats) = _critic_update_state(critic_module, buffer, k, index, max_workgroups)
    td3_target(_td3_actor(actor_target_module), QCriticParams.from_module(critic_target_module, A), buffer, k, index, discount=discount, target_noise=target_noise,
               noise_clip=noise_clip, max_action=max_action, noise=noise, out=y)
    _, stats = twinq_grad(critic, buffer.obs[k], buffer.act[k], y, index, grads=grads, stats=own_stats if stats is None else stats,
                          workspace=workspace, max_workgroups=max_workgroups)
    return stats


def td3_critic_loss_ctde(critic_module, critic_target_module, actor_target_modules, buffer: ReplayBuffer, k: int = 0,
                         index: Optional[torch.Tensor] = None, *, discount: float = 0.99, target_noise: float = 0.2, noise_clip: float = 0.5,
                         max_action: float = 1.0, noise=None, stats: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> torch.Tensor:
    """`td3_critic_loss` for the centralized (CTDE) critic of a two-agent `buffer`, for agent k's reward and done: `td3_target_ctde` on
    the two target actors and the target critic, then `twinq_grad_ctde` on the live `critic_module` (MLP_Critic_CTDE: fc1 .. fc6 over
    [obs_0 | obs_1 | act_0 | act_1]); fills `critic_module.fc{1..6}.{weight,bias}.grad` in place.  noise: the pair of [B, A_m]
    smoothing draws, or None.  Returns stats (stats[0] = the loss).  y, the workspace and stats are cached on the buffer under a key of
    their own: from the second call on with an unchanged B nothing is allocated.  The optimiser step stays the caller's."""
    if not isinstance(buffer, ReplayBuffer):
        raise ValueError("td3_critic_loss_ctde: buffer must be a ReplayBuffer")
    A = sum(buffer.action_dims)
    grads, critic, (y, workspace, own_stats) = _critic_update_state(critic_module, buffer, k, index, max_workgroups, ("td3_ctde",), action_dim=A)
    td3_target_ctde([_td3_actor(m) for m in actor_target_modules], QCriticParams.from_module(critic_target_module, A), buffer, k, index, discount=discount, target_noise=target_noise,
                    noise_clip=noise_clip, max_action=max_action, noise=noise, out=y)
    _, stats = twinq_grad_ctde(critic, buffer.obs, buffer.act, y, index, grads=grads, stats=own_stats if stats is None else stats,
                               workspace=workspace, max_workgroups=max_workgroups)
    return stats


def dpg_actor_workspace_bytes(actor_dims, critic_hidden: int, batch: int, max_workgroups: int = 0) -> int:
    """Bytes of workspace one `dpg_actor_grad` call needs (qr_dpg_actor_workspace_bytes); actor_dims = (obs_dim, hidden, action_dim)."""
    return _lib.workspace_bytes("qr_dpg_actor_workspace_bytes", *actor_dims, critic_hidden, batch, max_workgroups)


def dpg_actor_grad(actor: ActorParams, critic: QCriticParams, obs: torch.Tensor, obs_next: Optional[torch.Tensor] = None,
                   index: Optional[torch.Tensor] = None, *, lam_T: float = 0.4, lam_S: float = 0.3, lam_M: float = 0.6, max_action: float = 1.0,
                   noise: Optional[torch.Tensor] = None, nominal: Optional[torch.Tensor] = None, grads: Optional[dict] = None,
                   stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, max_workgroups: int = 0):
    """TD3's actor loss and its gradients (qr_dpg_actor_grad; td3.py:183-196 without the equivariant term, with
    algos/policy_regularization.py), c = clamp to +-max_action, i = index[j]:
        loss = -mean_j Q1(obs[i], c(pi(obs[i]))) + lam_T mse(c(pi(obs[i])), c(pi(obs_next[i])))
               + lam_S mse(c(pi(obs[i])), c(pi(obs[i] + noise))) + lam_M mse(c(pi(obs[i])), nominal)
    — no autograd, no copies of the minibatch's rows.  actor: MLP_Actor_TD3's six tensors as `ActorParams` (the tanh-of-mean form in
    one of the three sizes of the rollout; its log_std is not read); critic: the twin critic, of which Q1 is read.  obs, obs_next
    [rows, D] contiguous float32 (obs_next: needed when lam_T != 0); noise [D]: ONE row, needed when lam_S != 0; nominal [A]: needed
    when lam_M != 0; index int64 [B], None: all rows in order.
    Returns (grads, stats): grads = {name: float32 tensor} for fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b — `grads` given: overwritten
    in place — and stats float32 [4] = loss, the mean of Q1, the share of pi(obs)'s components outside +-max_action, the weighted sum
    of the three smoothness terms."""
    what = "dpg_actor_grad"
    dev = critic.device
    D, A, H = critic.dims
    shapes = ck.actor(what, actor, PPO_ACTOR_DIMS, D, A, dev, _lib.ACTOR_TANH_MEAN, False, "the actor must be of MLP_Actor_TD3's form: the tanh-of-mean rule, no log_std head")
    ck.nonneg(what, ck.LAMS, lam_T, lam_S, lam_M, max_action)
    rows = ck.rows(what, "obs", obs, D, dev)
    if lam_T != 0 and ck.rows(what, "obs_next", obs_next, D, dev) != rows:
        raise ValueError(f"{what}: obs_next must have obs's {rows} rows")
    if (lam_S != 0 and noise is None) or (lam_M != 0 and nominal is None):
        raise ValueError(f"{what}: noise [{D}] is required when lam_S != 0, nominal [{A}] when lam_M != 0")
    ck.flat(what, "noise", noise, torch.float32, D, dev, True)
    ck.flat(what, "nominal", nominal, torch.float32, A, dev, True)
    B = ck.index(what, index, dev, rows)
    grads, stats, workspace = _grad_outputs(what, shapes, dev, B, grads, stats, workspace,
                                            lambda: dpg_actor_workspace_bytes(actor.dims, H, B, max_workgroups), size_given=False)
    if workspace is None:
        return grads, stats
    b = _lib.transitions(obs=obs, obs_next=obs_next if lam_T != 0 else None, index=index, batch=B, rows=rows)
    g = _lib.dpg_grad_args(grads, stats, noise if lam_S != 0 else None, nominal if lam_M != 0 else None, workspace, lam_T=lam_T, lam_S=lam_S,
                           lam_M=lam_M, max_action=max_action, max_workgroups=max_workgroups)
    p = actor.as_c()
    p.log_std = None
    _lib.launch(dev, "qr_dpg_actor_grad", p, critic.as_c(), b, g)
    return grads, stats


def td3_actor_loss(actor_module, critic_module, buffer: ReplayBuffer, k: int = 0, index: Optional[torch.Tensor] = None, *,
                   lam_T: float = 0.4, lam_S: float = 0.3, lam_M: float = 0.6, max_action: float = 1.0, noise: Optional[torch.Tensor] = None,
                   nominal: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> torch.Tensor:
    """The actor update of TD3.train, as the reference writes it, without autograd: `dpg_actor_grad` on the live `actor_module`
    (attributes fc1, fc2, fc3) and `critic_module` (fc1 .. fc6, of which Q1 is read) for agent k of `buffer`; writes the gradients into
    `actor_module.fc{1,2,3}.{weight,bias}.grad` in place, as `loss.backward()` after `zero_grad()` leaves them.  The defaults are the
    reference's (args_parse.py); noise: policy_regularization's ONE [D] row of N(0, 0.05) draws; nominal: its [A] hover action.
    Returns stats (stats[0] = the loss).  From the second call on with an unchanged B nothing is allocated: the workspace and stats
    are cached on the buffer.  The optimiser step follows on these .grad tensors (`optim.DeviceAdamW`, or torch's), then
    `soft_update`."""
    grads = _actor_grads(actor_module)
    actor = _td3_actor(actor_module)
    critic = QCriticParams.from_module(critic_module, buffer.action_dims[k])
    workspace, own_stats = buffer._actor_scratch("actor", k, index, max_workgroups, critic.device,
                                                 lambda B: dpg_actor_workspace_bytes(actor.dims, critic.dims[2], B, max_workgroups))
    _, stats = dpg_actor_grad(actor, critic, buffer.obs[k], buffer.obs_next[k], index, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M,
                              max_action=max_action, noise=noise, nominal=nominal, grads=grads, stats=own_stats if stats is None else stats,
                              workspace=workspace, max_workgroups=max_workgroups)
    return stats


def dpg_actor_workspace_bytes_ctde(k: int, critic_hidden: int, batch: int, max_workgroups: int = 0) -> int:
    """Bytes of workspace one `dpg_actor_grad_ctde` call needs for agent k (qr_ctde_dpg_actor_workspace_bytes): `dpg_actor_workspace_bytes`'
    figure for CTDE_ACTOR_DIMS[k]."""
    return _lib.workspace_bytes("qr_ctde_dpg_actor_workspace_bytes", k, critic_hidden, batch, max_workgroups)


_TD3_FORM = (_lib.ACTOR_TANH_MEAN, False, "the actors must be of MLP_Actor_TD3's form: the tanh-of-mean rule, no log_std head")


def _ctde_actor_launch(what: str, actors, critic: QCriticParams, obs, obs_next, index, k, action_other, lam_T, lam_S, lam_M, max_action, noise, nominal,
                       form=_TD3_FORM):
    """`dpg_actor_grad_ctde`'s and `sac.sac_actor_grad_ctde`'s checks up to the outputs (form: what `_checks.actor` asks of both actors):
    returns (shapes of agent k's tensors, B, rows, the four widths, obs_next[k])."""
    dev = critic.device
    D, A, H = critic.dims
    if k not in (0, 1):
        raise ValueError(f"{what}: k must be 0 or 1 (two agents), got {k}")
    o = 1 - k
    actors = tuple(actors) if actors is not None else ()
    if len(actors) != 2 or actors[k] is None:
        raise ValueError(f"{what}: actors must be a pair, one entry per agent; agent {k}'s is required")
    if (actors[o] is None) == (action_other is None):
        raise ValueError(f"{what}: give either agent {o}'s actor or action_other, not " + ("both" if action_other is not None else "neither"))
    obs = tuple(obs) if obs is not None else ()
    if len(obs) != 2:
        raise ValueError(f"{what}: obs must be a pair, one tensor per agent")
    for m in range(2):
        if obs[m] is None or obs[m].dim() != 2 or obs[m].shape[1] < 1:
            raise ValueError(f"{what}: obs[{m}] must be a contiguous float32 [rows, width] tensor on {dev}")
    od = [x.shape[1] for x in obs]
    rows = ck.rows(what, "obs[0]", obs[0], od[0], dev)
    if ck.rows(what, "obs[1]", obs[1], od[1], dev) != rows:
        raise ValueError(f"{what}: obs[1] must have obs[0]'s {rows} rows")
    B = ck.index(what, index, dev, rows)
    ad = [0, 0]
    ad[k] = actors[k].dims[2]
    if action_other is not None:
        ck.tensor(what, "action_other", action_other, torch.float32, (B, "width"), dev)
        if action_other.shape[1] < 1:
            raise ValueError(f"{what}: action_other must hold at least one column")
        ad[o] = action_other.shape[1]
    else:
        ad[o] = actors[o].dims[2]
    if sum(od) != D or sum(ad) != A:
        raise ValueError(f"{what}: the widths of obs {od[0]}+{od[1]} / action {ad[0]}+{ad[1]} do not add up to the critic's {D} / {A}")
    shapes = None
    for m in (k, o):
        if actors[m] is None:
            continue
        s = ck.actor(what, actors[m], PPO_ACTOR_DIMS, od[m], ad[m], dev, *form)
        if actors[m].dims != CTDE_ACTOR_DIMS[m]:
            raise ValueError(f"{what}: actor {m} must have the sizes {CTDE_ACTOR_DIMS[m]} (obs, hidden, action), got {actors[m].dims}")
        shapes = s if m == k else shapes
    ck.nonneg(what, ck.LAMS, lam_T, lam_S, lam_M, max_action)
    nxt = None
    if lam_T != 0:
        nxt = tuple(obs_next)[k] if obs_next is not None and len(tuple(obs_next)) == 2 else None
        if nxt is None:
            raise ValueError(f"{what}: obs_next must be a pair whose entry {k} is given when lam_T != 0")
        if ck.rows(what, f"obs_next[{k}]", nxt, od[k], dev) != rows:
            raise ValueError(f"{what}: obs_next[{k}] must have obs's {rows} rows")
    if (lam_S != 0 and noise is None) or (lam_M != 0 and nominal is None):
        raise ValueError(f"{what}: noise [{od[k]}] is required when lam_S != 0, nominal [{ad[k]}] when lam_M != 0")
    ck.flat(what, "noise", noise, torch.float32, od[k], dev, True)
    ck.flat(what, "nominal", nominal, torch.float32, ad[k], dev, True)
    return shapes, B, rows, od, ad, nxt


def dpg_actor_grad_ctde(actors, critic: QCriticParams, obs, obs_next=None, index: Optional[torch.Tensor] = None, *, k: int = 0,
                        action_other: Optional[torch.Tensor] = None, lam_T: float = 0.4, lam_S: float = 0.3, lam_M: float = 0.6,
                        max_action: float = 1.0, noise: Optional[torch.Tensor] = None, nominal: Optional[torch.Tensor] = None,
                        grads: Optional[dict] = None, stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                        max_workgroups: int = 0):
    """Agent k's TD3 actor loss under the centralized (CTDE) critic of two agents and its gradients (qr_ctde_dpg_actor_grad; td3.py:180-196
    without the equivariant term, with algos/policy_regularization.py), c = clamp to +-max_action, i = index[j], a_m = c(pi_m(obs[m][i])):
        loss_k = -mean_j Q1([obs[0][i] | obs[1][i] | a_0 | a_1]) + lam_T mse(a_k, c(pi_k(obs_next[k][i])))
                 + lam_S mse(a_k, c(pi_k(obs[k][i] + noise))) + lam_M mse(a_k, nominal)
    — no autograd, nothing concatenated.  actors: the pair of `ActorParams` of the sizes CTDE_ACTOR_DIMS; the other agent's runs forward
    only inside the kernel and gets NO gradient (the reference leaves one in its .grad, which that agent zeroes before reading).  Or
    actors[1 - k] None with action_other float32 [B, A_other] by minibatch position, used as it is (no clamp): then the other agent's
    widths are free as long as all four add up to the critic's.  obs, obs_next: pairs of contiguous float32 [rows, D_m]; obs_next[k] is
    needed when lam_T != 0, obs_next[1 - k] never.  noise [D_k], nominal [A_k], index, grads, stats, workspace, max_workgroups and
    the return value (grads of agent k's six tensors, stats [4]): `dpg_actor_grad`'s."""
    what = "dpg_actor_grad_ctde"
    dev = critic.device
    shapes, B, rows, od, ad, nxt = _ctde_actor_launch(what, actors, critic, obs, obs_next, index, k, action_other, lam_T, lam_S, lam_M, max_action,
                                                      noise, nominal)
    grads, stats, workspace = _grad_outputs(what, shapes, dev, B, grads, stats, workspace,
                                            lambda: dpg_actor_workspace_bytes_ctde(k, critic.dims[2], B, max_workgroups), size_given=False)
    if workspace is None:
        return grads, stats
    b = _lib.ctde_transitions(obs=obs, obs_next=(nxt, None) if k == 0 else (None, nxt), index=index, batch=B, rows=rows, obs_dims=od, action_dims=ad)
    g = _lib.ctde_dpg_grad_args(grads, stats, noise if lam_S != 0 else None, nominal if lam_M != 0 else None, workspace, agent=k,
                                action_other=action_other, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M, max_action=max_action, max_workgroups=max_workgroups)
    _lib.launch(dev, "qr_ctde_dpg_actor_grad", *_ctde_actors_c(actors), critic.as_c(), b, g)
    return grads, stats


def _actor_grads(actor_module) -> dict:
    """The live actor's six .grad tensors by name, made where there is none."""
    return module_grads(_lib.DPG_GRAD_NAMES, (t for l in (actor_module.fc1, actor_module.fc2, actor_module.fc3) for t in (l.weight, l.bias)))


def td3_actor_loss_ctde(actor_modules, critic_module, buffer: ReplayBuffer, k: int = 0, index: Optional[torch.Tensor] = None, *,
                        lam_T: float = 0.4, lam_S: float = 0.3, lam_M: float = 0.6, max_action: float = 1.0, noise: Optional[torch.Tensor] = None,
                        nominal: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> torch.Tensor:
    """`td3_actor_loss` for agent k of a two-agent `buffer` under the centralized (CTDE) critic: `dpg_actor_grad_ctde` on the two live
    actors (attributes fc1, fc2, fc3) and `critic_module` (MLP_Critic_CTDE, of which Q1 is read); fills
    `actor_modules[k].fc{1,2,3}.{weight,bias}.grad` in place, as `loss.backward()` after `zero_grad()` leaves them, and does not touch
    `actor_modules[1 - k]` (neither its tensors nor its .grad).  noise, nominal: agent k's.  Returns stats (stats[0] = the loss).  The
    workspace and stats are cached on the buffer under a key of their own: from the second call on with an unchanged B nothing is
    allocated.  The optimiser step stays the caller's."""
    what = "td3_actor_loss_ctde"
    if not isinstance(buffer, ReplayBuffer) or buffer.n_agents != 2:
        raise ValueError(f"{what}: buffer must be a two-agent ReplayBuffer")
    if k not in (0, 1):
        raise ValueError(f"{what}: k must be 0 or 1 (two agents), got {k}")
    actor_modules = tuple(actor_modules)
    if len(actor_modules) != 2:
        raise ValueError(f"{what}: actor_modules must be the pair of both agents' actors")
    grads = _actor_grads(actor_modules[k])
    critic = QCriticParams.from_module(critic_module, sum(buffer.action_dims))
    workspace, own_stats = buffer._actor_scratch("actor_ctde", k, index, max_workgroups, critic.device,
                                                 lambda B: dpg_actor_workspace_bytes_ctde(k, critic.dims[2], B, max_workgroups))
    _, stats = dpg_actor_grad_ctde([_td3_actor(m) for m in actor_modules], critic, buffer.obs, buffer.obs_next, index, k=k, lam_T=lam_T, lam_S=lam_S,
                                   lam_M=lam_M, max_action=max_action, noise=noise, nominal=nominal, grads=grads,
                                   stats=own_stats if stats is None else stats, workspace=workspace, max_workgroups=max_workgroups)
    return stats


def _tensors_of(x):
    """The tensors of a module (its parameters, in order), of a sequence of modules, or a sequence of tensors as it is."""
    if isinstance(x, torch.nn.Module):
        return [p.data for p in x.parameters()]
    out = []
    for e in x:
        out += [p.data for p in e.parameters()] if isinstance(e, torch.nn.Module) else [e]
    return out


def soft_update(params, targets, tau: float = 0.005) -> None:
    """TD3's soft target update (td3.py:207-211) of up to 24 tensors in ONE launch (qr_soft_update), in place on the targets:
        target = tau * param + (1 - tau) * target
    with the bits of the reference's `target_param.data.copy_(tau * param.data + (1 - tau) * target_param.data)`.  params, targets: a
    module, a sequence of modules (their parameters in order: `soft_update([critic, actor], [critic_t, actor_t])`) or a sequence of
    tensors, pairwise of equal element counts; contiguous float32 on one GPU."""
    what = "soft_update"
    ps, ts = _tensors_of(params), _tensors_of(targets)
    if len(ps) != len(ts) or not 1 <= len(ps) <= _lib.SOFT_UPDATE_MAX:
        raise ValueError(f"{what}: needs 1..{_lib.SOFT_UPDATE_MAX} (param, target) pairs, got {len(ps)} params and {len(ts)} targets")
    if not 0.0 <= float(tau) <= 1.0:
        raise ValueError(f"{what}: tau must lie in [0, 1], got {tau}")
    dev = ts[0].device
    for k, (p, t) in enumerate(zip(ps, ts)):
        for name, x in (("param", p), ("target", t)):
            if x.dtype != torch.float32 or x.device != dev or not x.is_contiguous() or x.numel() < 1:
                raise ValueError(f"{what}: {name} {k} must be a non-empty contiguous float32 tensor on {dev}")
        if p.numel() != t.numel():
            raise ValueError(f"{what}: pair {k} has {p.numel()} and {t.numel()} elements")
        if p.data_ptr() == t.data_ptr():
            raise ValueError(f"{what}: pair {k}: the target is its own param")
    ck.require_gpu(dev)
    _lib.launch(dev, "qr_soft_update", _lib.soft_update_args(ps, ts, tau))
