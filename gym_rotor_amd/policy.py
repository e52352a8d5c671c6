"""Actor parameters for the policy-in-the-loop rollout (`QuadVecEnv.rollout_actor`), critic parameters for the on-device values
of a horizon (`RolloutStorage.compute_values`), the PPO actor loss and its gradients for one minibatch (`ppo_actor_grad`,
`actor_loss`), the PPO critic loss and its gradients for one minibatch (`ppo_critic_grad`, `critic_loss`).

The networks are the reference's MLP actors: `MLP_Actor_PPO` (algos/ppo/ppo_mlp.py:6-58: fc1 -> relu
-> fc2 -> relu -> mean_linear -> tanh, plus a state-independent `log_std`), `MLP_Actor_TD3`
(algos/td3/td3_mlp.py:5-34: the same with fc3 as the mean head and the exploration std) and
`MLP_Actor_SAC` (algos/sac/sac_mlp.py:16-82: mean and log_std heads, tanh applied to the sample);
sizes are the reference's
defaults (args_parse.py:40 `actor_hidden_dim=[16, 4]`, obs/action dims of the wrappers).  The
tensors are used by the kernel in place, in torch.nn.Linear layout — `ActorParams.from_module`
takes a live module, so an optimiser step is seen by the next rollout without any copy.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _checks as ck
from . import _lib

# (obs_dim, hidden_dim, action_dim) per agent: main.py:68-73 + args_parse.py:40
ACTOR_DIMS = {"coupled": ((23, 16, 4),), "decoupled": ((15, 16, 4), (3, 4, 1))}


@dataclass
class ActorParams:
    fc1_w: torch.Tensor
    fc1_b: torch.Tensor
    fc2_w: torch.Tensor
    fc2_b: torch.Tensor
    mean_w: torch.Tensor
    mean_b: torch.Tensor
    log_std: Optional[torch.Tensor]               # [A] state-independent log std (PPO; TD3: log exploration std)
    log_std_w: Optional[torch.Tensor] = None      # [A, H] \ state-dependent log_std head (SAC); log_std is then None
    log_std_b: Optional[torch.Tensor] = None      # [A]    /
    squash: int = _lib.ACTOR_TANH_MEAN            # TANH_MEAN: tanh(mean) + noise, clamp; TANH_SAMPLE: tanh(mean + noise)

    NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std", "log_std_w", "log_std_b")

    @property
    def dims(self):
        return (self.fc1_w.shape[1], self.fc1_w.shape[0], self.mean_w.shape[0])

    @classmethod
    def from_module(cls, actor) -> "ActorParams":
        """From a reference-style actor module (attributes fc1, fc2, mean_linear, log_std)."""
        return cls(actor.fc1.weight.data, actor.fc1.bias.data, actor.fc2.weight.data, actor.fc2.bias.data,
                   actor.mean_linear.weight.data, actor.mean_linear.bias.data, actor.log_std.data.reshape(-1))

    @classmethod
    def from_sac_module(cls, actor) -> "ActorParams":
        """From the reference's SAC actor (algos/sac/sac_mlp.py:16-82: fc1, fc2, mean_linear, log_std_linear);
        rollout_actor then does MLP_Actor_SAC.sample: action = tanh(mean + exp(clamp(log_std, -20, 2)) eps)."""
        return cls(actor.fc1.weight.data, actor.fc1.bias.data, actor.fc2.weight.data, actor.fc2.bias.data,
                   actor.mean_linear.weight.data, actor.mean_linear.bias.data, None,
                   actor.log_std_linear.weight.data, actor.log_std_linear.bias.data, _lib.ACTOR_TANH_SAMPLE)

    @classmethod
    def from_td3_module(cls, actor, explor_noise_std: float) -> "ActorParams":
        """From the reference's TD3 actor (algos/td3/td3_mlp.py:5-34: fc1, fc2, fc3, tanh).  TD3.choose_action
        (td3.py:82-96) is clip(actor(obs) + N(0, explor_noise_std)) — the PPO path with mean_linear = fc3
        and log_std = log(explor_noise_std); for explor_noise_std = 0 call rollout_actor(deterministic=True)."""
        import math
        A = actor.fc3.weight.shape[0]
        ls = math.log(explor_noise_std) if explor_noise_std > 0 else -30.0
        return cls(actor.fc1.weight.data, actor.fc1.bias.data, actor.fc2.weight.data, actor.fc2.bias.data,
                   actor.fc3.weight.data, actor.fc3.bias.data,
                   torch.full((A,), ls, dtype=torch.float32, device=actor.fc3.weight.device))

    @classmethod
    def random(cls, obs_dim: int, hidden: int, action_dim: int, device, generator=None, log_std: float = 0.0) -> "ActorParams":
        """Same initial distribution as the reference module: torch.nn.Linear's default
        U(+-1/sqrt(fan_in)), mean_linear weight x0.1 and bias 0 (ppo_mlp.py:26-28)."""
        def lin(o, i, wscale=1.0, bscale=1.0):
            k = i ** -0.5
            w = (torch.rand(o, i, device=device, generator=generator) * 2 - 1) * k * wscale
            b = (torch.rand(o, device=device, generator=generator) * 2 - 1) * k * bscale
            return w, b
        w1, b1 = lin(hidden, obs_dim)
        w2, b2 = lin(hidden, hidden)
        w3, b3 = lin(action_dim, hidden, 0.1, 0.0)
        return cls(w1, b1, w2, b2, w3, b3, torch.full((action_dim,), float(log_std), device=device))

    def check(self, dims, device):
        if self.dims != tuple(dims):
            raise ValueError(f"actor sizes {self.dims} do not match {tuple(dims)} (obs, hidden, action)")
        shapes = {"fc1_w": (dims[1], dims[0]), "fc1_b": (dims[1],), "fc2_w": (dims[1], dims[1]), "fc2_b": (dims[1],),
                  "mean_w": (dims[2], dims[1]), "mean_b": (dims[2],), "log_std": (dims[2],),
                  "log_std_w": (dims[2], dims[1]), "log_std_b": (dims[2],)}
        if (self.log_std_w is None) != (self.log_std_b is None) or (self.log_std is None and self.log_std_w is None):
            raise ValueError("actor needs either log_std or the (log_std_w, log_std_b) head")
        if self.squash not in (_lib.ACTOR_TANH_MEAN, _lib.ACTOR_TANH_SAMPLE):
            raise ValueError("actor.squash must be ACTOR_TANH_MEAN or ACTOR_TANH_SAMPLE")
        for n in self.NAMES:
            t = getattr(self, n)
            if t is None:
                continue
            if tuple(t.shape) != shapes[n] or t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
                raise ValueError(f"actor tensor {n} must be a contiguous float32 {shapes[n]} tensor on {device}")

    def as_c(self) -> _lib.QrActor:
        q = _lib.QrActor()
        for n in self.NAMES:
            t = getattr(self, n)
            setattr(q, n, None if t is None else t.data_ptr())
        q.obs_dim, q.hidden_dim, q.action_dim = self.dims
        q.squash = int(self.squash)
        return q


@dataclass
class CriticParams:
    """One agent's critic for `RolloutStorage.compute_values`: the reference's `MLP_Critic` / `MLP_Critic_CTDE`
    (algos/ppo/ppo_mlp.py:64-126: fc1 -> tanh -> fc2 -> tanh -> fc3), any input width up to 24 and hidden width up to 64.
    The tensors are the module's own (contiguous float32, torch.nn.Linear layout), used by the kernel in place.
    inputs: which agents' observation rows form the input row, in order — (0,) or (1,): that agent's own row (MLP_Critic);
    (0, 1): both rows concatenated (MLP_Critic_CTDE's torch.cat)."""
    fc1_w: torch.Tensor
    fc1_b: torch.Tensor
    fc2_w: torch.Tensor
    fc2_b: torch.Tensor
    fc3_w: torch.Tensor
    fc3_b: torch.Tensor
    inputs: tuple = (0,)

    NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")

    def __post_init__(self):
        self.inputs = tuple(int(i) for i in self.inputs)
        if self.inputs not in ((0,), (1,), (0, 1)):
            raise ValueError(f"critic inputs must be (0,), (1,) or (0, 1), got {self.inputs}")
        if self.fc1_w.dim() != 2:
            raise ValueError("critic tensor fc1_w must be [hidden, in]")
        hidden, din = self.fc1_w.shape
        if not 1 <= din <= _lib.CRITIC_MAX_IN or not 1 <= hidden <= _lib.CRITIC_MAX_HIDDEN:
            raise ValueError(f"critic sizes in = {din}, hidden = {hidden} are outside 1..{_lib.CRITIC_MAX_IN} / 1..{_lib.CRITIC_MAX_HIDDEN}")
        shapes = {"fc1_w": (hidden, din), "fc1_b": (hidden,), "fc2_w": (hidden, hidden), "fc2_b": (hidden,), "fc3_w": (1, hidden), "fc3_b": (1,)}
        for n in self.NAMES:
            t = getattr(self, n)
            if tuple(t.shape) != shapes[n] or t.dtype != torch.float32 or t.device != self.fc1_w.device or not t.is_contiguous():
                raise ValueError(f"critic tensor {n} must be a contiguous float32 {shapes[n]} tensor on {self.fc1_w.device}, "
                                 f"got {t.dtype} {tuple(t.shape)} on {t.device}")

    @property
    def dims(self):
        """(input width, hidden width)"""
        return (self.fc1_w.shape[1], self.fc1_w.shape[0])

    @property
    def device(self):
        return self.fc1_w.device

    @classmethod
    def from_module(cls, critic, inputs=(0,)) -> "CriticParams":
        """From a module shaped like the reference's critics (attributes fc1, fc2, fc3)."""
        return cls(critic.fc1.weight.data, critic.fc1.bias.data, critic.fc2.weight.data, critic.fc2.bias.data,
                   critic.fc3.weight.data, critic.fc3.bias.data, inputs)

    def as_c(self, row_widths: Sequence[int]) -> _lib.QrCritic:
        """The launch struct for observation rows of these widths (one per agent): in0 / in1 are the widths of the rows this
        critic reads, 0 for the others."""
        take = [int(row_widths[k]) if k in self.inputs and k < len(row_widths) else 0 for k in range(2)]
        if max(self.inputs) >= len(row_widths) or sum(take) != self.dims[0]:
            raise ValueError(f"critic with inputs {self.inputs} reads {self.dims[0]} columns, the observation rows are {list(row_widths)} wide")
        q = _lib.QrCritic()
        for n in self.NAMES:
            setattr(q, n, getattr(self, n).data_ptr())
        q.in0, q.in1 = take
        q.hidden_dim = self.dims[1]
        return q


@dataclass
class QCriticParams:
    """One agent's twin critic for the TD3 critic half (`td3.td3_target`, `td3.twinq_grad`): the reference's TD3 / SAC `MLP_Critic`
    (algos/td3/td3_mlp.py:36-99: Q1 = fc3(relu(fc2(relu(fc1(sa))))), Q2 = fc6(relu(fc5(relu(fc4(sa))))), sa = the observation row
    followed by the action row), obs_dim + action_dim up to 28 and hidden width up to 64.  The twelve tensors are the module's own
    (contiguous float32, torch.nn.Linear layout), used by the kernels in place.  action_dim: how many of fc1's input columns are
    the action's (the trailing ones)."""
    fc1_w: torch.Tensor
    fc1_b: torch.Tensor
    fc2_w: torch.Tensor
    fc2_b: torch.Tensor
    fc3_w: torch.Tensor
    fc3_b: torch.Tensor
    fc4_w: torch.Tensor
    fc4_b: torch.Tensor
    fc5_w: torch.Tensor
    fc5_b: torch.Tensor
    fc6_w: torch.Tensor
    fc6_b: torch.Tensor
    action_dim: int = 4

    NAMES = _lib.TWINQ_GRAD_NAMES

    def __post_init__(self):
        self.action_dim = int(self.action_dim)
        if self.fc1_w.dim() != 2:
            raise ValueError("critic tensor fc1_w must be [hidden, obs_dim + action_dim]")
        hidden, din = self.fc1_w.shape
        if not 2 <= din <= _lib.QCRITIC_MAX_IN or not 1 <= hidden <= _lib.QCRITIC_MAX_HIDDEN:
            raise ValueError(f"twin critic sizes in = {din}, hidden = {hidden} are outside 2..{_lib.QCRITIC_MAX_IN} / 1..{_lib.QCRITIC_MAX_HIDDEN}")
        if not 1 <= self.action_dim < din:
            raise ValueError(f"twin critic: action_dim = {self.action_dim} must leave at least one observation column of the {din} inputs")
        for n, s in self.shapes.items():
            t = getattr(self, n)
            if tuple(t.shape) != s or t.dtype != torch.float32 or t.device != self.fc1_w.device or not t.is_contiguous():
                raise ValueError(f"critic tensor {n} must be a contiguous float32 {s} tensor on {self.fc1_w.device}, "
                                 f"got {t.dtype} {tuple(t.shape)} on {t.device}")

    @property
    def shapes(self) -> dict:
        hidden, din = self.fc1_w.shape
        one = {"1_w": (hidden, din), "1_b": (hidden,), "2_w": (hidden, hidden), "2_b": (hidden,), "3_w": (1, hidden), "3_b": (1,)}
        return {n: one[f"{(int(n[2]) - 1) % 3 + 1}{n[3:]}"] for n in self.NAMES}

    @property
    def dims(self):
        """(obs_dim, action_dim, hidden width)"""
        return (self.fc1_w.shape[1] - self.action_dim, self.action_dim, self.fc1_w.shape[0])

    @property
    def device(self):
        return self.fc1_w.device

    @classmethod
    def from_module(cls, critic, action_dim: int) -> "QCriticParams":
        """From a module shaped like the reference's twin critic (attributes fc1 .. fc6)."""
        layers = [getattr(critic, f"fc{k}") for k in range(1, 7)]
        return cls(*[t for l in layers for t in (l.weight.data, l.bias.data)], action_dim)

    def as_c(self) -> _lib.QrQCritic:
        q = _lib.QrQCritic()
        for n in self.NAMES:
            setattr(q, n, getattr(self, n).data_ptr())
        q.obs_dim, q.action_dim, q.hidden_dim = self.dims
        q.reserved0 = 0
        return q


def _critic_launch_args(critic: CriticParams, rows, n_rows: int, value: torch.Tensor, what: str):
    dev = value.device
    ck.require_gpu(dev)
    if critic.device != dev:
        raise ValueError(f"{what}: the critic's tensors are on {critic.device}, the values on {dev}")
    rows, widths = ck.obs_rows(what, rows, n_rows, dev)
    q = critic.as_c(widths)
    return q, (_lib.ptr(rows[0]) if q.in0 else None), (_lib.ptr(rows[1]) if q.in1 else None)


def critic_values(critic: CriticParams, obs, value: torch.Tensor) -> None:
    """value.flatten()[i] = V(row i) in one launch (qr_critic_values).  obs: the per-agent observation row tensors [.., D_k]
    (contiguous float32; an agent the critic does not read may be None); value: float32, one element per row, with ONE element
    stride — e.g. `storage.value[..., k]`."""
    if value.dtype != torch.float32:
        raise ValueError("critic_values: value must be float32")
    n_rows, stride = value.numel(), ck.element_stride("critic_values", "value", value)
    q, p0, p1 = _critic_launch_args(critic, obs, n_rows, value, "critic_values")
    if n_rows == 0:   # nothing to launch (and an empty tensor has no address to pass)
        return
    _lib.launch(value.device, "qr_critic_values", q, p0, p1, n_rows, value.data_ptr(), stride)


def critic_next_values(critic: CriticParams, final_obs, done: torch.Tensor, truncated: Optional[torch.Tensor], value: torch.Tensor,
                       next_value: torch.Tensor) -> None:
    """next_value[t, n] = V(final_obs[t, n]) where the env was re-sampled in step t (any agent's done, or truncated), value[t+1, n]
    elsewhere, in one launch (qr_critic_next_values).  final_obs: per-agent [T, N, D_k]; done [T, N, n_agents] bool / uint8;
    truncated [T, N] or None; value [T+1, N] and next_value [T, N] float32 with the same single element stride."""
    if next_value.dim() != 2 or value.dim() != 2:
        raise ValueError("critic_next_values: value must be [T+1, N] and next_value [T, N]")
    T, N = next_value.shape
    dev = next_value.device
    if value.dtype != torch.float32 or next_value.dtype != torch.float32 or value.device != dev or tuple(value.shape) != (T + 1, N):
        raise ValueError(f"critic_next_values: value must be float32 [{T + 1}, {N}] and next_value float32 [{T}, {N}] on one device")
    stride = ck.element_stride("critic_next_values", "next_value", next_value)
    if T * N > 1 and ck.element_stride("critic_next_values", "value", value) != stride:
        raise ValueError("critic_next_values: value and next_value must have the same element stride")
    n_agents = ck.reset_flags("critic_next_values", done, truncated, T, N, dev)
    q, p0, p1 = _critic_launch_args(critic, final_obs, T * N, next_value, "critic_next_values")
    if T >= 1 and N == 0:
        return
    _lib.launch(dev, "qr_critic_next_values", q, p0, p1, done.data_ptr(), n_agents, _lib.ptr(truncated), T, N, value.data_ptr(),
                next_value.data_ptr(), stride)


# ----------------------------------------------------------------------------------------------------------------
# the actor half of a PPO minibatch update (qr_ppo_actor_grad)
# ----------------------------------------------------------------------------------------------------------------
PPO_ACTOR_DIMS = tuple(d for dims in ACTOR_DIMS.values() for d in dims)   # the sizes qr_ppo_actor_grad is built for
_GRAD_SHAPES = lambda D, H, A: {"fc1_w": (H, D), "fc1_b": (H,), "fc2_w": (H, H), "fc2_b": (H,), "mean_w": (A, H), "mean_b": (A,), "log_std": (A,)}


def ppo_workspace_bytes(dims, batch: int, max_workgroups: int = 0) -> int:
    """Bytes of workspace one `ppo_actor_grad` launch needs (qr_ppo_actor_workspace_bytes)."""
    return _lib.workspace_bytes("qr_ppo_actor_workspace_bytes", dims[0], dims[1], dims[2], batch, max_workgroups)


def module_grads(names, params) -> dict:
    """How the "on live modules" wrappers start: each parameter's .grad, made (zeros) where there is none or it is not contiguous —
    what `loss.backward()` after `zero_grad()` leaves to write into.  Returns {name: p.grad} over `names` (parameters past the
    names get their .grad too)."""
    params = list(params)
    for p in params:
        if p.grad is None or not p.grad.is_contiguous():
            p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return {n: p.grad for n, p in zip(names, params)}


def _grad_outputs(what: str, shapes: dict, dev, B: int, grads, stats, workspace, workspace_bytes, size_given: bool = True, n_stats: int = 4):
    """How the gradient functions (ppo_actor_grad, ppo_critic_grad, td3.twinq_grad, td3.dpg_actor_grad, sac.sac_actor_grad) end their checks:
    `grads` ({name: tensor} over `shapes`) and `stats` [n_stats] made or checked, the GPU-only error, B == 0, and the workspace made from
    `workspace_bytes()` or checked (size_given: the library is asked for the size beside a given workspace too, so a max_workgroups
    it refuses is reported under the size query's name).  Returns (grads, stats, workspace); workspace None: B == 0, there is nothing
    to launch (and an empty tensor has no address to pass) — grads and stats are zero-filled and the caller returns them."""
    if grads is None:
        grads = {n: torch.empty(s, dtype=torch.float32, device=dev) for n, s in shapes.items()}
    ck.named(what, "grads[{!r}]", grads, shapes, dev, by_numel=True)
    if stats is None:
        stats = torch.empty(n_stats, dtype=torch.float32, device=dev)
    else:
        ck.flat(what, "stats", stats, torch.float32, n_stats, dev)
    ck.require_gpu(dev)
    if B == 0:
        for n in shapes:
            grads[n].zero_()
        stats.zero_()
        return grads, stats, None
    need = workspace_bytes() if workspace is None or size_given else 0
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=dev)
    elif workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"{what}: workspace must be a contiguous tensor on {dev}")
    return grads, stats, workspace


def ppo_actor_grad(actor: ActorParams, obs: torch.Tensor, action: torch.Tensor, logp_old: torch.Tensor, advantage: torch.Tensor,
                   index: Optional[torch.Tensor] = None, *, final_obs: Optional[torch.Tensor] = None, done: Optional[torch.Tensor] = None,
                   truncated: Optional[torch.Tensor] = None, clip: float = 0.2, entropy_coef: float = 0.0, lam_T: float = 0.0,
                   lam_S: float = 0.0, lam_M: float = 0.0, noise: Optional[torch.Tensor] = None, nominal: Optional[torch.Tensor] = None,
                   max_action: float = 1.0, col_offset: int = 0, grads: Optional[dict] = None, stats: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None, max_workgroups: int = 0, entropy_coef_dev: Optional[torch.Tensor] = None):
    """PPO's actor loss (ppo.py:169-182 + policy_regularization.py) and its gradients for ONE agent and one minibatch, in one launch
    plus a small reduction (qr_ppo_actor_grad) — no autograd, no copies of the minibatch's rows.
    obs [T+1, N, D] contiguous float32 (the storage's rows of this agent); action / logp_old [T, N, ..]: this agent's columns start at
    `col_offset` of each row (a per-agent view with col_offset = 0, or the storage's [T, N, 5] rows with the agent's offset);
    advantage: float32, T * N elements with one element stride (`advantage[..., k]`); index: int64 [B] rows of the flat [T * N]
    transitions, None = all of them in order.  final_obs [T, N, D] with done [T, N, n_agents] (and truncated [T, N]) give the
    reference's obs_next for lam_T (without them: obs[t + 1]).  noise [D]: the ONE draw of N(0, 0.05) the spatial term adds to every
    row (required when lam_S != 0); nominal [A]: `RolloutStorage.nominal_action` (required when lam_M != 0).  entropy_coef_dev: a
    float32 tensor of one element on obs' device that the launch reads the entropy coefficient from, instead of `entropy_coef`
    (qr_ppo_actor_grad_dev: the bits of passing that float by value; a captured launch follows the word).
    Returns (grads, stats): grads = {name: float32 tensor} for fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, log_std — `grads` given:
    overwritten in place — and stats float32 [4] = loss, mean surrogate, clip fraction, mean of (rho - 1) - log rho."""
    what = "ppo_actor_grad"
    dev = obs.device
    if actor.dims not in PPO_ACTOR_DIMS:
        raise ValueError(f"{what}: actor sizes {actor.dims} are not among {PPO_ACTOR_DIMS} (obs, hidden, action)")
    if actor.squash != _lib.ACTOR_TANH_MEAN or actor.log_std_w is not None or actor.log_std is None:
        raise ValueError(f"{what}: the actor must be of MLP_Actor_PPO's form: the tanh-of-mean rule and a log_std parameter, no log_std head")
    actor.check(actor.dims, dev)
    D, H, A = actor.dims
    if obs.dtype != torch.float32 or obs.dim() != 3 or obs.shape[0] < 2 or obs.shape[2] != D or not obs.is_contiguous():
        raise ValueError(f"{what}: obs must be contiguous float32 [T+1, N, {D}], got {obs.dtype} {tuple(obs.shape)}")
    T, N = obs.shape[0] - 1, obs.shape[1]
    if N < 1:
        raise ValueError(f"{what}: obs holds no env")
    col_offset = int(col_offset)
    if col_offset < 0:
        raise ValueError(f"{what}: col_offset must be >= 0")
    rs = ck.rows_view(what, "action", action, T, N, A, col_offset, dev)
    if ck.rows_view(what, "logp_old", logp_old, T, N, A, col_offset, dev) != rs:
        raise ValueError(f"{what}: action and logp_old must have the same row stride")
    if advantage.dtype != torch.float32 or advantage.device != dev or advantage.numel() != T * N:
        raise ValueError(f"{what}: advantage must be float32 with {T * N} elements on {dev}")
    adv_stride = ck.element_stride(what, "advantage", advantage)
    n_agents = 0
    if final_obs is not None:
        ck.tensor(what, "final_obs", final_obs, torch.float32, (T, N, D), dev)
        if done is None:
            raise ValueError(f"{what}: final_obs needs done")
        n_agents = ck.reset_flags(what, done, truncated, T, N, dev)
    else:
        done = truncated = None
    B = ck.index(what, index, dev, T * N)
    if lam_S == 0:
        noise = None
    elif noise is None:
        raise ValueError(f"{what}: noise is required when lam_S != 0")
    ck.flat(what, "noise", noise, torch.float32, D, dev, True)
    if lam_M == 0:
        nominal = None
    elif nominal is None:
        raise ValueError(f"{what}: nominal is required when lam_M != 0")
    ck.flat(what, "nominal", nominal, torch.float32, A, dev, True)
    ck.scalar(what, "entropy_coef_dev", entropy_coef_dev, torch.float32, dev)
    grads, stats, workspace = _grad_outputs(what, _GRAD_SHAPES(D, H, A), dev, B, grads, stats, workspace,
                                            lambda: ppo_workspace_bytes((D, H, A), B, max_workgroups))
    if workspace is None:
        return grads, stats
    b = _lib.ppo_batch_args(obs, action, logp_old, advantage, workspace, final_obs=final_obs, done=done, truncated=truncated, index=index,
                            noise=noise, nominal=nominal, batch=B, n_envs=N, n_steps=T, n_agents=n_agents, row_stride=rs, col_offset=col_offset,
                            adv_stride=adv_stride, max_workgroups=max_workgroups, clip=clip, entropy_coef=entropy_coef, lam_T=lam_T, lam_S=lam_S,
                            lam_M=lam_M, max_action=max_action)
    g = _lib.ppo_grad_args(grads, stats)
    if entropy_coef_dev is None:
        _lib.launch(dev, "qr_ppo_actor_grad", actor.as_c(), b, g)
    else:
        _lib.launch(dev, "qr_ppo_actor_grad_dev", actor.as_c(), b, g, entropy_coef_dev.data_ptr())
    return grads, stats


def actor_loss(module, storage, k: int, advantage: torch.Tensor, index: Optional[torch.Tensor] = None, **coeffs) -> torch.Tensor:
    """The actor update of a training loop, as the reference writes it, without autograd: runs `storage.actor_grad` for agent k on the
    live `module` (attributes fc1, fc2, mean_linear, log_std — its tensors are read in place) and writes the gradients into
    `module.<param>.grad` in place (log_std in the module's [1, A] shape), as `loss.backward()` after `zero_grad()` leaves them.
    coeffs: `RolloutStorage.actor_grad`'s, among them entropy_coef_dev= (the coefficient read from a device word).
    Returns stats (stats[0] = the loss).  Gradient clipping, the optimiser step and the schedule follow on these .grad tensors: `optim.DeviceAdamW` (one launch), or torch's."""
    grads = module_grads(_lib.PPO_GRAD_NAMES, (module.fc1.weight, module.fc1.bias, module.fc2.weight, module.fc2.bias, module.mean_linear.weight,
                                               module.mean_linear.bias, module.log_std))
    _, stats = storage.actor_grad(k, ActorParams.from_module(module), advantage, index, grads=grads, **coeffs)
    return stats


# ----------------------------------------------------------------------------------------------------------------
# the critic half of a PPO minibatch update (qr_ppo_critic_grad)
# ----------------------------------------------------------------------------------------------------------------
def ppo_critic_workspace_bytes(dims, batch: int, max_workgroups: int = 0) -> int:
    """Bytes of workspace one `ppo_critic_grad` launch needs (qr_ppo_critic_workspace_bytes); dims = (input width, hidden width)."""
    return _lib.workspace_bytes("qr_ppo_critic_workspace_bytes", dims[0], dims[1], batch, max_workgroups)


def ppo_critic_grad(critic: CriticParams, obs, target: torch.Tensor, index: Optional[torch.Tensor] = None, *, l2_reg: float = 0.0,
                    grads: Optional[dict] = None, stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                    max_workgroups: int = 0):
    """PPO's critic loss (ppo.py:193-214: the mean squared error of V against the TD target plus l2_reg times the squared norms of the
    three weight tensors) and its gradients for ONE critic and one minibatch, in one launch plus a small reduction
    (qr_ppo_critic_grad) — no autograd, no copies of the minibatch's rows.
    obs: the per-agent observation row tensors [.., D_k] as `critic_values` takes them (contiguous float32; an agent the critic does
    not read may be None), at least target.numel() rows each, of which the leading ones are used — `storage.obs` passes as it is;
    target: float32 with ONE element stride, e.g. `storage.td_target[..., k]`; index: int64 [B] rows of the flat target, None = all
    of them in order.
    Returns (grads, stats): grads = {name: float32 tensor} for fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b — `grads` given: overwritten
    in place — and stats float32 [4] = loss, mse, mean error, population variance of the minibatch's targets (explained variance =
    1 - (stats[1] - stats[2] ** 2) / stats[3])."""
    what = "ppo_critic_grad"
    dev = target.device
    if target.dtype != torch.float32:
        raise ValueError(f"{what}: target must be float32, got {target.dtype}")
    rows, stride = target.numel(), ck.element_stride(what, "target", target)
    if critic.device != dev:
        raise ValueError(f"{what}: the critic's tensors are on {critic.device}, the target on {dev}")
    obs, widths = ck.obs_rows(what, obs, rows, dev, at_least=True)
    q = critic.as_c(widths)
    B = ck.index(what, index, dev, rows)
    if B and rows < 1:
        raise ValueError(f"{what}: an index needs a target with at least one element")
    shapes = {n: tuple(getattr(critic, n).shape) for n in _lib.PPO_CRITIC_GRAD_NAMES}
    grads, stats, workspace = _grad_outputs(what, shapes, dev, B, grads, stats, workspace,
                                            lambda: ppo_critic_workspace_bytes(critic.dims, B, max_workgroups))
    if workspace is None:
        return grads, stats
    b = _lib.critic_batch_args(obs[0] if q.in0 else None, obs[1] if q.in1 else None, target, workspace, index=index, batch=B, rows=rows,
                               target_stride=stride, max_workgroups=max_workgroups, l2_reg=l2_reg)
    _lib.launch(dev, "qr_ppo_critic_grad", q, b, _lib.critic_grad_args(grads, stats))
    return grads, stats


def critic_loss(module, storage, k: int, index: Optional[torch.Tensor] = None, inputs=(0,), **coeffs) -> torch.Tensor:
    """The critic update of a training loop, as the reference writes it, without autograd — the twin of `actor_loss`: runs
    `storage.critic_grad` for agent k on the live `module` (attributes fc1, fc2, fc3 — its tensors are read in place; inputs: the
    agents whose observation rows it reads, `CriticParams.inputs`) and writes the gradients into `module.fc{1,2,3}.{weight,bias}.grad`
    in place, as `loss.backward()` after `zero_grad()` leaves them.  coeffs: l2_reg, target, stats, max_workgroups.  Returns stats
    (stats[0] = the loss).  Gradient clipping, the optimiser step and the schedule follow on these .grad tensors: `optim.DeviceAdamW` (one launch), or torch's."""
    params = (module.fc1.weight, module.fc1.bias, module.fc2.weight, module.fc2.bias, module.fc3.weight, module.fc3.bias)
    if "grads" in coeffs:
        raise ValueError("critic_loss writes into the module's .grad tensors: it takes no grads")
    grads = module_grads(_lib.PPO_CRITIC_GRAD_NAMES, params)
    _, stats = storage.critic_grad(k, CriticParams.from_module(module, inputs), index, grads=grads, **coeffs)
    return stats


def c_actor_array(actors: Sequence[ActorParams]):
    arr = (_lib.QrActor * len(actors))()
    for k, a in enumerate(actors):
        arr[k] = a.as_c()
    return arr


def random_actors(kind: str, device, generator=None, log_std: float = 0.0, algo: str = "ppo") -> List[ActorParams]:
    """Random-init actors of the reference's sizes for `kind`.  algo='ppo' (also TD3's form): parameter log_std, tanh-of-mean rule.
    algo='sac': MLP_Actor_SAC's form — a state-dependent log_std head (bias = log_std, weights x0.1) and the tanh-of-sample rule
    (sac_mlp.py:60-82), i.e. what rollout_actor runs in its general (POLICY = 2) kernel."""
    if algo not in ("ppo", "sac"):
        raise ValueError("algo must be 'ppo' or 'sac'")
    actors = [ActorParams.random(*d, device=device, generator=generator, log_std=log_std) for d in ACTOR_DIMS[kind]]
    if algo == "sac":
        for a in actors:
            _, hidden, adim = a.dims
            k = hidden ** -0.5
            a.log_std_w = (torch.rand(adim, hidden, device=device, generator=generator) * 2 - 1) * k * 0.1
            a.log_std_b = torch.full((adim,), float(log_std), device=device)
            a.log_std, a.squash = None, _lib.ACTOR_TANH_SAMPLE
    return actors


# ----------------------------------------------------------------------------------------------------------------
# a population of policies for QuadVecEnv.evaluate_population (qr_evaluate_population)
# ----------------------------------------------------------------------------------------------------------------
def population_layout(n_policies: int, envs_per_policy: int):
    """(Epad, N) of qr_evaluate_population's block layout: P policies of E episodes each live on ONE env of N = P * Epad envs,
    Epad = E rounded up to a multiple of 64 (a 64-env tile never holds two policies).  Policy p owns envs [p Epad, p Epad + E)."""
    P, E = int(n_policies), int(envs_per_policy)
    if P < 1 or E < 1:
        raise ValueError("a population needs n_policies >= 1 and envs_per_policy >= 1")
    epad = (E + 63) // 64 * 64
    return epad, P * epad


def population_env_index(n_policies: int, envs_per_policy: int, device=None) -> torch.Tensor:
    """int64 [P, E]: the env that flies episode e of policy p (p * Epad + e) — the live envs, in block order."""
    epad, _ = population_layout(n_policies, envs_per_policy)
    return torch.arange(n_policies, device=device)[:, None] * epad + torch.arange(envs_per_policy, device=device)[None, :]


def population_view(t: torch.Tensor, n_policies: int, envs_per_policy: int, env_dim: int = 0) -> torch.Tensor:
    """The [.., P, E, ..] view of a tensor whose dimension `env_dim` runs over the N = P * Epad envs: the padding sliced off,
    no copy."""
    epad, n = population_layout(n_policies, envs_per_policy)
    env_dim = env_dim % t.dim()
    if t.shape[env_dim] != n:
        raise ValueError(f"dimension {env_dim} has {t.shape[env_dim]} entries, the population layout {n} = {n_policies} x {epad}")
    return t.unflatten(env_dim, (n_policies, epad)).narrow(env_dim + 1, 0, envs_per_policy)


def population_tile(block: torch.Tensor, n_policies: int, envs_per_policy: int, out: torch.Tensor, env_dim: int = 0) -> torch.Tensor:
    """Copy `block` — E entries along `env_dim`, the prepared state of E episodes — into every policy's block of `out` (N entries
    along `env_dim`).  The padding envs of `out` keep what they hold."""
    env_dim = env_dim % out.dim()
    if block.dim() != out.dim() or block.shape[env_dim] != envs_per_policy:
        raise ValueError(f"the block has {block.shape[env_dim]} entries along dimension {env_dim}, not {envs_per_policy}")
    population_view(out, n_policies, envs_per_policy, env_dim).copy_(block.unsqueeze(env_dim))
    return out


_WEIGHTS = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b")


class ActorPopulation:
    """P policies of one form as stacked tensors: per agent ONE `ActorParams` whose tensors carry a leading [P] dimension
    (contiguous float32), which is how qr_evaluate_population reads them — the pointers are policy 0's, policy p's tensor starts
    p * numel elements later.  `len(pop)` is P; `pop[p]` are the ordinary per-agent ActorParams VIEWS of policy p (no copy:
    `evaluate` and `rollout_actor` take them as they are, and an in-place update of the stack is seen through them)."""

    def __init__(self, agents: Sequence[ActorParams]):
        self.agents = list(agents)
        if not self.agents:
            raise ValueError("a population needs at least one agent")
        sizes = {getattr(a, n).shape[0] for a in self.agents for n in ActorParams.NAMES if getattr(a, n) is not None}
        if len(sizes) != 1:
            raise ValueError(f"stacked actor tensors disagree on the number of policies: {sorted(sizes)}")
        self.n_policies = int(sizes.pop())

    def __len__(self) -> int:
        return self.n_policies

    def __getitem__(self, p: int) -> List[ActorParams]:
        p = int(p)
        if not -self.n_policies <= p < self.n_policies:
            raise IndexError(f"policy {p} of {self.n_policies}")
        return [ActorParams(*[None if getattr(a, n) is None else getattr(a, n)[p] for n in ActorParams.NAMES], a.squash)
                for a in self.agents]

    def __iter__(self):
        return (self[p] for p in range(self.n_policies))

    def select(self, index) -> "ActorPopulation":
        """The sub-population of the policies `index` names (a slice: views; an index tensor / list: copies) — how a population is
        sharded: every rank evaluates its own slice."""
        def take(t):
            if t is None:
                return None
            s = t[index]
            return s if s.is_contiguous() else s.contiguous()
        return ActorPopulation([ActorParams(*[take(getattr(a, n)) for n in ActorParams.NAMES], a.squash) for a in self.agents])

    @classmethod
    def stack(cls, members: Sequence[Sequence[ActorParams]]) -> "ActorPopulation":
        """From P ordinary actor lists (one ActorParams per agent each).  All members must have the same number of agents, tensor
        sizes, dtype and device, and ONE form: the same `squash` rule and the same log_std source per agent.  ValueError otherwise."""
        members = [list(m) for m in members]
        if not members:
            raise ValueError("stack needs at least one policy")
        first = members[0]
        agents = []
        for m in members:
            if len(m) != len(first):
                raise ValueError(f"policies with {len(first)} and {len(m)} actors cannot be stacked")
        for k, ref in enumerate(first):
            cols = {}
            for n in ActorParams.NAMES:
                r = getattr(ref, n)
                for m in members:
                    t = getattr(m[k], n)
                    if (t is None) != (r is None) or m[k].squash != ref.squash:
                        raise ValueError(f"agent {k}: all policies of a population share one form (squash rule and log_std source)")
                    if t is not None and (t.shape != r.shape or t.dtype != r.dtype or t.device != r.device):
                        raise ValueError(f"agent {k}: actor tensor {n} differs in size, dtype or device between policies "
                                         f"({tuple(t.shape)} {t.dtype} on {t.device} against {tuple(r.shape)} {r.dtype} on {r.device})")
                cols[n] = None if r is None else torch.stack([getattr(m[k], n) for m in members]).contiguous()
            agents.append(ActorParams(**cols, squash=ref.squash))
        return cls(agents)

    @classmethod
    def perturb(cls, base_actors: Sequence[ActorParams], n: int, sigma: float, generator=None, antithetic: bool = True, eps=None):
        """The evolution-strategy constructor: n policies theta + sigma eps_i around `base_actors`, over ALL weight and bias tensors
        (fc1, fc2 and the mean head; the log_std source is copied, evaluation never reads it).  eps ~ N(0, 1) from `generator`.
        antithetic (n even): pairs are adjacent — policy 2k is theta + sigma eps_k, policy 2k + 1 is theta - sigma eps_k, with the
        SAME float32 product sigma eps_k, so a pair's mean is theta up to the one rounding of each member to float32.
        Returns (population, eps): eps is one dict per agent, tensor name -> [n, ...] float32, row i the draw of policy i (row
        2k + 1 = -row 2k when antithetic) — what the estimator sum_i fitness_i eps_i / (n sigma) needs.
        `eps`: given draws in that form instead of the generator's ([n, ...] per tensor; antithetic: the even rows are used)."""
        n = int(n)
        if n < 1 or (antithetic and n % 2):
            raise ValueError("perturb needs n >= 1, and an even n when antithetic")
        agents, draws = [], []
        for k, a in enumerate(base_actors):
            cols, e_k = {}, {}
            for name in ActorParams.NAMES:
                t = getattr(a, name)
                if t is None:
                    cols[name] = None
                elif name not in _WEIGHTS:
                    cols[name] = t.detach().unsqueeze(0).expand(n, *t.shape).contiguous()
                else:
                    t = t.detach()
                    half = n // 2 if antithetic else n
                    if eps is not None:
                        given = eps[k][name]
                        if tuple(given.shape) != (n,) + tuple(t.shape):
                            raise ValueError(f"eps[{k}][{name!r}] must be [{n}, ...] like the stacked tensor")
                        e = (given[0::2] if antithetic else given).to(t)
                    else:
                        e = torch.randn((half,) + tuple(t.shape), dtype=t.dtype, device=t.device, generator=generator)
                    d = float(sigma) * e
                    if antithetic:
                        cols[name] = torch.stack([t + d, t - d], 1).reshape((n,) + tuple(t.shape)).contiguous()
                        e_k[name] = torch.stack([e, -e], 1).reshape((n,) + tuple(t.shape))
                    else:
                        cols[name], e_k[name] = (t + d).contiguous(), e
            agents.append(ActorParams(**cols, squash=a.squash))
            draws.append(e_k)
        return cls(agents), draws

    def check(self, kind: str, device):
        """The host-side argument check of evaluate_population: the reference's sizes for `kind`, contiguous float32 on `device`."""
        dims = ACTOR_DIMS[kind]
        if len(self.agents) != len(dims):
            raise ValueError(f"kind {kind!r} needs {len(dims)} actor(s)")
        for a, d in zip(self.agents, dims):
            for n in ActorParams.NAMES:
                t = getattr(a, n)
                if t is not None and (t.dtype != torch.float32 or t.device != device or not t.is_contiguous()):
                    raise ValueError(f"stacked actor tensor {n} must be a contiguous float32 tensor on {device}")
        for a_, d in zip(self[0], dims):
            a_.check(d, device)

    def c_array(self):
        """QrActor array of policy 0 — the stacked-tensor rule's base pointers."""
        return c_actor_array(self[0])
