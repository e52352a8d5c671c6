"""One-call TD3 and SAC updates: `Td3Updater` and `SacUpdater`, the bodies of the reference's `TD3.train` (algos/td3/td3.py:98-214) and
`SAC.train` (algos/sac/sac.py:108-223) for all agents of a buffer, composed from the library's public calls — `ReplayBuffer.sample_index`,
the `td3_*_loss` / `sac_*_loss` launches — and `optim.PolyakAdamW`, which steps a twin critic's twelve tensors as ONE group (one clip,
one step counter, as the reference's `AdamW(critic.parameters())`) and applies the soft target update in the same launch.

Per iteration and agent: TD3 — sample, refill the noise, critic loss (3 launches), critic step (1), and every policy_update_freq-th
iteration actor loss (2) and actor step (1); SAC — sample, refill, critic loss (3), critic step (1), actor loss (2), ONE step for the
actor and log_alpha that also leaves alpha = exp(log_alpha) (1).  The soft updates ride on the steps: a network's target is updated
in the launch that steps the network (see `_Updater._polyak_now`).  Nothing synchronises; `capture` records policy_update_freq
iterations in one graph.

The collection half of the same loop (main.py:140-181) is `OffPolicyCollector`: the uniform-random warm-up, TD3's decaying exploration
std or SAC's sampled actions, one horizon per call into a `RolloutStorage`, and the append with the reference's time-limit done rule.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _checks as ck
from . import _lib
from .episodes import EpisodeTracker
from .noise import check_seed, noise_fill
from .optim import PolyakAdamW
from .sac import sac_actor_loss, sac_actor_loss_ctde, sac_critic_loss, sac_critic_loss_ctde
from .rollout import RolloutStorage
from .td3 import TIME_LIMITS, ReplayBuffer, td3_actor_loss, td3_actor_loss_ctde, td3_critic_loss, td3_critic_loss_ctde

MODES = ("single", "dtde", "ctde")   # Coupled with one agent; Decoupled with own critics; Decoupled with one centralized critic per agent
T0, ETA_MIN = 1_000_000, 1e-5        # CosineAnnealingWarmRestarts(T_0, eta_min) of both algorithms (td3.py:79-80, sac.py:81-82)
NOISE_SOURCES = ("torch", "device")  # who draws: torch.Tensor.normal_ per tensor, or one noise_fill launch per agent (noise.py)
# every name a `_noise_shapes` can return: a tensor's place here is part of its stream id
NOISE_NAMES = ("smooth", "reg", "next", "eps", "eps_reg", "eps_next", "eps_pert", "noise_logp", "eps_logp", "eps_other")
REG_STD = 0.05                       # policy_regularization's N(0, 0.05) row
# the collector's warm-up stream: above every `noise_stream` id, so that a collector and an updater sharing a seed never share words
COLLECTOR_STREAM = 1 << 29


def noise_stream(k: int, name: str, j: int = 0) -> int:
    """The stream id of agent k's noise tensor `name` (position j inside a ctde pair, else 0) under noise_source="device"."""
    return (k << 8) | (NOISE_NAMES.index(name) << 2) | j


def _noise_source(what: str, noise_source, noise_seed, generator) -> int:
    if noise_source not in NOISE_SOURCES:
        raise ValueError(f"{what}: noise_source must be one of {NOISE_SOURCES}, got {noise_source!r}")
    if noise_source == "device" and generator is not None:
        raise ValueError(f"{what}: noise_source='device' draws from the library's own stream (noise_seed); it takes no torch generator")
    return check_seed(what, noise_seed)


def _layers(module, names, what: str):
    out = []
    for n in names:
        layer = getattr(module, n, None)
        if layer is None or not hasattr(layer, "weight") or not hasattr(layer, "bias"):
            raise ValueError(f"{what}: a module has no layer {n} with weight and bias")
        out += [layer.weight, layer.bias]
    return out


def _per_agent(v, n: int, name: str, what: str):
    vs = [float(x) for x in v] if isinstance(v, (list, tuple)) else [float(v)] * n
    if len(vs) != n:
        raise ValueError(f"{what}: {name} is a number or one number per agent")
    return vs


CRITIC_LAYERS = ("fc1", "fc2", "fc3", "fc4", "fc5", "fc6")


class _Updater:
    """What `Td3Updater` and `SacUpdater` share: the arguments, the critic optimisers, the minibatch tensors, the iteration loop and
    the graph capture."""
    what = "_Updater"
    actor_layers: Sequence[str] = ()

    def __init__(self, actors, critics, critic_targets, *, mode, discount, tau, policy_update_freq, lam_T, lam_S, lam_M, max_action, lr_a, lr_c,
                 grad_max_norm, batch_size, nominal, generator, refill_noise, noise_source="torch", noise_seed=0):
        what = self.what
        self.noise_seed = _noise_source(what, noise_source, noise_seed, generator)
        self.noise_source = noise_source
        self.actors, self.critics, self.critic_targets = list(actors), list(critics), list(critic_targets)
        n = self.n_agents = len(self.actors)
        if mode not in MODES:
            raise ValueError(f"{what}: mode must be one of {MODES}, got {mode!r}")
        if n < 1 or len(self.critics) != n or len(self.critic_targets) != n:
            raise ValueError(f"{what} needs one actor, critic and critic target per agent")
        if (mode == "single" and n != 1) or (mode in ("dtde", "ctde") and n != 2):
            raise ValueError(f"{what}: mode 'single' is one agent, 'dtde' and 'ctde' are two; got {n}")
        self.mode = mode
        self.discount, self.tau, self.max_action = float(discount), float(tau), float(max_action)
        self.lam_T, self.lam_S, self.lam_M = float(lam_T), float(lam_S), float(lam_M)
        self.policy_update_freq, self.batch_size = int(policy_update_freq), int(batch_size)
        if self.policy_update_freq < 1 or self.batch_size < 1:
            raise ValueError(f"{what}: policy_update_freq and batch_size must be >= 1")
        if not 0.0 <= self.tau <= 1.0:
            raise ValueError(f"{what}: tau must lie in [0, 1], got {tau}")
        if not 0.0 <= self.discount < float("inf") or not 0.0 < self.max_action < float("inf"):
            raise ValueError(f"{what}: discount must be finite and >= 0, max_action finite and > 0")
        self.lr_a, self.lr_c = _per_agent(lr_a, n, "lr_a", what), _per_agent(lr_c, n, "lr_c", what)
        self.grad_max_norm = float(grad_max_norm)
        self.nominal = list(nominal) if nominal is not None else [None] * n
        if len(self.nominal) != n:
            raise ValueError(f"{what}: nominal is one [A_k] tensor (or None) per agent")
        if self.lam_M != 0.0 and any(x is None for x in self.nominal):
            raise ValueError(f"{what}: lam_M != 0 needs every agent's nominal action")
        self.generator, self.refill_noise = generator, bool(refill_noise)
        self.total_it = 0
        self.actor_params = [_layers(m, self.actor_layers, what) for m in self.actors]
        critic_params = [_layers(m, CRITIC_LAYERS, what) for m in self.critics]
        target_params = [_layers(m, CRITIC_LAYERS, what) for m in self.critic_targets]
        self.device = critic_params[0][0].device
        hyper = dict(tau=self.tau, max_norm=self.grad_max_norm, t0=T0, eta_min=ETA_MIN)
        self._hyper = hyper
        self.critic_opts = [PolyakAdamW(critic_params[k], targets=[t.data for t in target_params[k]], lr=self.lr_c[k], **hyper) for k in range(n)]
        f32 = dict(dtype=torch.float32, device=self.device)
        self.critic_stats = [torch.zeros(4, **f32) for _ in range(n)]
        self.index, self.noise, self._dims, self._fills = None, None, None, None

    # -- the minibatch tensors -------------------------------------------------------------------------------------------------------
    def _noise_shapes(self, k: int, B: int, od, ad) -> dict:
        raise NotImplementedError

    def _prepare(self, buffer: ReplayBuffer) -> None:
        what = self.what
        if not isinstance(buffer, ReplayBuffer):
            raise ValueError(f"{what}.update: buffer must be a ReplayBuffer")
        if buffer.n_agents != self.n_agents:
            raise ValueError(f"{what}.update: the buffer has {buffer.n_agents} agents, the updater {self.n_agents}")
        if not 1 <= self.batch_size <= buffer.current_size:
            raise ValueError(f"{what}.update: cannot draw {self.batch_size} of {buffer.current_size} transitions")
        dims = (tuple(buffer.obs_dims), tuple(buffer.action_dims), self.batch_size)
        if dims == self._dims:
            return
        dev, B = self.device, self.batch_size
        self.index = [torch.zeros(B, dtype=torch.int64, device=dev) for _ in range(self.n_agents)]
        self.noise = []
        for k in range(self.n_agents):
            shapes = self._noise_shapes(k, B, buffer.obs_dims, buffer.action_dims)
            self.noise.append({name: (tuple(torch.zeros(s, dtype=torch.float32, device=dev) for s in shape) if isinstance(shape, list) else
                                      torch.zeros(shape, dtype=torch.float32, device=dev)) for name, shape in shapes.items()})
        # per agent what one noise_fill launch takes: the tensors in `noise[k]`'s order, their stream ids and standard deviations
        self._fills = []
        for k in range(self.n_agents):
            flat = [(name, j, x) for name, t in self.noise[k].items() for j, x in enumerate(t if isinstance(t, tuple) else (t,))]
            self._fills.append(([x for _, _, x in flat], [noise_stream(k, name, j) for name, j, _ in flat],
                                [REG_STD if name == "reg" else 1.0 for name, _, _ in flat]))
        self._dims = dims

    def _refill(self, k: int, buffer: ReplayBuffer) -> None:
        """Agent k's draws of this iteration, in place: standard normal for the samples, N(0, 0.05) for policy_regularization's row.
        noise_source "torch": one `normal_` per tensor.  "device": ONE `noise_fill` launch over all of them, keyed by noise_seed, the
        buffer's draw number as `sample_index` has just left it — read on the device where the buffer keeps its counters there, so
        that a captured graph draws fresh noise at every replay, the same an eager iteration draws for that minibatch number — and
        `noise_stream(k, name, j)`."""
        if not self.refill_noise:
            return
        if self.noise_source == "device":
            tensors, streams, stds = self._fills[k]
            noise_fill(tensors, seed=self.noise_seed, draw=buffer.draw, streams=streams, b=stds,
                       draw_dev=None if buffer.state is None else buffer.state[2:3])
            return
        for name, t in self.noise[k].items():
            for x in (t if isinstance(t, tuple) else (t,)):
                if name == "reg":
                    x.normal_(0.0, 0.05, generator=self.generator)
                else:
                    x.normal_(generator=self.generator)

    # -- the loop --------------------------------------------------------------------------------------------------------------------
    def _polyak_now(self) -> bool:
        """Is this a delayed-update iteration (total_it % policy_update_freq == 0)?  Then the critic's step carries its soft update:
        between that step and the place where the reference updates the target (td3.py:207-208, sac.py:219-221) nothing writes the
        critic and nothing reads its target, so the target gets the same bits there and here."""
        return self.total_it % self.policy_update_freq == 0

    def _iterate(self, buffer: ReplayBuffer, k: int, polyak: bool) -> None:
        raise NotImplementedError

    def _stats(self):
        raise NotImplementedError

    def update(self, buffer: ReplayBuffer, iterations: int = 1):
        """`iterations` training iterations, each one the agents' `train` calls in index order (main.py:194-204).  Returns the per-agent
        stats tensors of the last iteration, on the device; nothing synchronises.  From the second call on with an unchanged batch
        size nothing is allocated."""
        if int(iterations) < 1:
            raise ValueError(f"{self.what}.update: iterations must be >= 1")
        self._prepare(buffer)
        for _ in range(int(iterations)):
            self.total_it += 1
            polyak = self._polyak_now()
            for k in range(self.n_agents):
                buffer.sample_index(self.batch_size, out=self.index[k])
                self._refill(k, buffer)
                self._iterate(buffer, k, polyak)
        return self._stats()

    def capture(self, buffer: ReplayBuffer):
        """Record policy_update_freq consecutive iterations — one delayed update among them, at the phase `total_it` has now — in one
        `torch.cuda.graph` (a linear chain of launches) and return a callable that replays them and returns `update`'s stats.
        Needs `buffer.use_device_state()`, so that every replay draws fresh minibatches, and one eager `update` on this buffer
        before it, which makes the workspaces and the .grad tensors.  Each replay advances the host's `total_it` by
        policy_update_freq; the buffer's host counters follow with `buffer.pull_device_state()`.  Capturing runs nothing."""
        what = self.what
        if not isinstance(buffer, ReplayBuffer) or buffer.state is None:
            raise ValueError(f"{what}.capture: the buffer must keep its counters on the device (ReplayBuffer.use_device_state())")
        if self._dims != (tuple(buffer.obs_dims), tuple(buffer.action_dims), self.batch_size) or self.total_it == 0:
            raise ValueError(f"{what}.capture: run update() on this buffer once first (it makes the workspaces the graph records)")
        ck.require_gpu(self.device)
        graph = torch.cuda.CUDAGraph()
        if self.noise_source == "torch" and self.generator is not None and self.refill_noise and hasattr(graph, "register_generator_state"):
            graph.register_generator_state(self.generator)
        start, host = self.total_it, (buffer.count, buffer.current_size, buffer.draw)
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(graph):
            stats = self.update(buffer, self.policy_update_freq)
        self.total_it = start                                     # nothing ran: the counters are where they were
        buffer.count, buffer.current_size, buffer.draw = host

        def replay():
            graph.replay()
            self.total_it += self.policy_update_freq
            return stats

        replay.graph = graph
        return replay


class Td3Updater(_Updater):
    """`TD3.train` (td3.py:98-214) for every agent of a `ReplayBuffer`, one call per `iterations` training iterations.

    actors, critics, actor_targets, critic_targets: per agent the live modules (actor: fc1, fc2, fc3; critic: fc1 .. fc6, in mode
    "ctde" the centralized MLP_Critic_CTDE of that agent) and their targets; all are read and updated in place.  mode: "single"
    (one agent), "dtde" (two agents, own critics) or "ctde" (two agents, each with a centralized critic).  The hyperparameters are the
    reference's names and defaults (args_parse.py:42-59, 76-78); lr_a, lr_c: a number or one per agent; the schedule is
    CosineAnnealingWarmRestarts(1_000_000, 1e-5).  nominal: per agent the [A_k] hover action of policy_regularization (needed when
    lam_M != 0).  generator: the torch generator of the noise draws (None: the device's default).  noise_source: "torch" draws each
    noise tensor with its own `normal_`; "device" fills all of an agent's tensors in ONE `noise_fill` launch from the library's
    counter-based stream, keyed by noise_seed, the buffer's draw number and `noise_stream(k, name, j)` — the same values eager and
    under graph replay for the same minibatch number, whatever the torch version; it takes no generator.
    Owns per agent `critic_opts[k]` (`PolyakAdamW` over the twelve critic tensors and their targets) and `actor_opts[k]` (over the
    six actor tensors and theirs), `index[k]` (int64 [B]) and `noise[k]` = {"smooth": the [B, A_k] smoothing draws (ctde: the pair),
    "reg": the [D_k] row}.  Per iteration and agent: `sample_index`, the draws, `td3_critic_loss[_ctde]`, the critic's step, and when
    total_it % policy_update_freq == 0 `td3_actor_loss[_ctde]` and the actor's step; the soft updates ride on those two steps."""
    what = "Td3Updater"
    actor_layers = ("fc1", "fc2", "fc3")

    def __init__(self, actors, critics, actor_targets, critic_targets, *, mode: str = "single", discount: float = 0.99, tau: float = 0.005,
                 target_noise: float = 0.2, noise_clip: float = 0.5, policy_update_freq: int = 3, lam_T: float = 0.4, lam_S: float = 0.3,
                 lam_M: float = 0.6, max_action: float = 1.0, lr_a=3e-4, lr_c=2e-4, grad_max_norm: float = 100.0, batch_size: int = 256,
                 nominal=None, generator: Optional[torch.Generator] = None, refill_noise: bool = True, noise_source: str = "torch",
                 noise_seed: int = 0):
        super().__init__(actors, critics, critic_targets, mode=mode, discount=discount, tau=tau, policy_update_freq=policy_update_freq, lam_T=lam_T,
                         lam_S=lam_S, lam_M=lam_M, max_action=max_action, lr_a=lr_a, lr_c=lr_c, grad_max_norm=grad_max_norm,
                         batch_size=batch_size, nominal=nominal, generator=generator, refill_noise=refill_noise, noise_source=noise_source,
                         noise_seed=noise_seed)
        self.actor_targets = list(actor_targets)
        if len(self.actor_targets) != self.n_agents:
            raise ValueError("Td3Updater needs one actor target per agent")
        self.target_noise, self.noise_clip = float(target_noise), float(noise_clip)
        if not 0.0 <= self.target_noise < float("inf") or not 0.0 <= self.noise_clip < float("inf"):
            raise ValueError("Td3Updater: target_noise and noise_clip must be finite and >= 0")
        targets = [_layers(m, self.actor_layers, self.what) for m in self.actor_targets]
        self.actor_opts = [PolyakAdamW(self.actor_params[k], targets=[t.data for t in targets[k]], lr=self.lr_a[k], **self._hyper)
                           for k in range(self.n_agents)]
        self.actor_stats = [torch.zeros(4, dtype=torch.float32, device=self.device) for _ in range(self.n_agents)]

    def _noise_shapes(self, k, B, od, ad):
        smooth = [(B, a) for a in ad] if self.mode == "ctde" else (B, ad[k])
        return {"smooth": smooth, "reg": (od[k],)}

    def _iterate(self, buffer, k, polyak):
        nz, idx = self.noise[k], self.index[k]
        c_kw = dict(discount=self.discount, target_noise=self.target_noise, noise_clip=self.noise_clip, max_action=self.max_action,
                    noise=nz["smooth"], stats=self.critic_stats[k])
        a_kw = dict(lam_T=self.lam_T, lam_S=self.lam_S, lam_M=self.lam_M, max_action=self.max_action, noise=nz["reg"], nominal=self.nominal[k],
                    stats=self.actor_stats[k])
        if self.mode == "ctde":
            td3_critic_loss_ctde(self.critics[k], self.critic_targets[k], self.actor_targets, buffer, k, idx, **c_kw)
        else:
            td3_critic_loss(self.critics[k], self.critic_targets[k], self.actor_targets[k], buffer, k, idx, **c_kw)
        self.critic_opts[k].step(polyak=polyak)
        if polyak:
            if self.mode == "ctde":
                td3_actor_loss_ctde(self.actors, self.critics[k], buffer, k, idx, **a_kw)
            else:
                td3_actor_loss(self.actors[k], self.critics[k], buffer, k, idx, **a_kw)
            self.actor_opts[k].step(polyak=True)

    def _stats(self):
        return self.critic_stats, self.actor_stats


class SacUpdater(_Updater):
    """`SAC.train` (sac.py:108-223) for every agent of a `ReplayBuffer`, one call per `iterations` training iterations.

    actors, critics, critic_targets: per agent the live modules (actor: fc1, fc2, mean_linear, log_std_linear; critic: fc1 .. fc6,
    in mode "ctde" that agent's centralized critic) and the critics' targets — SAC has no target actor.  mode, the shared
    hyperparameters, nominal and generator: `Td3Updater`'s.  sac_alpha: the entropy temperature (args_parse.py:61), with
    automatic_entropy_tuning the value in use until the first alpha step (sac.py:152, 213); target_entropy: None is -A_k.
    Owns per agent `critic_opts[k]` (twelve tensors with their targets), `actor_opts[k]` (eight tensors) and, with automatic
    entropy tuning, `log_alpha[k]` (a one-entry parameter, zero at the start), `alpha[k]` (float32 [1] on the device) and
    `alpha_opts[k]` — AdamW at lr_a without clipping or schedule (sac.py:88) that leaves alpha = exp(log_alpha) in the same launch;
    `index[k]` and `noise[k]`, the draws of every sample the iteration takes, by the loss calls' argument names ("next": the critic
    half's `noise`).  Per iteration and agent: `sample_index`, the draws, `sac_critic_loss[_ctde]`, the critic's step (with its soft
    update when total_it % policy_update_freq == 0), `sac_actor_loss[_ctde]`, and ONE launch that steps the actor and log_alpha."""
    what = "SacUpdater"
    actor_layers = ("fc1", "fc2", "mean_linear", "log_std_linear")

    def __init__(self, actors, critics, critic_targets, *, mode: str = "single", discount: float = 0.99, tau: float = 0.005,
                 policy_update_freq: int = 3, lam_T: float = 0.4, lam_S: float = 0.3, lam_M: float = 0.6, max_action: float = 1.0, lr_a=3e-4,
                 lr_c=2e-4, grad_max_norm: float = 100.0, automatic_entropy_tuning: bool = False, target_entropy=None, sac_alpha: float = 0.05,
                 batch_size: int = 256, nominal=None, generator: Optional[torch.Generator] = None, refill_noise: bool = True, noise_source: str = "torch",
                 noise_seed: int = 0):
        super().__init__(actors, critics, critic_targets, mode=mode, discount=discount, tau=tau, policy_update_freq=policy_update_freq, lam_T=lam_T,
                         lam_S=lam_S, lam_M=lam_M, max_action=max_action, lr_a=lr_a, lr_c=lr_c, grad_max_norm=grad_max_norm,
                         batch_size=batch_size, nominal=nominal, generator=generator, refill_noise=refill_noise, noise_source=noise_source,
                         noise_seed=noise_seed)
        n, dev = self.n_agents, self.device
        if not 0.0 <= float(sac_alpha) < float("inf"):
            raise ValueError(f"SacUpdater: sac_alpha must be finite and >= 0, got {sac_alpha}")
        self.target_entropy = list(target_entropy) if isinstance(target_entropy, (list, tuple)) else [target_entropy] * n
        if len(self.target_entropy) != n:
            raise ValueError("SacUpdater: target_entropy is None, a number or one per agent")
        self.automatic_entropy_tuning = bool(automatic_entropy_tuning)
        self.actor_opts = [PolyakAdamW(self.actor_params[k], lr=self.lr_a[k], **self._hyper) for k in range(n)]
        self.actor_stats = [torch.zeros(_lib.SAC_ACTOR_STATS, dtype=torch.float32, device=dev) for _ in range(n)]
        if self.automatic_entropy_tuning:
            self.log_alpha = [torch.zeros(1, dtype=torch.float32, device=dev, requires_grad=True) for _ in range(n)]
            self.alpha = [torch.full((1,), float(sac_alpha), dtype=torch.float32, device=dev) for _ in range(n)]
            self.alpha_opts = [PolyakAdamW([self.log_alpha[k]], exp_out=self.alpha[k], lr=self.lr_a[k]) for k in range(n)]
        else:
            self.log_alpha, self.alpha, self.alpha_opts = [None] * n, [float(sac_alpha)] * n, [None] * n

    def _noise_shapes(self, k, B, od, ad):
        own = (B, ad[k])
        shapes = {"next": own, "eps": own, "eps_reg": own, "eps_next": own, "eps_pert": own, "reg": (od[k],)}
        if self.mode == "ctde":
            shapes.update({"next": [(B, a) for a in ad], "noise_logp": own, "eps_logp": own, "eps_other": (B, ad[1 - k])})
        return shapes

    def _iterate(self, buffer, k, polyak):
        nz, idx = self.noise[k], self.index[k]
        c_kw = dict(discount=self.discount, alpha=self.alpha[k], noise=nz["next"], stats=self.critic_stats[k])
        a_kw = dict(log_alpha=self.log_alpha[k], target_entropy=self.target_entropy[k], alpha=self.alpha[k], lam_T=self.lam_T, lam_S=self.lam_S,
                    lam_M=self.lam_M, max_action=self.max_action, eps=nz["eps"], eps_reg=nz["eps_reg"], eps_next=nz["eps_next"],
                    eps_pert=nz["eps_pert"], noise=nz["reg"], nominal=self.nominal[k], stats=self.actor_stats[k])
        if self.mode == "ctde":
            sac_critic_loss_ctde(self.critics[k], self.critic_targets[k], self.actors, buffer, k, idx, noise_logp=nz["noise_logp"], **c_kw)
        else:
            sac_critic_loss(self.critics[k], self.critic_targets[k], self.actors[k], buffer, k, idx, **c_kw)
        self.critic_opts[k].step(polyak=polyak)
        if self.mode == "ctde":
            sac_actor_loss_ctde(self.actors, self.critics[k], buffer, k, idx, eps_logp=nz["eps_logp"], eps_other=nz["eps_other"], **a_kw)
        else:
            sac_actor_loss(self.actors[k], self.critics[k], buffer, k, idx, **a_kw)
        if self.alpha_opts[k] is None:
            self.actor_opts[k].step(polyak=False)
        else:
            PolyakAdamW.step_all([(self.actor_opts[k], False), (self.alpha_opts[k], False)])

    def _stats(self):
        return self.critic_stats, self.actor_stats


class OffPolicyCollector:
    """The collection half of the reference's TD3 / SAC loop (main.py:140-181), one horizon of T env-steps per `collect` call: a host
    object with no kernel of its own — every launch is one the library already has.

    env: a Coupled or Decoupled `QuadVecEnv` with auto_reset=True (and max_episode_steps set, or no transition is ever at the time
    limit); buffer: the `ReplayBuffer` the horizons are appended to, with the env's agents and observation widths.  While
    total_timesteps < start_timesteps the actions are uniform in [-1, 1) (rand * 2 - 1, main.py:155), drawn with torch into a tensor
    made once and flown through the given-actions rollout (qr_rollout); afterwards the actors run inside the step kernel
    (`RolloutStorage.collect`: qr_rollout_actor) — algo "td3": tanh-of-mean actors whose `log_std` tensors are set in place to
    log(explor_noise_std), "sac": tanh-of-sample actors as they are.  Then `buffer.append(storage, time_limit=time_limit)`.

    explor_noise_std follows the reference's recurrence (main.py:74-77, 237-239), one step of it per env-step collected, the warm-up's
    included: std <- std - (init - min) / decay_timesteps while std > min, else min; decay_timesteps=None keeps it at init
    (use_explor_noise_decay off).  Deviation: the reference applies it before every step, here a launch flies T steps, so the value
    at the horizon's first step is held for the horizon.  Likewise the warm-up ends at a horizon's boundary.
    time_limit "solved" sets buffer.time_limit_rule.x_lim to the env's.  Nothing synchronises, and from the second call of each kind
    nothing is allocated.  total_timesteps: env-steps collected per env so far, a host int.
    noise_source="device": the warm-up's actions are ONE uniform `noise_fill` launch in (-1, 1) under (noise_seed, draw = total_timesteps,
    stream COLLECTOR_STREAM, which no updater's tensor has) instead of torch's three; it takes no generator.
    track_episodes=True: the collector owns `episodes`, an `EpisodeTracker` with the buffer's time-limit rule (x_lim the env's), and
    every `collect` ends with `episodes.update(storage, record=total_timesteps >= start_timesteps)`, total_timesteps read before the
    horizon is counted: warm-up horizons advance the carries and are not recorded (main.py:218).  False: `episodes` is None."""
    ALGOS = ("td3", "sac")

    def __init__(self, env, buffer: ReplayBuffer, horizon: int, start_timesteps: int = 0, algo: str = "td3", explor_noise_std_init: float = 0.3,
                 explor_noise_std_min: float = 0.05, decay_timesteps: Optional[int] = None, time_limit: str = "solved",
                 generator: Optional[torch.Generator] = None, noise_source: str = "torch", noise_seed: int = 0, track_episodes: bool = False):
        what = "OffPolicyCollector"
        self.noise_seed = _noise_source(what, noise_source, noise_seed, generator)
        self.noise_source = noise_source
        if algo not in self.ALGOS:
            raise ValueError(f"{what}: algo must be one of {self.ALGOS}, got {algo!r}")
        if time_limit not in TIME_LIMITS:
            raise ValueError(f"{what}: time_limit must be one of {TIME_LIMITS}, got {time_limit!r}")
        self.T, self.start_timesteps = int(horizon), int(start_timesteps)
        if self.T < 1 or self.start_timesteps < 0:
            raise ValueError(f"{what}: horizon must be >= 1 and start_timesteps >= 0")
        if decay_timesteps is not None and int(decay_timesteps) < 1:
            raise ValueError(f"{what}: decay_timesteps must be >= 1 (None: no decay)")
        self.std_init, self.std_min = float(explor_noise_std_init), float(explor_noise_std_min)
        if not 0.0 < self.std_min <= self.std_init < float("inf"):
            raise ValueError(f"{what}: need 0 < explor_noise_std_min <= explor_noise_std_init < inf, got {self.std_min}, {self.std_init}")
        if not isinstance(buffer, ReplayBuffer):
            raise ValueError(f"{what}: buffer must be a ReplayBuffer")
        if not getattr(env, "auto_reset", False):
            raise ValueError(f"{what} needs an env with auto_reset=True: a horizon runs through episode ends")
        if env.n_agents != buffer.n_agents or list(env.obs_dims) != buffer.obs_dims or sum(buffer.action_dims) != env.action_dim:
            raise ValueError(f"{what}: the env has {env.n_agents} agent(s) with observations {list(env.obs_dims)} and {env.action_dim} action "
                             f"columns; the buffer has {buffer.n_agents} with {buffer.obs_dims} and {buffer.action_dims}")
        if self.T * env.num_envs > buffer.capacity:
            raise ValueError(f"{what}: a horizon of {self.T} x {env.num_envs} transitions does not fit a buffer of {buffer.capacity}")
        if time_limit == "solved" and buffer.obs_dims[0] < 3:
            raise ValueError(f"{what}: time_limit='solved' reads ex, the first three words of agent 0's observation")
        self.env, self.buffer, self.algo, self.time_limit, self.generator = env, buffer, algo, time_limit, generator
        self.noise_std_decay = 0.0 if decay_timesteps is None else (self.std_init - self.std_min) / int(decay_timesteps)
        self.explor_noise_std = self.std_init
        self.total_timesteps = 0
        if time_limit == "solved":
            buffer.time_limit_rule = buffer.time_limit_rule._replace(x_lim=float(env.x_lim))
        self.storage = RolloutStorage(env, self.T, action_dims=buffer.action_dims)
        self.random_actions = torch.empty(self.T, env.num_envs, env.action_dim, dtype=torch.float32, device=env.device) if self.start_timesteps else None
        # the training curve (main.py:212-235): None unless asked for — then one more C call per horizon, behind the append
        self.episodes = EpisodeTracker(self.storage, rule=buffer.time_limit_rule._replace(x_lim=float(env.x_lim))) if track_episodes else None

    @staticmethod
    def decay(std: float, noise_std_decay: float, std_min: float, steps: int = 1) -> float:
        """`steps` applications of main.py:237-239 to the exploration std."""
        for _ in range(steps):
            std = std - noise_std_decay if std > std_min else std_min
        return std

    def _check_actors(self, actors) -> list:
        what = "OffPolicyCollector.collect"
        actors = list(actors)
        if len(actors) != self.env.n_agents:
            raise ValueError(f"{what} needs one actor per agent ({self.env.n_agents}), got {len(actors)}")
        for a in actors:
            if self.algo == "td3" and (a.squash != _lib.ACTOR_TANH_MEAN or a.log_std is None or a.log_std_w is not None):
                raise ValueError(f"{what}: algo 'td3' takes tanh-of-mean actors with a log_std tensor (ActorParams.from_td3_module)")
            if self.algo == "sac" and (a.squash != _lib.ACTOR_TANH_SAMPLE or a.log_std_w is None):
                raise ValueError(f"{what}: algo 'sac' takes tanh-of-sample actors with a log_std head (ActorParams.from_sac_module)")
        return actors

    def collect(self, actors, **kw) -> RolloutStorage:
        """One horizon into `storage` and from there into the buffer.  actors: one `ActorParams` per agent (checked in the warm-up too);
        kw goes to `RolloutStorage.collect` (noise, noise_seed, max_action).  Returns the storage."""
        env, st = self.env, self.storage
        actors = self._check_actors(actors)
        if self.total_timesteps < self.start_timesteps:
            cur = env._last_obs
            if cur is None:
                raise ValueError("no current observation: call env.get_norm_error_state() or env.step() first")
            st.set_initial_obs(cur)
            if self.noise_source == "device":   # one launch; the draw number is the env-steps collected so far
                noise_fill([self.random_actions], seed=self.noise_seed, draw=self.total_timesteps, streams=[COLLECTOR_STREAM], kind="uniform")
            else:
                self.random_actions.uniform_(0.0, 1.0, generator=self.generator).mul_(2.0).sub_(1.0)
            env.rollout(self.random_actions, out=st.horizon())
            st.act_all.copy_(self.random_actions)   # (the given-actions rollout does not write the action rows)
        else:
            if self.algo == "td3":
                for a in actors:
                    a.log_std.fill_(math.log(self.explor_noise_std))
            st.collect(env, actors, **kw)
        self.buffer.append(st, time_limit=self.time_limit)
        if self.episodes is not None:   # (total_timesteps is still the count before this horizon: warm-up horizons are not recorded)
            self.episodes.update(st, record=self.total_timesteps >= self.start_timesteps)
        self.explor_noise_std = self.decay(self.explor_noise_std, self.noise_std_decay, self.std_min, self.T)
        self.total_timesteps += self.T
        return st
