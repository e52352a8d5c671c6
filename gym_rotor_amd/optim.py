"""The optimiser half of a PPO update on the device: `DeviceAdamW` — gradient-norm clipping, AdamW and the cosine schedule with warm
restarts in one launch (`qr_adamw_step`), with the step count and the schedule in device memory — and `PpoUpdater`, the K-epoch,
shuffle and minibatch loop of the reference's `PPO.train` (algos/ppo/ppo.py:148-214) over `actor_loss`, `critic_loss` and those steps.
`PolyakAdamW` (`qr_adamw_polyak_step`) is the same step for up to sixteen tensors with the soft target update and SAC's
exp(log_alpha) in the same launch: the optimiser of `offpolicy.Td3Updater` / `offpolicy.SacUpdater`.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import torch

from . import _checks as ck
from . import _lib
from .noise import check_seed, noise_fill
from .policy import actor_loss, critic_loss
from .shuffle import ppo_stream, shuffle


def _f32(v) -> float:
    """The float32 the C-ABI holds for `v`."""
    return C.c_float(float(v)).value


class DeviceAdamW:
    """`clip_grad_norm_(params, max_norm)`, `torch.optim.AdamW(params, lr, betas, eps, weight_decay).step()` and
    `CosineAnnealingWarmRestarts(T_0=t0, eta_min).step()` — in that order, the reference's (ppo.py:185-190) — as ONE launch per
    `step()`.  max_norm < 0: no clipping; t0 = 0: a constant rate.  The reference's values: max_norm=100, t0=1_000_000, eta_min=1e-5,
    lr 3e-4 (actors) / 2e-4 (critics).

    params: 1..8 contiguous float32 tensors on one device, 65 536 entries at the most together; they are updated in place (a live
    module's parameters: the next launch of the library reads the new weights).  `step()` reads each parameter's `.grad` (contiguous
    float32, as `actor_loss` / `critic_loss` leave them), synchronises nothing and allocates nothing.
    Deviations from torch: `.grad` is READ ONLY — it keeps the unclipped gradient, where clip_grad_norm_ scales it in place; betas,
    eps, weight_decay and max_norm are held as float32 (the attributes show the values in use: beta2 = 0.999 is 0.99900001287...).
    State: `exp_avg`, `exp_avg_sq` (flat float32, the tensors back to back), `step_count` (int64 [1]) and `stats` (float32 [4] = the
    last step's gradient norm, clip coefficient, learning rate and step number) on the parameters' device."""

    def __init__(self, params, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, max_norm: float = -1.0,
                 t0: int = 0, eta_min: float = 0.0):
        self.params = list(params)
        if not 1 <= len(self.params) <= _lib.ADAMW_MAX_TENSORS:
            raise ValueError(f"DeviceAdamW takes 1..{_lib.ADAMW_MAX_TENSORS} parameter tensors, got {len(self.params)}")
        self.device = self.params[0].device
        for k, p in enumerate(self.params):
            if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or not p.is_contiguous() or p.numel() < 1:
                raise ValueError(f"DeviceAdamW: parameter {k} must be a contiguous float32 tensor with at least one entry")
            if p.device != self.device:
                raise ValueError(f"DeviceAdamW: parameter {k} is on {p.device}, parameter 0 on {self.device}")
        self.numel = sum(p.numel() for p in self.params)
        if self.numel > _lib.ADAMW_MAX_ENTRIES:
            raise ValueError(f"DeviceAdamW: {self.numel} entries, at most {_lib.ADAMW_MAX_ENTRIES} per optimiser")
        self._set_hyper(dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm, t0=t0, eta_min=eta_min))
        self.exp_avg = torch.zeros(self.numel, dtype=torch.float32, device=self.device)
        self.exp_avg_sq = torch.zeros(self.numel, dtype=torch.float32, device=self.device)
        self.step_count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.stats = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._group = _lib.QrAdamWGroup()

    def _set_hyper(self, h):
        lr, eta_min, t0 = float(h["lr"]), float(h["eta_min"]), int(h["t0"])
        betas = (_f32(h["betas"][0]), _f32(h["betas"][1]))
        eps, weight_decay, max_norm = _f32(h["eps"]), _f32(h["weight_decay"]), _f32(h["max_norm"])
        for name, v in (("lr", lr), ("eta_min", eta_min), ("eps", eps), ("weight_decay", weight_decay)):
            if not (v >= 0.0 and math.isfinite(v)):
                raise ValueError(f"DeviceAdamW: {name} must be finite and >= 0, got {v}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"DeviceAdamW: betas must lie in [0, 1), got {betas}")
        if t0 < 0 or math.isnan(max_norm):
            raise ValueError("DeviceAdamW: t0 must be >= 0 and max_norm a number (negative: no clipping)")
        self.lr, self.eta_min, self.t0, self.betas, self.eps, self.weight_decay, self.max_norm = lr, eta_min, t0, betas, eps, weight_decay, max_norm

    def hyper(self) -> dict:
        return dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, max_norm=self.max_norm, t0=self.t0,
                    eta_min=self.eta_min)

    def _grads(self) -> list:
        """The parameters' current .grad tensors, checked.  This runs once per minibatch for every parameter, so the test stands here
        and `_checks.flat` only words the refusal."""
        grads = []
        for k, p in enumerate(self.params):
            g = p.grad
            if g is None:
                raise ValueError(f"{type(self).__name__}.step: parameter {k} has no .grad")
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.device or g.numel() != p.numel():
                ck.flat(f"{type(self).__name__}.step", f"the .grad of parameter {k}", g, torch.float32, p.numel(), self.device)
            grads.append(g)
        return grads

    def _fill(self) -> _lib.QrAdamWGroup:
        """The launch struct of the next step, from the parameters' current .grad tensors."""
        return _lib.adamw_group(self._group, self.params, self._grads(), self.exp_avg, self.exp_avg_sq, self.step_count, self.stats, **self.hyper())

    def step(self) -> None:
        """One optimiser step (clip, AdamW, schedule) in one launch on the current stream."""
        DeviceAdamW.step_all([self])

    @staticmethod
    def step_all(opts: Sequence["DeviceAdamW"]) -> None:
        """One step of each of several optimisers on one device in ONE launch (one workgroup each; more than 8: one launch per 8).
        The result is that of stepping them one by one."""
        opts = list(opts)
        if not opts:
            return
        dev = opts[0].device
        if any(o.device != dev for o in opts):
            raise ValueError("DeviceAdamW.step_all: the optimisers must be on one device")
        if len({id(o) for o in opts}) != len(opts):
            raise ValueError("DeviceAdamW.step_all: an optimiser appears twice")
        groups = [o._fill() for o in opts]
        ck.require_gpu(dev)
        for i in range(0, len(groups), _lib.ADAMW_MAX_GROUPS):
            chunk = groups[i:i + _lib.ADAMW_MAX_GROUPS]
            _lib.launch(dev, "qr_adamw_step", (_lib.QrAdamWGroup * len(chunk))(*chunk), len(chunk))

    @property
    def steps(self) -> int:
        """Steps taken so far (a host read of the device counter: for logging)."""
        return int(self.step_count.item())

    def current_lr(self) -> float:
        """The rate the NEXT step uses — `scheduler.get_last_lr()[0]` after `steps` steps (a host read: for logging)."""
        if self.t0 == 0:
            return self.lr
        return self.eta_min + (self.lr - self.eta_min) * (1.0 + math.cos(math.pi * (self.steps % self.t0) / self.t0)) / 2.0

    def state_dict(self) -> dict:
        return {"step": self.step_count.clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(), "hyper": self.hyper()}

    def load_state_dict(self, state: dict) -> None:
        """Copies into the existing state tensors (their addresses stay: a captured graph keeps working)."""
        for name, dst in (("step", self.step_count), ("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            src = state[name]
            if src.dtype != dst.dtype or src.numel() != dst.numel():
                raise ValueError(f"DeviceAdamW.load_state_dict: {name} must be {dst.dtype} with {dst.numel()} entries")
        self._set_hyper(state["hyper"])
        for name, dst in (("step", self.step_count), ("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            dst.copy_(state[name].reshape(dst.shape))


def _check_pairs(what: str, params, grads, dev) -> None:
    """`adamw_step`'s and `adamw_polyak_step`'s check of the parameters and their gradients."""
    for k, (p, g) in enumerate(zip(params, grads)):
        for kind, t in (("parameter", p), ("gradient", g)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() != p.numel() or t.numel() < 1:
                raise ValueError(f"{what}: {kind} {k} must be a contiguous float32 tensor of {p.numel()} >= 1 entries on {dev}")


def _check_state(what: str, params, exp_avg, exp_avg_sq, step, stats, dev) -> int:
    """... and of the state tensors; returns the parameters' entries together."""
    total = sum(p.numel() for p in params)
    ck.flat(what, "exp_avg", exp_avg, torch.float32, total, dev)
    ck.flat(what, "exp_avg_sq", exp_avg_sq, torch.float32, total, dev)
    ck.scalar(what, "step", step, torch.int64, dev, optional=False)
    ck.flat(what, "stats", stats, torch.float32, 4, dev, True)
    return total


def adamw_step(params, grads, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: torch.Tensor, stats: Optional[torch.Tensor], *, lr: float,
               betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, max_norm: float = -1.0, t0: int = 0, eta_min: float = 0.0) -> None:
    """One `qr_adamw_step` launch for ONE group on explicit tensors (what `DeviceAdamW.step` does with its own state and the
    parameters' .grad): params / grads 1..8 contiguous float32 tensors each, exp_avg / exp_avg_sq float32 with as many entries as the
    parameters together, step int64 [1], stats float32 [4] or None — all on one device."""
    params, grads = list(params), list(grads)
    if not 1 <= len(params) <= _lib.ADAMW_MAX_TENSORS or len(grads) != len(params):
        raise ValueError(f"adamw_step takes 1..{_lib.ADAMW_MAX_TENSORS} parameter tensors and as many gradients")
    dev = params[0].device
    _check_pairs("adamw_step", params, grads, dev)
    _check_state("adamw_step", params, exp_avg, exp_avg_sq, step, stats, dev)
    ck.require_gpu(dev)
    g = _lib.adamw_group(None, params, grads, exp_avg, exp_avg_sq, step, stats, lr=lr, eta_min=eta_min, t0=t0, betas=betas, eps=eps,
                         weight_decay=weight_decay, max_norm=max_norm)
    _lib.launch(dev, "qr_adamw_step", g, 1)


class PolyakAdamW(DeviceAdamW):
    """`DeviceAdamW` for 1..16 tensors with what TD3.train / SAC.train do right after the optimiser step in the same launch
    (`qr_adamw_polyak_step`): the soft update of the parameters' target tensors (td3.py:207-211, sac.py:219-221) and, for SAC's
    one-entry `log_alpha`, alpha = exp(log_alpha) (sac.py:213).  Sixteen tensors hold the reference's twin critic as ONE group: one
    clip over all twelve tensors and one step counter, as `torch.optim.AdamW(critic.parameters())` has them (td3.py:166-171).

    targets: None, or one tensor (contiguous float32, the parameter's size and device, not the parameter itself) or None per
    parameter; `step(polyak=True)` leaves target = tau * param + (1 - tau) * target, the bits of `soft_update` run after the step, and
    `step(polyak=False)` leaves the targets alone (the iterations between TD3's delayed updates).  exp_out: a float32 tensor of one
    entry that every step leaves at exp(the new parameter); only for one parameter of one entry.  State, hyperparameters,
    `state_dict` / `load_state_dict` and the deviations from torch are `DeviceAdamW`'s; a group of at most 8 tensors without targets
    and exp_out gets `DeviceAdamW`'s bits."""

    def __init__(self, params, *, targets=None, tau: float = 0.005, exp_out: Optional[torch.Tensor] = None, lr: float, betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 1e-2, max_norm: float = -1.0, t0: int = 0, eta_min: float = 0.0):
        self.params = list(params)
        if not 1 <= len(self.params) <= _lib.POLYAK_MAX_TENSORS:
            raise ValueError(f"PolyakAdamW takes 1..{_lib.POLYAK_MAX_TENSORS} parameter tensors, got {len(self.params)}")
        self.device = self.params[0].device if isinstance(self.params[0], torch.Tensor) else None
        for k, p in enumerate(self.params):
            if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or not p.is_contiguous() or p.numel() < 1:
                raise ValueError(f"PolyakAdamW: parameter {k} must be a contiguous float32 tensor with at least one entry")
            if p.device != self.device:
                raise ValueError(f"PolyakAdamW: parameter {k} is on {p.device}, parameter 0 on {self.device}")
        self.numel = sum(p.numel() for p in self.params)
        if self.numel > _lib.ADAMW_MAX_ENTRIES:
            raise ValueError(f"PolyakAdamW: {self.numel} entries, at most {_lib.ADAMW_MAX_ENTRIES} per optimiser")
        self.targets = None
        if targets is not None:
            self.targets = list(targets)
            if len(self.targets) != len(self.params):
                raise ValueError(f"PolyakAdamW: targets holds {len(self.targets)} entries for {len(self.params)} parameters (None where there is none)")
            for k, (p, t) in enumerate(zip(self.params, self.targets)):
                if t is None:
                    continue
                if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel()
                        or t.device != self.device):
                    raise ValueError(f"PolyakAdamW: target {k} must be a contiguous float32 tensor of {p.numel()} entries on {self.device}")
                if t.data_ptr() == p.data_ptr():
                    raise ValueError(f"PolyakAdamW: target {k} is its own parameter")
        self.tau = float(tau)
        if not 0.0 <= self.tau <= 1.0:
            raise ValueError(f"PolyakAdamW: tau must lie in [0, 1], got {tau}")
        if exp_out is not None:
            if self.numel != 1:
                raise ValueError(f"PolyakAdamW: exp_out needs a group of one entry, this one has {self.numel}")
            if (not isinstance(exp_out, torch.Tensor) or exp_out.dtype != torch.float32 or exp_out.numel() != 1 or exp_out.device != self.device
                    or exp_out.data_ptr() == self.params[0].data_ptr()):
                raise ValueError(f"PolyakAdamW: exp_out must be a float32 tensor of one entry on {self.device}, not the parameter itself")
        self.exp_out = exp_out
        self._set_hyper(dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm, t0=t0, eta_min=eta_min))
        self.exp_avg = torch.zeros(self.numel, dtype=torch.float32, device=self.device)
        self.exp_avg_sq = torch.zeros(self.numel, dtype=torch.float32, device=self.device)
        self.step_count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.stats = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._group = _lib.QrAdamWPolyakGroup()

    def _set_hyper(self, h):
        try:
            super()._set_hyper(h)
        except ValueError as e:
            raise ValueError(str(e).replace("DeviceAdamW", "PolyakAdamW")) from None

    def _fill(self, polyak: bool = True) -> _lib.QrAdamWPolyakGroup:
        """The launch struct of the next step, from the parameters' current .grad tensors."""
        return _lib.adamw_polyak_group(self._group, self.params, self._grads(), self.targets if polyak else None, self.exp_avg, self.exp_avg_sq,
                                       self.step_count, self.stats, self.exp_out, tau=self.tau, **self.hyper())

    def step(self, polyak: bool = True) -> None:
        """One optimiser step (clip, AdamW, schedule), the targets' soft update when `polyak`, and exp_out — one launch."""
        PolyakAdamW.step_all([(self, polyak)])

    @staticmethod
    def step_all(opts) -> None:
        """One step of each of several optimisers on one device in ONE launch (one workgroup each; more than 7: one launch per 7).
        opts: (optimiser, polyak) pairs, or optimisers (polyak = True).  The result is that of stepping them one by one."""
        pairs = [o if isinstance(o, tuple) else (o, True) for o in opts]
        if not pairs:
            return
        for o, _ in pairs:
            if not isinstance(o, PolyakAdamW):
                raise ValueError("PolyakAdamW.step_all takes PolyakAdamW optimisers (DeviceAdamW.step_all steps the others)")
        dev = pairs[0][0].device
        if any(o.device != dev for o, _ in pairs):
            raise ValueError("PolyakAdamW.step_all: the optimisers must be on one device")
        if len({id(o) for o, _ in pairs}) != len(pairs):
            raise ValueError("PolyakAdamW.step_all: an optimiser appears twice")
        groups = [o._fill(bool(polyak)) for o, polyak in pairs]
        ck.require_gpu(dev)
        for i in range(0, len(groups), _lib.POLYAK_MAX_GROUPS):
            chunk = groups[i:i + _lib.POLYAK_MAX_GROUPS]
            _lib.launch(dev, "qr_adamw_polyak_step", (_lib.QrAdamWPolyakGroup * len(chunk))(*chunk), len(chunk))


def adamw_polyak_step(params, grads, targets, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: torch.Tensor, stats: Optional[torch.Tensor],
                      exp_out: Optional[torch.Tensor] = None, *, tau: float = 0.005, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                      weight_decay: float = 1e-2, max_norm: float = -1.0, t0: int = 0, eta_min: float = 0.0) -> None:
    """One `qr_adamw_polyak_step` launch for ONE group on explicit tensors (what `PolyakAdamW.step` does with its own state and the
    parameters' .grad): params / grads 1..16 contiguous float32 tensors each, targets None or one tensor or None per parameter,
    exp_avg / exp_avg_sq / step / stats as `adamw_step` takes them, exp_out float32 [1] or None (a group of one entry only) — all on
    one device."""
    params, grads = list(params), list(grads)
    if not 1 <= len(params) <= _lib.POLYAK_MAX_TENSORS or len(grads) != len(params):
        raise ValueError(f"adamw_polyak_step takes 1..{_lib.POLYAK_MAX_TENSORS} parameter tensors and as many gradients")
    dev = params[0].device
    what = "adamw_polyak_step"
    _check_pairs(what, params, grads, dev)
    if targets is not None:
        targets = list(targets)
        if len(targets) != len(params):
            raise ValueError("adamw_polyak_step: targets holds one entry per parameter (None where there is none)")
        for k, (p, t) in enumerate(zip(params, targets)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() != p.numel()
                                  or t.data_ptr() == p.data_ptr()):
                raise ValueError(f"adamw_polyak_step: target {k} must be a contiguous float32 tensor of {p.numel()} entries on {dev}, not the "
                                 f"parameter itself")
    if not 0.0 <= float(tau) <= 1.0:
        raise ValueError(f"adamw_polyak_step: tau must lie in [0, 1], got {tau}")
    total = _check_state(what, params, exp_avg, exp_avg_sq, step, stats, dev)
    if exp_out is not None and (total != 1 or exp_out.dtype != torch.float32 or exp_out.numel() != 1 or exp_out.device != dev
                                or exp_out.data_ptr() == params[0].data_ptr()):
        raise ValueError(f"adamw_polyak_step: exp_out must be a float32 tensor of one entry on {dev}, for a group of one entry")
    ck.require_gpu(dev)
    g = _lib.adamw_polyak_group(None, params, grads, targets, exp_avg, exp_avg_sq, step, stats, exp_out, tau=tau, lr=lr, eta_min=eta_min, t0=t0,
                                betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm)
    _lib.launch(dev, "qr_adamw_polyak_step", g, 1)


def minibatch_slices(n_rows: int, batch_size: int):
    """The contiguous slices of a permutation of n_rows that are its minibatches: ceil(n_rows / batch_size) of them, the last one
    shorter (ppo.py:152-153, 168, 194)."""
    n_rows, batch_size = int(n_rows), int(batch_size)
    if n_rows < 1 or batch_size < 1:
        raise ValueError("minibatch_slices needs n_rows >= 1 and batch_size >= 1")
    return [slice(i, min(i + batch_size, n_rows)) for i in range(0, n_rows, batch_size)]


SOURCES = ("torch", "device")        # who shuffles and who draws: torch's generator, or the library's keyed streams (shuffle.py, noise.py)
NOISE_STD = 0.05                     # policy_regularization's N(0, 0.05) row (policy_regularization.py:21)


class PpoUpdater:
    """`PPO.train`'s update loop (ppo.py:148-214) for all agents of an env kind, after `compute_gae` / `normalize`: per agent and
    epoch one shuffle, then the actor's minibatches (`actor_loss`, then a `DeviceAdamW` step), then the critic's (`critic_loss`, then
    a step).  When actor_batch_size == critic_batch_size the two halves walk the minibatches together — `actor_loss`, `critic_loss`,
    then ONE `DeviceAdamW.step_all` launch for both networks; the result is the same bits, since neither network reads the other
    during an update.  Otherwise they are stepped separately, in the reference's order.

    actors / critics: one live module per agent (attributes fc1, fc2, mean_linear, log_std / fc1, fc2, fc3), read and updated in
    place; actor_opts / critic_opts: their `DeviceAdamW`s; critic_inputs: per agent the observation rows its critic reads ((k,) by
    default, (0, 1) for CTDE).  noise / nominal: per agent the [D_k] draw of the spatial term and the [A_k] nominal action
    (`RolloutStorage.nominal_action`), required when lam_S / lam_M != 0; the noise tensor is read at every minibatch, so the caller
    may refill it in place between updates.  The hyperparameters are the reference's names and defaults (args_parse.py:65-78).

    shuffle_source / noise_source ("torch" by default: the behaviour and the bits described above).  "device" takes the epoch's
    permutation from `shuffle` into one kept [rows] buffer, and draws agent k's [D_k] noise row afresh before EVERY actor minibatch,
    as the reference does, with `noise_fill(kind="normal", a=0, b=noise_std)` into a tensor the updater owns (`noise=` is then
    refused) — both keyed by `seed`, the streams `ppo_stream(k, "shuffle")` / `ppo_stream(k, "noise")` and two draw numbers that
    live on the device: `state` int64 [2] = the shuffles and the noise rows drawn so far, each advanced by an in-place add behind its
    reader (host copies: `epoch_draw`, `minibatch_draw`).  With either device source the entropy coefficient is also kept in the
    float32 device word `entropy_dev`, set from the host's value after each decay and read by the launch (`entropy_coef_dev=`): the
    float32 the by-value path would pass.  So nothing in an epoch depends on a host value, and `capture` can record it."""

    def __init__(self, actors, critics, actor_opts, critic_opts, *, critic_inputs=None, K_epochs: int = 20, actor_batch_size: int = 128,
                 critic_batch_size: int = 128, clip: float = 0.2, entropy_coef: float = 1e-2, entropy_coef_decay: float = 0.99,
                 l2_reg: float = 1e-4, lam_T: float = 0.4, lam_S: float = 0.3, lam_M: float = 0.6, noise=None, nominal=None,
                 max_action: float = 1.0, shuffle_source: str = "torch", noise_source: str = "torch", seed: int = 0,
                 noise_std: float = NOISE_STD):
        self.actors, self.critics, self.actor_opts, self.critic_opts = list(actors), list(critics), list(actor_opts), list(critic_opts)
        n = len(self.actors)
        if n < 1 or not (len(self.critics) == len(self.actor_opts) == len(self.critic_opts) == n):
            raise ValueError("PpoUpdater needs one actor, critic, actor optimiser and critic optimiser per agent")
        for name, v in (("shuffle_source", shuffle_source), ("noise_source", noise_source)):
            if v not in SOURCES:
                raise ValueError(f"PpoUpdater: {name} must be one of {SOURCES}, got {v!r}")
        self.shuffle_source, self.noise_source, self.seed = shuffle_source, noise_source, check_seed("PpoUpdater", seed)
        self.noise_std = float(noise_std)
        if not 0.0 <= self.noise_std <= 3.4028234663852886e38:
            raise ValueError(f"PpoUpdater: noise_std must be a finite float32 number >= 0, got {noise_std}")
        if noise_source == "device" and noise is not None:
            raise ValueError("PpoUpdater: noise_source='device' draws the noise rows itself; it takes no noise=")
        self.critic_inputs = [tuple(i) for i in critic_inputs] if critic_inputs is not None else [(k,) for k in range(n)]
        self.noise = list(noise) if noise is not None else [None] * n
        self.nominal = list(nominal) if nominal is not None else [None] * n
        if not (len(self.critic_inputs) == len(self.noise) == len(self.nominal) == n):
            raise ValueError("PpoUpdater: critic_inputs, noise and nominal are per agent")
        if int(K_epochs) < 1 or int(actor_batch_size) < 1 or int(critic_batch_size) < 1:
            raise ValueError("PpoUpdater: K_epochs and the batch sizes must be >= 1")
        self.K_epochs, self.actor_batch_size, self.critic_batch_size = int(K_epochs), int(actor_batch_size), int(critic_batch_size)
        self.clip, self.entropy_coef, self.entropy_coef_decay, self.l2_reg = float(clip), float(entropy_coef), float(entropy_coef_decay), float(l2_reg)
        self.lam_T, self.lam_S, self.lam_M, self.max_action = float(lam_T), float(lam_S), float(lam_M), float(max_action)
        dev = self.device = self.actor_opts[0].device
        self.actor_stats = [torch.zeros(4, dtype=torch.float32, device=dev) for _ in range(n)]
        self.critic_stats = [torch.zeros(4, dtype=torch.float32, device=dev) for _ in range(n)]
        self.device_sources = "device" in (shuffle_source, noise_source)
        self.epoch_draw, self.minibatch_draw = 0, 0
        self.state, self.entropy_dev, self._perm, self._rows = None, None, None, None
        if self.device_sources:
            self.state = torch.zeros(2, dtype=torch.int64, device=dev)
            self.entropy_dev = torch.full((1,), self.entropy_coef, dtype=torch.float32, device=dev)
        if noise_source == "device":
            self.noise = [torch.zeros(m.fc1.weight.shape[1], dtype=torch.float32, device=dev) for m in self.actors]

    def _epoch(self, storage, advantage: torch.Tensor, k: int, generator) -> None:
        """One epoch of agent k: the shuffle, then its minibatches.  With the device sources every launch reads what it needs on the
        device, so this is also what `capture` records."""
        rows = storage.T * storage.N
        a_kw = dict(clip=self.clip, entropy_coef=self.entropy_coef, lam_T=self.lam_T, lam_S=self.lam_S, lam_M=self.lam_M,
                    noise=self.noise[k], nominal=self.nominal[k], max_action=self.max_action, stats=self.actor_stats[k])
        if self.device_sources:
            a_kw["entropy_coef_dev"] = self.entropy_dev
        c_kw = dict(inputs=self.critic_inputs[k], l2_reg=self.l2_reg, stats=self.critic_stats[k])
        actor, critic, opt_a, opt_c = self.actors[k], self.critics[k], self.actor_opts[k], self.critic_opts[k]
        if self.shuffle_source == "device":
            perm = shuffle(self._perm, n=rows, seed=self.seed, draw=self.epoch_draw, stream=ppo_stream(k, "shuffle"), draw_dev=self.state[0:1])
            self.state[0:1].add_(1)                       # behind its reader, on the same stream
            self.epoch_draw += 1
        else:
            perm = torch.randperm(rows, device=storage.device, generator=generator)

        def actor_minibatch(sl):
            if self.noise_source == "device":
                noise_fill([self.noise[k]], seed=self.seed, draw=self.minibatch_draw, streams=[ppo_stream(k, "noise")], kind="normal", a=0.0,
                           b=self.noise_std, draw_dev=self.state[1:2])
                self.state[1:2].add_(1)
                self.minibatch_draw += 1
            actor_loss(actor, storage, k, advantage, perm[sl], **a_kw)

        if self.actor_batch_size == self.critic_batch_size:
            both = [opt_a, opt_c]
            for sl in minibatch_slices(rows, self.actor_batch_size):
                actor_minibatch(sl)
                critic_loss(critic, storage, k, perm[sl], **c_kw)
                DeviceAdamW.step_all(both)
        else:
            for sl in minibatch_slices(rows, self.actor_batch_size):
                actor_minibatch(sl)
                opt_a.step()
            for sl in minibatch_slices(rows, self.critic_batch_size):
                critic_loss(critic, storage, k, perm[sl], **c_kw)
                opt_c.step()

    def _decay(self) -> None:
        """The host's decay (ppo.py:149) and, with a device source, the word the launches read: the float32 of the host's value."""
        self.entropy_coef *= self.entropy_coef_decay
        if self.entropy_dev is not None:
            self.entropy_dev.fill_(self.entropy_coef)

    def update(self, storage, advantage: torch.Tensor, generator: Optional[torch.Generator] = None):
        """One PPO update from `storage` (after compute_gae: td_target is read from it) and the normalised `advantage`
        [T, N, n_agents].  Returns (actor_stats, critic_stats): per agent the stats tensors of the last minibatch, on the device,
        no synchronisation.  From the second call on nothing is allocated but the permutations — and with shuffle_source="device",
        which takes no generator, nothing at all."""
        if storage.n_agents != len(self.actors):
            raise ValueError(f"the storage has {storage.n_agents} agents, the updater {len(self.actors)}")
        if generator is not None and self.shuffle_source == "device":
            raise ValueError("PpoUpdater.update: shuffle_source='device' shuffles from the library's own stream (seed); it takes no torch generator")
        rows = storage.T * storage.N
        if self.shuffle_source == "device" and (self._perm is None or self._perm.numel() != rows):
            self._perm = torch.zeros(rows, dtype=torch.int64, device=storage.device)
        self._rows = rows
        self._decay()
        for k in range(len(self.actors)):
            for _ in range(self.K_epochs):
                self._epoch(storage, advantage, k, generator)
        return self.actor_stats, self.critic_stats

    def _grad_addresses(self):
        """The address of every parameter's .grad, None where there is none: what a recorded epoch writes and steps from."""
        return [None if p.grad is None else p.grad.data_ptr() for o in self.actor_opts + self.critic_opts for p in o.params]

    def capture(self, storage, advantage: torch.Tensor):
        """Record ONE epoch per agent — the shuffle, then per minibatch the noise row, `actor_loss`, `critic_loss`, the optimiser
        step(s) and the counter adds, a linear chain of launches — in one `torch.cuda.graph` each, and return a callable that
        performs one whole update: the host's entropy decay and the fill of its device word, then per agent K_epochs replays of that
        agent's graph, then the host counters.  It returns `update`'s stats tensors.  `storage` and `advantage` are read in place: a
        later `collect` / `compute_gae` into the same tensors is what the next call trains on.  Needs both device sources and one
        eager `update` on this storage before it, which makes the workspaces, the .grad tensors and the permutation buffer.
        Capturing runs nothing and leaves the host counters where they were.  The callable raises ValueError where a parameter's
        .grad has been rebound since (the graphs write and read the recorded tensors)."""
        if self.shuffle_source != "device" or self.noise_source != "device":
            raise ValueError("PpoUpdater.capture needs shuffle_source='device' and noise_source='device': a replay cannot follow torch's generator")
        if storage.n_agents != len(self.actors):
            raise ValueError(f"the storage has {storage.n_agents} agents, the updater {len(self.actors)}")
        if self._rows is None or self._perm is None or None in self._grad_addresses():
            raise ValueError("PpoUpdater.capture: run update() on this storage once first (it makes the workspaces the graphs record)")
        rows = storage.T * storage.N
        if rows != self._rows:
            raise ValueError(f"PpoUpdater.capture: the storage holds T * N = {rows} rows, the last update ran on {self._rows}")
        ck.require_gpu(self.device)
        host = (self.epoch_draw, self.minibatch_draw)
        graphs = []
        torch.cuda.synchronize(self.device)
        for k in range(len(self.actors)):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._epoch(storage, advantage, k, None)
            graphs.append(graph)
        per_update = tuple(c - h for c, h in zip((self.epoch_draw, self.minibatch_draw), host))   # one epoch of every agent
        self.epoch_draw, self.minibatch_draw = host                                               # nothing ran
        grads = self._grad_addresses()

        def replay():
            if self._grad_addresses() != grads:
                raise ValueError("PpoUpdater.capture: a parameter's .grad was rebound after the capture; capture again")
            self._decay()
            for graph in graphs:
                for _ in range(self.K_epochs):
                    graph.replay()
            self.epoch_draw += per_update[0] * self.K_epochs
            self.minibatch_draw += per_update[1] * self.K_epochs
            return self.actor_stats, self.critic_stats

        replay.graphs = graphs
        return replay

    def state_dict(self) -> dict:
        return {"seed": self.seed, "epoch_draw": self.epoch_draw, "minibatch_draw": self.minibatch_draw, "entropy_coef": self.entropy_coef}

    def load_state_dict(self, state: dict) -> None:
        """Copies into the existing device tensors (their addresses stay: a captured graph keeps working — under the seed it was
        recorded with: the seed is a launch argument)."""
        seed, e, m = check_seed("PpoUpdater.load_state_dict", state["seed"]), int(state["epoch_draw"]), int(state["minibatch_draw"])
        if not (0 <= e < 2 ** 63 and 0 <= m < 2 ** 63):
            raise ValueError("PpoUpdater.load_state_dict: the draw numbers must lie in [0, 2^63)")
        self.seed, self.epoch_draw, self.minibatch_draw, self.entropy_coef = seed, e, m, float(state["entropy_coef"])
        if self.state is not None:
            self.state.copy_(torch.tensor([e, m], dtype=torch.int64))
            self.entropy_dev.fill_(self.entropy_coef)

