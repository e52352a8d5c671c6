"""An evolution-strategy generation around the population evaluation launch: `es_perturb` writes the antithetic population
theta +- sigma eps in one launch (qr_es_perturb), `es_gradient` shapes the fitness and forms the gradient estimate in one C call
(qr_es_gradient), and `EvolutionStrategy.step()` is the whole generation: the common episodes, the perturbation,
`QuadVecEnv.evaluate_population`, the per-policy fitness, the estimator and `DeviceAdamW`.

The perturbation stream (include/quadrotor_hip.h, QrEsPerturb; restated in NumPy by tests/es_ref.py): the draw of antithetic pair j for
element e of a tensor with n elements and Q = ceil(n / 4) quads is element j * 4 Q + e of the `noise_fill` stream
(seed, draw = generation, stream id of the tensor, "normal", a = 0, b = 1).  So the eps of a generation is what `noise_fill` writes into
a [P / 2, 4 Q] tensor under that key, bit for bit, and it is never stored: the estimator regenerates it.  A generation is a function
of (seed, generation) alone — which is what a sharded run needs: each rank perturbs its own slice of the population with no broadcast.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import torch

from . import _checks as ck
from . import _lib
from .noise import check_seed
from .optim import DeviceAdamW
from .policy import ACTOR_DIMS, ActorParams, ActorPopulation, _WEIGHTS, module_grads, population_layout, population_view

NAMES = _WEIGHTS                      # the perturbed tensors of an actor, in stream order
SHAPINGS = tuple(_lib.ES_SHAPING_ID)
FITNESS = ("benchmark", "return")
ES_STREAM = 1 << 28                   # above every `offpolicy.noise_stream` id, below `offpolicy.COLLECTOR_STREAM`
MAX_POLICIES = _lib.ES_MAX_POLICIES


def es_stream(k: int, name: str) -> int:
    """The default stream id of agent k's tensor `name` (one of fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b)."""
    k = int(k)
    if name not in NAMES or not 0 <= k < 1 << 16:
        raise ValueError(f"es_stream: agent 0 <= k < 65536 and a name of {NAMES}, got {k}, {name!r}")
    return ES_STREAM | (k << 8) | NAMES.index(name)


def es_workspace_numel(n_policies: int) -> int:
    """float64 elements of workspace one `es_gradient` call needs (qr_es_workspace_bytes / 8)."""
    return _lib.workspace_bytes("qr_es_workspace_bytes", n_policies) // 8


def population_like(base_actors: Sequence[ActorParams], n: int) -> ActorPopulation:
    """An `ActorPopulation` of n policies with uninitialised stacked tensors of `base_actors`' sizes and form: what `es_perturb` fills."""
    n = int(n)
    if n < 1:
        raise ValueError("population_like needs n >= 1")
    agents = []
    for a in base_actors:
        cols = {name: None if getattr(a, name) is None else torch.empty((n,) + tuple(getattr(a, name).shape), dtype=torch.float32,
                                                                         device=getattr(a, name).device) for name in ActorParams.NAMES}
        agents.append(ActorParams(**cols, squash=a.squash))
    return ActorPopulation(agents)


def _check_key(what: str, n_policies, sigma, seed, generation, streams, n_tensors, dev, max_workgroups):
    """(P, sigma, seed, generation, generation_dev, streams) of one launch, checked."""
    P = int(n_policies)
    if P < 2 or P % 2 or P > MAX_POLICIES:
        raise ValueError(f"{what}: the population must hold an even number of policies in 2..{MAX_POLICIES}, got {P}")
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma) and sigma <= 3.4028234663852886e38) or C.c_float(sigma).value <= 0.0:
        raise ValueError(f"{what}: sigma must be a finite float32 number > 0, got {sigma}")
    seed = check_seed(what, seed)
    gen_dev = None
    if isinstance(generation, torch.Tensor):
        gen_dev, generation = generation, 0
        ck.scalar(what, "a generation on the device", gen_dev, torch.int64, dev)
    else:
        generation = int(generation)
        if not 0 <= generation < 2 ** 63:
            raise ValueError(f"{what}: generation must lie in [0, 2^63), got {generation}")
    streams = [int(s) for s in streams]
    if len(streams) != n_tensors or len(set(streams)) != n_tensors or min(streams) < 0 or max(streams) >= _lib.NOISE_MAX_STREAM:
        raise ValueError(f"{what}: streams must be {n_tensors} pairwise distinct ids in [0, 2^30), got {streams}")
    if int(max_workgroups) < 0:
        raise ValueError(f"{what}: max_workgroups must be >= 0")
    return P, sigma, seed, generation, gen_dev, streams


def _check_quads(what: str, tensors, P: int):
    if sum((t.numel() + 3) // 4 for t in tensors) * (P // 2) >= 2 ** 31:
        raise ValueError(f"{what}: (P / 2) * the tensors' quads of four elements must stay below 2^31")


def es_perturb_tensors(base: Sequence[torch.Tensor], out: Sequence[torch.Tensor], *, sigma: float, seed: int, generation, streams: Sequence[int],
                       copies=(), max_workgroups: int = 0) -> None:
    """One qr_es_perturb launch on explicit tensors: out[i] ([P, ...], P even) gets base[i] + sigma eps in its even rows and
    base[i] - sigma eps in its odd rows, eps of pair j from (seed, generation, streams[i]); copies: (src, dst) pairs, dst [P, ...] gets
    src in every row.  1..16 tensors and at most 8 copies, contiguous float32 on one device; generation: an int in [0, 2^63) or an int64
    device tensor of one element, which the launch reads.  Every check comes before the launch."""
    what = "es_perturb"
    base, out, copies = list(base), list(out), [tuple(c) for c in copies]
    if not 1 <= len(base) <= _lib.ES_MAX_TENSORS or len(out) != len(base):
        raise ValueError(f"{what}: 1..{_lib.ES_MAX_TENSORS} base tensors and as many stacked outputs, got {len(base)} and {len(out)}")
    if len(copies) > _lib.ES_MAX_COPIES:
        raise ValueError(f"{what}: at most {_lib.ES_MAX_COPIES} copied tensors, got {len(copies)}")
    if not isinstance(out[0], torch.Tensor) or out[0].dim() < 1:
        raise ValueError(f"{what}: out[0] must be a stacked [P, ...] tensor")
    dev = out[0].device
    P, sigma, seed, generation, gen_dev, streams = _check_key(what, out[0].shape[0], sigma, seed, generation, streams, len(base), dev, max_workgroups)
    pairs = [(f"base[{i}]", b, f"out[{i}]", o) for i, (b, o) in enumerate(zip(base, out))]
    pairs += [(f"copies[{i}] source", s, f"copies[{i}] destination", d) for i, (s, d) in enumerate(copies)]
    for sn, s, dn, d in pairs:
        if not isinstance(s, torch.Tensor) or s.dtype != torch.float32 or s.device != dev or not s.is_contiguous() or s.numel() < 1:
            raise ValueError(f"{what}: {sn} must be a non-empty contiguous float32 tensor on {dev}")
        if (not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or d.device != dev or not d.is_contiguous() or d.dim() < 1
                or d.shape[0] != P or d.numel() != P * s.numel()):
            raise ValueError(f"{what}: {dn} must be a contiguous float32 [{P}, {s.numel()} elements] tensor on {dev}")
    _check_quads(what, base, P)
    ck.require_gpu(dev)
    _lib.launch(dev, "qr_es_perturb", _lib.es_perturb_args(base, out, copies, streams, n_policies=P, sigma=sigma, seed=seed, generation=generation,
                                                           generation_dev=gen_dev, max_workgroups=max_workgroups))


def _default_streams(n_agents: int) -> List[int]:
    return [es_stream(k, name) for k in range(n_agents) for name in NAMES]


def es_perturb(base_actors: Sequence[ActorParams], population: ActorPopulation, *, sigma: float, seed: int, generation,
               streams: Optional[Sequence[int]] = None, max_workgroups: int = 0) -> ActorPopulation:
    """The evolution-strategy population of one generation, in place and in one launch: policy 2j of `population` becomes
    theta + sigma eps_j and policy 2j + 1 theta - sigma eps_j around `base_actors`, over the weight and bias tensors of every agent
    (fc1, fc2 and the mean head) — `ActorPopulation.perturb`'s arithmetic (the same float32 product, then one rounding of each member)
    with eps from the keyed stream; the log_std source is copied into every row.  base_actors: one `ActorParams` per agent;
    population: an `ActorPopulation` of P policies of the same sizes and form (`population_like`), P even in 2..8192.
    streams: one id per perturbed tensor, agent by agent in the order of `NAMES`; default `es_stream(k, name)`.  Returns `population`."""
    base_actors = list(base_actors)
    if not isinstance(population, ActorPopulation) or len(population.agents) != len(base_actors) or not base_actors:
        raise ValueError(f"es_perturb: population must be an ActorPopulation of {len(base_actors)} agent(s), like base_actors")
    base, out, copies = [], [], []
    for k, (a, s) in enumerate(zip(base_actors, population.agents)):
        if a.squash != s.squash:
            raise ValueError(f"es_perturb: agent {k}: the population and the base differ in form (squash rule)")
        for name in ActorParams.NAMES:
            t, o = getattr(a, name), getattr(s, name)
            if (t is None) != (o is None):
                raise ValueError(f"es_perturb: agent {k}: the population and the base differ in form (tensor {name})")
            if t is None:
                continue
            if tuple(o.shape[1:]) != tuple(t.shape):
                raise ValueError(f"es_perturb: agent {k}: stacked tensor {name} must be [P, {', '.join(map(str, t.shape))}], got {tuple(o.shape)}")
            if name in NAMES:
                base.append(t.detach()), out.append(o)
            else:
                copies.append((t.detach(), o))
    es_perturb_tensors(base, out, sigma=sigma, seed=seed, generation=generation, copies=copies, max_workgroups=max_workgroups,
                       streams=_default_streams(len(base_actors)) if streams is None else streams)
    return population


def _shaping(what: str, shaping) -> int:
    if shaping not in _lib.ES_SHAPING_ID:
        raise ValueError(f"{what}: shaping must be one of {SHAPINGS}, got {shaping!r}")
    return _lib.ES_SHAPING_ID[shaping]


def es_gradient(fitness: torch.Tensor, grads, *, sigma: float, seed: int, generation, streams: Optional[Sequence[int]] = None,
                shaping: str = "centered_rank", stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                max_workgroups: int = 0) -> torch.Tensor:
    """The evolution-strategy gradient estimate of one generation in one C call (qr_es_gradient):
        grads[e] = -(1 / (P sigma)) sum_j w_j eps_j[e],   w_j = u_2j - u_2j+1
    with eps regenerated from (seed, generation, stream) — the draws `es_perturb` used under the same key — and u the shaped fitness:
    "centered_rank" (rank / (P - 1) - 1/2, ties share their mean rank, a NaN ranks as -inf) or "standardize" ((f - mean) / (std + 1e-8);
    a non-finite fitness gives zero gradients).  The sum is float64 in a fixed order, rounded to float32 once: the same bits from call
    to call.  The sign makes it a descent gradient: an optimiser step on it ascends the fitness.
    fitness: contiguous float32 [P], policy 2j and 2j + 1 the antithetic pair j; grads: one {name: tensor} dict per agent over `NAMES`
    (then streams defaults to `es_stream(k, name)`), or a flat sequence of 1..16 tensors with `streams` given — contiguous float32 of the
    base tensors' sizes, overwritten.  stats: float64 [4], made when None: fitness mean, maximum, index of the maximum, and 1 where a
    fitness is not finite; workspace: float64 [>= es_workspace_numel(P)], made when None.  Returns stats."""
    what = "es_gradient"
    grads = list(grads)
    if grads and all(isinstance(g, dict) for g in grads):
        for k, g in enumerate(grads):
            if any(n not in g for n in NAMES):
                raise ValueError(f"{what}: grads[{k}] must hold a tensor for each of {NAMES}")
        flat = [g[n] for g in grads for n in NAMES]
        if streams is None:
            streams = _default_streams(len(grads))
    else:
        flat = grads
        if streams is None:
            raise ValueError(f"{what}: a flat sequence of gradient tensors needs streams")
    if not 1 <= len(flat) <= _lib.ES_MAX_TENSORS:
        raise ValueError(f"{what}: 1..{_lib.ES_MAX_TENSORS} gradient tensors, got {len(flat)}")
    if not isinstance(fitness, torch.Tensor) or fitness.dtype != torch.float32 or fitness.dim() != 1 or not fitness.is_contiguous():
        raise ValueError(f"{what}: fitness must be a contiguous float32 [P] tensor")
    dev = fitness.device
    P, sigma, seed, generation, gen_dev, streams = _check_key(what, fitness.numel(), sigma, seed, generation, streams, len(flat), dev, max_workgroups)
    shaping = _shaping(what, shaping)
    for i, g in enumerate(flat):
        if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.device != dev or not g.is_contiguous() or g.numel() < 1:
            raise ValueError(f"{what}: gradient tensor {i} must be a non-empty contiguous float32 tensor on {dev}")
    _check_quads(what, flat, P)
    if stats is not None and (not isinstance(stats, torch.Tensor) or stats.dtype != torch.float64 or stats.device != dev
                              or stats.numel() != _lib.ES_STATS or not stats.is_contiguous()):
        raise ValueError(f"{what}: stats must be a contiguous float64 [{_lib.ES_STATS}] tensor on {dev}")
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float64 or workspace.device != dev
                                  or workspace.numel() < P // 2 or not workspace.is_contiguous()):
        raise ValueError(f"{what}: workspace must be a contiguous float64 tensor of at least {P // 2} elements on {dev}")
    ck.require_gpu(dev)
    if stats is None:
        stats = torch.empty(_lib.ES_STATS, dtype=torch.float64, device=dev)
    if workspace is None:
        workspace = torch.empty(es_workspace_numel(P), dtype=torch.float64, device=dev)
    g = _lib.es_gradient_args(fitness, flat, stats, workspace, streams, shaping=shaping, n_policies=P, sigma=sigma, seed=seed,
                              generation=generation, generation_dev=gen_dev, max_workgroups=max_workgroups)
    _lib.launch(dev, "qr_es_gradient", g)
    return stats


def population_fitness(flat: dict, n_policies: int, envs_per_policy: int, fitness: str = "benchmark", out: Optional[torch.Tensor] = None,
                       scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [P]: the per-policy mean over its E episodes of one metric of `QuadVecEnv.evaluate_population`'s result `flat`:
    "benchmark" (the benchmark reward) or "return" (the episode return, summed over the agents).  The sum and the division by E are
    float64 (`scratch` [P], made when None), the result is rounded to float32 once (`out`, made when None)."""
    if fitness not in FITNESS:
        raise ValueError(f"fitness must be one of {FITNESS}, got {fitness!r}")
    P, E = int(n_policies), int(envs_per_policy)
    key = "benchmark" if fitness == "benchmark" else "episode_return"
    v = population_view(flat[key], P, E)
    if scratch is None:
        scratch = torch.empty(P, dtype=torch.float64, device=v.device)
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=v.device)
    torch.sum(v, dim=tuple(range(1, v.dim())), out=scratch)
    scratch.div_(E)
    out.copy_(scratch)
    return out


def _module_params(module, k: int):
    try:
        return [module.fc1.weight, module.fc1.bias, module.fc2.weight, module.fc2.bias, module.mean_linear.weight, module.mean_linear.bias]
    except AttributeError:
        raise ValueError(f"EvolutionStrategy: actor module {k} must have the reference's attributes fc1, fc2, mean_linear and log_std") from None


class EvolutionStrategy:
    """An evolution strategy on the reference's MLP actors, one generation per `step()`:

        es = EvolutionStrategy("coupled", [actor], population=1024, episodes_per_policy=64, sigma=0.05, seed=0)
        for _ in range(100):
            stats = es.step()          # float64 [4] on the device: fitness mean, max, index of the max, non-finite flag

    actor_modules: one live module per agent (attributes fc1, fc2, mean_linear, log_std; `ActorParams.from_module`) on the GPU; their
    weights are the base theta and are updated in place.  One `QuadVecEnv` of population x roundup(episodes_per_policy, 64) envs and one
    `ActorPopulation` are built once and reused.  step(), in this order: (1) the common-random-number episodes — prepared once as
    `evaluate.evaluate_population` prepares them (reset(env_type='eval', seed), the fused generator of `traj_mode`, the first
    observation) — are copied into every policy's block; (2) `es_perturb` under (seed, generation); (3) `env.evaluate_population`,
    max_steps steps at the most (default round(5 s / dt)); (4) `population_fitness`: the per-policy mean of `fitness`; (5) `es_gradient`
    into the modules' .grad; (6) `DeviceAdamW.step_all` (one optimiser per agent; `optimizer`: DeviceAdamW's keywords, default lr = 0.01
    without weight decay) — ascent on the fitness.  step() returns the stats tensor (overwritten by the next call), synchronises
    nothing and allocates no device memory from the second call on; `generation` advances by one per call.  log_std is not perturbed.
    The modules' weight tensors and their .grad tensors are captured at construction and must not be rebound afterwards
    (zero_grad(set_to_none=True), module.to(...), an assigned .grad): step() checks their identity and raises.
    env_kw: device, substeps, layout, env_offset, max_action."""

    def __init__(self, kind: str, actor_modules, *, population: int, episodes_per_policy: int, sigma: float = 0.05, seed: int,
                 traj_mode: Optional[int] = 0, fitness: str = "benchmark", shaping: str = "centered_rank", max_steps: Optional[int] = None,
                 optimizer: Optional[dict] = None, **env_kw):
        what = "EvolutionStrategy"
        if kind not in ACTOR_DIMS:
            raise ValueError(f"{what}: kind must be 'coupled' or 'decoupled' (Quad-v0 has no actor), got {kind!r}")
        modules = list(actor_modules) if isinstance(actor_modules, (list, tuple)) else [actor_modules]
        if len(modules) != len(ACTOR_DIMS[kind]):
            raise ValueError(f"{what}: kind {kind!r} needs {len(ACTOR_DIMS[kind])} actor module(s), got {len(modules)}")
        P, E = int(population), int(episodes_per_policy)
        if P < 2 or P % 2 or P > MAX_POLICIES:
            raise ValueError(f"{what}: population must be even and in 2..{MAX_POLICIES}, got {P}")
        if E < 1:
            raise ValueError(f"{what}: episodes_per_policy must be >= 1, got {E}")
        sigma = float(sigma)
        if not (sigma > 0.0 and math.isfinite(sigma)):
            raise ValueError(f"{what}: sigma must be finite and > 0, got {sigma}")
        if fitness not in FITNESS:
            raise ValueError(f"{what}: fitness must be one of {FITNESS}, got {fitness!r}")
        _shaping(what, shaping)
        if max_steps is not None and int(max_steps) < 1:
            raise ValueError(f"{what}: max_steps must be >= 1")
        unknown = set(env_kw) - {"device", "substeps", "layout", "env_offset", "max_action"}
        if unknown:
            raise ValueError(f"{what}: unknown keyword(s) {sorted(unknown)}")
        self.kind, self.n_policies, self.envs_per_policy, self.sigma, self.seed = kind, P, E, sigma, check_seed(what, seed)
        self.traj_mode, self.fitness, self.shaping = traj_mode, fitness, shaping
        self.max_action = float(env_kw.pop("max_action", 1.0))
        self.generation = 0
        self._max_steps = None if max_steps is None else int(max_steps)
        self.modules = modules
        self.params = [_module_params(m, k) for k, m in enumerate(modules)]
        self.base = [ActorParams.from_module(m) for m in modules]
        for a, d in zip(self.base, ACTOR_DIMS[kind]):
            a.check(d, self.base[0].fc1_w.device)
        self.optimizers = [DeviceAdamW(p, **dict(dict(lr=1e-2, weight_decay=0.0), **(optimizer or {}))) for p in self.params]
        self._build(env_kw)

    def _build(self, env_kw):
        """The env, the prepared episodes, the population and every buffer a generation touches."""
        from .evaluate import _prepare_episodes, _tile_episodes
        from .vec_env import QuadVecEnv
        P, E = self.n_policies, self.envs_per_policy
        _, n = population_layout(P, E)
        self._src, src_obs = _prepare_episodes(self.kind, E, self.traj_mode, self.seed, **env_kw)
        self.env = QuadVecEnv(self.kind, n, seed=self.seed, goal_mode=self.traj_mode, autotune=False, **env_kw)
        dev = self.env.device
        if self.base[0].fc1_w.device != dev:
            raise ValueError(f"EvolutionStrategy: the actor modules are on {self.base[0].fc1_w.device}, the env on {dev}")
        self.max_steps = int(round(5.0 / self.env.dt)) if self._max_steps is None else self._max_steps
        self._obs = _tile_episodes(self._src, src_obs, self.env, P)
        self.population = population_like(self.base, P)
        G, A = self.env.n_agents, self.env.action_dim
        self._out = {"episode_return": torch.zeros(n, G, dtype=torch.float64, device=dev), "benchmark": torch.zeros(n, dtype=torch.float64, device=dev),
                     "length": torch.zeros(n, dtype=torch.int32, device=dev), "terminated": torch.zeros(n, dtype=torch.bool, device=dev),
                     "success": torch.zeros(n, G, dtype=torch.bool, device=dev), "final_error": torch.zeros(n, 4, dtype=torch.float32, device=dev),
                     "action": torch.zeros(n, A, dtype=torch.float32, device=dev)}
        for k, d in enumerate(self.env.obs_dims):
            self._out[f"obs{k}"] = torch.zeros(n, d, dtype=torch.float32, device=dev)
        self._fit64 = torch.zeros(P, dtype=torch.float64, device=dev)
        self.fitness_values = torch.zeros(P, dtype=torch.float32, device=dev)   # the last generation's fitness [P]
        self.stats = torch.zeros(_lib.ES_STATS, dtype=torch.float64, device=dev)
        self._workspace = torch.zeros(es_workspace_numel(P), dtype=torch.float64, device=dev)
        self._grads = [module_grads(NAMES, params) for params in self.params]

    def prepare_episodes(self) -> list:
        """Step (1): the prepared episodes (state, parameters, integrators, goal, generator state, episode index) into every policy's
        block of the env; returns the observation rows the first actions are computed from."""
        from .evaluate import _tile_episodes
        return _tile_episodes(self._src, None, self.env, self.n_policies, obs=self._obs)

    def _check_bound(self):
        """The weights and .grad tensors captured at construction must still be the modules': a rebound one (zero_grad(set_to_none=True),
        module.to(...), an assigned .grad) would leave the estimator writing where the optimiser no longer reads."""
        for k, (params, grads, a) in enumerate(zip(self.params, self._grads, self.base)):
            for n, p in zip(NAMES, params):
                if p.grad is not grads[n] or p.data_ptr() != getattr(a, n).data_ptr():
                    raise RuntimeError(f"EvolutionStrategy.step: agent {k}'s {n} or its .grad was rebound after construction; build a new "
                                       f"EvolutionStrategy (load_state_dict continues the stream)")

    def step(self) -> torch.Tensor:
        """One generation; returns stats (float64 [4] on the device, overwritten by the next call)."""
        P, E, key = self.n_policies, self.envs_per_policy, dict(sigma=self.sigma, seed=self.seed, generation=self.generation)
        self._check_bound()
        obs = self.prepare_episodes()
        es_perturb(self.base, self.population, **key)
        self.env.evaluate_population(self.population, E, max_steps=self.max_steps, obs=obs, max_action=self.max_action, out=self._out)
        population_fitness(self._out, P, E, self.fitness, out=self.fitness_values, scratch=self._fit64)
        es_gradient(self.fitness_values, self._grads, shaping=self.shaping, stats=self.stats, workspace=self._workspace, **key)
        DeviceAdamW.step_all(self.optimizers)
        self.generation += 1
        return self.stats

    def best(self) -> List[ActorParams]:
        """The fittest member of the last generation as per-agent `ActorParams` (copies; a host read of the stats)."""
        if self.generation < 1:
            raise ValueError("EvolutionStrategy.best: no generation has been evaluated yet")
        p = int(self.stats[2].item())
        return [ActorParams(*[None if getattr(a, n) is None else getattr(a, n).clone() for n in ActorParams.NAMES], a.squash)
                for a in self.population[p]]

    def state_dict(self) -> dict:
        """seed, generation, sigma and the optimisers' state: with the modules' own weights, what a resumed run needs to continue the
        same stream."""
        return {"seed": self.seed, "generation": self.generation, "sigma": self.sigma, "optimizers": [o.state_dict() for o in self.optimizers]}

    def load_state_dict(self, state: dict) -> None:
        if len(state["optimizers"]) != len(self.optimizers):
            raise ValueError(f"EvolutionStrategy.load_state_dict: {len(state['optimizers'])} optimiser states for {len(self.optimizers)} agent(s)")
        seed, generation, sigma = check_seed("EvolutionStrategy.load_state_dict", state["seed"]), int(state["generation"]), float(state["sigma"])
        if generation < 0 or not (sigma > 0.0 and math.isfinite(sigma)):
            raise ValueError("EvolutionStrategy.load_state_dict: generation must be >= 0 and sigma finite and > 0")
        if seed != self.seed:
            raise ValueError(f"EvolutionStrategy.load_state_dict: the state was saved under seed {seed}, this object prepared its episodes under "
                             f"{self.seed}")
        for o, s in zip(self.optimizers, state["optimizers"]):
            o.load_state_dict(s)
        self.generation, self.sigma = generation, sigma
