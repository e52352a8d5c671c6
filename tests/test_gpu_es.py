"""The evolution-strategy entries on the GPU (qr_es_perturb, qr_es_gradient; es.es_perturb, es.es_gradient, EvolutionStrategy).

The stream contract carries the tests: the eps of a generation is what `noise_fill` writes into a [P / 2, 4 Q] tensor under the same key,
so the perturbation is compared bit for bit with `ActorPopulation.perturb(eps=...)` on those draws, and the estimator with a long-double
sum over them on the host.  The utilities are compared with tests/es_ref.py exactly.  Every output sits between sentinel words."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import es_ref as R
from test_gpu_noise import SENTINEL, arena, bits, sentinels_intact

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 3
GENERATIONS = (0, 2 ** 32 + 1)
DIMS = ((23, 16, 4), (15, 16, 4), (3, 4, 1))   # (3, 4, 1): tensors of 1, 4 and 12 elements — a partial quad, rows that are not 16-byte aligned
SIGMA = 0.1
INF, NAN = float("inf"), float("nan")


def es():
    from gym_rotor_amd import es as ES
    return ES


def base_actor(dims, misaligned=(0, 3)):
    """A random actor whose tensors are carved from a sentinel arena (two of them one float past a 16-byte boundary)."""
    from gym_rotor_amd.policy import ActorParams
    a = ActorParams.random(*dims, device="cuda", generator=torch.Generator("cuda").manual_seed(5), log_std=-0.5)
    names = [n for n in ActorParams.NAMES if getattr(a, n) is not None]
    buf, views, guard = arena([getattr(a, n).numel() for n in names], misaligned)
    for n, v in zip(names, views):
        v.copy_(getattr(a, n).reshape(-1))
        setattr(a, n, v.view(getattr(a, n).shape))
    return a, (buf, guard)


def population_arena(a, P, misaligned=(1, 4)):
    """An ActorPopulation of P policies like `a`, its stacked tensors carved from a sentinel arena."""
    from gym_rotor_amd.policy import ActorParams, ActorPopulation
    names = [n for n in ActorParams.NAMES if getattr(a, n) is not None]
    buf, views, guard = arena([P * getattr(a, n).numel() for n in names], misaligned)
    cols = {n: None for n in ActorParams.NAMES}
    for n, v in zip(names, views):
        cols[n] = v.view((P,) + tuple(getattr(a, n).shape))
    return ActorPopulation([ActorParams(**cols, squash=a.squash)]), (buf, guard)


def draws(a, P, generation, streams=None, seed=SEED):
    """{name: float32 [P / 2, n]}: the generation's eps of every perturbed tensor, materialised by noise_fill into [P / 2, 4 Q] tensors."""
    from gym_rotor_amd import noise_fill
    ES = es()
    streams = [ES.es_stream(0, n) for n in ES.NAMES] if streams is None else streams
    full = [torch.empty(P // 2, 4 * R.quads(getattr(a, n).numel()), device="cuda") for n in ES.NAMES]
    noise_fill(full, seed=seed, draw=generation, streams=streams)
    return {n: t[:, :getattr(a, n).numel()].contiguous() for n, t in zip(ES.NAMES, full)}


# ---------------------------------------------------------------- the perturbation
@pytest.mark.parametrize("P", [2, 6, 130])
@pytest.mark.parametrize("dims", DIMS)
def test_perturbation_bit_for_bit(dims, P):
    from gym_rotor_amd.policy import ActorPopulation
    ES = es()
    a, (abuf, aguard) = base_actor(dims)
    before = abuf.clone()
    for generation in GENERATIONS:
        pop, (buf, guard) = population_arena(a, P)
        assert ES.es_perturb([a], pop, sigma=SIGMA, seed=SEED, generation=generation) is pop
        e = draws(a, P, generation)
        eps = [{n: torch.stack([e[n], -e[n]], 1).reshape((P,) + tuple(getattr(a, n).shape)) for n in ES.NAMES}]
        want, _ = ActorPopulation.perturb([a], P, SIGMA, eps=eps)
        for n in ES.NAMES:
            got, ref = getattr(pop.agents[0], n), getattr(want.agents[0], n)
            assert torch.equal(bits(got), bits(ref)), (n, generation)
            # a pair's members are one rounding each from theta +- d: their sum is 2 theta within half an ulp of each
            pair = got[0::2].double() + got[1::2].double() - 2.0 * getattr(a, n).double()
            assert bool((pair.abs() <= 2.0 ** -24 * (got[0::2].abs() + got[1::2].abs()).double()).all()), n
            assert not torch.equal(got[0], got[1])
        assert torch.equal(pop.agents[0].log_std, a.log_std.expand(P, -1))
        assert sentinels_intact(buf, guard)
    assert torch.equal(abuf, before)   # the base is only read


def test_generation_read_from_a_device_word():
    ES = es()
    a, _ = base_actor(DIMS[2])
    word = torch.tensor([GENERATIONS[1]], dtype=torch.int64, device="cuda")
    by_value, _ = population_arena(a, 6)
    by_word, (buf, guard) = population_arena(a, 6)
    ES.es_perturb([a], by_value, sigma=SIGMA, seed=SEED, generation=GENERATIONS[1])
    ES.es_perturb([a], by_word, sigma=SIGMA, seed=SEED, generation=word)
    for n in ES.NAMES:
        assert torch.equal(bits(getattr(by_value.agents[0], n)), bits(getattr(by_word.agents[0], n)))
    assert sentinels_intact(buf, guard) and int(word) == GENERATIONS[1]
    grads = [torch.empty_like(getattr(a, n)) for n in ES.NAMES]
    grads2 = [torch.empty_like(g) for g in grads]
    fit = torch.randn(6, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    streams = [ES.es_stream(0, n) for n in ES.NAMES]
    ES.es_gradient(fit, grads, sigma=SIGMA, seed=SEED, generation=GENERATIONS[1], streams=streams)
    ES.es_gradient(fit, grads2, sigma=SIGMA, seed=SEED, generation=word, streams=streams)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(grads, grads2))


def test_stream_independence():
    ES = es()
    a, _ = base_actor(DIMS[0])
    P = 6
    base = [getattr(a, n) for n in ES.NAMES]
    streams = [ES.es_stream(0, n) for n in ES.NAMES]
    key = dict(sigma=SIGMA, seed=SEED, generation=3)

    def run(keep, **kw):
        out = [torch.empty((P,) + tuple(base[i].shape), device="cuda") for i in keep]
        ES.es_perturb_tensors([base[i] for i in keep], out, streams=[streams[i] for i in keep], **dict(key, **kw))
        return dict(zip(keep, out))

    every = run(range(6))
    dropped = run([0, 2, 3, 5])                         # fc1_b and mean_w are not in the launch
    reordered = run([5, 3, 0])                          # another place in the launch
    one_workgroup = run(range(6), max_workgroups=1)     # another grid
    for other in (dropped, reordered, one_workgroup):
        for i, t in other.items():
            assert torch.equal(bits(t), bits(every[i])), i
    later = run(range(6), generation=4)
    other_seed = run(range(6), seed=SEED + 1)
    for i in range(6):
        assert not torch.equal(later[i], every[i]) and not torch.equal(other_seed[i], every[i])
    # two tensors of one size under two streams differ; under one stream they would be equal
    same = [torch.empty(P, 16, device="cuda") for _ in range(2)]
    ES.es_perturb_tensors([base[1], base[3]], same, streams=[7, 8], **key)
    assert not torch.equal(same[0] - base[1], same[1] - base[3])


# ---------------------------------------------------------------- the utilities
def fitness_cases(P):
    rng = np.random.default_rng(P)
    f = rng.normal(0, 3, P).astype(np.float32)
    cases = {"random": f.copy()}
    t = f.copy()
    t[rng.integers(0, P, max(2, P // 3))] = np.float32(1.25)      # planted ties
    t[-1] = t[0]
    cases["ties"] = t
    s = t.copy()                                                   # NaNs, both infinities, a tie among each, -0 against +0
    for v, k in ((NAN, 0), (NAN, P // 2), (INF, 1), (-INF, P - 1), (-INF, P // 3), (0.0, P // 4), (-0.0, P // 5)):
        s[k] = v
    cases["special"] = s
    cases["equal"] = np.full(P, -2.5, dtype=np.float32)
    cases["all_nan"] = np.full(P, NAN, dtype=np.float32)
    return cases


def shaped(fit, shaping, P):
    """(w float64 [P / 2], stats float64 [4]) of one qr_es_gradient call, the workspace between sentinel words."""
    ES = es()
    sent = torch.full((P // 2 + 16,), SENTINEL, dtype=torch.int64, device="cuda")
    ws = sent[8:8 + P // 2].view(torch.float64)
    stats = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    g = torch.empty(5, device="cuda")
    out = ES.es_gradient(torch.from_numpy(fit).cuda(), [g], sigma=SIGMA, seed=SEED, generation=0, streams=[11], shaping=shaping, stats=stats, workspace=ws)
    assert out is stats and bool((sent[:8] == SENTINEL).all()) and bool((sent[8 + P // 2:] == SENTINEL).all())
    return ws.cpu().numpy().copy(), stats.cpu().numpy(), g


@pytest.mark.parametrize("P", [2, 6, 64, 66, 130, 8192])
def test_centered_rank_weights_equal_the_restatement(P):
    for name, f in fitness_cases(P).items():
        w, stats, g = shaped(f, "centered_rank", P)
        assert np.array_equal(w, R.pair_weights(f)), (name, P)
        assert np.array_equal(stats, R.fitness_stats(f), equal_nan=True), (name, stats)
        if name in ("equal", "all_nan"):
            assert (w == 0.0).all() and bool((g == 0.0).all())


@pytest.mark.parametrize("P", [2, 6, 66, 8192])
def test_standardize_weights(P):
    cases = fitness_cases(P)
    for name in ("random", "ties", "equal"):
        f = cases[name]
        w, stats, _ = shaped(f, "standardize", P)
        want = R.pair_weights(f, R.STANDARDIZE)
        # w_j = (f_2j - f_2j+1) / (std + 1e-8): the numerator is exact, the denominator a float64 sum of P terms in index order
        assert (np.abs(w - want) <= P * 2.0 ** -52 * np.abs(want)).all(), (name, P, np.abs(w - want).max())
        ref = R.fitness_stats(f)
        assert abs(stats[0] - ref[0]) <= P * 2.0 ** -52 * np.abs(f.astype(np.float64)).mean() and np.array_equal(stats[1:], ref[1:])
    for name in ("special", "all_nan"):
        w, stats, g = shaped(cases[name], "standardize", P)
        assert (w == 0.0).all() and stats[3] == 1.0 and bool((g == 0.0).all()), name
        assert np.array_equal(stats, R.fitness_stats(cases[name]), equal_nan=True)


# ---------------------------------------------------------------- the estimator
@pytest.mark.parametrize("dims,P", [(DIMS[2], 2), (DIMS[2], 6), (DIMS[2], 130), (DIMS[0], 130), (DIMS[1], 6)])
def test_estimator_against_the_host_sum(dims, P):
    """The bound per element, derived: the device's float64 sum of P / 2 rounded products (fused or not) is within
    (P / 2) 2^-53 sum_j |w_j eps_j[e]| of the exact sum, the division by P sigma keeps that relative size, and the one rounding to
    float32 adds 2^-24 |g|:   |got - g| <= 2^-24 |g| + (P / 2) 2^-53 sum_j |w_j eps_j[e]| / (P sigma)   (es_ref.gradient_bound).
    g is the long-double sum over the device's own draws (noise_fill's, equal by the contract) and the exact w."""
    ES = es()
    a, _ = base_actor(dims)
    sizes = [getattr(a, n).numel() for n in ES.NAMES]
    streams = [ES.es_stream(0, n) for n in ES.NAMES]
    rng = np.random.default_rng(P)
    fit = rng.normal(0, 2, P).astype(np.float32)
    for generation in GENERATIONS:
        buf, views, guard = arena(sizes, misaligned=(0, 2, 5))       # unaligned gradient tensors among them
        fit_t = torch.from_numpy(fit).cuda()
        ES.es_gradient(fit_t, views, sigma=SIGMA, seed=SEED, generation=generation, streams=streams)
        assert sentinels_intact(buf, guard)
        w = R.pair_weights(fit)
        e = draws(a, P, generation)
        worst = 0.0
        for n, v in zip(ES.NAMES, views):
            d = e[n].cpu().numpy()
            g = R.gradient(w, d, SIGMA, wide=True)
            err = np.abs(v.cpu().numpy().astype(np.longdouble) - g)
            bound = R.gradient_bound(w, d, SIGMA, g.astype(np.float64))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (n, generation, float(err.max()), float(bound.max()))
        print(f"estimator {dims} P {P} generation {generation}: worst error / bound {worst:.3f}")
        # the same bits from call to call and for another grid
        again = [torch.empty_like(v) for v in views]
        ES.es_gradient(fit_t, again, sigma=SIGMA, seed=SEED, generation=generation, streams=streams)
        one = [torch.empty_like(v) for v in views]
        ES.es_gradient(fit_t, one, sigma=SIGMA, seed=SEED, generation=generation, streams=streams, max_workgroups=1)
        for v, x, y in zip(views, again, one):
            assert torch.equal(bits(v), bits(x)) and torch.equal(bits(v), bits(y))
    # the dict form with the default streams is the flat form
    grads = [{n: torch.empty_like(getattr(a, n)) for n in ES.NAMES}]
    ES.es_gradient(fit_t, grads, sigma=SIGMA, seed=SEED, generation=GENERATIONS[1])
    assert all(torch.equal(bits(grads[0][n]).reshape(-1), bits(v)) for n, v in zip(ES.NAMES, views))
    # equal fitness everywhere: zero in every element
    ES.es_gradient(torch.full((P,), 3.5, device="cuda"), views, sigma=SIGMA, seed=SEED, generation=0, streams=streams)
    assert all(bool((v == 0.0).all()) for v in views)


# ---------------------------------------------------------------- errors
def test_error_codes_touch_nothing():
    from gym_rotor_amd import _lib as L
    ES = es()
    lib = L.load()
    a, _ = base_actor(DIMS[2])
    P = 6
    pop, (buf, guard) = population_arena(a, P)
    before = buf.clone()
    base = [getattr(a, n) for n in ES.NAMES]
    out = [getattr(pop.agents[0], n) for n in ES.NAMES]
    key = dict(n_policies=P, sigma=SIGMA, seed=SEED, generation=0, generation_dev=None, max_workgroups=0)
    stream = torch.cuda.current_stream().cuda_stream

    def perturb(change):
        p = L.es_perturb_args(base, out, [(a.log_std, pop.agents[0].log_std)], list(range(6)), **key)
        change(p)
        return lib.qr_es_perturb(C.byref(p), stream)

    assert perturb(lambda p: setattr(p.tensor[2], "out", None)) == -1
    assert perturb(lambda p: setattr(p, "n_policies", 5)) == -3
    assert perturb(lambda p: setattr(p.tensor[1], "stream", 0)) == -3
    assert perturb(lambda p: setattr(p.tensor[0], "out", p.tensor[0].out + 2)) == -4
    torch.cuda.synchronize()
    assert torch.equal(buf, before)

    gbuf, grads, gguard = arena([t.numel() for t in base])
    gbefore = gbuf.clone()
    fit = torch.zeros(P, device="cuda")
    stats = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.full((P // 2,), -7.0, dtype=torch.float64, device="cuda")

    def gradient(change):
        g = L.es_gradient_args(fit, grads, stats, ws, list(range(6)), shaping=0, **key)
        change(g)
        return lib.qr_es_gradient(C.byref(g), stream)

    assert gradient(lambda g: setattr(g, "fitness", None)) == -1
    assert gradient(lambda g: setattr(g, "workspace_bytes", 8 * (P // 2) - 1)) == -3
    assert gradient(lambda g: setattr(g, "shaping", 2)) == -3
    assert gradient(lambda g: setattr(g, "stats", g.stats + 4)) == -4
    torch.cuda.synchronize()
    assert torch.equal(gbuf, gbefore) and bool((stats == -7.0).all()) and bool((ws == -7.0).all())
    with pytest.raises(ValueError, match="QR_E_SIZE"):     # the Python layer reports a refusal of the library as a ValueError
        L.check(gradient(lambda g: setattr(g, "n_policies", 8194)), "qr_es_gradient")


# ---------------------------------------------------------------- a closed loop without the env
class Actor(torch.nn.Module):
    """The reference's MLP_Actor_PPO in its attributes (fc1, fc2, mean_linear, log_std)."""

    def __init__(self, d, h, a):
        super().__init__()
        self.fc1, self.fc2, self.mean_linear = torch.nn.Linear(d, h), torch.nn.Linear(h, h), torch.nn.Linear(h, a)
        self.log_std = torch.nn.Parameter(torch.zeros(1, a))


def weights(module):
    return [module.fc1.weight, module.fc1.bias, module.fc2.weight, module.fc2.bias, module.mean_linear.weight, module.mean_linear.bias]


def flat(modules):
    return torch.cat([p.detach().reshape(-1) for m in modules for p in weights(m)])


def test_closed_loop_approaches_the_target():
    """fitness_p = -|theta_p - theta*|^2 on the perturbed (3, 4, 1) population, es_gradient into .grad, DeviceAdamW(lr = 0.05) without
    clipping, schedule or weight decay, 20 generations of P = 64 at sigma = 0.1.  The float64 restatement with its own AdamW ends at
    0.182 of the initial distance (tests/test_es_host.py asserts < 0.25); the condition here, as there, is below one half."""
    from gym_rotor_amd import DeviceAdamW
    from gym_rotor_amd.policy import ActorParams
    ES = es()
    sizes, theta0, target, streams = R.loop_problem()
    P, sigma, generations = R.LOOP["P"], R.LOOP["sigma"], R.LOOP["generations"]
    module = Actor(3, 4, 1).cuda()
    at = 0
    for p, n in zip(weights(module), sizes):
        p.data.copy_(torch.from_numpy(theta0[at:at + n]).view(p.shape))
        p.grad = torch.zeros_like(p)
        at += n
    goal = torch.from_numpy(target).cuda()
    a = ActorParams.from_module(module)
    pop = ES.population_like([a], P)
    opt = DeviceAdamW(weights(module), lr=R.LOOP["lr"], weight_decay=0.0)
    grads = [{n: p.grad for n, p in zip(ES.NAMES, weights(module))}]
    d0 = float((flat([module]) - goal).norm())
    for generation in range(generations):
        ES.es_perturb([a], pop, sigma=sigma, seed=SEED, generation=generation, streams=streams)
        theta = torch.cat([getattr(pop.agents[0], n).reshape(P, -1) for n in ES.NAMES], 1)
        fit = -((theta - goal) ** 2).sum(1)
        ES.es_gradient(fit, grads, sigma=sigma, seed=SEED, generation=generation, streams=streams)
        opt.step()
    ratio = float((flat([module]) - goal).norm()) / d0
    print(f"closed loop: final / initial distance {ratio:.4f}")
    assert ratio < 0.5, ratio


# ---------------------------------------------------------------- end to end
def manual_generation(kind, modules, opts, src, src_obs, env, P, E, generation, sigma, max_steps):
    """One generation composed by hand from the public pieces, on its own env and modules."""
    from gym_rotor_amd import DeviceAdamW
    from gym_rotor_amd.evaluate import _tile_episodes
    from gym_rotor_amd.policy import ActorParams
    ES = es()
    base = [ActorParams.from_module(m) for m in modules]
    obs = _tile_episodes(src, src_obs, env, P)
    pop = ES.es_perturb(base, ES.population_like(base, P), sigma=sigma, seed=SEED, generation=generation)
    out = env.evaluate_population(pop, E, max_steps=max_steps, obs=obs)
    fit = ES.population_fitness(out, P, E, "benchmark")
    grads = []
    for m in modules:
        for p in weights(m):
            p.grad = torch.zeros_like(p)
        grads.append({n: p.grad for n, p in zip(ES.NAMES, weights(m))})
    stats = ES.es_gradient(fit, grads, sigma=sigma, seed=SEED, generation=generation)
    DeviceAdamW.step_all(opts)
    return stats, fit


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
def test_end_to_end_generations_equal_the_manual_composition(kind):
    from gym_rotor_amd import DeviceAdamW, EvolutionStrategy, QuadVecEnv
    from gym_rotor_amd.evaluate import _prepare_episodes
    from gym_rotor_amd.policy import ACTOR_DIMS, population_layout
    P, E, T, sigma = 8, 64, 50, 0.05
    torch.manual_seed(3)
    modules = [Actor(*d).cuda() for d in ACTOR_DIMS[kind]]
    mine = copy.deepcopy(modules)
    resumed = copy.deepcopy(modules)
    strategy = EvolutionStrategy(kind, modules, population=P, episodes_per_policy=E, sigma=sigma, seed=SEED, max_steps=T, optimizer=dict(lr=0.02))
    src, src_obs = _prepare_episodes(kind, E, 0, SEED, device="cuda")
    env = QuadVecEnv(kind, population_layout(P, E)[1], seed=SEED, goal_mode=0, autotune=False, device="cuda")
    opts = [DeviceAdamW(weights(m), lr=0.02, weight_decay=0.0) for m in mine]
    start = flat(modules).clone()
    after, saved = [], None
    for generation in range(3):
        stats = strategy.step()
        want_stats, want_fit = manual_generation(kind, mine, opts, src, src_obs, env, P, E, generation, sigma, T)
        assert strategy.generation == generation + 1
        assert torch.equal(bits(flat(modules)), bits(flat(mine))), generation
        assert torch.equal(strategy.fitness_values, want_fit) and torch.equal(stats, want_stats)
        assert float(stats[3]) == 0.0 and float(stats[1]) == float(want_fit.max()) and int(stats[2]) == int(want_fit.argmax())
        after.append(flat(modules).clone())
        if generation == 0:
            saved = (copy.deepcopy(strategy.state_dict()), [copy.deepcopy(m.state_dict()) for m in modules])
            best = strategy.best()
            assert torch.equal(best[0].fc1_w, strategy.population[int(stats[2])][0].fc1_w)
    assert not torch.equal(after[0], start) and not torch.equal(after[1], after[0]) and not torch.equal(after[2], after[1])
    # a state saved after generation 1, loaded into a fresh object, reproduces generations 2 and 3
    for m, s in zip(resumed, saved[1]):
        m.load_state_dict(s)
    fresh = EvolutionStrategy(kind, resumed, population=P, episodes_per_policy=E, sigma=sigma, seed=SEED, max_steps=T, optimizer=dict(lr=0.02))
    fresh.load_state_dict(saved[0])
    assert fresh.generation == 1
    for generation in (1, 2):
        fresh.step()
        assert torch.equal(bits(flat(resumed)), bits(after[generation])), generation
    # a .grad rebound behind the object's back is refused, not silently ignored
    resumed[0].fc1.weight.grad = torch.zeros_like(resumed[0].fc1.weight)
    with pytest.raises(RuntimeError, match="rebound"):
        fresh.step()
    assert fresh.generation == 3


def test_torch_ops_give_the_functional_forms_bits():
    ES = es()
    a, _ = base_actor(DIMS[1])
    P = 6
    pop, _ = population_arena(a, P)
    ES.es_perturb([a], pop, sigma=SIGMA, seed=SEED, generation=9)
    base = [getattr(a, n) for n in ES.NAMES]
    streams = [ES.es_stream(0, n) for n in ES.NAMES]
    out = [torch.empty((P,) + tuple(t.shape), device="cuda") for t in base]
    log_std = torch.empty(P, 4, device="cuda")
    torch.ops.gym_rotor_amd.qr_es_perturb(base, out, [a.log_std], [log_std], streams, SIGMA, SEED, 9, None, 0)
    assert all(torch.equal(bits(o), bits(getattr(pop.agents[0], n))) for n, o in zip(ES.NAMES, out)) and torch.equal(log_std, pop.agents[0].log_std)
    word = torch.tensor([9], dtype=torch.int64, device="cuda")
    out2 = [torch.empty_like(o) for o in out]
    torch.ops.gym_rotor_amd.qr_es_perturb(base, out2, [], [], streams, SIGMA, SEED, 0, word, 0)
    assert all(torch.equal(bits(o), bits(q)) for o, q in zip(out, out2))
    fit = torch.randn(P, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    for shaping, name in enumerate(ES.SHAPINGS):
        want = [torch.empty_like(t) for t in base]
        want_stats = ES.es_gradient(fit, want, sigma=SIGMA, seed=SEED, generation=9, streams=streams, shaping=name)
        got = [torch.empty_like(t) for t in base]
        stats = torch.empty(4, dtype=torch.float64, device="cuda")
        ws = torch.empty(ES.es_workspace_numel(P), dtype=torch.float64, device="cuda")
        torch.ops.gym_rotor_amd.qr_es_gradient(fit, got, stats, ws, streams, SIGMA, SEED, 9, None, shaping, 0)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(got, want)) and torch.equal(stats, want_stats)
