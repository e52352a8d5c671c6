"""Population evaluation on the GPU (qr_evaluate_population: eval_kernel with a policy per block of tiles): every policy's block
against a separate `evaluate` of that policy from the same starts, the tile geometry, nothing written outside the blocks, the
float64 oracle per block, evaluate_population end to end and the torch op."""
import numpy as np
import pytest
import torch

from test_gpu_evaluate_oracle import WARM_CALLS, _actors, _compare, _env, _fly_oracle, _np, _starts

pytestmark = pytest.mark.gpu

KINDS = ("coupled", "decoupled")
SOA = ("pos_vel", "att_rate", "integ", "params", "goal", "traj")   # [fields, N] buffers of the env
RESULTS = ("episode_return", "benchmark", "length", "terminated", "success", "final_error", "obs0", "obs1", "action")
GUARD = 64


def _bits(t):
    """A tensor as integers of its own width: equality that also holds for the NaN sentinels."""
    return t.contiguous().view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _three_policies(kind, seed=3):
    """Three deliberately different actors (test_gpu_evaluate_oracle._actors: small mean weights and the hover-thrust bias; here with
    the mean weights scaled by 0.1, 1 and 3 and different draws): they crash different envs at different steps."""
    return [_actors(kind, seed + k, weight=w) for k, w in enumerate((0.1, 1.0, 3.0))]


class _Flight:
    """P policies x E episodes in ONE launch from starts common to all policies, and what that needs around it.

    The E starts are made on an E-env env (`src`, test_gpu_evaluate_oracle._starts: a doomed third, a resting third, the rest as
    the reset drew them) and tiled into the blocks of an env of P * Epad envs.  Every padding env and every padding row — of the
    observation rows that go in and of each output — holds a sentinel (NaN where the type has one), the outputs lie inside guard
    tensors, and `check_untouched` compares all of it with what it was, bit for bit."""

    def __init__(self, kind, P, E, T, layout="mixed", substeps=1, goal_mode=None, seed=5, **kw):
        from gym_rotor_amd.policy import population_env_index, population_layout, population_tile
        self.kind, self.P, self.E, self.T = kind, P, E, T
        self.epad, self.n = population_layout(P, E)
        cfg = dict(seed=seed, layout=layout, substeps=substeps, goal_mode=goal_mode, **kw)
        self.src = _env(kind, E, **cfg)
        self.warm = WARM_CALLS.get(goal_mode, 0)
        self.obs, self.state, self.params, self.draws = _starts(self.src, warm=self.warm)
        self.sd = self.src.state_dict()
        self.env = env = _env(kind, self.n, **cfg)
        self.idx = population_env_index(P, E, "cuda")
        self.pad = torch.ones(self.n, dtype=torch.bool, device="cuda")
        self.pad[self.idx.reshape(-1)] = False
        assert int(self.pad.sum()) == P * (self.epad - E)
        for k in SOA:
            if k == "goal" and self.sd[k] is not None:   # (the goal buffer of a stateless mode: made by get_desired(store_goal=True))
                env._ensure_goal()
            buf = getattr(env, "_" + k)
            if buf is not None:
                buf[:, self.pad] = float("nan")
                population_tile(self.sd[k], P, E, buf, env_dim=1)
        env._steps[self.pad] = -12345
        population_tile(self.sd["steps"], P, E, env._steps)
        population_tile(self.sd["episode"], P, E, env._episode)
        self.obs_in = [population_tile(o, P, E, torch.full((self.n, o.shape[1]), float("nan"), device="cuda")) for o in self.obs]
        self.before = {k: getattr(env, "_" + k).clone() for k in SOA + ("steps",) if getattr(env, "_" + k) is not None}
        self.steps0 = env.episode_steps.clone()

    def launch(self, population, op=False):
        from gym_rotor_amd import torch_ops
        env, n = self.env, self.n
        G = env.n_agents
        shapes = {"episode_return": ((G,), torch.float64), "benchmark": ((), torch.float64), "length": ((), torch.int32),
                  "terminated": ((), torch.bool), "success": ((G,), torch.bool), "final_error": ((4,), torch.float32),
                  "obs0": ((env.obs_dims[0],), torch.float32), "action": ((env.action_dim,), torch.float32)}
        if len(env.obs_dims) > 1:
            shapes["obs1"] = ((env.obs_dims[1],), torch.float32)
        self.guard = {k: torch.full((n + 2 * GUARD,) + s, True if dt == torch.bool else 77, dtype=dt, device="cuda") for k, (s, dt) in shapes.items()}
        out = {k: g[GUARD:GUARD + n] for k, g in self.guard.items()}
        if op:
            torch_ops.evaluate_population(env, population, self.E, self.T, [o.clone() for o in self.obs_in], out)
            got = out
        else:
            got = env.evaluate_population(population, self.E, max_steps=self.T, obs=[o.clone() for o in self.obs_in], out=out)
            assert got["obs0"] is out["obs0"]
            last = env._last_obs[0] if isinstance(env._last_obs, tuple) else env._last_obs
            assert last is got["obs0"] and env._policy_steps == 0   # (as evaluate: the rows are current, the noise stream stays)
        torch.cuda.synchronize()
        self.got = got
        return got

    def check_untouched(self):
        """Guard rows before and behind every output, every padding row of every output, and the padding envs' state, integrators,
        parameters, goal, generator state and step counter: all as they were."""
        keep = torch.ones(self.n + 2 * GUARD, dtype=torch.bool, device="cuda")
        keep[GUARD + self.idx.reshape(-1)] = False
        for k, g in self.guard.items():
            fill = True if g.dtype == torch.bool else 77
            assert bool((g[keep] == fill).all()), (k, "a guard or padding row was written")
            assert int(keep.sum()) == 2 * GUARD + int(self.pad.sum())
        for k, was in self.before.items():
            now = getattr(self.env, "_" + k)
            sel = (slice(None), self.pad) if now.dim() == 2 else (self.pad,)
            assert torch.equal(_bits(now[sel]), _bits(was[sel])), (k, "a padding env was written")

    def block(self, p, t, env_dim=0):
        """Policy p's E live entries of a per-env tensor."""
        return t.narrow(env_dim, p * self.epad, self.E)

    def compare_with_separate_evaluates(self, population, exact=True):
        """Policy p's block against evaluate(population[p]) on the E-env env from the same starts: the same kernel on the same
        inputs, so every result and everything written back is compared bit for bit, in every layout."""
        src, got = self.src, self.got
        singles = []
        for p in range(self.P):
            src.load_state_dict(self.sd)
            want = src.evaluate(population[p], max_steps=self.T, obs=[o.clone() for o in self.obs])
            torch.cuda.synchronize()
            singles.append(want)
            for k in ("length", "terminated", "success"):
                assert torch.equal(self.block(p, got[k]), want[k]), (p, k)
            for k in ("episode_return", "benchmark", "final_error", "obs0", "obs1", "action"):
                if k in want:
                    assert torch.equal(self.block(p, got[k]), want[k]), (p, k)
            assert torch.equal(self.block(p, self.env.get_current_state()), src.get_current_state()), p
            for k in SOA + ("steps",):
                a, b = getattr(self.env, "_" + k), getattr(src, "_" + k)
                if a is not None:
                    assert torch.equal(_bits(self.block(p, a, a.dim() - 1)), _bits(b)), (p, k)
            assert torch.equal(self.block(p, self.env.episode_steps - self.steps0), want["length"]), p
        return singles


def _assert_policies_matter(fl, singles, fates=True):
    """Guards: a launch that flew policy 0 everywhere cannot have passed — the policies' results differ pairwise — and both early
    crashes and survivors of all T steps occur."""
    for p in range(fl.P):
        for q in range(p + 1, fl.P):
            assert not torch.equal(singles[p]["episode_return"], singles[q]["episode_return"]), (p, q)
            assert not torch.equal(singles[p]["action"], singles[q]["action"]), (p, q)
    if fates:
        term = torch.stack([s["terminated"] for s in singles])
        length = torch.stack([s["length"] for s in singles])
        assert bool(term.any()) and bool((~term).any()) and bool((length[term] < fl.T).any()) and bool((length[~term] == fl.T).all())


# ---------------------------------------------------------------------------------------------------------------------
# 1. each policy gets its own weights and its own rows
# ---------------------------------------------------------------------------------------------------------------------
CASES = [(k, g, "mixed", s) for k in KINDS for g in (None, 1, 5) for s in (1, 4)]
CASES += [("coupled", 1, "f64", 1), ("decoupled", 5, "f64", 4), ("coupled", 5, "f32", 4), ("decoupled", None, "f32", 1)]


@pytest.mark.parametrize("kind,goal_mode,layout,substeps", CASES)
def test_each_policy_flies_its_own_block(kind, goal_mode, layout, substeps):
    """P = 3 x E = 70 (Epad = 128: two tiles per policy, the second with 6 live rows) from common starts, against three separate
    evaluate calls on a 70-env env: length, terminated, success, returns, benchmark, final_error, final rows, last action, and the
    written-back state, integrators, generator state, goal and step counters, all bit for bit (one kernel, the same inputs) — in
    the default, float64 and float32 layouts alike.  Padding envs and rows, and guard rows around the outputs: untouched."""
    from gym_rotor_amd import ActorPopulation
    fl = _Flight(kind, 3, 70, 200, layout=layout, substeps=substeps, goal_mode=goal_mode)
    pop = ActorPopulation.stack(_three_policies(kind))
    fl.launch(pop)
    singles = fl.compare_with_separate_evaluates(pop)
    fl.check_untouched()
    _assert_policies_matter(fl, singles)


# ---------------------------------------------------------------------------------------------------------------------
# 2. tile geometry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P,E,T", [(5, 64, 60), (5, 128, 60), (130, 1, 60), (1, 70, 60), (1, 64, 60), (3, 65, 1), (4, 63, 60)])
def test_tile_geometry(kind, P, E, T):
    """Blocks without padding (E = 64, 128), 130 one-row tiles (policy indices beyond one wave's worth of lanes), a ragged tile per
    policy (63, 65), one policy (= evaluate on the same E envs) and max_steps = 1: every block against evaluate of its policy."""
    from gym_rotor_amd import ActorPopulation
    fl = _Flight(kind, P, E, T, goal_mode=1, seed=21)
    base = _actors(kind, 8, weight=1.0)
    if P <= 5:
        pop = ActorPopulation.stack([_actors(kind, 8 + p, weight=(0.1, 1.0, 3.0, 0.5, 2.0)[p]) for p in range(P)])
    else:   # the evolution-strategy constructor, on the GPU: 65 antithetic pairs around one actor
        pop, eps = ActorPopulation.perturb(base, P, 0.3, generator=torch.Generator("cuda").manual_seed(1))
        assert torch.equal(pop.agents[0].fc1_w, base[0].fc1_w[None] + 0.3 * eps[0]["fc1_w"])
    fl.launch(pop)
    singles = fl.compare_with_separate_evaluates(pop)
    fl.check_untouched()
    if T == 1:
        assert all(bool((s["length"] == 1).all()) for s in singles)
    if P > 1:
        acts = torch.stack([s["action"] for s in singles])
        assert len({tuple(a.flatten().tolist()) for a in acts}) == P, "every policy flew its own weights"
    if P > 1 and E >= 63 and T > 1:
        _assert_policies_matter(fl, singles, fates=True)


# ---------------------------------------------------------------------------------------------------------------------
# 3. nothing outside the blocks is written
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("goal_mode", [None, 6, 3])
def test_nothing_outside_the_blocks_is_written(kind, goal_mode):
    """P = 4 x E = 70, outputs inside guard tensors, padding rows and padding envs pre-filled with sentinels (NaN in every float
    buffer — also in the observation rows that go IN, which must not reach a live lane): afterwards all of it is unchanged, every
    live row has been written, and no live result is a NaN.  Goal mode 3 (stateful): the launch also writes the goal buffer and
    all eight generator fields at each lane's freeze."""
    from gym_rotor_amd import ActorPopulation
    fl = _Flight(kind, 4, 70, 80, goal_mode=goal_mode, seed=7)
    pop = ActorPopulation.stack([_actors(kind, 20 + p, weight=w) for p, w in enumerate((0.1, 1.0, 3.0, 0.3))])
    got = fl.launch(pop)
    fl.check_untouched()
    live = fl.idx.reshape(-1)
    for k, v in got.items():
        rows = v[live]
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(rows).all()), k
        if k == "length":
            assert bool(((rows >= 1) & (rows <= 80)).all())   # (77, the fill, is a possible length: the range is the check)
        elif k in ("obs0", "final_error", "action", "episode_return", "benchmark"):
            assert bool((rows.reshape(len(live), -1) != 77).any(1).all()), (k, "a live row was not written")
    for k in ("pos_vel", "att_rate", "integ"):
        assert bool(torch.isfinite(getattr(fl.env, "_" + k)[:, live]).all()), k
    assert bool((fl.env.episode_steps[live] - fl.steps0[live] == got["length"][live]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. independent anchor: the float64 oracle per block
# ---------------------------------------------------------------------------------------------------------------------
class _Block:
    """Policy p's block of the population env with the attributes test_gpu_evaluate_oracle._compare reads of an env."""

    def __init__(self, fl, p):
        env = fl.env
        self.kind, self.num_envs, self.goal_mode = env.kind, fl.E, env.goal_mode
        self._state = fl.block(p, env.get_current_state())
        self.integ = fl.block(p, env.integ)
        self.episode_steps = fl.block(p, env.episode_steps)
        self._traj = None if env._traj is None else fl.block(p, env._traj, 1)
        self._goal = None if env._goal is None else fl.block(p, env._goal, 1)

    def get_current_state(self):
        return self._state


@pytest.mark.parametrize("kind,goal_mode,substeps", [("coupled", 5, 1), ("decoupled", 6, 4)])
def test_population_against_the_float64_oracle(kind, goal_mode, substeps):
    """One configuration per wrapper with a fused goal generator (the circle: stateful, its run-up ending inside the flight; the
    eight-shaped curve with Magnus substeps): test_evaluate_host.eval_oracle flown per policy from the common starts, each policy's
    block compared by test_gpu_evaluate_oracle._compare — its bars (OBS_BAR, STATE_BAR, RETURN_BAR, BENCH_BAR, ACTION_BAR, GOAL_BAR)
    and its handling of decision ties (_ties: within the row bar of a threshold, at most TIE_CAP), nothing restated here and no env
    left out beyond what that helper excludes for evaluate on the same inputs."""
    from gym_rotor_amd import ActorPopulation
    T = 200
    fl = _Flight(kind, 3, 70, T, substeps=substeps, goal_mode=goal_mode, seed=5)
    # (three draws of the actors those bars were set with — mean weights x 0.1, 200 steps: an unstabilised loop with larger
    #  weights amplifies the float32 action's rounding beyond the state bar, as that file notes for longer flights)
    policies = [_actors(kind, s) for s in (3, 4, 6)]
    theta0 = _np(fl.env._traj[1]).copy()
    fl.launch(ActorPopulation.stack(policies))
    fl.check_untouched()
    wants = []
    for p, actors in enumerate(policies):
        want = _fly_oracle(kind, fl.state, fl.params, T, actors, goal_mode=goal_mode, draws=fl.draws, n_sub=substeps, warm_calls=fl.warm)
        got = {k: fl.block(p, v) for k, v in fl.got.items()}
        _compare(f"{kind} goal {goal_mode} x{substeps}, policy {p}", _Block(fl, p), got, want, "mixed", fl.block(p, fl.steps0),
                 calls0=1 + fl.warm, theta0=theta0[p * fl.epad:p * fl.epad + fl.E])
        wants.append(want)
    term = np.stack([w["terminated"] for w in wants])
    assert term.any() and (~term).any(), "the oracle alone shows both fates"
    for p in range(3):
        for q in range(p + 1, 3):
            assert not np.array_equal(wants[p]["episode_return"], wants[q]["episode_return"]), "the oracle's policies differ"


# ---------------------------------------------------------------------------------------------------------------------
# 5. end to end and the torch op
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = ("episode_return", "benchmark", "length", "terminated", "success", "final_error")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", [None, 1])
def test_evaluate_population_end_to_end(kind, mode):
    """evaluate_population(common_episodes=True): policy p's [E, ...] results are evaluate_policy(kind, population[p], E)'s, bit for
    bit per episode; per_policy() and best() agree with them.  The same policy twice: common episodes give two identical blocks,
    common_episodes=False two different ones (every episode has its own draws)."""
    from gym_rotor_amd import ActorPopulation, evaluate_policy, evaluate_population
    E, sec = 70, 1.0
    policies = _three_policies(kind, seed=11)
    pop = ActorPopulation.stack(policies)
    res = evaluate_population(kind, pop, E, traj_mode=mode, eval_seconds=sec)
    assert len(res) == 3 and tuple(res.length.shape) == (3, E) and tuple(res.episode_return.shape)[:2] == (3, E)
    bench = []
    for p in range(3):
        one = evaluate_policy(kind, pop[p], E, traj_mode=mode, eval_seconds=sec)
        for k in FIELDS:
            assert torch.equal(getattr(res, k)[p], getattr(one, k)), (p, k)
            assert torch.equal(getattr(res[p], k), getattr(one, k)), (p, k)
        assert res[p].summary() == one.summary()
        bench.append(float(one.benchmark.double().mean()))
    assert res.per_policy()["benchmark"].tolist() == pytest.approx(bench, rel=1e-13)
    assert res.best() == int(np.argmax(bench)) and len(set(bench)) == 3
    twice = ActorPopulation.stack([policies[1], policies[1]])
    same = evaluate_population(kind, twice, E, traj_mode=mode, eval_seconds=sec)
    own = evaluate_population(kind, twice, E, traj_mode=mode, eval_seconds=sec, common_episodes=False)
    for k in FIELDS:
        assert torch.equal(getattr(same, k)[0], getattr(same, k)[1]), k
    assert not torch.equal(own.episode_return[0], own.episode_return[1]) and not torch.equal(own.final_error[0], own.final_error[1])
    assert torch.equal(own.length >= 1, torch.ones_like(own.terminated)) and bool(torch.isfinite(own.episode_return).all())


@pytest.mark.parametrize("kind", KINDS)
def test_torch_op_matches_evaluate_population(kind):
    """torch.ops.gym_rotor_amd.qr_evaluate_population (torch_ops.evaluate_population) gives the bits of the method, the env's state,
    integrators, generator state and step counters afterwards included, and writes nothing else either."""
    from gym_rotor_amd import ActorPopulation
    pop = ActorPopulation.stack(_three_policies(kind, seed=30))
    a = _Flight(kind, 3, 70, 150, goal_mode=1, seed=13)
    want = a.launch(pop)
    b = _Flight(kind, 3, 70, 150, goal_mode=1, seed=13)
    got = b.launch(pop, op=True)
    b.check_untouched()
    live = a.idx.reshape(-1)
    for k in want:
        assert torch.equal(got[k][live], want[k][live]), k
    assert torch.equal(b.env.get_current_state()[live], a.env.get_current_state()[live])
    for k in SOA + ("steps",):
        x, y = getattr(a.env, "_" + k), getattr(b.env, "_" + k)
        if x is not None:
            assert torch.equal(_bits(x), _bits(y)), k
    term = want["terminated"][live]
    assert bool(term.any()) and bool((~term).any())
