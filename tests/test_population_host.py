"""Population evaluation (qr_evaluate_population / QuadVecEnv.evaluate_population / gym_rotor_amd.evaluate_population) without a GPU:
the C-ABI struct mirror and argument checks, ActorPopulation (stack, perturb), the block layout's index maps and PopulationResult."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from test_evaluate_host import _bare_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_qr_population_mirrors_the_header(tmp_path):
    """QrPopulation in gym_rotor_amd/_lib.py against include/quadrotor_hip.h, compiled: sizes and offsets; the ABI version stays."""
    from gym_rotor_amd import _lib as L
    fl = [f[0] for f in L.QrPopulation._fields_]
    lines = ['printf("QrPopulation %zu\\n", sizeof(QrPopulation));'] + [f'printf("{f} %zu\\n", offsetof(QrPopulation, {f}));' for f in fl]
    lines.append('printf("abi %d\\n", QR_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert fl == ["n_policies", "envs_per_policy"]
    assert int(out["QrPopulation"]) == C.sizeof(L.QrPopulation) == 8
    for f in fl:
        assert int(out[f]) == getattr(L.QrPopulation, f).offset, f
    assert "qr_evaluate_population" in L.SYMBOLS and hasattr(L.load(), "qr_evaluate_population")
    assert int(out["abi"]) == L.ABI_VERSION == 16


def _fake_call():
    """A qr_evaluate_population call that passes every check of qr_evaluate_actor, on fake device addresses (never touched: every
    case below returns before a launch)."""
    from gym_rotor_amd import _lib as L
    e, o, pol = L.QrEnv(), L.QrEvalOut(), L.QrPolicyRollout()
    L.load().qr_default_coeffs(C.byref(e.coeffs))
    e.kind, e.num_envs, e.pos_vel, e.att_rate, e.integ = 1, 3 * 128, 0x1000, 0x2000, 0x3000
    w = [0x10000 + 0x100 * k for k in range(7)]
    arr = (L.QrActor * 1)(L.QrActor(*w, None, None, 23, 16, 4, 0))
    pol.actors, pol.obs0_in, pol.max_action = arr, 0x5000, 1.0
    o.episode_return, o.benchmark, o.length, o.terminated, o.success, o.obs0 = 0x6000, 0x7000, 0x8000, 0x9000, 0xA000, 0xB000
    return e, pol, o, arr


def test_qr_evaluate_population_argument_errors_without_gpu():
    """The population's own checks (NULL pop: QR_E_NULL; P < 1, E < 1, num_envs != P * roundup(E, 64): QR_E_SIZE) and
    qr_evaluate_actor's, which it shares, all on the host before a launch."""
    from gym_rotor_amd import _lib as L
    lib = L.load()
    e, pol, o, arr = _fake_call()
    call = lambda pop, T=10, sub=1: lib.qr_evaluate_population(C.byref(e), C.byref(pol), None if pop is None else C.byref(pop), T, sub,
                                                               C.byref(o), None)
    assert call(None) == -1
    for P, E in ((0, 70), (-1, 70), (3, 0), (3, -5)):
        assert call(L.QrPopulation(P, E)) == -3, (P, E)
    for P, E in ((3, 129), (3, 64), (2, 70), (4, 70), (384, 2), (1, 300)):   # 3 x 128 envs: a wrong P, a wrong Epad, E not padded
        assert call(L.QrPopulation(P, E)) == -3, (P, E)
    good = L.QrPopulation(3, 70)   # 3 x roundup(70, 64) = 384
    # qr_evaluate_actor's checks behind it
    assert call(good, T=0) == -3 and call(good, sub=0) == -3
    arr[0].hidden_dim = 32
    assert call(good) == -3
    arr[0].hidden_dim = 16
    o.success = None
    assert call(good) == -1
    o.success = 0xA000
    e.kind = 0
    assert call(good) == -2                                   # Quad-v0 has no actor
    e.kind = 2
    assert call(good) == -1                                   # MODUL needs obs1 rows in and out
    e.kind, e.num_envs = 1, 0
    assert call(good) == -3                                   # an empty batch holds no population
    assert lib.qr_evaluate_actor(C.byref(e), C.byref(pol), 10, 1, C.byref(o), None) == 0   # (and stays a no-op for evaluate)


def test_evaluate_population_argument_errors_raise_before_any_launch():
    """QuadVecEnv.evaluate_population checks kind, population type, env size against the block layout and the stacked sizes in
    Python (the shell has no device buffers at all)."""
    from gym_rotor_amd import ActorPopulation, random_actors
    from gym_rotor_amd.policy import ActorParams
    pop = ActorPopulation.stack([random_actors("coupled", CPU) for _ in range(3)])
    with pytest.raises(ValueError, match="coupled"):
        _bare_env("quad").evaluate_population(pop, 70)
    with pytest.raises(TypeError, match="ActorPopulation"):
        _bare_env("coupled", n=384).evaluate_population(random_actors("coupled", CPU), 70)
    with pytest.raises(ValueError, match="3 x 128 = 384"):
        _bare_env("coupled", n=300).evaluate_population(pop, 70)
    with pytest.raises(ValueError, match="envs_per_policy >= 1"):
        _bare_env("coupled", n=384).evaluate_population(pop, 0)
    with pytest.raises(ValueError, match="2 actor"):
        _bare_env("decoupled", n=384).evaluate_population(pop, 70)
    with pytest.raises(ValueError, match="actor sizes"):
        _bare_env("coupled", n=384).evaluate_population(ActorPopulation.stack([[ActorParams.random(23, 32, 4, CPU)]] * 3), 70)
    with pytest.raises(ValueError, match="max_steps"):
        _bare_env("coupled", n=384).evaluate_population(pop, 70, max_steps=0)
    with pytest.raises(ValueError, match="no current observation"):
        _bare_env("coupled", n=384).evaluate_population(pop, 70)


# ---------------------------------------------------------------------------------------------------------------------
# ActorPopulation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,algo", [("coupled", "ppo"), ("decoupled", "ppo"), ("decoupled", "sac")])
def test_stack_round_trips(kind, algo):
    from gym_rotor_amd import ActorPopulation, random_actors
    from gym_rotor_amd.policy import ACTOR_DIMS, ActorParams
    g = torch.Generator().manual_seed(4)
    members = [random_actors(kind, CPU, generator=g, algo=algo) for _ in range(5)]
    pop = ActorPopulation.stack(members)
    assert len(pop) == 5 and len(pop.agents) == len(ACTOR_DIMS[kind]) and len(list(pop)) == 5
    pop.check(kind, CPU)
    for p, m in enumerate(members):
        for a, b, d in zip(pop[p], m, ACTOR_DIMS[kind]):
            a.check(d, CPU)                      # ordinary actors: what evaluate / rollout_actor accept
            assert a.squash == b.squash and a.dims == d
            for n in ActorParams.NAMES:
                ta, tb = getattr(a, n), getattr(b, n)
                assert (ta is None) == (tb is None)
                if ta is not None:
                    assert torch.equal(ta, tb) and ta.is_contiguous(), n
    # the stacked-tensor rule: contiguous [P, ...], policy p's tensor p * numel elements behind policy 0's; pop[p] is a view
    for a, a0, a3 in zip(pop.agents, pop[0], pop[3]):
        for n in ActorParams.NAMES:
            t = getattr(a, n)
            if t is not None:
                assert t.is_contiguous() and t.shape[0] == 5
                assert getattr(a3, n).data_ptr() - getattr(a0, n).data_ptr() == 3 * getattr(a0, n).numel() * 4
    pop.agents[0].fc1_b[2].fill_(9.0)
    assert bool((pop[2][0].fc1_b == 9.0).all()) and not bool((members[2][0].fc1_b == 9.0).any())   # a view of the stack, a copy of the input
    assert pop[-1][0].fc1_w.data_ptr() == pop[4][0].fc1_w.data_ptr()
    with pytest.raises(IndexError):
        pop[5]
    sub = pop.select(slice(1, 4))
    assert len(sub) == 3 and torch.equal(sub[0][0].fc2_w, pop[1][0].fc2_w)
    sub.check(kind, CPU)


def test_stack_rejects_mixed_sizes_and_forms():
    from gym_rotor_amd import ActorPopulation, random_actors
    from gym_rotor_amd.policy import ActorParams
    a, b = random_actors("coupled", CPU), random_actors("coupled", CPU)
    with pytest.raises(ValueError, match="at least one"):
        ActorPopulation.stack([])
    with pytest.raises(ValueError, match="size"):
        ActorPopulation.stack([a, [ActorParams.random(23, 32, 4, CPU)]])
    with pytest.raises(ValueError, match="size"):
        ActorPopulation.stack([a, [ActorParams.random(15, 16, 4, CPU)]])
    with pytest.raises(ValueError, match="actors cannot be stacked"):
        ActorPopulation.stack([a, random_actors("decoupled", CPU)])
    with pytest.raises(ValueError, match="one form"):
        ActorPopulation.stack([a, random_actors("coupled", CPU, algo="sac")])
    b[0].squash = 1
    with pytest.raises(ValueError, match="one form"):
        ActorPopulation.stack([a, b])
    b[0].squash = 0
    b[0].fc1_w = b[0].fc1_w.double()
    with pytest.raises(ValueError, match="dtype"):
        ActorPopulation.stack([a, b])


def test_perturb_is_antithetic():
    """Pairs are adjacent: policy 2k = theta + sigma eps_k, 2k + 1 = theta - sigma eps_k, eps returned per policy.  On dyadic
    inputs, where no float32 operation rounds, the pair mean IS the base and the difference IS 2 sigma eps.  On normal draws each
    member is rounded to float32 once (relative error 2^-24), which is all that separates the pair mean from the base."""
    from gym_rotor_amd import ActorPopulation, random_actors
    from gym_rotor_amd.policy import ACTOR_DIMS, ActorParams
    W = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b")
    kind, n, sigma = "decoupled", 6, 0.25
    rng = np.random.default_rng(0)
    base = random_actors(kind, CPU)
    for a in base:   # multiples of 1/64 below 4; sigma eps multiples of 1/32 below 1: sums and differences are exact in float32
        for name in W:
            t = getattr(a, name)
            t.copy_(torch.from_numpy(rng.integers(-256, 257, tuple(t.shape)) / 64.0))
    eps = [{name: torch.from_numpy(rng.integers(-32, 33, (n,) + tuple(getattr(a, name).shape)) / 8.0).float() for name in W} for a in base]
    pop, got = ActorPopulation.perturb(base, n, sigma, eps=eps)
    assert len(pop) == n
    pop.check(kind, CPU)
    for a, b, e, e_in in zip(pop.agents, base, got, eps):
        assert a.squash == b.squash and torch.equal(a.log_std, b.log_std[None].expand(n, -1))   # the log_std source: copied
        for name in W:
            t, th = getattr(a, name), getattr(b, name)
            assert torch.equal(e[name][0::2], e_in[name][0::2]) and torch.equal(e[name][1::2], -e_in[name][0::2])
            assert torch.equal((t[0::2] + t[1::2]) / 2, th[None].expand(n // 2, *th.shape)), name
            assert torch.equal(t[0::2] - t[1::2], 2 * sigma * e[name][0::2]), name
            assert torch.equal(t, th[None] + sigma * e[name]), name
    # normal draws from a generator: reproducible, pairs adjacent, rounding-level symmetric
    base = random_actors(kind, CPU, generator=torch.Generator().manual_seed(1))
    pop, eps = ActorPopulation.perturb(base, n, 0.05, generator=torch.Generator().manual_seed(2))
    pop2, eps2 = ActorPopulation.perturb(base, n, 0.05, generator=torch.Generator().manual_seed(2))
    u = 2.0 ** -24
    for a, a2, b, e, e2 in zip(pop.agents, pop2.agents, base, eps, eps2):
        for name in W:
            t, th, ee = getattr(a, name).double(), getattr(b, name).double(), e[name].double()
            assert torch.equal(getattr(a, name), getattr(a2, name)) and torch.equal(e[name], e2[name])
            assert torch.equal(e[name][1::2], -e[name][0::2]) and float(ee.std()) > 0.5
            big = torch.maximum(t[0::2].abs(), t[1::2].abs())
            assert bool((((t[0::2] + t[1::2]) / 2 - th[None]).abs() <= u * big).all()), name
            # difference: two member roundings, and sigma eps taken twice with sigma rounded to float32 and the product rounded
            assert bool(((t[0::2] - t[1::2] - 2 * 0.05 * ee[0::2]).abs() <= 2 * u * big + 4 * u * (0.05 * ee[0::2]).abs()).all()), name
    # not antithetic: n independent draws; an odd n only then
    pop, eps = ActorPopulation.perturb(base, 5, 0.05, generator=torch.Generator().manual_seed(3), antithetic=False)
    assert len(pop) == 5 and not torch.equal(eps[0]["fc1_w"][1], -eps[0]["fc1_w"][0])
    assert torch.equal(pop.agents[0].fc1_w, base[0].fc1_w[None] + 0.05 * eps[0]["fc1_w"])
    with pytest.raises(ValueError, match="even"):
        ActorPopulation.perturb(base, 5, 0.05)
    assert all(a.dims == d for a, d in zip(pop[4], ACTOR_DIMS[kind])) and ActorParams.NAMES[0] == "fc1_w"


# ---------------------------------------------------------------------------------------------------------------------
# the block layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 63, 64, 65, 70, 128])
@pytest.mark.parametrize("P", [1, 3])
def test_block_layout(P, E):
    """Epad, the env <-> (policy, episode) maps and the tiling of an E-env state into the blocks, against the issue's formulas
    restated per tile: tile b belongs to policy b // tpp and has min(E - (b % tpp) * 64, 64) live rows."""
    from gym_rotor_amd.policy import population_env_index, population_layout, population_tile, population_view
    epad, n = population_layout(P, E)
    assert epad % 64 == 0 and 0 <= epad - E < 64 and n == P * epad
    tpp = epad // 64
    live = np.zeros(n, bool)
    owner = np.full(n, -1)
    for b in range(n // 64):
        p, rows = b // tpp, min(E - (b % tpp) * 64, 64)
        assert 1 <= rows <= 64
        live[b * 64:b * 64 + rows] = True
        owner[b * 64:b * 64 + 64] = p
    idx = population_env_index(P, E).numpy()
    assert idx.shape == (P, E) and np.array_equal(np.sort(idx.ravel()), np.flatnonzero(live))
    for p in range(P):
        assert np.array_equal(idx[p], p * epad + np.arange(E)) and (owner[idx[p]] == p).all()
    assert live.sum() == P * E
    # views: [N, D] rows and [F, N] SoA buffers; no copy, padding sliced off
    rows = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    v = population_view(rows, P, E)
    assert v.shape == (P, E, 3) and torch.equal(v, rows[torch.from_numpy(idx)]) and v.data_ptr() == rows.data_ptr()
    soa = torch.arange(6 * n, dtype=torch.float64).reshape(6, n)
    assert torch.equal(population_view(soa, P, E, 1), soa[:, torch.from_numpy(idx)])
    assert torch.equal(population_view(soa, P, E, -1), population_view(soa, P, E, 1))
    # tiling an E-env state into every block; padding untouched
    block = torch.randn(6, E, dtype=torch.float64)
    big = torch.full((6, n), -7.0, dtype=torch.float64)
    population_tile(block, P, E, big, env_dim=1)
    for p in range(P):
        assert torch.equal(big[:, p * epad:p * epad + E], block)
    assert bool((big[:, torch.from_numpy(~live)] == -7.0).all())
    r_block = torch.randn(E, 15)
    r_big = population_tile(r_block, P, E, torch.full((n, 15), -7.0))
    assert torch.equal(r_big[torch.from_numpy(idx)], r_block[None].expand(P, E, 15)) and bool((r_big[torch.from_numpy(~live)] == -7.0).all())
    with pytest.raises(ValueError):
        population_view(rows[:-1], P, E)
    with pytest.raises(ValueError):
        population_tile(r_block[:-1] if E > 1 else torch.randn(2, 15), P, E, r_big)


def test_block_layout_rejects_empty_populations():
    from gym_rotor_amd.policy import population_layout
    for P, E in ((0, 5), (2, 0), (-1, 64)):
        with pytest.raises(ValueError):
            population_layout(P, E)


# ---------------------------------------------------------------------------------------------------------------------
# PopulationResult
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,E,G", [(4, 70, 2), (3, 64, 1), (5, 1, 2)])
def test_population_result_per_policy_and_best(P, E, G):
    """per_policy() and best() on synthetic per-env tensors against NumPy over the live rows; the padding rows hold sentinels that
    would wreck every mean if one were read."""
    from gym_rotor_amd import EvalResult, PopulationResult
    from gym_rotor_amd.policy import population_layout
    epad, n = population_layout(P, E)
    r = np.random.default_rng(P * 100 + E)
    live = (np.arange(n) % epad) < E
    length = np.where(live, r.integers(1, 1001, n), -10 ** 6).astype(np.int32)
    flat = {"episode_return": np.where(live[:, None], r.uniform(-50, 900, (n, G)), 1e30),
            "benchmark": np.where(live, r.uniform(0, 1000, n), -1e30),
            "length": length, "terminated": np.where(live, length < 1000, True),
            "success": np.where(live[:, None], (length == 1000)[:, None] | (r.random((n, G)) < 0.3), True),
            "final_error": np.where(live[:, None], r.normal(size=(n, 4)), np.nan).astype(np.float32)}
    flat["terminated"][live] = r.random(int(live.sum())) < 0.4
    res = PopulationResult({k: torch.from_numpy(v) for k, v in flat.items()}, P, E)
    assert len(res) == P
    for k, v in flat.items():
        view = getattr(res, k)
        assert tuple(view.shape) == (P, E) + v.shape[1:], k
        assert np.array_equal(view.numpy(), v[live].reshape((P, E) + v.shape[1:])), k
        assert view.data_ptr() == res.flat[k].data_ptr()   # a view, not a copy
    pp = res.per_policy()
    want = {k: flat[k][live].reshape((P, E) + flat[k].shape[1:]).astype(np.float64).mean(1)
            for k in ("episode_return", "benchmark", "success", "length", "terminated")}
    for k, w in want.items():
        assert tuple(pp[k].shape) == w.shape and pp[k].dtype == torch.float64, k
        np.testing.assert_allclose(pp[k].numpy(), w, rtol=1e-13, atol=0, err_msg=k)
    assert res.best() == int(np.argmax(want["benchmark"])) == res.best("benchmark")
    assert res.best("episode_return") == int(np.argmax(want["episode_return"].sum(1)))
    assert res.best("length") == int(np.argmax(want["length"]))
    for p in (0, P - 1):
        one = res[p]
        assert isinstance(one, EvalResult) and one.length.numel() == E
        s = one.summary()
        assert s["episodes"] == E and s["benchmark_reward"] == round(float(want["benchmark"][p]), 4)
        assert s["eval_reward"] == [round(float(x), 4) for x in want["episode_return"][p]]
        assert s["mean_length"] == pytest.approx(float(want["length"][p]), rel=1e-13)
