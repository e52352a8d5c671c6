"""The evolution-strategy entries (qr_es_perturb, qr_es_gradient; gym_rotor_amd/es.py) without a GPU: the restatement of
tests/es_ref.py on hand-made cases, the structs against the compiled header, every error code of the two entries (each case fails one
check, so nothing is ever launched), every ValueError of the Python side before a launch, and EvolutionStrategy's constructor checks and
state_dict round trip."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import es_ref as R  # noqa: E402
import noise_ref as NR  # noqa: E402

from gym_rotor_amd import _lib as L  # noqa: E402
from gym_rotor_amd import es as ES  # noqa: E402
from gym_rotor_amd.policy import ActorParams  # noqa: E402

INF, NAN = float("inf"), float("nan")
NULL, SIZE, ALIGN = -1, -3, -4
SEED = 2 ** 40 + 3


# ---------------------------------------------------------------- the restatement
def test_stream_index_is_the_noise_stream_of_a_half_by_4q_tensor():
    n, half, gen, s = 6, 3, 2 ** 32 + 1, 77      # Q = 2: rows of 8 stream elements, of which 6 are the tensor's
    e = R.eps(n, half, SEED, gen, s)
    flat = NR.normal(half * 8, SEED, gen, s)
    for j in range(half):
        for k in range(n):
            assert R.stream_index(j, k, n) == j * 8 + k and e[j, k] == flat[j * 8 + k]
    # the quad of (j, e) is j * Q + e // 4: its words come from that counter alone
    z = NR.normals_from_words(NR.words(4, SEED, gen, s, first_quad=2 * 2 + 1))
    assert np.array_equal(e[2, 4:6], z[0, :2])
    assert not np.array_equal(R.eps(n, half, SEED, gen + 1, s), e) and not np.array_equal(R.eps(n, half, SEED, gen, s + 1), e)


def test_perturbation_rounds_the_product_first():
    theta = np.array([1.0, -0.25, 3.0], dtype=np.float32)
    draws = np.array([[0.5, 1.0, -2.0], [np.float32(1) / np.float32(3), 0.1, 7.0]], dtype=np.float32)
    got = R.perturb(theta, draws, 0.1)
    d = (np.float32(0.1) * draws).astype(np.float32)
    assert got.shape == (4, 3) and got.dtype == np.float32
    assert np.array_equal(got[0], theta + d[0]) and np.array_equal(got[1], theta - d[0]) and np.array_equal(got[3], theta - d[1])
    # a case where one rounding of theta + sigma * eps differs from two: the product's low bits decide a tie
    th, s, e = np.float32(1.0), np.float32(2.0 ** -24 + 2.0 ** -47), np.float32(1.0)
    assert R.perturb([th], [[e]], s)[0, 0] == np.float32(np.float32(s * e) + th)
    # a pair's mean is theta within one rounding of each member
    assert np.abs(got[0::2].astype(np.float64) + got[1::2] - 2.0 * theta).max() <= 2.0 ** -23 * np.abs(got).max()


def test_centered_ranks_by_hand():
    assert np.array_equal(R.centered_ranks([3.0, 1.0, 2.0, 4.0]), np.array([2, 0, 1, 3]) / 3.0 - 0.5)
    # ties share their mean rank; a NaN ranks as -inf and ties with it
    u = R.centered_ranks([1.0, 2.0, 2.0, NAN, -INF, 5.0])
    assert np.array_equal(u, np.array([2.0, 3.5, 3.5, 0.5, 0.5, 5.0]) / 5.0 - 0.5)
    assert np.array_equal(R.pair_weights([1.0, 2.0, 2.0, NAN, -INF, 5.0]), np.array([u[0] - u[1], u[2] - u[3], u[4] - u[5]]))
    assert np.array_equal(R.centered_ranks([NAN, NAN]), [0.0, 0.0]) and np.array_equal(R.centered_ranks([-0.0, 0.0]), [0.0, 0.0])
    assert np.array_equal(R.centered_ranks([INF, -INF]), [0.5, -0.5])
    assert abs(R.centered_ranks(np.arange(64.0)).sum()) <= 1e-12


@pytest.mark.parametrize("P", [2, 6, 64, 8192])
def test_all_equal_fitness_gives_zero_weights(P):
    for v in (0.0, -3.25, INF, NAN):
        w = R.pair_weights(np.full(P, v, dtype=np.float32))
        assert w.shape == (P // 2,) and (w == 0.0).all()
    assert (R.pair_weights(np.full(P, 1.5, dtype=np.float32), R.STANDARDIZE) == 0.0).all()


def test_standardize_and_stats_by_hand():
    f = np.array([1.0, 3.0, 5.0, 7.0], dtype=np.float32)
    std = np.sqrt(((f.astype(np.float64) - 4.0) ** 2).sum() / 3.0)
    assert np.array_equal(R.pair_weights(f, R.STANDARDIZE), np.array([-2.0, -2.0]) / (std + 1e-8))
    u = (f.astype(np.float64) - 4.0) / (std + 1e-8)
    assert np.abs(R.pair_weights(f, R.STANDARDIZE) - (u[0::2] - u[1::2])).max() <= 1e-15
    for bad in (NAN, INF, -INF):
        g = f.copy()
        g[2] = bad
        assert (R.pair_weights(g, R.STANDARDIZE) == 0.0).all() and R.fitness_stats(g)[3] == 1.0
    assert np.array_equal(R.fitness_stats([1.0, 7.0, 7.0, NAN, -2.0, 3.0])[1:], [7.0, 1.0, 1.0])
    assert np.array_equal(R.fitness_stats(f), [4.0, 7.0, 3.0, 0.0])
    assert np.array_equal(R.fitness_stats([NAN, -INF])[1:], [-INF, 0.0, 1.0])


def test_estimator_by_hand():
    w, draws = np.array([0.5, -1.0]), np.array([[1.0, 2.0, 0.0], [3.0, -1.0, 4.0]])
    s = np.float64(np.float32(0.1))
    assert np.allclose(R.gradient(w, draws, 0.1), -np.array([0.5 - 3.0, 1.0 + 1.0, -4.0]) / (4 * s), rtol=1e-15, atol=0)
    assert np.abs(R.gradient(w, draws, 0.1, wide=True) - R.gradient(w, draws, 0.1)).max() <= 1e-15
    # plain ES: f = a . theta is ascended — the estimate is a descent direction of -f
    rng = np.random.default_rng(0)
    a, e = rng.normal(size=5), R.eps(5, 512, 1, 0, 3)
    fit = np.stack([e @ a, -(e @ a)], 1).reshape(-1)            # f(theta +- sigma eps) - f(theta), up to sigma
    g = R.gradient(R.pair_weights(fit), e, 1.0)
    assert g @ a < 0 and abs(g @ a) / (np.linalg.norm(g) * np.linalg.norm(a)) > 0.9
    b = R.gradient_bound(w, draws, 0.1, R.gradient(w, draws, 0.1))
    assert (b > 0).all() and (b < 1e-6).all()


def test_closed_loop_of_the_restatement_halves_the_distance_with_room():
    sizes, theta0, target, streams = R.loop_problem()     # the device test's problem and settings
    assert streams == [ES.es_stream(0, n) for n in ES.NAMES]
    ratio = R.closed_loop(sizes, theta0, target, seed=SEED, streams=streams, **R.LOOP)
    assert ratio < 0.25, ratio      # 0.182: the device test's condition, < 0.5, with room


# ---------------------------------------------------------------- the structs and the C entries' errors
def test_structs_mirror_the_header(tmp_path):
    structs = ("QrEsTensor", "QrEsCopy", "QrEsPerturb", "QrEsGradient")
    lines = ['printf("abi %d\\n", QR_ABI_VERSION);']
    lines += [f'printf("{n} %d\\n", {n});' for n in ("QR_ES_MAX_TENSORS", "QR_ES_MAX_COPIES", "QR_ES_MAX_POLICIES", "QR_ES_STATS", "QR_ES_CENTERED_RANK",
                                                     "QR_ES_STANDARDIZE")]
    for s in structs:
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f, _ in getattr(L, s)._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for s in structs:
        assert int(out[s]) == C.sizeof(getattr(L, s)), s
        for f, _ in getattr(L, s)._fields_:
            assert int(out[f"{s}.{f}"]) == getattr(getattr(L, s), f).offset, (s, f)
    assert (int(out["QR_ES_MAX_TENSORS"]), int(out["QR_ES_MAX_COPIES"]), int(out["QR_ES_MAX_POLICIES"]), int(out["QR_ES_STATS"])) == (
        L.ES_MAX_TENSORS, L.ES_MAX_COPIES, L.ES_MAX_POLICIES, L.ES_STATS)
    assert (int(out["QR_ES_CENTERED_RANK"]), int(out["QR_ES_STANDARDIZE"])) == (L.ES_CENTERED_RANK, L.ES_STANDARDIZE)
    lib = L.load()
    assert {"qr_es_perturb", "qr_es_gradient", "qr_es_workspace_bytes"} <= set(L.SYMBOLS) and hasattr(lib, "qr_es_gradient")
    assert int(out["abi"]) == L.ABI_VERSION == lib.qr_abi_version()


def test_workspace_bytes():
    lib = L.load()
    for P in (2, 6, 130, 8192):
        assert lib.qr_es_workspace_bytes(P) == 8 * ES.es_workspace_numel(P) == 4 * P
    for P in (0, 1, 3, -2, 8194, 8193):
        assert lib.qr_es_workspace_bytes(P) == SIZE
        with pytest.raises(ValueError):
            ES.es_workspace_numel(P)


def _fake_perturb():
    """A QrEsPerturb over made-up, aligned addresses that passes every check but for what a case changes."""
    p = L.QrEsPerturb()
    a = iter(range(0x10000, 0x90000, 0x1000))
    p.n_tensors, p.n_copies, p.n_policies, p.max_workgroups, p.sigma, p.seed, p.generation = 3, 2, 6, 0, 0.1, SEED, 5
    for k in range(3):
        t = p.tensor[k]
        t.base, t.out, t.count, t.stream = next(a), next(a), (12, 1, 4)[k], 100 + k
    for k in range(2):
        c = p.copy[k]
        c.src, c.dst, c.count = next(a), next(a), 4
    return p


def _fake_gradient():
    g = L.QrEsGradient()
    a = iter(range(0x10000, 0x90000, 0x1000))
    g.n_tensors, g.n_policies, g.shaping, g.max_workgroups, g.sigma, g.seed, g.generation = 3, 6, 0, 0, 0.1, SEED, 5
    for k in range(3):
        t = g.tensor[k]
        t.out, t.count, t.stream = next(a), (12, 1, 4)[k], 100 + k
    g.fitness, g.stats, g.workspace, g.workspace_bytes = next(a), next(a), next(a), 24
    return g


def _set(s, path, value):
    for part in path[:-1]:
        s = s[part] if isinstance(part, int) else getattr(s, part)
    setattr(s, path[-1], value)


SHARED_CASES = [
    (("n_policies",), 0, SIZE), (("n_policies",), 1, SIZE), (("n_policies",), 7, SIZE), (("n_policies",), 8194, SIZE), (("n_policies",), -2, SIZE),
    (("n_tensors",), 0, SIZE), (("n_tensors",), 17, SIZE), (("tensor", 1, "count"), 0, SIZE), (("tensor", 1, "count"), -4, SIZE),
    (("tensor", 0, "count"), 2 ** 31, SIZE), (("tensor", 2, "stream"), 2 ** 30, SIZE),
    (("tensor", 2, "stream"), 100, SIZE), (("tensor", 1, "stream"), 102, SIZE), (("tensor", 0, "reserved0"), 1, SIZE),
    (("sigma",), 0.0, SIZE), (("sigma",), -0.1, SIZE), (("sigma",), NAN, SIZE), (("sigma",), INF, SIZE), (("reserved0",), 1.0, SIZE),
    (("max_workgroups",), -1, SIZE), (("generation",), -1, SIZE),
    (("tensor", 0, "out"), None, NULL), (("tensor", 2, "out"), None, NULL),
    (("tensor", 1, "out"), 0x50002, ALIGN), (("generation_dev",), 0x60004, ALIGN)]


@pytest.mark.parametrize("path,value,want", SHARED_CASES + [
    (("n_copies",), -1, SIZE), (("n_copies",), 9, SIZE), (("copy", 1, "count"), 0, SIZE), (("copy", 0, "count"), 2 ** 31, SIZE),
    (("tensor", 0, "base"), None, NULL), (("copy", 0, "src"), None, NULL), (("copy", 1, "dst"), None, NULL),
    (("tensor", 2, "base"), 0x50001, ALIGN), (("copy", 0, "src"), 0x50002, ALIGN), (("copy", 1, "dst"), 0x50003, ALIGN)])
def test_perturb_errors(path, value, want):
    lib = L.load()
    p = _fake_perturb()
    _set(p, path, value)
    assert lib.qr_es_perturb(C.byref(p), None) == want


@pytest.mark.parametrize("path,value,want", SHARED_CASES + [
    (("shaping",), 2, SIZE), (("shaping",), -1, SIZE), (("workspace_bytes",), 23, SIZE),
    (("fitness",), None, NULL), (("stats",), None, NULL), (("workspace",), None, NULL),
    (("fitness",), 0x50002, ALIGN), (("stats",), 0x50004, ALIGN), (("workspace",), 0x50004, ALIGN)])
def test_gradient_errors(path, value, want):
    lib = L.load()
    g = _fake_gradient()
    _set(g, path, value)
    assert lib.qr_es_gradient(C.byref(g), None) == want


def test_null_structs_and_the_order_of_the_checks():
    lib = L.load()
    assert lib.qr_es_perturb(None, None) == NULL and lib.qr_es_gradient(None, None) == NULL
    p = _fake_perturb()   # a size error comes before a NULL pointer, a NULL pointer before a misaligned one
    p.tensor[0].base, p.tensor[1].out = None, 0x50002
    assert lib.qr_es_perturb(C.byref(p), None) == NULL
    p.sigma = 0.0
    assert lib.qr_es_perturb(C.byref(p), None) == SIZE
    g = _fake_gradient()
    g.stats, g.tensor[1].out = None, 0x50002
    assert lib.qr_es_gradient(C.byref(g), None) == NULL
    g.n_policies = 7
    assert lib.qr_es_gradient(C.byref(g), None) == SIZE
    # (P / 2) * the quads of all tensors must stay below 2^31: 4096 * (2^19 + 1 + 1)
    p, g = _fake_perturb(), _fake_gradient()
    p.n_policies = g.n_policies = 8192
    p.tensor[0].count = g.tensor[0].count = 2 ** 21
    g.workspace_bytes = 4 * 8192
    assert lib.qr_es_perturb(C.byref(p), None) == SIZE and lib.qr_es_gradient(C.byref(g), None) == SIZE
    # generation_dev given: a negative `generation` is not read; a device word takes the place of the value
    p = _fake_perturb()
    p.generation, p.generation_dev, p.tensor[0].base = -1, 0x60008, None
    assert lib.qr_es_perturb(C.byref(p), None) == NULL


# ---------------------------------------------------------------- the Python layer before a launch
def _actor(dims=(3, 4, 1), log_std=True):
    g = torch.Generator().manual_seed(1)
    a = ActorParams.random(*dims, device="cpu", generator=g)
    if not log_std:
        a.log_std = None
    return a


def test_es_stream():
    ids = [ES.es_stream(k, n) for k in range(3) for n in ES.NAMES]
    assert len(set(ids)) == 18 and all(ES.ES_STREAM <= i < 1 << 29 for i in ids) and ES.es_stream(0, "fc1_w") == 1 << 28
    from gym_rotor_amd import offpolicy
    assert offpolicy.noise_stream(255, offpolicy.NOISE_NAMES[-1], 3) < ES.ES_STREAM < offpolicy.COLLECTOR_STREAM
    for bad in ((0, "log_std"), (-1, "fc1_w"), (1 << 16, "fc1_w")):
        with pytest.raises(ValueError):
            ES.es_stream(*bad)


def test_population_like():
    a = _actor()
    pop = ES.population_like([a], 6)
    assert len(pop) == 6 and pop.agents[0].fc1_w.shape == (6, 4, 3) and pop.agents[0].log_std.shape == (6, 1) and pop.agents[0].log_std_w is None
    with pytest.raises(ValueError):
        ES.population_like([a], 0)


KEY = dict(sigma=0.1, seed=SEED, generation=0)


def test_es_perturb_value_errors():
    a = _actor()
    pop = ES.population_like([a], 6)
    with pytest.raises(RuntimeError, match="GPU only"):     # every check passes: what is left is that no CPU kernel exists
        ES.es_perturb([a], pop, **KEY)
    for P in (1, 3, 8194):
        with pytest.raises(ValueError, match="even number"):
            ES.es_perturb([a], ES.population_like([a], P), **KEY)
    for bad in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=NAN), dict(sigma=INF), dict(sigma=1e-60), dict(seed=-1), dict(seed=2 ** 64),
                dict(generation=-1), dict(generation=2 ** 63), dict(generation=torch.zeros(1, dtype=torch.int32)),
                dict(generation=torch.zeros(2, dtype=torch.int64)), dict(streams=[1, 2, 3]), dict(streams=[1, 2, 3, 4, 5, 5]),
                dict(streams=[1, 2, 3, 4, 5, 2 ** 30]), dict(streams=[-1, 2, 3, 4, 5, 6]), dict(max_workgroups=-1)):
        with pytest.raises(ValueError):
            ES.es_perturb([a], pop, **dict(KEY, **bad))
    with pytest.raises(ValueError, match="ActorPopulation"):
        ES.es_perturb([a], [a], **KEY)
    with pytest.raises(ValueError, match="ActorPopulation"):
        ES.es_perturb([a, a], pop, **KEY)
    with pytest.raises(ValueError, match="differ in form"):
        ES.es_perturb([_actor(log_std=False)], pop, **KEY)
    with pytest.raises(ValueError, match="stacked tensor fc1_w"):
        ES.es_perturb([_actor((15, 16, 4))], pop, **KEY)
    wrong = ES.population_like([a], 6)
    wrong.agents[0].fc2_b = wrong.agents[0].fc2_b.double()
    with pytest.raises(ValueError, match=r"out\[3\]"):
        ES.es_perturb([a], wrong, **KEY)
    wrong = ES.population_like([a], 6)
    wrong.agents[0].log_std = torch.empty(6, 2)[:, :1]
    with pytest.raises(ValueError, match="destination"):
        ES.es_perturb([a], wrong, **KEY)
    t, o = torch.zeros(5), torch.zeros(6, 5)
    for base, out in (([], []), ([t] * 17, [o] * 17), ([t], [o, o]), ([torch.zeros(0)], [torch.zeros(6, 0)]), ([t.double()], [o]), ([t], [torch.zeros(6, 4)]),
                      ([t], [torch.zeros(6, 10)[:, ::2]]), ([t], [torch.zeros(())])):
        with pytest.raises(ValueError):
            ES.es_perturb_tensors(base, out, streams=list(range(len(base))), **KEY)
    with pytest.raises(ValueError, match="at most 8"):
        ES.es_perturb_tensors([t], [o], streams=[0], copies=[(t, o)] * 9, **KEY)


def test_es_gradient_value_errors():
    fit = torch.zeros(6)
    grads = [{n: torch.zeros_like(getattr(_actor(), n)) for n in ES.NAMES}]
    with pytest.raises(RuntimeError, match="GPU only"):
        ES.es_gradient(fit, grads, **KEY)
    with pytest.raises(RuntimeError, match="GPU only"):
        ES.es_gradient(fit, [torch.zeros(3)], streams=[9], stats=torch.zeros(4, dtype=torch.float64), workspace=torch.zeros(3, dtype=torch.float64), **KEY)
    for f in (torch.zeros(7), torch.zeros(0), torch.zeros(6, dtype=torch.float64), torch.zeros(2, 3), torch.zeros(12)[::2], [0.0] * 6, torch.zeros(8194)):
        with pytest.raises(ValueError):
            ES.es_gradient(f, grads, **KEY)
    for bad in (dict(shaping="rank"), dict(sigma=0.0), dict(seed=-1), dict(generation=-1), dict(streams=[1, 2]), dict(max_workgroups=-1),
                dict(stats=torch.zeros(4)), dict(stats=torch.zeros(5, dtype=torch.float64)), dict(workspace=torch.zeros(2, dtype=torch.float64)),
                dict(workspace=torch.zeros(3))):
        with pytest.raises(ValueError):
            ES.es_gradient(fit, grads, **dict(KEY, **bad))
    with pytest.raises(ValueError, match="needs streams"):
        ES.es_gradient(fit, [torch.zeros(3)], **KEY)
    with pytest.raises(ValueError, match="each of"):
        ES.es_gradient(fit, [{"fc1_w": torch.zeros(3)}], **KEY)
    for g in ([], [torch.zeros(3)] * 17, [torch.zeros(0)], [torch.zeros(3, dtype=torch.float64)], [torch.zeros(6)[::2]]):
        with pytest.raises(ValueError):
            ES.es_gradient(fit, g, streams=list(range(len(g))), **KEY)


def test_population_fitness_on_the_cpu():
    P, E = 4, 3
    flat = {"benchmark": torch.arange(P * 64, dtype=torch.float64), "episode_return": torch.ones(P * 64, 2, dtype=torch.float64)}
    got = ES.population_fitness(flat, P, E)
    assert got.dtype == torch.float32 and torch.equal(got, torch.tensor([1.0, 65.0, 129.0, 193.0]))
    assert torch.equal(ES.population_fitness(flat, P, E, "return"), torch.full((P,), 2.0))
    with pytest.raises(ValueError):
        ES.population_fitness(flat, P, E, "success")


# ---------------------------------------------------------------- EvolutionStrategy
class _Actor(torch.nn.Module):
    def __init__(self, d, h, a):
        super().__init__()
        self.fc1, self.fc2, self.mean_linear = torch.nn.Linear(d, h), torch.nn.Linear(h, h), torch.nn.Linear(h, a)
        self.log_std = torch.nn.Parameter(torch.zeros(1, a))


def _modules(kind="decoupled"):
    torch.manual_seed(0)
    from gym_rotor_amd.policy import ACTOR_DIMS
    return [_Actor(*d) for d in ACTOR_DIMS[kind]]


def test_constructor_checks():
    ok = dict(population=8, episodes_per_policy=4, seed=1)
    for kind, mods, kw in (("quad", _modules("coupled"), {}), ("coupled", _modules("decoupled"), {}), ("decoupled", _modules("coupled"), {}),
                           ("coupled", _modules("coupled"), dict(population=7)), ("coupled", _modules("coupled"), dict(population=0)),
                           ("coupled", _modules("coupled"), dict(population=8194)), ("coupled", _modules("coupled"), dict(episodes_per_policy=0)),
                           ("coupled", _modules("coupled"), dict(sigma=0.0)), ("coupled", _modules("coupled"), dict(sigma=NAN)),
                           ("coupled", _modules("coupled"), dict(seed=-1)), ("coupled", _modules("coupled"), dict(fitness="success")),
                           ("coupled", _modules("coupled"), dict(shaping="rank")), ("coupled", _modules("coupled"), dict(max_steps=0)),
                           ("coupled", _modules("coupled"), dict(num_envs=3)), ("coupled", [torch.nn.Linear(2, 2)], {}),
                           ("coupled", [_Actor(15, 16, 4)], {}), ("coupled", _modules("coupled"), dict(optimizer=dict(lr=-1.0)))):
        with pytest.raises(ValueError):
            ES.EvolutionStrategy(kind, mods, **dict(ok, **kw))
    if not torch.cuda.is_available():    # every check passed: what is left is that the env needs a GPU
        with pytest.raises(RuntimeError):
            ES.EvolutionStrategy("coupled", _modules("coupled"), **ok)


class _HostES(ES.EvolutionStrategy):
    """The object without its env: what state_dict / load_state_dict touch lives on the modules' device."""

    def _build(self, env_kw):
        pass


def test_state_dict_round_trip():
    a = _HostES("decoupled", _modules(), population=8, episodes_per_policy=4, seed=SEED, sigma=0.07, optimizer=dict(lr=0.02))
    assert a.generation == 0 and len(a.optimizers) == 2 and a.optimizers[0].lr == 0.02 and a.optimizers[0].weight_decay == 0.0
    a.generation = 5
    a.optimizers[1].exp_avg.fill_(0.25), a.optimizers[1].step_count.fill_(5), a.optimizers[0].exp_avg_sq.fill_(2.0)
    state = a.state_dict()
    assert state["seed"] == SEED and state["generation"] == 5 and state["sigma"] == 0.07 and len(state["optimizers"]) == 2
    b = _HostES("decoupled", _modules(), population=8, episodes_per_policy=4, seed=SEED)
    b.load_state_dict(state)
    assert b.generation == 5 and b.sigma == 0.07 and b.optimizers[0].lr == 0.02
    for x, y in zip(a.optimizers, b.optimizers):
        assert torch.equal(x.exp_avg, y.exp_avg) and torch.equal(x.exp_avg_sq, y.exp_avg_sq) and torch.equal(x.step_count, y.step_count)
    state["optimizers"][0]["exp_avg"].fill_(9.0)       # the state holds copies
    assert not (a.optimizers[0].exp_avg == 9.0).any()
    with pytest.raises(ValueError, match="seed"):
        _HostES("decoupled", _modules(), population=8, episodes_per_policy=4, seed=1).load_state_dict(a.state_dict())
    with pytest.raises(ValueError):
        _HostES("coupled", _modules("coupled"), population=8, episodes_per_policy=4, seed=SEED).load_state_dict(a.state_dict())
    with pytest.raises(ValueError):
        b.load_state_dict(dict(a.state_dict(), generation=-1))
    with pytest.raises(ValueError, match="no generation"):
        _HostES("decoupled", _modules(), population=8, episodes_per_policy=4, seed=SEED).best()
