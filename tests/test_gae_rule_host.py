"""PPO's advantages over the done flag the reference stores (qr_gae_rule; rollout.gae_rule, RolloutStorage.compute_gae(time_limit=,
rule=, normalized=, done_eff=), ppo.PpoCollector) without a GPU: the restatement of tests/gae_rule_ref.py against the GAE oracle and on
the hand-made rows of tests/replay_rule_ref.py, the new struct's layout, every error code of the new entry, every ValueError of the
Python side before a launch, the unchanged default path of compute_gae, and the collector's construction checks."""
import contextlib
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gae_rule_ref as G  # noqa: E402
import replay_rule_ref as RR  # noqa: E402
from test_replay_host import COUPLED, DECOUPLED, fake_storage  # noqa: E402
from test_replay_rule_host import _Env, rule_storage  # noqa: E402

from oracle import gae_oracle as go  # noqa: E402
from gym_rotor_amd import _lib as L  # noqa: E402
from gym_rotor_amd.ppo import PpoCollector  # noqa: E402
from gym_rotor_amd.rollout import RolloutStorage, gae_rule, gae_rule_workspace_numel  # noqa: E402
from gym_rotor_amd.td3 import TimeLimitRule  # noqa: E402

T, N = 3, 65
GAMMA, LAM = 0.99, 0.9
RULE = (RR.X_LIM, RR.POS_TOL, RR.ROT_TOL)
INF, NAN = float("inf"), float("nan")


def values_for(s, seed=0):
    """value [T + 1, N, G] and next_value [T, N, G] float32 for a fake storage: a critic's outputs, made up."""
    rng = np.random.default_rng(1000 + seed)
    value = rng.normal(0, 2, (s.T + 1, s.N, s.n_agents)).astype(np.float32)
    next_value = np.where(rng.uniform(size=(s.T, s.N, 1)) < 0.5, value[1:], rng.normal(0, 2, (s.T, s.N, s.n_agents))).astype(np.float32)
    return value, next_value


def numpy_of(s):
    """(obs, final_obs, reward, done, truncated) of a fake storage as NumPy arrays: the first five arguments of gae_rule_ref.run."""
    return ([o.cpu().numpy() for o in s.obs], None if s.final_obs is None else [f.cpu().numpy() for f in s.final_obs], s.reward.cpu().numpy(),
            s.done.cpu().numpy(), s.truncated.cpu().numpy())


def real_storage(s, device="cpu", x_lim=1.5):
    """A RolloutStorage that holds a fake storage's rows: what compute_gae reads, on `device`."""
    dims = [o.shape[-1] for o in s.obs]
    env = types.SimpleNamespace(kind="decoupled" if s.n_agents == 2 else "coupled", num_envs=s.N, auto_reset=True, obs_rows=True, n_agents=s.n_agents,
                                obs_dims=dims, action_dim=sum(s.action_dims), device=torch.device(device))
    if x_lim is not None:
        env.x_lim = x_lim
    st = RolloutStorage(env, s.T, action_dims=s.action_dims, final_obs=s.final_obs is not None)
    for dst, src in zip(st.obs, s.obs):
        dst.copy_(src)
    if s.final_obs is not None:
        for dst, src in zip(st.final_obs, s.final_obs):
            dst.copy_(src)
    st.reward.copy_(s.reward), st.done.copy_(s.done), st.truncated.copy_(s.truncated)
    return st


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("dims", [COUPLED, DECOUPLED])
def test_restatement_without_the_rule_is_the_oracle(dims):
    s = rule_storage(dims, seed=1)
    value, next_value = values_for(s, 1)
    a = numpy_of(s)
    for nv in (None, next_value):
        got = G.run(*a, value, nv, GAMMA, LAM, rule=None)
        M = N * s.n_agents
        want_nv = value[1:] if nv is None else nv
        adv, tgt = go.gae(a[2].reshape(T, M), a[3].reshape(T, M), value[:-1].reshape(T, M), want_nv.reshape(T, M), GAMMA, LAM)
        assert np.array_equal(got["done_eff"], a[3])
        assert np.abs(got["advantage"].reshape(T, M) - adv).max() <= 1e-12 and np.abs(got["td_target"].reshape(T, M) - tgt).max() <= 1e-12
        for k in range(s.n_agents):
            assert np.abs(got["normalized"][..., k] - go.normalize(adv.reshape(T, N, -1)[..., k])).max() <= 1e-9
        f32 = G.run(*a, value, nv, GAMMA, LAM, rule=None, f32=True)
        assert f32["advantage"].dtype == np.float32
        assert np.abs(f32["advantage"] - got["advantage"]).max() <= 2e-6 * max(1.0, np.abs(got["advantage"]).max())


@pytest.mark.parametrize("dims,final", [(COUPLED, True), (DECOUPLED, True), (DECOUPLED, False)])
def test_planted_rows_hold_what_the_cases_say(dims, final):
    s = rule_storage(dims, final_obs=final, seed=2)
    value, next_value = values_for(s, 2)
    got = G.run(*numpy_of(s), value, next_value, GAMMA, LAM, rule=RULE)
    places = RR.places(T, N)
    for (t, n), want in RR.expected(places, s.n_agents).items():
        assert tuple(float(x) for x in got["done_eff"][t, n]) == tuple(want), (t, n, places[(t, n)])
    own = numpy_of(s)[3]
    lim = numpy_of(s)[4]
    assert np.array_equal(got["done_eff"][~lim], own[~lim])
    assert (got["done_eff"] & ~own).any() and (~got["done_eff"] & own).any()


@pytest.mark.parametrize("dims", [COUPLED, DECOUPLED])
def test_the_rule_moves_the_advantages_the_way_the_cases_predict(dims):
    """At t = 1 env 20 is "solved" (own done 0: the reference does not bootstrap and cuts the recursion) and env 21 is "own_done_far"
    (own done 1, not solved: the reference bootstraps and the recursion continues); step 0 of both envs is an ordinary transition."""
    s = rule_storage(dims, seed=3)
    s.done[0, 20:22] = False
    s.truncated[0, 20:22] = False
    RR.plant(s, {(1, 20): "solved", (1, 21): "own_done_far"})
    value, next_value = values_for(s, 3)
    a = numpy_of(s)
    ruled = G.run(*a, value, next_value, GAMMA, LAM, rule=RULE)
    plain = G.run(*a, value, next_value, GAMMA, LAM, rule=None)
    r, v, nv = a[2].astype(np.float64), value.astype(np.float64), next_value.astype(np.float64)
    for g in range(s.n_agents):
        # "solved": the TD error has no bootstrap term and nothing of step 2 reaches step 1
        assert ruled["done_eff"][1, 20, g] and not plain["done_eff"][1, 20, g]
        assert ruled["advantage"][1, 20, g] == r[1, 20, g] - v[1, 20, g]
        assert abs(plain["advantage"][1, 20, g] - (r[1, 20, g] + GAMMA * nv[1, 20, g] - v[1, 20, g] + GAMMA * LAM * plain["advantage"][2, 20, g])) <= 1e-12
        # "own_done_far": the other way round
        assert not ruled["done_eff"][1, 21, g] and plain["done_eff"][1, 21, g]
        assert plain["advantage"][1, 21, g] == r[1, 21, g] - v[1, 21, g]
        assert abs(ruled["advantage"][1, 21, g] - (r[1, 21, g] + GAMMA * nv[1, 21, g] - v[1, 21, g] + GAMMA * LAM * ruled["advantage"][2, 21, g])) <= 1e-12
        # and the step before inherits the difference through gamma * lambda
        for n in (20, 21):
            d1 = ruled["advantage"][1, n, g] - plain["advantage"][1, n, g]
            d0 = ruled["advantage"][0, n, g] - plain["advantage"][0, n, g]
            assert abs(d1) > 1e-3 and abs(d0 - GAMMA * LAM * d1) <= 1e-12, (n, g)
    others = np.ones(N, dtype=bool)
    others[20:22] = False
    keep = ~a[4][:, others].any(0)   # envs that never meet the time limit are untouched
    assert keep.any() and np.array_equal(ruled["advantage"][:, others][:, keep], plain["advantage"][:, others][:, keep])


def test_stats_and_normalisation_of_the_restatement():
    rng = np.random.default_rng(5)
    adv = rng.normal(0.3, 2.0, (4, 9, 2))
    st = G.sums(adv)
    assert st.shape == (2, 3) and (st[:, 2] == 36).all()
    nrm = G.normalize(adv, st)
    want = (adv - adv.mean((0, 1))) / (adv.reshape(-1, 2).std(0, ddof=1) + 1e-4)
    assert np.abs(nrm - want).max() <= 1e-12
    torch_nrm = RolloutStorage.normalize(torch.from_numpy(adv).float(), torch.from_numpy(G.sums(adv.astype(np.float32)))).numpy()
    assert np.abs(torch_nrm - G.normalize(adv.astype(np.float32), G.sums(adv.astype(np.float32)))).max() <= 1e-6


# ---------------------------------------------------------------- the struct and the C entry's errors
def test_struct_mirrors_the_header(tmp_path):
    lines = ['printf("abi %d\\n", QR_ABI_VERSION);', 'printf("QrGaeRule %zu\\n", sizeof(QrGaeRule));']
    lines += [f'printf("QrGaeRule.{f} %zu\\n", offsetof(QrGaeRule, {f}));' for f, _ in L.QrGaeRule._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["QrGaeRule"]) == C.sizeof(L.QrGaeRule)
    for f, _ in L.QrGaeRule._fields_:
        assert int(out[f"QrGaeRule.{f}"]) == getattr(L.QrGaeRule, f).offset, f
    lib = L.load()
    assert {"qr_gae_rule", "qr_gae_rule_workspace_bytes"} <= set(L.SYMBOLS) and hasattr(lib, "qr_gae_rule")
    assert int(out["abi"]) == L.ABI_VERSION == 16 and lib.qr_abi_version() == 16   # a struct and two entries were added: the version stays


def test_workspace_bytes():
    lib = L.load()
    for n, na in ((0, 1), (1, 1), (64, 1), (65, 1), (32, 2), (33, 2), (64 * 257 + 1, 2), (16384, 2)):
        assert lib.qr_gae_rule_workspace_bytes(n, na) == 8 * gae_rule_workspace_numel(n, na) == 8 * max(1, (n * na + 63) // 64) * 2 * na
    assert lib.qr_gae_rule_workspace_bytes(-1, 1) == lib.qr_gae_rule_workspace_bytes(5, 0) == lib.qr_gae_rule_workspace_bytes(5, 3) == -3


NULL, SIZE, ALIGN = -1, -3, -4


def _fake_gae(na=2):
    """A QrGaeRule over made-up, aligned addresses, with the rule, every optional output and the normalisation, that passes every
    check but for what a case changes: each case fails one, so nothing is ever launched."""
    e = L.QrGaeRule()
    p = iter(range(0x10000, 0x80000, 0x1000))
    for name in ("reward", "done", "truncated", "term_obs0", "term_obs1", "value", "next_value", "advantage", "td_target", "done_eff", "stats",
                 "normalized", "workspace"):
        setattr(e, name, next(p))
    e.n_envs, e.n_steps, e.n_agents, e.d0, e.d1, e.rule, e.reserved0 = 65, 3, na, 15, 3, 1, 0
    e.workspace_bytes = 8 * gae_rule_workspace_numel(65, na)
    e.gamma, e.lam, e.x_lim, e.pos_tol, e.rot_tol, e.norm_eps = 0.99, 0.9, 1.0, 0.03, 0.03, 1e-4
    return e


@pytest.mark.parametrize("name,value,want", [
    ("n_steps", 0, SIZE), ("n_envs", -1, SIZE), ("n_envs", 2 ** 35 + 1, SIZE), ("n_agents", 0, SIZE), ("n_agents", 3, SIZE), ("reserved0", 1, SIZE),
    ("rule", 2, SIZE), ("rule", -1, SIZE), ("d0", 2, SIZE), ("d1", 0, SIZE), ("pos_tol", -1e-9, SIZE), ("pos_tol", NAN, SIZE), ("pos_tol", INF, SIZE),
    ("rot_tol", -0.03, SIZE), ("rot_tol", NAN, SIZE), ("rot_tol", INF, SIZE), ("x_lim", 0.0, SIZE), ("x_lim", -1.0, SIZE), ("x_lim", NAN, SIZE),
    ("x_lim", INF, SIZE), ("norm_eps", -1e-4, SIZE), ("norm_eps", NAN, SIZE), ("norm_eps", INF, SIZE), ("workspace_bytes", 8 * 4 * 3 - 1, SIZE),
    ("reward", None, NULL), ("done", None, NULL), ("value", None, NULL), ("advantage", None, NULL), ("td_target", None, NULL),
    ("truncated", None, NULL), ("term_obs0", None, NULL), ("term_obs1", None, NULL), ("stats", None, NULL), ("workspace", None, NULL),
    ("reward", 0x10002, ALIGN), ("value", 0x20001, ALIGN), ("next_value", 0x20002, ALIGN), ("advantage", 0x30003, ALIGN),
    ("td_target", 0x30002, ALIGN), ("normalized", 0x40002, ALIGN), ("term_obs0", 0x50002, ALIGN), ("term_obs1", 0x50001, ALIGN),
    ("stats", 0x60004, ALIGN), ("workspace", 0x70004, ALIGN)])
def test_gae_rule_errors(name, value, want):
    lib = L.load()
    e = _fake_gae()
    setattr(e, name, value)
    assert lib.qr_gae_rule(C.byref(e), None) == want
    assert lib.qr_gae_rule(None, None) == NULL


def test_gae_rule_errors_that_depend_on_what_is_asked_for():
    lib = L.load()
    e = _fake_gae()
    e.n_envs, e.n_steps = 1, 1                     # one transition per agent: no unbiased std
    assert lib.qr_gae_rule(C.byref(e), None) == SIZE
    e.normalized = None
    e.n_envs = 0                                   # every check passes; no envs: nothing is launched
    assert lib.qr_gae_rule(C.byref(e), None) == 0
    e = _fake_gae(1)                               # one agent: agent 1's members are not read
    e.term_obs1, e.d1, e.n_envs, e.normalized = None, 0, 0, None
    assert lib.qr_gae_rule(C.byref(e), None) == 0
    e = _fake_gae()                                # without the rule its members are not read
    e.rule, e.truncated, e.term_obs0, e.term_obs1, e.d0, e.d1, e.x_lim, e.pos_tol = 0, None, 0x50002, None, 0, 0, NAN, -1.0
    e.normalized, e.n_envs = None, 0
    assert lib.qr_gae_rule(C.byref(e), None) == 0
    e.next_value = 0x20002                         # (next_value is read without the rule too)
    assert lib.qr_gae_rule(C.byref(e), None) == ALIGN
    e = _fake_gae()                                # without normalized norm_eps is not read; without stats neither is the workspace
    e.normalized, e.norm_eps, e.n_envs = None, NAN, 0
    assert lib.qr_gae_rule(C.byref(e), None) == 0
    e.stats, e.workspace, e.workspace_bytes = None, 0x70004, 0
    assert lib.qr_gae_rule(C.byref(e), None) == 0
    e = _fake_gae()                                # every optional output null
    e.done_eff, e.stats, e.normalized, e.workspace, e.next_value, e.n_envs = None, None, None, None, None, 0
    assert lib.qr_gae_rule(C.byref(e), None) == 0
    # the order: sizes before pointers before alignment
    e = _fake_gae()
    e.n_steps, e.reward = 0, None
    assert lib.qr_gae_rule(C.byref(e), None) == SIZE
    e = _fake_gae()
    e.truncated, e.reward = None, 0x10002
    assert lib.qr_gae_rule(C.byref(e), None) == NULL
    e = _fake_gae()
    e.stats = None                                 # normalized without stats
    assert lib.qr_gae_rule(C.byref(e), None) == NULL


# ---------------------------------------------------------------- the Python side's checks, all before a launch
def _good(s=None, seed=4):
    s = rule_storage(DECOUPLED, seed=seed) if s is None else s
    value, next_value = values_for(s, seed)
    na = s.n_agents
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)
    return dict(reward=s.reward, done=s.done, value=torch.from_numpy(value), advantage=z(s.T, s.N, na), td_target=z(s.T, s.N, na),
                next_value=torch.from_numpy(next_value), truncated=s.truncated, term_obs=s.final_obs, rule=TimeLimitRule(), done_eff=z(s.T, s.N, na, dtype=torch.bool),
                stats=z(na, 3, dtype=torch.float64), normalized=z(s.T, s.N, na), workspace=z(gae_rule_workspace_numel(s.N, na), dtype=torch.float64))


def test_gae_rule_checks():
    good = _good()
    s = rule_storage(DECOUPLED, seed=4)
    bad = [dict(reward=good["reward"][..., 0]), dict(reward=good["reward"].double()), dict(reward=good["reward"].transpose(0, 1)),
           dict(done=good["done"][:2]), dict(done=good["done"].float()), dict(value=good["value"][:2]), dict(value=good["value"].double()),
           dict(value=good["value"][:3], next_value=None), dict(next_value=good["next_value"][:2]), dict(next_value=good["next_value"].double()),
           dict(advantage=good["advantage"][:2]), dict(td_target=good["td_target"].double()), dict(truncated=None), dict(term_obs=None),
           dict(truncated=good["truncated"][:2]), dict(truncated=good["truncated"].float()), dict(term_obs=s.final_obs[:1]),
           dict(term_obs=[s.final_obs[0][..., :2], s.final_obs[1]]), dict(term_obs=[s.final_obs[0], s.final_obs[1][:2]]),
           dict(term_obs=[s.final_obs[0].double(), s.final_obs[1]]), dict(rule=TimeLimitRule(0.0)), dict(rule=(1.0, NAN, 0.03)), dict(rule=(1.0, 0.03, -1.0)),
           dict(done_eff=good["done_eff"].float()), dict(done_eff=good["done_eff"][:2]), dict(stats=None), dict(stats=good["stats"].float()),
           dict(stats=good["stats"][:1]), dict(normalized=good["normalized"][:2]), dict(normalized=good["normalized"].double()),
           dict(workspace=good["workspace"][:3]), dict(workspace=good["workspace"].float()), dict(norm_eps=-1.0), dict(norm_eps=NAN), dict(norm_eps=INF)]
    for change in bad:
        with pytest.raises(ValueError):
            gae_rule(**dict(good, **change))
    one = fake_storage(*COUPLED, 1, 1)
    with pytest.raises(ValueError, match="two transitions"):
        gae_rule(**_good(one))
    with pytest.raises(ValueError, match="one or two agents"):
        gae_rule(**dict(good, reward=torch.zeros(3, 65, 3)))
    for ok in (good, dict(good, rule=None, truncated=None, term_obs=None), dict(good, value=good["value"][:3]), dict(good, rule=(2.0, 0.1, 0.2)),
               dict(good, done=good["done"].to(torch.uint8), done_eff=None, stats=None, normalized=None, workspace=None, next_value=None)):
        with pytest.raises(RuntimeError):            # all checks passed: there is no CPU kernel
            gae_rule(**ok)


def test_compute_gae_checks():
    s = rule_storage(DECOUPLED, seed=6)
    st = real_storage(s)
    assert st.env_x_lim == 1.5 and real_storage(s, x_lim=None).env_x_lim is None
    with pytest.raises(ValueError, match="time_limit"):
        st.compute_gae(time_limit="reference")
    with pytest.raises(ValueError, match="time_limit"):
        st.compute_gae(time_limit="solved ")
    for rule in (TimeLimitRule(0.0), TimeLimitRule(NAN), TimeLimitRule(1.0, -0.01), TimeLimitRule(1.0, 0.03, INF)):
        with pytest.raises(ValueError):
            st.compute_gae(time_limit="solved", rule=rule)
        with pytest.raises(ValueError):
            st.compute_gae(rule=rule)
    with pytest.raises(ValueError, match="next_value"):
        st.compute_gae(time_limit="solved", next_value=torch.zeros(T, N, 1))
    with pytest.raises(ValueError, match="next_value"):
        st.compute_gae(normalized=True, next_value=torch.zeros(T, N, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="last_value"):
        st.compute_gae(done_eff=True, last_value=torch.zeros(N))
    no_trunc = real_storage(s)
    no_trunc.truncated = None
    with pytest.raises(ValueError, match="time_limit='solved' needs the storage's truncated flags"):
        no_trunc.compute_gae(time_limit="solved")
    with pytest.raises(RuntimeError):                # "own" does not need them
        no_trunc.compute_gae(normalized=True)
    narrow = real_storage(fake_storage((2,), (4,), 3, 65))
    with pytest.raises(ValueError, match="three words"):
        narrow.compute_gae(time_limit="solved")
    tiny = real_storage(fake_storage(*COUPLED, 1, 1))
    with pytest.raises(ValueError, match="two transitions"):
        tiny.compute_gae(normalized=True)
    before = st.value.clone()
    for kw in (dict(time_limit="solved"), dict(normalized=True), dict(done_eff=True), dict(rule=TimeLimitRule(2.0)), dict(time_limit="solved", want_stats=False)):
        with pytest.raises(RuntimeError):            # all checks passed: there is no CPU kernel
            st.compute_gae(last_value=torch.ones(N, 2), **kw)
    assert torch.equal(st.value, before) and st.advantage_normalized is None and st.done_eff is None and st.gae_stats is None


def test_compute_gae_with_defaults_is_the_call_it_was(monkeypatch):
    """compute_gae() with its keyword-only arguments at their defaults makes the one qr_gae call it made and never touches qr_gae_rule:
    the storage's library handle and the module's are replaced by an object that has no such entry."""
    calls = []

    class OldLibrary:
        def qr_gae(self, *args):
            calls.append(args)
            return 0

    s = rule_storage(DECOUPLED, seed=7)
    st = real_storage(s)
    st._lib = OldLibrary()
    monkeypatch.setattr(L, "load", lambda: OldLibrary())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())   # (the stand-in launches nothing)
    assert not hasattr(OldLibrary(), "qr_gae_rule")
    nv = torch.zeros(T, N, 2)
    out = st.compute_gae(0.98, 0.8, last_value=torch.ones(N, 2), next_value=nv)
    assert len(out) == 3 and out[0] is st.advantage and out[1] is st.td_target and tuple(out[2].shape) == (2, 3)
    assert float(out[2][0, 2]) == T * N and torch.equal(st.value[T], torch.ones(N, 2))
    out = st.compute_gae(want_stats=False, time_limit="own", rule=None, normalized=False, done_eff=False)
    assert len(out) == 2 and len(calls) == 2
    a = calls[0]
    assert a[:4] == (st.reward.data_ptr(), st.done.data_ptr(), st.value.data_ptr(), nv.data_ptr()) and a[4:8] == (T, N * 2, 0.98, 0.8)
    assert a[8:10] == (st.advantage.data_ptr(), st.td_target.data_ptr()) and a[10] is not None and calls[1][3] is None and calls[1][10] is None
    assert st.advantage_normalized is None and st.done_eff is None and st.gae_stats is None


# ---------------------------------------------------------------- PpoCollector on the host
def test_collector_checks():
    env = _Env()
    good = dict(horizon=3)
    for change in (dict(time_limit="reference"), dict(horizon=0), dict(horizon=-3), dict(gamma=NAN), dict(gamma=-0.1), dict(lam=INF), dict(lam=-1.0),
                   dict(rule=TimeLimitRule(0.0)), dict(rule=(1.0, NAN, 0.03)), dict(rule=(1.0, 0.03, -0.5))):
        with pytest.raises(ValueError):
            PpoCollector(env, **dict(good, **change))
    with pytest.raises(ValueError, match="auto_reset"):
        PpoCollector(_Env(auto_reset=False), **good)
    with pytest.raises(TypeError):
        PpoCollector(env, 3, 0.99)                   # everything behind the horizon is keyword-only
    narrow = _Env("coupled")
    narrow.obs_dims = [2]
    with pytest.raises(ValueError, match="three words"):
        PpoCollector(narrow, **good)
    assert env.calls == []
    col = PpoCollector(env, **good)
    assert col.rule == TimeLimitRule(1.5, 0.03, 0.03) and col.time_limit == "solved" and (col.gamma, col.lam) == (0.99, 0.9)
    assert col.storage.T == 3 and col.storage.N == env.num_envs and col.storage.env_x_lim == 1.5 and col.episodes is None
    own = PpoCollector(_Env("coupled"), 5, gamma=0.95, lam=0.8, time_limit="own", rule=(2.0, 0.1, 0.2), track_episodes=True)
    assert own.rule == TimeLimitRule(2.0, 0.1, 0.2) and own.episodes is not None and own.episodes.rule == own.rule and own.episodes.N == 4
    assert PpoCollector(narrow, 3, time_limit="own").storage.obs[0].shape[-1] == 2
    env._last_obs = None
    with pytest.raises(ValueError, match="observation"):
        col.collect([None, None], [None, None])
    assert env.calls == []
