"""The time-limit "solved" done rule (qr_replay_add_rule; td3.ReplayBuffer.add / append with time_limit=, td3.replay_add with
time_limit_rule=) and `OffPolicyCollector` without a GPU: the literal restatement of tests/replay_rule_ref.py against `add` on CPU
tensors with the hand-made rows, the new struct's layout, every error code of the new entry, every ValueError of the Python side before
a launch, and the collector's host logic (warm-up, exploration-std schedule) over a stand-in env."""
import ctypes as C
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_ref as R  # noqa: E402
import replay_rule_ref as RR  # noqa: E402
from test_replay_host import COUPLED, DECOUPLED, _fake_add, _set, fake_storage  # noqa: E402

from gym_rotor_amd import _lib as L  # noqa: E402
from gym_rotor_amd.offpolicy import OffPolicyCollector  # noqa: E402
from gym_rotor_amd.policy import ActorParams  # noqa: E402
from gym_rotor_amd.td3 import ReplayBuffer, TimeLimitRule, replay_add  # noqa: E402

T, N = 3, 65


def rule_storage(dims, T=T, N=N, device="cpu", final_obs=True, seed=0):
    """fake_storage with the hand-made rows planted; besides them, the first three words of every seventh env's terminal observation
    are scaled into the tolerance's neighbourhood, so that random time-limit rows fall on both sides of it."""
    s = fake_storage(*dims, T, N, device=device, final_obs=final_obs, seed=seed)
    for src in ([s.obs[0][1:]] if s.final_obs is None else [s.final_obs[0]]):
        src[:, ::7, :3] *= 0.02
    if s.n_agents == 2:
        (s.obs[1][1:] if s.final_obs is None else s.final_obs[1])[:, ::7, 0] *= 0.01
    RR.plant(s, RR.places(T, N))
    return s


def _numpy(s):
    return ([o.cpu().numpy() for o in s.obs], None if s.final_obs is None else [f.cpu().numpy() for f in s.final_obs], s.act_all.cpu().numpy(),
            s.reward.cpu().numpy(), s.done.cpu().numpy(), s.truncated.cpu().numpy())


# ---------------------------------------------------------------- the rule's restatement against ReplayBuffer.add (CPU tensors)
def test_hand_made_values():
    assert float(np.float64(RR.F03)) <= 0.03 < float(np.float64(RR.F03_UP))
    assert abs(np.float64(RR.B1_DOWN) * np.pi) <= 0.03 < abs(np.float64(RR.B1_UP) * np.pi)
    assert np.float32(-1.0) == -1.0 and np.float32(0.031) > 0.03


@pytest.mark.parametrize("dims,final", [(COUPLED, True), (DECOUPLED, True), (DECOUPLED, False), (COUPLED, False)])
def test_add_solved_is_the_restatement(dims, final):
    cap = 200
    s = rule_storage(dims, final_obs=final, seed=3)
    buf = ReplayBuffer(cap, *dims, "cpu")
    for t in buf.obs + buf.obs_next + buf.act + buf.rwd + buf.done:
        t.fill_(-7.0)
    buf.count, buf.current_size = 190, 190   # the horizon wraps
    ref = [{k: v.numpy().copy() for k, v in buf.tensors(a).items()} for a in range(buf.n_agents)]
    buf.add(s, time_limit="solved")
    nxt = RR.append(ref, 190, *_numpy(s))
    assert nxt == buf.count == (190 + T * N) % cap and buf.current_size == cap
    for a in range(buf.n_agents):
        for name, got in buf.tensors(a).items():
            assert np.array_equal(got.numpy().view(np.uint32), ref[a][name].view(np.uint32)), (a, name)
    untouched = np.setdiff1d(np.arange(cap), (190 + np.arange(T * N)) % cap)
    assert (buf.done[0][untouched] == -7.0).all()
    # the planted rows hold what the cases say, written out
    for (t, n), want in RR.expected(RR.places(T, N), buf.n_agents).items():
        row = (190 + t * N + n) % cap
        assert tuple(float(buf.done[a][row]) for a in range(buf.n_agents)) == tuple(want), (t, n, RR.places(T, N)[(t, n)])
    # and the rule is not the own flag: both kinds of difference occur
    own = s.done.reshape(T * N, -1).numpy().astype(np.float32)
    stored = RR.stored_done(*[_numpy(s)[i] for i in (0, 1, 3, 4, 5)]).reshape(T * N, -1)
    assert ((stored == 1) & (own == 0)).any() and ((stored == 0) & (own == 1)).any()
    lim = s.truncated.reshape(-1).numpy()
    assert np.array_equal(stored[~lim], own[~lim]) and 5 < int((stored[lim] == 1).sum()) < int(lim.sum())


def test_rule_numbers_are_used():
    """x_lim scales ex, and the two tolerances are separate numbers."""
    s = rule_storage(DECOUPLED, seed=4)
    args = [_numpy(s)[i] for i in (0, 1, 3, 4, 5)]
    base = RR.stored_done(*args)
    for rule in (TimeLimitRule(2.0, 0.03, 0.03), TimeLimitRule(1.0, 0.1, 0.03), TimeLimitRule(1.0, 0.03, 0.001)):
        buf = ReplayBuffer(200, *DECOUPLED, "cpu")
        buf.time_limit_rule = rule
        buf.add(s, time_limit="solved")
        want = RR.stored_done(*args, *rule).reshape(T * N, -1)
        assert not np.array_equal(want, base.reshape(T * N, -1)), rule
        for a in range(2):
            assert np.array_equal(buf.done[a][:T * N].numpy(), want[:, a]), (rule, a)


@pytest.mark.parametrize("dims,final", [(COUPLED, True), (DECOUPLED, True), (DECOUPLED, False)])
def test_own_is_todays_add(dims, final):
    s = rule_storage(dims, final_obs=final, seed=5)
    bufs = [ReplayBuffer(200, *dims, "cpu") for _ in range(2)]
    for b in bufs:
        b.count = b.current_size = 190
    ref = [{k: v.numpy().copy() for k, v in bufs[0].tensors(a).items()} for a in range(bufs[0].n_agents)]
    bufs[0].add(s)
    bufs[1].add(s, time_limit="own")
    R.append(ref, 190, *_numpy(s))   # the append rule as it was: the agent's own flag
    for a in range(bufs[0].n_agents):
        for name, t in bufs[0].tensors(a).items():
            assert torch.equal(t, bufs[1].tensors(a)[name]) and np.array_equal(t.numpy().view(np.uint32), ref[a][name].view(np.uint32)), (a, name)
    assert (bufs[0].count, bufs[0].current_size) == (bufs[1].count, bufs[1].current_size)


# ---------------------------------------------------------------- the struct and the C entry's errors
def test_struct_mirrors_the_header(tmp_path):
    lines = ['printf("abi %d\\n", QR_ABI_VERSION);', 'printf("QrReplayAddRule %zu\\n", sizeof(QrReplayAddRule));',
             'printf("QrReplayAdd %zu\\n", sizeof(QrReplayAdd));']
    lines += [f'printf("QrReplayAddRule.{f} %zu\\n", offsetof(QrReplayAddRule, {f}));' for f, _ in L.QrReplayAddRule._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["QrReplayAddRule"]) == C.sizeof(L.QrReplayAddRule) == C.sizeof(L.QrReplayAdd) + 24
    assert int(out["QrReplayAdd"]) == C.sizeof(L.QrReplayAdd)
    for f, _ in L.QrReplayAddRule._fields_:
        assert int(out[f"QrReplayAddRule.{f}"]) == getattr(L.QrReplayAddRule, f).offset, f
    lib = L.load()
    assert "qr_replay_add_rule" in L.SYMBOLS and hasattr(lib, "qr_replay_add_rule")
    assert int(out["abi"]) == L.ABI_VERSION == 16 and lib.qr_abi_version() == 16   # a struct and an entry were added: the version stays


NULL, SIZE, ALIGN = -1, -3, -4
INF, NAN = float("inf"), float("nan")


def _fake_rule(na=2):
    """A QrReplayAddRule over test_replay_host's made-up addresses that passes every check but for what a case changes."""
    return L.QrReplayAddRule(_fake_add(na), 1.0, 0.03, 0.03)


ADD_CASES = [
    ("n_agents", 0, None, SIZE), ("n_agents", 3, None, SIZE), ("reserved0", 1, None, SIZE), ("capacity", 0, None, SIZE), ("n_steps", 0, None, SIZE),
    ("n_envs", 0, None, SIZE), ("capacity", 194, None, SIZE), ("count", 200, None, SIZE), ("count", -1, None, SIZE), ("obs_dim", 0, 1, SIZE),
    ("obs_dim", 4097, 0, SIZE), ("action_dim", 0, 0, SIZE), ("col_offset", 5, 1, SIZE), ("col_offset", -1, 0, SIZE), ("action_row", 4, None, SIZE),
    ("action", None, None, NULL), ("reward", None, None, NULL), ("done", None, None, NULL), ("obs", None, 1, NULL), ("buf_obs", None, 0, NULL),
    ("buf_obs_next", None, 1, NULL), ("buf_action", None, 0, NULL), ("buf_reward", None, 1, NULL), ("buf_done", None, 0, NULL),
    ("final_obs", None, 1, NULL), ("obs", 0x10002, 0, ALIGN), ("buf_done", 0x20001, 1, ALIGN), ("reward", 0x30002, None, ALIGN),
    ("state", 0x40004, None, ALIGN),
    # the rule's own
    ("truncated", None, None, NULL), ("obs_dim", 2, 0, SIZE)]


@pytest.mark.parametrize("name,value,k,want", ADD_CASES)
def test_replay_add_rule_errors_of_the_append(name, value, k, want):
    lib = L.load()
    r = _fake_rule()
    if (name, value) == ("capacity", 194):
        r.add.count = 0
    _set(r.add, name, value, k)
    assert lib.qr_replay_add_rule(C.byref(r), None) == want
    assert lib.qr_replay_add_rule(None, None) == NULL


@pytest.mark.parametrize("name,value", [("pos_tol", -1e-9), ("pos_tol", NAN), ("pos_tol", INF), ("rot_tol", -0.03), ("rot_tol", NAN), ("rot_tol", INF),
                                        ("x_lim", 0.0), ("x_lim", -1.0), ("x_lim", NAN), ("x_lim", INF)])
def test_replay_add_rule_errors_of_the_numbers(name, value):
    lib = L.load()
    r = _fake_rule()
    setattr(r, name, value)
    assert lib.qr_replay_add_rule(C.byref(r), None) == SIZE
    r.add.truncated = None          # sizes are reported before pointers, as in qr_replay_add
    assert lib.qr_replay_add_rule(C.byref(r), None) == SIZE
    r = _fake_rule(1)               # one agent: agent 1's members are not read
    setattr(r, name, value)
    assert lib.qr_replay_add_rule(C.byref(r), None) == SIZE


def test_replay_add_rule_error_order():
    lib = L.load()
    r = _fake_rule()
    r.add.truncated, r.add.obs[0] = None, 0x10002
    assert lib.qr_replay_add_rule(C.byref(r), None) == NULL    # pointers before alignment
    r = _fake_rule()
    r.pos_tol = r.rot_tol = 0.0                                 # zero tolerances are allowed; the plain entry does not need truncated
    r.add.obs[0] = 0x10002
    assert lib.qr_replay_add_rule(C.byref(r), None) == ALIGN
    a = _fake_add()
    a.truncated = None
    a.obs[0] = 0x10002
    assert lib.qr_replay_add(C.byref(a), None) == ALIGN


# ---------------------------------------------------------------- the Python side's checks, all before a launch
def test_append_solved_checks():
    s = fake_storage(*DECOUPLED, 3, 65)
    buf = ReplayBuffer(200, *DECOUPLED, "cpu")
    for method in (buf.append, buf.add):
        with pytest.raises(ValueError):
            method(s, time_limit="reference")                          # not a rule
        with pytest.raises(ValueError):
            method(s, "solved ")
    no_trunc = fake_storage(*DECOUPLED, 3, 65)
    no_trunc.truncated = None
    for method in (buf.append, buf.add):
        with pytest.raises(ValueError, match="truncated"):
            method(no_trunc, time_limit="solved")
    no_trunc.reset_mask = lambda: no_trunc.done.any(-1)
    buf.add(no_trunc)                                                   # "own" does not need it
    assert buf.count == 195
    buf.count = buf.current_size = 0
    for bad in (ReplayBuffer(194, *DECOUPLED, "cpu"), ReplayBuffer(200, *COUPLED, "cpu"), ReplayBuffer(200, (15, 4), (4, 1), "cpu")):
        with pytest.raises(ValueError):
            bad.append(s, time_limit="solved")
    narrow = ReplayBuffer(200, (2,), (4,), "cpu")                      # ex is three words
    with pytest.raises(ValueError):
        narrow.append(fake_storage((2,), (4,), 3, 65), time_limit="solved")
    for rule in (TimeLimitRule(0.0), TimeLimitRule(-1.0), TimeLimitRule(INF), TimeLimitRule(NAN), TimeLimitRule(1.0, -0.01), TimeLimitRule(1.0, NAN),
                 TimeLimitRule(1.0, 0.03, -1.0), TimeLimitRule(1.0, 0.03, INF)):
        buf.time_limit_rule = rule
        for method in (buf.append, buf.add):
            with pytest.raises(ValueError):
                method(s, time_limit="solved")
    buf.time_limit_rule = TimeLimitRule()
    with pytest.raises(RuntimeError):                                   # all checks passed: there is no CPU kernel
        buf.append(s, time_limit="solved")
    assert (buf.count, buf.current_size) == (0, 0)
    t = [buf.tensors(k) for k in range(2)]
    good = dict(tensors=t, obs=s.obs, final_obs=s.final_obs, action=s.act_all, reward=s.reward, done=s.done, truncated=s.truncated, count=0,
                time_limit_rule=TimeLimitRule())
    for change in (dict(truncated=None), dict(time_limit_rule=TimeLimitRule(0.0)), dict(time_limit_rule=(1.0, 0.03, NAN)), dict(count=200),
                   dict(time_limit_rule=(1.0, -0.03)), dict(reward=s.reward[..., 0])):
        with pytest.raises(ValueError):
            replay_add(**dict(good, **change))
    with pytest.raises(RuntimeError):
        replay_add(**good)
    with pytest.raises(RuntimeError):
        replay_add(**dict(good, time_limit_rule=(2.0, 0.1, 0.2)))      # a plain tuple of the three numbers will do


# ---------------------------------------------------------------- OffPolicyCollector on the host
class _Env:
    """What OffPolicyCollector and RolloutStorage read of a QuadVecEnv, with launches that record their arguments and write nothing."""

    def __init__(self, kind="decoupled", num_envs=4, auto_reset=True):
        dims = DECOUPLED if kind == "decoupled" else COUPLED
        self.kind, self.num_envs, self.auto_reset, self.obs_rows = kind, num_envs, auto_reset, True
        self.n_agents, self.obs_dims, self.action_dim = len(dims[0]), list(dims[0]), sum(dims[1])
        self.device, self.x_lim = torch.device("cpu"), 1.5
        self._last_obs = tuple(torch.zeros(num_envs, d) for d in dims[0]) if len(dims[0]) > 1 else torch.zeros(num_envs, dims[0][0])
        self.calls = []

    def rollout(self, actions, out=None):
        self.calls.append(("rollout", actions.clone(), out))
        return out

    def rollout_actor(self, actors, n_steps, obs=None, out=None, **kw):
        self.calls.append(("rollout_actor", [None if a.log_std is None else a.log_std.clone() for a in actors], out, kw))
        return out


class _CpuBuffer(ReplayBuffer):
    """`append` through the torch twin: there is no CPU kernel."""

    def append(self, storage, time_limit="own"):
        self.appended = getattr(self, "appended", []) + [time_limit]
        self.add(storage, time_limit=time_limit)


def _actors(algo="td3"):
    g = torch.Generator().manual_seed(0)
    actors = [ActorParams.random(15, 16, 4, "cpu", g), ActorParams.random(3, 4, 1, "cpu", g)]
    if algo == "sac":
        for a in actors:
            a.log_std_w, a.log_std_b = torch.zeros(a.mean_w.shape), torch.zeros(a.mean_b.shape)
            a.log_std, a.squash = None, L.ACTOR_TANH_SAMPLE
    return actors


def test_collector_checks():
    env, buf = _Env(), ReplayBuffer(100, *DECOUPLED, "cpu")
    good = dict(horizon=3, start_timesteps=6, algo="td3", explor_noise_std_init=0.3, explor_noise_std_min=0.05, decay_timesteps=100)
    bad = [dict(algo="ppo"), dict(algo="TD3"), dict(horizon=0), dict(horizon=-3), dict(start_timesteps=-1), dict(decay_timesteps=0),
           dict(decay_timesteps=-5), dict(explor_noise_std_min=0.4), dict(explor_noise_std_min=0.0), dict(explor_noise_std_min=-0.1),
           dict(explor_noise_std_init=INF), dict(explor_noise_std_init=NAN), dict(time_limit="reference"), dict(horizon=26)]
    for change in bad:
        with pytest.raises(ValueError):
            OffPolicyCollector(env, buf, **dict(good, **change))
    with pytest.raises(ValueError, match="auto_reset"):
        OffPolicyCollector(_Env(auto_reset=False), buf, **good)
    with pytest.raises(ValueError):
        OffPolicyCollector(_Env("coupled"), buf, **good)                # agent count
    with pytest.raises(ValueError):
        OffPolicyCollector(env, ReplayBuffer(100, (15, 4), (4, 1), "cpu"), **good)
    with pytest.raises(ValueError):
        OffPolicyCollector(env, ReplayBuffer(100, (15, 3), (4, 2), "cpu"), **good)
    with pytest.raises(ValueError):
        OffPolicyCollector(env, [buf], **good)
    assert env.calls == [] and buf.time_limit_rule == TimeLimitRule()   # a refused constructor touched nothing
    col = OffPolicyCollector(env, buf, **good)
    assert buf.time_limit_rule == TimeLimitRule(1.5, 0.03, 0.03) and col.total_timesteps == 0 and col.storage.T == 3
    for actors in (_actors()[:1], _actors("sac"), [_actors()[0], _actors("sac")[1]]):
        with pytest.raises(ValueError):
            col.collect(actors)
    sac = OffPolicyCollector(env, ReplayBuffer(100, *DECOUPLED, "cpu"), 3, algo="sac", time_limit="own")
    assert sac.buffer.time_limit_rule == TimeLimitRule() and sac.random_actions is None
    with pytest.raises(ValueError):
        sac.collect(_actors("td3"))
    env._last_obs = None
    with pytest.raises(ValueError, match="observation"):
        col.collect(_actors())
    assert env.calls == [] and col.total_timesteps == 0 and buf.count == 0


def test_collector_warm_up_schedule_and_append():
    """Warm-up horizons fly uniform actions in [-1, 1) through the given-actions rollout and store them; afterwards the actors' log_std
    hold log(std) of the reference's recurrence (main.py:74-77, 237-239) iterated once per env-step, read at each horizon's first step."""
    T, init, low, steps = 3, 0.3, 0.05, 20           # the decay per step is 0.0125: the floor is reached inside the run
    env, buf = _Env(), _CpuBuffer(1000, *DECOUPLED, "cpu")
    col = OffPolicyCollector(env, buf, horizon=T, start_timesteps=5, algo="td3", explor_noise_std_init=init, explor_noise_std_min=low,
                             decay_timesteps=steps, time_limit="solved", generator=torch.Generator().manual_seed(1))
    actors = _actors()
    want, std, decay = [], init, (init - low) / steps
    for step in range(12 * T):                        # the reference's loop, step by step
        if step % T == 0:
            want.append(std)
        std = std - decay if std > low else low
    for call in range(12):
        assert col.explor_noise_std == want[call] and col.total_timesteps == call * T
        assert col.collect(actors) is col.storage
        kind = env.calls[-1][0]
        if call * T < 5:                              # total_timesteps 0 and 3
            assert kind == "rollout"
            a = env.calls[-1][1]
            assert a.shape == (T, 4, 5) and float(a.min()) >= -1.0 and float(a.max()) < 1.0 and a.std() > 0.3
            assert torch.equal(col.storage.act_all, a) and env.calls[-1][2]["obs0"].data_ptr() == col.storage.obs[0][1:].data_ptr()
        else:
            assert kind == "rollout_actor"
            for ls in env.calls[-1][1]:
                assert torch.equal(ls, torch.full_like(ls, math.log(want[call])))
    assert [c[0] for c in env.calls] == ["rollout"] * 2 + ["rollout_actor"] * 10
    assert want[0] == init and want[-1] == low and low < want[5] < init and col.explor_noise_std == low
    assert not torch.equal(env.calls[0][1], env.calls[1][1])
    assert buf.appended == ["solved"] * 12 and buf.count == 12 * T * 4 and col.total_timesteps == 36
    # no decay: the std stays; SAC-form actors are flown as they are
    env2, buf2 = _Env(), _CpuBuffer(1000, *DECOUPLED, "cpu")
    keep = OffPolicyCollector(env2, buf2, horizon=T, algo="td3", explor_noise_std_init=0.2, explor_noise_std_min=0.05, time_limit="own")
    for _ in range(3):
        keep.collect(actors)
    assert keep.explor_noise_std == 0.2 and torch.equal(actors[0].log_std, torch.full((4,), math.log(0.2))) and buf2.appended == ["own"] * 3
    sac = OffPolicyCollector(env2, buf2, horizon=T, algo="sac")
    sac.collect(_actors("sac"))
    assert env2.calls[-1][0] == "rollout_actor" and env2.calls[-1][1] == [None, None] and buf2.appended[-1] == "solved"


def test_decay_is_the_references_line():
    d = OffPolicyCollector.decay
    assert d(0.3, 0.1, 0.05) == 0.3 - 0.1 and d(0.05, 0.1, 0.05) == 0.05 and d(0.04, 0.1, 0.05) == 0.05
    assert d(0.06, 0.1, 0.05) == 0.06 - 0.1          # the reference's line undershoots once before it holds the floor
    assert d(0.06, 0.1, 0.05, steps=2) == 0.05 and d(0.3, 0.0, 0.05, steps=7) == 0.3
