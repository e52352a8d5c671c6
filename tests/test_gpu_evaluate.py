"""Batched policy evaluation on the GPU (qr_evaluate_actor: eval_kernel): against the existing actor rollout and the reference's
accounting, freezing, success flags decided on purpose, the wave-uniform early exit, evaluate_policy end to end and the torch op."""
import math
import time

import numpy as np
import pytest
import torch

from test_evaluate_host import eval_accounting

pytestmark = pytest.mark.gpu

FRAMEWORK = {"coupled": "MONO", "decoupled": "MODUL"}


def _env(kind, n, **kw):
    from gym_rotor_amd import QuadVecEnv
    kw.setdefault("autotune", False)
    return QuadVecEnv(kind, n, device="cuda", **kw)


def _rows(env, x=None, v=None, yaw=None):
    """[N, 18] states (x, v, vec(R) column-major, W) at rest with identity attitude, optionally offset."""
    n = env.num_envs
    s = np.zeros((n, 18))
    s[:, 6:15] = np.eye(3).reshape(-1, order="F")
    if x is not None:
        s[:, 0:3] = x
    if v is not None:
        s[:, 3:6] = v
    if yaw is not None:
        c, sn = math.cos(yaw), math.sin(yaw)
        s[:, 6:15] = np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]]).reshape(-1, order="F")
    return s


def _start(env, mixed_fates=True):
    """Episode starts: reset('train'); then every third env doomed (x 0.9 m, v 3.9 m/s outwards: crosses |ex| = 1 within a few
    steps), every third at rest at the origin (survives a quiet actor), the rest as the reset drew them.  Generator start, first
    goal and first observation as eval_policy forms them (main.py:305-309)."""
    env.reset("train")
    if mixed_fates:
        cur = env.get_current_state().cpu().numpy()
        doomed, rest = _rows(env, x=(0.9, 0, 0), v=(3.9, 0, 0)), _rows(env)
        k = np.arange(env.num_envs) % 3
        cur[k == 0], cur[k == 1] = doomed[k == 0], rest[k == 1]
        env.set_state(cur, integ=np.zeros((env.num_envs, 8)))
    if env.goal_mode is not None:
        env.mark_traj_start()
        env.get_desired(store_goal=True)
    return [o.clone() for o in env.get_norm_error_state()]   # (the env's own row buffers: step() overwrites them)


def _quiet_actors(kind, seed):
    """Random actors of the reference's sizes whose means stay near 0 (thrust ~ 1.15 hover, small moments)."""
    from gym_rotor_amd import random_actors
    actors = random_actors(kind, "cuda", generator=torch.Generator("cuda").manual_seed(seed), log_std=-0.5)
    for a in actors:
        a.mean_w.mul_(0.1)
    return actors


def _np(t):
    return t.detach().cpu().numpy()


CASES = [(k, g, lay, s) for k in ("coupled", "decoupled") for g in (None, 0, 6) for lay in ("mixed", "f64", "f32") for s in (1, 4)]
# the generator's stateful modes (TRAJ == 2: the one path with evaluate-only code, the write-back at each lane's freeze)
CASES += [(k, g, lay, s) for k in ("coupled", "decoupled") for g, lay, s in ((2, "mixed", 1), (3, "mixed", 4), (4, "f64", 1), (5, "f64", 4))]


@pytest.mark.parametrize("kind,goal_mode,layout,substeps", CASES)
def test_evaluate_matches_the_actor_rollout(kind, goal_mode, layout, substeps):
    """From the same starts, rollout_actor(deterministic=True, T) with auto_reset off, reduced on the host by eval_policy's accounting
    (test_evaluate_host.eval_accounting), against evaluate(max_steps=T): length, terminated, success identical; returns and
    benchmark within 1e-6; final_error and the final rows equal to the rollout's row at each env's terminal step.  (w_adapt = 0:
    in the rollout an env flown on after its crash could otherwise push its whole wave into more substeps — evaluate never
    steps a finished env on.)"""
    T, n = 200, 300
    env = _env(kind, n, seed=5, layout=layout, substeps=substeps, goal_mode=goal_mode, w_adapt=0.0)
    obs = _start(env)
    sd = env.state_dict()
    actors = _quiet_actors(kind, 3)
    ro = env.rollout_actor(actors, T, deterministic=True)
    torch.cuda.synchronize()
    fw = FRAMEWORK[kind]
    want = eval_accounting(_np(ro["reward"]), _np(ro["terminated"]), _np(ro["obs0"]), _np(ro["obs1"]) if "obs1" in ro else None, fw, T)
    env.load_state_dict(sd)
    got = env.evaluate(actors, max_steps=T, obs=[o.clone() for o in obs])
    torch.cuda.synchronize()
    term, length = _np(got["terminated"]), _np(got["length"])
    assert term.any() and (~term).any(), "both early crashes and survivors of all T steps"
    assert (length == want["length"]).all() and (term == want["terminated"]).all()
    assert (_np(got["success"]) == want["success"]).all()
    for k in ("episode_return", "benchmark"):
        g, w = _np(got[k]), want[k]
        rel = np.abs(g - w) / np.maximum(np.abs(w), 1.0)
        print(f"{kind} goal {goal_mode} {layout} x{substeps}: {k} max rel {rel.max():.1e}, identical {np.array_equal(g, w)}")
        assert rel.max() <= 1e-6, k
    # (the default and float64 layouts: the rollout's bits.  The float32 layout has no non-adaptive actor rollout, and the compiler
    #  contracts some float32 products differently in the two kernels: the last bits of a row may differ)
    idx, last = np.arange(n), length - 1
    pairs = [(_np(got["final_error"]), want["final_error"]), (_np(got["obs0"]), _np(ro["obs0"])[last, idx]),
             (_np(got["action"]), _np(ro["action"])[last, idx])]
    if "obs1" in ro:
        pairs.append((_np(got["obs1"]), _np(ro["obs1"])[last, idx]))
    for g, w in pairs:
        if layout == "f32":
            assert np.abs(g.astype(np.float64) - w).max() <= 1e-5
        else:
            assert np.array_equal(g, w)
    assert env._last_obs[0] is got["obs0"] if isinstance(env._last_obs, tuple) else env._last_obs is got["obs0"]
    assert env._policy_steps == 0   # (evaluate does not advance rollout_actor's noise stream)


@pytest.mark.parametrize("kind,layout,substeps,goal_mode", [("coupled", "mixed", 1, None), ("decoupled", "mixed", 4, 1),
                                                             ("decoupled", "f64", 1, 0), ("coupled", "f32", 4, 6),
                                                             ("coupled", "mixed", 1, 3), ("decoupled", "f64", 4, 5),
                                                             ("coupled", "mixed", 4, 2), ("decoupled", "mixed", 1, 4)])
def test_evaluate_freezes_each_env_at_its_terminal_step(kind, layout, substeps, goal_mode):
    """After evaluate, each env's state is the state after `length` step() calls from the same start with the same actions (the
    rollout's action rows), and episode_steps has advanced by `length`."""
    T, n = 150, 300
    env = _env(kind, n, seed=9, layout=layout, substeps=substeps, goal_mode=goal_mode, w_adapt=0.0, max_episode_steps=10 ** 6)
    obs = _start(env)
    sd = env.state_dict()
    actors = _quiet_actors(kind, 4)
    acts = env.rollout_actor(actors, T, deterministic=True)["action"].clone()
    env.load_state_dict(sd)
    states = []
    for t in range(T):
        env.step(acts[t])
        states.append(env.get_current_state())
    states = torch.stack(states)
    env.load_state_dict(sd)
    steps0 = env.episode_steps.clone()
    got = env.evaluate(actors, max_steps=T, obs=[o.clone() for o in obs])
    cur = env.get_current_state()
    torch.cuda.synchronize()
    length = got["length"].long()
    assert (length < T).any() and (length == T).any()
    want = states[length - 1, torch.arange(n, device="cuda")]
    err = (cur - want).abs().max().item()
    print(f"{kind} {layout} x{substeps} goal {goal_mode}: frozen state vs step() max |d| {err:.1e}")
    assert err <= (2e-5 if layout == "f32" else 1e-6)
    assert torch.equal(env.episode_steps - steps0, got["length"])


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
def test_success_flags_decided_on_purpose(kind):
    """An actor with all weights zero and the mean bias that gives hover thrust (zero moments) at a hover goal: success for every agent
    after 1000 steps, not terminated.  Offset x by 0.02 m: success[0] = 0, still flying.  MODUL, yaw offset 0.02 rad: success[1] = 0,
    success[0] = 1."""
    from gym_rotor_amd import random_actors
    from gym_rotor_amd.constants import QuadConstants
    n = 128
    c = QuadConstants()
    hover = c.m_nominal * c.g / 4
    maxf = c.c_tw_nominal * hover
    avrg, scale = (c.min_force + maxf) / 2, maxf - (c.min_force + maxf) / 2
    actors = random_actors(kind, "cuda")
    for a in actors:
        for t in (a.fc1_w, a.fc1_b, a.fc2_w, a.fc2_b, a.mean_w, a.mean_b):
            t.zero_()
    actors[0].mean_b[0] = math.atanh((hover - avrg) / scale)
    env = _env(kind, n, use_UDM=False)

    def run(**off):
        env.set_state(_rows(env, **off), integ=np.zeros((n, 8)))
        return env.evaluate(actors, obs=env.get_norm_error_state())

    G = 2 if kind == "decoupled" else 1
    r = run()
    assert (_np(r["length"]) == 1000).all() and not _np(r["terminated"]).any()
    assert _np(r["success"]).all(), _np(r["final_error"])[:2]
    r = run(x=(0.02, 0, 0))
    assert not _np(r["terminated"]).any() and not _np(r["success"])[:, 0].any()
    if G == 2:
        assert _np(r["success"])[:, 1].all()
        r = run(yaw=0.02)
        assert not _np(r["terminated"]).any() and _np(r["success"])[:, 0].all() and not _np(r["success"])[:, 1].any()


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
def test_early_exit_when_every_env_has_crashed(kind):
    """Every env doomed: the launch ends with its longest-surviving env, also when asked for a million steps (the wave-uniform exit)."""
    n = 4096
    env = _env(kind, n, seed=2)
    env.set_state(_rows(env, x=(0.9, 0, 0), v=(3.9, 0, 0)), integ=np.zeros((n, 8)))
    actors = _quiet_actors(kind, 7)
    obs = env.get_norm_error_state()
    sd = env.state_dict()
    r = env.evaluate(actors, max_steps=1000, obs=[o.clone() for o in obs])
    torch.cuda.synchronize()
    assert _np(r["terminated"]).all() and _np(r["length"]).max() < 1000
    env.load_state_dict(sd)
    t0 = time.perf_counter()
    r2 = env.evaluate(actors, max_steps=10 ** 6, obs=[o.clone() for o in obs])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert dt < 2.0, dt
    assert torch.equal(r2["length"], r["length"]) and torch.equal(r2["episode_return"], r["episode_return"])


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
@pytest.mark.parametrize("mode", [0, 1])
def test_evaluate_policy_end_to_end(kind, mode):
    """eval_policy in one call over 4096 episodes: summary() agrees with the per-episode tensors, and a second run gives the same bits."""
    from gym_rotor_amd import evaluate_policy
    actors = _quiet_actors(kind, 1)
    a = evaluate_policy(kind, actors, 4096, traj_mode=mode)
    b = evaluate_policy(kind, actors, 4096, traj_mode=mode)
    for k in ("episode_return", "benchmark", "length", "terminated", "success", "final_error"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    s = a.summary()
    ret = _np(a.episode_return)
    assert s["episodes"] == 4096
    assert s["eval_reward"] == [round(float(ret[:, g].mean()), 4) for g in range(ret.shape[1])]
    assert s["benchmark_reward"] == round(float(_np(a.benchmark).mean()), 4)
    assert s["mean_length"] == pytest.approx(float(_np(a.length).mean()), rel=1e-12)
    assert s["terminated_fraction"] == pytest.approx(float(_np(a.terminated).mean()), rel=1e-12)
    assert s["success_rate"] == pytest.approx(_np(a.success).mean(0).tolist(), rel=1e-12)
    L = _np(a.length)
    term = _np(a.terminated)
    assert ((L >= 1) & (L <= 1000)).all() and (L[~term] == 1000).all() and term[L < 1000].all()
    print(f"evaluate_policy {kind} mode {mode}: {s}")


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
def test_torch_op_matches_evaluate(kind):
    """torch.ops.gym_rotor_amd.qr_evaluate_actor (torch_ops.evaluate) gives the bits of QuadVecEnv.evaluate, state included."""
    from gym_rotor_amd import torch_ops
    n, T = 500, 300
    env = _env(kind, n, seed=13, goal_mode=1)
    obs = _start(env)
    sd = env.state_dict()
    actors = _quiet_actors(kind, 5)
    want = env.evaluate(actors, max_steps=T, obs=[o.clone() for o in obs])
    s_want = env.get_current_state()
    env.load_state_dict(sd)
    out = {k: torch.empty_like(v) for k, v in want.items()}
    torch_ops.evaluate(env, actors, T, [o.clone() for o in obs], out)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(out[k], want[k]), k
    assert torch.equal(env.get_current_state(), s_want)
