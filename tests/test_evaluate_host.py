"""Batched policy evaluation (qr_evaluate_actor / QuadVecEnv.evaluate / gym_rotor_amd.evaluate) without a GPU: the accounting of the
reference's eval loop restated in NumPy and checked on its recorded flights, the C-ABI struct mirror, EvalResult.summary and the
argument checks that run before any launch."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# eval_policy's accounting (main.py:316-373, utils/utils.py:21-47), restated over batches of per-step rows
# ---------------------------------------------------------------------------------------------------------------------
def error_state(obs0, obs1, framework, x_lim=1.0):
    """get_error_state's ex, eb1 (utils/utils.py:21-38) from float32 observation rows [..., D]: float64, as NumPy forms them."""
    ex = obs0[..., 0:3].astype(np.float64) * x_lim
    eb1 = (obs1[..., 0] if framework == "MODUL" else obs0[..., 18]).astype(np.float64) * np.pi
    return ex, eb1


def benchmark_reward(ex, eb1):
    """benchmark_reward_func (utils/utils.py:42-47): interp(-|ex| - |eb1|, [-2, 0], [0, 1]), elementwise."""
    return np.interp(-np.linalg.norm(ex, axis=-1) + -np.abs(eb1), [-2.0, 0.0], [0.0, 1.0])


def eval_accounting(rewards, dones, obs0, obs1, framework, max_steps, x_lim=1.0):
    """Per-episode results of eval_policy from per-step rows of N episodes flown on past their end: rewards [T, N, G], dones
    [T, N, G], obs rows after each step [T, N, D] (T >= max_steps or the episode ends earlier).  Returns episode_return [N, G]
    (float64 sums through the terminal step), benchmark [N], length [N], terminated [N], success [N, G] (judged at the last
    step when length == max_steps; an early end: 0), final_error [N, 4]."""
    T, N, G = rewards.shape
    any_done = dones[:max_steps].any(-1)                            # [T', N]
    first = np.where(any_done.any(0), any_done.argmax(0), max_steps - 1)
    length = first + 1
    assert (length <= T).all(), "the rows end before some episode does"
    ex, eb1 = error_state(obs0[:max_steps], None if obs1 is None else obs1[:max_steps], framework, x_lim)
    bstep = benchmark_reward(ex, eb1)                                # [T', N]
    alive = np.arange(min(T, max_steps))[:, None] < length[None, :]   # steps through the terminal one
    ret = (rewards[:max_steps].astype(np.float64) * alive[..., None]).sum(0)
    bench = (bstep * alive).sum(0)
    idx = np.arange(N)
    exl, eb1l = ex[first, idx], eb1[first, idx]
    full = length == max_steps
    success = np.zeros((N, G), bool)
    success[:, 0] = full & (np.abs(exl) <= 0.01).all(-1)
    if G > 1:
        success[:, 1] = full & (np.abs(eb1l) <= 0.01)
    final_error = np.concatenate([exl, eb1l[:, None]], 1).astype(np.float32)
    return {"episode_return": ret, "benchmark": bench, "length": length.astype(np.int32), "terminated": any_done[first, idx],
            "success": success, "final_error": final_error}


def _loop_one(rewards, dones, obs0, obs1, framework, max_steps):
    """main.py:316-373 for ONE episode as the reference loops over it (scalar, step by step), without the 4-decimal rounding of the
    running reward (the launch sums in float64).  Returns (episode_reward, benchmark, timesteps, success or None)."""
    G = rewards.shape[-1]
    episode_reward, bench, success = [0.0] * G, 0.0, None
    for t in range(max_steps):
        ex, eb1 = error_state(obs0[t], None if obs1 is None else obs1[t], framework)
        episode_reward = [episode_reward[g] + float(rewards[t, g]) for g in range(G)]
        bench += float(np.interp(-np.linalg.norm(ex) + -abs(eb1), [-2.0, 0.0], [0.0, 1.0]))
        if dones[t].any() or t + 1 == max_steps:
            if t + 1 == max_steps:
                success = [bool((abs(ex) <= 0.01).all())] + ([bool(abs(eb1) <= 0.01)] if framework == "MODUL" else [])
            return episode_reward, bench, t + 1, success
    raise AssertionError("unreachable")


FLIGHTS = [("mono", "MONO", m) for m in (0, 1, 6)] + [("modul", "MODUL", m) for m in (0, 1, 6)]


def _flight(golden, fw, mode):
    g = golden(f"closedloop_td3_{fw}")
    p = f"m{mode}_"
    obs1 = g[p + "obs1"] if p + "obs1" in g else None
    return g[p + "rewards"], g[p + "dones"], g[p + "obs0"], obs1


@pytest.mark.parametrize("fw,framework,mode", FLIGHTS)
def test_accounting_on_the_reference_eval_flights(golden, fw, framework, mode):
    """The recorded flights of the shipped TD3 actor in the reference's own eval loop (modes 0 / 1 / 6: rewards, dones and observation
    rows per step).  A 1000-step evaluation (the whole flight where it is shorter) of each, as the restatement computes it, against the
    reference loop run step by step over the same rows; then the same flight cut short by a done planted at step 300 (first-done
    truncation, terminal step included, success 0) and judged over 40 steps (success decided at the last step)."""
    rewards, dones, obs0, obs1 = _flight(golden, fw, mode)
    assert not dones.any()  # (the shipped policy keeps every flight in the air)
    b = lambda a: None if a is None else a[:, None]
    cases = [(rewards, dones, min(1000, len(rewards))), (rewards, dones, 40)]
    cut = dones.copy()
    cut[300, -1] = 1
    cases.append((rewards, cut, min(1000, len(rewards))))
    for rw, dn, T in cases:
        got = eval_accounting(rw[:, None], dn[:, None], obs0[:, None], b(obs1), framework, T)
        ret, bench, length, success = _loop_one(rw, dn, obs0, obs1, framework, T)
        assert got["length"][0] == length and bool(got["terminated"][0]) == bool(dn[:T].any())
        np.testing.assert_allclose(got["episode_return"][0], ret, rtol=1e-12, atol=1e-9)
        assert abs(got["benchmark"][0] - bench) <= 1e-9 * max(1.0, bench)
        assert list(got["success"][0]) == (success if success is not None else [False] * rw.shape[1])
    # what the flights themselves give: 1000 steps of the shipped policy earn most of the benchmark's range
    full = eval_accounting(rewards[:, None], dones[:, None], obs0[:, None], b(obs1), framework, min(1000, len(rewards)))
    assert 0.5 * full["length"][0] < full["benchmark"][0] <= full["length"][0]


def test_accounting_edge_cases():
    """Terminal-step inclusion, the benchmark's clamp at -2 (interp's left end), ties at the 0.01 success boundary, and several
    episodes of different lengths side by side."""
    T, N = 6, 4
    rewards = np.full((T, N, 2), 0.5, np.float32)
    rewards[2, 1, 1] = -1.0                                # the crash override of agent 1 at the terminal step of env 1
    dones = np.zeros((T, N, 2), np.uint8)
    dones[2, 1, 1] = 1                                     # agent 1's done ends env 1 at step 3
    obs0 = np.zeros((T, N, 15), np.float32)
    obs1 = np.zeros((T, N, 3), np.float32)
    obs0[:, 2, 0:3] = 1.5                                  # |ex| = 2.6 > 2: benchmark 0 per step (clamp), never success
    obs0[:, 3, 0] = np.float32(0.01)                       # at the bar: float32(0.01) widened is 0.0099999998, inside
    obs1[:, 0, 0] = np.float32(0.01 / np.pi)
    got = eval_accounting(rewards, dones, obs0, obs1, "MODUL", T)
    assert list(got["length"]) == [6, 3, 6, 6] and list(got["terminated"]) == [False, True, False, False]
    np.testing.assert_allclose(got["episode_return"][1], [1.5, 0.0])      # 0.5 + 0.5 + (0.5 | -1.0): the terminal step counts
    assert got["benchmark"][2] == 0.0 and got["success"][2].tolist() == [False, True]
    assert got["success"][1].tolist() == [False, False]                   # ended early: 0 (the reference would re-append old flags)
    want_s0 = bool(np.float64(np.float32(0.01)) <= 0.01)
    assert got["success"][3].tolist() == [want_s0, True]
    e = float(np.float64(np.float32(0.01 / np.pi)) * np.pi)
    assert got["success"][0].tolist() == [True, e <= 0.01]
    np.testing.assert_allclose(got["benchmark"][0], T * (1 - e / 2), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# eval_policy in closed loop on the float64 oracle (the reference for tests/test_gpu_evaluate_oracle.py)
# ---------------------------------------------------------------------------------------------------------------------
def oracle_action(actors, obs, max_action=1.0):
    """The deterministic action of one actor per agent on the oracle: clip(mean, +-max_action) (PPO / TD3 form, ppo.py:100-101),
    tanh(mean) for an actor with a log_std head (SAC form, sac.py:104-105), rounded to float32 as the kernel's action is."""
    from oracle import actor_oracle as ao
    cols = [ao.sac_sample(p, o)[0] if "log_std_w" in p else ao.choose_action(p, o, None, max_action)[0] for p, o in zip(actors, obs)]
    return np.concatenate(cols, 1).astype(np.float32)


def eval_oracle(kind, state, params, max_steps, actors=None, actions=None, max_action=1.0, goal_mode=None, draws=(None, None, None),
                n_sub=1, perturb=None, fly_on=5, warm_calls=0):
    """eval_policy (main.py:270-404) for N envs from existing pieces only: traj_oracle forms the goal before every step, actor_oracle
    the deterministic action (`actors`: one dict of weights per agent; or `actions` [T, A]: recorded ones), quad_oracle.step_batch
    advances the env, eval_accounting reduces the rows.  Every env is flown `fly_on` steps past its own end (a decision tie with
    the GPU is judged on those rows) and then parked at rest, so the rows stay finite.  perturb=seed: the knife-edge probe —
    actions jittered by +-2e-7 relative after the float32 rounding, x and v rounded to float32 after every step.
    Returns eval_accounting's dict plus, per env AT ITS OWN TERMINAL STEP, state [N,18], integ [N,8], goal [N,12] and the
    generator dict `traj`; and `rows`: obs0[, obs1], action, reward, done of every step flown [T', N, .]."""
    from oracle import quad_oracle as orc
    from oracle import traj_oracle as trj
    fw = "MODUL" if kind == "decoupled" else "MONO"
    state = np.array(state, dtype=np.float64)
    n = len(state)
    rng = None if perturb is None else np.random.default_rng(perturb)
    tr, goal12 = None, np.tile(orc.DEFAULT_GOAL, (n, 1))

    def desired():
        xd, vd, b1d, _, Wd = trj.get_desired_batch(tr, state)
        return np.concatenate([xd, vd, b1d, Wd], 1)

    if goal_mode is not None:  # main.py:305-309: mark_traj_start, the first goal, the first observation
        tr = trj.traj_start_batch(state, goal_mode, theta_b1d=draws[0], t_traj=draws[1], w_b1d=draws[2])
        for _ in range(warm_calls):   # (the generator's clock run ahead with the env held at its start, to reach a late phase sooner)
            desired()
        goal12 = desired()
    first = orc.error_obs_batch(kind, state, goal12, np.zeros((n, 8)))
    obs, integ = first["obs"], first["integ"]
    rest = np.zeros(18)
    rest[6] = rest[10] = rest[14] = 1.0
    live, ended_at = np.ones(n, bool), np.full(n, max_steps)
    rows = {k: [] for k in ("obs0", "obs1", "action", "reward", "done")}
    end = {"state": np.zeros((n, 18)), "integ": np.zeros((n, 8)), "goal": np.zeros((n, 12)),
           "traj": None if tr is None else {k: np.array(v) for k, v in tr.items()}}
    for t in range(max_steps):
        if tr is not None:
            goal12 = desired()
        act = np.broadcast_to(actions[t], (n, len(actions[t]))) if actions is not None else oracle_action(actors, obs, max_action)
        act = np.asarray(act, np.float32).astype(np.float64)
        if rng is not None:
            act = act * (1.0 + rng.uniform(-2e-7, 2e-7, act.shape))
        out = orc.step_batch(kind, state, act, params, goal12, integ, n_sub=n_sub)
        state, integ, obs = out["state"], out["integ"], out["obs"]
        if rng is not None:
            state[:, 0:6] = state[:, 0:6].astype(np.float32)
        for k, v in (("obs0", obs[0]), ("obs1", obs[1] if len(obs) > 1 else None), ("action", act.astype(np.float32)),
                     ("reward", out["reward"]), ("done", out["done"])):
            if v is not None:
                rows[k].append(v)
        ending = live & (out["done"].any(1) | (t + 1 == max_steps))
        if ending.any():
            end["state"][ending], end["integ"][ending], end["goal"][ending] = state[ending], integ[ending], goal12[ending]
            if tr is not None:
                for k, v in tr.items():
                    if isinstance(v, np.ndarray) and v.shape[:1] == (n,):
                        end["traj"][k][ending] = v[ending]
            ended_at[ending] = t + 1
        live &= ~ending
        gone = t + 1 >= ended_at + fly_on
        state[gone], integ[gone] = rest, 0.0
        if not live.any() and t + 1 >= min(max_steps, ended_at.max() + fly_on):
            break
    rows = {k: np.stack(v) for k, v in rows.items() if v}
    res = eval_accounting(rows["reward"], rows["done"], rows["obs0"], rows.get("obs1"), fw, max_steps, x_lim=orc.X_LIM)
    assert (res["length"] == ended_at).all()
    res.update(end, rows=rows)
    return res


@pytest.mark.parametrize("fw,kind,mode", [("mono", "coupled", 1), ("modul", "decoupled", 6)])
def test_eval_oracle_on_the_reference_eval_flights(golden, fw, kind, mode):
    """The closed-loop helper with the RECORDED actions of the shipped TD3 actor in place of the actor, on one reference flight
    per wrapper: what it accounts equals eval_accounting of the reference's recorded rows — lengths and flags identical, returns
    within the 1e-6 per step and rows within the 2e-7 that test_oracle_replays_the_shipped_policy_flights allows, the frozen
    state within its 1e-9.  (The benchmark's step is 0.5 (2 - |ex| - |eb1|): at most 0.5 (sqrt 3 + pi) times the row bar.)
    Both flights last all T steps without a done (the shipped policy keeps flying), so the helper's bookkeeping of an EARLY end
    — the capture at the terminal step, the parking after fly_on — is not pinned to the reference here: it is checked by the
    helper's own assertion that eval_accounting finds the lengths it froze at."""
    g = golden(f"closedloop_td3_{fw}")
    p = f"m{mode}_"
    framework = fw.upper()
    T = min(1000, len(g[p + "actions"]))
    obs1 = g[p + "obs1"][:, None] if p + "obs1" in g else None
    want = eval_accounting(g[p + "rewards"][:, None], g[p + "dones"][:, None], g[p + "obs0"][:, None], obs1, framework, T)
    got = eval_oracle(kind, g[p + "init_state"][None], np.atleast_2d(g["params"]), T, actions=g[p + "actions"], goal_mode=mode,
                      draws=tuple(g[p + "draws"]))
    assert got["length"][0] == want["length"][0] == T and not got["terminated"][0] and not want["terminated"][0]
    assert (got["success"] == want["success"]).all()
    assert np.abs(got["episode_return"] - want["episode_return"]).max() <= 1e-6 * T
    assert abs(got["benchmark"][0] - want["benchmark"][0]) <= 0.5 * (np.sqrt(3) + np.pi) * 2e-7 * T
    assert np.abs(got["final_error"] - want["final_error"]).max() <= 2e-7 * np.pi
    assert np.abs(got["rows"]["obs0"][T - 1, 0].astype(np.float64) - g[p + "obs0"][T - 1]).max() <= 2e-7
    from conftest import grouped_rel_err
    assert grouped_rel_err(got["state"], g[p + "states"][T][None]) <= 1e-9
    assert got["traj"]["calls"][0] == T + 1


# ---------------------------------------------------------------------------------------------------------------------
# which eval kernels the build holds
# ---------------------------------------------------------------------------------------------------------------------
def test_the_build_holds_exactly_the_24_eval_kernels(tmp_path):
    """The eval_kernel<...> symbols of the built library's gfx950 code object (llvm-objdump --offloading, demangled names, as
    tools/codeobj_diff.py lists kernels): exactly the 24 instantiations that the table of tests/test_gpu_evaluate_oracle.py flies."""
    import re
    import shutil
    from test_gpu_evaluate_oracle import INSTANCES, TABLE, instance_of
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    objdump = shutil.which("llvm-objdump", path=os.pathsep.join([f"{rocm}/lib/llvm/bin", f"{rocm}/llvm/bin", os.environ.get("PATH", "")]))
    assert objdump, f"llvm-objdump not found under {rocm} or on PATH: the build's kernels cannot be listed"
    lib = os.environ.get("QR_LIB") or os.path.join(ROOT, "gym_rotor_amd", "libquadrotor_hip.so")
    shutil.copy(lib, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", "lib.so"], check=True, capture_output=True, cwd=tmp_path)
    co = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert co, "no gfx950 code object in the library"
    syms = subprocess.run([objdump, "--syms", "-C", str(tmp_path / co[0])], check=True, capture_output=True, text=True).stdout
    found = set(re.findall(r" F \.text\s+[0-9a-f]+\s+(?:\.protected )?(?:void )?qr::eval_kernel<([^>]*)>\(qr::EvalLaunch\)$", syms, re.M))
    types = {"mixed": "float, double", "f64": "double, double", "f32": "float, float"}
    name = lambda kind, layout, traj, mag: f"{ {'coupled': 1, 'decoupled': 2}[kind]}, {types[layout]}, {traj}, {'true' if mag else 'false'}"
    assert len(found) == 24, sorted(found)
    assert found == {name(*i) for i in INSTANCES}
    assert found == {name(*instance_of(*row[:4])) for row in TABLE}


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_qr_eval_out_mirrors_the_header(tmp_path):
    """QrEvalOut in gym_rotor_amd/_lib.py against include/quadrotor_hip.h, compiled: sizes and offsets."""
    from gym_rotor_amd import _lib as L
    fl = [f[0] for f in L.QrEvalOut._fields_]
    lines = ['printf("QrEvalOut %zu\\n", sizeof(QrEvalOut));'] + [f'printf("{f} %zu\\n", offsetof(QrEvalOut, {f}));' for f in fl]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["QrEvalOut"]) == C.sizeof(L.QrEvalOut)
    for f in fl:
        assert int(out[f]) == getattr(L.QrEvalOut, f).offset, f
    assert "qr_evaluate_actor" in L.SYMBOLS and L.ABI_VERSION == 16


def test_qr_evaluate_actor_argument_errors_without_gpu():
    """Every argument check of qr_evaluate_actor runs on the host before a launch (fake device addresses are never touched)."""
    from gym_rotor_amd import _lib as L
    lib = L.load()
    e, o, pol = L.QrEnv(), L.QrEvalOut(), L.QrPolicyRollout()
    lib.qr_default_coeffs(C.byref(e.coeffs))
    e.kind, e.num_envs, e.pos_vel, e.att_rate, e.integ = 0, 64, 0x1000, 0x2000, 0x3000
    assert lib.qr_evaluate_actor(C.byref(e), None, 10, 1, C.byref(o), None) == -1
    assert lib.qr_evaluate_actor(C.byref(e), C.byref(pol), 10, 1, C.byref(o), None) == -2        # Quad-v0 has no actor
    e.kind = 1
    assert lib.qr_evaluate_actor(C.byref(e), C.byref(pol), 0, 1, C.byref(o), None) == -3         # max_steps < 1
    assert lib.qr_evaluate_actor(C.byref(e), C.byref(pol), 10, 0, C.byref(o), None) == -3        # substeps < 1
    assert lib.qr_evaluate_actor(C.byref(e), C.byref(pol), 10, 1, C.byref(o), None) == -1        # no actors / obs / outputs
    w = [0x10000 + 0x100 * k for k in range(7)]
    actor = L.QrActor(*w, None, None, 23, 16, 4, 0)
    arr = (L.QrActor * 1)(actor)
    pol.actors, pol.obs0_in, pol.max_action = arr, 0x5000, 1.0
    o.episode_return, o.benchmark, o.length, o.terminated, o.success, o.obs0 = 0x6000, 0x7000, 0x8000, 0x9000, 0xA000, 0xB000
    arr[0].hidden_dim = 32
    assert lib.qr_evaluate_actor(C.byref(e), C.byref(pol), 10, 1, C.byref(o), None) == -3        # actor sizes (fill_actor)
    arr[0].hidden_dim = 16
    o.success = None
    assert lib.qr_evaluate_actor(C.byref(e), C.byref(pol), 10, 1, C.byref(o), None) == -1
    e.num_envs = 0
    o.success = 0xA000
    assert lib.qr_evaluate_actor(C.byref(e), C.byref(pol), 10, 1, C.byref(o), None) == 0         # empty batch: nothing to launch
    e.kind, e.num_envs = 2, 64
    assert lib.qr_evaluate_actor(C.byref(e), C.byref(pol), 10, 1, C.byref(o), None) == -1        # MODUL needs obs1 rows in and out


def _bare_env(kind, obs_rows=True, n=8):
    """A QuadVecEnv shell with the attributes the host-side checks read (no GPU: the constructor would refuse)."""
    from gym_rotor_amd import QuadVecEnv
    from gym_rotor_amd.constants import ACTION_DIM, N_AGENTS, OBS_DIMS
    env = QuadVecEnv.__new__(QuadVecEnv)
    env.kind, env.obs_rows, env.num_envs, env.device = kind, obs_rows, n, torch.device("cpu")
    env.obs_dims, env.action_dim, env.n_agents, env.dt = OBS_DIMS[kind], ACTION_DIM[kind], N_AGENTS[kind], 1 / 200
    env._last_obs = None
    return env


def test_evaluate_argument_errors_raise_before_any_launch():
    """QuadVecEnv.evaluate applies rollout_actor's checks (wrappers only, obs_rows, actor sizes) and its own (max_steps >= 1) in
    Python: none of these reaches the library (the shell has no device buffers at all)."""
    from gym_rotor_amd import evaluate_policy, random_actors
    from gym_rotor_amd.policy import ActorParams
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="coupled"):
        _bare_env("quad").evaluate([])
    with pytest.raises(ValueError, match="coupled"):
        evaluate_policy("quad", [], 16)
    with pytest.raises(ValueError, match="obs_rows"):
        _bare_env("coupled", obs_rows=False).evaluate(random_actors("coupled", cpu))
    with pytest.raises(ValueError, match="max_steps"):
        _bare_env("coupled").evaluate(random_actors("coupled", cpu), max_steps=0)
    with pytest.raises(ValueError, match="actor sizes"):
        _bare_env("coupled").evaluate([ActorParams.random(23, 32, 4, cpu)])
    with pytest.raises(ValueError, match="2 actor"):
        _bare_env("decoupled").evaluate(random_actors("coupled", cpu))
    with pytest.raises(ValueError, match="no current observation"):
        _bare_env("decoupled").evaluate(random_actors("decoupled", cpu))


# ---------------------------------------------------------------------------------------------------------------------
# EvalResult.summary
# ---------------------------------------------------------------------------------------------------------------------
def _result(n, g, seed):
    from gym_rotor_amd import EvalResult
    r = np.random.default_rng(seed)
    length = r.integers(1, 1001, n).astype(np.int32)
    return EvalResult(torch.from_numpy(r.uniform(-50, 900, (n, g))), torch.from_numpy(r.uniform(0, 1000, n)), torch.from_numpy(length),
                      torch.from_numpy(length < 1000), torch.from_numpy((length == 1000)[:, None] & (r.random((n, g)) < 0.5)))


def test_summary_on_cpu_tensors():
    res = _result(1000, 2, 3)
    s = res.summary()
    ret, bench = res.episode_return.numpy(), res.benchmark.numpy()
    assert s["eval_reward"] == [round(float(ret[:, k].mean()), 4) for k in range(2)]
    assert s["benchmark_reward"] == round(float(bench.mean()), 4)
    assert all(x == round(x, 4) for x in s["eval_reward"] + [s["benchmark_reward"]])
    assert s["success_rate"] == pytest.approx(res.success.double().mean(0).tolist(), abs=1e-15)
    assert s["mean_length"] == pytest.approx(float(res.length.double().mean()), rel=1e-15)
    assert s["terminated_fraction"] == pytest.approx(float(res.terminated.double().mean()), rel=1e-15) and s["episodes"] == 1000
    assert 0.0 < s["terminated_fraction"] < 1.0


_GLOO_EVAL = textwrap.dedent("""
    import os, sys, torch, torch.distributed as dist
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    from test_evaluate_host import _result
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    full = _result(1001, 2, 11)
    cut = 501
    sl = slice(0, cut) if rank == 0 else slice(cut, 1001)
    from gym_rotor_amd import EvalResult
    part = EvalResult(full.episode_return[sl], full.benchmark[sl], full.length[sl], full.terminated[sl], full.success[sl])
    got = part.summary()
    dist.barrier(); dist.destroy_process_group()
    want = full.summary()
    assert got["episodes"] == 1001 and got["eval_reward"] == want["eval_reward"] and got["benchmark_reward"] == want["benchmark_reward"], (got, want)
    for k in ("success_rate", "mean_length", "terminated_fraction"):
        assert abs(torch.tensor(got[k], dtype=torch.float64) - torch.tensor(want[k], dtype=torch.float64)).max() < 1e-12, k
    print("ok", rank)
""")


def test_summary_all_reduces_over_gloo(tmp_path):
    """World size 2 over gloo: each rank summarises its shard of 1001 episodes and gets the figures of all of them."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    script = tmp_path / "w.py"
    script.write_text(_GLOO_EVAL.format(root=ROOT, tests=os.path.join(ROOT, "tests"), port=port))
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p in procs:
        out, err = p.communicate(timeout=180)
        assert p.returncode == 0, err
        assert "ok" in out
