"""Batched policy evaluation (qr_evaluate_actor: eval_kernel) against the float64 oracle in closed loop — goal oracle, actor oracle,
step oracle and the reference's accounting (test_evaluate_host.eval_oracle) — in every one of its 24 instantiations, the stateful
generator's write-back at each env's own terminal step, the flight continued by the next launch, and the edges of the launch."""
import math

import numpy as np
import pytest
import torch

from conftest import GROUPS, grouped_rel_err
from oracle import quad_oracle as orc
from test_evaluate_host import eval_oracle

pytestmark = pytest.mark.gpu

KINDS = ("coupled", "decoupled")


# ---------------------------------------------------------------------------------------------------------------------
# the table: which instantiation a case launches, by the launcher's rule restated (launch_eval_kind in qr_launch.h)
# ---------------------------------------------------------------------------------------------------------------------
def instance_of(kind, layout, substeps, goal_mode):
    """(kind, layout, TRAJ, MAG): TRAJ 0 without a goal mode, 1 for the stateless modes 0 / 1 / 6, 2 for the stateful 2-5; Magnus
    substeps for two or more substeps in the default layout only."""
    traj = 0 if goal_mode is None else 2 if goal_mode in (2, 3, 4, 5) else 1
    return kind, layout, traj, layout == "mixed" and substeps >= 2


INSTANCES = {(k, lay, tr, mag) for k in KINDS for tr in (0, 1, 2)
             for lay, mag in (("mixed", False), ("mixed", True), ("f64", False), ("f32", False))}

# (kind, layout, substeps, goal_mode, max_steps).  Every flight is 200 steps or fewer: the state bars were set for flights on GIVEN
# actions; here the float32 action feeds back (the oracle's and the kernel's action differ by an ulp now and then, 4.5e-8 measured),
# and the unstabilised loop amplifies that: the float64 layout's state error is 5e-7 after 200 steps and 3.3e-6 (v) after 400, the
# same with one and with four substeps — beyond its 2e-6 bar.  The circle's switch from run-up to circle at call 350 is therefore
# reached by running the generator's clock WARM_CALLS ahead at the start state, not by a 400-step flight.
WARM_CALLS = {5: 250}
# The float32 layout: numbers on a flight of F32_NUMBER_STEPS, decisions and write-back on one of F32_STEPS (see F32_BAR).
F32_STEPS, F32_NUMBER_STEPS = 20, 8
TABLE = [
    ("coupled", "mixed", 1, None, 200), ("coupled", "mixed", 4, None, 200), ("coupled", "f64", 1, None, 200), ("coupled", "f32", 4, None, F32_STEPS),
    ("coupled", "mixed", 1, 0, 200), ("coupled", "mixed", 4, 1, 200), ("coupled", "f64", 1, 6, 200), ("coupled", "f32", 1, 0, F32_STEPS),
    ("coupled", "mixed", 1, 2, 200), ("coupled", "mixed", 4, 3, 200), ("coupled", "f64", 4, 5, 200), ("coupled", "f32", 4, 4, 4 * F32_STEPS),
    ("decoupled", "mixed", 1, None, 200), ("decoupled", "mixed", 4, None, 200), ("decoupled", "f64", 4, None, 200), ("decoupled", "f32", 1, None, F32_STEPS),
    ("decoupled", "mixed", 1, 6, 200), ("decoupled", "mixed", 4, 0, 200), ("decoupled", "f64", 1, 1, 200), ("decoupled", "f32", 4, 1, F32_STEPS),
    ("decoupled", "mixed", 1, 3, 200), ("decoupled", "mixed", 4, 5, 200), ("decoupled", "f64", 4, 2, 200), ("decoupled", "f32", 1, 4, 4 * F32_STEPS),
]
assert {instance_of(*r[:4]) for r in TABLE} == INSTANCES and len(INSTANCES) == 24 and len(TABLE) == 24, \
    "the table must launch every eval_kernel instantiation, one row each"
assert all({r[3] for r in TABLE if r[0] == k} == {None, 0, 1, 2, 3, 4, 5, 6} for k in KINDS), "every goal mode on each wrapper"

# ---------------------------------------------------------------------------------------------------------------------
# bars (none of them new)
# ---------------------------------------------------------------------------------------------------------------------
OBS_BAR = 1e-5                 # observation rows, default and float64 layouts (test_trajectory_vs_oracle_256_envs_1000_steps)
STATE_BAR = {"mixed": 1e-5, "f64": 2e-6}   # grouped_rel_err of the state (the same test)
RETURN_BAR = 2e-5              # per step: the suite's reward bar (worst_rwd <= 2e-5), summed over the episode
# benchmark step = 0.5 (2 - |ex| - |eb1|), ex = 3 observation words (x_lim = 1), eb1 = pi times one: rows within OBS_BAR move it by at
# most 0.5 (sqrt 3 + pi) 1e-5 = 2.4e-5 per step, rounded to 2.5e-5
BENCH_BAR = 2.5e-5
ACTION_BAR = 2e-5              # test_closed_loop_vs_oracle_1000_envs: "closed loop: actor rounding feeds back"
GOAL_BAR = 3e-6                # the float32 goal words (test_gpu_replays_the_shipped_policy_flights); a write-back one call off is >= 2.5e-4
TIE_CAP = 3                    # test_production_mode_1000_steps_every_episode_vs_oracle
# The float32 layout is outside the parity bar by design; its only bar in the suite is test_f32_layout_runs_close's 5e-6 on the state.
# It is used as it stands, for every number of the float32 rows, and as the window inside which a decision may differ.  In closed loop
# the layout's error grows by about 3.5e-7 per step (measured on MI355X, worst of the six rows, state: 6.6e-7 after 1 step, 2.4e-6
# after 5, 3.6e-6 after 8, 4.6e-6 after 12, 7.4e-6 after 20, 1.1e-5 after 40), so 5e-6 holds for about 12 steps: the numbers are
# compared on a flight of F32_NUMBER_STEPS = 8 (the doomed third ends within 6).  The same starts are then flown F32_STEPS = 20 —
# the two stateful rows 80: they take their goal from the start position, so a doomed env needs 52 steps to get 1 m away from it —
# for the decisions, the counters and the generator's write-back only; the figures of that flight are printed, not asserted.
F32_BAR = 5e-6


def _np(t):
    return t.detach().cpu().numpy()


def _env(kind, n, **kw):
    from gym_rotor_amd import QuadVecEnv
    kw.setdefault("autotune", False)
    kw.setdefault("max_episode_steps", 10 ** 6)   # (so that episode_steps exists)
    return QuadVecEnv(kind, n, device="cuda", **kw)


def _hover_bias(c=None):
    """The mean bias of the thrust component that gives hover thrust at the nominal mass (test_success_flags_decided_on_purpose)."""
    from gym_rotor_amd.constants import QuadConstants
    c = c or QuadConstants()
    return math.atanh((c.hover_force - c.avrg_act) / c.scale_act)


def _actors(kind, seed, algo="ppo", weight=0.1, zero=False):
    """Actors of the reference's sizes with small mean weights and the hover-thrust bias: most envs at rest stay in the air for a few
    hundred steps, none is stabilised.  algo 'sac': a state-dependent log_std head and the tanh-of-sample rule; 'td3': TD3's form
    (log_std = log of a zero exploration std).  zero: all weights zero — exact hover."""
    from gym_rotor_amd import random_actors
    actors = random_actors(kind, "cuda", generator=torch.Generator("cuda").manual_seed(seed), log_std=-0.5, algo="sac" if algo == "sac" else "ppo")
    for a in actors:
        a.mean_w.mul_(weight)
        if algo == "td3":
            a.log_std.fill_(-30.0)
        if zero:
            for t in (a.fc1_w, a.fc1_b, a.fc2_w, a.fc2_b, a.mean_w, a.mean_b):
                t.zero_()
    actors[0].mean_b[0] = _hover_bias()
    return actors


def _weights(actors):
    """The actors' tensors as float64 arrays for actor_oracle (an actor with a log_std head is flown by its SAC rule)."""
    names = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std_w", "log_std_b")
    return [{k: _np(getattr(a, k)).astype(np.float64) for k in names if getattr(a, k) is not None} for a in actors]


# (start heights whose phase boundary is NOT on a multiple of dt: there the device clock, calls * dt in float32, and the reference's
#  accumulated float64 t may switch one call apart — test_stateful_phase_boundaries_within_one_call)
Z0 = {2: (-0.49321, -0.47137, -0.31234, -0.45613), 3: (-0.61357, -0.74213, -0.50777, -0.33391), 4: (-0.3, 0.2, 0.0, -0.1), 5: (0.0, -0.2, 0.1, -0.05)}


def _starts(env, x_lim=1.0, rest_x=None, warm=0):
    """Episode starts as test_gpu_evaluate._start makes them: reset('train'), then every third env doomed (0.1 x_lim inside the
    bound at 3.9 m/s outwards), every third at rest (stateful goal modes: at the start heights that reach their branches, as in
    test_stateful_phase_boundaries_within_one_call; `rest_x`: at these positions), the rest as the reset drew them; generator
    start with injected draws, first goal, first observation.  Returns (observation rows, state [N,18], params or None, draws)."""
    n, mode = env.num_envs, env.goal_mode
    env.reset("train")
    cur = _np(env.get_current_state())
    k = np.arange(n) % 3
    rest = np.zeros((n, 18))
    rest[:, 6] = rest[:, 10] = rest[:, 14] = 1.0
    doomed = rest.copy()
    doomed[:, 0], doomed[:, 3] = 0.9 * x_lim, 3.9
    if mode in Z0:
        rest[:, 0:2] = (0.1, -0.2)
        rest[:, 2] = np.resize(Z0[mode], n)
    if rest_x is not None:
        rest[:, 0:3] = np.resize(np.asarray(rest_x, np.float64).reshape(-1, 3), (n, 3))
    cur[k == 0], cur[k == 1] = doomed[k == 0], rest[k == 1]
    env.set_state(cur, integ=np.zeros((n, 8)))
    draws = (None, None, None)
    if mode is not None:
        rng = np.random.default_rng(17)
        draws = (rng.uniform(-0.4, 0.4, n).astype(np.float32), rng.uniform(2, 5, n).astype(np.float32), rng.uniform(-0.45, 0.45, n).astype(np.float32))
        env.mark_traj_start(theta_b1d=draws[0], t_traj=draws[1], w_b1d=draws[2])
        for _ in range(warm):
            env.get_desired()
        env.get_desired(store_goal=True)
    obs = [o.clone() for o in env.get_norm_error_state()]   # (from zero integrators, as the oracle forms it: main.py:305-309)
    params = None if env.params is None else _np(env.params).astype(np.float64)
    return obs, _np(env.get_current_state()), params, tuple(None if d is None else d.astype(np.float64) for d in draws)


def _done_words(kind, rows, t, i):
    """The normalised error components the done rule reads (coupled:95-110, decoupled:116-140) of env i after step t."""
    o0 = rows["obs0"][t, i].astype(np.float64)
    if kind == "coupled":
        return np.concatenate([o0[0:3], o0[6:9], o0[20:23]])
    return np.concatenate([o0[0:3], o0[6:9], o0[12:15], rows["obs1"][t, i, 2:3].astype(np.float64)])


def _ties(kind, got, want, bar, x_lim=1.0):
    """Envs whose length / terminated / success differ from the oracle's.  Each must be a tie: the oracle's deciding quantity — at
    the step where the two decisions part, the earlier of the two terminal steps — within `bar` (in observation units) of its
    threshold: a normalised error word of the done rule against 1, or |ex| / |eb1| against 0.01 (m, rad).  Anything else fails."""
    glen, wlen = _np(got["length"]), want["length"]
    bad_done = (glen != wlen) | (_np(got["terminated"]) != want["terminated"])
    bad_succ = ~bad_done & (_np(got["success"]) != want["success"]).any(1)
    rows = want["rows"]
    for i in np.flatnonzero(bad_done):
        t = min(glen[i], wlen[i]) - 1
        assert t < len(rows["obs0"]), (i, glen[i], wlen[i])
        margin = np.abs(np.abs(_done_words(kind, rows, t, i)) - 1.0).min()
        assert margin <= bar, f"env {i}: length {glen[i]} vs the oracle's {wlen[i]}, nearest done word {margin:.2e} from its threshold"
    for i in np.flatnonzero(bad_succ):
        t = wlen[i] - 1
        ex = np.abs(rows["obs0"][t, i, 0:3].astype(np.float64)) * x_lim
        eb1 = abs(float(rows["obs1"][t, i, 0] if kind == "decoupled" else rows["obs0"][t, i, 18])) * np.pi
        margin = min(np.abs(ex - 0.01).min() / x_lim, abs(eb1 - 0.01) / np.pi)
        assert margin <= bar, f"env {i}: success differs, |ex| {ex}, |eb1| {eb1}"
    return bad_done | bad_succ


def _fly_oracle(kind, state, params, T, actors, **kw):
    """The oracle's evaluation, flown twice: as specified, and with jittered actions and float32-rounded x, v.  The two must decide
    every env alike — a knife-edge input is an input problem, caught before the GPU is compared."""
    w = _weights(actors)
    want = eval_oracle(kind, state, params, T, actors=w, **kw)
    probe = eval_oracle(kind, state, params, T, actors=w, perturb=1, **kw)
    for k in ("length", "terminated", "success"):
        assert (want[k] == probe[k]).all(), f"knife-edge inputs: {k} differs under a 2e-7 perturbation at {np.flatnonzero((want[k] != probe[k]).reshape(len(state), -1).any(1))}"
    return want


def _compare(tag, env, got, want, layout, steps0, calls0=1, x_lim=1.0, numbers=True, theta0=None):
    """Everything evaluate returns and everything it freezes, per env, against the oracle's result.  numbers=False (the float32
    layout's long flights): the decisions, the counters and the generator's write-back only; the figures are printed, not asserted."""
    kind, n = env.kind, env.num_envs
    f32 = layout == "f32"
    obs_bar, state_bar = (F32_BAR, F32_BAR) if f32 else (OBS_BAR, STATE_BAR[layout])
    tie = _ties(kind, got, want, obs_bar, x_lim)
    assert tie.sum() <= TIE_CAP, f"{tie.sum()} decision ties"
    ok = ~tie
    length = want["length"]
    assert (_np(got["length"])[ok] == length[ok]).all() and (_np(got["terminated"])[ok] == want["terminated"][ok]).all()
    assert (_np(got["success"])[ok] == want["success"][ok]).all()
    # (float32 layout: a reward is at most first order in the rows, the benchmark step 0.5 (sqrt 3 + pi) times their error)
    ret_bar, bench_bar = (F32_BAR, 0.5 * (math.sqrt(3) + math.pi) * F32_BAR) if f32 else (RETURN_BAR, BENCH_BAR)
    worst = lambda err: (err.reshape(n, -1).max(1) if err.ndim > 1 else err)[ok].max()
    e_ret = worst(np.abs(_np(got["episode_return"]) - want["episode_return"]) / length[:, None])
    e_bench = worst(np.abs(_np(got["benchmark"]) - want["benchmark"]) / length)
    idx, last = np.arange(n), length - 1
    rows = want["rows"]
    scale = np.array([x_lim, x_lim, x_lim, np.pi])
    e_fe = worst(np.abs(_np(got["final_error"]).astype(np.float64) - want["final_error"]) / scale)
    e_obs = worst(np.abs(_np(got["obs0"]).astype(np.float64) - rows["obs0"][last, idx]))
    if kind == "decoupled":
        e_obs = max(e_obs, worst(np.abs(_np(got["obs1"]).astype(np.float64) - rows["obs1"][last, idx])))
    e_act = worst(np.abs(_np(got["action"]).astype(np.float64) - rows["action"][last, idx]))
    e_state = grouped_rel_err(_np(env.get_current_state())[ok], want["state"][ok])
    # integrators (words in metres / radians: ex x_lim, eb1 pi and their trapezoid sums): the observation bar times that scale
    iscale = np.array([x_lim] * 6 + [np.pi] * 2)
    e_integ = worst(np.abs(_np(env.integ).astype(np.float64) - want["integ"]) / iscale)
    print(f"{tag}: {int((~want['terminated']).sum())}/{n} survive, ties {int(tie.sum())}; per step: return {e_ret:.1e} benchmark {e_bench:.1e}; "
          f"final_error {e_fe:.1e} rows {e_obs:.1e} action {e_act:.1e} state {e_state:.1e} integ {e_integ:.1e}" + ("" if numbers else " (not asserted)"))
    if numbers:
        assert e_ret <= ret_bar and e_bench <= bench_bar, (e_ret, e_bench)
        assert e_fe <= obs_bar and e_obs <= obs_bar and e_act <= ACTION_BAR, (e_fe, e_obs, e_act)
        assert e_state <= state_bar and e_integ <= obs_bar, (e_state, e_integ)
    assert (_np(env.episode_steps - steps0)[ok] == length[ok]).all()
    if env.goal_mode is not None:
        assert (_np(env._traj[0])[ok] == calls0 + length[ok]).all(), "the generator's call counter: one call per step flown"
    if env.goal_mode in (2, 3, 4, 5):   # TRAJ == 2: the generator's persistent fields as the oracle's generator held them at that env's terminal step
        tr = want["traj"]
        e_goal = np.abs(_np(env._goal).T.astype(np.float64) - want["goal"])[ok].max()
        traj = _np(env._traj).astype(np.float64)
        e_bdot = np.abs(traj[[2, 7]].T - tr["b1d_dot"][:, 0:2])[ok].max()
        e_init = np.abs(traj[4:7].T - tr["x_init"])[ok].max()
        flags = tr["started"] * 1 + tr["complete"] * 2 + tr["manual"] * 4 + tr["manual_init"] * 8 + tr["landed"] * 16
        print(f"{tag}: goal {e_goal:.1e} b1d_dot {e_bdot:.1e} x_init {e_init:.1e}; flags at the terminal step {sorted(set(flags[ok].tolist()))}")
        assert e_goal <= GOAL_BAR and e_bdot <= GOAL_BAR and e_init <= GOAL_BAR, (e_goal, e_bdot, e_init)
        assert (traj[3][ok] == flags[ok]).all(), np.flatnonzero(traj[3] != flags)
        # (field 1, theta_init, is set at mark_traj_start and only carried: the value from before the launch)
        assert theta0 is not None and np.array_equal(_np(env._traj[1])[ok], theta0[ok])
    return ok


def _run(tag, kind, n, T, actors, layout="mixed", substeps=1, goal_mode=None, x_lim=1.0, rest_x=None, max_action=1.0, out=None,
         numbers_steps=None, setup=None, **kw):
    """One case: env, starts, the oracle's evaluation (knife-edge inputs refused on it alone), the launch, the comparison.
    numbers_steps = K (float32 layout): the numbers are compared on a flight of K steps from these starts, the T-step flight —
    from the same starts again — for the decisions, the counters and the generator's write-back only."""
    env = _env(kind, n, layout=layout, substeps=substeps, goal_mode=goal_mode, **kw)
    if setup is not None:   # (what the constructor cannot express, e.g. QrCoeffs.CW apart from Cw12)
        setup(env)
    warm = WARM_CALLS.get(goal_mode, 0)
    obs, state, params, draws = _starts(env, x_lim, rest_x, warm)
    env.start = (env.state_dict(), [o.clone() for o in obs])
    theta0 = None if env._traj is None else _np(env._traj[1]).copy()
    for steps, numbers in ([(numbers_steps, True)] if numbers_steps else []) + [(T, numbers_steps is None)]:
        env.load_state_dict(env.start[0])
        want = _fly_oracle(kind, state, params, steps, actors, goal_mode=goal_mode, draws=draws, n_sub=substeps, max_action=max_action, warm_calls=warm)
        steps0 = env.episode_steps.clone()
        got = env.evaluate(actors, max_steps=steps, obs=[o.clone() for o in obs], max_action=max_action, out=out)
        torch.cuda.synchronize()
        ok = _compare(f"{tag}, {steps} steps", env, got, want, layout, steps0, calls0=1 + warm, x_lim=x_lim, numbers=numbers, theta0=theta0)
    return env, got, want, ok


# ---------------------------------------------------------------------------------------------------------------------
# every instantiation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,layout,substeps,goal_mode,T", TABLE)
def test_every_eval_instantiation_against_the_oracle(kind, layout, substeps, goal_mode, T):
    """300 envs (four full tiles and a ragged one) from doomed, resting and reset-drawn starts: length, terminated and success as
    the oracle decides them (ties: within the row bar of a threshold, at most 3), returns and benchmark per step, final rows,
    last action, frozen state, integrators, step and call counters and — stateful modes — the goal buffer and generator fields
    of each env's own terminal step.
    Measured on an MI355X, worst over the rows: default layout return 1.8e-6 and benchmark 1.4e-6 per step, rows and state 5.9e-6,
    goal words 1.6e-6; float64 layout 1.0e-7, 1.0e-7, 4.2e-7 / 5.3e-7; float32 layout after its 8 steps return 4.5e-7 and benchmark
    7.9e-7 per step, rows 2.8e-6, state 3.6e-6 (bar 5e-6; its longer flight is compared in decisions and write-back only); no tie
    in any row."""
    env, got, want, ok = _run(f"{kind} {layout} x{substeps} goal {goal_mode}", kind, 300, T, _actors(kind, 3), layout, substeps, goal_mode,
                              numbers_steps=F32_NUMBER_STEPS if layout == "f32" else None)
    term = want["terminated"]
    assert term.any() and (~term).any(), "the oracle alone shows both fates"
    assert (want["length"][term] < T).any()
    if goal_mode in (2, 3, 5):   # some survivor's flight crosses a phase switch of the generator
        tr = want["traj"]
        later = {2: tr["manual"], 3: want["goal"][:, 2] == -0.25, 5: tr["b1d_dot"][:, 0] != 0.0}[goal_mode]
        assert later[~term].any(), "no survivor reached the mode's later phase"


# ---------------------------------------------------------------------------------------------------------------------
# the flight continued by the next launch (stateful write-back, behavioural)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode,T1,T2", [(2, 15, 45), (3, 40, 60), (4, 10, 20), (5, 340, 30)])
def test_flight_continues_after_evaluate(kind, mode, T1, T2):
    """evaluate(T1), then the survivors fly on with rollout_actor(deterministic, T2) across a phase switch of the generator (take-off
    reaching its end height, landing its cut-off height, the circle's run-up ending at call 350): the bits of ONE
    rollout_actor(deterministic, T1 + T2) from the same start.  Nothing the next launch needs was left in registers.
    Stay (mode 4) has NO switch to cross: it is in manual mode from its second call on, before T1 ends; for that row T2 only
    checks that the held goal is carried on unchanged."""
    n = 300
    env = _env(kind, n, seed=11, goal_mode=mode, w_adapt=0.0)
    obs, _, _, _ = _starts(env)
    sd = env.state_dict()
    actors = _actors(kind, 6)
    full = env.rollout_actor(actors, T1 + T2, obs=[o.clone() for o in obs], deterministic=True)
    s_full, traj_full, goal_full = env.get_current_state(), env._traj.clone(), env._goal.clone()
    env.load_state_dict(sd)
    ev = env.evaluate(actors, max_steps=T1, obs=[o.clone() for o in obs])
    surv = (ev["length"] == T1) & ~ev["terminated"]
    assert surv.any() and ((~surv).any() or T1 < 52)   # (a doomed env needs 52 steps to get 1 m away from a goal taken at its start)
    flags1, goal1 = env._traj[3].clone(), env._goal.clone()
    cont = env.rollout_actor(actors, T2, deterministic=True)
    torch.cuda.synchronize()
    for k in ("obs0", "obs1", "action", "reward", "terminated"):
        if k in full:
            assert torch.equal(cont[k][:, surv], full[k][T1:, surv]), k
    assert torch.equal(env.get_current_state()[surv], s_full[surv])
    assert torch.equal(env._traj[:, surv], traj_full[:, surv]) and torch.equal(env._goal[:, surv], goal_full[:, surv])
    switched = {2: env._traj[3] != flags1, 3: (env._goal[2] == -0.25) & (goal1[2] != -0.25), 4: goal1[2] == env._goal[2],
                5: (env._traj[2] != 0) | (env._traj[7] != 0)}[mode]   # (stay: no switch, the goal stays as it was)
    assert bool(switched[surv].any()), "T2 crosses a phase switch of the generator (stay: the goal is held)"


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_max_steps_one(kind):
    """max_steps == 1: every env has length 1, success is judged at that step — an env at rest at the goal succeeds."""
    env, got, want, ok = _run(f"{kind} max_steps 1", kind, 130, 1, _actors(kind, 2, zero=True), use_UDM=False)
    assert (_np(got["length"]) == 1).all()
    rest = np.arange(130) % 3 == 1
    assert _np(got["success"])[rest].all() and want["success"][rest].all() and not _np(got["terminated"])[rest].any()


@pytest.mark.parametrize("kind", KINDS)
def test_out_of_bounds_at_the_start(kind):
    """Envs that start with |ex| > x_lim: length 1, terminated, return -1 for the agent that is done and — decoupled — the other
    agent's normalised reward."""
    n = 130
    env = _env(kind, n, use_UDM=False)
    actors = _actors(kind, 2)
    state = np.zeros((n, 18))
    state[:, 6] = state[:, 10] = state[:, 14] = 1.0
    out_ = np.arange(n) % 2 == 0
    state[out_, 0] = 1.2
    env.set_state(state, integ=np.zeros((n, 8)))
    obs = [o.clone() for o in env.get_norm_error_state()]
    state = _np(env.get_current_state())
    want = _fly_oracle(kind, state, None, 50, actors)
    steps0 = env.episode_steps.clone()
    got = env.evaluate(actors, max_steps=50, obs=obs)
    torch.cuda.synchronize()
    _compare(f"{kind} out of bounds at the start", env, got, want, "mixed", steps0)
    ret = _np(got["episode_return"])
    assert (_np(got["length"])[out_] == 1).all() and _np(got["terminated"])[out_].all() and (ret[out_, 0] == -1.0).all()
    assert (_np(got["length"])[~out_] == 50).all()
    if kind == "decoupled":
        assert ((ret[out_, 1] > 0.9) & (ret[out_, 1] <= 1.0)).all() and np.abs(ret[out_, 1] - want["episode_return"][out_, 1]).max() <= RETURN_BAR


@pytest.mark.parametrize("kind", KINDS)
def test_tile_geometry_and_no_write_past_the_batch(kind):
    """Batches of 1, 63, 64, 65 and 129 envs: each env's results are the bits it has inside a 300-env batch (evaluate has no
    cross-env coupling), and no output row before the first or past the N-th is written (outputs inside guard tensors)."""
    T, big, G = 60, 300, 64
    actors = _actors(kind, 8)
    env, ref, want, _ = _run(f"{kind} 300 envs, 60 steps", kind, big, T, actors, seed=21)
    sd, obs_all = env.start
    s_ref, i_ref = env.get_current_state(), env.integ.clone()
    term = _np(ref["terminated"])
    for n in (1, 63, 64, 65, 129):
        e = _env(kind, n, seed=21)
        for k in ("pos_vel", "att_rate", "integ", "params"):   # the first n envs of the big batch, bit for bit
            getattr(e, "_" + k).copy_(sd[k][:, :n])
        guard, out = {}, {}
        for k, v in ref.items():
            guard[k] = torch.full((n + 2 * G,) + tuple(v.shape[1:]), True if v.dtype == torch.bool else 77, dtype=v.dtype, device="cuda")
            out[k] = guard[k][G:G + n]
        got = e.evaluate(actors, max_steps=T, obs=[o[:n].clone() for o in obs_all], out=out)
        torch.cuda.synchronize()
        for k, v in ref.items():
            fill = True if v.dtype == torch.bool else 77
            assert torch.equal(got[k], v[:n]), (n, k)
            assert bool((guard[k][:G] == fill).all()) and bool((guard[k][G + n:] == fill).all()), (n, k, "guard rows written")
        assert torch.equal(e.get_current_state(), s_ref[:n]) and torch.equal(e.integ, i_ref[:n])
        if n >= 63:
            assert term[:n].any() and (~term[:n]).any()


@pytest.mark.parametrize("kind", KINDS)
def test_non_default_limits_and_reward_coefficients(kind):
    """x_lim = 2 and other reward coefficients (QuadConstants), the same values in the oracle.  Envs hover at 8, 12, 15 and 25 mm from
    the goal — both sides of |ex| = 0.01 in METRES and of 0.01 in normalised units: without the x_lim factor in ex the 12 and 15 mm
    envs would succeed; the doomed third starts 0.2 m inside the 2 m bound."""
    from gym_rotor_amd.constants import QuadConstants
    c = QuadConstants(x_lim=2.0, Cx=8.0, Cv=0.7, Cb1=4.5, Cw12=0.9, CW3=0.3)
    n, T = 130, 100
    rest_x = [(0.008, 0, 0), (0, -0.012, 0), (0, 0, 0.015), (0.025, 0, 0)]
    with orc.constants(c):
        assert (orc.X_LIM, orc.CW, orc.REWARD_MIN, orc.REWARD_MIN_1, orc.REWARD_MIN_2) == (2.0, 0.9, c.reward_min, c.reward_min_1, c.reward_min_2)
        env, got, want, ok = _run(f"{kind} x_lim 2", kind, n, T, _actors(kind, 2, zero=True), x_lim=2.0, rest_x=rest_x, use_UDM=False, constants=c)
    i = np.flatnonzero(np.arange(n) % 3 == 1)
    succ = _np(got["success"])[i, 0]
    assert (succ == (i % 4 == 0)).all() and (want["success"][i, 0] == succ).all(), succ
    assert want["terminated"].any() and (~want["terminated"]).any()


@pytest.mark.parametrize("kind", KINDS)
def test_max_action_clamps_the_mean(kind):
    """max_action = 0.5 with an actor whose tanh(mean) often exceeds it: the action is the oracle's clip(mean, +-0.5)."""
    actors = _actors(kind, 4, weight=5.0)
    actors[0].mean_b[1], actors[0].mean_b[2] = 1.0, -1.0   # tanh: +-0.76
    env, got, want, ok = _run(f"{kind} max_action 0.5", kind, 130, 30, actors, max_action=0.5)
    acts = want["rows"]["action"]
    assert (np.abs(acts) == 0.5).mean() > 0.1 and np.abs(acts).max() == 0.5 and np.abs(_np(got["action"])).max() == 0.5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_sac_and_td3_form_actors(kind, algo):
    """SAC's form (a log_std head, tanh of the sample) and TD3's (a log exploration std): evaluate ignores the head and flies
    tanh(mean) / clip(mean)."""
    actors = _actors(kind, 5, algo=algo, weight=3.0)
    assert (actors[0].log_std_w is not None) == (algo == "sac")
    env, got, want, ok = _run(f"{kind} {algo}-form actor", kind, 130, 60, actors)
    assert want["terminated"].any() and (~want["terminated"]).any()


@pytest.mark.parametrize("kind", KINDS)
def test_nominal_parameters_without_a_params_buffer(kind):
    """use_UDM=False: the env has no parameter buffer (params=None: nominal), against the nominal oracle."""
    actors = _actors(kind, 9)
    env = _env(kind, 130, use_UDM=False)
    assert env.params is None
    obs, state, params, _ = _starts(env)
    assert params is None and env.params is None
    want = _fly_oracle(kind, state, None, 120, actors)
    steps0 = env.episode_steps.clone()
    got = env.evaluate(actors, max_steps=120, obs=obs)
    torch.cuda.synchronize()
    _compare(f"{kind} nominal, no params buffer", env, got, want, "mixed", steps0)
    assert want["terminated"].any() and (~want["terminated"]).any()
