"""Every runtime coefficient (QrCoeffs) off its default, through every kernel that reads it, against the float64 oracle flown
under the same constants (oracle.quad_oracle.constants) and against the reference's own vectors for two all-fields sets
(tests/golden/onestep_coeffs_{A,B}.npz).  The bars are the suite's own (coeff_cases.py names where each comes from); that a kernel
ignoring a field WOULD miss them is checked on the CPU (test_oracle_coeffs.py: test_power_of_the_single_field_sweep)."""
import math

import numpy as np
import pytest
import torch

import coeff_cases as cc
from conftest import grouped_rel_err
from oracle import quad_oracle as orc
from oracle import traj_oracle as trj

pytestmark = pytest.mark.gpu
KINDS = orc.KINDS
SETS = ("A", "B")


def _np(t):
    return t.detach().cpu().numpy()


def _env(kind, n, constants, udm, cw=None, **kw):
    from gym_rotor_amd import QuadVecEnv
    kw.setdefault("autotune", False)
    env = QuadVecEnv(kind, n, device="cuda", want_raw_reward=True, constants=constants, UDM_percentage=udm, **kw)
    if cw is not None:      # CW apart from Cw12: the ABI's field, which QuadConstants ties to Cw12
        env._cenv.coeffs.CW = cw
        env._sync_structs()
    return env


def _set_goal(env, goal):
    g = torch.as_tensor(goal, dtype=torch.float32, device=env.device)
    env.set_goal_state(g[:, 0:3], g[:, 3:6], g[:, 6:9], None, g[:, 9:12])


def _obs_list(obs):
    return [obs] if isinstance(obs, torch.Tensor) else list(obs)


def _onestep(kind, layout, substeps, constants, udm, cw, d):
    """One step() from the inputs `d` (state, action, params or None, goal, integ): what the kernel left, as float64 arrays."""
    n = d["state"].shape[0]
    env = _env(kind, n, constants, udm, cw, layout=layout, substeps=substeps, obs_rows=True, use_UDM=d["params"] is not None,
               reset_on_done=substeps > 1, w_adapt=16.0 if substeps == 1 else 0.0)
    if substeps > 1:    # the plain Magnus-substep kernel, as test_onestep_golden_magnus_substeps reaches it (w_adapt = 0: also where 2.5 W_lim > 16)
        plan = env.launch_plan()
        assert plan["mag"] == 1 and plan["adapt"] == 0
    assert (env.params is None) == (d["params"] is None)
    env.set_state(d["state"], integ=d["integ"], **({} if d["params"] is None else {"params": d["params"]}))
    _set_goal(env, d["goal"])
    obs, rwd, done, _, _ = env.step(torch.from_numpy(d["action"].astype(np.float32)).cuda())
    torch.cuda.synchronize()
    got = dict(state=_np(env.get_current_state()), obs=[_np(o).astype(np.float64) for o in _obs_list(obs)],
               reward_raw=_np(env._reward_raw).astype(np.float64), reward=_np(rwd).astype(np.float64), done=_np(done).astype(bool))
    if kind != "quad":
        got["integ"] = _np(env.integ).astype(np.float64)
    return got


def _check_onestep(tag, kind, layout, substeps, c, got, want, margin, ulp=None, exact_done=None):
    """The comparisons of test_onestep_golden at its bars; `want`: dict(state, obs, integ, reward_raw, reward, done), `margin`: per row
    the distance of the nearest deciding quantity from its threshold, relative to its limit (coeff_cases.done_margin).  Done flags:
    identical except within DONE_WINDOW; the rows excused are at most DONE_CAP of the case — the `ulp` rows (put inside the window
    on purpose) apart; `exact_done`: rows that must decide alike whatever their margin.  Returns the figures, for the record."""
    n = len(margin)
    ulp = np.zeros(n, bool) if ulp is None else ulp
    fig = {"state": grouped_rel_err(got["state"], want["state"])}
    if kind != "quad":
        fig["obs"] = max((np.abs(g - w.astype(np.float64)) / np.maximum(np.abs(w), 1.0) / bar).max() * cc.OBS_TOL
                         for g, w, bar in zip(got["obs"], want["obs"], cc.obs_bars(kind, c)))
        fig["integ"] = np.abs(got["integ"] - want["integ"]).max()
    else:
        fig["obs"] = (np.abs(got["obs"][0] - want["state"]) / np.maximum(np.abs(want["state"]), 1.0)).max()   # Quad-v0's row: the float32 state, per word
    fig["reward_raw"] = np.abs(got["reward_raw"] - want["reward_raw"]).max() / max(1.0, np.abs(want["reward_raw"]).max())
    differs = (got["done"] != want["done"]).any(1)
    same = got["done"] == want["done"]
    fig["reward"] = np.abs(got["reward"] - want["reward"])[same].max()
    fig["done_excused"] = int((differs & ~ulp).sum())
    print(f"{tag} {kind}/{layout}/S={substeps}: " + " ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in fig.items())
          + f" ulp rows deciding otherwise {int((differs & ulp).sum())}")
    assert fig["state"] <= cc.ONESTEP_TOL[(layout, substeps)], fig
    assert fig["obs"] <= cc.OBS_TOL, fig          # (per word, in units of its own bar: obs_bars)
    if kind != "quad":
        assert fig["integ"] <= cc.INTEG_TOL, fig
    assert fig["reward_raw"] <= cc.RAW_TOL and fig["reward"] <= cc.REWARD_TOL, fig
    assert (margin[differs] < cc.DONE_WINDOW).all(), (np.flatnonzero(differs), margin[differs])
    assert fig["done_excused"] <= cc.DONE_CAP * n
    if exact_done is not None:
        assert not differs[exact_done].any(), np.flatnonzero(differs & exact_done)
    # The kernel's own rule on the kernel's own numbers, exact and independent of the oracle's last ulp.  The wrappers decide on the
    # float32 observation words they return (coupled:95-110, decoupled:116-140), in every layout.  Quad-v0 in the default layout holds
    # x and v as float32 and compares them with x_lim_up / v_lim_up, the smallest float32 not below the limit: |x_f32| < up must be
    # |x_f32| < limit in float64 — a limit rounded the other way, or (float)x_lim in one integrator variant, decides the rows one
    # ulp inside the limit otherwise.  (W and the Euler angles of those rows are far from their thresholds: asserted.)
    if kind != "quad":
        o = got["obs"]
        words = [o[0][:, 0:3], o[0][:, 6:9], o[0][:, 20:23]] if kind == "coupled" else [o[0][:, 0:3], o[0][:, 6:9], o[0][:, 12:15]]
        own = [(np.abs(np.concatenate(words, 1)) >= 1.0).any(1)] + ([np.abs(o[1][:, 2]) >= 1.0] if kind == "decoupled" else [])
        assert np.array_equal(np.stack(own, 1), got["done"]), "done flags against the returned observation words"
    elif layout == "mixed" and ulp.any():
        s_ = got["state"][ulp]
        assert np.array_equal(s_[:, 0:6], s_[:, 0:6].astype(np.float32).astype(np.float64)), "x, v of the default layout are float32 numbers"
        own = (np.abs(s_[:, 0:3]) >= c.x_lim).any(1) | (np.abs(s_[:, 3:6]) >= c.v_lim).any(1)
        R = np.swapaxes(s_[:, 6:15].reshape(-1, 3, 3), 1, 2)
        ang = np.degrees(np.maximum(np.abs(np.arctan2(R[:, 2, 1], R[:, 2, 2])), np.abs(np.arcsin(np.clip(R[:, 2, 0], -1, 1)))))
        assert (np.abs(s_[:, 15:18]).max(1) < 0.9 * c.W_lim).all() and (ang < 0.9 * c.euler_lim).all()
        assert own.any() and not own.all(), "the ulp rows end on both sides of the limit"
        assert np.array_equal(own, got["done"][ulp, 0]), (own, got["done"][ulp, 0])
    return fig


# ---------------------------------------------------------------------------------------------------------------------
# a. one field at a time
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_env", [False, True], ids=["nominal", "per-env-params"])
@pytest.mark.parametrize("name,kind", [(f, k) for f in cc.FIELDS for k in KINDS if k in cc.FIELDS[f][2]])   # (a kind that does not read a field is not flown for it)
def test_single_field_sweep(name, kind, per_env):
    """One field off its default, one step() in the default layout with one RK4 substep and with two Magnus substeps and in the
    float64 layout, from starts scaled to the perturbed limits, non-zero integrator words and goals with non-zero Wd; per-env
    parameters drawn around the (perturbed) nominals at 13 %, or none (nominal: the kernel's own nom[] / nom_f[]).  For x_lim = 0.7
    and v_lim = 3.3 (not float32 numbers) ten rows end within 1-5 float32 ulps of the limit: in the float64 layout Quad-v0 must
    decide them as the oracle does (its error there is 2e-8 at most, an ulp is 6e-8 / 2.4e-7); in the default layout, which alone
    reads x_lim_up / v_lim_up, as its own returned float32 x, v decide against the float64 limit (_check_onestep)."""
    c = cc.quad_constants(name)
    cw = cc.FIELDS[name][1].get("CW")
    with orc.constants(**cc.oracle_kw(name)):
        d = cc.sweep_inputs(kind, name, per_env)
        want = orc.step_batch(kind, d["state"], d["action"], d["params"], d["goal"], d["integ"])
        margin = cc.done_margin(kind, want)
    assert want["done"].any() and not want["done"].all()
    for layout, substeps in cc.VARIANTS:
        if substeps > 1:
            with orc.constants(**cc.oracle_kw(name)):     # (the oracle's converged step does not depend on the split; n_sub as a check of that)
                assert grouped_rel_err(orc.step_batch(kind, d["state"], d["action"], d["params"], d["goal"], d["integ"], n_sub=2)["state"], want["state"]) < 1e-12
        got = _onestep(kind, layout, substeps, c, cc.UDM_SWEEP, cw, d)
        exact = d["ulp"] if (layout == "f64" and kind == "quad") else None
        _check_onestep(f"sweep {name} {'per-env' if per_env else 'nominal'}", kind, layout, substeps, c, got, want, margin, d["ulp"], exact)


# ---------------------------------------------------------------------------------------------------------------------
# b. all fields at once, against the reference's own vectors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,substeps", cc.VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SETS)
def test_onestep_golden_under_coefficient_sets(name, kind, layout, substeps, golden):
    """test_onestep_golden on the reference flown with every coefficient moved (set A down, set B up; CW apart from Cw12)."""
    g = golden(f"onestep_coeffs_{name}")
    d = cc.of_kind(g, kind)
    c, udm, cw, kw = cc.coeff_set(g)
    d["obs"] = [d[f"obs{k}"] for k in range(1 if kind != "decoupled" else 2)]
    want = dict(state=d["next_state"], obs=d["obs"], integ=d["next_integ"], reward_raw=d["reward_raw"], reward=d["reward"], done=d["done"])
    with orc.constants(**kw):
        margin = cc.done_margin(kind, want)
    got = _onestep(kind, layout, substeps, c, udm, cw, d)
    _check_onestep(f"set {name}", kind, layout, substeps, c, got, want, margin)


@pytest.mark.parametrize("layout", ["mixed", "f64"])
@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
@pytest.mark.parametrize("name", SETS)
def test_error_obs_formats_under_coefficient_sets(name, kind, layout, golden):
    """get_norm_error_state in either format on either wrapper (qr_error_obs_format) at the bars of
    test_error_obs_in_either_format_on_either_wrapper, the observation bar scaled per word as obs_bars derives it."""
    g = golden(f"onestep_coeffs_{name}")
    c, udm, cw, kw = cc.coeff_set(g)
    n = g["errobs_state"].shape[0]
    for fw, okind in (("MONO", "coupled"), ("MODUL", "decoupled")):
        env = _env(kind, n, c, udm, cw, use_UDM=False, layout=layout)
        env.set_state(g["errobs_state"], integ=g["errobs_integ"])
        _set_goal(env, g["errobs_goal"])
        rows = env.get_norm_error_state(fw)
        for k, (r, bar) in enumerate(zip(rows, cc.obs_bars(okind, c))):
            err = np.abs(_np(r).astype(np.float64) - g[f"errobs_{fw}_obs{k}"])
            print(f"set {name} {kind}/{layout} {fw} row {k}: {(err / bar).max() * cc.OBS_TOL:.2e}")
            assert (err <= bar).all()
        assert np.abs(_np(env.integ) - g[f"errobs_{fw}_next_integ"]).max() <= 4e-6


# ---------------------------------------------------------------------------------------------------------------------
# c. the long paths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,substeps", [("mixed", 1), ("mixed", 4), ("f64", 1)])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SETS)
def test_free_trajectories_under_coefficient_sets(name, kind, layout, substeps, golden):
    """256 envs, 200 free steps with step() and the same with rollout(): the state within the trajectory bar (1e-5 grouped) of the
    oracle flown under the same constants, rewards within 2e-5 where both decide alike, the two launch families bit for bit."""
    c, udm, cw, kw = cc.coeff_set(golden(f"onestep_coeffs_{name}"))
    n, T, A = 256, 200, orc.ACTION_DIM[kind]
    rng = np.random.default_rng(31 + 7 * KINDS.index(kind) + (0 if name == "A" else 100))
    with orc.constants(**kw):
        state = cc.state_in(orc.sample_reset_state(rng, n, "train"))
        state[:, 3:6] *= 0.3; state[:, 15:18] *= 0.3
        state = cc.state_in(state)
        params = cc.f32r(orc.sample_params(rng, n, "train"))
        acts = cc.f32r(0.3 * rng.uniform(-1, 1, (T, n, A)))
        acts[:, :, 0] += np.float32(math.atanh((c.hover_force - c.avrg_act) / c.scale_act))     # around hover at the set's own vehicle
        acts = cc.f32r(np.clip(acts, -1, 1))
        s, integ = state.copy(), np.zeros((n, 8))
        if kind != "quad":
            integ = orc.error_obs_batch(kind, s)["integ"]
        alive = np.ones(n, bool)
        rw, dn = np.zeros((T, n, orc.N_AGENTS[kind])), np.zeros((T, n, orc.N_AGENTS[kind]), bool)
        for t in range(T):
            o = orc.step_batch(kind, s, acts[t], params, None, integ, n_sub=substeps)
            s, integ, rw[t], dn[t] = o["state"], o["integ"], o["reward"], o["done"]
            alive &= np.abs(s[:, 15:18]).max(1) < 14.0     # (below w_adapt = 16 rad/s: the regime the parity bar is stated for)
    assert alive.mean() > 0.5 and dn.any()
    tact = torch.from_numpy(acts.astype(np.float32)).cuda()
    out = []
    for mode in ("step", "rollout"):
        env = _env(kind, n, c, udm, cw, layout=layout, substeps=substeps, obs_rows=True)
        env.set_state(state, integ=np.zeros((n, 8)), params=params)
        if kind != "quad":
            env.get_norm_error_state()
        if mode == "step":
            r, dd = zip(*[(x[1].clone(), x[2].clone()) for x in (env.step(tact[t].contiguous()) for t in range(T))])
            r, dd = torch.stack(r), torch.stack(dd)
        else:
            ro = env.rollout(tact)
            r, dd = ro["reward"], ro["terminated"]
        torch.cuda.synchronize()
        out.append((_np(env.get_current_state()), _np(r).reshape(T, n, -1).astype(np.float64), _np(dd).reshape(T, n, -1).astype(bool)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    got_s, got_r, got_d = out[0]
    err = grouped_rel_err(got_s[alive], s[alive])
    same = (got_d == dn) & alive[None, :, None]
    e_r = np.abs(got_r - rw)[same].max()
    print(f"set {name} free run {kind}/{layout}/S={substeps}: state {err:.2e} reward {e_r:.2e} done differs {(~(got_d == dn))[:, alive].mean():.1e}")
    assert err <= 1e-5 and e_r <= 2e-5
    assert (got_d != dn)[:, alive].mean() <= 1e-3


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
@pytest.mark.parametrize("goal_mode", [None, 1, 6])
@pytest.mark.parametrize("name", SETS)
def test_evaluate_under_coefficient_sets(name, kind, goal_mode, golden):
    """evaluate_policy's launch (qr_evaluate_actor: its own copy of the reward code, the fused goal generator with the set's dt and
    eight-curve values) against the oracle's evaluation under the same constants, with the helpers and bars of
    test_gpu_evaluate_oracle.py."""
    import test_gpu_evaluate_oracle as ev
    c, udm, cw, kw = cc.coeff_set(golden(f"onestep_coeffs_{name}"))
    def set_cw(env):            # CW apart from Cw12 in the eval kernel's own copy of the reward code
        env._cenv.coeffs.CW = cw
        env._sync_structs()

    actors = ev._actors(kind, 3)
    actors[0].mean_b[0] = ev._hover_bias(c)
    with orc.constants(**kw):
        env, got, want, ok = ev._run(f"set {name} {kind} goal {goal_mode}", kind, 300, 200, actors, "mixed", 1, goal_mode, x_lim=c.x_lim,
                                     constants=c, UDM_percentage=udm, setup=set_cw)
    assert want["terminated"].any() and (~want["terminated"]).any()


@pytest.mark.parametrize("layout", ["mixed", "f64"])
@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
@pytest.mark.parametrize("name", SETS)
def test_rollout_actor_with_injected_noise_under_coefficient_sets(name, kind, layout, golden):
    """qr_rollout_actor with injected noise (the stochastic PPO rule) in closed loop, 300 envs x 64 steps, against oracle env +
    oracle actor under the set: test_closed_loop_vs_oracle_1000_envs at its bars (action 2e-5, float64-layout state 2e-6, rows
    2e-5), the default layout at the trajectory bar 1e-5.  Envs whose rate leaves the regime (|W| >= 14 rad/s) are not compared."""
    import test_gpu_evaluate_oracle as ev
    from oracle import actor_oracle as ao
    c, udm, cw, kw = cc.coeff_set(golden(f"onestep_coeffs_{name}"))
    n, T = 300, 64
    rng = np.random.default_rng(41 + len(kind))
    actors = ev._actors(kind, 7, weight=1.0)
    actors[0].mean_b[0] = ev._hover_bias(c)
    names = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std")
    pw = [{f: _np(getattr(a, f)).astype(np.float64) for f in names} for a in actors]
    adims = [p["mean_w"].shape[0] for p in pw]
    env = _env(kind, n, c, udm, cw, layout=layout, obs_rows=True)
    with orc.constants(**kw):
        state = cc.state_in(orc.sample_reset_state(rng, n, "train"))
        params = cc.f32r(orc.sample_params(rng, n, "train"))
        env.set_state(state, integ=np.zeros((n, 8)), params=params)
        state = _np(env.get_current_state())
        env.get_norm_error_state()
        eps = rng.standard_normal((T, n, env.action_dim)).astype(np.float32)
        out = env.rollout_actor(actors, T, noise=torch.from_numpy(eps).cuda())
        torch.cuda.synchronize()
        o = orc.error_obs_batch(kind, state, None, np.zeros((n, 8)))
        s, integ, obs = state, o["integ"], o["obs"]
        alive, worst_a, worst_r = np.ones(n, bool), 0.0, 0.0
        for t in range(T):
            col, acts = 0, []
            for k, p in enumerate(pw):
                a_, _, _ = ao.choose_action(p, obs[k], eps[t, :, col:col + adims[k]])
                acts.append(a_); col += adims[k]
            act = np.concatenate(acts, 1).astype(np.float32)
            worst_a = max(worst_a, np.abs(act - _np(out["action"][t]))[alive].max())
            o = orc.step_batch(kind, s, act.astype(np.float64), params, None, integ)
            s, integ, obs = o["state"], o["integ"], o["obs"]
            alive &= np.abs(s[:, 15:18]).max(1) < 14.0
            same = (_np(out["terminated"][t]).reshape(n, -1).astype(bool) == o["done"]) & alive[:, None]
            worst_r = max(worst_r, np.abs(_np(out["reward"][t]).reshape(n, -1) - o["reward"])[same].max())
    e_s = grouped_rel_err(_np(env.get_current_state())[alive], s[alive])
    e_o = np.abs(_np(out["obs0"][T - 1]) - obs[0])[alive].max()
    print(f"set {name} rollout_actor with noise {kind}/{layout}: action {worst_a:.2e} state {e_s:.2e} rows {e_o:.2e} reward {worst_r:.2e}, {int(alive.sum())}/{n} in regime")
    assert alive.mean() > 0.5
    assert worst_a <= 2e-5 and e_s <= (2e-6 if layout == "f64" else 1e-5) and e_o <= 2e-5 and worst_r <= 2e-5


# phase boundaries of the stateful generator per mode (take-off: ramp end, manual entry; landing: ramp end, landed; stay: manual
# entry; circle: run-up end, circle end, manual entry)
PHASE_BOUNDARIES = {2: 2, 3: 2, 4: 1, 5: 3}
# start heights: the first puts the ramp's end on a whole number of calls at 250 AND 400 Hz (4 s; 0.5 s), the others do not
STATEFUL_Z0 = {2: (-0.3, -0.4, -0.25, -0.31234), 3: (-0.75, -1.25, -0.5, -0.61357), 4: (-0.3, 0.2, 0.0, -0.1), 5: (0.0, -0.2, 0.1, -0.05)}
STATEFUL_SPEED = {2: 0.05, 3: 1.0, 4: 0.0, 5: 0.4}      # the generator's own speed in the mode: |v| of the bound |v| dt


@pytest.mark.parametrize("mode", [2, 3, 4, 5])
@pytest.mark.parametrize("freq", [250, 400])
def test_stateful_goal_modes_off_the_default_rate(freq, mode):
    """qr_get_desired in the stateful modes (take-off, landing, stay, circle) at 250 and 400 Hz, call by call against traj_oracle
    under the same dt, the vehicle following the goal it was given (x = xd + vd dt, v = vd of the call before), so that way-point and
    cut-off tests are met and every phase is reached — the circle through both circles into manual mode.  The device clocks its
    phases with t = calls * dt in float32, the reference accumulates float64 t += dt (quadrotor_hip.h, deviation 2 of the stateful
    modes): at a phase boundary the two may switch one call apart, and the goal then differs by at most one call's worth of motion,
    |v| dt.  Asserted: the bound at every call; every other call exact (GOAL_BAR = 3e-6 of test_gpu_evaluate_oracle.py, all fifteen
    goal words); and the calls that use the bound: at most one per phase boundary per env."""
    from gym_rotor_amd.constants import QuadConstants
    c = QuadConstants(freq=freq)
    z0, speed, bar = STATEFUL_Z0[mode], STATEFUL_SPEED[mode], 3e-6
    n = len(z0)
    state = np.zeros((n, 18)); state[:, 6] = state[:, 10] = state[:, 14] = 1.0
    state[:, 0:2] = (0.1, -0.2)
    state[:, 2] = z0
    end = {2: max(abs(-0.5 - z) for z in z0) / 0.05, 3: max(abs(-0.25 - z) for z in z0) / 1.0, 4: 0.0, 5: 0.7 / 0.4 + 2 * 2 * np.pi / 0.4}[mode]
    calls = int(end * freq) + 60
    env = _env("decoupled", n, c, 10.0, goal_mode=mode, layout="f64", use_UDM=False)
    env.set_state(state)
    env.mark_traj_start()
    used, worst_x, worst_exact = np.zeros(n, int), 0.0, 0.0
    with orc.constants(c):
        assert orc.DT == 1.0 / freq
        tr = trj.traj_start_batch(state, mode)
        for k in range(calls):
            got = _np(torch.cat(env.get_desired(), 1)).astype(np.float64)     # xd, vd, b1d, b1d_dot, Wd
            want = np.concatenate(trj.get_desired_batch(tr, state), 1)
            err = np.abs(got - want)
            ex = err[:, 0:3].max(1)
            assert (ex <= speed * c.dt + bar).all(), (k, ex)
            off = err.max(1) > bar
            used += off
            worst_x, worst_exact = max(worst_x, ex.max()), max(worst_exact, err[~off].max() if (~off).any() else 0.0)
            state = state.copy()
            state[:, 0:3] = cc.f32r(got[:, 0:3] + got[:, 3:6] * c.dt)      # the vehicle follows the goal it was given, one call of its
            state[:, 3:6] = got[:, 3:6]                                    # velocity ahead (the landing's cut-off test needs x beyond it)
            env.set_state(state)
        flags = _np(env._traj[3]).astype(int)
    print(f"stateful mode {mode} at {freq} Hz: {calls} calls, calls using the bound per env {used.tolist()}, worst position difference {worst_x:.2e} m "
          f"(bound {speed * c.dt:.1e}), other calls {worst_exact:.2e}; flags {flags.tolist()}")
    assert (used <= PHASE_BOUNDARIES[mode]).all(), used
    want_flags = tr["started"] * 1 + tr["complete"] * 2 + tr["manual"] * 4 + tr["manual_init"] * 8 + tr["landed"] * 16
    assert np.array_equal(flags, want_flags) and (want_flags & 2).all(), "every env reached the end of its trajectory, as the oracle's generator did"


@pytest.mark.parametrize("count", [1.0, 0.5])
@pytest.mark.parametrize("name", SETS)
def test_eight_curve_standalone_past_its_end(name, count, golden):
    """qr_get_desired, mode 6, with the set's eight-curve values and dt and a small eight_count (0.5: not a whole number), called
    past eight_count * eight_T: the goal is held from there on.  Against traj_oracle under the same values; goal words within
    GOAL_BAR (3e-6, test_gpu_evaluate_oracle.py), relative to the largest value of the word over the batch where that exceeds 1
    (the curve's amplitudes and speeds: A1 to 1.8 m, A2 w2 to 2.2 m/s)."""
    import dataclasses
    c, udm, cw, kw = cc.coeff_set(golden(f"onestep_coeffs_{name}"))
    c = dataclasses.replace(c, eight_count=count)
    n = 130
    rng = np.random.default_rng(5)
    with orc.constants(**orc.overrides_of(c)):
        state = cc.state_in(orc.sample_reset_state(rng, n, "train"))
        env = _env("coupled", n, c, udm, goal_mode=6, use_UDM=False)
        env.set_state(state, integ=np.zeros((n, 8)))
        env.mark_traj_start()
        tr = trj.traj_start_batch(state, 6)
        calls = int(1.5 * count * c.eight_T * c.freq)
        worst, held = 0.0, 0
        prev = None
        for k in range(calls):
            got = _np(torch.cat(env.get_desired(), 1)).astype(np.float64)
            want = np.concatenate(trj.get_desired_batch(tr, state), 1)
            scale = np.maximum(1.0, np.abs(want).max(0))
            worst = max(worst, (np.abs(got - want) / scale).max())
            if prev is not None and (k + 1) * c.dt > count * c.eight_T + c.dt:
                held += 1
                assert np.array_equal(got, prev), "the goal is held past the curve's end"
            prev = got
    print(f"set {name} eight curve count {count}: {worst:.2e} over {calls} calls, {held} held")
    assert held > 0.3 * calls and worst <= 3e-6


# ---------------------------------------------------------------------------------------------------------------------
# d. both reset samplers
# ---------------------------------------------------------------------------------------------------------------------
def _check_reset_distribution(s, p, c, udm, n):
    """test_reset_distribution_and_determinism / test_in_launch_reset_pool_distribution at the scaled ranges: |v| <= v_lim / 2,
    |W| <= W_lim / 2 with the observed maxima within 2 % of the bound and the spread of a uniform; parameters within nominal
    (1 +- udm), c_tw half of that, spread width / sqrt 3 within 3 %.  The position range (0.6 m) and the attitude range (50 deg) are
    the reference's literals (quad.py:343-356): they do not move with x_lim or euler_lim."""
    width = udm / 100 * np.array([1, 1, 1, 1, 1, 0.5])
    rel = p / c.nominal_params - 1.0
    assert (np.abs(rel) <= width * (1 + 1e-5) + 1e-7).all()
    assert np.allclose(rel.mean(0), 0, atol=0.03 * width.max()) and np.allclose(rel.std(0), width / np.sqrt(3), rtol=0.03)
    zero = np.abs(s[:, 0:6]).max(1) == 0
    assert abs(zero.mean() - 0.2) < 0.01
    nz = ~zero
    for sl, bound in ((slice(0, 3), 0.6), (slice(3, 6), c.v_lim / 2), (slice(15, 18), c.W_lim / 2)):
        m = np.abs(s[nz, sl]).max()
        assert 0.98 * bound < m <= bound * (1 + 1e-6), (sl, m, bound)
        col = s[nz, sl.start + 1]
        assert abs(col.mean()) < 0.02 * bound and abs(col.std() - bound / np.sqrt(3)) < 0.02 * bound
    R = np.swapaxes(s[:, 6:15].astype(np.float64).reshape(n, 3, 3), 1, 2)
    roll = np.arctan2(R[:, 2, 1], R[:, 2, 2]); pitch = -np.arcsin(np.clip(R[:, 2, 0], -1, 1))
    lim = np.deg2rad(50.0)
    assert np.abs(roll).max() <= lim + 1e-6 and np.abs(pitch).max() <= lim + 1e-6 and np.abs(roll).max() > 0.98 * lim and np.abs(pitch).max() > 0.98 * lim


@pytest.mark.parametrize("name", SETS)
def test_reset_samplers_under_coefficient_sets(name, golden):
    """reset('train'), reset('eval') and the in-launch reset (auto_reset=True, every env crashed) with every coefficient moved."""
    c, udm, cw, kw = cc.coeff_set(golden(f"onestep_coeffs_{name}"))
    n = 64 * 2000
    env = _env("coupled", n, c, udm, cw, seed=11, auto_reset=True, obs_rows=True)
    env.reset("train")
    _check_reset_distribution(_np(env.get_current_state()), _np(env.params).astype(np.float64), c, udm, n)
    # the in-launch reset: every env put far outside the arena, one step, all re-sampled
    env.get_norm_error_state()
    before = _np(env.get_current_state())
    st = before.copy(); st[:, 0] = 5.0 * c.x_lim
    env.set_state(st)
    _, _, done, _, _ = env.step(torch.zeros(n, 4, device="cuda"))
    assert bool(done.all())
    s2, p2 = _np(env.get_current_state()), _np(env.params).astype(np.float64)
    assert np.abs(s2[:, 0]).max() <= 0.6 and (s2[:, 0:6] != before[:, 0:6]).any(1).mean() > 0.79     # every env re-drawn (a fifth at the origin at rest, like some before)
    _check_reset_distribution(s2, p2, c, udm, n)
    # eval reset: the new nominals exactly (as float32), x ~ U(+-0.4) whatever x_lim, everything else at rest
    se = _np(env.reset("eval"))
    assert 0.39 < np.abs(se[:, 0:3]).max() <= 0.4 and np.abs(se[:, 3:6]).max() == 0 and np.abs(se[:, 15:18]).max() == 0
    assert np.array_equal(_np(env.params), np.tile(c.nominal_params.astype(np.float32), (n, 1)))
    # without domain randomisation: no parameter buffer, and a step flies the set's nominal vehicle (the oracle's, under the set)
    e2 = _env("coupled", 4096, c, udm, cw, seed=3, use_UDM=False, obs_rows=True)
    s0 = _np(e2.reset("train")).astype(np.float64)
    assert e2.params is None
    full = _np(e2.get_current_state())
    e2.get_norm_error_state()
    a = np.zeros((4096, 4), np.float32)
    e2.step(torch.from_numpy(a).cuda())
    with orc.constants(**kw):
        first = orc.error_obs_batch("coupled", full)
        want = orc.step_batch("coupled", full, a.astype(np.float64), None, None, first["integ"])
    assert grouped_rel_err(_np(e2.get_current_state()), want["state"]) <= cc.ONESTEP_TOL[("mixed", 1)]
    assert np.abs(s0[:, 3:6]).max() <= c.v_lim / 2 * (1 + 1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# e. marshalling
# ---------------------------------------------------------------------------------------------------------------------
def test_op_coeffs_carry_every_field_by_name(golden):
    """The float list the torch custom ops receive (env._op_coeffs) against the struct the ctypes path passes, field by field and
    by name, and against the set's own values: nothing swapped, nothing left at a default."""
    from gym_rotor_amd import _lib, torch_ops as ops
    c, udm, cw, kw = cc.coeff_set(golden("onestep_coeffs_A"))
    env = _env("decoupled", 64, c, udm, cw, w_adapt=12.5)
    names = [n for n, _ in _lib.QrCoeffs._fields_]
    assert names == ops._COEFF_NAMES and len(env._op_coeffs) == len(names) == 34
    want = dict(CW=cw, dt=1.0 / c.freq, euler_lim_deg=c.euler_lim, udm_fraction=udm / 100, w_adapt=12.5)
    for name, v in zip(names, env._op_coeffs):
        assert v == getattr(env._cenv.coeffs, name), name
        assert v == float(want[name] if name in want else getattr(c, name)), name
    dflt = _lib.default_coeffs()
    assert all(v != getattr(dflt, n) for n, v in zip(names, env._op_coeffs)), "set A moves every field"
    assert len(set(zip(env._op_coeffs, env._op_coeffs[1:]))) == 33 and all(a != b for a, b in zip(env._op_coeffs, env._op_coeffs[1:]))


# ---------------------------------------------------------------------------------------------------------------------
# f. the launch rule reads W_lim
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_launch_rule_follows_w_lim(kind):
    """With in-launch resets the rate-adaptive kernel is compiled in only where an in-regime env could reach it: 2.5 W_lim > w_adapt
    (wants_adapt).  W_lim = 5.1: the plain kernel.  W_lim = 4 pi: the rate-adaptive one, and while every env is in regime (|W|
    below w_adapt; the envs are re-sampled at 4 pi) its results are the plain kernel's (w_adapt = 0):
    * qr_rollout_actor (the wrappers): bit for bit — in regime it runs the plain kernel's code path;
    * qr_rollout on given actions: the rate-adaptive instantiation forms its quaternion stages in delta form (qr_step.h:
      kDelta), so not the same bits; the bars of test_adaptive_kernel_in_regime's free run apply until the first differing done flag
      (after it the two runs re-sample different envs)."""
    from gym_rotor_amd.constants import QuadConstants
    n, T, A = 1000, 100, orc.ACTION_DIM[kind]
    lo, hi = QuadConstants(W_lim=5.1), QuadConstants(W_lim=4 * math.pi)
    assert _env(kind, n, lo, 10.0, auto_reset=True).launch_plan()["adapt"] == 0
    assert _env(kind, n, lo, 10.0, auto_reset=True).launch_plan(T)["adapt"] == 0
    acts = (torch.rand(T, n, A, device="cuda", generator=torch.Generator("cuda").manual_seed(9)) * 2 - 1) * 0.3
    out, pol = [], []
    for w_adapt in (16.0, 0.0):
        env = _env(kind, n, hi, 10.0, seed=4, auto_reset=True, w_adapt=w_adapt)
        assert env.launch_plan(T)["adapt"] == (1 if w_adapt else 0) and env.launch_plan()["adapt"] == (1 if w_adapt else 0)
        env.reset("train")
        sd = env.state_dict()
        ro = env.rollout(acts)
        out.append((_np(env.get_current_state()), _np(ro["reward"]), _np(ro["terminated"])))
        if kind != "quad":
            import test_gpu_evaluate_oracle as ev
            env.load_state_dict(sd)
            assert env.launch_plan(T, actor="ppo")["adapt"] == (1 if w_adapt else 0)
            env.get_norm_error_state()
            ra = env.rollout_actor(ev._actors(kind, 6), T, deterministic=True)
            torch.cuda.synchronize()
            pol.append([_np(env.get_current_state()), _np(env.integ)] + [_np(ra[k]) for k in ("obs0", "obs1", "action", "reward", "terminated") if k in ra])
    assert np.abs(out[0][0][:, 15:18]).max() < 16.0
    if pol:
        assert np.abs(pol[0][0][:, 15:18]).max() < 16.0 and pol[0][-1].any(), "in regime, and some env was re-sampled"
        assert all(np.array_equal(x, y) for x, y in zip(*pol)), "rollout_actor: the rate-adaptive kernel in regime is the plain one, bit for bit"
    differs = (out[0][2] != out[1][2]).reshape(T, -1).any(1)
    t_same = int(np.argmax(differs)) if differs.any() else T
    # (T // 2: a margin measured with this seed, not a bound — on an MI355X no done flag differed in any of the 100 steps)
    assert t_same >= T // 2, f"done flags part at step {t_same}"
    e_r = np.abs(out[0][1][:t_same] - out[1][1][:t_same]).max()
    print(f"W_lim 4 pi, {kind}: adaptive against plain kernel, rewards {e_r:.2e} over {t_same} steps")
    assert e_r <= 1e-5
    if t_same == T:
        assert grouped_rel_err(out[0][0], out[1][0]) <= 1e-6
