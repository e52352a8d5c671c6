"""Every episode start the device samples, against the value its key must give (tests/reset_ref.py: the NumPy restatement of
qr_rng.h's two Philox streams and of sample_start / make_pool; tests/test_reset_host.py checks the restatement itself).

x, v, W and the parameters are compared BIT FOR BIT (the sign of a zero included), the goal generator's draws through the bits of
the generator state they produce, R = Rz(yaw) Ry(pitch) Rx(roll) under the attitude bar: 4 x the float32 error of the restatement's
own plain-float32 composition on the same words (reset_ref.attitude_bar; + 16 * 2^-24 for layout 'f32'; never above 1e-5).
Nothing read back from the device feeds the reference except what forms the key: the episode and per-tile reset counters before the
launch, and the recorded terminated / truncated rows (a lane's pool slot is its rank among its tile's resetting lanes).  The goal
generator's state is compared between twins on the device, as it starts from theta_init = atan2_fast(...), which goes through
v_rcp_f32 and has no restatement; where mode 0's b1d is restated (reset_ref.mode0_b1d) it is from that float32.

Small throughout: 64 * 6 + 17 envs, a seed and (for qr_reset) an env offset with non-zero high words."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reset_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ("quad", "coupled", "decoupled")
N, SEED = RR.TEST_N, RR.TEST_SEED
TILES = (N + 63) // 64


def _env(kind, **kw):
    from gym_rotor_amd import QuadVecEnv
    kw.setdefault("seed", SEED)
    env = QuadVecEnv(kind, N, device="cuda", obs_rows=True, **kw)
    return env


def _np(t):
    return t.detach().cpu().numpy()


def _coeffs(env):
    return RR.coeffs(env.constants, env.UDM_percentage)


def _gid(env):
    return (np.arange(N, dtype=object) + env.env_offset).astype(np.uint64)


def _compare(env, idx, ref, label):
    """The envs `idx` of `env` against the restated starts `ref` (one row per entry of idx): bits of x, v, W and the parameters, R under
    the bar.  Prints the worst attitude error and its bar."""
    s = _np(env.get_current_state())[idx]
    want = RR.state_rows(ref)
    for name, sl in (("x", slice(0, 3)), ("v", slice(3, 6)), ("W", slice(15, 18))):
        eq = RR.bits_equal(s[:, sl], want[:, sl])
        assert eq.all(), (label, name, int((~eq).any(1).sum()), len(idx), idx[(~eq).any(1)][:5], s[(~eq).any(1)][:2, sl], want[(~eq).any(1)][:2, sl])
    if env.params is not None:
        p = _np(env.params)[idx]
        eq = RR.bits_equal(p, ref["params"])
        assert eq.all(), (label, "params", int((~eq).any(1).sum()), len(idx), p[(~eq).any(1)][:2], ref["params"][(~eq).any(1)][:2])
    e32, bar = RR.attitude_bar(ref, env.layout)
    err = float(np.abs(RR.rows_R(s) - ref["R"]).max())
    print(f"[attitude] {label}: rows {len(idx)} device error {err:.3e} bar {bar:.3e} (e32 {e32:.3e})")
    assert err <= bar, (label, err, bar)
    return err, bar


def _kill(env, kill):
    """Make the envs in `kill` terminate in the next step: x far outside the arena."""
    st = _np(env.get_current_state())
    st[kill, 0] = 5.0
    env.set_state(st, mask=torch.as_tensor(kill, device=env.device))


def _first_obs(env):
    if env.kind != "quad":
        env.get_norm_error_state()


# ---------------------------------------------------------------------------------------------------------------------
# 1. qr_reset
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["f64", "mixed", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_qr_reset_gives_the_start_of_its_key(kind, layout):
    """reset('train') at episode 1, a masked second reset (masked rows: episode 2; the others keep their bits), reset('eval'), for env
    offsets 0, 192 and 2^32 + 320 (the host takes a 64-bit offset: its high word is part of the key); then use_UDM=False, a
    non-default UDM_percentage and overridden v_lim / W_lim (reset_v, reset_W are half of them: tests/coeff_cases.py sets them so)."""
    from gym_rotor_amd.constants import QuadConstants
    rng = np.random.default_rng(11)
    for off in RR.TEST_OFFSETS:
        env = _env(kind, layout=layout, env_offset=off)
        c, gid, tag = _coeffs(env), _gid(env), f"qr_reset {kind} {layout} offset {off}"
        assert _np(env._episode).max() == 0
        env.reset("train")
        assert (_np(env._episode) == 1).all()
        every = np.arange(N)
        _compare(env, every, RR.start_from_words(RR.draw20_words(SEED, gid, 1), True, False, c), tag + " train")
        before, p_before = _np(env.get_current_state()), _np(env.params).copy()
        mask = rng.random(N) < 0.5
        mask[[0, 63, 64, N - 1]] = (True, False, True, True)
        env.reset("train", mask=torch.as_tensor(mask, device="cuda"))
        ep = _np(env._episode)
        assert np.array_equal(ep, 1 + mask.astype(np.int32))
        _compare(env, every, RR.start_from_words(RR.draw20_words(SEED, gid, ep), True, False, c), tag + " masked")
        after = _np(env.get_current_state())
        assert RR.bits_equal(after[~mask], before[~mask]).all() and RR.bits_equal(_np(env.params)[~mask], p_before[~mask]).all()
        assert (np.abs(after[mask][:, 16] - before[mask][:, 16]) > 0).mean() > 0.7      # (20 % start at rest: W = 0 both times)
        env.reset("eval")
        assert np.array_equal(_np(env._episode), ep + 1)
        _compare(env, every, RR.start_from_words(RR.draw20_words(SEED, gid, ep + 1), False, True, c), tag + " eval")
    off = RR.TEST_OFFSETS[1]
    variants = (("no UDM", dict(use_UDM=False)), ("UDM 13 %", dict(UDM_percentage=13.0)),
                ("v_lim 3.3 W_lim 5.1", dict(constants=QuadConstants(v_lim=3.3, W_lim=5.1, m_nominal=1.83, c_tw_nominal=2.6))))
    for name, kw in variants:
        env = _env(kind, layout=layout, env_offset=off, **kw)
        env.reset("train")
        c = _coeffs(env)
        ref = RR.start_from_words(RR.draw20_words(SEED, _gid(env), 1), env.use_UDM, False, c)
        assert (env.params is None) == (not env.use_UDM)
        _compare(env, np.arange(N), ref, f"qr_reset {kind} {layout} {name}")
    assert c["reset_v"] == np.float32(1.65) and c["reset_W"] == np.float32(2.55)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the in-launch pool, one-step launches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["helper", "plain", "f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_in_launch_pool_one_step(kind, variant):
    """Per tile 1, 12, 13, 64, 0 and 5 lanes (and the ragged tail's last three) killed at random positions: after one step each env
    that reset holds start_from_words(pool_words(seed, gfirst, count = the tile's counter before the step, slot = its rank)) — ranks up
    to 63, so passes 0..5 — and after a second step, with other lanes, the starts of count + 1.  Default layout under either choice of
    the launch rule (a helper wave that samples pass 0 and hands it over through LDS / the stepping wave alone), and the uniform
    layouts (which have the plain instantiation only); env offsets 0 and 128; without domain randomisation as well."""
    layout = variant if variant in ("f64", "f32") else "mixed"
    helper = {"helper": True, "plain": False}.get(variant)
    rng = np.random.default_rng(5 + KINDS.index(kind))
    zero = torch.zeros(N, 5 if kind == "decoupled" else 4, device="cuda")
    for off, udm in ((0, True), (128, True), (0, False)):
        env = _env(kind, layout=layout, env_offset=off, auto_reset=True, helper=helper, use_UDM=udm)
        if helper is not None:
            assert env.kernel_info()[2] == (128 if helper else 64)      # threads per workgroup: with / without the helper wave
        env.reset("train")
        _first_obs(env)
        c = _coeffs(env)
        for step in range(2):
            kill = RR.kill_rows(rng)
            rc, ep = _np(env._reset_count).copy(), _np(env._episode).copy()
            assert (rc == step).all()
            _kill(env, kill)
            _, _, done, _, _ = env.step(zero)
            rows = _np(done).reshape(N, -1).any(1)
            assert rows[kill].all() and rows.sum() <= kill.sum() + 8    # (an env may also end its episode by itself: it takes a slot too)
            assert np.array_equal(_np(env._episode), ep + rows) and (_np(env._reset_count) == step + 1).all()
            idx, gfirst, count, slot = RR.pool_keys(rows, off, rc)
            assert slot.max() == 63 and (np.bincount(slot // 12, minlength=6) > 0).all()
            ref = RR.start_from_words(RR.pool_words(SEED, gfirst, count, slot), udm, False, c, pool=True)
            _compare(env, idx, ref, f"pool one-step {kind} {variant} offset {off} UDM {udm} count {step}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the in-launch pool inside multi-step launches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("helper_rollout", [True, False])
@pytest.mark.parametrize("launch", ["rollout-quad", "rollout-coupled", "rollout_actor-coupled"])
def test_in_launch_pool_multi_step(launch, helper_rollout):
    """max_episode_steps = 4 and launches of T = 4 env-steps: the time limit ends every episode at the launch's last step, so the final
    state of each env that reset there is the start of count = (the tile's counter before the launch) + 3 — the helper wave samples
    that pool a step ahead — with ranks 0..63 in a whole tile; a second launch gives count + 7.  An env that crashed earlier in the
    launch does not reach the limit at t = 3: it is not compared, and the ranks come from the recorded terminated / truncated rows.
    qr_rollout on given actions (Quad-v0, coupled) and qr_rollout_actor with a zero-mean actor, under either launch-rule choice."""
    from gym_rotor_amd import policy
    what, kind = launch.split("-")
    T, off = 4, 128
    env = _env(kind, env_offset=off, auto_reset=True, max_episode_steps=T, helper_rollout=helper_rollout)
    env.reset("train")
    _first_obs(env)
    c = _coeffs(env)
    acts = torch.zeros(T, N, 4, device="cuda")
    if what == "rollout_actor":
        g = torch.Generator(device="cuda"); g.manual_seed(3)
        actors = policy.random_actors(kind, "cuda", generator=g, log_std=-1.0)
        for a in actors:
            a.mean_w.zero_(); a.mean_b.zero_()
    for n_launch in range(2):
        rc = _np(env._reset_count).copy()
        assert (rc == T * n_launch).all()
        out = env.rollout(acts) if what == "rollout" else env.rollout_actor(actors, T)
        assert (_np(env._reset_count) == rc + T).all()
        ended = _np(out["terminated"]).reshape(T, N, -1).any(2) | _np(out["truncated"]).astype(bool)
        rows = ended[T - 1]
        assert rows.mean() > 0.9
        idx, gfirst, count, slot = RR.pool_keys(rows, off, rc + (T - 1))
        assert slot.max() == 63                                         # a whole tile at once: passes 0..5
        ref = RR.start_from_words(RR.pool_words(SEED, gfirst, count, slot), True, False, c, pool=True)
        _compare(env, idx, ref, f"pool {launch} helper_rollout {helper_rollout} count rc + {T * n_launch + T - 1}")
        assert (_np(env.episode_steps)[rows] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the goal generator's draws (word 19)
# ---------------------------------------------------------------------------------------------------------------------
def _draw_tensors(draws, idx=None):
    """[N] float32 device tensors of traj_draws' three results (rows `idx` of an otherwise neutral batch)."""
    full = [np.zeros(N, np.float32), np.full(N, 3.0, np.float32), np.zeros(N, np.float32)]
    for f, d in zip(full, draws):
        f[slice(None) if idx is None else idx] = d
    return [torch.as_tensor(f, device="cuda") for f in full]


@pytest.mark.parametrize("goal_mode", [0, 1, 5])
def test_mark_traj_start_draws_are_word_19(goal_mode):
    """mark_traj_start() without draws on env A against a twin B handed traj_draws(draw20_words(seed, gid, episode)[:, 19]): equal
    generator state (and, for the stateful mode, goal buffer) in every bit.  Mode 0 reads theta_b1d, mode 1 t_traj and w_b1d; mode 5
    (stateful) reads none and must not care."""
    off = RR.TEST_OFFSETS[1]
    A, B = (_env("coupled", env_offset=off, goal_mode=goal_mode) for _ in range(2))
    for e in (A, B):
        e.reset("train")
    ep = _np(A._episode)
    assert (ep == 1).all()
    A.mark_traj_start()
    th, tt, wb = _draw_tensors(RR.traj_draws(RR.draw20_words(SEED, _gid(A), ep)[:, 19]))
    B._traj.fill_(7.0)                                          # (B's reset left the same rows there: make the call below write them)
    B.mark_traj_start(theta_b1d=th, t_traj=tt, w_b1d=wb)
    a, b = _np(A._traj), _np(B._traj)
    assert RR.bits_equal(a, b).all(), (goal_mode, int((~RR.bits_equal(a, b)).sum()))
    if goal_mode == 0:
        assert len(np.unique(a[2])) > 0.9 * N                   # (b1d_x: the draw reached the state)
        (c0, s0), _ = RR.mode0_b1d(a[1], RR.draw20_words(SEED, _gid(A), ep)[:, 19])   # qr_traj_start: the draw rounded, then the sum
        assert RR.bits_equal(a[2], c0).all() and RR.bits_equal(a[3], s0).all()
    if goal_mode == 1:
        assert len(np.unique(a[2])) > 0.9 * N and len(np.unique(a[3])) > 0.9 * N
    if A._goal is not None:
        assert RR.bits_equal(_np(A._goal), _np(B._goal)).all()
    # and a neutral draw gives another state: the comparison above can tell
    if goal_mode in (0, 1):
        B.mark_traj_start(theta_b1d=0.0 * th, t_traj=0.0 * tt + 3.0, w_b1d=0.0 * wb)
        assert (~RR.bits_equal(a, _np(B._traj))).any(0).mean() > 0.9


@pytest.mark.parametrize("goal_mode,helper", [(0, True), (0, False), (1, True), (1, False), (5, None)])
def test_in_launch_reset_goal_draws_are_the_pools_word_19(goal_mode, helper):
    """After an in-launch reset of killed lanes on env A (traj_start + the episode's first traj_goal, inside the step launch), a twin B
    takes A's state with set_state, then mark_traj_start with traj_draws(pool_words(...)[:, 19]), then one get_desired: the reset
    lanes' generator state is equal in every bit, all eight words — and, for the stateful mode, xd, vd, b1d of the goal buffer.
    Mode 0's b1d (words 2, 3) may take either of the two values its source admits, both words the same one (reset_ref.mode0_b1d:
    the step kernel is free to fuse theta_b1d's product into the sum under the sincos; the restated sincos_small is checked in
    every bit against the twin's unfused values first).  Not compared bit for bit: Wd (goal words 9..11) of the stateful mode, a float64 sum of products that the compiler may fuse
    differently in the step kernel and in qr_get_desired; it is held to 1e-6 instead."""
    off = 128
    A = _env("coupled", env_offset=off, goal_mode=goal_mode, auto_reset=True, helper=helper)
    B = _env("coupled", env_offset=off, goal_mode=goal_mode)
    if helper is not None:
        assert A.kernel_info()[2] == (128 if helper else 64)
    A.reset("train")
    _first_obs(A)
    kill = RR.kill_rows(np.random.default_rng(9 + goal_mode))
    rc = _np(A._reset_count).copy()
    _kill(A, kill)
    _, _, done, _, _ = A.step(torch.zeros(N, 4, device="cuda"))
    rows = _np(done).reshape(N, -1).any(1)
    assert rows[kill].all()
    idx, gfirst, count, slot = RR.pool_keys(rows, off, rc)
    words = RR.pool_words(SEED, gfirst, count, slot)
    _compare(A, idx, RR.start_from_words(words, True, False, _coeffs(A), pool=True), f"pool one-step coupled goal mode {goal_mode} helper {helper}")
    mask = torch.as_tensor(rows, device="cuda")
    B.reset("train")
    B.set_state(A.get_current_state())
    th, tt, wb = _draw_tensors(RR.traj_draws(words[:, 19]), idx)
    B.mark_traj_start(mask=mask, theta_b1d=th, t_traj=tt, w_b1d=wb)
    B.get_desired(mask=mask)
    a, b = _np(A._traj)[:, idx], _np(B._traj)[:, idx]
    eq = RR.bits_equal(a, b)
    if goal_mode == 0:
        # words 2, 3 = (cos, sin)(theta_init + theta_b1d): the source admits two roundings of the ARGUMENT (reset_ref.mode0_b1d) —
        # the twin, handed theta_b1d as a number, has the unfused one in every row; the step kernel may have either, both words alike
        (c0, s0), (c1, s1) = RR.mode0_b1d(b[1], words[:, 19])
        assert RR.bits_equal(b[2], c0).all() and RR.bits_equal(b[3], s0).all()
        unfused, fused = eq[2] & eq[3], RR.bits_equal(a[2], c1) & RR.bits_equal(a[3], s1)
        print(f"[mode 0] helper {helper}: rows {len(idx)} unfused {int(unfused.sum())} fused {int(fused.sum())} neither {int((~(unfused | fused)).sum())}")
        assert (unfused | fused).all(), (helper, a[:, ~(unfused | fused)][:4, :4], c0[~(unfused | fused)][:4], c1[~(unfused | fused)][:4])
        eq[2:4] = True
    assert eq.all(), (goal_mode, helper, int((~eq).any(0).sum()), np.flatnonzero((~eq).any(1)))
    assert (a[0] == 1.0).all()                                  # one get_desired into the new episode
    if goal_mode in (0, 1):
        assert len(np.unique(a[2])) > 0.9 * len(idx)
    if A._goal is not None:
        ga, gb = _np(A._goal)[:, idx], _np(B._goal)[:, idx]
        assert RR.bits_equal(ga[:9], gb[:9]).all()
        assert np.abs(ga[9:] - gb[9:]).max() <= 1e-6
