"""Agent k's TD3 actor half under the centralized (CTDE) critic on the device (ctde_dpg_actor_kernel + dpg_reduce_kernel:
qr_ctde_dpg_actor_grad; dpg_actor_grad_ctde, td3_actor_loss_ctde) against the reference's float64 autograd
(tests/golden/ctde_actor.npz) and the float64 restatement of tests/ctde_actor_ref.py.

The bar, per tensor and statistic (twinq_gpu_util.bar): err <= max(2e-6 * max(1, |x64|), e32), e32 = the error of eager
float32 torch autograd of the same CTDE update on the same inputs on this device, no factor on it.  ReLU's gradient jumps where a
pre-activation crosses 0, so every gradient comparison runs on rows of a fixture case (all of which keep |z| >= 2e-5 in float64,
asserted again here for exactly the rows used).  B <= 130 everywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctde_actor_ref as R  # noqa: E402
from ctde_actor_ref import ACTOR_NAMES, CASES, Q1_NAMES  # noqa: E402
from test_ctde_critic_host import _Td3Actor, _Twin  # noqa: E402
from twinq_gpu_util import _cuda, _idx, _np, bar  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
LIB_NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b")
DIMS = ((15, 16, 4), (3, 4, 1))


@pytest.fixture(scope="module")
def cases():
    g = R.load()
    return {n: R.case(g, n) for n in CASES}


def _actors(c):
    from gym_rotor_amd import ActorParams
    return [None if R.actor_of(c, m) is None else ActorParams(*[_cuda(t) for t in R.actor_of(c, m)], None) for m in (0, 1)]


def _critic(c, q2_scale=1.0):
    """The twin critic: Q1 from the fixture, Q2 = Q1's tensors scaled (never read by the actor half)."""
    from gym_rotor_amd import QCriticParams
    q1 = [_cuda(t) for t in R.q1_of(c)]
    return QCriticParams(*q1, *[(t * q2_scale).contiguous() for t in q1], c["c_fc1_w"].shape[1] - c["obs0"].shape[1] - c["obs1"].shape[1])


def _rows_of(c, key, index):
    """A by-position tensor of the fixture for the minibatch `index` (None: all rows)."""
    return None if key not in c else _cuda(c[key] if index is None else c[key][np.asarray(index)])


def run(c, index=None, lam=None, critic=None, actors=None, obs=None, obs_next="own", noise="own", nominal="own", action_other="own", **kw):
    """dpg_actor_grad_ctde on a fixture case in its own form; action_other: "own" (the case's, by position), a tensor, or None."""
    from gym_rotor_amd import dpg_actor_grad_ctde
    k = c["k"]
    lam = c["lam"] if lam is None else lam
    if isinstance(obs_next, str):
        obs_next = [None, None]
        obs_next[k] = _cuda(c[f"obs_next{k}"])
    own = lambda v, key: _cuda(c[key], torch.float32) if isinstance(v, str) else v
    ao = _rows_of(c, "action_other", index) if isinstance(action_other, str) else action_other
    grads, stats = dpg_actor_grad_ctde(actors or _actors(c), critic or _critic(c), obs or (_cuda(c["obs0"]), _cuda(c["obs1"])), obs_next, _idx(index), k=k,
                                       action_other=ao, lam_T=lam[0], lam_S=lam[1], lam_M=lam[2], max_action=c["max_action"], noise=own(noise, "noise"),
                                       nominal=own(nominal, "nominal"), **kw)
    torch.cuda.synchronize()
    return grads, stats


def _pi(w, x):
    return torch.tanh(torch.relu(torch.relu(x @ w[0].T + w[1]) @ w[2].T + w[3]) @ w[4].T + w[5])


def torch_ctde(c, dtype, index=None, lam=None):
    """Eager torch autograd of the CTDE actor update on the device in `dtype` (index clones, both actors, two cat, Q1, three more passes of
    agent k's actor, backward): what e32 is measured with.  Returns (grads of agent k, stats, the other agent's action as Q1 read it)."""
    idx = np.arange(130) if index is None else np.asarray(index)
    lam = c["lam"] if lam is None else lam
    k, ma = c["k"], c["max_action"]
    w = [None if R.actor_of(c, m) is None else [_cuda(t, dtype).requires_grad_() for t in R.actor_of(c, m)] for m in (0, 1)]
    q = [_cuda(t, dtype) for t in R.q1_of(c)]
    x = [_cuda(c[f"obs{m}"][idx], dtype) for m in (0, 1)]
    xn = _cuda(c[f"obs_next{k}"][idx], dtype)
    mu = _pi(w[k], x[k])
    a = [None, None]
    a[k] = mu.clamp(-ma, ma)
    a[1 - k] = _pi(w[1 - k], x[1 - k]).clamp(-ma, ma) if w[1 - k] is not None else _cuda(c["action_other"][idx], dtype)
    sa = torch.cat([torch.cat(x, 1), torch.cat(a, 1)], 1)
    q1 = torch.relu(torch.relu(sa @ q[0].T + q[1]) @ q[2].T + q[3]) @ q[4].T + q[5]
    mse = torch.nn.functional.mse_loss
    reg = (lam[0] * mse(a[k], _pi(w[k], xn).clamp(-ma, ma)) + lam[1] * mse(a[k], _pi(w[k], x[k] + _cuda(c["noise"], dtype)[None, :]).clamp(-ma, ma))
           + lam[2] * mse(a[k], _cuda(c["nominal"], dtype)[None, :].expand_as(a[k])))
    loss = -q1.mean() + reg
    loss.backward()
    grads = {n: _np(t.grad).astype(np.float64) for n, t in zip(ACTOR_NAMES, w[k])}
    stats = np.array([loss.item(), q1.mean().item(), (mu.abs() > ma).double().mean().item(), float(reg.detach())], dtype=np.float64)
    return grads, stats, a[1 - k].detach()


def check(label, c, grads, stats, index=None, lam=None, g64=None, s64=None):
    """Gradients and statistics within the bar of the float64 values (default: the restatement on rows `index`), after the margin of
    exactly these rows has been asserted; the clamp share exactly.  Prints and returns the worst err / bar."""
    idx = np.arange(130) if index is None else np.asarray(index)
    lam = c["lam"] if lam is None else lam
    assert R.case_margin(c, idx) >= R.MARGIN
    if g64 is None:
        s64, g64 = R.case_f64(c, idx, lam)
    g32, s32, _ = torch_ctde(c, torch.float32, index, lam)
    worst = (0.0, "", 0.0, 0.0)
    for n, ln in zip(ACTOR_NAMES, LIB_NAMES):
        want = np.asarray(g64[n], dtype=np.float64)
        got = _np(grads[ln]).astype(np.float64).reshape(want.shape)
        assert np.isfinite(got).all(), (label, n)
        e32, err = float(np.abs(g32[n] - want).max()), float(np.abs(got - want).max())
        worst = max(worst, (err / bar(want, e32), n, err, e32))
    st = _np(stats).astype(np.float64)
    assert np.isfinite(st).all(), label
    for j, n in enumerate(R.STATS):
        e32, err = abs(s32[j] - s64[j]), abs(st[j] - s64[j])
        worst = max(worst, (err / bar(s64[j], e32), n, err, float(e32)))
    assert _np(stats)[2] == np.float32(s64[2]), (label, "the clamp share is an exact count")
    print(f"ctde actor {label}: worst err / bar = {worst[0]:.3f} at {worst[1]} (err {worst[2]:.3e}, e32 {worst[3]:.3e})")
    assert worst[0] <= 1.0, (label, worst)
    return worst[0]


def _same(a, b):
    return all(torch.equal(a[0][n], b[0][n]) for n in LIB_NAMES) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------------
# qr_ctde_dpg_actor_grad
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_against_the_reference_float64_in_both_forms(cases, name):
    c = cases[name]
    k = c["k"]
    ref = dict(g64={n: c["g_" + n] for n in ACTOR_NAMES}, s64=np.array([float(c[key]) for key in R.STATS]))
    grads, stats = run(c)
    assert all(grads[ln].shape == c[f"a{k}_{n}"].shape for n, ln in zip(ACTOR_NAMES, LIB_NAMES)) and stats.shape == (4,)
    check(name, c, grads, stats, **ref)
    if name not in R.SUPPLIED:
        # the supplied form, fed with eager torch's float32 action of the other agent: within the bar (its tanh is not the kernel's)
        a_other = torch_ctde(c, torch.float32)[2].contiguous()
        actors = _actors(c)
        actors[1 - k] = None
        check(name + " (other action supplied)", c, *run(c, actors=actors, action_other=a_other), **ref)


def test_each_coefficient_alone_and_zero_coefficients_skip_their_inputs(cases):
    for name in ("k0", "k1"):
        c = cases[name]
        for lam in ((0.4, 0.0, 0.0), (0.0, 0.3, 0.0), (0.0, 0.0, 0.6)):
            check(f"{name} lam={lam}", c, *run(c, lam=lam), lam=lam)
    for name in ("noreg", "k1"):
        c = cases[name]
        z = (0.0, 0.0, 0.0)
        base = run(c, lam=z, obs_next=None, noise=None, nominal=None)
        assert _same(base, run(c, lam=z))                                 # obs_next, noise and nominal passed, all lam = 0
        nan = lambda key: torch.full_like(_cuda(c[key], torch.float32), float("nan"))
        nxt = [nan("obs_next0"), nan("obs_next1")]
        assert _same(base, run(c, lam=z, obs_next=nxt, noise=nan("noise"), nominal=nan("nominal")))   # ... and never read
        assert float(base[1][3]) == 0.0 and float(base[1][0]) == -float(base[1][1])
        check(name + " all lam = 0", c, *base, lam=z)


def _guarded(c, need):
    k = c["k"]
    grads = {ln: torch.full((c[f"a{k}_{n}"].size + 2,), SENTINEL, device="cuda") for n, ln in zip(ACTOR_NAMES, LIB_NAMES)}
    return grads, torch.full((6,), SENTINEL, device="cuda"), torch.full((need // 8 + 2,), SENTINEL, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name", ("k0", "k1", "sat0", "sat1", "w28a", "w28b"))
def test_batch_sizes_into_guarded_buffers(cases, name):
    from gym_rotor_amd import dpg_actor_workspace_bytes_ctde
    c = cases[name]
    for B in (1, 63, 64, 65, 130):
        idx = np.arange(130 - B, 130)
        g, stats, ws = _guarded(c, dpg_actor_workspace_bytes_ctde(c["k"], 62, B))
        run(c, idx, grads={n: t[1:-1] for n, t in g.items()}, stats=stats[1:-1], workspace=ws[1:-1])
        for n, t in g.items():
            assert t[0] == SENTINEL and t[-1] == SENTINEL, (name, B, n)
        assert stats[0] == SENTINEL and stats[-1] == SENTINEL and ws[0] == SENTINEL and ws[-1] == SENTINEL
        check(f"{name} B={B}", c, {n: t[1:-1] for n, t in g.items()}, stats[1:-1], idx)


@pytest.mark.parametrize("name", ("k0", "k1"))
def test_refuses_a_short_workspace_and_writes_nothing(cases, name):
    from gym_rotor_amd import dpg_actor_workspace_bytes_ctde
    c = cases[name]
    need = dpg_actor_workspace_bytes_ctde(c["k"], 62, 130)
    g, stats, ws = _guarded(c, need)
    short = ws.view(torch.uint8)[8:8 + need - 1]                                                        # one byte short, 8-byte aligned
    with pytest.raises(ValueError, match="QR_E_SIZE"):
        run(c, grads={n: t[1:-1] for n, t in g.items()}, stats=stats[1:-1], workspace=short)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in g.values()) and (stats == SENTINEL).all() and (ws == SENTINEL).all()


@pytest.mark.parametrize("name", ("k0", "k1", "w28b"))
def test_index_forms(cases, name):
    c = cases[name]
    k = c["k"]
    rng = np.random.default_rng(4)
    base = run(c)
    assert _same(run(c, np.arange(130)), base)                                                          # identity: the same bits
    perm = rng.permutation(130)
    check(name + " permuted", c, *run(c, perm), perm)
    rep = np.concatenate([np.full(40, 17), np.arange(30), np.full(7, 129)])
    check(name + " repeated", c, *run(c, rep), rep)
    wild = np.array([-1, 130, 5, 10 ** 12, -10 ** 12, 129] * 12)
    ao = _rows_of(c, "action_other", np.clip(wild, 0, 129))                                             # by position: the same tensor for both
    assert _same(run(c, wild, action_other=ao), run(c, np.clip(wild, 0, 129), action_other=ao))         # clamped: the same bits
    # only the rows the index names are read: NaN everywhere else, and in all of the other agent's obs_next
    part = rng.permutation(130)[:70]
    obs, nxt = [_cuda(c["obs0"]), _cuda(c["obs1"])], [_cuda(c["obs_next0"]), _cuda(c["obs_next1"])]
    want = run(c, part)
    rest = torch.ones(130, dtype=torch.bool, device="cuda")
    rest[_idx(part)] = False
    obs[0][rest], obs[1][rest], nxt[k][rest] = float("nan"), float("nan"), float("nan")
    nxt[1 - k][:] = float("nan")
    assert _same(run(c, part, obs=obs, obs_next=nxt), want)
    check(name + " 70 of 130 rows", c, *want, part)


@pytest.mark.parametrize("name", ("k0", "k1"))
def test_grids_are_deterministic_and_agree(cases, name):
    c = cases[name]
    runs = {}
    for mw in (1, 2, 3, 0):
        a, b = run(c, max_workgroups=mw), run(c, max_workgroups=mw)
        assert _same(a, b), mw                                                                          # equal inputs and grid: equal bits
        check(f"{name} max_workgroups={mw}", c, *a)
        runs[mw] = a
    assert _same(runs[3], runs[0])                                                                      # 130 rows are three tiles


@pytest.mark.parametrize("name", ("k0", "k1"))
def test_gradients_do_not_depend_on_what_is_not_read(cases, name):
    c = cases[name]
    k = c["k"]
    base = run(c)
    assert _same(base, run(c, critic=_critic(c, q2_scale=float("nan"))))                                # Q2 NaN
    critic = _critic(c)
    q = critic.as_c()
    for n in ("fc4_w", "fc4_b", "fc5_w", "fc5_b", "fc6_w", "fc6_b"):
        setattr(q, n, None)
    critic.as_c = lambda: q                                                                             # Q2 = NULL at the C entry
    assert _same(base, run(c, critic=critic))
    actors = _actors(c)
    actors[1 - k].log_std = torch.full((DIMS[1 - k][2],), float("nan"), device="cuda")                  # the other actor's log_std
    assert _same(base, run(c, actors=actors))
    nxt = [_cuda(c["obs_next0"]), _cuda(c["obs_next1"])]
    nxt[1 - k][:] = float("nan")                                                                        # the other agent's obs_next
    assert _same(base, run(c, obs_next=nxt))
    assert all(torch.isfinite(base[0][n]).all() for n in LIB_NAMES)


@pytest.mark.parametrize("name", ("k1", "w28a"))
def test_torch_op_gives_the_ctypes_path_bits(cases, name):
    c = cases[name]
    k = c["k"]
    actors, critic = _actors(c), _critic(c)
    index = np.random.default_rng(5).permutation(130)[:100]
    grads, stats = run(c, index)
    g_op, s_op = [torch.zeros_like(getattr(actors[k], n)) for n in LIB_NAMES], torch.zeros(4, device="cuda")
    lists = [[] if a is None else [getattr(a, n) for n in LIB_NAMES] for a in actors]
    torch.ops.gym_rotor_amd.qr_ctde_dpg_actor_grad(lists[0], lists[1], [getattr(critic, n) for n in critic.NAMES], k, _cuda(c["obs0"]), _cuda(c["obs1"]),
                                                   _cuda(c[f"obs_next{k}"]), _idx(index), _rows_of(c, "action_other", index), _cuda(c["noise"]),
                                                   _cuda(c["nominal"], torch.float32), g_op, s_op, *c["lam"], c["max_action"])
    torch.cuda.synchronize()
    assert all(torch.equal(a, grads[n]) for a, n in zip(g_op, LIB_NAMES)) and torch.equal(s_op, stats)


# ------------------------------------------------------------------------------------------------------------------------
# td3_actor_loss_ctde, and the written-out loop
# ------------------------------------------------------------------------------------------------------------------------
def _fill(m, tensors, names=ACTOR_NAMES):
    with torch.no_grad():
        for n, t in zip(names, tensors):
            getattr(getattr(m, n[:3]), "weight" if n.endswith("w") else "bias").copy_(torch.from_numpy(t))
    return m.cuda()


def _live(c):
    """Both live actors, the centralized twin critic (Q2 as torch initialised it) and a two-agent buffer holding the case's rows."""
    from gym_rotor_amd import ReplayBuffer
    actors = [_fill(_Td3Actor(*DIMS[m]), R.actor_of(c, m)) for m in (0, 1)]
    critic = _fill(_Twin(23, c["c_fc1_w"].shape[0]), R.q1_of(c), Q1_NAMES)
    buf = ReplayBuffer(130, [15, 3], [4, 1], "cuda")
    for m in (0, 1):
        buf.obs[m].copy_(_cuda(c[f"obs{m}"]))
        buf.obs_next[m].copy_(_cuda(c[f"obs_next{m}"]))
    buf.count, buf.current_size = 0, 130
    return actors, critic, buf


@pytest.mark.parametrize("name", ("k0", "k1", "sat1"))
def test_td3_actor_loss_ctde_end_to_end(cases, name):
    from gym_rotor_amd import td3_actor_loss_ctde
    c = cases[name]
    k = c["k"]
    actors, critic, buf = _live(c)
    other = list(actors[1 - k].parameters())
    other[0].grad = torch.full_like(other[0], 3.5)
    held = [p.grad for p in other]
    kw = dict(lam_T=c["lam"][0], lam_S=c["lam"][1], lam_M=c["lam"][2], max_action=c["max_action"], noise=_cuda(c["noise"]), nominal=_cuda(c["nominal"], torch.float32))
    stats = td3_actor_loss_ctde(actors, critic, buf, k, None, **kw)
    torch.cuda.synchronize()
    grads = {ln: getattr(getattr(actors[k], n[:3]), "weight" if n.endswith("w") else "bias").grad for n, ln in zip(ACTOR_NAMES, LIB_NAMES)}
    assert all(g.shape == c[f"a{k}_{n}"].shape for (ln, g), n in zip(grads.items(), ACTOR_NAMES))
    check(name + " (live modules)", c, grads, stats)
    before, s0 = {n: g.clone() for n, g in grads.items()}, stats.clone()
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    stats2 = td3_actor_loss_ctde(actors, critic, buf, k, None, **kw)                                    # allocates nothing, the same bits
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem
    assert stats2.data_ptr() == stats.data_ptr() and torch.equal(stats2, s0) and all(torch.equal(grads[n], before[n]) for n in LIB_NAMES)
    # the other agent's actor: its .grad objects are the ones they were, with the values they had
    assert all(a is b for a, b in zip(held, (p.grad for p in other))) and all(g is None for g in held[1:]) and bool((held[0] == 3.5).all())
    assert all(torch.equal(p.data, _cuda(t)) for p, t in zip(other, R.actor_of(c, 1 - k)))


def _q1_of_pi_f64(actors, critic, obs):
    """mean Q1([obs_0 | obs_1 | pi_0 | pi_1]) recomputed in float64 on the CPU from the weights."""
    w = [[_np(p.data).astype(np.float64) for p in a.parameters()] for a in actors]
    q = [_np(p.data).astype(np.float64) for p in critic.parameters()][:6]
    x = [_np(o).astype(np.float64) for o in obs]
    a = [np.clip(R.actor_pass(w[m], x[m])[2], -1.0, 1.0) for m in (0, 1)]
    return float(R.q1_and_dqda(q, np.concatenate(x, 1), np.concatenate(a, 1))[2].mean())


@pytest.mark.parametrize("k", (0, 1))
def test_one_written_out_ctde_iteration(k):
    from gym_rotor_amd import ActorParams, DeviceAdamW, QuadVecEnv, ReplayBuffer, RolloutStorage, soft_update, td3_actor_loss_ctde, td3_critic_loss_ctde
    T, N, B = 4, 64, 64
    torch.manual_seed(31 + k)
    env = QuadVecEnv("decoupled", N, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=100, seed=21)
    env.reset("train")
    mk = lambda: ([_Td3Actor(*d).cuda() for d in DIMS], _Twin(23, 62).cuda())
    (actors, critic), (actors_t, critic_t) = mk(), mk()
    for a, t in zip(actors + [critic], actors_t + [critic_t]):
        t.load_state_dict(a.state_dict())
    storage = RolloutStorage(env, T)
    storage.set_initial_obs(env.get_norm_error_state())
    env.rollout_actor([ActorParams.from_td3_module(a, 0.1) for a in actors], T, out=storage.horizon(), noise_seed=5)
    buf = ReplayBuffer(1000, env.obs_dims, [4, 1], "cuda")
    buf.add(storage)
    g = torch.Generator(device="cuda").manual_seed(2)
    idx = buf.sample(B, g)
    eps = (torch.randn(B, 4, device="cuda", generator=g), torch.randn(B, 1, device="cuda", generator=g))
    cp = list(critic.parameters())
    for p in list(actors[k].parameters()) + cp:
        p.grad = torch.zeros_like(p)
    copts = [DeviceAdamW(cp[:6], lr=1e-3, max_norm=-1), DeviceAdamW(cp[6:], lr=1e-3, max_norm=-1)]
    aopt = DeviceAdamW(list(actors[k].parameters()), lr=1e-4, max_norm=-1)
    obs = [buf.obs[m][idx] for m in (0, 1)]
    other = [p.data.clone() for p in actors[1 - k].parameters()]
    td3_critic_loss_ctde(critic, critic_t, actors_t, buf, k, idx, noise=eps)
    DeviceAdamW.step_all(copts)
    torch.cuda.synchronize()
    q_before = _q1_of_pi_f64(actors, critic, obs)
    stats = td3_actor_loss_ctde(actors, critic, buf, k, idx, lam_T=0.0, lam_S=0.0, lam_M=0.0)
    aopt.step()
    torch.cuda.synchronize()
    q_after = _q1_of_pi_f64(actors, critic, obs)
    print(f"ctde iteration k={k}: mean Q1(obs, pi(obs)) {q_before:.8f} -> {q_after:.8f} (stats {stats.tolist()})")
    assert abs(float(stats[1]) - q_before) <= 1e-5 * max(1.0, abs(q_before)) and q_after > q_before
    before = [p.data.clone() for p in actors_t[k].parameters()]
    soft_update([critic, actors[k]], [critic_t, actors_t[k]], 0.005)
    assert all(not torch.equal(a, b.data) for a, b in zip(before, actors_t[k].parameters()))
    assert all(torch.equal(a, p.data) for a, p in zip(other, actors[1 - k].parameters())) and all(p.grad is None for p in actors[1 - k].parameters())


@pytest.mark.parametrize("name", ("k0", "k1"))
def test_actor_update_captured_in_a_graph_replays_the_eager_bits(cases, name):
    from gym_rotor_amd import DeviceAdamW, soft_update, td3_actor_loss_ctde
    c = cases[name]
    k = c["k"]

    def fresh():
        actors, critic, buf = _live(c)
        actor_t = _Td3Actor(*DIMS[k]).cuda()
        actor_t.load_state_dict(actors[k].state_dict())
        for p in actors[k].parameters():
            p.grad = torch.zeros_like(p)
        return actors, critic, actor_t, DeviceAdamW(list(actors[k].parameters()), lr=1e-3, max_norm=-1), buf

    kw = dict(noise=_cuda(c["noise"]), nominal=_cuda(c["nominal"], torch.float32))

    def chain(actors, critic, actor_t, opt, buf):
        td3_actor_loss_ctde(actors, critic, buf, k, None, **kw)
        opt.step()
        soft_update(actors[k], actor_t, 0.005)

    eager = fresh()
    for _ in range(3):
        chain(*eager)
    torch.cuda.synchronize()
    cap = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(*cap)                                                   # the first of the three eagerly: the caches are filled outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # a single chain of launches, no parallel branches
        chain(*cap)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip((p for m in (eager[0][k], eager[2]) for p in m.parameters()), (p for m in (cap[0][k], cap[2]) for p in m.parameters())):
        assert torch.equal(a.data, b.data)
    assert not torch.equal(next(eager[0][k].parameters()).data, _cuda(c[f"a{k}_fc1_w"]))                # (and the three steps did move the actor)
