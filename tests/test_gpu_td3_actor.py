"""The TD3 actor half on the device (dpg_actor_kernel + dpg_reduce_kernel: qr_dpg_actor_grad; soft_update_kernel: qr_soft_update;
td3_actor_loss, soft_update) against the reference's float64 autograd (tests/golden/td3_actor.npz) and the float64 restatement of
tests/td3_actor_ref.py.

The bar, per tensor and statistic: err <= max(2e-6 * max(1, |x64|), e32), e32 = the error of eager float32 torch autograd on the same
inputs on this device.  ReLU's gradient jumps where a pre-activation crosses 0, so every gradient comparison runs on rows of a fixture
case (all of which keep |z| >= 2e-5 in float64, asserted again here for the rows used)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import td3_actor_ref as R  # noqa: E402
from td3_actor_ref import ACTOR_NAMES, CASES, Q1_NAMES  # noqa: E402
from test_td3_critic_host import _Actor, _Twin  # noqa: E402
from twinq_gpu_util import _cuda, _idx, _np, bar  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
LIB_NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b")


@pytest.fixture(scope="module")
def cases():
    g = R.load()
    return {n: R.case(g, n) for n in CASES}


def _actor(c):
    from gym_rotor_amd import ActorParams
    return ActorParams(*[_cuda(c["a_" + n]) for n in ACTOR_NAMES], None)


def _critic(c, q2_scale=1.0):
    """The twin critic: Q1 from the fixture, Q2 = Q1's tensors scaled (never read by the actor half)."""
    from gym_rotor_amd import QCriticParams
    q1 = [_cuda(c["c_" + n]) for n in Q1_NAMES]
    return QCriticParams(*q1, *[(t * q2_scale).contiguous() for t in q1], c["a_fc3_w"].shape[0])


def run(c, index=None, lam=None, critic=None, obs=None, obs_next="own", noise="own", nominal="own", **kw):
    from gym_rotor_amd import dpg_actor_grad
    lam = c["lam"] if lam is None else lam
    own = lambda v, k: _cuda(c[k], torch.float32) if isinstance(v, str) else v
    grads, stats = dpg_actor_grad(_actor(c), critic or _critic(c), _cuda(c["obs"]) if obs is None else obs, own(obs_next, "obs_next"), _idx(index),
                                  lam_T=lam[0], lam_S=lam[1], lam_M=lam[2], max_action=c["max_action"], noise=own(noise, "noise"),
                                  nominal=own(nominal, "nominal"), **kw)
    torch.cuda.synchronize()
    return grads, stats


def torch_dpg(c, dtype, index=None, lam=None):
    """Eager torch autograd on the device in `dtype` (index clones + three actor passes + Q1 + backward): what e32 is measured with."""
    idx = np.arange(130) if index is None else np.asarray(index)
    lam = c["lam"] if lam is None else lam
    ma = c["max_action"]
    w = [_cuda(c["a_" + n], dtype).requires_grad_() for n in ACTOR_NAMES]
    q = [_cuda(c["c_" + n], dtype) for n in Q1_NAMES]
    pi = lambda x: torch.tanh(torch.relu(torch.relu(x @ w[0].T + w[1]) @ w[2].T + w[3]) @ w[4].T + w[5])
    x, xn = _cuda(c["obs"][idx], dtype), _cuda(c["obs_next"][idx], dtype)
    mu = pi(x)
    a = mu.clamp(-ma, ma)
    sa = torch.cat([x, a], 1)
    q1 = torch.relu(torch.relu(sa @ q[0].T + q[1]) @ q[2].T + q[3]) @ q[4].T + q[5]
    mse = torch.nn.functional.mse_loss
    reg = (lam[0] * mse(a, pi(xn).clamp(-ma, ma)) + lam[1] * mse(a, pi(x + _cuda(c["noise"], dtype)[None, :]).clamp(-ma, ma))
           + lam[2] * mse(a, _cuda(c["nominal"], dtype)[None, :].expand_as(a)))
    loss = -q1.mean() + reg
    loss.backward()
    grads = {n: _np(t.grad).astype(np.float64) for n, t in zip(ACTOR_NAMES, w)}
    return grads, np.array([loss.item(), q1.mean().item(), (mu.abs() > ma).double().mean().item(), float(reg.detach())], dtype=np.float64)


def check(label, c, grads, stats, index=None, lam=None, g64=None, s64=None):
    """Gradients and statistics within the bar of the float64 values (default: the restatement on rows `index`), after the margin of
    exactly these rows has been asserted; the clamp share exactly.  Prints and returns the worst err / bar."""
    idx = np.arange(130) if index is None else np.asarray(index)
    lam = c["lam"] if lam is None else lam
    w, q = [c["a_" + n] for n in ACTOR_NAMES], [c["c_" + n] for n in Q1_NAMES]
    assert R.margins(w, q, c["obs"][idx], c["obs_next"][idx], c["noise"], c["max_action"])[0] >= R.MARGIN
    if g64 is None:
        s64, g64 = R.dpg_actor_grad_f64(w, q, c["obs"][idx], c["obs_next"][idx], c["noise"], c["nominal"], lam, c["max_action"])
    g32, s32 = torch_dpg(c, torch.float32, index, lam)
    worst = (0.0, "", 0.0, 0.0)
    for n, ln in zip(ACTOR_NAMES, LIB_NAMES):
        want = np.asarray(g64[n], dtype=np.float64)
        got = _np(grads[ln]).astype(np.float64).reshape(want.shape)
        assert np.isfinite(got).all(), (label, n)
        e32, err = float(np.abs(g32[n] - want).max()), float(np.abs(got - want).max())
        worst = max(worst, (err / bar(want, e32), n, err, e32))
    st = _np(stats).astype(np.float64)
    assert np.isfinite(st).all(), label
    for k, n in enumerate(R.STATS):
        e32, err = abs(s32[k] - s64[k]), abs(st[k] - s64[k])
        worst = max(worst, (err / bar(s64[k], e32), n, err, float(e32)))
    assert _np(stats)[2] == np.float32(s64[2]), (label, "the clamp share is an exact count")
    print(f"dpg actor {label}: worst err / bar = {worst[0]:.3f} at {worst[1]} (err {worst[2]:.3e}, e32 {worst[3]:.3e})")
    assert worst[0] <= 1.0, (label, worst)
    return worst[0]


def _same(a, b):
    return all(torch.equal(a[0][n], b[0][n]) for n in LIB_NAMES) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------------
# qr_dpg_actor_grad
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_against_the_reference_float64(cases, name):
    c = cases[name]
    grads, stats = run(c)
    assert all(grads[ln].shape == c["a_" + n].shape for n, ln in zip(ACTOR_NAMES, LIB_NAMES)) and stats.shape == (4,)
    s64 = np.array([float(c[k]) for k in R.STATS])
    check(name, c, grads, stats, g64={n: c["g_" + n] for n in ACTOR_NAMES}, s64=s64)


def test_zero_coefficients_skip_their_inputs_bit_for_bit(cases):
    c = cases["noreg"]
    base = run(c, obs_next=None, noise=None, nominal=None)
    assert _same(base, run(c))                                       # obs_next, noise and nominal passed, all lam = 0
    nan = lambda k: torch.full_like(_cuda(c[k], torch.float32), float("nan"))
    assert _same(base, run(c, obs_next=nan("obs_next"), noise=nan("noise"), nominal=nan("nominal")))   # ... and never read
    assert float(base[1][3]) == 0.0 and float(base[1][0]) == -float(base[1][1])
    m = cases["mono"]
    for lam in ((0.4, 0.0, 0.0), (0.0, 0.3, 0.0), (0.0, 0.0, 0.6)):  # each term alone
        check(f"mono lam={lam}", m, *run(m, lam=lam), lam=lam)


def _guarded(c, need):
    grads = {ln: torch.full((c["a_" + n].size + 2,), SENTINEL, device="cuda") for n, ln in zip(ACTOR_NAMES, LIB_NAMES)}
    return grads, torch.full((6,), SENTINEL, device="cuda"), torch.full((need // 8 + 2,), SENTINEL, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name", ("mono", "dtde1", "sat"))
def test_batch_sizes_into_guarded_buffers(cases, name):
    from gym_rotor_amd.td3 import dpg_actor_workspace_bytes
    c = cases[name]
    dims = (c["obs"].shape[1], c["a_fc1_w"].shape[0], c["a_fc3_w"].shape[0])
    for B in (1, 63, 64, 65, 130):
        idx = np.arange(130 - B, 130)
        g, stats, ws = _guarded(c, dpg_actor_workspace_bytes(dims, 62, B))
        run(c, idx, grads={n: t[1:-1] for n, t in g.items()}, stats=stats[1:-1], workspace=ws[1:-1])
        for n, t in g.items():
            assert t[0] == SENTINEL and t[-1] == SENTINEL, (name, B, n)
        assert stats[0] == SENTINEL and stats[-1] == SENTINEL and ws[0] == SENTINEL and ws[-1] == SENTINEL
        check(f"{name} B={B}", c, {n: t[1:-1] for n, t in g.items()}, stats[1:-1], idx)


def test_index_forms(cases):
    c = cases["mono"]
    rng = np.random.default_rng(4)
    base = run(c)
    assert _same(run(c, np.arange(130)), base)                                                          # identity: the same bits
    perm = rng.permutation(130)
    check("permuted", c, *run(c, perm), perm)
    rep = np.concatenate([np.full(40, 17), np.arange(30), np.full(7, 129)])
    check("repeated", c, *run(c, rep), rep)
    wild = np.array([-1, 130, 5, 10 ** 12, -10 ** 12, 129] * 12)
    assert _same(run(c, wild), run(c, np.clip(wild, 0, 129)))                                           # clamped: the same bits
    # only the rows the index names are read: NaN everywhere else
    part = rng.permutation(130)[:70]
    obs, nxt = _cuda(c["obs"]), _cuda(c["obs_next"])
    want = run(c, part)
    rest = torch.ones(130, dtype=torch.bool, device="cuda")
    rest[_idx(part)] = False
    obs[rest], nxt[rest] = float("nan"), float("nan")
    assert _same(run(c, part, obs=obs, obs_next=nxt), want)
    check("70 of 130 rows", c, *want, part)


def test_grids_are_deterministic_and_agree(cases):
    c = cases["mono"]
    runs = {}
    for mw in (1, 2, 3, 0):
        a, b = run(c, max_workgroups=mw), run(c, max_workgroups=mw)
        assert _same(a, b), mw                                                                          # equal inputs and grid: equal bits
        check(f"max_workgroups={mw}", c, *a)
        runs[mw] = a
    assert _same(runs[3], runs[0])                                                                      # 130 rows are three tiles


def test_refuses_a_short_workspace_and_writes_nothing(cases):
    from gym_rotor_amd.td3 import dpg_actor_workspace_bytes
    c = cases["mono"]
    need = dpg_actor_workspace_bytes((23, 16, 4), 62, 130)
    g, stats, ws = _guarded(c, need)
    short = ws.view(torch.uint8)[8:8 + need - 1]                                                        # one byte short, 8-byte aligned
    with pytest.raises(ValueError, match="QR_E_SIZE"):
        run(c, grads={n: t[1:-1] for n, t in g.items()}, stats=stats[1:-1], workspace=short)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in g.values()) and (stats == SENTINEL).all() and (ws == SENTINEL).all()


def test_gradients_do_not_depend_on_q2(cases):
    c = cases["mono"]
    base = run(c)
    assert _same(base, run(c, critic=_critic(c, q2_scale=-3.5)))
    critic = _critic(c)
    q = critic.as_c()
    for n in ("fc4_w", "fc4_b", "fc5_w", "fc5_b", "fc6_w", "fc6_b"):
        setattr(q, n, None)
    critic.as_c = lambda: q                                                                             # Q2 = NULL at the C entry
    assert _same(base, run(c, critic=critic))


def test_torch_ops_give_the_ctypes_path_bits(cases):
    c = cases["dtde0"]
    actor, critic = _actor(c), _critic(c)
    idx = _idx(np.random.default_rng(5).permutation(130)[:100])
    grads, stats = run(c, _np(idx))
    g_op, s_op = [torch.zeros_like(getattr(actor, n)) for n in LIB_NAMES], torch.zeros(4, device="cuda")
    torch.ops.gym_rotor_amd.qr_dpg_actor_grad([getattr(actor, n) for n in LIB_NAMES], [getattr(critic, n) for n in critic.NAMES], 4, _cuda(c["obs"]),
                                              _cuda(c["obs_next"]), idx, _cuda(c["noise"]), _cuda(c["nominal"], torch.float32), g_op, s_op, *c["lam"], c["max_action"])
    torch.cuda.synchronize()
    assert all(torch.equal(a, grads[n]) for a, n in zip(g_op, LIB_NAMES)) and torch.equal(s_op, stats)
    from gym_rotor_amd import soft_update
    p, t = [torch.randn(7, 5, device="cuda"), torch.randn(3, device="cuda")], [torch.randn(7, 5, device="cuda"), torch.randn(3, device="cuda")]
    t2 = [x.clone() for x in t]
    soft_update(p, t, 0.25)
    torch.ops.gym_rotor_amd.qr_soft_update(p, t2, 0.25)
    assert all(torch.equal(a, b) for a, b in zip(t, t2))


# ------------------------------------------------------------------------------------------------------------------------
# qr_soft_update
# ------------------------------------------------------------------------------------------------------------------------
def _modules(seed):
    torch.manual_seed(seed)
    return _Twin().cuda(), _Actor().cuda()


def test_soft_update_of_an_actor_and_a_twin_critic_in_one_launch():
    from gym_rotor_amd import soft_update
    (critic, actor), (critic_t, actor_t) = _modules(1), _modules(2)
    params = [p.data for m in (critic, actor) for p in m.parameters()]
    assert len(params) == 18
    # every target inside a guarded buffer
    bufs = [torch.full((p.numel() + 2,), SENTINEL, device="cuda") for p in params]
    targets = [b[1:-1] for b in bufs]
    for t, m in zip(targets, (p.data for m in (critic_t, actor_t) for p in m.parameters())):
        t.copy_(m.reshape(-1))
    before_p, before_t = [p.clone() for p in params], [t.clone() for t in targets]
    for tau in (0.005, 0.5):
        want = [R.soft_update_f32(_np(p).reshape(-1), _np(t), tau) for p, t in zip(params, targets)]
        soft_update(params, targets, tau)
        torch.cuda.synchronize()
        for k, (t, w) in enumerate(zip(targets, want)):
            assert np.array_equal(_np(t).view(np.uint32), w.view(np.uint32)), (tau, k)
    assert all(b[0] == SENTINEL and b[-1] == SENTINEL for b in bufs)
    assert all(torch.equal(p, q) for p, q in zip(params, before_p))                                     # params are read only
    for t, b in zip(targets, before_t):
        t.copy_(b)
    soft_update(params, targets, 0.0)
    assert all(torch.equal(t.view(torch.int32), b.view(torch.int32)) for t, b in zip(targets, before_t))  # tau = 0 leaves the bits
    soft_update(params, targets, 1.0)
    assert all(torch.equal(t, p.reshape(-1)) for t, p in zip(targets, params))                          # tau = 1 copies
    # modules as they are, the reference's loop as the yardstick
    ref = [t.data.clone() for m in (critic_t, actor_t) for t in m.parameters()]
    for p, t in zip(params, ref):
        t.copy_(0.005 * p + (1 - 0.005) * t)
    soft_update([critic, actor], [critic_t, actor_t])
    assert all(torch.equal(t.data, r) for t, r in zip((t for m in (critic_t, actor_t) for t in m.parameters()), ref))
    # one large tensor: more entries than one sweep of the grid
    p, t = torch.randn(300_001, device="cuda"), torch.randn(300_001, device="cuda")
    want = R.soft_update_f32(_np(p), _np(t), 0.005)
    soft_update([p], [t], 0.005)
    assert np.array_equal(_np(t).view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------
# td3_actor_loss, and the written-out loop
# ------------------------------------------------------------------------------------------------------------------------
def _fill(m, c, prefix, names):
    with torch.no_grad():
        for n in names:
            getattr(getattr(m, n[:3]), "weight" if n.endswith("w") else "bias").copy_(torch.from_numpy(c[prefix + n]))
    return m.cuda()


def _buffer(c):
    from gym_rotor_amd import ReplayBuffer
    buf = ReplayBuffer(130, [c["obs"].shape[1]], [c["a_fc3_w"].shape[0]], "cuda")
    buf.obs[0].copy_(_cuda(c["obs"]))
    buf.obs_next[0].copy_(_cuda(c["obs_next"]))
    buf.count, buf.current_size = 0, 130
    return buf


@pytest.mark.parametrize("name", ("mono", "dtde0", "dtde1"))
def test_td3_actor_loss_end_to_end(cases, name):
    from gym_rotor_amd import td3_actor_loss
    c = cases[name]
    D, H, A = c["obs"].shape[1], c["a_fc1_w"].shape[0], c["a_fc3_w"].shape[0]
    actor, critic, buf = _fill(_Actor(D, H, A), c, "a_", ACTOR_NAMES), _fill(_Twin(D + A, 62), c, "c_", Q1_NAMES), _buffer(c)
    kw = dict(lam_T=c["lam"][0], lam_S=c["lam"][1], lam_M=c["lam"][2], max_action=c["max_action"], noise=_cuda(c["noise"]), nominal=_cuda(c["nominal"], torch.float32))
    stats = td3_actor_loss(actor, critic, buf, 0, None, **kw)
    torch.cuda.synchronize()
    grads = {ln: getattr(getattr(actor, n[:3]), "weight" if n.endswith("w") else "bias").grad for n, ln in zip(ACTOR_NAMES, LIB_NAMES)}
    assert all(g.shape == c["a_" + n].shape for (ln, g), n in zip(grads.items(), ACTOR_NAMES))
    check(name + " (end to end)", c, grads, stats)
    before, s0 = {n: g.clone() for n, g in grads.items()}, stats.clone()
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    stats2 = td3_actor_loss(actor, critic, buf, 0, None, **kw)                                          # allocates nothing, the same bits
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem
    assert stats2.data_ptr() == stats.data_ptr() and torch.equal(stats2, s0) and all(torch.equal(grads[n], before[n]) for n in LIB_NAMES)


def _q1_of_pi(actor, critic, obs):
    with torch.no_grad():
        a = torch.tanh(actor.fc3(torch.relu(actor.fc2(torch.relu(actor.fc1(obs)))))).clamp(-1, 1)
        return float(critic.fc3(torch.relu(critic.fc2(torch.relu(critic.fc1(torch.cat([obs, a], 1)))))).double().mean())


def test_collect_sample_and_two_whole_td3_iterations():
    from gym_rotor_amd import (ActorParams, DeviceAdamW, QuadVecEnv, ReplayBuffer, RolloutStorage, soft_update, td3_actor_loss, td3_critic_loss)
    T, N = 3, 70
    torch.manual_seed(11)
    env = QuadVecEnv("coupled", N, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=100, seed=21)
    env.reset("train")
    actor, critic, actor_t, critic_t = _Actor().cuda(), _Twin().cuda(), _Actor().cuda(), _Twin().cuda()
    actor_t.load_state_dict(actor.state_dict())
    critic_t.load_state_dict(critic.state_dict())
    storage = RolloutStorage(env, T)
    storage.set_initial_obs(env.get_norm_error_state())
    env.rollout_actor([ActorParams.from_td3_module(actor, 0.1)], T, out=storage.horizon(), noise_seed=5)
    buf = ReplayBuffer(1000, env.obs_dims, [4], "cuda")
    buf.add(storage)
    g = torch.Generator(device="cuda").manual_seed(2)
    idx = buf.sample(128, g)
    eps = torch.randn(128, 4, device="cuda", generator=g)
    noise, nominal = 0.05 * torch.randn(23, device="cuda", generator=g), torch.tensor([-0.3, 0.0, 0.0, 0.0], device="cuda")
    cp = list(critic.parameters())
    for p in list(actor.parameters()) + cp:
        p.grad = torch.zeros_like(p)
    copts = [DeviceAdamW(cp[:6], lr=1e-3, max_norm=-1), DeviceAdamW(cp[6:], lr=1e-3, max_norm=-1)]     # DeviceAdamW takes eight tensors
    aopt = DeviceAdamW(list(actor.parameters()), lr=1e-4, max_norm=-1)
    obs = buf.obs[0][idx]
    for it in range(2):
        td3_critic_loss(critic, critic_t, actor_t, buf, 0, idx, noise=eps)
        DeviceAdamW.step_all(copts)
        q_before = _q1_of_pi(actor, critic, obs)
        stats = td3_actor_loss(actor, critic, buf, 0, idx, lam_T=0.0, lam_S=0.0, lam_M=0.0, noise=noise, nominal=nominal)
        aopt.step()
        torch.cuda.synchronize()
        q_after = _q1_of_pi(actor, critic, obs)
        print(f"td3 iteration {it}: mean Q1(obs, pi(obs)) {q_before:.6f} -> {q_after:.6f} (stats {stats.tolist()})")
        assert abs(float(stats[1]) - q_before) <= 1e-5 * max(1.0, abs(q_before)) and q_after > q_before
        before = [p.data.clone() for p in actor_t.parameters()]
        soft_update([critic, actor], [critic_t, actor_t], 0.005)
        assert all(not torch.equal(a, b.data) for a, b in zip(before, actor_t.parameters()))
    assert torch.isfinite(td3_actor_loss(actor, critic, buf, 0, idx, noise=noise, nominal=nominal)).all()


def test_actor_update_captured_in_a_graph_replays_the_eager_bits(cases):
    from gym_rotor_amd import DeviceAdamW, soft_update, td3_actor_loss
    c = cases["mono"]

    def fresh():
        actor, critic = _fill(_Actor(), c, "a_", ACTOR_NAMES), _fill(_Twin(), c, "c_", Q1_NAMES)
        actor_t = _Actor().cuda()
        actor_t.load_state_dict(actor.state_dict())
        for p in actor.parameters():
            p.grad = torch.zeros_like(p)
        return actor, critic, actor_t, DeviceAdamW(list(actor.parameters()), lr=1e-3, max_norm=-1), _buffer(c)

    kw = dict(noise=_cuda(c["noise"]), nominal=_cuda(c["nominal"], torch.float32))

    def chain(actor, critic, actor_t, opt, buf):
        td3_actor_loss(actor, critic, buf, 0, None, **kw)
        opt.step()
        soft_update(actor, actor_t, 0.005)

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
    for a, b in zip((p for m in (eager[0], eager[2]) for p in m.parameters()), (p for m in (cap[0], cap[2]) for p in m.parameters())):
        assert torch.equal(a.data, b.data)
    assert not torch.equal(next(eager[0].parameters()).data, _cuda(c["a_fc1_w"]))                       # (and the three steps did move the actor)
