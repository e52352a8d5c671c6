"""The TD3 critic half on the device (td3_target_kernel: qr_twinq_target; twinq_kernel + twinq_reduce_kernel: qr_twinq_grad;
td3_critic_loss, ReplayBuffer) against the reference's float64 autograd (tests/golden/td3_critic.npz) and the float64 restatement
of tests/td3_ref.py.

The bar, per tensor and statistic: err <= max(2e-6 * max(1, |x64|), e32), e32 = the error of eager float32 torch on the same inputs
on this device.  ReLU's gradient jumps where a pre-activation crosses 0, so every gradient comparison runs on rows of a fixture case
(all of which keep |z| >= 2e-5 in float64, asserted again here for the rows used)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import td3_ref  # noqa: E402
from td3_ref import ACTOR_NAMES, NAMES  # noqa: E402
from test_td3_critic_host import CASES, _Actor, _Twin  # noqa: E402
from twinq_gpu_util import _cuda, _idx, _np, _q, _twin_module, bar, torch_twinq  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
STATS = ("loss", "mse1", "mse2", "mean_y")


@pytest.fixture(scope="module")
def cases():
    g = td3_ref.load()
    return {n: td3_ref.case(g, n) for n in CASES}


def _critic(c, prefix="c_"):
    from gym_rotor_amd import QCriticParams
    return QCriticParams(*[_cuda(c[prefix + n]) for n in NAMES], int(c["action_dim"]))


def _actor(c):
    from gym_rotor_amd import ActorParams
    return ActorParams(*[_cuda(c["a_" + n]) for n in ACTOR_NAMES], None) if "a_fc1_w" in c else None


def _tensors(c):
    return {"obs": _cuda(c["obs"]), "act": _cuda(c["action"]), "rwd": _cuda(c["reward"]), "obs_next": _cuda(c["obs_next"]), "done": _cuda(c["done"])}


def _scalars(c):
    return {k: float(c[k]) for k in ("discount", "target_noise", "noise_clip", "max_action")}


def run_target(c, index=None, eps="own", **over):
    from gym_rotor_amd import td3_target
    B = 130 if index is None else len(index)
    if isinstance(eps, str):
        eps = c.get("eps")
        eps = None if eps is None else (eps if index is None else eps[:B])
    kw = dict(_scalars(c), noise=None if eps is None else _cuda(eps))
    if "a_fc1_w" not in c:
        kw["action_next"] = _cuda(c["a_next_in"] if index is None else c["a_next_in"][:B])
    kw.update(over)
    y = td3_target(_actor(c), _critic(c, "t_"), _tensors(c), 0, _idx(index), **kw)
    torch.cuda.synchronize()
    return y


def run_twinq(c, y, index=None, critic=None, **kw):
    from gym_rotor_amd import twinq_grad
    grads, stats = twinq_grad(critic or _critic(c), _cuda(c["obs"]), _cuda(c["action"]), _cuda(np.asarray(y, dtype=np.float32)), _idx(index), **kw)
    torch.cuda.synchronize()
    return grads, stats


# ------------------------------------------------------------------------------------------------------------------------
# eager torch on the device, in a given dtype: what e32 is measured with
# ------------------------------------------------------------------------------------------------------------------------
def torch_target(c, dtype, index=None, eps=None, a_next=None):
    idx = np.arange(130) if index is None else np.asarray(index)
    on, r, d = (_cuda(c[k][idx], dtype) for k in ("obs_next", "reward", "done"))
    with torch.no_grad():
        if "a_fc1_w" in c:
            w = [_cuda(c["a_" + n], dtype) for n in ACTOR_NAMES]
            h = torch.relu(on @ w[0].T + w[1])
            a = torch.tanh(torch.relu(h @ w[2].T + w[3]) @ w[4].T + w[5])
            if eps is not None:
                a = a + (_cuda(eps, dtype) * float(c["target_noise"])).clamp(-float(c["noise_clip"]), float(c["noise_clip"]))
            a = a.clamp(-float(c["max_action"]), float(c["max_action"]))
        else:
            a = _cuda(a_next, dtype)
        m = _twin_module(c, "t_", dtype)
        sa = torch.cat([on, a], 1)
        y = r[:, None] + float(c["discount"]) * (1 - d[:, None]) * torch.min(_q(m, sa, 0), _q(m, sa, 1))
    return _np(y[:, 0]).astype(np.float64)


def check_y(label, y, y64, y32):
    got = _np(y).astype(np.float64)
    assert np.isfinite(got).all(), label
    err, e32 = float(np.abs(got - y64).max()), float(np.abs(y32 - y64).max())
    b = bar(y64, e32)
    print(f"td3 target {label}: err / bar = {err / b:.3f} (err {err:.3e}, e32 {e32:.3e})")
    assert err <= b, (label, err, b)


def check_grads(label, c, grads, stats, y32, index=None, g64=None, s64=None):
    """Gradients and statistics within the bar of the float64 values (default: the restatement on rows `index` against y32, the
    float32 target the launch was given), after the margin of exactly these rows has been asserted.  Prints the worst err / bar."""
    idx = np.arange(130) if index is None else np.asarray(index)
    w = [c["c_" + n] for n in NAMES]
    assert td3_ref.margin(w, c["obs"][idx], c["action"][idx]) >= td3_ref.MARGIN
    y32 = np.asarray(y32, dtype=np.float32)
    if g64 is None:
        loss, m1, m2, g64 = td3_ref.twinq_grad_f64(w, c["obs"][idx], c["action"][idx], y32)
        s64 = np.array([loss, m1, m2, y32.astype(np.float64).mean()])
    g32, s32 = torch_twinq(c, torch.float32, y32, index)
    worst = (0.0, "", 0.0, 0.0)
    for n in NAMES:
        want = np.asarray(g64[n], dtype=np.float64)
        got = _np(grads[n]).astype(np.float64).reshape(want.shape)
        assert np.isfinite(got).all(), (label, n)
        e32 = float(np.abs(g32[n].reshape(want.shape) - want).max())
        err = float(np.abs(got - want).max())
        worst = max(worst, (err / bar(want, e32), n, err, e32))
    st = _np(stats).astype(np.float64)
    assert np.isfinite(st).all(), label
    for q, n in enumerate(STATS):
        e32 = abs(s32[q] - s64[q])
        err = abs(st[q] - s64[q])
        worst = max(worst, (err / bar(s64[q], e32), n, err, float(e32)))
    print(f"twinq {label}: worst err / bar = {worst[0]:.3f} at {worst[1]} (err {worst[2]:.3e}, e32 {worst[3]:.3e})")
    assert worst[0] <= 1.0, (label, worst)


# ------------------------------------------------------------------------------------------------------------------------
# qr_twinq_target
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_target_fixture_cases_against_the_reference_float64(cases, name):
    c = cases[name]
    y = run_target(c)
    assert y.shape == (130,) and y.dtype == torch.float32
    check_y(name, y, c["y"], torch_target(c, torch.float32, eps=c.get("eps"), a_next=c.get("a_next_in")))


def test_target_without_noise_is_zero_noise_bit_for_bit(cases):
    for name in ("nonoise", "mono", "dtde1"):
        c = cases[name]
        assert torch.equal(run_target(c, eps=None), run_target(c, eps=np.zeros((130, int(c["action_dim"])), dtype=np.float32))), name
    assert not torch.equal(run_target(cases["mono"], eps=None), run_target(cases["mono"]))


def test_target_of_done_rows_is_the_reward_exactly(cases):
    for name in ("sat", "mono", "dtde1", "w28"):
        c = cases[name]
        y, done = _np(run_target(c)), c["done"] > 0
        assert done.sum() >= 3 and np.array_equal(y[done], c["reward"][done]), name
        assert not np.any(y[~done] == c["reward"][~done]), name


def test_target_reads_only_the_rows_the_index_names(cases):
    c = cases["mono"]
    idx = np.array([5, 7, 70, 129, 64, 63, 7])
    t = _tensors(c)
    want = run_target(c, idx)
    t["obs_next"][6] = float("nan")
    t["obs_next"][128, 3] = float("inf")
    t["rwd"][0] = float("nan")
    out = torch.full((len(idx) + 2,), SENTINEL, device="cuda")
    from gym_rotor_amd import td3_target
    td3_target(_actor(c), _critic(c, "t_"), t, 0, _idx(idx), noise=_cuda(c["eps"][:len(idx)]), out=out[1:-1], **_scalars(c))
    torch.cuda.synchronize()
    assert torch.equal(out[1:-1], want) and out[0] == SENTINEL and out[-1] == SENTINEL     # y untouched by the NaN rows, guards intact


@pytest.mark.parametrize("name", ("mono", "dtde1", "h5"))
def test_target_batch_sizes_into_guarded_outputs(cases, name):
    c = cases[name]
    full = _np(run_target(c, eps=None))
    for B in (1, 63, 64, 65, 130):
        idx = np.arange(130 - B, 130)
        out = torch.full((B + 2,), SENTINEL, device="cuda")
        run_target(c, idx, eps=None, out=out[1:-1])
        got = _np(out)
        assert got[0] == SENTINEL and got[-1] == SENTINEL and np.array_equal(got[1:-1], full[130 - B:]), (name, B)


def test_target_index_forms(cases):
    c = cases["mono"]
    rng = np.random.default_rng(3)
    base = run_target(c, None, eps=None)
    assert torch.equal(run_target(c, np.arange(130), eps=None), base)                                   # identity
    perm = rng.permutation(130)
    assert torch.equal(run_target(c, perm, eps=None), base[torch.from_numpy(perm).cuda()])               # y permutes with the index
    rep = np.array([3, 3, 3, 129, 0, 3])
    assert torch.equal(run_target(c, rep, eps=None), base[torch.from_numpy(rep).cuda()])                 # repeats
    wild = np.array([-1, 130, 5, 10 ** 12, -10 ** 12, 129])
    assert torch.equal(run_target(c, wild, eps=None), run_target(c, np.clip(wild, 0, 129), eps=None))    # clamped
    tail = np.arange(64, 130)
    assert torch.equal(run_target(c, tail, eps=None), base[64:])
    # the noise belongs to the minibatch position, not to the row
    eps = c["eps"]
    a = run_target(c, perm, eps=eps)
    y64 = td3_ref.td3_target_f64(c, perm, eps=eps)[1]
    check_y("permuted, noise by position", a, y64, torch_target(c, torch.float32, perm, eps=eps))


# ------------------------------------------------------------------------------------------------------------------------
# qr_twinq_grad
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_twinq_fixture_cases_against_the_reference_float64(cases, name):
    c = cases[name]
    y32 = c["y"].astype(np.float32)
    grads, stats = run_twinq(c, y32)
    s64 = np.array([c["loss"], c["mse1"], c["mse2"], c["y"].mean()], dtype=np.float64)
    check_grads(name, c, grads, stats, y32, g64={n: c["g_" + n] for n in NAMES}, s64=s64)


def _guarded(critic, B, need):
    grads = {n: torch.full((torch.Size(s).numel() + 2,), SENTINEL, device="cuda") for n, s in critic.shapes.items()}
    stats = torch.full((6,), SENTINEL, device="cuda")
    ws = torch.full((need // 8 + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    return grads, stats, ws


@pytest.mark.parametrize("name", ("mono", "dtde1", "h5"))
def test_twinq_batch_sizes_into_guarded_buffers(cases, name):
    from gym_rotor_amd.td3 import twinq_workspace_bytes
    c = cases[name]
    critic = _critic(c)
    for B in (1, 63, 64, 65, 130):
        idx = np.arange(130 - B, 130)
        y32 = c["y"][idx].astype(np.float32)
        g, stats, ws = _guarded(critic, B, twinq_workspace_bytes(critic.dims, B))
        run_twinq(c, y32, idx, critic, grads={n: t[1:-1] for n, t in g.items()}, stats=stats[1:-1], workspace=ws[1:-1])
        for n, t in g.items():
            assert t[0] == SENTINEL and t[-1] == SENTINEL, (name, B, n)
        assert stats[0] == SENTINEL and stats[-1] == SENTINEL and ws[0] == SENTINEL and ws[-1] == SENTINEL
        check_grads(f"{name} B={B}", c, {n: t[1:-1] for n, t in g.items()}, stats[1:-1], y32, idx)


def _same(a, b):
    return all(torch.equal(a[0][n], b[0][n]) for n in NAMES) and torch.equal(a[1], b[1])


def test_twinq_index_forms(cases):
    c = cases["mono"]
    rng = np.random.default_rng(4)
    y32 = c["y"].astype(np.float32)
    base = run_twinq(c, y32)
    assert _same(run_twinq(c, y32, np.arange(130)), base)                                               # identity: the same bits
    perm = rng.permutation(130)
    check_grads("permuted", c, *run_twinq(c, y32[perm], perm), y32[perm], perm)
    rep = np.concatenate([np.full(40, 17), np.arange(30), np.full(7, 129)])
    yr = rng.standard_normal(len(rep)).astype(np.float32)
    check_grads("repeated", c, *run_twinq(c, yr, rep), yr, rep)
    wild = np.array([-1, 130, 5, 10 ** 12, -10 ** 12, 129] * 12)
    yw = rng.standard_normal(len(wild)).astype(np.float32)
    assert _same(run_twinq(c, yw, wild), run_twinq(c, yw, np.clip(wild, 0, 129)))                       # clamped: the same bits
    tail = np.arange(64, 130)
    check_grads("rows [64, 130)", c, *run_twinq(c, y32[tail], tail), y32[tail], tail)


def test_twinq_grids_are_deterministic_and_agree(cases):
    c = cases["mono"]
    y32 = c["y"].astype(np.float32)
    runs = {}
    for mw in (1, 2, 3, 0):
        a, b = run_twinq(c, y32, max_workgroups=mw), run_twinq(c, y32, max_workgroups=mw)
        assert _same(a, b), mw                                                                          # equal inputs and grid: equal bits
        check_grads(f"max_workgroups={mw}", c, *a, y32)
        runs[mw] = a
    assert _same(runs[3], runs[0])                                                                      # 130 rows are three tiles


def test_twinq_refuses_a_short_workspace_and_writes_nothing(cases):
    from gym_rotor_amd.td3 import twinq_workspace_bytes
    c = cases["mono"]
    critic = _critic(c)
    need = twinq_workspace_bytes(critic.dims, 130)
    g, stats, ws = _guarded(critic, 130, need)
    short = ws.view(torch.uint8)[8:8 + need - 1]                                                        # one byte short, 8-byte aligned
    with pytest.raises(ValueError, match="QR_E_SIZE"):
        run_twinq(c, c["y"].astype(np.float32), None, critic, grads={n: t[1:-1] for n, t in g.items()}, stats=stats[1:-1], workspace=short)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in g.values()) and (stats == SENTINEL).all() and (ws == SENTINEL).all()


def test_q1_gradients_do_not_depend_on_q2(cases):
    c = cases["mono"]
    y32 = c["y"].astype(np.float32)
    base = run_twinq(c, y32)
    c2 = dict(c)
    for n in NAMES[6:]:
        c2["c_" + n] = (c["c_" + n] * 1.5 + 0.01).astype(np.float32)
    other = run_twinq(c2, y32)
    for n in NAMES[:6]:
        assert torch.equal(base[0][n], other[0][n]), n
    assert torch.equal(base[1][1], other[1][1]) and torch.equal(base[1][3], other[1][3])                 # Q1's mse and mean y
    assert not torch.equal(base[0]["fc5_w"], other[0]["fc5_w"]) and not torch.equal(base[1][2], other[1][2])


def test_torch_ops_give_the_ctypes_path_bits(cases):
    c = cases["dtde0"]
    t, critic, tcritic, actor = _tensors(c), _critic(c), _critic(c, "t_"), _actor(c)
    idx = _idx(np.random.default_rng(5).permutation(130)[:100])
    eps = _cuda(c["eps"][:100])
    y = run_target(c, _np(idx), eps=c["eps"][:100])
    y_op = torch.full((100,), SENTINEL, device="cuda")
    torch.ops.gym_rotor_amd.qr_twinq_target([getattr(actor, n) for n in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b")],
                                          [getattr(tcritic, n) for n in NAMES], 4, t["obs_next"], t["rwd"], t["done"], idx, eps, None, y_op,
                                          *[float(c[k]) for k in ("discount", "target_noise", "noise_clip", "max_action")])
    assert torch.equal(y_op, y)
    grads, stats = run_twinq(c, _np(y), _np(idx))
    g_op, s_op = [torch.zeros_like(getattr(critic, n)) for n in NAMES], torch.zeros(4, device="cuda")
    torch.ops.gym_rotor_amd.qr_twinq_grad([getattr(critic, n) for n in NAMES], 4, t["obs"], t["act"], y, idx, g_op, s_op)
    torch.cuda.synchronize()
    assert all(torch.equal(a, grads[n]) for a, n in zip(g_op, NAMES)) and torch.equal(s_op, stats)


# ------------------------------------------------------------------------------------------------------------------------
# td3_critic_loss, ReplayBuffer
# ------------------------------------------------------------------------------------------------------------------------
def _actor_module(c):
    D, H, A = c["a_fc1_w"].shape[1], c["a_fc1_w"].shape[0], c["a_fc3_w"].shape[0]
    m = _Actor(D, H, A)
    with torch.no_grad():
        for n in ACTOR_NAMES:
            getattr(getattr(m, n[:3]), "weight" if n.endswith("w") else "bias").copy_(torch.from_numpy(c["a_" + n]))
    return m.cuda()


def _buffer(c):
    from gym_rotor_amd import ReplayBuffer
    buf = ReplayBuffer(130, [c["obs"].shape[1]], [c["action"].shape[1]], "cuda")
    for dst, k in ((buf.obs, "obs"), (buf.obs_next, "obs_next"), (buf.act, "action"), (buf.rwd, "reward"), (buf.done, "done")):
        dst[0].copy_(_cuda(c[k]))
    buf.count, buf.current_size = 0, 130
    return buf


@pytest.mark.parametrize("name", ("mono", "dtde0", "dtde1"))
def test_td3_critic_loss_end_to_end(cases, name):
    from gym_rotor_amd import td3_critic_loss
    c = cases[name]
    critic, target, actor, buf = _twin_module(c, "c_", torch.float32), _twin_module(c, "t_", torch.float32), _actor_module(c), _buffer(c)
    eps = _cuda(c["eps"])
    stats = td3_critic_loss(critic, target, actor, buf, 0, None, noise=eps, **_scalars(c))
    torch.cuda.synchronize()
    y = buf._cache[(0, 130, 0)][0]
    check_y(name + " (end to end)", y, c["y"], torch_target(c, torch.float32, eps=c["eps"]))
    grads = {n: getattr(getattr(critic, n[:3]), "weight" if n.endswith("w") else "bias").grad for n in NAMES}
    assert all(g.shape == getattr(getattr(critic, n[:3]), "weight" if n.endswith("w") else "bias").shape for n, g in grads.items())
    check_grads(name + " (end to end)", c, grads, stats, _np(y))
    # the second call allocates nothing, and gives the same bits
    before = {n: g.clone() for n, g in grads.items()}
    s0 = stats.clone()
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    stats2 = td3_critic_loss(critic, target, actor, buf, 0, None, noise=eps, **_scalars(c))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem
    assert stats2.data_ptr() == stats.data_ptr() and torch.equal(stats2, s0) and all(torch.equal(grads[n], before[n]) for n in NAMES)


def test_collect_add_sample_loss_and_two_optimiser_steps():
    from gym_rotor_amd import ActorParams, DeviceAdamW, QCriticParams, QuadVecEnv, ReplayBuffer, RolloutStorage, td3_critic_loss, td3_target, twinq_grad
    T, N = 3, 70
    torch.manual_seed(11)
    env = QuadVecEnv("coupled", N, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=100, seed=21)
    env.reset("train")
    actor, critic = _Actor().cuda(), _Twin().cuda()
    actor_t, critic_t = _Actor().cuda(), _Twin().cuda()
    actor_t.load_state_dict(actor.state_dict())
    critic_t.load_state_dict(critic.state_dict())
    storage = RolloutStorage(env, T)
    storage.set_initial_obs(env.get_norm_error_state())
    env.rollout_actor([ActorParams.from_td3_module(actor, 0.1)], T, out=storage.horizon(), noise_seed=5)
    buf = ReplayBuffer(1000, env.obs_dims, [4], "cuda")
    buf.add(storage)
    torch.cuda.synchronize()
    assert (buf.count, buf.current_size) == (T * N, T * N)
    assert torch.equal(buf.obs[0][:T * N], storage.obs[0][:-1].reshape(T * N, 23)) and torch.equal(buf.act[0][:T * N], storage.act_all.reshape(T * N, 4))
    g = torch.Generator(device="cuda").manual_seed(2)
    idx = buf.sample(128, g)
    assert len(set(idx.tolist())) == 128 and int(idx.max()) < T * N
    eps = torch.randn(128, 4, device="cuda", generator=g)
    stats = td3_critic_loss(critic, critic_t, actor_t, buf, 0, idx, noise=eps)
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and all(torch.isfinite(p.grad).all() for p in critic.parameters())
    assert abs(float(stats[0]) - float(stats[1]) - float(stats[2])) <= 1e-5 * max(1.0, float(stats[0]))
    # two optimiser steps on a fixed minibatch and a fixed y lower the loss: two groups of six tensors (DeviceAdamW takes eight)
    y = td3_target(ActorParams.from_td3_module(actor_t, 0.0), QCriticParams.from_module(critic_t, 4), buf, 0, idx, noise=eps)
    params = [t for k in range(1, 7) for t in (getattr(critic, f"fc{k}").weight, getattr(critic, f"fc{k}").bias)]
    opts = [DeviceAdamW(params[:6], lr=1e-3, max_norm=-1), DeviceAdamW(params[6:], lr=1e-3, max_norm=-1)]
    grads = dict(zip(NAMES, (p.grad for p in params)))
    losses = []
    for _ in range(3):
        _, st = twinq_grad(QCriticParams.from_module(critic, 4), buf.obs[0], buf.act[0], y, idx, grads=grads)
        losses.append(float(st[0]))
        DeviceAdamW.step_all(opts)
    torch.cuda.synchronize()
    print("td3 critic: loss over two optimiser steps", losses)
    assert losses[2] < losses[1] < losses[0]
