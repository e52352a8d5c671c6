"""SAC's critic half on the device (sac_target_kernel: qr_sac_target; sac_target, sac_critic_loss, the torch op) against the
reference's float64 modules (tests/golden/sac_critic.npz) and the float64 restatement of tests/sac_ref.py.

The bar, per output: err <= max(2e-6 * max(1, |x64|), e32), e32 = the error of eager float32 torch — the reference's own lines — on
the same inputs on this device; no factor on e32.  Every case prints err / bar before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sac_ref  # noqa: E402
import td3_ref  # noqa: E402
from sac_ref import ACTOR_NAMES  # noqa: E402
from td3_ref import NAMES  # noqa: E402
from test_sac_critic_host import CASES, LIVE, _SacActor  # noqa: E402
from twinq_gpu_util import _cuda, _idx, _np, _q, _twin_module, bar, torch_twinq  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
STATS = ("loss", "mse1", "mse2", "mean_y")


@pytest.fixture(scope="module")
def cases():
    g = sac_ref.load()
    return {n: sac_ref.case(g, n) for n in CASES}


def _critic(c, prefix="t_"):
    from gym_rotor_amd import QCriticParams
    return QCriticParams(*[_cuda(c[prefix + n]) for n in NAMES], int(c["action_dim"]))


def _actor(c):
    from gym_rotor_amd import ActorParams
    from gym_rotor_amd import _lib
    if "a_fc1_w" not in c:
        return None
    w = [_cuda(c["a_" + n]) for n in ACTOR_NAMES]
    return ActorParams(*w[:6], None, w[6], w[7], _lib.ACTOR_TANH_SAMPLE)


def _tensors(c):
    return {"obs": _cuda(c["obs"]), "act": _cuda(c["action"]), "rwd": _cuda(c["reward"]), "obs_next": _cuda(c["obs_next"]), "done": _cuda(c["done"])}


def run_target(c, index=None, eps="own", outputs=True, tensors=None, **over):
    """(y, action_out, logp_out) of one sac_target call on case c; eps: "own" (the case's first B rows, None when absent), an array
    or None."""
    from gym_rotor_amd import sac_target
    B = 130 if index is None else len(index)
    A = int(c["action_dim"])
    if isinstance(eps, str):
        eps = c.get("eps")
        eps = None if eps is None else eps[:B]
    kw = dict(discount=float(c["discount"]), alpha=float(c["alpha"]), noise=None if eps is None else _cuda(eps))
    if "a_fc1_w" not in c:
        kw.update(action_next=_cuda(c["a_next_in"][:B]), logp_next=_cuda(c["logp_next_in"][:B]))
    if outputs:
        kw.update(action_out=torch.full((B, A), SENTINEL, device="cuda"), logp_out=torch.full((B,), SENTINEL, device="cuda"))
    kw.update(over)
    y = sac_target(_actor(c), _critic(c), tensors or _tensors(c), 0, _idx(index), **kw)
    torch.cuda.synchronize()
    return y, kw.get("action_out"), kw.get("logp_out")


# ------------------------------------------------------------------------------------------------------------------------
# eager torch on the device, in a given dtype: what e32 is measured with (sac_mlp.py:65-76 with rsample's draw supplied, sac.py:146-153)
# ------------------------------------------------------------------------------------------------------------------------
def torch_target(c, dtype, index=None, eps=None):
    """(a', logp, y) as float64 NumPy arrays, computed by eager torch in `dtype` on the device."""
    idx = np.arange(130) if index is None else np.asarray(index)
    B = len(idx)
    on, r, d = (_cuda(c[k][idx], dtype) for k in ("obs_next", "reward", "done"))
    with torch.no_grad():
        if "a_fc1_w" in c:
            w = [_cuda(c["a_" + n], dtype) for n in ACTOR_NAMES]
            h = torch.relu(torch.relu(on @ w[0].T + w[1]) @ w[2].T + w[3])
            mean, log_std = h @ w[4].T + w[5], torch.clamp(h @ w[6].T + w[7], min=-20, max=2)
            std = log_std.exp()
            normal = torch.distributions.Normal(mean, std)
            x_t = mean + std * (_cuda(eps, dtype) if eps is not None else torch.zeros_like(mean))
            a = torch.tanh(x_t)
            logp = normal.log_prob(x_t)
            logp -= torch.log((1 - a.pow(2)) + 1e-6)
            logp = logp.sum(1, keepdim=True)
        else:
            a, logp = _cuda(c["a_next_in"][:B], dtype), _cuda(c["logp_next_in"][:B], dtype)[:, None]
        m = _twin_module(c, "t_", dtype)
        sa = torch.cat([on, a], 1)
        q = torch.min(_q(m, sa, 0), _q(m, sa, 1)) - float(c["alpha"]) * logp
        y = r[:, None] + float(c["discount"]) * (1 - d[:, None]) * q
    return tuple(_np(t).astype(np.float64) for t in (a, logp[:, 0], y[:, 0]))


def check(label, what, got, x64, x32):
    got = _np(got).astype(np.float64).reshape(x64.shape)
    assert np.isfinite(got).all(), (label, what)
    err, e32 = float(np.abs(got - x64).max()), float(np.abs(x32.reshape(x64.shape) - x64).max())
    b = bar(x64, e32)
    print(f"sac target {label} {what}: err / bar = {err / b:.3f} (err {err:.3e}, e32 {e32:.3e})")
    return err <= b, (label, what, err, b)


def check_all(label, outs, want64, want32):
    res = [check(label, what, g, w64, w32) for what, g, w64, w32 in zip(("y", "action_out", "logp_out"), outs, want64, want32)]
    assert all(ok for ok, _ in res), [info for ok, info in res if not ok]


# ------------------------------------------------------------------------------------------------------------------------
# qr_sac_target
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_target_fixture_cases_against_the_reference_float64(cases, name):
    c = cases[name]
    y, a, lp = run_target(c)
    assert y.shape == (130,) and y.dtype == torch.float32
    a32, l32, y32 = torch_target(c, torch.float32, eps=c.get("eps"))
    check_all(name, (y, a, lp), (c["y"], c["a_next"], c["logp"]), (y32, a32, l32))


def test_target_of_done_rows_is_the_reward_exactly(cases):
    for name in ("sat", "clamp", "mono", "dtde1", "w28"):
        c = cases[name]
        y, done = _np(run_target(c)[0]), c["done"] > 0
        assert done.sum() >= 3 and np.array_equal(y[done], c["reward"][done]), name
        assert not np.any(y[~done] == c["reward"][~done]), name


@pytest.mark.parametrize("name", ("mono", "dtde1", "h5", "w28"))
def test_target_batch_sizes_into_guarded_outputs(cases, name):
    c = cases[name]
    A = int(c["action_dim"])
    c2 = dict(c)
    full = [_np(t) for t in run_target(c, eps=None)]
    for B in (1, 63, 64, 65, 130):
        idx = np.arange(130 - B, 130)
        if "a_fc1_w" not in c:   # the supplied a' and logp go by minibatch position
            c2["a_next_in"], c2["logp_next_in"] = c["a_next_in"][130 - B:], c["logp_next_in"][130 - B:]
        out = torch.full((B + 2,), SENTINEL, device="cuda")
        ao = torch.full((B + 2, A), SENTINEL, device="cuda")
        lo = torch.full((B + 2,), SENTINEL, device="cuda")
        run_target(c2, idx, eps=None, out=out[1:-1], action_out=ao[1:-1], logp_out=lo[1:-1])
        for got, want in ((_np(out), full[0]), (_np(ao), full[1]), (_np(lo), full[2])):
            assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all() and np.array_equal(got[1:-1], want[130 - B:]), (name, B)


def test_target_index_forms(cases):
    c = cases["mono"]
    rng = np.random.default_rng(3)
    base = run_target(c, None, eps=None)

    def same(a, b, sel=None):
        return all(torch.equal(x, y if sel is None else y[torch.from_numpy(np.asarray(sel)).cuda()]) for x, y in zip(a, b))

    assert same(run_target(c, np.arange(130), eps=None), base)                                           # identity
    rev = np.arange(129, -1, -1)
    assert same(run_target(c, rev, eps=None), base, rev)                                                 # reversed order
    rep = np.array([3, 3, 3, 129, 0, 3])
    assert same(run_target(c, rep, eps=None), base, rep)                                                 # repeats
    wild = np.array([-1, 130, 5, 10 ** 12, -10 ** 12, 129])
    assert same(run_target(c, wild, eps=None), run_target(c, np.clip(wild, 0, 129), eps=None))           # clamped
    # 300 minibatch rows of a 130-row buffer (five tiles, repeats): the noise belongs to the minibatch position, not to the row
    idx = rng.integers(0, 130, 300)
    eps = rng.standard_normal((300, 4)).astype(np.float32)
    outs = run_target(c, idx, eps=eps)
    yal = lambda t: (t[2], t[0], t[1])                                                                   # (a', logp, y) -> (y, a', logp)
    check_all("300 rows, noise by position", outs, yal(sac_ref.sac_target_f64(c, idx, eps=eps)), yal(torch_target(c, torch.float32, idx, eps=eps)))


def test_target_reads_only_the_rows_the_index_names(cases):
    c = cases["mono"]
    idx = np.array([5, 7, 70, 129, 64, 63, 7])
    want = run_target(c, idx)
    t = _tensors(c)
    rest = torch.ones(130, dtype=torch.bool, device="cuda")
    rest[_idx(idx)] = False
    for k in ("obs", "act", "rwd", "obs_next", "done"):                                                  # NaN in every row the index does not name
        t[k][rest] = float("nan")
    got = run_target(c, idx, tensors=t)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_target_without_noise_is_zero_noise_bit_for_bit(cases):
    for name in ("noeps", "mono", "dtde1", "clamp"):
        c = cases[name]
        zeros = np.zeros((130, int(c["action_dim"])), dtype=np.float32)
        assert all(torch.equal(a, b) for a, b in zip(run_target(c, eps=None), run_target(c, eps=zeros))), name
    assert not torch.equal(run_target(cases["mono"], eps=None)[0], run_target(cases["mono"])[0])


def test_alpha_as_a_float_and_as_a_device_tensor(cases):
    for name in ("mono", "dtde1", "w28"):
        c = cases[name]
        for alpha in (0.2, 0.0, 1.75):
            a = run_target(c, alpha=alpha)
            b = run_target(c, alpha=torch.tensor([alpha], dtype=torch.float32, device="cuda"))
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, alpha)
    assert not torch.equal(run_target(cases["mono"], alpha=0.2)[0], run_target(cases["mono"], alpha=1.75)[0])


@pytest.mark.parametrize("name", ("mono", "dtde0", "dtde1", "h5", "sat"))
def test_alpha_zero_is_the_td3_target_of_the_same_action(cases, name):
    from gym_rotor_amd import td3_target
    c = cases[name]
    y, a, _ = run_target(c, alpha=0.0)
    y_td3 = td3_target(None, _critic(c), _tensors(c), 0, None, discount=float(c["discount"]), action_next=a)
    torch.cuda.synchronize()
    assert torch.equal(y, y_td3)
    assert not torch.equal(y, run_target(c)[0])


def test_outputs_on_or_off_leave_y_unchanged(cases):
    for name in ("mono", "dtde0", "dtde1", "w28", "clamp"):
        c = cases[name]
        y, a, lp = run_target(c)
        assert torch.equal(run_target(c, outputs=False)[0], y), name
        B, A = 130, int(c["action_dim"])
        assert torch.equal(run_target(c, outputs=False, action_out=torch.empty(B, A, device="cuda"))[0], y), name
        assert torch.equal(run_target(c, outputs=False, logp_out=torch.empty(B, device="cuda"))[0], y), name


def test_supplied_action_and_logp(cases):
    c = cases["w28"]                                                                                      # 24 + 4: wider than any actor
    outs = run_target(c)
    assert torch.equal(outs[1], _cuda(c["a_next_in"])) and torch.equal(outs[2], _cuda(c["logp_next_in"]))   # the outputs are copies
    for name in ("mono", "dtde0", "dtde1", "clamp", "sat"):                                               # a case's own a' and logp fed back in
        c = cases[name]
        y, a, lp = run_target(c)
        from gym_rotor_amd import sac_target
        y2 = sac_target(None, _critic(c), _tensors(c), 0, None, discount=float(c["discount"]), alpha=float(c["alpha"]), action_next=a, logp_next=lp)
        torch.cuda.synchronize()
        assert torch.equal(y2, y), name


def test_torch_op_gives_the_ctypes_path_bits(cases):
    c = cases["dtde0"]
    t, tcritic, actor = _tensors(c), _critic(c), _actor(c)
    idx = np.random.default_rng(5).permutation(130)[:100]
    eps = c["eps"][:100]
    y, a, lp = run_target(c, idx, eps=eps)
    y_op, a_op, l_op = torch.full((100,), SENTINEL, device="cuda"), torch.full((100, 4), SENTINEL, device="cuda"), torch.full((100,), SENTINEL, device="cuda")
    aw = [actor.fc1_w, actor.fc1_b, actor.fc2_w, actor.fc2_b, actor.mean_w, actor.mean_b, actor.log_std_w, actor.log_std_b]
    torch.ops.gym_rotor_amd.qr_sac_target(aw, [getattr(tcritic, n) for n in NAMES], 4, t["obs_next"], t["rwd"], t["done"], _idx(idx), _cuda(eps), None,
                                          None, y_op, a_op, l_op, float(c["discount"]), float(c["alpha"]))
    torch.cuda.synchronize()
    assert torch.equal(y_op, y) and torch.equal(a_op, a) and torch.equal(l_op, lp)
    y_dev = torch.full((100,), SENTINEL, device="cuda")
    torch.ops.gym_rotor_amd.qr_sac_target(aw, [getattr(tcritic, n) for n in NAMES], 4, t["obs_next"], t["rwd"], t["done"], _idx(idx), _cuda(eps), None,
                                          None, y_dev, None, None, float(c["discount"]), 0.0, torch.tensor([float(c["alpha"])], device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(y_dev, y)


# ------------------------------------------------------------------------------------------------------------------------
# sac_critic_loss
# ------------------------------------------------------------------------------------------------------------------------
def _actor_module(c):
    D, H, A = c["a_fc1_w"].shape[1], c["a_fc1_w"].shape[0], c["a_mean_w"].shape[0]
    m = _SacActor(D, H, A)
    with torch.no_grad():
        for lin, n in ((m.fc1, "fc1"), (m.fc2, "fc2"), (m.mean_linear, "mean"), (m.log_std_linear, "log_std")):
            lin.weight.copy_(torch.from_numpy(c[f"a_{n}_w"]))
            lin.bias.copy_(torch.from_numpy(c[f"a_{n}_b"]))
    return m.cuda()


def _buffer(c):
    from gym_rotor_amd import ReplayBuffer
    buf = ReplayBuffer(130, [c["obs"].shape[1]], [c["action"].shape[1]], "cuda")
    for dst, k in ((buf.obs, "obs"), (buf.obs_next, "obs_next"), (buf.act, "action"), (buf.rwd, "reward"), (buf.done, "done")):
        dst[0].copy_(_cuda(c[k]))
    buf.count, buf.current_size = 0, 130
    return buf


def check_grads(label, c, grads, stats, y32):
    """The twelve gradients and the statistics within the bar of the float64 restatement against y32, the float32 target the second
    launch was given, after the ReLU margin of these rows has been asserted.  Prints the worst err / bar."""
    w = [c["c_" + n] for n in NAMES]
    assert td3_ref.margin(w, c["obs"], c["action"]) >= td3_ref.MARGIN
    y32 = np.asarray(y32, dtype=np.float32)
    loss, m1, m2, g64 = td3_ref.twinq_grad_f64(w, c["obs"], c["action"], y32)
    s64 = np.array([loss, m1, m2, y32.astype(np.float64).mean()])
    g32, s32 = torch_twinq(c, torch.float32, y32)
    worst = (0.0, "", 0.0, 0.0)
    for n in NAMES:
        want = np.asarray(g64[n], dtype=np.float64)
        got = _np(grads[n]).astype(np.float64).reshape(want.shape)
        assert np.isfinite(got).all(), (label, n)
        e32, err = float(np.abs(g32[n].reshape(want.shape) - want).max()), float(np.abs(got - want).max())
        worst = max(worst, (err / bar(want, e32), n, err, e32))
    st = _np(stats).astype(np.float64)
    assert np.isfinite(st).all(), label
    for q, n in enumerate(STATS):
        e32, err = abs(s32[q] - s64[q]), abs(st[q] - s64[q])
        worst = max(worst, (err / bar(s64[q], e32), n, err, float(e32)))
    print(f"sac critic loss {label}: worst err / bar = {worst[0]:.3f} at {worst[1]} (err {worst[2]:.3e}, e32 {worst[3]:.3e})")
    assert worst[0] <= 1.0, (label, worst)


@pytest.mark.parametrize("name", LIVE)
def test_sac_critic_loss_end_to_end(cases, name):
    from gym_rotor_amd import sac_critic_loss
    c = cases[name]
    critic, target, actor, buf = _twin_module(c, "c_", torch.float32), _twin_module(c, "t_", torch.float32), _actor_module(c), _buffer(c)
    eps = _cuda(c["eps"])
    kw = dict(discount=float(c["discount"]), alpha=float(c["alpha"]), noise=eps)
    stats = sac_critic_loss(critic, target, actor, buf, 0, None, **kw)
    torch.cuda.synchronize()
    y = buf._cache[("sac", 0, 130, 0)][0]
    assert torch.equal(y, run_target(c)[0])
    ok, info = check(name + " (end to end)", "y", y, c["y"], torch_target(c, torch.float32, eps=c["eps"])[2])
    assert ok, info
    grads = {n: getattr(getattr(critic, n[:3]), "weight" if n.endswith("w") else "bias").grad for n in NAMES}
    assert all(g.shape == getattr(getattr(critic, n[:3]), "weight" if n.endswith("w") else "bias").shape for n, g in grads.items())
    check_grads(name + " (end to end)", c, grads, stats, _np(y))
    # the second call allocates nothing, and gives the same bits
    before = {n: g.clone() for n, g in grads.items()}
    s0 = stats.clone()
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    stats2 = sac_critic_loss(critic, target, actor, buf, 0, None, **kw)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem
    assert stats2.data_ptr() == stats.data_ptr() and torch.equal(stats2, s0) and all(torch.equal(grads[n], before[n]) for n in NAMES)


def test_sac_critic_loss_in_a_graph_replays_the_same_bits(cases):
    from gym_rotor_amd import sac_critic_loss
    c = cases["mono"]
    critic, target, actor, buf = _twin_module(c, "c_", torch.float32), _twin_module(c, "t_", torch.float32), _actor_module(c), _buffer(c)
    eps = _cuda(c["eps"])
    alpha = torch.tensor([float(c["alpha"])], device="cuda")
    kw = dict(discount=float(c["discount"]), alpha=alpha, noise=eps)
    stats = sac_critic_loss(critic, target, actor, buf, 0, None, **kw)                                   # eager: allocates the cache and .grad
    torch.cuda.synchronize()
    grads = {n: getattr(getattr(critic, n[:3]), "weight" if n.endswith("w") else "bias").grad for n in NAMES}
    want = {n: g.clone() for n, g in grads.items()}
    s0, y0 = stats.clone(), buf._cache[("sac", 0, 130, 0)][0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                                          # a single chain of two launches plus the reduction
        sac_critic_loss(critic, target, actor, buf, 0, None, **kw)
    for g in grads.values():
        g.fill_(SENTINEL)
    stats.fill_(SENTINEL)
    buf._cache[("sac", 0, 130, 0)][0].fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf._cache[("sac", 0, 130, 0)][0], y0) and torch.equal(stats, s0) and all(torch.equal(grads[n], want[n]) for n in NAMES)
    alpha.fill_(1.5)                                                                                       # the device alpha is read at replay
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf._cache[("sac", 0, 130, 0)][0], run_target(c, alpha=1.5)[0])
