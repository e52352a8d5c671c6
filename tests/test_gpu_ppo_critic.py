"""PPO's critic loss and its gradients on the device (ppo_critic_kernel + ppo_critic_reduce_kernel: qr_ppo_critic_grad,
RolloutStorage.critic_grad, critic_loss) against the reference's float64 autograd (tests/golden/ppo_critic_grad.npz) and the float64
restatement of tests/test_ppo_critic_host.py.

The bar, per tensor and per statistic, is DESIGN.md §8.5's: max(2e-6 * max(1, ||g64||_inf), e32), where e32 is the error of EAGER
FLOAT32 TORCH AUTOGRAD — the path this launch replaces, never the kernel — on the same inputs against the same float64.  Each test
prints the worst err / bar it saw before it asserts (pytest -s)."""
import numpy as np
import pytest
import torch

from test_critic_host import _Critic
from test_ppo_critic_host import CASES, NAMES, T, N, case, critic_grad_f64, f64_on_rows
from test_ppo_critic_host import fixture  # noqa: F401  (the module-scoped fixture file)

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


def _np(t):
    return t.detach().cpu().numpy()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _critic(c):
    from gym_rotor_amd import CriticParams
    return CriticParams(*[_cuda(t) for t in c["w"]], c["inputs"])


def _run(c, index=None, **over):
    from gym_rotor_amd import ppo_critic_grad
    kw = dict(l2_reg=c["l2_reg"])
    kw.update(over)
    grads, stats = ppo_critic_grad(_critic(c), [_cuda(o) for o in c["obs"]], _cuda(c["target"]),
                                   None if index is None else _cuda(np.asarray(index, dtype=np.int64)), **kw)
    torch.cuda.synchronize()
    return grads, stats


def _params(m):
    return (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias)


def _module(w, dtype):
    m = _Critic(w[0].shape[1], w[0].shape[0])
    with torch.no_grad():
        for p, t in zip(_params(m), w):
            p.copy_(torch.as_tensor(np.asarray(t)).reshape(p.shape))
    return m.to(dtype).cuda()


def torch_eval(m, x, y, l2_reg):
    """ppo.py:193-210 in eager torch with autograd, in the dtype of module `m`, on the GPU: (gradients in NAMES' order, [loss, mse,
    mean error, population variance of the target]) as float64 NumPy."""
    dt = m.fc1.weight.dtype
    x, y = (torch.as_tensor(np.asarray(t)).to(dt).cuda() for t in (x, y))
    err = m(x) - y[:, None]
    mse = err.pow(2).mean()
    loss = mse
    for name, param in m.named_parameters():
        if "weight" in name:
            loss = loss + param.pow(2).sum() * l2_reg
    m.zero_grad()
    loss.backward()
    grads = [_np(p.grad).astype(np.float64) for p in _params(m)]
    return grads, np.array([loss.item(), mse.item(), err.mean().item(), y.var(unbiased=False).item() if y.numel() > 1 else 0.0], dtype=np.float64)


def e32_of(w, x, y, l2_reg, g64, s64):
    """The error of eager float32 torch autograd against the float64 values: (per tensor, per statistic)."""
    g32, s32 = torch_eval(_module(w, torch.float32), x, y, l2_reg)
    return [float(np.abs(a - b.reshape(a.shape)).max()) for a, b in zip(g32, g64)], np.abs(s32 - s64)


def bar(v64, e32):
    return max(2e-6 * max(1.0, float(np.abs(v64).max())), float(e32))


def check(label, grads, stats, g64, s64, e32g, e32s):
    """Every gradient tensor and the four statistics within the bar.  Prints the worst ratio err / bar."""
    worst = (0.0, "", 0.0, 0.0)
    for n, want, e in zip(NAMES, g64, e32g):
        got = _np(grads[n]).astype(np.float64).reshape(want.shape)
        assert np.isfinite(got).all(), (label, n)
        err, b = float(np.abs(got - want).max()), bar(want, e)
        worst = max(worst, (err / b, n, err, e))
    st = _np(stats).astype(np.float64)
    assert np.isfinite(st).all(), label
    for q, n in enumerate(("loss", "mse", "mean_err", "target_var")):
        err, b = abs(st[q] - s64[q]), bar(s64[q], e32s[q])
        worst = max(worst, (err / b, n, err, float(e32s[q])))
    print(f"ppo critic {label}: worst err / bar = {worst[0]:.3f} at {worst[1]} (err {worst[2]:.3e}, e32 {worst[3]:.3e}); max e32 {max(e32g):.3e}")
    assert worst[0] <= 1.0, (label, worst)


def check_rows(label, c, grads, stats, idx=None, l2_reg=None):
    """Against the float64 restatement on rows idx of a fixture case."""
    l2 = c["l2_reg"] if l2_reg is None else l2_reg
    g64, s64 = f64_on_rows(c, idx, l2)
    rows = np.arange(T * N) if idx is None else np.asarray(idx)
    check(label, grads, stats, g64, s64, *e32_of(c["w"], c["x"][rows], c["target"][rows], l2, g64, s64))


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_against_the_reference_float64(fixture, name):  # noqa: F811
    c = case(fixture, name)
    grads, stats = _run(c)
    g64 = [c["g_" + n] for n in NAMES]
    s64 = np.array([c["loss"], c["mse"], c["mean_err"], c["target_var"]])
    check(name, grads, stats, g64, s64, *e32_of(c["w"], c["x"], c["target"], c["l2_reg"], g64, s64))


def _guarded(sizes, dtype=torch.float32, gap=16):
    """Slices of the given sizes of ONE buffer of sentinels, `gap` sentinel elements before and after each: (buffer, mask of the
    guard elements, views)."""
    buf = torch.full((sum(sizes) + gap * (len(sizes) + 1),), SENTINEL, dtype=dtype, device="cuda")
    views, mask, o = [], torch.ones_like(buf, dtype=torch.bool), gap
    for s in sizes:
        views.append(buf[o:o + s]); mask[o:o + s] = False; o += s + gap
    return buf, mask, views


def _guarded_outputs(c, need_bytes):
    D, H = c["fc1_w"].shape[1], c["fc1_w"].shape[0]
    buf, mask, views = _guarded([H * D, H, H * H, H, H, 1, 4])
    wbuf, wmask, (ws,) = _guarded([need_bytes // 8], torch.float64)
    return (buf, mask, wbuf, wmask), dict(zip(NAMES, views[:6])), views[6], ws


def _guards_intact(g, written=True):
    buf, mask, wbuf, wmask = g
    ok = bool((buf[mask] == SENTINEL).all()) and bool((wbuf[wmask] == SENTINEL).all())
    inner = bool((buf[~mask] != SENTINEL).all()) and bool((wbuf[~wmask] != SENTINEL).all())
    return ok and (inner if written else bool((buf == SENTINEL).all()) and bool((wbuf == SENTINEL).all()))


@pytest.mark.parametrize("name", ["mono", "ctde", "h5"])
def test_row_counts_with_guarded_outputs(fixture, name):  # noqa: F811
    from gym_rotor_amd.policy import ppo_critic_workspace_bytes
    c = case(fixture, name)
    dims = (c["fc1_w"].shape[1], c["fc1_w"].shape[0])
    for B in (1, 63, 64, 65, 130):
        g, grads, stats, ws = _guarded_outputs(c, ppo_critic_workspace_bytes(dims, B))
        idx = np.arange(B)
        _run(c, None if B == T * N else idx, grads=grads, stats=stats, workspace=ws)
        assert _guards_intact(g), B
        check_rows(f"{name} B={B}", c, grads, stats, idx)


def test_index_forms_and_clamping(fixture):  # noqa: F811
    c = case(fixture, "mono")
    rng = np.random.default_rng(3)
    g0, s0 = _run(c)
    g1, s1 = _run(c, np.arange(T * N))
    assert all(torch.equal(g0[n], g1[n]) for n in NAMES) and torch.equal(s0, s1)       # arange = None, bit for bit
    gp, sp = _run(c, rng.permutation(T * N))
    check_rows("mono permuted", c, gp, sp)
    rep = rng.integers(0, T * N, 97)
    assert len(np.unique(rep)) < 97
    gr, sr = _run(c, rep)
    check_rows("mono repeats", c, gr, sr, rep)
    # out-of-range entries: the result of the clamped index, bit for bit (the obs tensor's rows past T * N are never reached)
    wild = rep.copy()
    wild[::7] = rng.integers(T * N, 2 ** 40, len(wild[::7]))
    wild[3::7] = -rng.integers(1, 2 ** 40, len(wild[3::7]))
    wild[5] = np.iinfo(np.int64).min; wild[6] = np.iinfo(np.int64).max
    gw, sw = _run(c, wild)
    gc, sc = _run(c, np.clip(wild, 0, T * N - 1))
    assert all(torch.equal(gw[n], gc[n]) for n in NAMES) and torch.equal(sw, sc)
    check_rows("mono clamped", c, gw, sw, np.clip(wild, 0, T * N - 1))
    # the rows [64, 130) alone
    tail = np.arange(64, T * N)
    gt, st_ = _run(c, tail)
    check_rows("mono rows [64, 130)", c, gt, st_, tail)


def test_grid_sizes_determinism_and_workspace(fixture):  # noqa: F811
    from gym_rotor_amd.policy import ppo_critic_workspace_bytes
    c = case(fixture, "mono")
    idx = np.random.default_rng(4).integers(0, T * N, 200)               # B = 200: four tiles
    g64, s64 = f64_on_rows(c, idx)
    e32g, e32s = e32_of(c["w"], c["x"][idx], c["target"][idx], c["l2_reg"], g64, s64)
    seen = {}
    for mw in (1, 2, 3, 0):
        ga, sa = _run(c, idx, max_workgroups=mw)
        gb, sb = _run(c, idx, max_workgroups=mw)
        assert all(torch.equal(ga[n], gb[n]) for n in NAMES) and torch.equal(sa, sb), mw     # the same grid: the same bits
        check(f"mono B=200 max_workgroups={mw}", ga, sa, g64, s64, e32g, e32s)
        seen[mw] = ({n: _np(ga[n]).astype(np.float64) for n in NAMES}, _np(sa).astype(np.float64))
    for mw in (2, 3, 0):                                                   # ... and within the bar of each other
        for n, want, e in zip(NAMES, g64, e32g):
            assert np.abs(seen[mw][0][n] - seen[1][0][n]).max() <= bar(want, e), (mw, n)
        assert all(abs(seen[mw][1][q] - seen[1][1][q]) <= bar(s64[q], e32s[q]) for q in range(4)), mw
    # a workspace one byte too small: the error code, and nothing launched
    need = ppo_critic_workspace_bytes((23, 62), 200, 2)
    assert need == 2 * 5461 * 8
    g, grads, stats, ws = _guarded_outputs(c, need)
    with pytest.raises(ValueError, match="QR_E_SIZE"):
        _run(c, idx, max_workgroups=2, grads=grads, stats=stats, workspace=ws.view(torch.uint8)[:need - 1])
    torch.cuda.synchronize()
    assert _guards_intact(g, written=False)
    _run(c, idx, max_workgroups=2, grads=grads, stats=stats, workspace=ws)
    assert _guards_intact(g)
    # an empty minibatch: zero gradients and statistics, no launch
    ge, se = _run(c, np.zeros(0, dtype=np.int64))
    assert all((ge[n] == 0).all() for n in NAMES) and (se == 0).all()


def test_l2_term(fixture):  # noqa: F811
    c, nol2 = case(fixture, "mono"), case(fixture, "mono_nol2")
    g0, s0 = _run(c, l2_reg=0.0)
    g1, s1 = _run(c, l2_reg=1e-4)
    gn, sn = _run(nol2)
    assert all(torch.equal(g0[n], gn[n]) for n in NAMES) and torch.equal(s0, sn)        # the fixture's own l2_reg = 0 case: the data term
    check_rows("mono l2_reg=0", c, g0, s0, None, 0.0)
    for n in NAMES:
        if n.endswith("_b"):
            assert torch.equal(g0[n], g1[n]), n                                        # no L2 on a bias: the same bits
        else:   # float32(d + 2 l2 W) - float32(d): the two roundings of the gradient, and float32's of the product
            d0, d1, w = (_np(t).astype(np.float64) for t in (g0[n], g1[n], _cuda(c[n])))
            tol = 2 * np.spacing(np.float32(np.abs(d1).max())) + 2e-4 * np.spacing(np.float32(np.abs(w).max()))
            assert np.abs((d1 - d0) - 2e-4 * w).max() <= tol, n
    assert torch.equal(s0[1:], s1[1:]) and s1[0] > s0[0]
    norms = sum(float((c[n].astype(np.float64) ** 2).sum()) for n in ("fc1_w", "fc2_w", "fc3_w"))
    assert abs((float(s1[0]) - float(s0[0])) - 1e-4 * norms) <= 2 * np.spacing(np.float32(float(s1[0])))


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
def test_storage_critic_grad_on_a_hand_built_storage(kind):
    """T = 3, N = 70, the default target (td_target's column), storage.obs read in place although its T + 1 rows exceed `rows`: NaN
    in obs row T and in every final_obs row proves neither is read.  Coupled: one critic; Decoupled: a DTDE critic per agent and a
    CTDE critic reading both row sets."""
    from gym_rotor_amd import CriticParams, QuadVecEnv, RolloutStorage
    T_, N_ = 3, 70
    env = QuadVecEnv(kind, N_, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=100)
    st = RolloutStorage(env, T_)
    assert st.final_obs is not None
    gen = torch.Generator("cuda").manual_seed(9)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=gen)
    for o in st.obs:
        o.copy_(rnd(*o.shape) * 2 - 1)
        o[T_] = float("nan")
    for f in st.final_obs:
        f.fill_(float("nan"))
    st.td_target.copy_(torch.randn(T_, N_, st.n_agents, device="cuda", generator=gen) * 3)
    widths = [o.shape[-1] for o in st.obs]
    specs = [(0, (0,))] if kind == "coupled" else [(0, (0,)), (1, (1,)), (1, (0, 1)), (0, (0, 1))]
    for j, (k, inputs) in enumerate(specs):
        torch.manual_seed(40 + j)
        m = _Critic(sum(widths[i] for i in inputs), 62).cuda()
        idx = torch.randperm(T_ * N_, device="cuda", generator=gen)[:150]
        grads, stats = st.critic_grad(k, CriticParams.from_module(m, inputs), idx, l2_reg=1e-4)
        torch.cuda.synchronize()
        i = _np(idx)
        x = np.concatenate([_np(st.obs[a][:T_]).reshape(T_ * N_, -1)[i] for a in inputs], axis=1)
        y = _np(st.td_target[..., k]).reshape(-1)[i]
        w = [_np(p) for p in _params(m)]
        g64, s64 = critic_grad_f64(w, x, y, 1e-4)
        check(f"storage {kind} agent {k} inputs {inputs}", grads, stats, g64, s64, *e32_of(w, x, y, 1e-4, g64, s64))
        ga, sa = st.critic_grad(k, CriticParams.from_module(m, inputs), l2_reg=1e-4)        # all T * N rows, in order
        torch.cuda.synchronize()
        x = np.concatenate([_np(st.obs[a][:T_]).reshape(T_ * N_, -1) for a in inputs], axis=1)
        y = _np(st.td_target[..., k]).reshape(-1)
        g64, s64 = critic_grad_f64(w, x, y, 1e-4)
        check(f"storage {kind} agent {k} inputs {inputs} all rows", ga, sa, g64, s64, *e32_of(w, x, y, 1e-4, g64, s64))
    assert set(st._critic_workspace) == {(k, B, 0) for k, _ in specs for B in (150, T_ * N_)} and not st._ppo_workspace


def test_end_to_end_collect_to_optimiser_steps():
    """collect -> compute_values -> compute_gae -> normalize -> actor_loss + critic_loss -> AdamW steps on both modules -> collect
    again, on 128 Coupled envs, T = 4: the critic's .grad tensors against eager torch autograd on the same minibatch; two critic steps
    on one fixed minibatch lower the mean squared error."""
    from gym_rotor_amd import ActorParams, CriticParams, QuadVecEnv, RolloutStorage, actor_loss, critic_loss
    from test_ppo_actor_host import _Actor
    n, T_ = 128, 4
    torch.manual_seed(5)
    actor, critic = _Actor(23, 16, 4).cuda(), _Critic(23, 62).cuda()
    env = QuadVecEnv("coupled", n, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=3, seed=21)
    env.reset("train")
    env.get_norm_error_state()
    st = RolloutStorage(env, T_)
    st.collect(env, [ActorParams.from_module(actor)])
    nv = st.compute_values([CriticParams.from_module(critic)])
    adv, td, stats = st.compute_gae(0.99, 0.9, next_value=nv)
    adv = RolloutStorage.normalize(adv, stats)
    idx = torch.randperm(T_ * n, device="cuda")[:300]
    noise, nominal = torch.randn(23, device="cuda") * 0.05, RolloutStorage.nominal_action(env, 0)
    a_stats = actor_loss(actor, st, 0, adv, idx, noise=noise, nominal=nominal, clip=0.2, entropy_coef=0.01, lam_T=0.4, lam_S=0.3, lam_M=0.6)
    c_stats = critic_loss(critic, st, 0, idx, l2_reg=1e-4)
    torch.cuda.synchronize()
    assert torch.isfinite(a_stats).all() and torch.isfinite(c_stats).all()
    grads = {k: p.grad.clone() for k, p in zip(NAMES, _params(critic))}
    assert all(g.shape == p.shape for g, p in zip(grads.values(), _params(critic)))
    i = _np(idx)
    x, y = _np(st.obs[0][:T_]).reshape(T_ * n, -1)[i], _np(td[..., 0]).reshape(-1)[i]
    w = [_np(p) for p in _params(critic)]
    g64, s64 = torch_eval(_module(w, torch.float64), x, y, 1e-4)
    check("end to end", grads, c_stats, g64, s64, *e32_of(w, x, y, 1e-4, g64, s64))
    ev = 1.0 - (float(c_stats[1]) - float(c_stats[2]) ** 2) / float(c_stats[3])                # the caller's explained variance
    assert np.isfinite(ev) and abs(ev - (1.0 - (s64[1] - s64[2] ** 2) / s64[3])) < 1e-4

    opt_a, opt_c = torch.optim.AdamW(actor.parameters(), lr=1e-2), torch.optim.AdamW(critic.parameters(), lr=1e-4)
    before, v_before = st.act_all.clone(), st.value.clone()
    opt_a.step(); opt_c.step()
    mse = [float(c_stats[1])]
    for _ in range(2):                                                       # the same minibatch, the module's tensors read in place
        s = critic_loss(critic, st, 0, idx, l2_reg=1e-4)
        mse.append(float(s[1]))
        opt_c.step()
    print(f"ppo critic end to end: mse over two AdamW steps {mse}")
    assert mse[2] < mse[0]
    env2 = QuadVecEnv("coupled", n, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=3, seed=21)
    env2.reset("train")
    env2.get_norm_error_state()
    st2 = RolloutStorage(env2, T_)
    st2.collect(env2, [ActorParams.from_module(actor)])
    st2.compute_values([CriticParams.from_module(critic)])
    torch.cuda.synchronize()
    assert not torch.equal(st2.act_all, before) and torch.isfinite(st2.act_all).all()          # both updates are seen by the next horizon
    assert not torch.equal(st2.value, v_before) and torch.isfinite(st2.value).all()


def test_torch_op_returns_the_bits_of_the_ctypes_path(fixture):  # noqa: F811
    c = case(fixture, "ctde")
    idx = _cuda(np.random.default_rng(6).permutation(T * N)[:100].astype(np.int64))
    g0, s0 = _run(c, _np(idx))
    a = _critic(c)
    w = [getattr(a, n) for n in NAMES]
    obs, target = [_cuda(o) for o in c["obs"]], _cuda(c["target"])
    grads = [torch.full_like(t, SENTINEL) for t in w]
    stats = torch.full((4,), SENTINEL, device="cuda")
    torch.ops.gym_rotor_amd.qr_ppo_critic_grad(w, [0, 1], obs[0], obs[1], target, idx, grads, stats, c["l2_reg"])
    torch.cuda.synchronize()
    assert all(torch.equal(g0[n], g) for n, g in zip(NAMES, grads)) and torch.equal(s0, stats)
    with pytest.raises(ValueError, match="float32"):
        torch.ops.gym_rotor_amd.qr_ppo_critic_grad(w, [0, 1], obs[0], obs[1], target.double(), idx, grads, stats, c["l2_reg"])
