"""PPO's actor loss and its gradients on the device (ppo_actor_kernel + ppo_reduce_kernel: qr_ppo_actor_grad, RolloutStorage.actor_grad,
actor_loss) against the reference's float64 autograd (tests/golden/ppo_actor_grad.npz) and the float64 restatement of
tests/test_ppo_actor_host.py.

The bar, per tensor and per statistic: max(2e-6 * max(1, ||g64||_inf), e32), where e32 is the error of EAGER FLOAT32 TORCH
AUTOGRAD — the path this launch replaces, never the kernel — on the same inputs against the same float64.  The bar was first
written with 4 * e32 (for tanh_fast's 2e-7 absolute error against tanhf's single ulp and a different order of summation); the first
MI355X run showed the factor is not needed — the worst error of any tensor in any test was 5.6e-7 (mono_sat, mean_w) against
e32 = 4.5e-7, everything else below 2e-7 — so it is 1.  Each test prints the worst figure it saw before it asserts (pytest -s)."""
import numpy as np
import pytest
import torch

from test_ppo_actor_host import CASES, COEFFS, NAMES, T, N, _Actor, case, f64_on_rows, ppo_f64
from test_ppo_actor_host import fixture  # noqa: F401  (the module-scoped fixture file)

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


def _np(t):
    return t.detach().cpu().numpy()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _actor(c):
    from gym_rotor_amd import ActorParams
    return ActorParams(*[_cuda(t) for t in c["w"]])


def _inputs(c):
    """(positional tensors of ppo_actor_grad, keyword tensors and coefficients) of a fixture case."""
    pos = [_cuda(c[k]) for k in ("obs", "action", "logp_old", "advantage")]
    kw = dict(final_obs=_cuda(c["final_obs"]), done=_cuda(c["done"]), truncated=_cuda(c["truncated"]), noise=_cuda(c["noise"]),
              nominal=_cuda(c["nominal"].astype(np.float32)), **c["co"])
    return pos, kw


def _run(c, index=None, **over):
    from gym_rotor_amd import ppo_actor_grad
    pos, kw = _inputs(c)
    kw.update(over)
    grads, stats = ppo_actor_grad(_actor(c), *pos, None if index is None else _cuda(np.asarray(index, dtype=np.int64)), **kw)
    torch.cuda.synchronize()
    return grads, stats


def _module(w, dtype):
    D, H, A = w[0].shape[1], w[0].shape[0], w[4].shape[0]
    m = _Actor(D, H, A)
    with torch.no_grad():
        for p, t in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.mean_linear.weight, m.mean_linear.bias, m.log_std), w):
            p.copy_(torch.as_tensor(np.asarray(t)).reshape(p.shape))
    return m.to(dtype).cuda()


def torch_eval(m, x, xn, act, old, adv, co, noise, nominal):
    """ppo.py:169-182 + policy_regularization.py in eager torch with autograd, in the dtype of module `m`, on the GPU: (gradients in
    NAMES' order, [loss, mean S, rows outside the clip range, mean (rho - 1) - log rho]) as float64 NumPy."""
    dt = m.fc1.weight.dtype
    x, xn, act, old, adv = (torch.as_tensor(np.asarray(t)).to(dt).cuda() for t in (x, xn, act, old, adv))
    clip, ent, lam_T, lam_S, lam_M, ma = (co[k] for k in COEFFS)
    dist = torch.distributions.Normal(m(x), m.log_std.expand(x.shape[0], -1).exp())
    ratio = torch.exp(dist.log_prob(act).sum(1, keepdim=True) - old.sum(1, keepdim=True))
    s1, s2 = ratio * adv[:, None], torch.clamp(ratio, 1 - clip, 1 + clip) * adv[:, None]
    surr = torch.min(s1, s2)
    loss = -(surr + ent * dist.entropy().sum(1, keepdim=True)).mean()
    a0 = m(x).clamp(-ma, ma)
    if lam_T:
        loss = loss + lam_T * torch.nn.functional.mse_loss(a0, m(xn).clamp(-ma, ma))
    if lam_S:
        loss = loss + lam_S * torch.nn.functional.mse_loss(a0, m(x + torch.as_tensor(np.asarray(noise)).to(dt).cuda()).clamp(-ma, ma))
    if lam_M:
        loss = loss + lam_M * torch.nn.functional.mse_loss(a0, torch.as_tensor(np.asarray(nominal)).to(dt).cuda().expand_as(a0))
    m.zero_grad()
    loss.backward()
    ps = (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.mean_linear.weight, m.mean_linear.bias, m.log_std)
    grads = [_np(p.grad).astype(np.float64).reshape(-1) if p is m.log_std else _np(p.grad).astype(np.float64) for p in ps]
    r = ratio.detach()
    stats = [loss.item(), surr.mean().item(), float(((r < 1 - clip) | (r > 1 + clip)).sum().item()), ((r - 1) - r.log()).mean().item()]
    return grads, np.array(stats, dtype=np.float64)


def _rows(c, idx=None):
    idx = np.arange(T * N) if idx is None else np.asarray(idx)
    D, A = c["fc1_w"].shape[1], c["mean_w"].shape[0]
    return (c["obs"][:-1].reshape(-1, D)[idx], c["obs_next"].reshape(-1, D)[idx], c["action"].reshape(-1, A)[idx],
            c["logp_old"].reshape(-1, A)[idx], c["advantage"][idx])


def e32_on_rows(c, idx=None):
    """The error of eager float32 torch autograd against the float64 restatement on rows idx: (per tensor, per statistic)."""
    g64, s64 = f64_on_rows(c, idx)
    g32, s32 = torch_eval(_module(c["w"], torch.float32), *_rows(c, idx), c["co"], c["noise"], c["nominal"])
    return [float(np.abs(a - b).max()) for a, b in zip(g32, g64)], np.abs(s32 - s64)


def bar(v64, e32):
    return max(2e-6 * max(1.0, float(np.abs(v64).max())), float(e32))


def check(label, grads, stats, g64, s64, e32g, e32s, n_rows):
    """Every gradient tensor and the three float statistics within the bar; the clip fraction exact.  Prints the worst ratio err / bar."""
    worst = (0.0, "", 0.0, 0.0)
    for n, want, e in zip(NAMES, g64, e32g):
        got = _np(grads[n]).astype(np.float64).reshape(want.shape)
        assert np.isfinite(got).all(), (label, n)
        err, b = float(np.abs(got - want).max()), bar(want, e)
        worst = max(worst, (err / b, n, err, e))
    st = _np(stats).astype(np.float64)
    for q, n in ((0, "loss"), (1, "surrogate"), (3, "kl")):
        err, b = abs(st[q] - s64[q]), bar(s64[q], e32s[q])
        worst = max(worst, (err / b, n, err, float(e32s[q])))
    print(f"ppo actor {label}: worst err / bar = {worst[0]:.3f} at {worst[1]} (err {worst[2]:.3e}, e32 {worst[3]:.3e}); "
          f"max e32 {max(e32g):.3e}; clip fraction {st[2]:.6f}")
    assert worst[0] <= 1.0, (label, worst)
    assert st[2] == np.float32(s64[2] / n_rows), (label, st[2], s64[2])


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_against_the_reference_float64(fixture, name):  # noqa: F811
    c = case(fixture, name)
    grads, stats = _run(c)
    g64 = [c["g_" + n] for n in NAMES]
    s64 = np.array([c["loss"], c["surr"], float(c["n_clipped"]), c["kl"]])
    e32g, e32s = e32_on_rows(c)
    check(name, grads, stats, g64, s64, e32g, e32s, T * N)


def _guarded(dims, gap=16):
    """The seven gradient tensors and stats as slices of ONE buffer of sentinels, `gap` sentinel floats before and after each."""
    D, H, A = dims
    sizes = [H * D, H, H * H, H, A * H, A, A, 4]
    buf = torch.full((sum(sizes) + gap * (len(sizes) + 1),), SENTINEL, dtype=torch.float32, device="cuda")
    views, mask, o = [], torch.ones_like(buf, dtype=torch.bool), gap
    for s in sizes:
        views.append(buf[o:o + s]); mask[o:o + s] = False; o += s + gap
    return buf, mask, dict(zip(NAMES, views[:7])), views[7]


@pytest.mark.parametrize("name", ["mono", "modul1"])
def test_row_counts_with_guarded_outputs(fixture, name):  # noqa: F811
    c = case(fixture, name)
    dims = (c["fc1_w"].shape[1], c["fc1_w"].shape[0], c["mean_w"].shape[0])
    for B in (1, 63, 64, 65, 130):
        buf, mask, grads, stats = _guarded(dims)
        idx = np.arange(B)
        _run(c, None if B == T * N else idx, grads=grads, stats=stats)
        assert (buf[mask] == SENTINEL).all() and (buf[~mask] != SENTINEL).all(), B
        g64, s64 = f64_on_rows(c, idx)
        e32g, e32s = e32_on_rows(c, idx)
        check(f"{name} B={B}", grads, stats, g64, s64, e32g, e32s, B)


def test_index_permutation_identity_and_repeats(fixture):  # noqa: F811
    c = case(fixture, "mono")
    rng = np.random.default_rng(3)
    g0, s0 = _run(c)
    g1, s1 = _run(c, np.arange(T * N))
    assert all(torch.equal(g0[n], g1[n]) for n in NAMES) and torch.equal(s0, s1)       # arange = None, bit for bit
    g64, s64 = f64_on_rows(c)
    e32g, e32s = e32_on_rows(c)
    gp, sp = _run(c, rng.permutation(T * N))
    check("mono permuted", gp, sp, g64, s64, e32g, e32s, T * N)
    rep = rng.integers(0, T * N, 97)
    assert len(np.unique(rep)) < 97
    gr, sr = _run(c, rep)
    check("mono repeats", gr, sr, *f64_on_rows(c, rep), *e32_on_rows(c, rep), 97)


def test_grid_sizes_determinism_and_workspace(fixture):  # noqa: F811
    from gym_rotor_amd.policy import ppo_workspace_bytes
    c = case(fixture, "mono")
    idx = np.random.default_rng(4).integers(0, T * N, 200)               # B = 200: four tiles
    g64, s64 = f64_on_rows(c, idx)
    e32g, e32s = e32_on_rows(c, idx)
    for mw in (1, 2, 3, 0):
        ga, sa = _run(c, idx, max_workgroups=mw)
        gb, sb = _run(c, idx, max_workgroups=mw)
        assert all(torch.equal(ga[n], gb[n]) for n in NAMES) and torch.equal(sa, sb), mw     # the same grid: the same bits
        check(f"mono B=200 max_workgroups={mw}", ga, sa, g64, s64, e32g, e32s, 200)
    # a workspace one byte too small: the error code, and nothing launched
    need = ppo_workspace_bytes((23, 16, 4), 200, 2)
    assert need == 2 * 734 * 8
    buf, mask, grads, stats = _guarded((23, 16, 4))
    with pytest.raises(ValueError, match="QR_E_SIZE"):
        _run(c, idx, max_workgroups=2, grads=grads, stats=stats, workspace=torch.zeros(need - 1, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()
    _run(c, idx, max_workgroups=2, grads=grads, stats=stats, workspace=torch.zeros(need, dtype=torch.uint8, device="cuda"))
    assert (buf[mask] == SENTINEL).all() and (buf[~mask] != SENTINEL).all()
    # an empty minibatch: zero gradients and statistics, no launch
    g, s = _run(c, np.zeros(0, dtype=np.int64))
    assert all((g[n] == 0).all() for n in NAMES) and (s == 0).all()


def _module_weights(m):
    return [_np(p).reshape(-1) if p is m.log_std else _np(p) for p in (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.mean_linear.weight,
                                                                     m.mean_linear.bias, m.log_std)]


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
def test_storage_actor_grad_on_a_hand_built_storage(kind):
    """T = 3, N = 70: about 10 % resets from every flag, NaN in every final_obs row of an env that did not reset; every agent from the
    storage's shared action / logprob rows.  Against the float64 restatement fed with storage.sample()'s obs_next."""
    from gym_rotor_amd import ActorParams, QuadVecEnv, RolloutStorage
    from gym_rotor_amd.policy import ACTOR_DIMS
    T_, N_ = 3, 70
    env = QuadVecEnv(kind, N_, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=100)
    st = RolloutStorage(env, T_)
    assert st.final_obs is not None
    gen = torch.Generator("cuda").manual_seed(7)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=gen)
    for o in st.obs:
        o.copy_(rnd(*o.shape) * 2 - 1)
    st.done.copy_(rnd(T_, N_, st.n_agents) < 0.04); st.truncated.copy_(rnd(T_, N_) < 0.04)
    mask = st.reset_mask()
    assert 0.03 < mask.float().mean() < 0.3
    for f in st.final_obs:
        f.copy_(rnd(*f.shape) * 2 - 1)
        f[~mask] = float("nan")
    st.act_all.copy_(rnd(*st.act_all.shape) * 1.6 - 0.8)
    adv = torch.randn(T_, N_, st.n_agents, device="cuda", generator=gen)
    obs, act, _, obs_next, _, logp = st.sample()
    for k, dims in enumerate(ACTOR_DIMS[kind]):
        torch.manual_seed(30 + k)
        m = _Actor(*dims).cuda()
        with torch.no_grad():   # log-probs of the stored actions under the policy, shifted so that the ratios spread around the clip range
            d = torch.distributions.Normal(m(st.obs[k][:-1]), m.log_std.exp())
            st.logprob[k].copy_(d.log_prob(st.act[k]) + (rnd(T_, N_, 1) - 0.5) * 0.8 / dims[2])
        co = dict(clip=0.2, entropy_coef=0.01, lam_T=0.4, lam_S=0.3, lam_M=0.6, max_action=1.0)
        noise = torch.randn(dims[0], device="cuda", generator=gen) * 0.05
        nominal = RolloutStorage.nominal_action(env, k)
        idx = torch.randperm(T_ * N_, device="cuda", generator=gen)[:150]
        grads, stats = st.actor_grad(k, ActorParams.from_module(m), adv, idx, noise=noise, nominal=nominal, **co)
        torch.cuda.synchronize()
        i = _np(idx)
        rows = [_np(t)[i] for t in (obs[k], obs_next[k], act[k], st.logprob[k].reshape(T_ * N_, -1), adv[..., k].reshape(-1))]
        assert all(np.isfinite(r).all() for r in rows)
        g64, s64 = ppo_f64(_module_weights(m), *rows, co, _np(noise), _np(nominal))
        g32, s32 = torch_eval(m, *rows, co, _np(noise), _np(nominal))
        e32g, e32s = [float(np.abs(a - b).max()) for a, b in zip(g32, g64)], np.abs(s32 - s64)
        assert all(torch.isfinite(grads[n]).all() for n in NAMES) and torch.isfinite(stats).all()
        check(f"storage {kind} agent {k}", grads, stats, g64, s64, e32g, e32s, 150)
    assert len(st._ppo_workspace) == len(ACTOR_DIMS[kind])


def test_end_to_end_collect_to_optimiser_step():
    """collect -> compute_values -> compute_gae -> normalize -> actor_loss on 128 Coupled envs, T = 4: the .grad tensors against eager
    torch float64 on storage.sample(); an AdamW step from them changes the next collection, since the kernels read the module's
    tensors in place."""
    from gym_rotor_amd import ActorParams, CriticParams, QuadVecEnv, RolloutStorage, actor_loss
    from test_critic_host import _Critic
    n, T_ = 128, 4

    def fresh():
        env = QuadVecEnv("coupled", n, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=3, seed=21)
        env.reset("train")
        env.get_norm_error_state()
        return env, RolloutStorage(env, T_)

    torch.manual_seed(5)
    m, critic = _Actor(23, 16, 4).cuda(), _Critic(23, 62).cuda()
    env, st = fresh()
    st.collect(env, [ActorParams.from_module(m)])
    assert st.reset_mask().any() and not st.reset_mask().all()
    nv = st.compute_values([CriticParams.from_module(critic)])
    adv, _, stats = st.compute_gae(0.99, 0.9, next_value=nv)
    adv = RolloutStorage.normalize(adv, stats)
    co = dict(clip=0.2, entropy_coef=0.01, lam_T=0.4, lam_S=0.3, lam_M=0.6, max_action=1.0)
    noise = torch.randn(23, device="cuda") * 0.05
    nominal = RolloutStorage.nominal_action(env, 0)
    idx = torch.randperm(T_ * n, device="cuda")[:300]
    got = actor_loss(m, st, 0, adv, idx, noise=noise, nominal=nominal, **co)
    torch.cuda.synchronize()
    ps = (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.mean_linear.weight, m.mean_linear.bias, m.log_std)
    assert m.log_std.grad.shape == (1, 4)
    grads = {k: p.grad.clone() for k, p in zip(NAMES, ps)}
    obs, act, _, obs_next, _, logp = st.sample()
    i = _np(idx)
    rows = [_np(t)[i] for t in (obs[0], obs_next[0], act[0], logp[0], adv.reshape(-1))]
    w = _module_weights(m)
    g64, s64 = torch_eval(_module(w, torch.float64), *rows, co, _np(noise), _np(nominal))
    g32, s32 = torch_eval(_module(w, torch.float32), *rows, co, _np(noise), _np(nominal))
    e32g, e32s = [float(np.abs(a - b).max()) for a, b in zip(g32, g64)], np.abs(s32 - s64)
    check("end to end", grads, got, g64, s64, e32g, e32s, 300)
    for p, g in zip(ps, grads.values()):
        p.grad = g.reshape(p.shape)

    before = st.act_all.clone()
    env_b, st_b = fresh()
    st_b.collect(env_b, [ActorParams.from_module(m)])
    assert torch.equal(st_b.act_all, before)                               # the same env, seed and weights: the same collection
    params = ActorParams.from_module(m)                                     # taken BEFORE the step: it points at the module's tensors
    torch.optim.AdamW(m.parameters(), lr=1e-2).step()
    env_c, st_c = fresh()
    st_c.collect(env_c, [params])
    torch.cuda.synchronize()
    assert not torch.equal(st_c.act_all, before) and torch.isfinite(st_c.act_all).all()


def test_torch_op_returns_the_bits_of_the_ctypes_path(fixture):  # noqa: F811
    c = case(fixture, "modul0")
    pos, kw = _inputs(c)
    idx = _cuda(np.random.default_rng(6).permutation(T * N)[:100].astype(np.int64))
    a = _actor(c)
    g0, s0 = _run(c, _np(idx))
    w = [getattr(a, n) for n in NAMES]
    grads = [torch.full_like(t, SENTINEL) for t in w]
    stats = torch.full((4,), SENTINEL, device="cuda")
    co = c["co"]
    torch.ops.gym_rotor_amd.qr_ppo_actor_grad(w, pos[0], kw["final_obs"], kw["done"], kw["truncated"], pos[1], pos[2], pos[3], idx, kw["noise"],
                                              kw["nominal"], grads, stats, 0, co["clip"], co["entropy_coef"], co["lam_T"], co["lam_S"], co["lam_M"],
                                              co["max_action"])
    torch.cuda.synchronize()
    assert all(torch.equal(g0[n], g) for n, g in zip(NAMES, grads)) and torch.equal(s0, stats)
    with pytest.raises(ValueError, match="float32"):
        torch.ops.gym_rotor_amd.qr_ppo_actor_grad(w, pos[0].double(), None, None, None, pos[1], pos[2], pos[3], idx, kw["noise"], kw["nominal"],
                                                  grads, stats, 0, co["clip"], co["entropy_coef"], co["lam_T"], co["lam_S"], co["lam_M"], co["max_action"])
