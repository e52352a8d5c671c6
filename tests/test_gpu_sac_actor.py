"""qr_sac_actor_grad on the device against tests/golden/sac_actor.npz (the reference's float64 autograd; tools/gen_golden_sac_actor.py)
and the float64 restatement (tests/sac_actor_ref.py).  The bar is DESIGN.md §8.6's through twinq_gpu_util.bar:
err <= max(2e-6 * max(1, |x64|), e32), e32 the error of eager float32 torch autograd on the same inputs on the device, no factor on it.
Each accuracy test prints its worst err / bar per case."""
import numpy as np
import pytest
import torch

import sac_actor_ref as R
from twinq_gpu_util import _cuda, _idx, _np, bar

pytestmark = pytest.mark.gpu

G = R.load()
NAMES = R.ACTOR_NAMES


def _params(c):
    from gym_rotor_amd import ActorParams, QCriticParams, _lib
    w = [_cuda(c["a_" + n]) for n in NAMES]
    actor = ActorParams(*w[:6], None, w[6], w[7], _lib.ACTOR_TANH_SAMPLE)
    critic = QCriticParams(*[_cuda(c["c_" + n]) for n in R.CRITIC_NAMES], action_dim=c["a_mean_w"].shape[0])
    return actor, critic


def _kw(c, B=None, **over):
    kw = dict(alpha=c["alpha"], lam_T=c["lam"][0], lam_S=c["lam"][1], lam_M=c["lam"][2], max_action=c["max_action"],
              noise=_cuda(c["noise"].astype(np.float32)), nominal=_cuda(c["nominal"].astype(np.float32)), target_entropy=c["target_entropy"])
    for k in R.EPS:
        kw[k] = _cuda(c[k][:B]) if k in c else None
    kw.update(over)
    return kw


def _run(c, index=None, B=None, **over):
    from gym_rotor_amd import sac_actor_grad
    actor, critic = _params(c)
    obs, obs_next = _cuda(c["obs"]), _cuda(c["obs_next"])
    if index is None and B is not None:
        index = np.arange(B)
    n = len(c["obs"]) if index is None else len(index)
    grads, stats = sac_actor_grad(actor, critic, obs, obs_next, _idx(index), **_kw(c, n, **over))
    torch.cuda.synchronize()
    return {k: _np(v).astype(np.float64) for k, v in grads.items()}, _np(stats).astype(np.float64)


def _eager(c, dtype, index=None, q_swap=False):
    """The reference's lines in eager torch autograd on the device in `dtype`: (grads, stats[:4]).  Normal(mean, std).log_prob(u) is
    written out with -eps^2 / 2 formed from eps: as -(u - mean)^2 / (2 std^2) it cancels in float32 where std is exp(-20) (`clamp`: an
    error of 0.85 in the mean logp), and an e32 of that size would leave the loss, the mean logp and alpha's gradient unchecked."""
    idx = np.arange(len(c["obs"])) if index is None else np.asarray(index)
    w = [_cuda(c["a_" + n], dtype).requires_grad_() for n in NAMES]
    q = [_cuda(c["c_" + n], dtype) for n in R.CRITIC_NAMES]
    if q_swap:
        q = q[6:] + q[:6]
    x, xn = _cuda(c["obs"][idx], dtype), _cuda(c["obs_next"][idx], dtype)
    eps = [_cuda(c[k][:len(idx)], dtype) if k in c else None for k in R.EPS]
    lam_T, lam_S, lam_M = c["lam"]
    ma = c["max_action"]

    def sample(x, e):
        h = torch.relu(torch.relu(x @ w[0].T + w[1]) @ w[2].T + w[3])
        mean, ls = h @ w[4].T + w[5], torch.clamp(h @ w[6].T + w[7], -20.0, 2.0)
        std = ls.exp()
        e = torch.zeros_like(mean) if e is None else e
        a = torch.tanh(mean + std * e)
        lp = -0.5 * e * e - ls - 0.5 * float(np.log(2 * np.pi)) - torch.log((1 - a.pow(2)) + 1e-6)
        return a, lp.sum(1, keepdim=True)

    def Q(k, a):
        sa = torch.cat([x, a], 1)
        return torch.relu(torch.relu(sa @ q[6 * k].T + q[6 * k + 1]) @ q[6 * k + 2].T + q[6 * k + 3]) @ q[6 * k + 4].T + q[6 * k + 5]

    a, lp = sample(x, eps[0])
    qmin = torch.min(Q(0, a), Q(1, a))
    loss = -(qmin - c["alpha"] * lp).mean()
    r = sample(x, eps[1])[0].clamp(-ma, ma)
    rn = sample(xn, eps[2])[0].clamp(-ma, ma)
    rp = sample(x + _cuda(c["noise"], dtype)[None, :], eps[3])[0].clamp(-ma, ma)
    mse = torch.nn.functional.mse_loss
    total = loss + lam_T * mse(r, rn) + lam_S * mse(r, rp) + lam_M * mse(r, _cuda(c["nominal"], dtype)[None, :].expand_as(r))
    total.backward()
    grads = {n: _np(t.grad).astype(np.float64) for n, t in zip(NAMES, w)}
    return grads, np.array([total.item(), qmin.mean().item(), lp.mean().item(), (total - loss).item()], dtype=np.float64)


def _worst(got_g, got_s, ref_g, ref_s, e32_g, e32_s):
    worst = 0.0
    for n in NAMES:
        worst = max(worst, np.abs(got_g[n].reshape(ref_g[n].shape) - ref_g[n]).max() / bar(ref_g[n], np.abs(e32_g[n] - ref_g[n]).max()))
    for k in range(4):
        worst = max(worst, abs(got_s[k] - ref_s[k]) / bar(ref_s[k], abs(e32_s[k] - ref_s[k])))
    return worst


@pytest.mark.parametrize("name", R.CASES)
def test_fixture_cases(name):
    """All fixture cases: eight gradients and six stats against the reference's float64 autograd; the two shares exact."""
    c = R.case(G, name)
    ag = torch.full((1,), float("nan"), device="cuda")
    g, s = _run(c, alpha_grad=ag)
    ref_g = {n: c["g_" + n] for n in NAMES}
    e32_g, e32_s = _eager(c, torch.float32)
    worst = _worst(g, s, ref_g, c["stats"], e32_g, e32_s)
    print(f"sac_actor {name}: worst err / bar = {worst:.3f}")
    assert worst <= 1.0
    assert s[4] == np.float32(c["stats"][4]) and s[5] == np.float32(c["stats"][5])
    assert abs(ag.item() - float(c["alpha_grad"])) <= bar(c["alpha_grad"], abs(-(c["target_entropy"] + e32_s[2]) - float(c["alpha_grad"])))


@pytest.mark.parametrize("name", ("mono", "dtde1", "sat"))
@pytest.mark.parametrize("B", (1, 63, 64, 65, 130))
def test_batch_sizes_guarded(name, B):
    """B around the tile size into guarded buffers: nothing outside the outputs is written, the values match the restatement."""
    from gym_rotor_amd import sac_actor_grad
    c = R.case(G, name)
    actor, critic = _params(c)
    D, H, A = actor.dims
    shapes = {"fc1_w": H * D, "fc1_b": H, "fc2_w": H * H, "fc2_b": H, "mean_w": A * H, "mean_b": A, "log_std_w": A * H, "log_std_b": A}
    guard = {n: torch.full((k + 16,), 7.5, device="cuda") for n, k in shapes.items()}
    sg = torch.full((6 + 16,), 7.5, device="cuda")
    idx = np.arange(B)
    sac_actor_grad(actor, critic, _cuda(c["obs"]), _cuda(c["obs_next"]), _idx(idx), grads={n: guard[n][8:8 + k] for n, k in shapes.items()},
                   stats=sg[8:14], **_kw(c, B))
    torch.cuda.synchronize()
    for n, k in shapes.items():
        assert (guard[n][:8] == 7.5).all() and (guard[n][8 + k:] == 7.5).all()
    assert (sg[:8] == 7.5).all() and (sg[14:] == 7.5).all()
    w, q, obs, obs_next, eps, kw = R.inputs(c, idx)
    rs, rg, _ = R.sac_actor_grad_f64(w, q, obs, obs_next, eps, **kw)
    e32_g, e32_s = _eager(c, torch.float32, idx)
    got = {n: _np(guard[n][8:8 + k]).astype(np.float64) for n, k in shapes.items()}
    worst = _worst(got, _np(sg[8:14]).astype(np.float64), rg, rs, e32_g, e32_s)
    print(f"sac_actor {name} B={B}: worst err / bar = {worst:.3f}")
    assert worst <= 1.0
    assert _np(sg[8:14])[4] == np.float32(rs[4]) and _np(sg[8:14])[5] == np.float32(rs[5])


def _bits(g, s):
    return [g[n].tobytes() for n in NAMES] + [s.tobytes()]


def test_index_forms():
    """Identity, permutation, repeats, out-of-range values clamped, NaN in every row the index does not name."""
    c = R.case(G, "mono")
    base = _bits(*_run(c))
    assert _bits(*_run(c, index=np.arange(130))) == base
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 130, 97)
    idx[:4] = idx[4:8]                                  # repeats
    w, q, obs, obs_next, eps, kw = R.inputs(c, idx)
    rs, rg, _ = R.sac_actor_grad_f64(w, q, obs, obs_next, eps, **kw)
    e32_g, e32_s = _eager(c, torch.float32, idx)
    d = dict(c)
    d["obs"], d["obs_next"] = c["obs"].copy(), c["obs_next"].copy()
    unnamed = np.setdiff1d(np.arange(130), idx)
    d["obs"][unnamed] = np.nan
    d["obs_next"][unnamed] = np.nan
    g, s = _run(d, index=idx)
    worst = _worst(g, s, rg, rs, e32_g, e32_s)
    print(f"sac_actor index forms: worst err / bar = {worst:.3f}")
    assert worst <= 1.0
    far = idx.copy()
    far[idx == idx.max()] = 10 ** 12
    far[idx == idx.min()] = -5
    clamped = np.clip(far, 0, 129)
    assert _bits(*_run(c, index=far)) == _bits(*_run(c, index=clamped))


def test_zero_coefficients_skip_their_passes():
    """A zero lam skips its pass bit for bit with NaN in the inputs it would read; each lam alone matches the restatement."""
    c = R.case(G, "mono")
    nan_rows, nan_eps = np.full_like(c["obs_next"], np.nan), _cuda(np.full_like(c["eps"], np.nan))
    nan_noise, nan_nom = _cuda(np.full(23, np.nan, np.float32)), _cuda(np.full(4, np.nan, np.float32))
    for lam in ((0.4, 0.0, 0.0), (0.0, 0.3, 0.0), (0.0, 0.0, 0.6), (0.0, 0.0, 0.0)):
        d = dict(c, lam=lam)
        clean = _run(d)
        over = {}
        if lam[0] == 0:
            d = dict(d, obs_next=nan_rows)
            over["eps_next"] = nan_eps
        if lam[1] == 0:
            over.update(eps_pert=nan_eps, noise=nan_noise)
        if lam[2] == 0:
            over["nominal"] = nan_nom
        if lam == (0.0, 0.0, 0.0):
            over["eps_reg"] = nan_eps
        assert _bits(*_run(d, **over)) == _bits(*clean)
        w, q, obs, obs_next, eps, kw = R.inputs(dict(c, lam=lam))
        rs, rg, _ = R.sac_actor_grad_f64(w, q, obs, obs_next, eps, **kw)
        e32_g, e32_s = _eager(dict(c, lam=lam), torch.float32)
        worst = _worst(*clean, rg, rs, e32_g, e32_s)
        print(f"sac_actor lam={lam}: worst err / bar = {worst:.3f}")
        assert worst <= 1.0


def test_eps_null_is_zeros_bit_for_bit():
    c = R.case(G, "noeps")
    z = _cuda(np.zeros((130, 4), np.float32))
    assert _bits(*_run(c)) == _bits(*_run(c, eps=z, eps_reg=z, eps_next=z, eps_pert=z))


def test_alpha_forms_and_alpha_grad():
    """alpha as a float and as a device tensor: the same bits; alpha_grad against the restatement, and absent changes no other bit."""
    c = R.case(G, "mono")
    base = _bits(*_run(c))
    assert _bits(*_run(c, alpha=torch.tensor([c["alpha"]], dtype=torch.float32, device="cuda"))) == base
    ag = torch.zeros(1, device="cuda")
    assert _bits(*_run(c, alpha_grad=ag, target_entropy=-3.25)) == base
    w, q, obs, obs_next, eps, kw = R.inputs(c)
    kw["target_entropy"] = -3.25
    _, _, want = R.sac_actor_grad_f64(w, q, obs, obs_next, eps, **kw)
    _, e32_s = _eager(c, torch.float32)
    assert abs(ag.item() - want) <= bar(want, abs(-(-3.25 + e32_s[2]) - want))


def test_critics_swapped():
    """Q1 and Q2 swapped: the same gradients within the bar, stats[5] mirrored."""
    c = R.case(G, "mono")
    d = dict(c)
    for k in range(1, 4):
        for x in "wb":
            d[f"c_fc{k}_{x}"], d[f"c_fc{k + 3}_{x}"] = c[f"c_fc{k + 3}_{x}"], c[f"c_fc{k}_{x}"]
    g, s = _run(d)
    e32_g, e32_s = _eager(c, torch.float32)
    worst = _worst(g, s, {n: c["g_" + n] for n in NAMES}, c["stats"], e32_g, e32_s)
    print(f"sac_actor swapped critics: worst err / bar = {worst:.3f}")
    assert worst <= 1.0
    assert s[5] == np.float32(1.0 - c["stats"][5])   # (no tie in the fixture: its |Q1 - Q2| margin)


def test_max_workgroups_deterministic():
    """max_workgroups 1, 2, 3 and 0: each grid gives the same bits twice, and every pair of grids lies within the bar of one another
    (and each within the bar of the fixture)."""
    c = R.case(G, "mono")
    ref_g = {n: c["g_" + n] for n in NAMES}
    e32_g, e32_s = _eager(c, torch.float32)
    runs = {}
    for mw in (1, 2, 3, 0):
        runs[mw], again = _run(c, max_workgroups=mw), _run(c, max_workgroups=mw)
        assert _bits(*runs[mw]) == _bits(*again)
        worst = _worst(*runs[mw], ref_g, c["stats"], e32_g, e32_s)
        print(f"sac_actor max_workgroups={mw}: worst err / bar = {worst:.3f}")
        assert worst <= 1.0
    worst = 0.0
    for i, a in enumerate((1, 2, 3, 0)):
        for b in (1, 2, 3, 0)[i + 1:]:
            for n in NAMES:
                worst = max(worst, np.abs(runs[a][0][n] - runs[b][0][n]).max() / bar(ref_g[n], np.abs(e32_g[n] - ref_g[n]).max()))
            for k in range(4):
                worst = max(worst, abs(runs[a][1][k] - runs[b][1][k]) / bar(c["stats"][k], abs(e32_s[k] - c["stats"][k])))
            assert runs[a][1][4] == runs[b][1][4] and runs[a][1][5] == runs[b][1][5]
    print(f"sac_actor max_workgroups pairwise: worst difference / bar = {worst:.3f}")
    assert worst <= 1.0


def test_short_workspace_refused_nothing_written():
    from gym_rotor_amd import _lib, sac_actor_grad, sac_actor_workspace_bytes
    c = R.case(G, "mono")
    actor, critic = _params(c)
    need = sac_actor_workspace_bytes(actor.dims, 62, 130)
    ws = torch.full((need // 8 - 1,), 3.0, dtype=torch.float64, device="cuda")
    grads = {n: torch.full_like(getattr(actor, n), 5.0) for n in NAMES}
    stats = torch.full((6,), 5.0, device="cuda")
    with pytest.raises(ValueError, match="QR_E_SIZE"):
        sac_actor_grad(actor, critic, _cuda(c["obs"]), _cuda(c["obs_next"]), None, grads=grads, stats=stats, workspace=ws, **_kw(c))
    torch.cuda.synchronize()
    assert (ws == 3.0).all() and (stats == 5.0).all() and all((t == 5.0).all() for t in grads.values())


def test_torch_op_gives_the_ctypes_bits():
    c = R.case(G, "dtde0")
    base = _bits(*_run(c))
    actor, critic = _params(c)
    kw = _kw(c)
    grads = [torch.empty_like(getattr(actor, n)) for n in NAMES]
    stats = torch.empty(6, device="cuda")
    torch.ops.gym_rotor_amd.qr_sac_actor_grad([getattr(actor, n) for n in NAMES], [getattr(critic, n) for n in R.CRITIC_NAMES], 4, _cuda(c["obs"]),
                                              _cuda(c["obs_next"]), None, kw["eps"], kw["eps_reg"], kw["eps_next"], kw["eps_pert"], kw["noise"],
                                              kw["nominal"], grads, stats, None, c["alpha"], c["target_entropy"], *c["lam"], c["max_action"])
    torch.cuda.synchronize()
    assert _bits(dict(zip(NAMES, (_np(t).astype(np.float64) for t in grads))), _np(stats).astype(np.float64)) == base


class _Actor(torch.nn.Module):
    def __init__(self, D, H, A):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(D, H), torch.nn.Linear(H, H)
        self.mean_linear, self.log_std_linear = torch.nn.Linear(H, A), torch.nn.Linear(H, A)


class _Critic(torch.nn.Module):
    def __init__(self, D, A, H):
        super().__init__()
        for k, (i, o) in enumerate(((D + A, H), (H, H), (H, 1)) * 2, 1):
            setattr(self, f"fc{k}", torch.nn.Linear(i, o))


def _live(c):
    from gym_rotor_amd import ReplayBuffer
    D, A, HC = c["obs"].shape[1], c["a_mean_w"].shape[0], c["c_fc1_w"].shape[0]
    actor, critic = _Actor(D, c["a_fc1_w"].shape[0], A).cuda(), _Critic(D, A, HC).cuda()
    with torch.no_grad():
        for m, names, prefix in ((actor, NAMES, "a_"), (critic, R.CRITIC_NAMES, "c_")):
            for n in names:
                layer = getattr(m, {"mean": "mean_linear", "log_std": "log_std_linear"}.get(n[:-2], n[:-2]))
                getattr(layer, "weight" if n.endswith("w") else "bias").copy_(torch.from_numpy(c[prefix + n]))
    buf = ReplayBuffer(130, [D], [A], torch.device("cuda"))
    buf.obs[0].copy_(_cuda(c["obs"]))
    buf.obs_next[0].copy_(_cuda(c["obs_next"]))
    return actor, critic, buf


def test_sac_actor_loss_live_modules():
    """sac_actor_loss end to end on live modules: the .grad tensors carry sac_actor_grad's bits, log_alpha.grad is written, and the
    second call allocates nothing."""
    from gym_rotor_amd import sac_actor_loss
    c = R.case(G, "mono")
    ag = torch.zeros(1, device="cuda")
    g, s = _run(c, alpha_grad=ag)
    actor, critic, buf = _live(c)
    log_alpha = torch.zeros(1, device="cuda", requires_grad=True)
    kw = _kw(c)
    kw.pop("target_entropy")
    stats = sac_actor_loss(actor, critic, buf, 0, None, log_alpha=log_alpha, **kw)
    torch.cuda.synchronize()
    params = [t for l in (actor.fc1, actor.fc2, actor.mean_linear, actor.log_std_linear) for t in (l.weight, l.bias)]
    assert _bits({n: _np(p.grad).astype(np.float64) for n, p in zip(NAMES, params)}, _np(stats).astype(np.float64)) == _bits(g, s)
    assert torch.equal(log_alpha.grad, ag)   # (target_entropy: None is -A, the fixture's)
    before = torch.cuda.memory_allocated()
    sac_actor_loss(actor, critic, buf, 0, None, log_alpha=log_alpha, **kw)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert ("sac_actor", 0, 130, 0) in buf._cache


def test_graph_replay_gives_the_eager_bits():
    """The actor chain captured in one graph (a single chain of launches) and replayed: the eager bits, and again after the device
    alpha changed."""
    from gym_rotor_amd import sac_actor_grad, sac_actor_workspace_bytes
    c = R.case(G, "mono")
    actor, critic = _params(c)
    obs, obs_next = _cuda(c["obs"]), _cuda(c["obs_next"])
    alpha = torch.tensor([c["alpha"]], dtype=torch.float32, device="cuda")
    kw = _kw(c, alpha=alpha)
    grads = {n: torch.empty_like(getattr(actor, n)) for n in NAMES}
    stats = torch.empty(6, device="cuda")
    ws = torch.empty(sac_actor_workspace_bytes(actor.dims, 62, 130) // 8, dtype=torch.float64, device="cuda")
    call = lambda: sac_actor_grad(actor, critic, obs, obs_next, None, grads=grads, stats=stats, workspace=ws, **kw)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for value in (c["alpha"], 0.7):
        alpha.fill_(value)
        call()
        torch.cuda.synchronize()
        eager = [_np(grads[n]).copy() for n in NAMES] + [_np(stats).copy()]
        for t in list(grads.values()) + [stats]:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(a, b) for a, b in zip(eager, [_np(grads[n]) for n in NAMES] + [_np(stats)]))


def test_whole_sac_iteration_on_a_collected_buffer():
    """One whole SAC iteration on a buffer collected from the env with the SAC actor itself (rollout_actor, ReplayBuffer.add, capacity
    above the current size, the index from ReplayBuffer.sample): sac_critic_loss and the critic's optimiser steps, sac_actor_loss with
    log_alpha, DeviceAdamW on the actor's eight tensors and on log_alpha, exp, soft_update.  Everything stays finite and the actor's
    own objective mean(alpha logp - min Q) over the minibatch (same draws, same critic, same alpha) falls across the actor step."""
    from gym_rotor_amd import (ActorParams, DeviceAdamW, QuadVecEnv, ReplayBuffer, RolloutStorage, sac_actor_loss, sac_critic_loss, soft_update)
    T, N, B = 3, 70, 128
    torch.manual_seed(13)
    env = QuadVecEnv("coupled", N, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=100, seed=23)
    env.reset("train")
    actor, critic, critic_t = _Actor(23, 16, 4).cuda(), _Critic(23, 4, 62).cuda(), _Critic(23, 4, 62).cuda()
    critic_t.load_state_dict(critic.state_dict())
    storage = RolloutStorage(env, T)
    storage.set_initial_obs(env.get_norm_error_state())
    env.rollout_actor([ActorParams.from_sac_module(actor)], T, out=storage.horizon(), noise_seed=7)
    buf = ReplayBuffer(1000, env.obs_dims, [4], "cuda")
    buf.add(storage)
    assert buf.current_size == T * N < buf.capacity
    g = torch.Generator(device="cuda").manual_seed(4)
    index = buf.sample(B, g)
    eps = [torch.randn(B, 4, device="cuda", generator=g) for _ in range(5)]
    noise, nominal = 0.05 * torch.randn(23, device="cuda", generator=g), torch.tensor([-0.3, 0.0, 0.0, 0.0], device="cuda")
    log_alpha = torch.full((1,), float(np.log(0.2)), device="cuda", requires_grad=True)
    alpha = log_alpha.detach().exp()
    a_params = [t for l in (actor.fc1, actor.fc2, actor.mean_linear, actor.log_std_linear) for t in (l.weight, l.bias)]
    q_params = list(critic.parameters())
    kw = dict(eps=eps[0], eps_reg=eps[1], eps_next=eps[2], eps_pert=eps[3], noise=noise, nominal=nominal)
    stats_q = sac_critic_loss(critic, critic_t, actor, buf, 0, index, alpha=alpha, noise=eps[4])
    DeviceAdamW.step_all([DeviceAdamW(q_params[:6], lr=2e-4), DeviceAdamW(q_params[6:], lr=2e-4)])
    full = sac_actor_loss(actor, critic, buf, 0, index, log_alpha=log_alpha, alpha=alpha, **kw).clone()   # all four passes
    own = dict(kw, lam_T=0.0, lam_S=0.0, lam_M=0.0)                                                         # the objective below is the loss pass's
    before = sac_actor_loss(actor, critic, buf, 0, index, log_alpha=log_alpha, alpha=alpha, **own).clone()
    a0 = alpha.clone()
    DeviceAdamW.step_all([DeviceAdamW(a_params, lr=3e-3), DeviceAdamW([log_alpha], lr=3e-4)])
    torch.exp(log_alpha.detach(), out=alpha)
    targets = [p.data.clone() for p in critic_t.parameters()]
    soft_update(critic, critic_t, 0.005)
    after = sac_actor_loss(actor, critic, buf, 0, index, log_alpha=log_alpha, alpha=a0, **own)
    torch.cuda.synchronize()
    for t in [stats_q, full, before, after, alpha, log_alpha.grad] + [p.data for p in a_params + q_params] + [p.grad for p in a_params]:
        assert torch.isfinite(t).all()
    assert not torch.equal(alpha, a0) and all(not torch.equal(a, b.data) for a, b in zip(targets, critic_t.parameters()))
    objective = lambda s: a0.item() * s[2].item() - s[1].item()
    assert abs(objective(before) - before[0].item()) <= 1e-5 * max(1.0, abs(objective(before)))   # with no smoothness term it IS the loss
    print(f"sac_actor iteration: objective {objective(before):+.6f} -> {objective(after):+.6f}, alpha {a0.item():.6f} -> {alpha.item():.6f}, "
          f"full loss {full[0].item():+.6f}")
    assert objective(after) < objective(before)
