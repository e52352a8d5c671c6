"""qr_ctde_sac_actor_grad on the device against tests/golden/sac_ctde_actor.npz (the reference's float64 autograd;
tools/gen_golden_sac_ctde_actor.py) and the float64 restatement (tests/sac_ctde_actor_ref.py).  The bar is DESIGN.md §8.6's through
twinq_gpu_util.bar: err <= max(2e-6 * max(1, |x64|), e32), e32 the error of eager float32 torch autograd on the same inputs on the
device, no factor on it.  Each accuracy test prints its worst err / bar per case."""
import numpy as np
import pytest
import torch

import sac_ctde_actor_ref as R
from test_ctde_critic_host import _SacActor, _Twin
from twinq_gpu_util import _cuda, _idx, _np, bar

pytestmark = pytest.mark.gpu

G = R.load()
NAMES = R.ACTOR_NAMES
DIMS = ((15, 16, 4), (3, 4, 1))
BOTH = tuple(n for n in R.CASES if n not in R.SUPPLIED)
DRAWS = ("eps", "eps_other", "eps_logp", "eps_reg", "eps_next", "eps_pert")


def _actor(c, m):
    from gym_rotor_amd import ActorParams, _lib
    w = R.actor_of(c, m)
    if w is None:
        return None
    w = [_cuda(t) for t in w]
    return ActorParams(*w[:6], None, w[6], w[7], _lib.ACTOR_TANH_SAMPLE)


def _critic(c, q_swap=False):
    from gym_rotor_amd import QCriticParams
    q = [_cuda(t) for t in R.critic_of(c)]
    return QCriticParams(*(q[6:] + q[:6] if q_swap else q), action_dim=c["other_action"].shape[1] + c["nominal"].shape[0])


def _kw(c, B, **over):
    kw = dict(k=c["k"], alpha=c["alpha"], lam_T=c["lam"][0], lam_S=c["lam"][1], lam_M=c["lam"][2], max_action=c["max_action"],
              noise=_cuda(c["noise"].astype(np.float32)), nominal=_cuda(c["nominal"].astype(np.float32)), target_entropy=c["target_entropy"])
    e = R.case_eps(c, np.arange(B))
    for n in DRAWS:
        kw[n] = _cuda(e[n]) if n in e else None
    if "action_other" in c:
        kw["action_other"] = _cuda(c["action_other"][:B])
    kw.update(over)
    return kw


def _call(c, index=None, supplied=None, q_swap=False, **over):
    """sac_actor_grad_ctde on a fixture case; supplied: a [B, A_other] array that stands in for the other agent's actor."""
    from gym_rotor_amd import sac_actor_grad_ctde
    k = c["k"]
    actors = [_actor(c, 0), _actor(c, 1)]
    n = 130 if index is None else len(index)
    if supplied is not None:
        actors[1 - k] = None
        over = dict(over, action_other=_cuda(np.asarray(supplied, dtype=np.float32)), eps_other=None)
    obs, nxt = [_cuda(c["obs0"]), _cuda(c["obs1"])], [_cuda(c["obs_next0"]), _cuda(c["obs_next1"])]
    out = sac_actor_grad_ctde(actors, _critic(c, q_swap), obs, nxt, _idx(index), **_kw(c, n, **over))
    torch.cuda.synchronize()
    return out


def _run(c, **kw):
    grads, stats = _call(c, **kw)
    return {n: _np(v).astype(np.float64) for n, v in grads.items()}, _np(stats).astype(np.float64)


def _eager(c, dtype, index=None, q_swap=False, lam=None, drop=(), same_logp=False, supplied=None):
    """The reference's lines (sac.py:176-190, policy_regularization) in eager torch autograd on the device in `dtype`: (agent k's grads,
    stats[:4]).  Normal(mean, std).log_prob(u) is written out with -eps^2 / 2 formed from eps (as
    -(u - mean)^2 / (2 std^2) it cancels in float32 where std is exp(-20))."""
    idx = np.arange(130) if index is None else np.asarray(index)
    k = c["k"]
    w = [None if R.actor_of(c, m) is None else [_cuda(t, dtype) for t in R.actor_of(c, m)] for m in (0, 1)]
    for t in w[k]:
        t.requires_grad_()
    q = [_cuda(t, dtype) for t in R.critic_of(c)]
    if q_swap:
        q = q[6:] + q[:6]
    x = [_cuda(c[f"obs{m}"][idx], dtype) for m in (0, 1)]
    xn = _cuda(c[f"obs_next{k}"][idx], dtype)
    e = {n: _cuda(v, dtype) for n, v in R.case_eps(c, idx).items() if n not in drop}
    if same_logp:
        e["eps_logp"] = e["eps"]
    lam_T, lam_S, lam_M = c["lam"] if lam is None else lam
    ma = c["max_action"]

    def sample(w, x, eps):
        h = torch.relu(torch.relu(x @ w[0].T + w[1]) @ w[2].T + w[3])
        mean, ls = h @ w[4].T + w[5], torch.clamp(h @ w[6].T + w[7], -20.0, 2.0)
        eps = torch.zeros_like(mean) if eps is None else eps
        a = torch.tanh(mean + ls.exp() * eps)
        lp = -0.5 * eps * eps - ls - 0.5 * float(np.log(2 * np.pi)) - torch.log((1 - a.pow(2)) + 1e-6)
        return a, lp.sum(1, keepdim=True)

    a_k, lp = sample(w[k], x[k], e.get("eps"))
    if "eps_logp" in e:
        lp = sample(w[k], x[k], e["eps_logp"])[1]
    if supplied is not None:
        a_o = _cuda(np.asarray(supplied, dtype=np.float32)[:len(idx)], dtype)
    elif "action_other" in c:
        a_o = _cuda(c["action_other"][:len(idx)], dtype)
    else:
        with torch.no_grad():
            a_o = sample(w[1 - k], x[1 - k], e.get("eps_other"))[0]
    sa = torch.cat(x + ([a_k, a_o] if k == 0 else [a_o, a_k]), 1)
    Q = lambda j: torch.relu(torch.relu(sa @ q[6 * j].T + q[6 * j + 1]) @ q[6 * j + 2].T + q[6 * j + 3]) @ q[6 * j + 4].T + q[6 * j + 5]
    qmin = torch.min(Q(0), Q(1))
    loss = -(qmin - c["alpha"] * lp).mean()
    total = loss
    mse = torch.nn.functional.mse_loss
    if lam_T or lam_S or lam_M:
        r = sample(w[k], x[k], e.get("eps_reg"))[0].clamp(-ma, ma)
        if lam_T:
            total = total + lam_T * mse(r, sample(w[k], xn, e.get("eps_next"))[0].clamp(-ma, ma))
        if lam_S:
            total = total + lam_S * mse(r, sample(w[k], x[k] + _cuda(c["noise"], dtype)[None, :], e.get("eps_pert"))[0].clamp(-ma, ma))
        if lam_M:
            total = total + lam_M * mse(r, _cuda(c["nominal"], dtype)[None, :].expand_as(r))
    total.backward()
    grads = {n: _np(t.grad).astype(np.float64) for n, t in zip(NAMES, w[k])}
    return grads, np.array([total.item(), qmin.mean().item(), lp.mean().item(), (total - loss).item()], dtype=np.float64)


def _worst(got_g, got_s, ref_g, ref_s, e32_g, e32_s):
    worst = 0.0
    for n in NAMES:
        worst = max(worst, np.abs(got_g[n].reshape(ref_g[n].shape) - ref_g[n]).max() / bar(ref_g[n], np.abs(e32_g[n] - ref_g[n]).max()))
    for j in range(4):
        worst = max(worst, abs(got_s[j] - ref_s[j]) / bar(ref_s[j], abs(e32_s[j] - ref_s[j])))
    return worst


def _bits(g, s):
    return [_np(g[n]).tobytes() for n in NAMES] + [_np(s).tobytes()]


@pytest.mark.parametrize("name", R.CASES)
def test_fixture_cases_in_both_forms(name):
    """Every fixture case against the reference's float64 autograd: eight gradients, six stats (the two shares exact) and alpha's
    gradient; then, where the case has both actors, the supplied form fed with the reference's float64 other action rounded to float32."""
    c = R.case(G, name)
    ref_g = {n: c["g_" + n] for n in NAMES}
    e32_g, e32_s = _eager(c, torch.float32)
    forms = [("as stored", None)] + ([] if name in R.SUPPLIED else [("supplied", c["other_action"].astype(np.float32))])
    for form, ao in forms:
        ag = torch.full((1,), float("nan"), device="cuda")
        g, s = _run(c, supplied=ao, alpha_grad=ag)
        worst = _worst(g, s, ref_g, c["stats"], e32_g, e32_s)
        print(f"sac_ctde_actor {name} ({form}): worst err / bar = {worst:.3f}")
        assert worst <= 1.0
        assert s[4] == np.float32(c["stats"][4]) and s[5] == np.float32(c["stats"][5])
        assert abs(ag.item() - float(c["alpha_grad"])) <= bar(c["alpha_grad"], abs(-(c["target_entropy"] + e32_s[2]) - float(c["alpha_grad"])))


@pytest.mark.parametrize("name", ("k0", "k1"))
def test_each_coefficient_alone_and_zero_coefficients_skip_their_inputs(name):
    c = R.case(G, name)
    nan = lambda t: torch.full_like(t, float("nan"))
    for j in range(3):
        lam = tuple(c["lam"][i] if i == j else 0.0 for i in range(3))
        over = dict(lam_T=lam[0], lam_S=lam[1], lam_M=lam[2])
        g, s = _run(c, **over)
        rs, rg, _ = R.case_f64(c, lam=lam)
        e32_g, e32_s = _eager(c, torch.float32, lam=lam)
        worst = _worst(g, s, rg, rs, e32_g, e32_s)
        print(f"sac_ctde_actor {name} lam {lam}: worst err / bar = {worst:.3f}")
        assert worst <= 1.0
        # a zero coefficient reads none of its inputs: NaN there, the same bits
        kw = _kw(c, 130, **over)
        poison = {}
        if lam[0] == 0:
            poison["eps_next"] = nan(kw["eps_next"])
        if lam[1] == 0:
            poison.update(eps_pert=nan(kw["eps_pert"]), noise=nan(kw["noise"]))
        if lam[2] == 0:
            poison["nominal"] = nan(kw["nominal"])
        assert _bits(*_call(c, **over, **poison)) == _bits(*_call(c, **over))
    zero = dict(lam_T=0.0, lam_S=0.0, lam_M=0.0)
    kw = _kw(c, 130)
    poison = {n: nan(kw[n]) for n in ("eps_reg", "eps_next", "eps_pert", "noise", "nominal")}
    assert _bits(*_call(c, **zero, **poison)) == _bits(*_call(c, **zero))


@pytest.mark.parametrize("name", ("k0", "k1", "sat1", "w28"))
@pytest.mark.parametrize("B", (1, 63, 64, 65, 130))
def test_batch_sizes_into_guarded_buffers(name, B):
    c = R.case(G, name)
    D, H, A = DIMS[c["k"]]
    shapes = {"fc1_w": H * D, "fc1_b": H, "fc2_w": H * H, "fc2_b": H, "mean_w": A * H, "mean_b": A, "log_std_w": A * H, "log_std_b": A}
    guard = {n: torch.full((m + 16,), 7.5, device="cuda") for n, m in shapes.items()}
    sg = torch.full((6 + 16,), 7.5, device="cuda")
    idx = np.arange(B)
    views = {n: guard[n][8:8 + m].view((H, D) if n == "fc1_w" else (H, H) if n == "fc2_w" else (A, H) if n.endswith("_w") else (m,)) for n, m in shapes.items()}
    _call(c, index=idx, grads=views, stats=sg[8:14])
    for n, m in shapes.items():
        assert (guard[n][:8] == 7.5).all() and (guard[n][8 + m:] == 7.5).all()
    assert (sg[:8] == 7.5).all() and (sg[14:] == 7.5).all()
    rs, rg, _ = R.case_f64(c, idx)
    e32_g, e32_s = _eager(c, torch.float32, idx)
    got = {n: _np(guard[n][8:8 + m]).astype(np.float64) for n, m in shapes.items()}
    gs = _np(sg[8:14]).astype(np.float64)
    worst = _worst(got, gs, rg, rs, e32_g, e32_s)
    print(f"sac_ctde_actor {name} B={B}: worst err / bar = {worst:.3f}")
    assert worst <= 1.0 and gs[4] == np.float32(rs[4]) and gs[5] == np.float32(rs[5])


@pytest.mark.parametrize("name", ("k0", "k1"))
def test_index_forms(name):
    """Permuted, repeated and 70-of-130 indices (the draws stay by minibatch position), against the restatement on those rows."""
    c = R.case(G, name)
    rng = np.random.default_rng(5)
    rep = rng.integers(0, 130, 130)
    rep[:6] = rep[6:12]
    for what, idx in (("permuted", rng.permutation(130)), ("repeated", rep), ("70 of 130", rng.permutation(130)[:70])):
        g, s = _run(c, index=idx)
        rs, rg, _ = R.case_f64(c, idx)
        e32_g, e32_s = _eager(c, torch.float32, idx)
        worst = _worst(g, s, rg, rs, e32_g, e32_s)
        print(f"sac_ctde_actor {name} index {what}: worst err / bar = {worst:.3f}")
        assert worst <= 1.0
    assert _bits(*_call(c, index=np.arange(130))) == _bits(*_call(c))


@pytest.mark.parametrize("name", ("k0", "k1"))
def test_grids_and_repeated_calls(name):
    c = R.case(G, name)
    ref_g, (e32_g, e32_s) = {n: c["g_" + n] for n in NAMES}, _eager(c, torch.float32)
    for mw in (1, 2, 3, 0):
        first = _call(c, max_workgroups=mw)
        worst = _worst(*[{n: _np(v).astype(np.float64) for n, v in first[0].items()}, _np(first[1]).astype(np.float64)], ref_g, c["stats"], e32_g, e32_s)
        print(f"sac_ctde_actor {name} max_workgroups={mw}: worst err / bar = {worst:.3f}")
        assert worst <= 1.0
        assert _bits(*_call(c, max_workgroups=mw)) == _bits(*first)           # a repeated call: the same bits
    assert _bits(*_call(c, max_workgroups=3)) == _bits(*_call(c, max_workgroups=0))   # three tiles: the same grid


@pytest.mark.parametrize("name", ("k0", "k1"))
def test_critics_swapped(name):
    c = R.case(G, name)
    g, s = _run(c, q_swap=True)
    e32_g, e32_s = _eager(c, torch.float32, q_swap=True)
    worst = _worst(g, s, {n: c["g_" + n] for n in NAMES}, c["stats"], e32_g, e32_s)
    print(f"sac_ctde_actor {name} Q1 <-> Q2: worst err / bar = {worst:.3f}")
    assert worst <= 1.0 and abs(s[5] - (1.0 - c["stats"][5])) <= 1e-6


@pytest.mark.parametrize("name", ("k0", "k1", "onedraw"))
def test_logp_draw_given_as_the_first_draw_is_the_one_draw_form(name):
    """eps_logp = the tensor given as eps, against eps_logp None: one sample either way, summed in another order, so within the bar of
    the restatement's one-draw form and not bit for bit."""
    c = R.case(G, name)
    kw = _kw(c, 130)
    a, fkw = R.case_args(c)
    one = {n: v for n, v in a[6].items() if n != "eps_logp"}
    rs, rg, _ = R.ctde_sac_actor_grad_f64(*a[:6], one, **fkw)
    e32_g, e32_s = _eager(c, torch.float32, drop=("eps_logp",))
    for what, over in (("None", dict(eps_logp=None)), ("the same tensor", dict(eps_logp=kw["eps"]))):
        g, s = _run(c, **over)
        worst = _worst(g, s, rg, rs, e32_g, e32_s)
        print(f"sac_ctde_actor {name} eps_logp {what}: worst err / bar = {worst:.3f}")
        assert worst <= 1.0


@pytest.mark.parametrize("name", ("k0", "k1"))
def test_bitwise_equal_forms(name):
    """Draws None against zeros where the code path is the same (not eps_logp: None is the one-draw form); alpha as a float and as a
    device tensor; alpha_grad given or not."""
    c = R.case(G, name)
    kw = _kw(c, 130)
    for n in ("eps", "eps_other", "eps_reg", "eps_next", "eps_pert"):
        assert _bits(*_call(c, **{n: None})) == _bits(*_call(c, **{n: torch.zeros_like(kw[n])})), n
    base = _bits(*_call(c))
    assert _bits(*_call(c, alpha=torch.tensor([c["alpha"]], dtype=torch.float32, device="cuda"))) == base
    ag = torch.full((1,), float("nan"), device="cuda")
    assert _bits(*_call(c, alpha_grad=ag)) == base and np.isfinite(ag.item())


@pytest.mark.parametrize("name", ("k0", "k1", "w28"))
def test_torch_op_gives_the_python_function_bits(name):
    c = R.case(G, name)
    k = c["k"]
    kw = _kw(c, 130)
    ag0, ag1 = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    base = _call(c, alpha_grad=ag0)
    lists = [[] if R.actor_of(c, m) is None else [_cuda(t) for t in R.actor_of(c, m)] for m in (0, 1)]
    grads = [torch.empty_like(base[0][n]) for n in NAMES]
    stats = torch.empty(6, device="cuda")
    torch.ops.gym_rotor_amd.qr_ctde_sac_actor_grad(lists[0], lists[1], [_cuda(t) for t in R.critic_of(c)], k, _cuda(c["obs0"]), _cuda(c["obs1"]),
                                                   _cuda(c[f"obs_next{k}"]), None, kw.get("action_other"), kw["eps"], kw["eps_logp"], kw["eps_other"],
                                                   kw["eps_reg"], kw["eps_next"], kw["eps_pert"], kw["noise"], kw["nominal"], grads, stats, ag1,
                                                   c["alpha"], c["target_entropy"], *c["lam"], c["max_action"])
    torch.cuda.synchronize()
    assert _bits(dict(zip(NAMES, grads)), stats) == _bits(*base) and ag0.item() == ag1.item()


def _fill(m, tensors, names):
    with torch.no_grad():
        for n, t in zip(names, tensors):
            layer = {"fc1": "fc1", "fc2": "fc2", "mean": "mean_linear", "log_std": "log_std_linear"}.get(n[:-2], n[:-2])
            getattr(getattr(m, layer), "weight" if n.endswith("w") else "bias").copy_(torch.from_numpy(t))
    return m.cuda()


def _live(c):
    """Both live actors, the centralized twin critic and a two-agent buffer holding the case's rows."""
    from gym_rotor_amd import ReplayBuffer
    actors = [_fill(_SacActor(*DIMS[m]), R.actor_of(c, m), NAMES) for m in (0, 1)]
    critic = _fill(_Twin(23, c["c_fc1_w"].shape[0]), R.critic_of(c), R.CRITIC_NAMES)
    buf = ReplayBuffer(130, [15, 3], [4, 1], "cuda")
    for m in (0, 1):
        buf.obs[m].copy_(_cuda(c[f"obs{m}"]))
        buf.obs_next[m].copy_(_cuda(c[f"obs_next{m}"]))
    buf.count, buf.current_size = 0, 130
    return actors, critic, buf


def _own(m):
    return [t for l in (m.fc1, m.fc2, m.mean_linear, m.log_std_linear) for t in (l.weight, l.bias)]


def _loss_kw(c):
    kw = _kw(c, 130)
    kw.pop("k")
    kw.pop("target_entropy")
    return kw


@pytest.mark.parametrize("name", ("k0", "k1", "sat1"))
def test_sac_actor_loss_ctde_on_live_modules(name):
    from gym_rotor_amd import sac_actor_loss_ctde
    c = R.case(G, name)
    k = c["k"]
    actors, critic, buf = _live(c)
    other = _own(actors[1 - k])
    other[0].grad = torch.full_like(other[0], 3.5)
    held = [p.grad for p in other]
    log_alpha = torch.zeros(1, device="cuda", requires_grad=True)
    kw = _loss_kw(c)
    stats = sac_actor_loss_ctde(actors, critic, buf, k, None, log_alpha=log_alpha, **kw)
    torch.cuda.synchronize()
    grads = dict(zip(NAMES, (p.grad for p in _own(actors[k]))))
    base = _call(c, alpha_grad=torch.zeros(1, device="cuda"))
    assert _bits(grads, stats) == _bits(*base)                                     # the function's bits, so inside the bar of the fixture
    assert abs(log_alpha.grad.item() - float(c["alpha_grad"])) <= 1e-5 * max(1.0, abs(float(c["alpha_grad"])))
    before, s0 = [g.clone() for g in grads.values()], stats.clone()
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    stats2 = sac_actor_loss_ctde(actors, critic, buf, k, None, log_alpha=log_alpha, **kw)               # allocates nothing, the same bits
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem
    assert stats2.data_ptr() == stats.data_ptr() and torch.equal(stats2, s0) and all(torch.equal(a, b) for a, b in zip(grads.values(), before))
    assert all(a is b for a, b in zip(held, (p.grad for p in other))) and all(g is None for g in held[1:]) and bool((held[0] == 3.5).all())
    assert all(torch.equal(p.data, _cuda(t)) for p, t in zip(other, R.actor_of(c, 1 - k)))


@pytest.mark.parametrize("name", ("k0", "k1"))
def test_captured_graph_replays_the_eager_bits(name):
    """sac_actor_loss_ctde captured once: the replay gives the eager bits, and again after the device alpha changed."""
    from gym_rotor_amd import sac_actor_loss_ctde
    c = R.case(G, name)
    k = c["k"]
    kw = _loss_kw(c)

    def fresh():
        actors, critic, buf = _live(c)
        log_alpha = torch.zeros(1, device="cuda", requires_grad=True)
        alpha = torch.full((1,), c["alpha"], device="cuda")
        for p in _own(actors[k]) + [log_alpha]:
            p.grad = torch.zeros_like(p)
        return actors, critic, buf, log_alpha, alpha

    def step(actors, critic, buf, log_alpha, alpha):
        return sac_actor_loss_ctde(actors, critic, buf, k, None, log_alpha=log_alpha, **{**kw, "alpha": alpha})

    def bits(state, stats):
        torch.cuda.synchronize()
        return [_np(p.grad).tobytes() for p in _own(state[0][k]) + [state[3]]] + [_np(stats).tobytes()]

    eager = fresh()
    e1 = bits(eager, step(*eager))
    eager[4].fill_(0.7)
    e2 = bits(eager, step(*eager))
    cap = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*cap)                                                                 # warm-up: the cache is filled outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stats = step(*cap)
    for p in _own(cap[0][k]) + [cap[3]]:
        p.grad.zero_()
    graph.replay()
    assert bits(cap, stats) == e1
    cap[4].fill_(0.7)
    graph.replay()
    assert bits(cap, stats) == e2 and e1 != e2


def _objective_f64(actors, critic, obs, k, alpha, eps):
    """mean(alpha logp - min Q) of the one-draw form, recomputed in float64 on the CPU from the live weights and the given draws."""
    w = [[_np(p.data).astype(np.float64) for p in _own(a)] for a in actors]
    q = [_np(p.data).astype(np.float64) for p in critic.parameters()]
    x = [_np(o).astype(np.float64) for o in obs]
    e = {"eps": _np(eps[k]), "eps_other": _np(eps[1 - k])}
    s = R.ctde_sac_actor_grad_f64(w, q, x, None, k, None, e, noise=None, nominal=None, lam=(0.0, 0.0, 0.0), max_action=1.0, alpha=alpha,
                                  target_entropy=0.0)[0]
    return float(s[0])


@pytest.mark.parametrize("k", (0, 1))
def test_one_written_out_ctde_sac_iteration(k):
    """sac_critic_loss_ctde, optimiser steps, sac_actor_loss_ctde with log_alpha, exp, soft_update — no autograd — on a Decoupled buffer
    collected with the SAC actors themselves.  The actor's objective with the same draws is lower after agent k's step."""
    from gym_rotor_amd import (ActorParams, DeviceAdamW, QuadVecEnv, ReplayBuffer, RolloutStorage, sac_actor_loss_ctde, sac_critic_loss_ctde,
                               soft_update)
    T, N, B = 4, 64, 64
    torch.manual_seed(41 + k)
    env = QuadVecEnv("decoupled", N, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=100, seed=21)
    env.reset("train")
    actors, critic, critic_t = [_SacActor(*d).cuda() for d in DIMS], _Twin(23, 62).cuda(), _Twin(23, 62).cuda()
    critic_t.load_state_dict(critic.state_dict())
    storage = RolloutStorage(env, T)
    storage.set_initial_obs(env.get_norm_error_state())
    env.rollout_actor([ActorParams.from_sac_module(a) for a in actors], T, out=storage.horizon(), noise_seed=5)
    buf = ReplayBuffer(1000, env.obs_dims, [4, 1], "cuda")
    buf.add(storage)
    g = torch.Generator(device="cuda").manual_seed(2)
    idx = buf.sample(B, g)
    draw = lambda: (torch.randn(B, 4, device="cuda", generator=g), torch.randn(B, 1, device="cuda", generator=g))
    eps_c, eps_a = draw(), draw()
    log_alpha = torch.zeros(1, device="cuda", requires_grad=True)
    alpha = torch.exp(log_alpha.detach())
    cp = list(critic.parameters())
    for p in _own(actors[k]) + cp + [log_alpha]:
        p.grad = torch.zeros_like(p)
    copts = [DeviceAdamW(cp[:6], lr=1e-3, max_norm=-1), DeviceAdamW(cp[6:], lr=1e-3, max_norm=-1)]
    aopt, lopt = DeviceAdamW(_own(actors[k]), lr=1e-4, max_norm=-1), DeviceAdamW([log_alpha], lr=1e-3, max_norm=-1)
    obs = [buf.obs[m][idx] for m in (0, 1)]
    other = [p.data.clone() for p in actors[1 - k].parameters()]
    sac_critic_loss_ctde(critic, critic_t, actors, buf, k, idx, alpha=alpha, noise=eps_c)
    DeviceAdamW.step_all(copts)
    torch.cuda.synchronize()
    a0 = float(alpha.item())
    before = _objective_f64(actors, critic, obs, k, a0, eps_a)
    stats = sac_actor_loss_ctde(actors, critic, buf, k, idx, log_alpha=log_alpha, alpha=alpha, lam_T=0.0, lam_S=0.0, lam_M=0.0, eps=eps_a[k],
                                eps_other=eps_a[1 - k])
    aopt.step()
    lopt.step()
    torch.exp(log_alpha.detach(), out=alpha)
    torch.cuda.synchronize()
    after = _objective_f64(actors, critic, obs, k, a0, eps_a)
    print(f"ctde sac iteration k={k}: mean(alpha logp - min Q) {before:.8f} -> {after:.8f} (stats {stats.tolist()}, alpha {a0} -> {alpha.item():.6f})")
    assert all(bool(torch.isfinite(p.grad).all()) for p in _own(actors[k]) + cp + [log_alpha])
    assert abs(float(stats[0]) - before) <= 1e-5 * max(1.0, abs(before)) and after < before
    tb = [p.data.clone() for p in critic_t.parameters()]
    soft_update(critic, critic_t, 0.005)
    assert all(not torch.equal(a, b.data) for a, b in zip(tb, critic_t.parameters()))
    assert all(torch.equal(a, p.data) for a, p in zip(other, actors[1 - k].parameters())) and all(p.grad is None for p in actors[1 - k].parameters())
