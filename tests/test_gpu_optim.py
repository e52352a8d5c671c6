"""The device-side optimiser step (adamw_step_kernel: qr_adamw_step, DeviceAdamW, the torch op) and PpoUpdater on the GPU, against
the float64 restatement of tests/optim_ref.py and torch's own float32 clip_grad_norm_ + AdamW + CosineAnnealingWarmRestarts.

The bar, per tensor after k steps: max(C_E32 * e32, k * 2^-24 * (4 max|x64| + 16 lr)), x = the parameters, exp_avg or
exp_avg_sq, e32 = the error of TORCH's float32 path — never the kernel's — on the same inputs against the same float64.  The second
term counts roundings: two in the decay product and one in the final subtraction, relative to |p|; about ten in the update term, whose
size is a small multiple of lr.  Each test prints the worst err / bar it saw before it asserts (pytest -s).

The hyperparameters the C-ABI holds as float32 (betas, eps, weight_decay, max_norm) are given as float32-representable numbers, so
that the kernel, the restatement and torch all compute with the same values."""
import copy

import numpy as np
import pytest
import torch

from optim_ref import run_f64, run_torch, schedule
from test_critic_host import _Critic
from test_ppo_actor_host import _Actor

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
C_E32 = 1.0                                   # the factor on e32: first run with 2, which was not needed
K = 5
f32 = lambda v: float(np.float32(v))
ACTOR = lambda D, H, A: [(H, D), (H,), (H, H), (H,), (A, H), (A,), (1, A)]
CRITIC = lambda D, H: [(H, D), (H,), (H, H), (H,), (1, H), (1,)]
GROUPS = {"actor_3_4_1": ACTOR(3, 4, 1), "actor_23_16_4": ACTOR(23, 16, 4), "critic_23_62": CRITIC(23, 62), "critic_1_1": CRITIC(1, 1)}
NUMEL = {"actor_3_4_1": 42, "actor_23_16_4": 728, "critic_23_62": 5457, "critic_1_1": 6}
NORMS = (0.4, 2.5, 0.9, 6.0, 0.7)             # total_norm of the k = 5 gradient sets: above max_norm = 1 in steps 2 and 4
HYPER = dict(lr=3e-4, betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(1e-2), max_norm=1.0, t0=3, eta_min=1e-5)


def _np(t):
    return t.detach().cpu().numpy()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(name, seed=0):
    """Float32 parameters and K gradient sets for a group: random, independent of the parameters (no feedback: errors do not
    amplify), the gradient sets scaled to the total norms NORMS."""
    rng = np.random.default_rng([seed, NUMEL[name]])
    shapes = GROUPS[name]
    p = [(rng.uniform(-1, 1, s) * 0.5).astype(np.float32) for s in shapes]
    sets = []
    for norm in NORMS:
        g = [rng.normal(size=s) for s in shapes]
        scale = norm / np.sqrt(sum((a * a).sum() for a in g))
        sets.append([(a * scale).astype(np.float32) for a in g])
    return p, sets


@pytest.fixture(scope="module")
def data():
    """Per group: the inputs, the float64 results after K steps and torch's float32 results on the GPU — computed once, never changed."""
    out = {}
    for name in GROUPS:
        p, sets = _inputs(name)
        assert sum(a.size for a in p) == NUMEL[name]
        out[name] = dict(p=p, sets=sets, f64=run_f64(p, sets, **HYPER), t32=run_torch(p, sets, torch.float32, "cuda", **HYPER))
    return out


def _device_run(p, sets, hyper, opt_out=None):
    """K steps of a fresh DeviceAdamW on clones.  Returns (parameters, exp_avg, exp_avg_sq as per-tensor float32 tensors, the optimiser,
    stats per step)."""
    from gym_rotor_amd import DeviceAdamW
    params = [torch.nn.Parameter(_cuda(a)) for a in p]
    opt = DeviceAdamW(params, **hyper)
    hist = []
    for g in sets:
        for q, gk in zip(params, g):
            q.grad = _cuda(gk)
        opt.step()
        hist.append(opt.stats.clone())
    torch.cuda.synchronize()
    sizes = [q.numel() for q in params]
    return [q.data for q in params], list(opt.exp_avg.split(sizes)), list(opt.exp_avg_sq.split(sizes)), opt, hist


def _check(label, got, f64, t32, k, lr):
    """Parameters, exp_avg and exp_avg_sq (three lists of tensors) within the bar.  Prints the worst err / bar and which term of the bar
    was the larger one there; returns that ratio."""
    worst, worst1 = (0.0, "", 0.0, 0.0, 0.0), 0.0
    for what, gs, ws, ts in zip(("p", "m", "v"), got, f64[:3], t32[:3]):
        for j, (g, w, t) in enumerate(zip(gs, ws, ts)):
            g = _np(g).astype(np.float64).reshape(w.shape)
            assert np.isfinite(g).all(), (label, what, j)
            err, e32 = float(np.abs(g - w).max()), float(np.abs(t.reshape(w.shape) - w).max())
            rounding = k * 2.0 ** -24 * (4 * float(np.abs(w).max()) + 16 * lr)
            worst = max(worst, (err / max(C_E32 * e32, rounding), f"{what}[{j}]", err, e32, rounding))
            worst1 = max(worst1, err / max(e32, rounding))
    print(f"adamw {label}: worst err / bar = {worst[0]:.3f} at {worst[1]} (err {worst[2]:.3e}, e32 {worst[3]:.3e}, rounding term {worst[4]:.3e}: "
          f"the {'e32' if C_E32 * worst[3] > worst[4] else 'rounding'} term is the larger); with a factor 1 on e32: {worst1:.3f}")
    assert worst[0] <= 1.0, (label, worst)
    return worst[0]


@pytest.mark.parametrize("name", list(GROUPS))
def test_against_float64(data, name):
    d = data[name]
    p, m, v, opt, hist = _device_run(d["p"], d["sets"], HYPER)
    infos = d["f64"][3]
    coefs = [i["clip_coef"] for i in infos]
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs)              # clipping active in some steps, inactive in others
    _check(name, (p, m, v), d["f64"], d["t32"], K, HYPER["lr"])
    assert opt.step_count.dtype == torch.int64 and int(opt.step_count) == K == opt.steps
    for t, (st, info) in enumerate(zip(hist, infos)):
        st = _np(st).astype(np.float64)
        assert abs(st[0] - info["total_norm"]) <= 2.0 ** -22 * info["total_norm"], (t, st[0], info["total_norm"])
        assert abs(st[1] - info["clip_coef"]) <= 2.0 ** -22 * info["clip_coef"]
        assert abs(st[2] - info["lr_t"]) <= np.spacing(np.float32(info["lr_t"])), (t, st[2], info["lr_t"])    # across the restart at t = 4
        assert st[3] == t + 1
    assert infos[3]["lr_t"] == HYPER["lr"] and infos[1]["lr_t"] < HYPER["lr"]
    assert opt.current_lr() == schedule(K, HYPER["lr"], HYPER["t0"], HYPER["eta_min"])


def test_clipping_modes_and_read_only_gradients(data):
    d = data["actor_23_16_4"]
    keep = [[g.copy() for g in s] for s in d["sets"]]

    def run(max_norm, sets=d["sets"]):
        from gym_rotor_amd import DeviceAdamW
        params = [torch.nn.Parameter(_cuda(a)) for a in d["p"]]
        opt = DeviceAdamW(params, **{**HYPER, "max_norm": max_norm})
        grads = [[_cuda(g) for g in s] for s in sets]
        for s in grads:
            for q, g in zip(params, s):
                q.grad = g
            opt.step()
        torch.cuda.synchronize()
        for s, s0 in zip(grads, keep):                                                # the gradient tensors: bit-unchanged
            assert all(np.array_equal(_np(g), g0) for g, g0 in zip(s, s0))
        return params, opt

    p_off, o_off = run(-1.0)
    p_big, o_big = run(7.0)                                                           # above every norm: the coefficient is 1
    assert all(torch.equal(a, b) for a, b in zip(p_off, p_big))
    assert torch.equal(o_off.exp_avg, o_big.exp_avg) and torch.equal(o_off.exp_avg_sq, o_big.exp_avg_sq)
    assert float(o_big.stats[1]) == 1.0 and float(o_off.stats[1]) == 1.0
    p_clip, _ = run(1.0)
    assert not all(torch.equal(a, b) for a, b in zip(p_off, p_clip))
    # max_norm = 0: every gradient is scaled to zero, the parameters change by the weight decay only — float32(p float32(1 - lr wd))
    p_zero, o_zero = run(0.0, d["sets"][:1])
    decay = np.float32(1.0 - HYPER["lr"] * HYPER["weight_decay"])
    for q, p0 in zip(p_zero, d["p"]):
        assert np.array_equal(_np(q), p0 * decay)
    assert not o_zero.exp_avg.any() and not o_zero.exp_avg_sq.any() and float(o_zero.stats[1]) == 0.0 and o_zero.steps == 1


def _guarded(sizes, dtype=torch.float32, gap=16):
    """Slices of the given sizes of ONE buffer of sentinels, `gap` sentinel elements before and after each: (buffer, mask of the
    guard elements, views)."""
    buf = torch.full((sum(sizes) + gap * (len(sizes) + 1),), SENTINEL, dtype=dtype, device="cuda")
    views, mask, o = [], torch.ones_like(buf, dtype=torch.bool), gap
    for s in sizes:
        views.append(buf[o:o + s]); mask[o:o + s] = False; o += s + gap
    return buf, mask, views


@pytest.mark.parametrize("name", ["actor_3_4_1", "critic_23_62", "critic_1_1"])
def test_guarded_buffers(data, name):
    """Parameters, moments, stats and step in guarded buffers, sentinels on both sides of each: nothing outside is written, and the
    results are the bits of DeviceAdamW on ordinary tensors."""
    from gym_rotor_amd import adamw_step
    d = data[name]
    sizes = [a.size for a in d["p"]]
    total = sum(sizes)
    buf, mask, views = _guarded(sizes + [total, total, 4])
    ibuf, imask, (step,) = _guarded([1], torch.int64, gap=2)
    params, (m, v, stats) = views[:len(sizes)], views[len(sizes):]
    for q, a in zip(params, d["p"]):
        q.copy_(_cuda(a).reshape(-1))
    m.zero_(); v.zero_(); stats.zero_(); step.zero_()
    sentinel_i = ibuf[imask].clone()
    for s in d["sets"][:2]:
        adamw_step(params, [_cuda(g).reshape(-1) for g in s], m, v, step, stats, **HYPER)
    torch.cuda.synchronize()
    assert bool((buf[mask] == SENTINEL).all()) and torch.equal(ibuf[imask], sentinel_i) and int(step) == 2
    p2, m2, v2, opt, hist = _device_run(d["p"], d["sets"][:2], HYPER)
    assert all(torch.equal(a, b.reshape(-1)) for a, b in zip(params, p2))
    assert torch.equal(m, opt.exp_avg) and torch.equal(v, opt.exp_avg_sq) and torch.equal(stats, opt.stats)
    # stats = NULL: the same bits, nothing else written
    before = buf.clone()
    for q, a in zip(params, d["p"]):
        q.copy_(_cuda(a).reshape(-1))
    m.zero_(); v.zero_(); step.zero_()
    for s in d["sets"][:2]:
        adamw_step(params, [_cuda(g).reshape(-1) for g in s], m, v, step, None, **HYPER)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def _fresh_opts(data, hyper=HYPER, poison=None):
    from gym_rotor_amd import DeviceAdamW
    opts = []
    for name in GROUPS:
        params = [torch.nn.Parameter(_cuda(a)) for a in data[name]["p"]]
        for q, g in zip(params, data[name]["sets"][1]):
            q.grad = _cuda(g)
        if poison == name:
            params[2].grad.view(-1)[3] = float("nan")
        opts.append(DeviceAdamW(params, **hyper))
    return opts


def _state(o):
    return [q.data for q in o.params] + [o.exp_avg, o.exp_avg_sq, o.stats, o.step_count]


def test_groups_in_one_launch(data):
    from gym_rotor_amd import DeviceAdamW
    one_by_one, together, again = _fresh_opts(data), _fresh_opts(data), _fresh_opts(data)
    for _ in range(2):
        for o in one_by_one:
            o.step()
        DeviceAdamW.step_all(together)
        DeviceAdamW.step_all(again)
    torch.cuda.synchronize()
    for a, b, c in zip(one_by_one, together, again):
        assert a.steps == b.steps == 2
        assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))          # four groups in one launch = four launches
        assert all(torch.equal(x, y) for x, y in zip(_state(b), _state(c)))          # the same launch from the same state: the same bits
    nine = _fresh_opts(data) + _fresh_opts(data) + _fresh_opts(data)[:1]             # more than 8: two launches
    DeviceAdamW.step_all(nine)
    first = _fresh_opts(data)
    DeviceAdamW.step_all(first)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for o, r in zip(nine, first + first + first) for x, y in zip(_state(o), _state(r)))


@pytest.mark.parametrize("edit", [dict(weight_decay=0.0), dict(t0=0), dict(weight_decay=0.0, t0=0, max_norm=-1.0)])
def test_edge_hyperparameters(data, edit):
    hyper = {**HYPER, **edit}
    for name in ("actor_23_16_4", "critic_1_1"):
        d = data[name]
        sets = d["sets"][:3]
        p, m, v, opt, hist = _device_run(d["p"], sets, hyper)
        _check(f"{name} {edit}", (p, m, v), run_f64(d["p"], sets, **hyper), run_torch(d["p"], sets, torch.float32, "cuda", **hyper), 3, hyper["lr"])
        if hyper["t0"] == 0:
            assert all(float(h[2]) == np.float32(hyper["lr"]) for h in hist)
    if hyper["weight_decay"] == 0.0:                                                  # a zero gradient then leaves the parameters as they are
        d = data["actor_3_4_1"]
        zero = [[np.zeros_like(g) for g in d["sets"][0]]]
        p, _, _, _, _ = _device_run(d["p"], zero, hyper)
        assert all(np.array_equal(_np(a), b) for a, b in zip(p, d["p"]))


def test_nan_gradient_stays_in_its_group(data):
    """A NaN in one gradient entry: the norm, the clip coefficient and with them ALL of that group's parameters are NaN, as
    clip_grad_norm_ (error_if_nonfinite=False) + AdamW leave them; the other groups of the launch hold the bits of a clean launch."""
    from gym_rotor_amd import DeviceAdamW
    clean, dirty = _fresh_opts(data), _fresh_opts(data, poison="actor_23_16_4")
    DeviceAdamW.step_all(clean)
    DeviceAdamW.step_all(dirty)
    torch.cuda.synchronize()
    for name, a, b in zip(GROUPS, clean, dirty):
        if name == "actor_23_16_4":
            assert all(torch.isnan(q).all() for q in b.params) and torch.isnan(b.exp_avg).all() and b.steps == 1
            assert torch.isnan(b.stats[0]) and torch.isnan(b.stats[1]) and float(b.stats[3]) == 1.0
        else:
            assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b))), name
    d = data["actor_23_16_4"]
    bad = [[g.copy() for g in d["sets"][1]]]
    bad[0][2].reshape(-1)[3] = np.nan
    pt, _, _, _ = run_torch(d["p"], bad, torch.float32, "cuda", **HYPER)
    assert all(np.isnan(a).all() for a in pt)                                         # torch does the same
    # without clipping only that entry is lost, in torch and here
    hyper = {**HYPER, "max_norm": -1.0}
    p, _, _, _, _ = _device_run(d["p"], bad, hyper)
    pt, _, _, _ = run_torch(d["p"], bad, torch.float32, "cuda", **hyper)
    for a, b in zip(p, pt):
        assert np.array_equal(np.isnan(_np(a)).reshape(-1), np.isnan(b).reshape(-1))
    assert sum(int(torch.isnan(a).sum()) for a in p) == 1


# ----------------------------------------------------------------------------------------------------------------
# with real gradients, PpoUpdater, graph capture
# ----------------------------------------------------------------------------------------------------------------
REF = dict(betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(1e-2), max_norm=100.0, t0=1_000_000, eta_min=1e-5)   # the reference's
T_, N_ = 3, 70


def _env(kind):
    from gym_rotor_amd import QuadVecEnv
    env = QuadVecEnv(kind, N_, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=100, seed=21)
    env.reset("train")
    env.get_norm_error_state()
    return env


def _hand_built(kind, seed=7):
    """A T = 3, N = 70 storage filled by hand, as tests/test_gpu_ppo_critic.py and tests/test_gpu_ppo_actor.py build theirs, with modules
    of the reference's sizes: (env, storage, advantage, actors, critics (DTDE), noise, nominal)."""
    from gym_rotor_amd import RolloutStorage
    from gym_rotor_amd.policy import ACTOR_DIMS
    env = _env(kind)
    st = RolloutStorage(env, T_)
    gen = torch.Generator("cuda").manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=gen)
    for o in st.obs:
        o.copy_(rnd(*o.shape) * 2 - 1)
    st.done.copy_(rnd(T_, N_, st.n_agents) < 0.04); st.truncated.copy_(rnd(T_, N_) < 0.04)
    mask = st.reset_mask()
    for f in st.final_obs:
        f.copy_(rnd(*f.shape) * 2 - 1)
        f[~mask] = float("nan")
    st.act_all.copy_(rnd(*st.act_all.shape) * 1.6 - 0.8)
    st.td_target.copy_(torch.randn(T_, N_, st.n_agents, device="cuda", generator=gen) * 3 + 2)
    adv = torch.randn(T_, N_, st.n_agents, device="cuda", generator=gen)
    actors, critics, noise, nominal = [], [], [], []
    for k, dims in enumerate(ACTOR_DIMS[kind]):
        torch.manual_seed(30 + k)
        m = _Actor(*dims).cuda()
        with torch.no_grad():
            d = torch.distributions.Normal(m(st.obs[k][:-1]), m.log_std.exp())
            st.logprob[k].copy_(d.log_prob(st.act[k]) + (rnd(T_, N_, 1) - 0.5) * 0.8 / dims[2])
        actors.append(m)
        critics.append(_Critic(dims[0], 62).cuda())
        noise.append(torch.randn(dims[0], device="cuda", generator=gen) * 0.05)
        nominal.append(RolloutStorage.nominal_action(env, k))
    return env, st, adv, actors, critics, noise, nominal


CO = dict(clip=0.2, lam_T=0.4, lam_S=0.3, lam_M=0.6, max_action=1.0)


def test_one_step_from_real_gradients():
    """One critic_loss and one actor_loss on the hand-built storage, then one DeviceAdamW.step each against torch's float32 clip + AdamW
    step from the same .grad tensors, at the bar with k = 1."""
    from gym_rotor_amd import DeviceAdamW, actor_loss, critic_loss
    env, st, adv, actors, critics, noise, nominal = _hand_built("coupled")
    idx = torch.randperm(T_ * N_, device="cuda", generator=torch.Generator("cuda").manual_seed(1))[:150]
    actor_loss(actors[0], st, 0, adv, idx, entropy_coef=0.01, noise=noise[0], nominal=nominal[0], **CO)
    critic_loss(critics[0], st, 0, idx, l2_reg=1e-4)
    torch.cuda.synchronize()
    for label, module, lr in (("actor", actors[0], 3e-4), ("critic", critics[0], 2e-4)):
        ps = list(module.parameters())
        assert sum(q.numel() for q in ps) == (728 if label == "actor" else 5457)
        p0, g0 = [_np(q).copy() for q in ps], [_np(q.grad).copy() for q in ps]
        assert all(np.isfinite(g).all() for g in g0) and any(np.abs(g).max() > 0 for g in g0)
        opt = DeviceAdamW(ps, lr=lr, **REF)
        opt.step()
        torch.cuda.synchronize()
        sizes = [q.numel() for q in ps]
        got = ([q.data for q in ps], list(opt.exp_avg.split(sizes)), list(opt.exp_avg_sq.split(sizes)))
        hyper = dict(lr=lr, **REF)
        f64 = run_f64(p0, [g0], **hyper)
        _check(f"real gradients, {label}", got, f64, run_torch(p0, [g0], torch.float32, "cuda", **hyper), 1, lr)
        assert all(np.array_equal(_np(q.grad), g) for q, g in zip(ps, g0))            # .grad keeps the unclipped gradient
        assert abs(float(opt.stats[0]) - f64[3][0]["total_norm"]) <= 2.0 ** -22 * f64[3][0]["total_norm"] and opt.steps == 1


def _opts(actors, critics, lr_c=1e-2):
    from gym_rotor_amd import DeviceAdamW
    return ([DeviceAdamW(m.parameters(), lr=3e-4, **REF) for m in actors], [DeviceAdamW(m.parameters(), lr=lr_c, **REF) for m in critics])


def _full_mse(st, critics):
    from gym_rotor_amd import CriticParams
    out = []
    for k, c in enumerate(critics):
        _, s = st.critic_grad(k, CriticParams.from_module(c, (k,)))
        out.append(float(s[1]))
    return out


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
def test_ppo_updater_against_the_loop_written_out(kind):
    """Batch 128 on T N = 210 rows (minibatches of 128 + 82), K_epochs = 2: parameters and optimiser state bit-equal to the loop written
    out below with actor_loss, critic_loss and DeviceAdamW.step one by one from the same generator seed — the updater itself walks the
    two halves together and steps both networks in one launch, the batch sizes being equal."""
    from gym_rotor_amd import ActorParams, PpoUpdater, RolloutStorage, actor_loss, critic_loss
    env, st, adv, actors, critics, noise, nominal = _hand_built(kind)
    n = len(actors)
    env0 = _env(kind)
    before = RolloutStorage(env0, T_)
    before.collect(env0, [ActorParams.from_module(m) for m in actors])
    logprob0 = before.logprob_all.clone()
    actors_b, critics_b = copy.deepcopy(actors), copy.deepcopy(critics)
    init = [[p.detach().clone() for p in m.parameters()] for m in actors]
    mse0 = _full_mse(st, critics)

    oa, oc = _opts(actors, critics)
    up = PpoUpdater(actors, critics, oa, oc, K_epochs=2, actor_batch_size=128, critic_batch_size=128, entropy_coef=1e-2, entropy_coef_decay=0.99,
                    l2_reg=1e-4, noise=noise, nominal=nominal, **CO)
    a_stats, c_stats = up.update(st, adv, generator=torch.Generator("cuda").manual_seed(5))
    torch.cuda.synchronize()

    ob_a, ob_c = _opts(actors_b, critics_b)
    gen, rows, ec = torch.Generator("cuda").manual_seed(5), T_ * N_, 1e-2 * 0.99
    for k in range(n):
        for _ in range(2):
            perm = torch.randperm(rows, device="cuda", generator=gen)
            for sl in (slice(0, 128), slice(128, 210)):
                actor_loss(actors_b[k], st, k, adv, perm[sl], entropy_coef=ec, noise=noise[k], nominal=nominal[k], **CO)
                ob_a[k].step()
            for sl in (slice(0, 128), slice(128, 210)):
                critic_loss(critics_b[k], st, k, perm[sl], inputs=(k,), l2_reg=1e-4)
                ob_c[k].step()
    torch.cuda.synchronize()
    assert up.entropy_coef == ec
    for k in range(n):
        for m, mb in ((actors[k], actors_b[k]), (critics[k], critics_b[k])):
            assert all(torch.equal(p, q) for p, q in zip(m.parameters(), mb.parameters()))
        for o, ob in ((oa[k], ob_a[k]), (oc[k], ob_c[k])):
            assert o.steps == ob.steps == 4
            assert torch.equal(o.exp_avg, ob.exp_avg) and torch.equal(o.exp_avg_sq, ob.exp_avg_sq)
        assert torch.isfinite(a_stats[k]).all() and torch.isfinite(c_stats[k]).all()
        assert not any(torch.equal(p, q) for p, q in zip(actors[k].parameters(), init[k]))
    mse1 = _full_mse(st, critics)
    print(f"ppo updater {kind}: critic mse on the full storage {mse0} -> {mse1}")
    assert all(b < a for a, b in zip(mse0, mse1))
    # the weights are read in place: the same env, seed and horizon collects other actions and log-probs after the update
    env1 = _env(kind)
    after = RolloutStorage(env1, T_)
    after.collect(env1, [ActorParams.from_module(m) for m in actors])
    torch.cuda.synchronize()
    assert torch.isfinite(after.logprob_all).all() and not torch.equal(after.logprob_all, logprob0)
    # a second update allocates nothing that stays
    gen2 = torch.Generator("cuda").manual_seed(6)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    up.update(st, adv, generator=gen2)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held and all(o.steps == 8 for o in oa + oc)


def test_updater_with_unequal_batch_sizes_steps_separately():
    """actor_batch_size != critic_batch_size: the reference's order, each network stepped after its own minibatch."""
    from gym_rotor_amd import PpoUpdater
    env, st, adv, actors, critics, noise, nominal = _hand_built("coupled")
    oa, oc = _opts(actors, critics)
    up = PpoUpdater(actors, critics, oa, oc, K_epochs=1, actor_batch_size=128, critic_batch_size=64, noise=noise, nominal=nominal, **CO)
    up.update(st, adv, generator=torch.Generator("cuda").manual_seed(5))
    torch.cuda.synchronize()
    assert oa[0].steps == 2 and oc[0].steps == 4
    assert all(torch.isfinite(p).all() for m in actors + critics for p in m.parameters())


def test_graph_capture_of_critic_grad_then_step():
    """The linear chain critic_grad -> DeviceAdamW.step on a fixed minibatch, captured once (grads, stats and workspace allocated
    before): three replays leave the bits of three eager rounds from the same start, and step == 3."""
    from gym_rotor_amd import DeviceAdamW, critic_loss
    env, st, adv, actors, critics, noise, nominal = _hand_built("coupled")
    critic, eager = critics[0], copy.deepcopy(critics[0])
    idx = torch.randperm(T_ * N_, device="cuda", generator=torch.Generator("cuda").manual_seed(2))[:128].contiguous()
    stats, stats_e = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    opt_e = DeviceAdamW(eager.parameters(), lr=1e-3, **REF)
    for _ in range(3):
        critic_loss(eager, st, 0, idx, l2_reg=1e-4, stats=stats_e)
        opt_e.step()
    torch.cuda.synchronize()

    start = [p.detach().clone() for p in critic.parameters()]
    opt = DeviceAdamW(critic.parameters(), lr=1e-3, **REF)
    critic_loss(critic, st, 0, idx, l2_reg=1e-4, stats=stats)             # allocates the .grad tensors (the workspace exists since the eager rounds)
    torch.cuda.synchronize()
    cur, side, graph = torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            critic_loss(critic, st, 0, idx, l2_reg=1e-4, stats=stats)
            opt.step()
    cur.wait_stream(side)
    torch.cuda.synchronize()
    assert opt.steps == 0 and all(torch.equal(p, s) for p, s in zip(critic.parameters(), start))       # capture executes nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert opt.steps == 3 == opt_e.steps
    assert all(torch.equal(p, q) for p, q in zip(critic.parameters(), eager.parameters()))
    assert torch.equal(opt.exp_avg, opt_e.exp_avg) and torch.equal(opt.exp_avg_sq, opt_e.exp_avg_sq)
    assert torch.equal(stats, stats_e) and torch.equal(opt.stats, opt_e.stats)


def test_torch_op_returns_the_bits_of_device_adamw(data):
    d = data["critic_23_62"]
    p, m, v, opt, hist = _device_run(d["p"], d["sets"][:2], HYPER)
    params = [_cuda(a) for a in d["p"]]
    exp_avg, exp_avg_sq = torch.zeros(5457, device="cuda"), torch.zeros(5457, device="cuda")
    step, stats = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((4,), SENTINEL, device="cuda")
    for s in d["sets"][:2]:
        torch.ops.gym_rotor_amd.qr_adamw_step(params, [_cuda(g) for g in s], exp_avg, exp_avg_sq, step, stats, HYPER["lr"], *HYPER["betas"],
                                              HYPER["eps"], HYPER["weight_decay"], HYPER["max_norm"], HYPER["t0"], HYPER["eta_min"])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(params, p)) and torch.equal(exp_avg, opt.exp_avg) and torch.equal(exp_avg_sq, opt.exp_avg_sq)
    assert torch.equal(stats, opt.stats) and int(step) == 2
    with pytest.raises(ValueError, match="step must be an int64"):
        torch.ops.gym_rotor_amd.qr_adamw_step(params, [_cuda(g) for g in d["sets"][0]], exp_avg, exp_avg_sq, step.int(), stats, 1e-3, 0.9, 0.999, 1e-8,
                                              1e-2, -1.0, 0, 0.0)
