"""Td3Updater and SacUpdater on the GPU: `update` against the same loop written out from public calls in the reference's order (soft
updates last, as td3.py:207-211 / sac.py:219-221 place them) bit for bit in all three modes; one iteration against the float64
restatement of tests/offpolicy_ref.py under the bar of tests/test_gpu_optim.py with a grad_max_norm between the Q-networks' own
gradient norms and their joint norm; steady-state allocation; graph capture against eager twins."""
import copy

import numpy as np
import pytest
import torch

import offpolicy_ref as R
from test_gpu_optim import _check, _np
from test_sac_critic_host import _SacActor
from test_td3_critic_host import _Actor, _Twin

pytestmark = pytest.mark.gpu
CAP, B, FREQ, H = 512, 130, 2, 62                                    # B: two 64-row tiles and a partial one
DIMS = {"single": ([23], [4]), "dtde": ([15, 3], [4, 1]), "ctde": ([15, 3], [4, 1])}
ACTOR_DIMS = {"single": [(23, 16, 4)], "dtde": [(15, 16, 4), (3, 4, 1)], "ctde": [(15, 16, 4), (3, 4, 1)]}


def _buffer(mode, seed=0):
    from gym_rotor_amd import ReplayBuffer
    od, ad = DIMS[mode]
    buf = ReplayBuffer(CAP, od, ad, "cuda", seed=77)
    g = torch.Generator(device="cuda").manual_seed(seed)
    for k in range(len(od)):
        buf.obs[k].copy_(torch.randn(CAP, od[k], device="cuda", generator=g) * 0.5)
        buf.obs_next[k].copy_(buf.obs[k] + torch.randn(CAP, od[k], device="cuda", generator=g) * 0.05)
        buf.act[k].copy_(torch.rand(CAP, ad[k], device="cuda", generator=g) * 2 - 1)
        buf.rwd[k].copy_(torch.rand(CAP, device="cuda", generator=g))
        buf.done[k].copy_((torch.rand(CAP, device="cuda", generator=g) < 0.1).float())
    buf.count, buf.current_size = 0, CAP
    return buf


def _modules(algo, mode, seed=1):
    torch.manual_seed(seed)
    od, ad = DIMS[mode]
    make = _Actor if algo == "td3" else _SacActor
    actors = [make(*d).cuda() for d in ACTOR_DIMS[mode]]
    din = [sum(od) + sum(ad)] * 2 if mode == "ctde" else [o + a for o, a in zip(od, ad)]
    critics = [_Twin(d, H).cuda() for d in din]
    nominal = [torch.tensor([0.1, 0.0, 0.0, 0.0], device="cuda")[:a].contiguous() for a in ad]
    return actors, critics, copy.deepcopy(actors), copy.deepcopy(critics), nominal


def _updater(algo, mode, mods, **kw):
    from gym_rotor_amd import SacUpdater, Td3Updater
    actors, critics, actors_t, critics_t, nominal = mods
    kw = dict(mode=mode, policy_update_freq=FREQ, batch_size=B, nominal=nominal, **kw)
    if algo == "td3":
        return Td3Updater(actors, critics, actors_t, critics_t, **kw)
    return SacUpdater(actors, critics, critics_t, automatic_entropy_tuning=True, **kw)


def _tensors(up):
    """Every tensor an update writes: live and target networks, optimiser states, stats, alpha."""
    out = []
    for m in up.actors + up.critics + up.critic_targets + list(getattr(up, "actor_targets", [])):
        out += [q.data for q in m.parameters()]
    for o in up.critic_opts + up.actor_opts + [a for a in getattr(up, "alpha_opts", []) if a is not None]:
        out += [o.exp_avg, o.exp_avg_sq, o.step_count, o.stats]
    out += up.critic_stats + up.actor_stats
    if hasattr(up, "alpha_opts"):
        out += [x.data for x in up.log_alpha] + list(up.alpha)
    return out


def _written_out(algo, mode, mods, buf, iterations, gen, layout):
    """The loop of TD3.train / SAC.train from public calls, in the reference's order: losses, optimiser steps WITHOUT the fused soft
    update, then `soft_update` where the reference has its copy_ lines.  layout: per agent the names and shapes of the draws."""
    import gym_rotor_amd as G
    actors, critics, actors_t, critics_t, nominal = mods
    n = len(actors)
    hyper = dict(max_norm=100.0, t0=1_000_000, eta_min=1e-5)
    names = ("fc1", "fc2", "fc3") if algo == "td3" else ("fc1", "fc2", "mean_linear", "log_std_linear")
    plist = lambda m, ns: [t for l in ns for t in (getattr(m, l).weight, getattr(m, l).bias)]
    six = ("fc1", "fc2", "fc3", "fc4", "fc5", "fc6")
    copt = [G.PolyakAdamW(plist(critics[k], six), lr=2e-4, **hyper) for k in range(n)]
    aopt = [G.PolyakAdamW(plist(actors[k], names), lr=3e-4, **hyper) for k in range(n)]
    cstats, astats = [torch.zeros(4, device="cuda") for _ in range(n)], [torch.zeros(4 if algo == "td3" else 6, device="cuda") for _ in range(n)]
    idx = [torch.zeros(B, dtype=torch.int64, device="cuda") for _ in range(n)]
    noise = [{name: (tuple(torch.zeros_like(x) for x in t) if isinstance(t, tuple) else torch.zeros_like(t)) for name, t in layout[k].items()}
             for k in range(n)]
    if algo == "sac":
        log_alpha = [torch.zeros(1, device="cuda", requires_grad=True) for _ in range(n)]
        alpha = [torch.full((1,), 0.05, device="cuda") for _ in range(n)]
        lopt = [G.PolyakAdamW([log_alpha[k]], exp_out=alpha[k], lr=3e-4) for k in range(n)]   # (exp_out's own value: test_one_iteration_against_float64)
    for it in range(1, iterations + 1):
        for k in range(n):
            buf.sample_index(B, out=idx[k])
            for name, t in noise[k].items():
                for x in (t if isinstance(t, tuple) else (t,)):
                    x.normal_(0.0, 0.05 if name == "reg" else 1.0, generator=gen)
            nz = noise[k]
            reg = dict(lam_T=0.4, lam_S=0.3, lam_M=0.6, max_action=1.0, noise=nz["reg"], nominal=nominal[k], stats=astats[k])
            if algo == "td3":
                kw = dict(discount=0.99, target_noise=0.2, noise_clip=0.5, max_action=1.0, noise=nz["smooth"], stats=cstats[k])
                if mode == "ctde":
                    G.td3_critic_loss_ctde(critics[k], critics_t[k], actors_t, buf, k, idx[k], **kw)
                else:
                    G.td3_critic_loss(critics[k], critics_t[k], actors_t[k], buf, k, idx[k], **kw)
                copt[k].step()
                if it % FREQ == 0:
                    if mode == "ctde":
                        G.td3_actor_loss_ctde(actors, critics[k], buf, k, idx[k], **reg)
                    else:
                        G.td3_actor_loss(actors[k], critics[k], buf, k, idx[k], **reg)
                    aopt[k].step()
                    G.soft_update(critics[k], critics_t[k], 0.005)
                    G.soft_update(actors[k], actors_t[k], 0.005)
            else:
                kw = dict(discount=0.99, alpha=alpha[k], noise=nz["next"], stats=cstats[k])
                eps = dict(log_alpha=log_alpha[k], alpha=alpha[k], eps=nz["eps"], eps_reg=nz["eps_reg"], eps_next=nz["eps_next"], eps_pert=nz["eps_pert"])
                if mode == "ctde":
                    G.sac_critic_loss_ctde(critics[k], critics_t[k], actors, buf, k, idx[k], noise_logp=nz["noise_logp"], **kw)
                else:
                    G.sac_critic_loss(critics[k], critics_t[k], actors[k], buf, k, idx[k], **kw)
                copt[k].step()
                if mode == "ctde":
                    G.sac_actor_loss_ctde(actors, critics[k], buf, k, idx[k], eps_logp=nz["eps_logp"], eps_other=nz["eps_other"], **eps, **reg)
                else:
                    G.sac_actor_loss(actors[k], critics[k], buf, k, idx[k], **eps, **reg)
                aopt[k].step()
                lopt[k].step()
                if it % FREQ == 0:
                    G.soft_update(critics[k], critics_t[k], 0.005)
    out = []
    for m in actors + critics + critics_t + (actors_t if algo == "td3" else []):
        out += [q.data for q in m.parameters()]
    for o in copt + aopt + (lopt if algo == "sac" else []):
        out += [o.exp_avg, o.exp_avg_sq, o.step_count, o.stats]
    out += cstats + astats
    if algo == "sac":
        out += [x.data for x in log_alpha] + alpha
    return out


@pytest.mark.parametrize("mode", ["single", "dtde", "ctde"])
@pytest.mark.parametrize("algo", ["td3", "sac"])
def test_update_against_the_loop_written_out(algo, mode):
    mods = _modules(algo, mode)
    twin = copy.deepcopy(mods)
    initial = [q.data.clone() for m in mods[3] for q in m.parameters()]
    up = _updater(algo, mode, mods, generator=torch.Generator(device="cuda").manual_seed(5))
    critic_stats, actor_stats = up.update(_buffer(mode), 2 * FREQ)
    want = _written_out(algo, mode, twin, _buffer(mode), 2 * FREQ, torch.Generator(device="cuda").manual_seed(5), up.noise)
    torch.cuda.synchronize()
    got = _tensors(up)
    assert len(got) == len(want) and up.total_it == 2 * FREQ
    for j, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), j
    assert critic_stats is up.critic_stats and actor_stats is up.actor_stats and all(bool(torch.isfinite(s).all()) for s in critic_stats + actor_stats)
    assert all(int(o.step_count) == 2 * FREQ for o in up.critic_opts)
    assert all(int(o.step_count) == (2 if algo == "td3" else 2 * FREQ) for o in up.actor_opts)
    assert all(not torch.equal(q.data, q0) for q, q0 in zip((q for m in up.critic_targets for q in m.parameters()), initial))


HP = dict(discount=0.99, tau=0.005, target_noise=0.2, noise_clip=0.5, lam_T=0.4, lam_S=0.3, lam_M=0.6, max_action=1.0, lr_a=3e-4, lr_c=2e-4)


def _arrays(m, names):
    return [_np(t).astype(np.float64) for l in names for t in (getattr(m, l).weight, getattr(m, l).bias)]


SIX = ("fc1", "fc2", "fc3", "fc4", "fc5", "fc6")


def _bar_check(label, opt, want, want32, lr):
    """The PARAMETERS under `_check`'s bar.  The moments are not held to it here: after a whole iteration they carry the loss kernels'
    own float32 gradient error (m = (1 - beta1) clip g), which that bar — made for exact gradient inputs — has no term for; they are
    held to it where the gradients are inputs (tests/test_gpu_adamw_polyak.py)."""
    _check(label, ([q.data for q in opt.params],), want[:1], want32[:1], 1, lr)


def _target_check(label, modules_t, names, want, want32_p, want_p, lr):
    """The bar of `_check` for the parameters scaled by tau — the target's share of the parameter's error — plus the soft-update line's own
    four half-ulps (float32(1 - tau), two products, one sum), which test_gpu_adamw_polyak.py pins bit for bit."""
    for j, (t, w, p32, p64) in enumerate(zip((x for l in names for x in (getattr(modules_t, l).weight, getattr(modules_t, l).bias)), want, want32_p, want_p)):
        e32 = float(np.abs(p32.reshape(p64.shape) - p64).max())
        bar_p = max(e32, 2.0 ** -24 * (4 * float(np.abs(p64).max()) + 16 * lr))
        err = float(np.abs(_np(t).astype(np.float64) - w).max())
        bar = HP["tau"] * bar_p + 4 * 2.0 ** -24 * float(np.abs(w).max())
        print(f"{label} target[{j}]: err {err:.3e}, bar {bar:.3e} (tau * {bar_p:.3e} + the line's rounding)")
        assert err <= bar, (label, j, err, bar)


@pytest.mark.parametrize("algo", ["td3", "sac"])
def test_one_iteration_against_float64(algo):
    """An update iteration in single mode against the float64 restatement on the updater's own minibatch and draws, with
    grad_max_norm between the Q-networks' own gradient norms and the joint norm: the clip is active only because it is joint."""
    mods = _modules(algo, "single", seed=4)
    names = ("fc1", "fc2", "fc3") if algo == "td3" else ("fc1", "fc2", "mean_linear", "log_std_linear")
    start = dict(actor=_arrays(mods[0][0], names), critic=_arrays(mods[1][0], SIX), actor_t=_arrays(mods[2][0], names), critic_t=_arrays(mods[3][0], SIX))
    nominal = _np(mods[4][0]).astype(np.float64)
    # a first pass of the restatement for the gradient norms (they do not depend on grad_max_norm in the first iteration)
    probe = _updater(algo, "single", copy.deepcopy(mods), generator=torch.Generator(device="cuda").manual_seed(9))
    probe.policy_update_freq = 1
    buf = _buffer("single")
    probe.update(buf, 1)
    idx = probe.index[0].cpu().numpy()
    batch = {k: _np(v)[idx].astype(np.float64) for k, v in buf.tensors(0).items()}
    noise = {k: _np(v).astype(np.float64) for k, v in probe.noise[0].items()}

    def restate(dtype, gmn):
        hp = dict(HP, grad_max_norm=gmn)
        if algo == "td3":
            return R.td3_iteration(dtype, start["actor"], start["critic"], start["actor_t"], start["critic_t"], batch, noise, nominal, hp)
        return R.sac_iteration(dtype, start["actor"], start["critic"], start["critic_t"], batch, noise, nominal, hp, 0.05, 0.0)

    first = restate(torch.float64, 100.0)
    h1, h2, joint = first["half_norms"][0], first["half_norms"][1], first["joint_norm"]
    gmn = float(np.float32(0.5 * (max(h1, h2) + joint)))
    assert max(h1, h2) < gmn < joint, (h1, h2, gmn, joint)            # each Q-network alone would not be clipped; together they are
    up = _updater(algo, "single", mods, generator=torch.Generator(device="cuda").manual_seed(9), grad_max_norm=gmn)
    up.policy_update_freq = 1
    up.update(_buffer("single"), 1)
    torch.cuda.synchronize()
    assert torch.equal(up.index[0], probe.index[0]) and all(torch.equal(a, b) for a, b in zip(up.noise[0].values(), probe.noise[0].values()))
    w64, w32 = restate(torch.float64, gmn), restate(torch.float32, gmn)
    assert float(up.critic_opts[0].stats[1]) < 1.0 and abs(float(up.critic_opts[0].stats[0]) - joint) <= 1e-4 * joint
    _bar_check(f"{algo} critic", up.critic_opts[0], (w64["critic"],) + w64["critic_m"], (w32["critic"],) + w32["critic_m"], HP["lr_c"])
    _bar_check(f"{algo} actor", up.actor_opts[0], (w64["actor"],) + w64["actor_m"], (w32["actor"],) + w32["actor_m"], HP["lr_a"])
    _target_check(f"{algo} critic", up.critic_targets[0], SIX, w64["critic_t"], w32["critic"], w64["critic"], HP["lr_c"])
    if algo == "td3":
        _target_check("td3 actor", up.actor_targets[0], names, w64["actor_t"], w32["actor"], w64["actor"], HP["lr_a"])
    else:
        la = np.float64(float(up.log_alpha[0].detach()))
        rounding = 2.0 ** -24 * (4 * abs(w64["log_alpha"]) + 16 * HP["lr_a"])
        assert abs(la - w64["log_alpha"]) <= max(abs(w32["log_alpha"] - w64["log_alpha"]), rounding)
        assert abs(np.float64(float(up.alpha[0])) - np.exp(la)) <= np.spacing(np.float32(np.exp(la)))


@pytest.mark.parametrize("algo", ["td3", "sac"])
def test_steady_state_allocates_nothing_and_targets_move_on_update_iterations(algo):
    mods = _modules(algo, "dtde")
    before = [[q.data.clone() for q in m.parameters()] for m in mods[3]]
    up, buf = _updater(algo, "dtde", mods), _buffer("dtde")
    mem, same = [], []
    for _ in range(2 * FREQ):
        up.update(buf, 1)
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
        same.append(all(torch.equal(a, b.data) for m0, m in zip(before, up.critic_targets) for a, b in zip(m0, m.parameters())))
    assert mem[1] == mem[2] == mem[3], mem                            # (iteration 2 is TD3's first actor half: its workspace and .grad)
    assert same == [True, False, False, False]                        # iteration 1 is no update iteration, iteration 2 is


def _capture_pair(algo, refill):
    ups, bufs = [], []
    for _ in range(2):
        up, buf = _updater(algo, "single", _modules(algo, "single"), refill_noise=refill), _buffer("single")
        buf.use_device_state()
        up.update(buf, FREQ)                                          # the eager call capture asks for; both twins take it
        g = torch.Generator(device="cuda").manual_seed(31)
        if not refill:
            for t in up.noise[0].values():
                t.normal_(generator=g)
        ups.append(up); bufs.append(buf)
    return ups, bufs


@pytest.mark.parametrize("algo", ["td3", "sac"])
def test_capture_replays_equal_eager_iterations(algo):
    (a, b), (buf_a, buf_b) = _capture_pair(algo, refill=False)
    replay = a.capture(buf_a)
    assert a.total_it == FREQ and (buf_a.count, buf_a.current_size, buf_a.draw) == (buf_b.count, buf_b.current_size, buf_b.draw)
    replay(); replay()
    b.update(buf_b, 2 * FREQ)
    torch.cuda.synchronize()
    for j, (x, y) in enumerate(zip(_tensors(a), _tensors(b))):
        assert torch.equal(x, y), j
    assert a.total_it == b.total_it == 3 * FREQ
    buf_a.pull_device_state()
    assert (buf_a.count, buf_a.current_size, buf_a.draw) == (buf_b.count, buf_b.current_size, buf_b.draw) and buf_b.draw == 3 * FREQ
    assert torch.equal(a.index[0], b.index[0])


def test_capture_with_noise_refill_draws_afresh():
    (a, _), (buf_a, _) = _capture_pair("sac", refill=True)
    replay = a.capture(buf_a)
    replay()
    first = {k: v.clone() for k, v in a.noise[0].items()}
    idx = a.index[0].clone()
    replay()
    torch.cuda.synchronize()
    assert all(not torch.equal(first[k], v) for k, v in a.noise[0].items()) and not torch.equal(idx, a.index[0])
    assert all(bool(torch.isfinite(t).all()) for t in _tensors(a) if t.is_floating_point())
