"""The replayable PPO update on the GPU: qr_ppo_actor_grad_dev against the by-value entry, `PpoUpdater` with the device sources against
the loop written out by hand with `shuffle`, `noise_fill`, `actor_loss(entropy_coef_dev=)`, `critic_loss` and `DeviceAdamW`, and
`capture` against eager updates — all bit for bit, on §8.7's shapes (2 epochs x 210 rows in minibatches of 128 + 82)."""
import copy
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_optim import CO, REF, T_, N_, _hand_built, _opts  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SEED = 2 ** 40 + 17
ROWS, SLICES = T_ * N_, (slice(0, 128), slice(128, 210))
KW = dict(K_epochs=2, actor_batch_size=128, critic_batch_size=128, entropy_coef=1e-2, entropy_coef_decay=0.99, l2_reg=1e-4, **CO)


# ---------------------------------------------------------------- the entry
@pytest.mark.parametrize("kind,k,dims", [("coupled", 0, (23, 16, 4)), ("decoupled", 0, (15, 16, 4)), ("decoupled", 1, (3, 4, 1))])
def test_dev_entry_gives_the_bits_of_the_value_entry(kind, k, dims):
    from gym_rotor_amd import ActorParams
    from gym_rotor_amd import _lib as L
    env, st, adv, actors, critics, noise, nominal = _hand_built(kind)
    actor = ActorParams.from_module(actors[k])
    assert actor.dims == dims
    idx = torch.randperm(ROWS, device="cuda", generator=torch.Generator("cuda").manual_seed(3))[:150].contiguous()
    kw = dict(noise=noise[k], nominal=nominal[k], **CO)
    words = torch.tensor([-7.25, 0.0, -7.25], device="cuda")
    grads = {n: torch.zeros_like(g) for n, g in st.actor_grad(k, actor, adv, idx, entropy_coef=0.0, **kw)[0].items()}
    stats = torch.zeros(4, device="cuda")
    for c in (1e-2, 0.37, 0.0):                      # the word is overwritten between the launches: each launch follows it
        want_g, want_s = st.actor_grad(k, actor, adv, idx, entropy_coef=c, **kw)
        words[1] = c
        st.actor_grad(k, actor, adv, idx, entropy_coef=123.0, entropy_coef_dev=words[1:2], grads=grads, stats=stats, **kw)   # the value is ignored
        torch.cuda.synchronize()
        assert set(grads) == set(L.PPO_GRAD_NAMES) and all(torch.equal(grads[n], want_g[n]) for n in grads), c
        assert torch.equal(stats, want_s) and torch.isfinite(stats).all()
        assert words.tolist() == [-7.25, C.c_float(c).value, -7.25]      # read only, and its neighbours untouched
    zero_g, _ = st.actor_grad(k, actor, adv, idx, entropy_coef=0.37, **kw)
    assert not torch.equal(zero_g["log_std"], grads["log_std"])          # the coefficient does reach the gradient
    # the torch op twin
    ga = [torch.zeros_like(grads[n]) for n in L.PPO_GRAD_NAMES]
    words[1] = 0.37
    m = actors[k]
    torch.ops.gym_rotor_amd.qr_ppo_actor_grad_dev([m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.mean_linear.weight, m.mean_linear.bias,
                                                   m.log_std], st.obs[k], st.final_obs[k], st.done, st.truncated, st.act_all, st.logprob_all,
                                                  adv[..., k], idx, noise[k], nominal[k], ga, stats, words[1:2], sum(st.action_dims[:k]), CO["clip"],
                                                  CO["lam_T"], CO["lam_S"], CO["lam_M"], CO["max_action"])
    torch.cuda.synchronize()
    assert all(torch.equal(a, zero_g[n]) for a, n in zip(ga, L.PPO_GRAD_NAMES))


# ---------------------------------------------------------------- the updater
def _same(mods_a, mods_b, opts_a, opts_b):
    for m, mb in zip(mods_a, mods_b):
        assert all(torch.equal(p, q) for p, q in zip(m.parameters(), mb.parameters()))
    for o, ob in zip(opts_a, opts_b):
        assert torch.equal(o.step_count, ob.step_count) and torch.equal(o.exp_avg, ob.exp_avg) and torch.equal(o.exp_avg_sq, ob.exp_avg_sq)


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
def test_device_sources_against_the_loop_written_out(kind):
    from gym_rotor_amd import PpoUpdater, actor_loss, critic_loss, noise_fill, ppo_stream, shuffle
    env, st, adv, actors, critics, _, nominal = _hand_built(kind)
    n = len(actors)
    actors_b, critics_b = copy.deepcopy(actors), copy.deepcopy(critics)
    init = [[p.detach().clone() for p in m.parameters()] for m in actors]
    oa, oc = _opts(actors, critics)
    up = PpoUpdater(actors, critics, oa, oc, nominal=nominal, shuffle_source="device", noise_source="device", seed=SEED, **KW)
    up.update(st, adv)
    torch.cuda.synchronize()

    ob_a, ob_c = _opts(actors_b, critics_b)
    word = torch.tensor([1e-2 * 0.99], dtype=torch.float32, device="cuda")
    perm = torch.zeros(ROWS, dtype=torch.int64, device="cuda")
    e = m = 0
    for k in range(n):
        nz = torch.zeros(actors_b[k].fc1.weight.shape[1], device="cuda")
        for _ in range(2):
            shuffle(perm, n=ROWS, seed=SEED, draw=e, stream=ppo_stream(k, "shuffle"))
            e += 1
            for sl in SLICES:
                noise_fill([nz], seed=SEED, draw=m, streams=[ppo_stream(k, "noise")], kind="normal", a=0.0, b=0.05)
                m += 1
                actor_loss(actors_b[k], st, k, adv, perm[sl], entropy_coef_dev=word, noise=nz, nominal=nominal[k], **CO)
                critic_loss(critics_b[k], st, k, perm[sl], inputs=(k,), l2_reg=1e-4)
                ob_a[k].step()
                ob_c[k].step()
        assert torch.equal(up.noise[k], nz) and (k + 1 < n or torch.equal(up._perm, perm))     # the agent's last row; the last permutation
    torch.cuda.synchronize()
    _same(actors + critics, actors_b + critics_b, oa + oc, ob_a + ob_c)
    assert all(o.steps == 4 for o in oa + oc) and (e, m) == (2 * n, 4 * n)
    assert up.state.tolist() == [e, m] == [up.epoch_draw, up.minibatch_draw] and torch.equal(up.entropy_dev, word)
    assert up.entropy_coef == 1e-2 * 0.99
    assert torch.equal(perm.sort().values, torch.arange(ROWS, device="cuda"))
    assert not any(torch.equal(p, q) for k in range(n) for p, q in zip(actors[k].parameters(), init[k]))
    # a second update allocates nothing, the permutation included
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    up.update(st, adv)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held and all(o.steps == 8 for o in oa + oc) and up.state.tolist() == [4 * n, 8 * n]


def _build(kind):
    from gym_rotor_amd import PpoUpdater
    env, st, adv, actors, critics, _, nominal = _hand_built(kind)
    oa, oc = _opts(actors, critics)
    up = PpoUpdater(actors, critics, oa, oc, nominal=nominal, shuffle_source="device", noise_source="device", seed=SEED, **KW)
    return env, st, adv, actors, critics, oa, oc, up, nominal


def _collect(env, st, adv, actors):
    """A fresh horizon into the same storage, and another advantage in the same tensor: what the next update trains on."""
    from gym_rotor_amd import ActorParams
    st.collect(env, [ActorParams.from_module(m) for m in actors])
    adv.neg_()


@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
def test_captured_updates_against_eager_updates(kind):
    from gym_rotor_amd import PpoUpdater
    n = 1 if kind == "coupled" else 2
    # eager: three updates, a fresh horizon before the third
    env_a, st_a, adv_a, actors_a, critics_a, oa_a, oc_a, up_a, nominal = _build(kind)
    up_a.update(st_a, adv_a)
    up_a.update(st_a, adv_a)
    _collect(env_a, st_a, adv_a, actors_a)
    torch.cuda.synchronize()
    saved = dict(mods=copy.deepcopy(actors_a + critics_a), opts=[o.state_dict() for o in oa_a + oc_a], up=up_a.state_dict())
    up_a.update(st_a, adv_a)
    torch.cuda.synchronize()
    # captured: the first update eager (it makes what the graphs record), then two through the callable
    env_b, st_b, adv_b, actors_b, critics_b, oa_b, oc_b, up_b, _ = _build(kind)
    up_b.update(st_b, adv_b)
    torch.cuda.synchronize()
    before = [p.detach().clone() for m in actors_b + critics_b for p in m.parameters()]
    replay = up_b.capture(st_b, adv_b)
    torch.cuda.synchronize()
    assert len(replay.graphs) == n and up_b.state.tolist() == [2 * n, 4 * n] == [up_b.epoch_draw, up_b.minibatch_draw]      # capturing ran nothing
    assert all(torch.equal(p, q) for p, q in zip(before, (p for m in actors_b + critics_b for p in m.parameters())))
    assert all(o.steps == 4 for o in oa_b + oc_b) and up_b.entropy_coef == 1e-2 * 0.99
    a_stats, c_stats = replay()
    _collect(env_b, st_b, adv_b, actors_b)
    replay()
    torch.cuda.synchronize()
    _same(actors_a + critics_a, actors_b + critics_b, oa_a + oc_a, oa_b + oc_b)
    assert all(o.steps == 12 for o in oa_b + oc_b)
    assert up_b.state.tolist() == up_a.state.tolist() == [6 * n, 12 * n] == [up_b.epoch_draw, up_b.minibatch_draw]
    assert torch.equal(up_b.entropy_dev, up_a.entropy_dev) and up_b.entropy_coef == up_a.entropy_coef == 1e-2 * 0.99 ** 3
    assert torch.equal(st_a.logprob_all, st_b.logprob_all) and not torch.equal(before[0], next(actors_b[0].parameters()))
    for k in range(n):
        assert a_stats[k] is up_b.actor_stats[k] and torch.equal(a_stats[k], up_a.actor_stats[k]) and torch.equal(c_stats[k], up_a.critic_stats[k])
    # a resumed updater reproduces the third update from the saved state
    mods_c = saved["mods"]
    actors_c, critics_c = mods_c[:n], mods_c[n:]
    oa_c, oc_c = _opts(actors_c, critics_c)
    for o, sd in zip(oa_c + oc_c, saved["opts"]):
        o.load_state_dict(sd)
    up_c = PpoUpdater(actors_c, critics_c, oa_c, oc_c, nominal=nominal, shuffle_source="device", noise_source="device", **KW)
    up_c.load_state_dict(saved["up"])
    up_c.update(st_a, adv_a)
    torch.cuda.synchronize()
    _same(actors_a + critics_a, actors_c + critics_c, oa_a + oc_a, oa_c + oc_c)
    assert up_c.state.tolist() == up_a.state.tolist() and torch.equal(up_c.entropy_dev, up_a.entropy_dev)
    # a rebound .grad is refused before anything runs
    p = next(actors_b[0].parameters())
    p.grad = p.grad.clone()
    with pytest.raises(ValueError, match="rebound"):
        replay()
    assert up_b.entropy_coef == up_a.entropy_coef and up_b.state.tolist() == [6 * n, 12 * n]
