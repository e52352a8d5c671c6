"""qr_gae_rule on the device (rollout.gae_rule, RolloutStorage.compute_gae(time_limit=, normalized=, done_eff=), ppo.PpoCollector, the
torch op): the effective done flag against `stored_done` of tests/replay_rule_ref.py bit for bit, the advantages against qr_gae run on
that flag bit for bit and against the float64 restatement of tests/gae_rule_ref.py within the bar of test_rollout_gae.py
(2e-6 * max(1, max |a_ref|)), the float64 sums within (n - 1) * 2^-53 * sum |x| of sums of the kernel's own advantages, the normalised
advantages within one float32 ulp of RolloutStorage.normalize on the same advantages and stats."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gae_rule_ref as G  # noqa: E402
import replay_rule_ref as RR  # noqa: E402
from test_critic_host import _Critic  # noqa: E402
from test_gae_rule_host import GAMMA, LAM, RULE, numpy_of, real_storage, values_for  # noqa: E402
from test_replay_host import COUPLED, DECOUPLED, fake_storage  # noqa: E402
from test_replay_rule_host import rule_storage  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 77, 64   # guard elements around every output and the workspace
T, N = 3, 65               # 65 envs: two workgroups with one agent, three with two; the last one partial


def _guarded(shape, dtype):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return whole[GUARD:GUARD + n].view(shape), whole


def _intact(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


def _bits(x):
    x = x.detach().cpu().contiguous().numpy()
    return x.view(np.uint8) if x.dtype != np.bool_ else x.astype(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def old_gae(reward, done, value, next_value, gamma=GAMMA, lam=LAM):
    """qr_gae, the existing entry, on the given done flags: (advantage, td_target)."""
    from gym_rotor_amd import _lib
    t, n, na = reward.shape
    adv, tgt = torch.empty_like(reward), torch.empty_like(reward)
    done = done.contiguous()
    rc = _lib.load().qr_gae(reward.data_ptr(), done.data_ptr(), value.data_ptr(), None if next_value is None else next_value.data_ptr(), t, n * na,
                            gamma, lam, adv.data_ptr(), tgt.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return adv, tgt


def run(s, value, next_value=None, rule=RULE, outputs=("done_eff", "stats", "normalized"), gamma=GAMMA, lam=LAM):
    """One gae_rule call over guarded outputs on the rows of a fake storage (on the GPU).  Returns the output tensors by name."""
    from gym_rotor_amd import gae_rule, gae_rule_workspace_numel
    t, n, na = s.reward.shape
    shapes = {"advantage": ((t, n, na), torch.float32), "td_target": ((t, n, na), torch.float32), "done_eff": ((t, n, na), torch.uint8),
              "stats": ((na, 3), torch.float64), "normalized": ((t, n, na), torch.float32),
              "workspace": ((gae_rule_workspace_numel(n, na),), torch.float64)}
    names = ("advantage", "td_target") + tuple(outputs) + (("workspace",) if "stats" in outputs else ())
    bufs = {k: _guarded(*shapes[k]) for k in names}
    kw = {k: v[0] for k, v in bufs.items()}
    term = None if rule is None else (s.final_obs if s.final_obs is not None else [o[1:] for o in s.obs])
    out = gae_rule(s.reward, s.done, value, kw.pop("advantage"), kw.pop("td_target"), gamma=gamma, lam=lam, next_value=next_value,
                   truncated=None if rule is None else s.truncated, term_obs=term, rule=rule, **kw)
    torch.cuda.synchronize()
    assert out[0].data_ptr() == bufs["advantage"][0].data_ptr()
    for name, (view, whole) in bufs.items():
        assert _intact(whole, view.numel()), name
    res = {k: v[0] for k, v in bufs.items()}
    if "done_eff" in res:   # (guarded as bytes, where a sentinel shows; the bytes are 0 and 1)
        assert int(res["done_eff"].max()) <= 1
        res["done_eff"] = res["done_eff"].bool()
    return res


def check(s, value, next_value, got, rule=RULE, what=""):
    """Every property of one call's outputs; returns the restatement's outputs."""
    from gym_rotor_amd import RolloutStorage
    ref = G.run(*numpy_of(s), value.cpu().numpy(), None if next_value is None else next_value.cpu().numpy(), GAMMA, LAM, rule=rule)
    if "done_eff" in got:
        assert np.array_equal(got["done_eff"].cpu().numpy(), ref["done_eff"]), what
    eff = torch.from_numpy(ref["done_eff"]).cuda()
    adv, tgt = old_gae(s.reward, eff, value, next_value)
    assert same_bits(got["advantage"], adv) and same_bits(got["td_target"], tgt), what
    scale = max(1.0, np.abs(ref["advantage"]).max())
    a = got["advantage"].cpu().numpy().astype(np.float64)
    err_a, err_t = np.abs(a - ref["advantage"]).max(), np.abs(got["td_target"].cpu().numpy() - ref["td_target"]).max()
    print(f"{what}: max |adv - ref| = {err_a:.3e}, max |td_target - ref| = {err_t:.3e}, bar {2e-6 * scale:.3e}")
    assert err_a <= 2e-6 * scale and err_t <= 2e-6 * scale, what
    if "stats" in got:
        st = got["stats"].cpu().numpy()
        t, n, na = a.shape
        for k in range(na):
            x = a[..., k].ravel()
            assert st[k, 2] == t * n, what
            assert abs(st[k, 0] - x.sum()) <= G.sum_bound(x) and abs(st[k, 1] - (x * x).sum()) <= G.sum_bound(x * x), (what, k)
    if "normalized" in got:
        want = RolloutStorage.normalize(got["advantage"], got["stats"]).cpu().numpy()
        have = got["normalized"].cpu().numpy()
        ulp = np.spacing(np.maximum(np.abs(want), np.abs(have)).astype(np.float32))
        assert (np.abs(have.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), what
        assert np.abs(have - ref["normalized"]).max() <= 2e-5, what      # (test_rollout_gae.py's bar for the normalised values)
    return ref


def _values(s, seed):
    value, next_value = values_for(s, seed)
    return torch.from_numpy(value).cuda(), torch.from_numpy(next_value).cuda()


@pytest.mark.parametrize("dims,final", [(COUPLED, True), (DECOUPLED, True), (DECOUPLED, False), (COUPLED, False)])
def test_planted_rows(dims, final):
    s = rule_storage(dims, device="cuda", final_obs=final, seed=11)
    value, next_value = _values(s, 11)
    got = run(s, value, next_value)
    ref = check(s, value, next_value, got, what=f"planted {dims} final={final}")
    places = RR.places(T, N)
    for (t, n), want in RR.expected(places, s.n_agents).items():
        assert tuple(float(x) for x in got["done_eff"][t, n]) == tuple(want), (t, n, places[(t, n)])
    own_adv, _ = old_gae(s.reward, s.done, value, next_value)
    eff, own, lim = got["done_eff"], s.done, s.truncated
    assert torch.equal(eff[~lim], own[~lim]) and bool((eff & ~own).any()) and bool((~eff & own).any())
    changed = got["advantage"] != own_adv
    assert bool((changed & (eff & ~own)).any()) and bool((changed & (~eff & own)).any())     # both directions, on time-limit rows
    assert not bool((changed & ~lim[..., None]).any(-1)[T - 1].any())                          # the last step only where the flag moved
    # and on the rows before them: env 5 is "solved" and env 7 "own_done_far" at t = 1; agent 0 of both continues through t = 0
    assert places[(1, 5)] == "solved" and places[(1, 7)] == "own_done_far" and not bool(eff[0, 5, 0]) and not bool(eff[0, 7, 0])
    for n in (5, 7):
        assert bool(changed[1, n, 0]) and bool(changed[0, n, 0]) and bool(eff[0, n, 0]) == bool(own[0, n, 0]), n
    assert np.abs(ref["advantage"] - own_adv.cpu().numpy()).max() > 1e-2
    # the bootstrap row instead of next_value
    got = run(s, value)
    check(s, value, None, got, what=f"planted {dims} final={final}, bootstrap row")


@pytest.mark.parametrize("dims", [COUPLED, DECOUPLED])
def test_rule_zero_is_qr_gae(dims):
    s = rule_storage(dims, device="cuda", seed=12)
    value, next_value = _values(s, 12)
    for nv in (None, next_value):
        got = run(s, value, nv, rule=None)
        adv, tgt = old_gae(s.reward, s.done, value, nv)
        assert same_bits(got["advantage"], adv) and same_bits(got["td_target"], tgt) and torch.equal(got["done_eff"], s.done)
        check(s, value, nv, got, rule=None, what=f"rule 0 {dims}")
    got = run(s, value[:T].contiguous(), next_value, rule=None, gamma=0.95, lam=0.5)     # [T] rows of value will do with next_value
    adv, tgt = old_gae(s.reward, s.done, value, next_value, 0.95, 0.5)
    assert same_bits(got["advantage"], adv) and same_bits(got["td_target"], tgt)


@pytest.mark.parametrize("dims", [COUPLED, DECOUPLED])
@pytest.mark.parametrize("t,n", [(1, 65), (8, 65), (9, 65), (17, 65), (3, 1), (2, 64 * 257 + 1)])
def test_shapes(dims, t, n):
    """Full and partial prefetch blocks of 8 steps, one env, and more partial vectors than the fold kernel has lanes."""
    s = fake_storage(*dims, t, n, device="cuda", seed=13 + t)
    s.final_obs[0][:, ::3, :3] *= 0.02
    if s.n_agents == 2:
        s.final_obs[1][:, ::3, 0] *= 0.01
    s.reward[:, ::5] = -1.0
    value, next_value = _values(s, 13 + t)
    got = run(s, value, next_value)
    check(s, value, next_value, got, what=f"{dims} T={t} N={n}")
    lim = s.truncated
    assert bool((got["done_eff"] & ~s.done).any()) or t * n < 500
    assert torch.equal(got["done_eff"][~lim], s.done[~lim])
    assert got["workspace"].numel() == max(1, (n * s.n_agents + 63) // 64) * 2 * s.n_agents


@pytest.mark.parametrize("dims", [COUPLED, DECOUPLED])
def test_stats_are_the_same_bits_from_call_to_call(dims):
    s = fake_storage(*dims, 5, 64 * 40 + 7, device="cuda", seed=14)
    value, next_value = _values(s, 14)
    a, b = run(s, value, next_value), run(s, value, next_value)
    for name in ("advantage", "td_target", "done_eff", "stats", "normalized", "workspace"):
        assert same_bits(a[name], b[name]), name
    st = a["stats"].cpu().numpy()
    assert (st[:, 2] == 5 * (64 * 40 + 7)).all() and (st[:, 1] > 0).all()
    if s.n_agents == 2:   # the agents' sums are their own columns'
        x = a["advantage"].double()
        assert abs(st[1, 0] - float(x[..., 1].sum())) <= 1e-9 * float(x[..., 1].abs().sum()) and abs(st[0, 0] - st[1, 0]) > 1e-6


@pytest.mark.parametrize("dims", [COUPLED, DECOUPLED])
def test_outputs_the_caller_did_not_ask_for(dims):
    from gym_rotor_amd import _lib as L
    from gym_rotor_amd import gae_rule_workspace_numel
    s = rule_storage(dims, device="cuda", seed=15)
    value, next_value = _values(s, 15)
    full = run(s, value, next_value)
    for outputs in ((), ("done_eff",), ("stats",), ("stats", "normalized")):
        part = run(s, value, next_value, outputs=outputs)
        for name in ("advantage", "td_target") + outputs:
            assert same_bits(part[name], full[name]), (outputs, name)
    # the entry itself: normalized without stats, and one transition per agent
    na = s.n_agents
    z = lambda *shape, dtype=torch.float32: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
    adv, tgt, nrm, st, ws = z(T, N, na), z(T, N, na), z(T, N, na), z(na, 3, dtype=torch.float64), z(gae_rule_workspace_numel(N, na), dtype=torch.float64)
    stream = torch.cuda.current_stream().cuda_stream
    e = L.gae_rule_args(s.reward, s.done, s.truncated, s.final_obs, value, next_value, adv, tgt, None, None, nrm, None, n_steps=T, n_envs=N, n_agents=na,
                        gamma=GAMMA, lam=LAM, rule=RULE)
    assert L.load().qr_gae_rule(C.byref(e), stream) == -1         # QR_E_NULL
    e = L.gae_rule_args(s.reward, s.done, s.truncated, s.final_obs, value, next_value, adv, tgt, None, st, nrm, ws, n_steps=1, n_envs=1, n_agents=na,
                        gamma=GAMMA, lam=LAM, rule=RULE)
    assert L.load().qr_gae_rule(C.byref(e), stream) == -3         # QR_E_SIZE
    torch.cuda.synchronize()
    for x in (adv, tgt, nrm, st, ws):
        assert bool((x == SENTINEL).all())                         # nothing was launched
    e.normalized = None                                            # T * N = 1 without the normalisation is a call like any other
    assert L.load().qr_gae_rule(C.byref(e), stream) == 0
    torch.cuda.synchronize()
    assert float(st[0, 2]) == 1.0 and float(st[0, 0]) == float(adv[0, 0, 0]) and bool((adv.reshape(-1)[na:] == SENTINEL).all())


def test_unaligned_advantages_take_the_scalar_normalise_pass():
    """A 16-byte aligned call and one whose advantage and normalized tensors start 4 bytes off give the same bits."""
    from gym_rotor_amd import gae_rule, gae_rule_workspace_numel
    s = rule_storage(DECOUPLED, device="cuda", seed=16)
    value, next_value = _values(s, 16)
    full = run(s, value, next_value)
    n = T * N * 2
    adv = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    nrm = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    off = 1 if adv.data_ptr() % 16 == 0 else 0       # (torch's allocations are 16-byte aligned: one float further is not)
    a, m = adv[off:off + n].view(T, N, 2), nrm[off:off + n].view(T, N, 2)
    assert a.data_ptr() % 16 != 0
    st = torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    gae_rule(s.reward, s.done, value, a, torch.empty(T, N, 2, device="cuda"), gamma=GAMMA, lam=LAM, next_value=next_value, truncated=s.truncated,
             term_obs=s.final_obs, rule=RULE, stats=st, normalized=m, workspace=torch.zeros(gae_rule_workspace_numel(N, 2), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert same_bits(a, full["advantage"]) and same_bits(m, full["normalized"]) and same_bits(st, full["stats"])
    assert bool((nrm[:off] == SENTINEL).all()) and bool((nrm[off + n:] == SENTINEL).all())


def _composition(st, next_value, rule, gamma=GAMMA, lam=LAM):
    """What a user of the parent writes for the same result: the reference's stored done in torch, qr_gae on it, the per-agent sums in
    torch, normalize.  Returns (done_eff, advantage, td_target, normalized)."""
    import math
    from gym_rotor_amd import RolloutStorage
    T_, N_ = st.T, st.N
    eff = st.done.clone()
    for k in range(st.n_agents):
        nxt = st.final_obs[k] if st.final_obs is not None else st.obs[k][1:]
        err = nxt[..., :3].double() * rule.x_lim if k == 0 else nxt[..., :1].double() * math.pi
        solved = (err.abs() <= (rule.pos_tol if k == 0 else rule.rot_tol)).all(-1) & (st.reward[..., k] != -1.0)
        eff[..., k] = torch.where(st.truncated, solved, st.done[..., k])
    adv, tgt = old_gae(st.reward, eff, st.value, next_value, gamma, lam)
    a64 = adv.double()
    stats = torch.cat([torch.stack([a64.sum((0, 1)), (a64 * a64).sum((0, 1))], 1),
                       torch.full((st.n_agents, 1), float(T_ * N_), dtype=torch.float64, device=adv.device)], 1)
    return eff, adv, tgt, RolloutStorage.normalize(adv, stats)


def _one_ulp(have, want):
    have, want = have.cpu().numpy(), want.cpu().numpy()
    ulp = np.spacing(np.maximum(np.abs(want), np.abs(have)).astype(np.float32))
    return bool((np.abs(have.astype(np.float64) - want.astype(np.float64)) <= ulp).all())


@pytest.mark.parametrize("dims,final", [(COUPLED, True), (DECOUPLED, True), (DECOUPLED, False)])
def test_compute_gae_on_a_storage(dims, final):
    from gym_rotor_amd import TimeLimitRule
    s = rule_storage(dims, device="cuda", final_obs=final, seed=17)
    value, next_value = _values(s, 17)
    st = real_storage(s, device="cuda:0", x_lim=1.0)
    st.value.copy_(value)
    adv, tgt, stats = st.compute_gae(GAMMA, LAM, next_value=next_value, time_limit="solved", normalized=True, done_eff=True)
    torch.cuda.synchronize()
    assert adv is st.advantage and tgt is st.td_target and stats is st.gae_stats and st.done_eff.dtype == torch.bool
    eff, want_adv, want_tgt, want_nrm = _composition(st, next_value, TimeLimitRule())
    assert torch.equal(st.done_eff, eff) and same_bits(adv, want_adv) and same_bits(tgt, want_tgt) and _one_ulp(st.advantage_normalized, want_nrm)
    kept = (st.advantage_normalized.data_ptr(), st.done_eff.data_ptr(), st.gae_stats.data_ptr())
    # another rule's numbers, the bootstrap row, no statistics
    rule = TimeLimitRule(1.25, 0.5, 0.01)
    out = st.compute_gae(GAMMA, LAM, last_value=value[T] * 0.5, time_limit="solved", rule=rule, want_stats=False, done_eff=True)
    torch.cuda.synchronize()
    eff2, want_adv, want_tgt, _ = _composition(st, None, rule)
    assert out[2] is None and torch.equal(st.done_eff, eff2) and not torch.equal(eff, eff2) and same_bits(out[0], want_adv) and same_bits(out[1], want_tgt)
    assert torch.equal(st.value[T], value[T] * 0.5) and kept == (st.advantage_normalized.data_ptr(), st.done_eff.data_ptr(), st.gae_stats.data_ptr())
    # "own" through the new entry, and the untouched default path
    adv_own = st.compute_gae(GAMMA, LAM, next_value=next_value, done_eff=True)[0].clone()
    assert torch.equal(st.done_eff, st.done)
    old = st.compute_gae(GAMMA, LAM, next_value=next_value)
    assert same_bits(old[0], adv_own) and len(old) == 3 and old[2] is not st.gae_stats


def test_a_real_rollout_through_the_collector():
    """max_episode_steps = 2 inside T = 3: every env meets its time limit (or crashes first)."""
    from gym_rotor_amd import CriticParams, PpoCollector, QuadVecEnv, RolloutStorage, TimeLimitRule, random_actors
    torch.manual_seed(3)
    env = QuadVecEnv("decoupled", 70, device="cuda", auto_reset=True, obs_rows=True, max_episode_steps=2, seed=4)
    env.reset("train")
    env.get_norm_error_state()
    rule = TimeLimitRule(float(env.x_lim), 1.0, 1.0)                # wide enough that freshly reset envs count as solved
    col = PpoCollector(env, 3, gamma=0.97, lam=0.85, time_limit="solved", rule=rule, track_episodes=True)   # (not compute_gae's defaults)
    actors = random_actors("decoupled", "cuda", torch.Generator(device="cuda").manual_seed(1), log_std=-1.0)
    critics = [CriticParams.from_module(_Critic(15, 16).cuda()), CriticParams.from_module(_Critic(3, 8).cuda(), inputs=(1,))]
    st, nrm = col.collect(actors, critics, noise_seed=5)
    torch.cuda.synchronize()
    assert st is col.storage and nrm is st.advantage_normalized and st.final_obs is not None and st.done_eff is None
    assert int(st.truncated.sum()) >= 1
    # what the collector's own call left, kept before anything else touches the storage
    got_adv, got_tgt, got_nrm, got_stats = st.advantage.clone(), st.td_target.clone(), nrm.clone(), st.gae_stats.clone()
    next_value = st.compute_values(critics)
    eff, adv, tgt, want = _composition(st, next_value, rule, 0.97, 0.85)
    assert same_bits(got_adv, adv) and same_bits(got_tgt, tgt) and _one_ulp(got_nrm, want)
    assert _one_ulp(got_nrm, RolloutStorage.normalize(got_adv, got_stats)) and float(got_stats[0, 2]) == 3 * 70
    assert torch.isfinite(got_nrm).all() and float(got_nrm.std()) > 0.5
    # the rule, the collector's gamma and lambda and the critics' next values all matter on this horizon
    assert not torch.equal(eff, st.done)
    assert not same_bits(got_adv, old_gae(st.reward, st.done, st.value, next_value, 0.97, 0.85)[0])
    assert not same_bits(got_adv, _composition(st, next_value, rule)[1]) and not same_bits(got_adv, _composition(st, None, rule, 0.97, 0.85)[1])
    # the effective flags, from a second call with the collector's arguments, whose advantages are the collector's
    st.compute_gae(col.gamma, col.lam, next_value=next_value, time_limit=col.time_limit, rule=col.rule, normalized=True, done_eff=True)
    torch.cuda.synchronize()
    assert torch.equal(st.done_eff, eff) and same_bits(st.advantage, got_adv) and same_bits(st.td_target, got_tgt)
    assert same_bits(st.advantage_normalized, got_nrm) and same_bits(st.gae_stats, got_stats)
    from gym_rotor_amd import _lib as L
    assert int(col.episodes.last[L.EP_COUNT]) == int(st.reset_mask().sum()) >= 70


def test_graph_capture():
    """One compute_gae(time_limit="solved", normalized=True) captured, replayed on three horizons, against eager calls."""
    horizons = [rule_storage(DECOUPLED, device="cuda", seed=20 + i) for i in range(3)]
    vals = [_values(h, 20 + i) for i, h in enumerate(horizons)]
    graphed, eager = real_storage(horizons[0], device="cuda:0"), real_storage(horizons[0], device="cuda:0")
    next_value = torch.zeros(T, N, 2, device="cuda")
    graphed.compute_gae(GAMMA, LAM, next_value=next_value, time_limit="solved", normalized=True, done_eff=True)   # (loads the library, makes the tensors)
    torch.cuda.synchronize()
    for x in (graphed.advantage, graphed.advantage_normalized, graphed.gae_stats):
        x.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.compute_gae(GAMMA, LAM, next_value=next_value, time_limit="solved", normalized=True, done_eff=True)
    torch.cuda.synchronize()
    assert not graphed.advantage.any() and not graphed.gae_stats.any()      # capturing ran nothing
    seen = []
    for h, (value, nv) in zip(horizons, vals):
        for st in (graphed, eager):
            for dst, src in zip(st.final_obs, h.final_obs):
                dst.copy_(src)
            st.reward.copy_(h.reward), st.done.copy_(h.done), st.truncated.copy_(h.truncated), st.value.copy_(value)
        next_value.copy_(nv)
        g.replay()
        eager.compute_gae(GAMMA, LAM, next_value=nv, time_limit="solved", normalized=True, done_eff=True)
        torch.cuda.synchronize()
        for name in ("advantage", "td_target", "done_eff", "gae_stats", "advantage_normalized"):
            assert same_bits(getattr(graphed, name), getattr(eager, name)), name
        seen.append(graphed.gae_stats.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


@pytest.mark.parametrize("dims,final", [(COUPLED, True), (DECOUPLED, True), (DECOUPLED, False)])
def test_torch_op_against_ctypes(dims, final):
    import gym_rotor_amd  # noqa: F401
    from gym_rotor_amd import gae_rule_workspace_numel
    s = rule_storage(dims, device="cuda", final_obs=final, seed=30)
    value, next_value = _values(s, 30)
    na = s.n_agents
    want = run(s, value, next_value, rule=(1.25, 0.04, 0.02))
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device="cuda")
    adv, tgt, eff, st, nrm, ws = z(T, N, na), z(T, N, na), z(T, N, na, dtype=torch.bool), z(na, 3, dtype=torch.float64), z(T, N, na), \
        z(gae_rule_workspace_numel(N, na), dtype=torch.float64)
    term = s.final_obs if final else [o[1:] for o in s.obs]
    torch.ops.gym_rotor_amd.qr_gae_rule(s.reward, s.done, s.truncated, term, value, next_value, adv, tgt, eff, st, nrm, ws, GAMMA, LAM, True,
                                        1.25, 0.04, 0.02, 1e-4)
    torch.cuda.synchronize()
    for name, x in (("advantage", adv), ("td_target", tgt), ("done_eff", eff), ("stats", st), ("normalized", nrm)):
        assert same_bits(x, want[name]), name
    own = run(s, value, None, rule=None, outputs=())
    torch.ops.gym_rotor_amd.qr_gae_rule(s.reward, s.done, None, [], value, None, adv, tgt, None, None, None, None, GAMMA, LAM, False, 0.0, 0.0, 0.0, 1e-4)
    torch.cuda.synchronize()
    assert same_bits(adv, own["advantage"]) and same_bits(tgt, own["td_target"]) and not same_bits(adv, want["advantage"])
