"""The restatement of in-loop action selection (tests/action_ref.py) against what it restates, on the CPU: the key layout against
tests/noise_ref.py where the two streams coincide, the rules against oracle/actor_oracle.py on random networks, that the keys
tests/test_gpu_action_noise.py runs tell every wrong key apart, and that the edge grids of tests/test_gpu_action_rules.py have finite
expected values and meaningful bars."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import action_ref as AR  # noqa: E402
import noise_ref as NR  # noqa: E402
from oracle import actor_oracle as ao  # noqa: E402
from test_gpu_noise import NORMAL_BAR, R_MAX  # noqa: E402  (the bar of tests/test_gpu_action_noise.py IS that test's, derivation included)

# ---------------------------------------------------------------------------------------------------------------------
# the key
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,draw,stream,first", [(0, 0, 0, 0), (2 ** 40 + 3, 2 ** 33 + 5, 9, 0), (2 ** 63 + 1, 2 ** 64 - 1, 2 ** 30 - 1, 2 ** 32 - 3)])
def test_rollout_words_coincide_with_the_noise_stream(seed, draw, stream, first):
    """(gid_lo, gid_hi ^ step_hi, step_lo, 0x80000000 | block) with block = 0x40000000 | stream IS noise_fill's counter
    (q_lo, q_hi ^ draw_hi, draw_lo, 0xC0000000 | stream): the same words for gid = q, step = draw."""
    n = 37
    q = np.arange(first, first + n, dtype=np.uint64)
    got = AR.rollout_words(seed, q, np.uint64(draw), 0x40000000 | stream)
    want = NR.words(4 * n, seed, draw, stream, first_quad=first)
    assert got.shape == want.shape == (n, 4) and np.array_equal(got, want)
    # and the normals made of them: rollout_eps's components 0..3 are normals_from_words of block 0
    z = AR.eps_from_blocks(got, got, 4)
    assert np.array_equal(z, NR.normals_from_words(want))


def test_rollout_eps_layout():
    """[T, n, A]; element (t, i) is keyed by (env_offset + i, step_base + t) alone; component 4 is position 0 of block 1; a launch
    split, a shard and the 2^64 wrap of the step give the same numbers."""
    seed, off, n, base, T = AR.NOISE_SEED, AR.NOISE_OFFSET, 7, AR.NOISE_STEPS, 5
    z = AR.rollout_eps(seed, off, n, base, T, 5)
    assert z.shape == (T, n, 5) and np.isfinite(z).all() and np.abs(z).max() <= R_MAX
    assert np.array_equal(z[..., :4], AR.rollout_eps(seed, off, n, base, T, 4))
    assert np.array_equal(z[3:], AR.rollout_eps(seed, off, n, base + 3, 2, 5))
    assert np.array_equal(z[:, 2:], AR.rollout_eps(seed, off + 2, n - 2, base, T, 5))
    for t, i in ((0, 0), (2, 3), (4, 6)):
        w0 = AR.rollout_words(seed, off + i, base + t, 0)
        w1 = AR.rollout_words(seed, off + i, base + t, 1)
        assert np.array_equal(z[t, i, :4], NR.normals_from_words(w0[None])[0])
        assert z[t, i, 4] == NR.normals_from_words(w1[None])[0, 0]
        ctr = (off + i) & 0xFFFFFFFF, ((off + i) >> 32) ^ ((base + t) >> 32), (base + t) & 0xFFFFFFFF, 0x80000000
        assert np.array_equal(w0, NR.philox4(*ctr, seed))
    wrap = AR.rollout_eps(seed, 0, 2, 2 ** 64 - 1, 2, 4)
    assert np.array_equal(wrap[1], AR.rollout_eps(seed, 0, 2, 0, 1, 4)[0])


# ---------------------------------------------------------------------------------------------------------------------
# discrimination: every mistake the GPU test exists for, made in the restatement on the GPU test's own keys
# ---------------------------------------------------------------------------------------------------------------------
def _wrong_eps(mistake: str, seed: int, A: int):
    """[5, NOISE_N, A] under the GPU test's keys with one mistake in the key."""
    T = sum(AR.NOISE_SPLITS)
    gid, step = AR.rollout_ids(AR.NOISE_OFFSET, AR.NOISE_N, AR.NOISE_STEPS, T)
    lo, s32 = NR.U32, np.uint64(32)
    fifth, blocks = 0, (0, 1)
    if mistake == "step_hi dropped":
        step = step & lo
    elif mistake == "gid_hi dropped":
        gid = gid & lo
    elif mistake == "seed_hi dropped":
        seed &= 0xFFFFFFFF
    elif mistake.startswith("block 1 at position"):
        fifth = int(mistake[-1])
    elif mistake == "blocks swapped":
        blocks = (1, 0)
    elif mistake in ("step +1", "step -1"):
        step = step + np.uint64(1) if mistake.endswith("+1") else step - np.uint64(1)
    elif mistake in ("gid +64", "gid -64"):
        gid = gid + np.uint64(64) if mistake.endswith("+64") else gid - np.uint64(64)
    elif mistake == "step_hi in word 3":                      # misplaced: the high word of the step joins the block word
        w = [np.moveaxis(NR.philox4(*np.broadcast_arrays(gid & lo, gid >> s32, step & lo, np.uint64(0x80000000 | b) | (step >> s32)), seed), 0, -1)
             for b in blocks]
        return AR.eps_from_blocks(w[0], w[1], A)
    elif mistake == "gid_hi in word 2":                       # misplaced: the high word of the id joins the step's low word
        w = [np.moveaxis(NR.philox4(*np.broadcast_arrays(gid & lo, step >> s32, (step & lo) ^ (gid >> s32), np.uint64(0x80000000 | b)), seed), 0, -1)
             for b in blocks]
        return AR.eps_from_blocks(w[0], w[1], A)
    elif mistake == "seed words exchanged":
        seed = ((seed & 0xFFFFFFFF) << 32) | (seed >> 32)
    else:
        raise AssertionError(mistake)
    return AR.eps_from_blocks(AR.rollout_words(seed, gid, step, blocks[0]), AR.rollout_words(seed, gid, step, blocks[1]), A, fifth)


MISTAKES = ("step_hi dropped", "gid_hi dropped", "seed_hi dropped", "block 1 at position 1", "block 1 at position 2", "block 1 at position 3",
            "blocks swapped", "step +1", "step -1", "gid +64", "gid -64", "step_hi in word 3", "gid_hi in word 2", "seed words exchanged")


# (a wrong word of block 1 reaches component 4 alone: Coupled, which draws nothing from block 1, has no such case)
CASES = [(m, A) for m in MISTAKES for A in (4, 5) if not (m.startswith("block 1") and A == 4)]


@pytest.mark.parametrize("seed", [AR.NOISE_SEED, AR.NOISE_OTHER_SEED])
@pytest.mark.parametrize("mistake,A", CASES)
def test_the_gpu_tests_keys_tell_each_wrong_key_apart(mistake, A, seed):
    """At least 99 % of the elements a mistake can reach differ from the right value by more than 100 bars.  What a mistake can
    reach: a wrong word of block 1 only component 4; the step's high word only the steps that have one — three of the five, since
    the run starts two steps below 2^32 in order to cross it (asserted) — and everything else every element."""
    T = sum(AR.NOISE_SPLITS)
    right = AR.rollout_eps(seed, AR.NOISE_OFFSET, AR.NOISE_N, AR.NOISE_STEPS, T, A)
    wrong = _wrong_eps(mistake, seed, A)
    assert right.shape == wrong.shape == (T, AR.NOISE_N, A)
    reach = np.ones(right.shape, dtype=bool)
    if mistake.startswith("block 1"):
        reach[..., :4] = False
    if mistake.startswith("step_hi"):
        has_hi = np.array([(AR.NOISE_STEPS + t) >> 32 != 0 for t in range(T)])
        assert has_hi.sum() == 3 and not has_hi[0] and has_hi[AR.NOISE_SPLITS[0] - 1]      # crossed inside the first launch
        reach[~has_hi] = False
        assert np.array_equal(right[~has_hi], wrong[~has_hi])
    far = np.abs(right - wrong) > 100.0 * NORMAL_BAR
    assert far[reach].mean() >= 0.99, (mistake, float(far[reach].mean()))
    assert reach.mean() >= (0.2 if mistake.startswith("block 1") else 0.6)


def test_the_gpu_tests_keys_have_the_high_words_the_issue_names():
    assert AR.NOISE_SEED >> 32 and AR.NOISE_OTHER_SEED >> 32 and AR.NOISE_OFFSET >> 32 and AR.NOISE_OFFSET % 64 == 0
    assert AR.NOISE_N == 133 and AR.NOISE_SPLITS == (3, 2) and AR.NOISE_STEPS == 2 ** 32 - 2
    assert AR.NOISE_SEED < 2 ** 63 and AR.NOISE_OTHER_SEED < 2 ** 63 and AR.NOISE_OTHER_SEED != AR.NOISE_SEED


# ---------------------------------------------------------------------------------------------------------------------
# the rules against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _network(rng, D, H, A, sac):
    p = {"fc1_w": rng.normal(0, 0.4, (H, D)), "fc1_b": rng.normal(0, 0.2, H), "fc2_w": rng.normal(0, 0.4, (H, H)), "fc2_b": rng.normal(0, 0.2, H),
         "mean_w": rng.normal(0, 0.8, (A, H)), "mean_b": rng.normal(0, 0.3, A)}
    if sac:
        p["log_std_w"], p["log_std_b"] = rng.normal(0, 3.0, (A, H)), rng.normal(-4, 3.0, A)     # wide: both clamps are met
    else:
        p["log_std"] = rng.normal(-1, 1.5, A)
    return p


def _hidden(p, obs):
    h = np.maximum(obs @ p["fc1_w"].T + p["fc1_b"], 0.0)
    return np.maximum(h @ p["fc2_w"].T + p["fc2_b"], 0.0)


@pytest.mark.parametrize("dims", [(23, 16, 4), (15, 16, 4), (3, 4, 1)])
def test_the_rules_are_the_oracles(dims):
    rng = np.random.default_rng(sum(dims))
    D, H, A = dims
    obs, eps = rng.normal(0, 2.0, (200, D)), rng.normal(0, 1.0, (200, A))
    for max_action in (1.0, 0.5, 0.05):
        p = _network(rng, D, H, A, sac=False)
        pre = _hidden(p, obs) @ p["mean_w"].T + p["mean_b"]
        a, lp, mean = AR.tanh_mean_rule(pre, p["log_std"], eps, max_action)
        wa, wl, wm = ao.choose_action(p, obs, eps, max_action)
        assert np.abs(a - wa).max() <= 1e-12 and np.abs(lp - wl).max() <= 1e-12 * np.abs(wl).max() and np.abs(mean - wm).max() <= 1e-12
        if A > 1:
            assert (np.abs(a) == max_action).any() and (np.abs(a) < max_action).any()
        a, _, _ = AR.tanh_mean_rule(pre, p["log_std"], None, max_action)
        assert np.abs(a - ao.choose_action(p, obs, None, max_action)[0]).max() <= 1e-12
        # the clamped form is the same rule on the clamped log_std
        wide = p["log_std"] * 12.0
        a1, l1, _ = AR.tanh_mean_rule(pre, wide, eps, max_action, clamp_log_std=True)
        a2, l2, _ = AR.tanh_mean_rule(pre, np.clip(wide, -20.0, 2.0), eps, max_action)
        assert np.array_equal(a1, a2) and np.array_equal(l1, l2)
    p = _network(rng, D, H, A, sac=True)
    h = _hidden(p, obs)
    pre, ls = h @ p["mean_w"].T + p["mean_b"], h @ p["log_std_w"].T + p["log_std_b"]
    a, lp, u, lsc = AR.tanh_sample_rule(pre, ls, eps)
    wa, wl, wm, wls = ao.sac_sample(p, obs, eps)
    if A > 1:
        assert (lsc == -20.0).any() and (lsc == 2.0).any() and ((lsc > -20.0) & (lsc < 2.0)).any()
    assert np.abs(a - wa).max() <= 1e-12 and np.abs(lp - wl).max() <= 1e-12 * np.abs(wl).max()
    assert np.abs(pre - wm).max() <= 1e-12 * np.abs(wm).max() and np.array_equal(lsc, wls)
    a, _, _, _ = AR.tanh_sample_rule(pre, ls, None)
    assert np.abs(a - ao.sac_sample(p, obs, None)[0]).max() <= 1e-12
    # the log-prob given the action: the rule's own where the action is the rule's (float32-exact actions: bit for bit the same formula)
    a, lp, u, lsc = AR.tanh_sample_rule(pre, ls, eps)
    keep = np.abs(a) < 0.999
    got = AR.sac_logp_from_action(lsc, eps, a.astype(np.float32))
    assert np.abs(got - lp)[keep].max() <= 1e-3            # (float32 rounding of a, through 2 a / (1 - a^2) <= 1000: 6e-8 * 1000)
    exact = -0.5 * eps ** 2 - lsc - ao.LOG_SQRT_2PI - np.log(1.0 - a.astype(np.float32).astype(np.float64) ** 2 + 1e-6)
    assert np.array_equal(got, exact)
    # and the Normal's given the action
    p = _network(rng, D, H, A, sac=False)
    pre = _hidden(p, obs) @ p["mean_w"].T + p["mean_b"]
    a, lp, mean = AR.tanh_mean_rule(pre, p["log_std"], eps, 0.5)
    got = AR.normal_logp_from_action(mean, np.broadcast_to(p["log_std"], mean.shape), a.astype(np.float32))
    z = (a - mean) * np.exp(-p["log_std"])
    assert np.abs(got - lp).max() <= (np.abs(z) * np.exp(-p["log_std"]) * 2.0 ** -24 + 1e-12).max() * 1.01 + 1e-9 * np.abs(lp).max()


def test_actor_params_accepts_a_log_std_head_with_the_tanh_mean_rule():
    """The combination tests/test_gpu_action_rules.py runs as 'mean_head' is one the host lets through (policy.ActorParams.check):
    either log_std source with either rule."""
    from gym_rotor_amd import ActorParams, _lib
    z = lambda *s: torch.zeros(*s)
    a = ActorParams(z(16, 23), z(16), z(16, 16), z(16), z(4, 16), z(4), None, z(4, 16), z(4), _lib.ACTOR_TANH_MEAN)
    a.check((23, 16, 4), torch.device("cpu"))
    with pytest.raises(ValueError):
        ActorParams(z(16, 23), z(16), z(16, 16), z(16), z(4, 16), z(4), None, None, None, _lib.ACTOR_TANH_MEAN).check((23, 16, 4), torch.device("cpu"))


# ---------------------------------------------------------------------------------------------------------------------
# the edge grids
# ---------------------------------------------------------------------------------------------------------------------
def _grid(rule, A, max_action=1.0):
    ls_values = AR.MEAN_LS if rule == "mean" else AR.SAC_LS
    for j, row in enumerate(AR.bias_sets(ls_values, A)):
        yield (j,) + AR.rule_launch(rule, row, max_action, index=j)


@pytest.mark.parametrize("A", [4, 5])
def test_sample_grid_is_finite_and_on_its_edges(A):
    seen_ls, seen_pre, seen4 = set(), set(), set()
    hit = set()
    for j, pre, ls, eps in _grid("sample", A):
        assert eps.shape == (1, AR.RULE_N, A) and eps.dtype == np.float32 and pre.dtype == ls.dtype == np.float32
        a, lp, u, lsc = AR.tanh_sample_rule(pre.astype(np.float64), ls.astype(np.float64), eps[0].astype(np.float64))
        for v in (a, lp, u, lsc, AR.sac_action_bar(pre, lsc, eps[0]), AR.sac_logp_bar(lsc, eps[0], a.astype(np.float32)),
                  AR.sac_logp_from_action(lsc, eps[0], a.astype(np.float32))):
            assert np.isfinite(v).all()
        assert np.abs(a).max() <= 1.0 and ((lsc >= -20.0) & (lsc <= 2.0)).all()
        assert float(np.abs(eps).max()) ** 2 < 1e30                      # z^2 stays far inside float32
        assert (AR.sac_logp_bar(lsc, eps[0], a.astype(np.float32)) <= 1e-5 * (1.0 + np.abs(lp) + 14.0)).all()   # tight everywhere
        seen_ls |= set(ls[:4].tolist()); seen_pre |= set(pre[:4].tolist())
        if A == 5:
            seen4.add((float(ls[4]), float(pre[4])))
        # the three draws around each edge put float64 u within a float32 ulp of u (or of sd eps) of it, on both sides
        k = len(AR.BASE_EPS)
        for e, ue in enumerate(AR.U_EDGES):
            tri = u[k + 3 * e:k + 3 * e + 3]
            assert (tri[0] <= ue).all() and (tri[2] >= ue).all() and (np.abs(tri[1] - ue) <= 2.0 ** -23 * (np.abs(ue) + np.abs(tri[1] - pre))).all()
            hit |= set(np.abs(a[k + 3 * e:k + 3 * e + 3]).astype(np.float32).ravel().tolist())
    f = lambda xs: {float(np.float32(x)) for x in xs}
    assert seen_ls == f(AR.SAC_LS) and seen_pre == f(AR.PRE)
    if A == 5:
        assert {l for l, _ in seen4} == f(AR.SAC_LS) and {p for _, p in seen4} == f(AR.PRE)
    assert hit == {1.0, float(np.float32(1.0 - 2.0 ** -24))}, sorted(hit)   # correctly rounded, the edge draws give the last float32 below one and 1.0f


@pytest.mark.parametrize("A", [4, 5])
@pytest.mark.parametrize("rule", ["mean", "mean_head"])
@pytest.mark.parametrize("max_action", AR.MAX_ACTIONS)
def test_mean_grid_is_finite_and_on_its_edges(max_action, rule, A):
    ma = float(np.float32(max_action))
    seen_ls, seen_pre, on, inside, outside = set(), set(), 0, 0, 0
    for j, pre, ls, eps in _grid(rule, A, max_action):
        lsc = np.clip(ls.astype(np.float64), -20.0, 2.0) if rule == "mean_head" else ls.astype(np.float64)
        a, lp, mean = AR.tanh_mean_rule(pre.astype(np.float64), ls.astype(np.float64), eps[0].astype(np.float64), ma, clamp_log_std=rule == "mean_head")
        a32 = a.astype(np.float32)
        for v in (a, lp, AR.mean_action_bar(pre, lsc, eps[0]), AR.mean_logp_bar(pre, lsc, a32), AR.normal_logp_from_action(mean, lsc, a32)):
            assert np.isfinite(v).all()
        assert np.abs(a).max() <= ma and float(np.abs(eps).max()) ** 2 * float(np.exp(-2 * lsc.min())) < 1e38
        seen_ls |= set(ls.tolist()); seen_pre |= set(pre.tolist())
        raw = mean + np.exp(lsc) * eps[0]
        k = len(AR.BASE_EPS)
        for e, b in enumerate((ma, -ma)):
            tri = raw[k + 3 * e:k + 3 * e + 3]
            assert (tri[0] <= b).all() and (tri[2] >= b).all()
            on += int((np.abs(tri[1] - b) <= 2.0 ** -23 * (np.abs(b) + np.abs(tri[1] - mean))).sum())
            inside += int((np.abs(tri) < ma).sum()); outside += int((np.abs(tri) > ma).sum())
    f = lambda xs: {float(np.float32(x)) for x in xs}
    assert seen_ls == f(AR.MEAN_LS if rule == "mean" else AR.SAC_LS) and seen_pre == f(AR.PRE)
    assert on > 0 and inside > 0 and outside > 0


def test_mean_logp_bar_is_small_where_the_action_is_clamped_far_from_the_mean():
    """The bar's relative form is 2 (2e-7 / |a - mean| + exp_rel): where the clamp holds the action 0.01 or more from the mean and
    |z| >= 1e3 (a small std) it is below 1e-4 of the value — log_std = -20 included, where the value is ~1e16 — and at log_std >= -1 it
    is below 1e-4 absolutely wherever |z| <= 6."""
    for ls in AR.MEAN_LS:
        for pre in AR.PRE:
            for a in (1.0, -1.0, 0.5, -0.05):
                mean = np.tanh(pre)
                z = (a - mean) * np.exp(-ls)
                bar = float(AR.mean_logp_bar(np.float32(pre), np.float32(ls), np.float32(a)))
                want = abs(float(AR.normal_logp_from_action(mean, ls, np.float32(a))))
                if abs(z) >= 1e3 and abs(a - mean) >= 0.01:
                    assert bar <= 1e-4 * want, (ls, pre, a, bar, want)
                if ls >= -1.0 and abs(z) <= 6.0:
                    assert bar <= 1e-4, (ls, pre, a, bar)


def test_heads_with_error_bounds_a_float32_evaluation():
    """The running bound of heads_with_error against float32 NumPy evaluations of the same network in two summation orders."""
    rng = np.random.default_rng(5)
    p = {k: v.astype(np.float32) for k, v in _network(rng, 23, 16, 4, sac=True).items()}
    obs = rng.normal(0, 20.0, (300, 23)).astype(np.float32)
    pre, ls, pe, le = AR.heads_with_error(p, obs)
    assert pe.shape == pre.shape and (pe > 0).all() and pe.max() < 1e-3 * max(1.0, np.abs(pre).max())
    for order in (slice(None), slice(None, None, -1)):
        def lin(w, b, x):
            y = b.copy()[None].repeat(len(x), 0)
            for k in list(range(w.shape[1]))[order]:
                y = (y + x[:, k:k + 1] * w[None, :, k]).astype(np.float32)
            return y
        h = np.maximum(lin(p["fc1_w"], p["fc1_b"], obs), 0)
        h = np.maximum(lin(p["fc2_w"], p["fc2_b"], h), 0)
        assert (np.abs(lin(p["mean_w"], p["mean_b"], h) - pre) <= pe).all() and (np.abs(lin(p["log_std_w"], p["log_std_b"], h) - ls) <= le).all()
