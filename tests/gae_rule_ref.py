"""NumPy restatement of qr_gae_rule (include/quadrotor_hip.h; RolloutStorage.compute_gae(time_limit="solved"), gae_rule): the done flag
the reference stores (main.py:169-173, 176-177: `stored_done` of tests/replay_rule_ref.py, imported) and a literal transcription of
ppo.py:134-146 in float64, run per (env, agent) column over that flag, with a variant that rounds to float32 where the kernel does."""
import numpy as np

import replay_rule_ref as RR

NORM_EPS = 1e-4   # ppo.py:146


def done_eff(obs, final_obs, reward, done, truncated, rule=None):
    """bool [T, N, n_agents]: the flag the scan reads.  rule: None (each agent's own flag) or (x_lim, pos_tol, rot_tol)."""
    if rule is None:
        return np.asarray(done, dtype=bool).copy()
    return RR.stored_done(obs, final_obs, reward, done, truncated, *rule) != 0


def _column(reward, done, value, next_value, gamma, lam, f32):
    """ppo.py:134-146 for one agent's horizon in one env: reward, done, value, next_value [T]."""
    T = len(reward)
    if f32:   # the kernel's float32 recurrence (the build contracts a product into the sum that follows it; not modelled)
        one, zero, gamma, lam = np.float32(1), np.float32(0), np.float32(gamma), np.float32(lam)
    else:
        one, zero = 1.0, 0.0
    td_errors = [reward[t] + gamma * next_value[t] * (one - done[t]) - value[t] for t in range(T)]   # ppo.py:138
    advantages, adv = [], zero
    for td_error, d in zip(reversed(td_errors), reversed(list(done))):                                 # ppo.py:143-145
        adv = td_error + gamma * (one - d) * lam * adv
        advantages.insert(0, adv)
    return advantages


def gae(reward, done, value, next_value, gamma, lam, f32=False):
    """reward, done [T, N, G], value [T, N, G] (V(obs[t])), next_value [T, N, G].  Returns advantage, td_target [T, N, G] in float64,
    or — f32 — in float32 with every operation rounded to float32."""
    dt = np.float32 if f32 else np.float64
    reward, value, next_value = (np.asarray(a).astype(dt) for a in (reward, value, next_value))
    d = np.asarray(done).astype(dt)
    T, N, G = reward.shape
    adv = np.zeros((T, N, G), dtype=dt)
    for n in range(N):
        for g in range(G):
            adv[:, n, g] = _column(reward[:, n, g], d[:, n, g], value[:, n, g], next_value[:, n, g], gamma, lam, f32)
    return adv, adv + value   # ppo.py:146: td_target = adv + V


def sums(adv):
    """float64 [G, 3]: per agent the sum, the sum of squares and the count of its advantages."""
    a = np.asarray(adv, dtype=np.float64)
    T, N, G = a.shape
    return np.stack([a.sum((0, 1)), (a * a).sum((0, 1)), np.full(G, float(T * N))], 1)


def normalize(adv, stats, eps=NORM_EPS):
    """ppo.py:146 with torch's unbiased std, per agent, as RolloutStorage.normalize writes it: float64 [T, N, G]."""
    s1, s2, n = stats[:, 0], stats[:, 1], stats[:, 2]
    mean = s1 / n
    var = (s2 - n * mean * mean) / (n - 1.0)
    std = np.sqrt(np.maximum(var, 0.0))
    return (np.asarray(adv, dtype=np.float64) - mean) / (std + eps)


def sum_bound(terms):
    """The bound of a float64 sum of these terms in any order against any other: (n - 1) * 2^-53 * sum |x| (tests/episode_ref.py)."""
    terms = np.asarray(terms, dtype=np.float64).ravel()
    return max(len(terms) - 1, 0) * 2.0 ** -53 * np.abs(terms).sum()


def run(obs, final_obs, reward, done, truncated, value, next_value, gamma, lam, rule=None, f32=False):
    """The whole call: done_eff, advantage, td_target, stats (of the float64 or float32 advantages), normalized."""
    de = done_eff(obs, final_obs, reward, done, truncated, rule)
    nv = value[1:] if next_value is None else next_value
    adv, tgt = gae(reward, de, value[:len(reward)], nv, gamma, lam, f32)
    st = sums(adv)
    return {"done_eff": de, "advantage": adv, "td_target": tgt, "stats": st, "normalized": normalize(adv, st) if reward.shape[0] * reward.shape[1] > 1 else None}
