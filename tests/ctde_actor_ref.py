"""Float64 NumPy restatement of agent k's TD3 actor half under the centralized (CTDE) critic of two agents (qr_ctde_dpg_actor_grad;
include/quadrotor_hip.h) with hand-derived gradients, built on tests/td3_actor_ref.py's pieces, and the loader of
tests/golden/ctde_actor.npz (tools/gen_golden_ctde_actor.py).  No torch, no GPU."""
import os

import numpy as np

from td3_actor_ref import ACTOR_NAMES, MARGIN, Q1_NAMES, ROWS, STATS, actor_backward, actor_pass, f64, q1_and_dqda  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ctde_actor.npz")
# sat0 / sat1: the issue's `sat`, k = 0 and k = 1 on the same networks and rows
CASES = ("k0", "k1", "h64", "h5", "noreg", "sat0", "sat1", "w28a", "w28b")
SUPPLIED = ("w28a", "w28b")   # the other agent's action is given, its actor is not


def load():
    return np.load(GOLDEN, allow_pickle=False)


def case(g, name: str) -> dict:
    """One case as a dict: k, obs0, obs1, obs_next0, obs_next1, a0_* / a1_* (the actors that exist), c_* (Q1), action_other (supplied
    form), noise, nominal, lam, max_action and the reference's float64 loss, q_mean, clamp_share, reg, g_*.  Networks and rows are the
    case's own or, where the key `shared` names another case, that case's."""
    assert name in [str(n) for n in g["cases"]]
    out = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
    if "shared" in out:
        owner = str(out.pop("shared"))
        for k in g.files:
            if k.startswith(owner + "_") and k[len(owner) + 1:].split("_")[0] in ("a0", "a1", "c", "obs0", "obs1", "obs") and k[len(owner) + 1:] not in out:
                out[k[len(owner) + 1:]] = g[k]
    out["k"] = int(out["k"])
    out["lam"] = tuple(float(v) for v in out["coeffs"][:3])
    out["max_action"] = float(out["coeffs"][3])
    return out


def actor_of(c, m):
    """Agent m's six tensors, or None where the case has none (the supplied form)."""
    return [c[f"a{m}_{n}"] for n in ACTOR_NAMES] if f"a{m}_fc1_w" in c else None


def q1_of(c):
    return [c["c_" + n] for n in Q1_NAMES]


def other_action(actors, obs, k, action_other, max_action, rows=None):
    """The other agent's action as the critic reads it, float64: supplied as it is, or its actor's clamped output."""
    if action_other is not None:
        return f64(action_other)
    mu = actor_pass([f64(t) for t in actors[1 - k]], f64(obs[1 - k]))[2]
    return np.clip(mu, -max_action, max_action)


def _row(obs, a_own, a_other, k):
    acts = [a_own, a_other] if k == 0 else [a_other, a_own]
    return np.concatenate([f64(obs[0]), f64(obs[1])], axis=1), np.concatenate(acts, axis=1)


def ctde_dpg_actor_grad_f64(actors, q, obs, obs_next_k, k, action_other, noise, nominal, lam, max_action):
    """(stats [4], grads {name: array}) of agent k's loss, derived by hand; float64.  actors: the pair of six-tensor lists (the other's
    None with action_other [B, A_other], by row); q: Q1's six; obs: the pair of [B, D_m] rows; obs_next_k, noise, nominal: agent k's."""
    w, q = [f64(t) for t in actors[k]], [f64(t) for t in q]
    x = f64(obs[k])
    B, A = x.shape[0], w[4].shape[0]
    lam_T, lam_S, lam_M = lam
    clip = lambda m: np.clip(m, -max_action, max_action)
    z1, z2, mu = actor_pass(w, x)
    a = clip(mu)
    ao = other_action(actors, obs, k, action_other, max_action)
    so, sa = _row(obs, a, ao, k)
    _, _, val, dqda = q1_and_dqda(q, so, sa)
    off = 0 if k == 0 else ao.shape[1]
    da = -dqda[:, off:off + A] / B          # the other agent's columns carry a value only
    reg = 0.0
    grads = [np.zeros_like(t) for t in w]
    others = []
    if lam_S != 0:
        others.append((x + f64(noise)[None, :], lam_S))
    if lam_T != 0:
        others.append((f64(obs_next_k), lam_T))
    for y, lam_y in others:
        y1, y2, mo = actor_pass(w, y)
        d = a - clip(mo)
        reg += lam_y * float(np.mean(d * d))
        c = 2.0 * lam_y / (B * A)
        da = da + c * d
        for gsum, gone in zip(grads, actor_backward(w, y, y1, y2, mo, -c * d * (np.abs(mo) <= max_action))):
            gsum += gone
    if lam_M != 0:
        d = a - f64(nominal)[None, :]
        reg += lam_M * float(np.mean(d * d))
        da = da + (2.0 * lam_M / (B * A)) * d
    for gsum, gone in zip(grads, actor_backward(w, x, z1, z2, mu, da * (np.abs(mu) <= max_action))):
        gsum += gone
    stats = np.array([-val.mean() + reg, val.mean(), float((np.abs(mu) > max_action).sum()) / (B * A), reg])
    return stats, dict(zip(ACTOR_NAMES, grads))


def margins(actors, q, obs, obs_next_k, k, action_other, noise, max_action):
    """The smallest |pre-activation|, float64, over: agent k's fc1 / fc2 on obs, obs_next and obs + noise; the other agent's fc1 / fc2 on
    its obs (where it has an actor); the critic's fc1 / fc2 on the concatenated row."""
    w = [f64(t) for t in actors[k]]
    x = f64(obs[k])
    m = np.inf
    for y in (x, f64(obs_next_k), x + f64(noise)[None, :]):
        z1, z2, _ = actor_pass(w, y)
        m = min(m, float(np.abs(z1).min()), float(np.abs(z2).min()))
    if actors[1 - k] is not None:
        z1, z2, _ = actor_pass([f64(t) for t in actors[1 - k]], f64(obs[1 - k]))
        m = min(m, float(np.abs(z1).min()), float(np.abs(z2).min()))
    a = np.clip(actor_pass(w, x)[2], -max_action, max_action)
    so, sa = _row(obs, a, other_action(actors, obs, k, action_other, max_action), k)
    c1, c2, _, _ = q1_and_dqda([f64(t) for t in q], so, sa)
    return min(m, float(np.abs(c1).min()), float(np.abs(c2).min()))


def case_margin(c, idx=None):
    """`margins` of a fixture case on rows idx (all)."""
    idx = np.arange(ROWS) if idx is None else np.asarray(idx)
    k = c["k"]
    ao = c["action_other"][idx] if "action_other" in c else None
    return margins([actor_of(c, 0), actor_of(c, 1)], q1_of(c), (c["obs0"][idx], c["obs1"][idx]), c[f"obs_next{k}"][idx], k, ao, c["noise"], c["max_action"])


def case_f64(c, idx=None, lam=None):
    """The restatement on rows idx of a fixture case (all rows; `action_other` follows the rows: it is by minibatch position)."""
    idx = np.arange(ROWS) if idx is None else np.asarray(idx)
    k = c["k"]
    ao = c["action_other"][idx] if "action_other" in c else None
    return ctde_dpg_actor_grad_f64([actor_of(c, 0), actor_of(c, 1)], q1_of(c), (c["obs0"][idx], c["obs1"][idx]), c[f"obs_next{k}"][idx], k, ao,
                                   c["noise"], c["nominal"], c["lam"] if lam is None else lam, c["max_action"])


def clamp_shares(c):
    """Per agent with an actor: (share of the components of pi_m(obs_m) with |pi| > max_action, the smallest distance of a |pi| from it)."""
    out = {}
    for m in range(2):
        w = actor_of(c, m)
        if w is not None:
            mu = actor_pass([f64(t) for t in w], f64(c[f"obs{m}"]))[2]
            out[m] = (float((np.abs(mu) > c["max_action"]).mean()), float(np.abs(np.abs(mu) - c["max_action"]).min()))
    return out
