"""Float64 NumPy restatement of the TD3 actor half (qr_dpg_actor_grad, qr_soft_update; include/quadrotor_hip.h) with hand-derived
gradients, and the loader of tests/golden/td3_actor.npz (tools/gen_golden_td3_actor.py).  No torch, no GPU."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "td3_actor.npz")
ACTOR_NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")     # the module's names; the library's: DPG_GRAD_NAMES
Q1_NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")
STATS = ("loss", "q_mean", "clamp_share", "reg")
CASES = ("mono", "dtde0", "dtde1", "h64", "h5", "h1", "noreg", "sat")
MARGIN = 2e-5         # every pre-activation keeps this distance from ReLU's kink
TANH_FAST_ERR = 2e-7  # absolute error of the device's tanh (qr_actor.h): how far the critic's fc1 input `a` may be off
ROWS = 130


def load():
    return np.load(GOLDEN, allow_pickle=False)


def case(g, name: str) -> dict:
    """One case as a dict.  Its critic (Q1's six float32 tensors c_<name>) is its own or, where the key `critic` names another case,
    that case's."""
    assert name in [str(n) for n in g["cases"]]
    out = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
    owner = str(out.pop("critic")) if "critic" in out else name
    for n in Q1_NAMES:
        out["c_" + n] = g[f"{owner}_c_{n}"]
    out["lam"] = tuple(float(v) for v in out["coeffs"][:3])
    out["max_action"] = float(out["coeffs"][3])
    return out


def f64(x):
    return np.asarray(x, dtype=np.float64)


def relu(x):
    return np.maximum(x, 0.0)


def actor_pass(w, x):
    """MLP_Actor_TD3 forwards: (z1, z2, mu)."""
    z1 = x @ w[0].T + w[1]
    z2 = relu(z1) @ w[2].T + w[3]
    return z1, z2, np.tanh(relu(z2) @ w[4].T + w[5])


def actor_backward(w, x, z1, z2, mu, dmu):
    """The six gradients of sum(dmu * mu) for one pass."""
    dp = dmu * (1.0 - mu * mu)
    dz2 = (dp @ w[4]) * (z2 > 0)
    dz1 = (dz2 @ w[2]) * (z1 > 0)
    return [dz1.T @ x, dz1.sum(0), dz2.T @ relu(z1), dz2.sum(0), dp.T @ relu(z2), dp.sum(0)]


def q1_and_dqda(q, obs, a):
    """(z1, z2, Q1 [B], dQ1/da [B, A]) of Q1 = fc3(relu(fc2(relu(fc1([obs | a])))))."""
    sa = np.concatenate([obs, a], axis=1)
    z1 = sa @ q[0].T + q[1]
    z2 = relu(z1) @ q[2].T + q[3]
    val = (relu(z2) @ q[4].T + q[5])[:, 0]
    dz2 = q[4] * (z2 > 0)
    dz1 = (dz2 @ q[2]) * (z1 > 0)
    return z1, z2, val, (dz1 @ q[0])[:, obs.shape[1]:]


def dpg_actor_grad_f64(w, q, obs, obs_next, noise, nominal, lam, max_action):
    """(stats [4], grads {name: array}) of the TD3 actor loss, derived by hand; float64.  w: the actor's six tensors, q: Q1's six."""
    w, q, obs = [f64(t) for t in w], [f64(t) for t in q], f64(obs)
    B, A = obs.shape[0], w[4].shape[0]
    lam_T, lam_S, lam_M = lam
    clip = lambda m: np.clip(m, -max_action, max_action)
    z1, z2, mu = actor_pass(w, obs)
    a = clip(mu)
    _, _, val, dqda = q1_and_dqda(q, obs, a)
    da = -dqda / B
    reg = 0.0
    grads = [np.zeros_like(t) for t in w]
    others = []
    if lam_S != 0:
        others.append((obs + f64(noise)[None, :], lam_S))
    if lam_T != 0:
        others.append((f64(obs_next), lam_T))
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
    for gsum, gone in zip(grads, actor_backward(w, obs, z1, z2, mu, da * (np.abs(mu) <= max_action))):
        gsum += gone
    stats = np.array([-val.mean() + reg, val.mean(), float((np.abs(mu) > max_action).sum()) / (B * A), reg])
    return stats, dict(zip(ACTOR_NAMES, grads))


def margins(w, q, obs, obs_next, noise, max_action):
    """(the smallest |pre-activation| over the actor's fc1, fc2 on obs, obs_next and obs + noise and the critic's fc1, fc2 on (obs, a);
    the critic's fc1 margin per hidden unit [H]), float64."""
    w, q, obs = [f64(t) for t in w], [f64(t) for t in q], f64(obs)
    m = np.inf
    for x in (obs, f64(obs_next), obs + f64(noise)[None, :]):
        z1, z2, mu = actor_pass(w, x)
        m = min(m, float(np.abs(z1).min()), float(np.abs(z2).min()))
    _, _, mu = actor_pass(w, obs)
    c1, c2, _, _ = q1_and_dqda(q, obs, np.clip(mu, -max_action, max_action))
    return min(m, float(np.abs(c1).min()), float(np.abs(c2).min())), np.abs(c1).min(0)


def clamp_shares(w, obs, obs_next, max_action):
    """Per input (obs, obs_next): (share of components with |pi| > max_action, the smallest distance of a |pi| from max_action)."""
    out = []
    for x in (obs, obs_next):
        mu = actor_pass([f64(t) for t in w], f64(x))[2]
        out.append((float((np.abs(mu) > max_action).mean()), float(np.abs(np.abs(mu) - max_action).min())))
    return out


def soft_update_f32(param, target, tau):
    """qr_soft_update's rule in float32, every operation rounded on its own: fl(fl(tau32 p) + fl(omt32 t))."""
    tau32, omt32 = np.float32(tau), np.float32(1.0 - float(tau))
    p, t = np.asarray(param, dtype=np.float32), np.asarray(target, dtype=np.float32)
    return (tau32 * p).astype(np.float32) + (omt32 * t).astype(np.float32)
