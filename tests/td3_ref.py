"""Float64 NumPy restatement of the TD3 critic half (qr_twinq_target, qr_twinq_grad; include/quadrotor_hip.h) with hand-derived
gradients, and the loader of tests/golden/td3_critic.npz (tools/gen_golden_td3_critic.py).  No torch, no GPU."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "td3_critic.npz")
NAMES = tuple(f"fc{k}_{x}" for k in range(1, 7) for x in "wb")
ACTOR_NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")
MARGIN = 2e-5   # every pre-activation of the gradient pass keeps this distance from ReLU's kink


def load():
    return np.load(GOLDEN, allow_pickle=False)


def case(g, name: str) -> dict:
    """One case as a dict: its own arrays, and its base case's for whatever it shares (key `base`).  critic = the twelve float32
    tensors c_<name>; target critic t_<name> (absent: the critic's own, as right after TD3's deepcopy); actor a_<name> (absent in
    w28, where a_next is an input)."""
    names = [str(n) for n in g["cases"]]
    assert name in names
    base = str(g[f"{name}_base"]) if f"{name}_base" in g.files else None
    out = {}
    for prefix in ([base] if base else []) + [name]:
        for k in g.files:
            if k.startswith(prefix + "_") and not any(k.startswith(o + "_") for o in names if len(o) > len(prefix) and o.startswith(prefix)):
                out[k[len(prefix) + 1:]] = g[k]
    out.pop("base", None)
    if "t_fc1_w" not in out:
        for n in NAMES:
            out["t_" + n] = out["c_" + n]
    if int(out["has_eps"]) == 0:
        out.pop("eps", None)
    return out


def relu(x):
    return np.maximum(x, 0.0)


def actor_forward(w, obs):
    """MLP_Actor_TD3: tanh(fc3(relu(fc2(relu(fc1(obs))))))."""
    h = relu(obs @ w[0].T + w[1])
    h = relu(h @ w[2].T + w[3])
    return np.tanh(h @ w[4].T + w[5])


def q_forward(w, sa):
    """One Q network: (z1, z2, q [B])."""
    z1 = sa @ w[0].T + w[1]
    z2 = relu(z1) @ w[2].T + w[3]
    return z1, z2, (relu(z2) @ w[4].T + w[5])[:, 0]


def td3_target_f64(c: dict, index=None, eps="own", a_next=None):
    """(a_next [B, A], y [B]) of td3.py:139-154 in float64.  eps: "own" (the case's, None when absent), an array, or None."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    idx = np.arange(len(c["obs_next"])) if index is None else np.asarray(index)
    on, r, d = f(c["obs_next"])[idx], f(c["reward"])[idx], f(c["done"])[idx]
    if eps == "own" if isinstance(eps, str) else False:
        eps = c.get("eps")
    ma, nc, tn = float(c["max_action"]), float(c["noise_clip"]), float(c["target_noise"])
    if a_next is None and "a_fc1_w" in c:
        a = actor_forward([f(c["a_" + n]) for n in ACTOR_NAMES], on)
        noise = np.clip(tn * f(eps), -nc, nc) if eps is not None else 0.0
        a_next = np.clip(a + noise, -ma, ma)
    elif a_next is None:
        a_next = f(c["a_next_in"])
    sa = np.concatenate([on, f(a_next)], axis=1)
    t = [f(c["t_" + n]) for n in NAMES]
    q = np.minimum(q_forward(t[:6], sa)[2], q_forward(t[6:], sa)[2])
    return a_next, r + float(c["discount"]) * (1.0 - d) * q


def twinq_grad_f64(w, obs, action, y):
    """loss, mse1, mse2 and the twelve gradients of mean (Q1 - y)^2 + mean (Q2 - y)^2, derived by hand; float64."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    sa, y = np.concatenate([f(obs), f(action)], axis=1), f(y)
    B = len(y)
    grads, mses = [], []
    for net in (w[:6], w[6:]):
        w1, b1, w2, b2, w3, b3 = (f(t) for t in net)
        z1, z2, q = q_forward((w1, b1, w2, b2, w3, b3), sa)
        t1, t2 = relu(z1), relu(z2)
        e = q - y
        mses.append(float(np.mean(e * e)))
        gq = (2.0 / B) * e                       # dLoss / dq
        dz2 = (gq[:, None] * w3) * (z2 > 0)      # [B, H]
        dz1 = (dz2 @ w2) * (z1 > 0)
        grads += [dz1.T @ sa, dz1.sum(0), dz2.T @ t1, dz2.sum(0), (gq @ t2)[None, :], np.array([gq.sum()])]
    return mses[0] + mses[1], mses[0], mses[1], dict(zip(NAMES, grads))


def margin(w, obs, action) -> float:
    """The smallest |pre-activation| of the four gradient-pass layers (z1 and z2 of Q1 and Q2) over all rows, float64."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    sa = np.concatenate([f(obs), f(action)], axis=1)
    m = np.inf
    for net in (w[:6], w[6:]):
        z1, z2, _ = q_forward([f(t) for t in net], sa)
        m = min(m, float(np.abs(z1).min()), float(np.abs(z2).min()))
    return m
