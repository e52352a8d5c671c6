"""Float64 NumPy restatement of SAC's soft target values (qr_sac_target; include/quadrotor_hip.h) as the reference writes them
(algos/sac/sac.py:135-153 with MLP_Actor_SAC.sample, algos/sac/sac_mlp.py:55-79, the sample restated with a supplied eps), and the
loader of tests/golden/sac_critic.npz (tools/gen_golden_sac_critic.py).  The twin-Q regression and its gradients are td3_ref's.  No
torch, no GPU."""
import os

import numpy as np

from td3_ref import NAMES, q_forward, relu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sac_critic.npz")
ACTOR_NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std_w", "log_std_b")
LOG_SIG_MIN, LOG_SIG_MAX, EPSILON = -20.0, 2.0, 1e-6


def load():
    return np.load(GOLDEN, allow_pickle=False)


def case(g, name: str) -> dict:
    """One case as a dict: its own arrays, and its base case's for whatever it shares (key `base`).  Target critic = the twelve
    float32 tensors t_<name>; the live critic c_<name> (only in the cases the end-to-end test runs); actor a_<name> (absent in w28,
    where a_next_in and logp_next_in are inputs); eps absent where has_eps = 0."""
    names = [str(n) for n in g["cases"]]
    assert name in names
    base = str(g[f"{name}_base"]) if f"{name}_base" in g.files else None
    out = {}
    for prefix in ([base] if base else []) + [name]:
        for k in g.files:
            if k.startswith(prefix + "_"):
                out[k[len(prefix) + 1:]] = g[k]
    out.pop("base", None)
    if int(out["has_eps"]) == 0:
        out.pop("eps", None)
    return out


def tanh64(u):
    """tanh in float64 as tools/gen_golden_sac_critic.py forms it: evaluated in long double and rounded once.  log(1 - a'^2 + 1e-6)
    multiplies one ulp of a' by 2e6 on a saturated component, and float64 tanh differs by an ulp from library to library (NumPy's
    against torch's: 2.2e-10 in logp), so both sides use this one, the correctly rounded value."""
    return np.tanh(np.asarray(u, dtype=np.longdouble)).astype(np.float64)


def actor_heads(w, obs):
    """MLP_Actor_SAC.forward: (mean, log_std clamped into [-20, 2])."""
    h = relu(obs @ w[0].T + w[1])
    h = relu(h @ w[2].T + w[3])
    return h @ w[4].T + w[5], np.clip(h @ w[6].T + w[7], LOG_SIG_MIN, LOG_SIG_MAX)


def sample(mean, log_std, eps):
    """MLP_Actor_SAC.sample with rsample's draw supplied: (a' [B, A], logp [B], u [B, A])."""
    std = np.exp(log_std)
    u = mean + std * eps
    a = tanh64(u)
    logp = -((u - mean) ** 2) / (2 * std ** 2) - log_std - np.log(np.sqrt(2 * np.pi))    # Normal(mean, std).log_prob(u)
    logp = logp - np.log((1 - a ** 2) + EPSILON)
    return a, logp.sum(1), u


def sac_target_f64(c: dict, index=None, eps="own", a_next=None, logp_next=None, alpha=None):
    """(a' [B, A], logp [B], y [B]) of sac.py:146-153 in float64.  eps: "own" (the case's, zeros when absent), an array [B, A] by
    minibatch position, or None: zeros."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    idx = np.arange(len(c["obs_next"])) if index is None else np.asarray(index)
    on, r, d = f(c["obs_next"])[idx], f(c["reward"])[idx], f(c["done"])[idx]
    if isinstance(eps, str):
        eps = c.get("eps")
        eps = None if eps is None else eps[:len(idx)]
    if a_next is None and "a_fc1_w" in c:
        mean, ls = actor_heads([f(c["a_" + n]) for n in ACTOR_NAMES], on)
        a_next, logp_next, _ = sample(mean, ls, np.zeros_like(mean) if eps is None else f(eps))
    elif a_next is None:
        a_next, logp_next = f(c["a_next_in"])[:len(idx)], f(c["logp_next_in"])[:len(idx)]
    sa = np.concatenate([on, f(a_next)], axis=1)
    t = [f(c["t_" + n]) for n in NAMES]
    q = np.minimum(q_forward(t[:6], sa)[2], q_forward(t[6:], sa)[2]) - (float(c["alpha"]) if alpha is None else alpha) * f(logp_next)
    return f(a_next), f(logp_next), r + float(c["discount"]) * (1.0 - d) * q
