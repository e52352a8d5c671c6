"""Float64 NumPy restatement of SAC's actor loss (qr_sac_actor_grad; include/quadrotor_hip.h) with hand-derived gradients, as the
reference writes it (algos/sac/sac.py:182-211, the non-CTDE branch without the spectral-norm term, algos/policy_regularization.py with
rl_algo == "SAC", MLP_Actor_SAC.sample with supplied draws), the loader of tests/golden/sac_actor.npz (tools/gen_golden_sac_actor.py)
and the margins the fixture's seeds were searched for.  No torch, no GPU."""
import os

import numpy as np

from sac_ref import ACTOR_NAMES, EPSILON, LOG_SIG_MAX, LOG_SIG_MIN, tanh64
from td3_actor_ref import MARGIN, ROWS, f64, q1_and_dqda, relu
from td3_ref import NAMES as CRITIC_NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sac_actor.npz")
CASES = ("mono", "dtde0", "dtde1", "h64", "h5", "noreg", "noeps", "alpha0", "clamp", "sat")
STATS = ("loss", "q_mean", "logp_mean", "reg", "ls_share", "q2_share")
EPS = ("eps", "eps_reg", "eps_next", "eps_pert")   # the order the reference draws them in: loss, reg, next, pert
SATURATED = ("clamp", "sat")                        # the cases whose float64 sides differ by more than rounding (tanh: libm)


def load():
    return np.load(GOLDEN, allow_pickle=False)


def case(g, name: str) -> dict:
    """One case as a dict: actor a_<name> (eight float32 tensors), critic c_<name> (twelve), obs, obs_next, the four eps (absent in
    `noeps`), noise, nominal, lam, max_action, alpha, target_entropy, and in float64 the stats, alpha_grad and gradients g_<name>."""
    assert name in [str(n) for n in g["cases"]]
    out = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
    out["lam"] = tuple(float(v) for v in out["coeffs"][:3])
    out["max_action"], out["alpha"], out["target_entropy"] = (float(v) for v in out["coeffs"][3:6])
    return out


def inputs(c: dict, index=None):
    """(w, q, obs, obs_next, eps4, kw) of a case for sac_actor_grad_f64; eps by minibatch position, rows by index."""
    w, q = [c["a_" + n] for n in ACTOR_NAMES], [c["c_" + n] for n in CRITIC_NAMES]
    idx = np.arange(len(c["obs"])) if index is None else np.asarray(index)
    eps = [c[k][:len(idx)] if k in c else None for k in EPS]
    kw = dict(noise=c["noise"], nominal=c["nominal"], lam=c["lam"], max_action=c["max_action"], alpha=c["alpha"], target_entropy=c["target_entropy"])
    return w, q, c["obs"][idx], c["obs_next"][idx], eps, kw


def sample_pass(w, x, eps):
    """MLP_Actor_SAC.sample forwards with rsample's draw supplied; everything the backward pass needs."""
    z1 = x @ w[0].T + w[1]
    z2 = relu(z1) @ w[2].T + w[3]
    h2 = relu(z2)
    mean, lsr = h2 @ w[4].T + w[5], h2 @ w[6].T + w[7]
    ls = np.clip(lsr, LOG_SIG_MIN, LOG_SIG_MAX)
    e = np.zeros_like(mean) if eps is None else f64(eps)
    se = np.exp(ls) * e
    u = mean + se
    a = tanh64(u)
    logp = (-0.5 * e * e - ls - np.log(np.sqrt(2 * np.pi)) - np.log((1 - a * a) + EPSILON)).sum(1)
    return dict(x=x, z1=z1, z2=z2, mean=mean, lsr=lsr, se=se, u=u, a=a, logp=logp, gate=(lsr >= LOG_SIG_MIN) & (lsr <= LOG_SIG_MAX))


def backward(w, p, ga, gl):
    """The eight gradients of sum(ga * a) + sum(gl * logp) for one pass; ga [B, A], gl a scalar."""
    om = 1.0 - p["a"] ** 2
    du = ga * om + gl * (2.0 * p["a"] * om / (om + EPSILON))
    dls = (du * p["se"] - gl) * p["gate"]
    h1, h2 = relu(p["z1"]), relu(p["z2"])
    dz2 = (du @ w[4] + dls @ w[6]) * (p["z2"] > 0)
    dz1 = (dz2 @ w[2]) * (p["z1"] > 0)
    return [dz1.T @ p["x"], dz1.sum(0), dz2.T @ h1, dz2.sum(0), du.T @ h2, du.sum(0), dls.T @ h2, dls.sum(0)]


def sac_actor_grad_f64(w, q, obs, obs_next, eps4, *, noise, nominal, lam, max_action, alpha, target_entropy, detail=False):
    """(stats [6], grads {name: array}, alpha_grad) of the SAC actor loss, derived by hand; float64.  w: the actor's eight tensors, q:
    the twin critic's twelve, eps4: the four draws (None: zeros).  detail: also the four passes and both critics' (z1, z2, Q)."""
    w, q, obs = [f64(t) for t in w], [f64(t) for t in q], f64(obs)
    B, A = obs.shape[0], w[4].shape[0]
    lam_T, lam_S, lam_M = lam
    clip = lambda m: np.clip(m, -max_action, max_action)
    inside = lambda m: np.abs(m) <= max_action
    p0 = sample_pass(w, obs, eps4[0])
    c1 = q1_and_dqda(q[:6], obs, p0["a"])
    c2 = q1_and_dqda(q[6:], obs, p0["a"])
    w2 = np.where(c2[2] < c1[2], 1.0, np.where(c2[2] == c1[2], 0.5, 0.0))[:, None]
    qmin = np.minimum(c1[2], c2[2])
    grads = backward(w, p0, -((1.0 - w2) * c1[3] + w2 * c2[3]) / B, alpha / B)
    reg, passes = 0.0, [p0]
    if lam_T != 0 or lam_S != 0 or lam_M != 0:
        pr = sample_pass(w, obs, eps4[1])
        passes.append(pr)
        r, gr = clip(pr["a"]), 0.0
        others = []
        if lam_S != 0:
            others.append((obs + f64(noise)[None, :], eps4[3], lam_S))
        if lam_T != 0:
            others.append((f64(obs_next), eps4[2], lam_T))
        for y, e, lam_y in others:
            po = sample_pass(w, y, e)
            passes.append(po)
            d = r - clip(po["a"])
            reg += lam_y * float(np.mean(d * d))
            c = 2.0 * lam_y / (B * A)
            gr = gr + c * d
            for gsum, gone in zip(grads, backward(w, po, -c * d * inside(po["a"]), 0.0)):
                gsum += gone
        if lam_M != 0:
            d = r - f64(nominal)[None, :]
            reg += lam_M * float(np.mean(d * d))
            gr = gr + (2.0 * lam_M / (B * A)) * d
        for gsum, gone in zip(grads, backward(w, pr, gr * inside(pr["a"]), 0.0)):
            gsum += gone
    lp = float(p0["logp"].mean())
    stats = np.array([alpha * lp - qmin.mean() + reg, qmin.mean(), lp, reg, float((~p0["gate"]).sum()) / (B * A),
                      float((c2[2] < c1[2]).sum()) / B])
    out = (stats, dict(zip(ACTOR_NAMES, grads)), -(target_entropy + lp))
    return out + (passes, (c1, c2)) if detail else out


def margins(w, q, obs, obs_next, eps4, *, noise, nominal, lam, max_action, alpha, target_entropy):
    """What the fixture's seeds were searched for, each the smallest over all rows and all passes that run, float64: relu (every
    ReLU pre-activation of the actor and of both critics), ls (raw log_std from -20 and from 2), clamp (|a| from max_action in the
    reg passes; inf where no reg pass runs, and where max_action >= 1: |tanh| cannot exceed it and torch.clamp passes the gradient at
    the bound, so the clamp has no kink to keep away from), q (|Q1 - Q2|)."""
    _, _, _, passes, (c1, c2) = sac_actor_grad_f64(w, q, obs, obs_next, eps4, noise=noise, nominal=nominal, lam=lam, max_action=max_action,
                                                   alpha=alpha, target_entropy=target_entropy, detail=True)
    m = {"relu": min(float(np.abs(z).min()) for c in (c1, c2) for z in c[:2]), "ls": np.inf, "clamp": np.inf,
         "q": float(np.abs(c1[2] - c2[2]).min())}
    for k, p in enumerate(passes):
        m["relu"] = min(m["relu"], float(np.abs(p["z1"]).min()), float(np.abs(p["z2"]).min()))
        m["ls"] = min(m["ls"], float(np.abs(p["lsr"] - LOG_SIG_MIN).min()), float(np.abs(p["lsr"] - LOG_SIG_MAX).min()))
        if k > 0 and max_action < 1.0:
            m["clamp"] = min(m["clamp"], float(np.abs(np.abs(p["a"]) - max_action).min()))
    return m
