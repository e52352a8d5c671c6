"""Float64 NumPy restatement of agent k's SAC actor half under the centralized (CTDE) twin critic of two agents
(qr_ctde_sac_actor_grad; include/quadrotor_hip.h) with hand-derived gradients, built on tests/sac_actor_ref.py's pieces, the loader of
tests/golden/sac_ctde_actor.npz (tools/gen_golden_sac_ctde_actor.py) and the margins the fixture's seeds were searched for.
No torch, no GPU."""
import os

import numpy as np

from sac_actor_ref import ACTOR_NAMES, CRITIC_NAMES, MARGIN, ROWS, STATS, backward, sample_pass  # noqa: F401
from sac_ref import LOG_SIG_MAX, LOG_SIG_MIN
from td3_actor_ref import f64, q1_and_dqda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sac_ctde_actor.npz")
# sat0 / sat1: the issue's `sat`, k = 0 and k = 1 on one set of networks and rows
CASES = ("k0", "k1", "h64", "h5", "noreg", "noeps", "onedraw", "alpha0", "clamp", "sat0", "sat1", "w28")
SUPPLIED = ("w28",)                          # the other agent's action is given, its actor is not
SATURATED = ("clamp", "sat0", "sat1")        # the cases whose float64 sides differ by more than rounding (tanh, exp: libm against torch)
# the draws in the order the reference makes them (sac.py:177-180, then policy_regularization): agent 0, agent 1, logp, reg, next, pert
EPS = ("eps0", "eps1", "eps_logp", "eps_reg", "eps_next", "eps_pert")


def load():
    return np.load(GOLDEN, allow_pickle=False)


def case(g, name: str) -> dict:
    """One case as a dict: k, obs0, obs1, obs_next0, obs_next1, a0_* / a1_* (the actors that exist, eight float32 tensors each), c_*
    (the twin critic's twelve), the draws that exist (EPS), action_other (supplied form), noise, nominal, lam, max_action, alpha,
    target_entropy and the reference's float64 stats, alpha_grad, g_* and other_action (what the critics read for agent 1 - k).
    Networks and rows are the case's own or, where the key `shared` names another case, that case's."""
    assert name in [str(n) for n in g["cases"]]
    out = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
    if "shared" in out:
        owner = str(out.pop("shared"))
        for k in g.files:
            if k.startswith(owner + "_") and k[len(owner) + 1:].split("_")[0] in ("a0", "a1", "c", "obs0", "obs1", "obs") and k[len(owner) + 1:] not in out:
                out[k[len(owner) + 1:]] = g[k]
    out["k"] = int(out["k"])
    out["lam"] = tuple(float(v) for v in out["coeffs"][:3])
    out["max_action"], out["alpha"], out["target_entropy"] = (float(v) for v in out["coeffs"][3:6])
    return out


def actor_of(c, m):
    """Agent m's eight tensors, or None where the case has none (the supplied form)."""
    return [c[f"a{m}_{n}"] for n in ACTOR_NAMES] if f"a{m}_fc1_w" in c else None


def critic_of(c):
    return [c["c_" + n] for n in CRITIC_NAMES]


def other_action(actors, obs, k, action_other, eps_other):
    """The other agent's action as the critics read it, float64: supplied as it is, or tanh of its actor's sample (no clamp)."""
    if action_other is not None:
        return f64(action_other)
    return sample_pass([f64(t) for t in actors[1 - k]], f64(obs[1 - k]), eps_other)["a"]


def _dqda_own(q6, obs, a_own, a_other, k):
    """(z1, z2, Q, dQ/da_k) of one critic on [obs_0 | obs_1 | a_0 | a_1]."""
    acts = [a_own, a_other] if k == 0 else [a_other, a_own]
    z1, z2, val, dqda = q1_and_dqda(q6, np.concatenate([f64(obs[0]), f64(obs[1])], axis=1), np.concatenate(acts, axis=1))
    off = 0 if k == 0 else a_other.shape[1]
    return z1, z2, val, dqda[:, off:off + a_own.shape[1]]   # the other agent's columns carry a value only


def ctde_sac_actor_grad_f64(actors, q, obs, obs_next_k, k, action_other, eps, *, noise, nominal, lam, max_action, alpha, target_entropy,
                            detail=False):
    """(stats [6], grads {name: array}, alpha_grad) of agent k's loss, derived by hand; float64.  actors: the pair of eight-tensor lists
    (the other's None with action_other [B, A_other], by row); q: the twin critic's twelve; obs: the pair of [B, D_m] rows; obs_next_k,
    noise, nominal: agent k's; eps: dict over "eps", "eps_other", "eps_logp", "eps_reg", "eps_next", "eps_pert" (absent or None: zeros;
    eps_logp absent: ONE sample).  detail: also agent k's passes (the loss pass first), both critics' (z1, z2, Q) and the other's pass."""
    w, q = [f64(t) for t in actors[k]], [f64(t) for t in q]
    x = f64(obs[k])
    B, A = x.shape[0], w[4].shape[0]
    lam_T, lam_S, lam_M = lam
    clip = lambda m: np.clip(m, -max_action, max_action)
    inside = lambda m: np.abs(m) <= max_action
    e = lambda n: eps.get(n)
    p0 = sample_pass(w, x, e("eps"))
    ao = other_action(actors, obs, k, action_other, e("eps_other"))
    c1 = _dqda_own(q[:6], obs, p0["a"], ao, k)
    c2 = _dqda_own(q[6:], obs, p0["a"], ao, k)
    w2 = np.where(c2[2] < c1[2], 1.0, np.where(c2[2] == c1[2], 0.5, 0.0))[:, None]
    qmin = np.minimum(c1[2], c2[2])
    ga = -((1.0 - w2) * c1[3] + w2 * c2[3]) / B
    passes = [p0]
    if e("eps_logp") is None:
        plog = p0
        grads = backward(w, p0, ga, alpha / B)
    else:   # the second sample: the same forward pass, another draw; it carries the entropy term alone
        plog = sample_pass(w, x, e("eps_logp"))
        passes.append(plog)
        grads = backward(w, p0, ga, 0.0)
        for gsum, gone in zip(grads, backward(w, plog, np.zeros_like(ga), alpha / B)):
            gsum += gone
    reg = 0.0
    if lam_T != 0 or lam_S != 0 or lam_M != 0:
        pr = sample_pass(w, x, e("eps_reg"))
        passes.append(pr)
        r, gr = clip(pr["a"]), 0.0
        others = []
        if lam_S != 0:
            others.append((x + f64(noise)[None, :], e("eps_pert"), lam_S))
        if lam_T != 0:
            others.append((f64(obs_next_k), e("eps_next"), lam_T))
        for y, ey, lam_y in others:
            po = sample_pass(w, y, ey)
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
    lp = float(plog["logp"].mean())
    stats = np.array([alpha * lp - qmin.mean() + reg, qmin.mean(), lp, reg, float((~p0["gate"]).sum()) / (B * A),
                      float((c2[2] < c1[2]).sum()) / B])
    out = (stats, dict(zip(ACTOR_NAMES, grads)), -(target_entropy + lp))
    if not detail:
        return out
    pother = None if action_other is not None else sample_pass([f64(t) for t in actors[1 - k]], f64(obs[1 - k]), e("eps_other"))
    return out + (passes, (c1, c2), pother)


def margins(actors, q, obs, obs_next_k, k, action_other, eps, **kw):
    """What the fixture's seeds were searched for, each the smallest over all rows and all passes that run, float64: relu (every ReLU
    pre-activation of agent k's passes, of the other agent's pass and of both critics), ls (raw log_std of either agent from -20 and
    from 2), clamp (|a| from max_action in agent k's reg passes; inf where none runs and where max_action >= 1, as
    tests/sac_actor_ref.py says), q (|Q1 - Q2|)."""
    _, _, _, passes, (c1, c2), pother = ctde_sac_actor_grad_f64(actors, q, obs, obs_next_k, k, action_other, eps, detail=True, **kw)
    m = {"relu": min(float(np.abs(z).min()) for c in (c1, c2) for z in c[:2]), "ls": np.inf, "clamp": np.inf,
         "q": float(np.abs(c1[2] - c2[2]).min())}
    n_loss = 1 if eps.get("eps_logp") is None else 2
    for j, p in enumerate(passes + ([] if pother is None else [pother])):
        m["relu"] = min(m["relu"], float(np.abs(p["z1"]).min()), float(np.abs(p["z2"]).min()))
        m["ls"] = min(m["ls"], float(np.abs(p["lsr"] - LOG_SIG_MIN).min()), float(np.abs(p["lsr"] - LOG_SIG_MAX).min()))
        if n_loss <= j < len(passes) and kw["max_action"] < 1.0:
            m["clamp"] = min(m["clamp"], float(np.abs(np.abs(p["a"]) - kw["max_action"]).min()))
    return m


def case_eps(c, idx=None):
    """The draws of a fixture case by minibatch position, under ctde_sac_actor_grad_f64's names."""
    n = ROWS if idx is None else len(idx)
    k = c["k"]
    names = {"eps": f"eps{k}", "eps_other": f"eps{1 - k}", "eps_logp": "eps_logp", "eps_reg": "eps_reg", "eps_next": "eps_next", "eps_pert": "eps_pert"}
    return {a: c[b][:n] for a, b in names.items() if b in c}


def case_args(c, idx=None, lam=None):
    """(positional arguments, keywords) of ctde_sac_actor_grad_f64 / margins for rows idx of a fixture case (all rows; the draws and
    `action_other` are by minibatch position)."""
    idx = np.arange(ROWS) if idx is None else np.asarray(idx)
    k = c["k"]
    ao = c["action_other"][:len(idx)] if "action_other" in c else None
    kw = dict(noise=c["noise"], nominal=c["nominal"], lam=c["lam"] if lam is None else lam, max_action=c["max_action"], alpha=c["alpha"],
              target_entropy=c["target_entropy"])
    return ([actor_of(c, 0), actor_of(c, 1)], critic_of(c), (c["obs0"][idx], c["obs1"][idx]), c[f"obs_next{k}"][idx], k, ao, case_eps(c, idx)), kw


def case_f64(c, idx=None, lam=None, **over):
    a, kw = case_args(c, idx, lam)
    kw.update(over)
    return ctde_sac_actor_grad_f64(*a, **kw)
