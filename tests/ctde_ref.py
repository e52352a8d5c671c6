"""Float64 NumPy restatement of the centralized-critic (CTDE) half of TD3 and SAC for two agents (qr_ctde_twinq_target,
qr_ctde_sac_target, qr_ctde_twinq_grad; include/quadrotor_hip.h) on tests/td3_ref.py's and tests/sac_ref.py's pieces, and the loader
of tests/golden/ctde_critic.npz (tools/gen_golden_ctde_critic.py).  No torch, no GPU."""
import os

import numpy as np

import sac_ref
import td3_ref
from td3_ref import NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ctde_critic.npz")
TD3_ACTOR = td3_ref.ACTOR_NAMES
SAC_ACTOR = sac_ref.ACTOR_NAMES
CASES = ("ctde", "h64", "h5", "w28", "sat", "clamp", "noeps", "twodraw", "onedraw")
f = lambda x: np.asarray(x, dtype=np.float64)


def load():
    return np.load(GOLDEN, allow_pickle=False)


def case(g, name: str) -> dict:
    """One case as a dict: its base case's arrays (key `base`) under its own.  c_* the critic, t_* its target, p{m}_* the TD3 target
    actors, s{m}_* the SAC actors (absent in w28: an_in0, an_in1, logp_in are inputs); eps{m} absent where has_eps = 0, elp{m} where
    has_elp = 0; the base's outputs are dropped."""
    base = str(g[f"{name}_base"]) if f"{name}_base" in g.files else None
    out = {}
    if base:
        out = {k[len(base) + 1:]: g[k] for k in g.files if k.startswith(base + "_")}
        out = {k: v for k, v in out.items() if not k.startswith(("td3_", "sac_", "g0_", "g1_"))}
    out.update({k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")})
    out.pop("base", None)
    if int(out["has_eps"]) == 0:
        out.pop("eps0", None), out.pop("eps1", None)
    if int(out["has_elp"]) == 0:
        out.pop("elp0", None), out.pop("elp1", None)
    return out


def rows(c: dict, which: str, index=None):
    """[x0 | x1] of obs / obsn / act in float64, gathered."""
    idx = np.arange(len(c["obs0"])) if index is None else np.asarray(index)
    return np.concatenate([f(c[which + "0"])[idx], f(c[which + "1"])[idx]], axis=1)


def _bellman(c, k, idx, sa, extra=0.0):
    t = [f(c["t_" + n]) for n in NAMES]
    q = np.minimum(td3_ref.q_forward(t[:6], sa)[2], td3_ref.q_forward(t[6:], sa)[2]) - extra
    return f(c["rwd"])[idx, k] + float(c["discount"]) * (1.0 - f(c["done"])[idx, k]) * q


def td3_target_f64(c: dict, k: int, index=None, eps="own"):
    """(a'_0, a'_1, y) of td3.py:124-154, the CTDE branch.  eps: "own" (the case's; none where absent), a pair of [B, A_m] arrays by
    minibatch position, or None."""
    idx = np.arange(len(c["obs0"])) if index is None else np.asarray(index)
    if isinstance(eps, str):
        eps = [c["eps0"][:len(idx)], c["eps1"][:len(idx)]] if "eps0" in c else None
    ma, nc, tn = float(c["max_action"]), float(c["noise_clip"]), float(c["target_noise"])
    a = []
    for m in (0, 1):
        if "p0_fc1_w" in c:
            mean = td3_ref.actor_forward([f(c[f"p{m}_{n}"]) for n in TD3_ACTOR], f(c[f"obsn{m}"])[idx])
            noise = np.clip(tn * f(eps[m]), -nc, nc) if eps is not None and eps[m] is not None else 0.0
            a.append(np.clip(mean + noise, -ma, ma))
        else:
            a.append(f(c[f"an_in{m}"])[:len(idx)])
    sa = np.concatenate([rows(c, "obsn", idx)] + a, axis=1)
    return a[0], a[1], _bellman(c, k, idx, sa)


def sac_target_f64(c: dict, k: int, index=None, eps="own", elp="own", alpha=None):
    """(a'_0, a'_1, logp, y) of sac.py:136-153, the CTDE branch: agent k sampled a second time for logp with the draw elp ([B, A_k];
    "own": the case's elp{k}, eps[k] where absent; None: eps[k])."""
    idx = np.arange(len(c["obs0"])) if index is None else np.asarray(index)
    if isinstance(eps, str):
        eps = [c["eps0"][:len(idx)], c["eps1"][:len(idx)]] if "eps0" in c else None
    if isinstance(elp, str):
        elp = c[f"elp{k}"][:len(idx)] if f"elp{k}" in c else None
    alpha = float(c["alpha"]) if alpha is None else alpha
    if "s0_fc1_w" in c:
        a, heads = [], []
        for m in (0, 1):
            mean, ls = sac_ref.actor_heads([f(c[f"s{m}_{n}"]) for n in SAC_ACTOR], f(c[f"obsn{m}"])[idx])
            e = np.zeros_like(mean) if eps is None or eps[m] is None else f(eps[m])
            heads.append((mean, ls, e))
            a.append(sac_ref.sample(mean, ls, e)[0])
        mean, ls, e = heads[k]
        logp = sac_ref.sample(mean, ls, e if elp is None else f(elp))[1]
    else:
        a, logp = [f(c[f"an_in{m}"])[:len(idx)] for m in (0, 1)], f(c["logp_in"])[:len(idx)]
    sa = np.concatenate([rows(c, "obsn", idx)] + a, axis=1)
    return a[0], a[1], logp, _bellman(c, k, idx, sa, alpha * logp)


def raw_log_std(c: dict, m: int):
    """Agent m's log_std head before the clamp, on all rows."""
    w = [f(c[f"s{m}_{n}"]) for n in SAC_ACTOR]
    h = td3_ref.relu(td3_ref.relu(f(c[f"obsn{m}"]) @ w[0].T + w[1]) @ w[2].T + w[3])
    return h @ w[6].T + w[7]


def twinq_grad_f64(c: dict, y, index=None):
    """loss, mse1, mse2 and the twelve gradients of the regression of the centralized critic c_* against y (td3_ref.twinq_grad_f64 on
    the concatenated rows)."""
    return td3_ref.twinq_grad_f64([c["c_" + n] for n in NAMES], rows(c, "obs", index), rows(c, "act", index), y)


def margin(c: dict) -> float:
    return td3_ref.margin([c["c_" + n] for n in NAMES], rows(c, "obs"), rows(c, "act"))
