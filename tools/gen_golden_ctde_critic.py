#!/usr/bin/env python
"""Generate tests/golden/ctde_critic.npz by RUNNING THE REFERENCE's modules (fdcl-gwu/gym-rotor: MLP_Actor_TD3 and MLP_Critic_CTDE,
algos/td3/td3_mlp.py; MLP_Actor_SAC, algos/sac/sac_mlp.py) in float64 autograd on the CPU with the centralized-critic (CTDE) branches
of TD3.train (algos/td3/td3.py:124-137, 151-161) and SAC.train (algos/sac/sac.py:136-144, 152-160), like tools/gen_golden_td3_critic.py.

    python tools/gen_golden_ctde_critic.py <path of the reference checkout>

Two agents, per case 130 transitions: obs0/1, obsn0/1 and act0/1 uniform in [-1, 1], rwd [130, 2] ~ N(0, 1), done [130, 2] ~
Bernoulli(0.1), the draws eps0/1 [130, A_m] (TD3's smoothing noise and SAC's rsample alike) and elp0/1 [130, A_m], SAC's second draw
of agent k for the log-probability (sac.py:141); the float32 weights of the centralized critic (c_*), its target (t_*), both TD3
target actors (p0_*, p1_*) and both SAC actors (s0_*, s1_*); the scalars.  MLP_Actor_SAC.sample draws its own noise, so its lines are
restated with a SUPPLIED draw, as tools/gen_golden_sac_critic.py does (tanh in long double, rounded once).  In float64, all 130 rows
as one minibatch, for k = 0 and 1: td3_a0, td3_a1, td3_y{k}; sac_a0, sac_a1, sac_logp{k}, sac_y{k}; and, in the cases that carry
gradients, the regression against td3_y{k}: g{k}_loss, g{k}_mse1, g{k}_mse2, g{k}_<tensor>.  Arrays only.
Cases (obs 0 + obs 1 / action 0 + action 1 -> hidden):
  ctde 15+3 / 4+1 -> 62      h64, h5: the same widths -> 64, 5      w28 16+4 / 5+3 -> 20: no actors, a' (and logp) are inputs (the
  hidden width keeps the file within the size limit of a committed file)
  on h5's networks and rows (key `base`; they store what differs and no gradients):
  sat      TD3: the target actors' weights x 8, eps x 4, done ~ Bernoulli(0.3): both clamps active
  clamp    SAC: the log_std heads x 60: raw log_std outside [-20, 2]
  noeps    no draws at all (has_eps = 0)
  twodraw  another second draw, twice as wide        onedraw  no second draw (has_elp = 0): logp from eps[k]
Every case keeps every pre-activation of the gradient pass at |z| >= 2e-5 in float64: the seeds are tried in order until it does.
"""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
from torch.distributions import Normal

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if len(sys.argv) < 2:
    raise SystemExit(__doc__)
sys.path.insert(0, sys.argv[1])

from algos.sac.sac_mlp import MLP_Actor_SAC, epsilon  # noqa: E402
from algos.td3.td3_mlp import MLP_Actor_TD3, MLP_Critic_CTDE  # noqa: E402

ROWS, MARGIN = 130, 2e-5
SC = {"discount": 0.99, "target_noise": 0.2, "noise_clip": 0.5, "max_action": 1.0, "alpha": 0.2}
# name: (obs widths, action widths, critic hidden, actor hiddens or None, first seed)
CASES = {"ctde": ((15, 3), (4, 1), 62, (16, 4), 100), "h64": ((15, 3), (4, 1), 64, (16, 4), 200), "h5": ((15, 3), (4, 1), 5, (16, 4), 300),
         "w28": ((16, 4), (5, 3), 20, None, 400)}
NAMES = tuple(f"fc{k}_{x}" for k in range(1, 7) for x in "wb")
f64 = lambda x: torch.as_tensor(x).double()


def tanh64(x):
    return torch.from_numpy(np.tanh(x.numpy().astype(np.longdouble)).astype(np.float64))


def critic_tensors(net):
    return [t for k in range(1, 7) for t in (getattr(net, f"fc{k}").weight, getattr(net, f"fc{k}").bias)]


def td3_actor_tensors(net):
    return [t for l in (net.fc1, net.fc2, net.fc3) for t in (l.weight, l.bias)]


def sac_actor_tensors(net):
    return [t for l in (net.fc1, net.fc2, net.mean_linear, net.log_std_linear) for t in (l.weight, l.bias)]


def sac_sample(actor, x, eps):
    """MLP_Actor_SAC.sample (sac_mlp.py:55-79) with rsample's draw supplied."""
    mean, log_std = actor.forward(x)
    std = log_std.exp()
    x_t = mean + std * (f64(eps) if eps is not None else torch.zeros_like(mean))
    action = tanh64(x_t)
    log_prob = Normal(mean, std).log_prob(x_t)
    log_prob -= torch.log((1 - action.pow(2)) + epsilon)
    return action, log_prob.sum(1, keepdim=True)


def run(m, d, eps, elp, grads):
    """Both train() branches in float64 for k = 0, 1.  m: float64 modules; eps / elp: pairs of draws or None."""
    out = {}
    obs, obsn, act = [f64(d[f"obs{i}"]) for i in (0, 1)], [f64(d[f"obsn{i}"]) for i in (0, 1)], [f64(d[f"act{i}"]) for i in (0, 1)]
    for k in (0, 1):
        rwd, done = f64(d["rwd"])[:, k:k + 1], f64(d["done"])[:, k:k + 1]
        with torch.no_grad():
            # td3.py:124-137, 151-154
            if m["p"] is not None:
                a_n = []
                for i in (0, 1):
                    a = m["p"][i](obsn[i])
                    noise = (f64(eps[i]) * SC["target_noise"]).clamp(-SC["noise_clip"], SC["noise_clip"]) if eps is not None else 0.0
                    a_n.append((a + noise).clamp(-SC["max_action"], SC["max_action"]))
            else:
                a_n = [f64(d["an_in0"]), f64(d["an_in1"])]
            q1, q2 = m["t"](obsn, a_n)
            y = rwd + SC["discount"] * (1 - done) * torch.min(q1, q2)
            out.update(td3_a0=a_n[0].numpy().copy(), td3_a1=a_n[1].numpy().copy())
            out[f"td3_y{k}"] = y[:, 0].numpy().copy()
            # sac.py:136-144, 152-153
            if m["s"] is not None:
                s_n = [sac_sample(m["s"][i], obsn[i], None if eps is None else eps[i])[0] for i in (0, 1)]
                own = None if eps is None else eps[k]
                _, logp = sac_sample(m["s"][k], obsn[k], own if elp is None else elp[k])
            else:
                s_n, logp = [f64(d["an_in0"]), f64(d["an_in1"])], f64(d["logp_in"])[:, None]
            q1, q2 = m["t"](obsn, s_n)
            ys = rwd + SC["discount"] * (1 - done) * (torch.min(q1, q2) - SC["alpha"] * logp)
            out.update(sac_a0=s_n[0].numpy().copy(), sac_a1=s_n[1].numpy().copy())
            out[f"sac_logp{k}"], out[f"sac_y{k}"] = logp[:, 0].numpy().copy(), ys[:, 0].numpy().copy()
        if grads:   # td3.py:157-167
            c1, c2 = m["c"](obs, act)
            m1, m2 = torch.nn.functional.mse_loss(c1, y), torch.nn.functional.mse_loss(c2, y)
            loss = m1 + m2
            m["c"].zero_grad()
            loss.backward()
            out.update({f"g{k}_loss": np.float64(loss.item()), f"g{k}_mse1": np.float64(m1.item()), f"g{k}_mse2": np.float64(m2.item())})
            for n, p in zip(NAMES, critic_tensors(m["c"])):
                out[f"g{k}_{n}"] = p.grad.numpy().copy()
    return out


def min_abs_z(c64, sa):
    with torch.no_grad():
        m = float("inf")
        for a, b in ((c64.fc1, c64.fc2), (c64.fc4, c64.fc5)):
            z1 = a(sa)
            z2 = b(torch.relu(z1))
            m = min(m, z1.abs().min().item(), z2.abs().min().item())
    return m


def build(spec, seed):
    od, ad, H, HA, _ = spec
    torch.manual_seed(seed)
    args = SimpleNamespace(obs_dim_n=list(od), action_dim_n=list(ad), critic_hidden_dim=H, actor_hidden_dim=list(HA) if HA else None)
    mods = {"c": MLP_Critic_CTDE(args), "t": MLP_Critic_CTDE(args),
            "p": [MLP_Actor_TD3(args, i) for i in (0, 1)] if HA else None, "s": [MLP_Actor_SAC(args, i) for i in (0, 1)] if HA else None}
    g = torch.Generator().manual_seed(10_000 + seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    d = {}
    for i in (0, 1):
        d[f"obs{i}"], d[f"obsn{i}"], d[f"act{i}"] = u(ROWS, od[i]), u(ROWS, od[i]), u(ROWS, ad[i])
    d["rwd"], d["done"] = torch.randn(ROWS, 2, generator=g), (torch.rand(ROWS, 2, generator=g) < 0.1).float()
    for i in (0, 1):
        d[f"eps{i}"], d[f"elp{i}"] = torch.randn(ROWS, ad[i], generator=g), torch.randn(ROWS, ad[i], generator=g)
    if not HA:
        d["an_in0"], d["an_in1"], d["logp_in"] = u(ROWS, ad[0]), u(ROWS, ad[1]), torch.randn(ROWS, generator=g)
    return mods, {k: v.numpy() for k, v in d.items()}


def to64(mods):
    return {k: (None if v is None else [copy.deepcopy(x).double() for x in v] if isinstance(v, list) else copy.deepcopy(v).double())
            for k, v in mods.items()}


def one_case(name, spec):
    seed = spec[4]
    while True:
        mods, d = build(spec, seed)
        m64 = to64(mods)
        sa = torch.cat([f64(d[k]) for k in ("obs0", "obs1", "act0", "act1")], 1)
        z = min_abs_z(m64["c"], sa)
        if z >= MARGIN:
            break
        seed += 1
    out = dict(d)
    out.update({k: np.float64(v) for k, v in SC.items()})
    out.update(seed=np.int64(seed), min_abs_z=np.float64(z), has_eps=np.int64(1), has_elp=np.int64(1), has_grads=np.int64(1),
               obs_dims=np.array(spec[0], dtype=np.int64), action_dims=np.array(spec[1], dtype=np.int64))
    for pre, key in (("c", "c"), ("t", "t")):
        for n, p in zip(NAMES, critic_tensors(mods[key])):
            out[f"{pre}_{n}"] = p.detach().numpy().copy()
    if mods["p"] is not None:
        for i in (0, 1):
            for n, p in zip(("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b"), td3_actor_tensors(mods["p"][i])):
                out[f"p{i}_{n}"] = p.detach().numpy().copy()
            for n, p in zip(("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std_w", "log_std_b"), sac_actor_tensors(mods["s"][i])):
                out[f"s{i}_{n}"] = p.detach().numpy().copy()
    eps, elp = [d["eps0"], d["eps1"]], [d["elp0"], d["elp1"]]
    out.update(run(m64, d, eps, elp, True))
    assert all(np.isfinite(np.asarray(a, dtype=np.float64)).all() for a in out.values())
    print(f"{name}: seed {seed}  min|z| {z:.3e}  loss0 {float(out['g0_loss']):.6f}  loss1 {float(out['g1_loss']):.6f}")
    return out, mods, d


def variant(name, mods, d, eps, elp, extra):
    res = run(to64(mods), d, eps, elp, False)
    res.update(extra, base=np.array("h5"), has_grads=np.int64(0))
    print(f"{name}: |td3_y0| {np.linalg.norm(res['td3_y0']):.3f}  |sac_y1| {np.linalg.norm(res['sac_y1']):.3f}")
    return {f"{name}_{k}": v for k, v in res.items()}


def main():
    allout, h5 = {}, None
    for name, spec in CASES.items():
        out, mods, d = one_case(name, spec)
        if name == "h5":
            h5 = (mods, d)
        allout.update({f"{name}_{k}": a for k, a in out.items()})
    mods, d = h5
    eps, elp = [d["eps0"], d["eps1"]], [d["elp0"], d["elp1"]]
    # sat
    m2 = copy.deepcopy(mods)
    with torch.no_grad():
        for a in m2["p"]:
            for lin in (a.fc1, a.fc2, a.fc3):
                lin.weight.mul_(8.0)
    g = torch.Generator().manual_seed(77)
    d2 = dict(d)
    d2["eps0"], d2["eps1"] = d["eps0"] * 4, d["eps1"] * 4
    d2["done"] = (torch.rand(ROWS, 2, generator=g) < 0.3).float().numpy()
    extra = {"eps0": d2["eps0"], "eps1": d2["eps1"], "done": d2["done"]}
    for i in (0, 1):
        for n, p in zip(("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b"), td3_actor_tensors(m2["p"][i])):
            extra[f"p{i}_{n}"] = p.detach().numpy().copy()
    allout.update(variant("sat", m2, d2, [d2["eps0"], d2["eps1"]], elp, extra))
    # clamp
    m3 = copy.deepcopy(mods)
    with torch.no_grad():
        for a in m3["s"]:
            a.log_std_linear.weight.mul_(60.0)
            a.log_std_linear.bias.mul_(60.0)
    extra = {}
    for i in (0, 1):
        for n, p in zip(("log_std_w", "log_std_b"), (m3["s"][i].log_std_linear.weight, m3["s"][i].log_std_linear.bias)):
            extra[f"s{i}_{n}"] = p.detach().numpy().copy()
    allout.update(variant("clamp", m3, d, eps, elp, extra))
    allout.update(variant("noeps", mods, d, None, None, {"has_eps": np.int64(0), "has_elp": np.int64(0)}))
    elp2 = [torch.randn(ROWS, a, generator=g).numpy() * 2 for a in (4, 1)]
    allout.update(variant("twodraw", mods, d, eps, elp2, {"elp0": elp2[0], "elp1": elp2[1]}))
    allout.update(variant("onedraw", mods, d, eps, None, {"has_elp": np.int64(0)}))
    allout["cases"] = np.array(list(CASES) + ["sat", "clamp", "noeps", "twodraw", "onedraw"])
    path = os.path.join(REPO, "tests", "golden", "ctde_critic.npz")
    np.savez_compressed(path, **allout)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
