#!/usr/bin/env python
"""Generate tests/golden/sac_critic.npz by RUNNING THE REFERENCE's SAC modules (fdcl-gwu/gym-rotor, algos/sac/sac_mlp.py:
MLP_Actor_SAC.forward; algos/td3/td3_mlp.py: MLP_Critic, which SAC uses) in float64 on the CPU with the target lines of SAC.train
(algos/sac/sac.py:135-153, the non-CTDE branch), like tools/gen_golden_td3_critic.py.

    python tools/gen_golden_sac_critic.py <path of the reference checkout>

MLP_Actor_SAC.sample draws its own noise (rsample), so its lines are restated here with a SUPPLIED eps:
    x_t = mean + std * eps;   log_prob = Normal(mean, std).log_prob(x_t);   action = tanh(x_t)
    log_prob -= log((1 - action^2) + 1e-6);   log_prob = log_prob.sum(1)                         (sac_mlp.py:66-76)
tanh alone is not torch's: it is evaluated in long double and rounded once to float64 (tanh64 below, the same lines as in
tests/sac_ref.py).  The correction line multiplies one ulp of the action by 2e6 wherever a component is saturated, and float64 tanh
differs by an ulp from library to library (torch's against NumPy's: 2.2e-10 in log_prob), so a fixture made with torch.tanh could not
be restated in NumPy to better than that; the correctly rounded value can.
Per case 130 transitions: obs, obs_next uniform in [-1, 1], action uniform in [-1, 1], reward ~ N(0, 1), done ~ Bernoulli(0.3), eps ~
N(0, 1) [130, A]; the float32 weights of the live actor (a_*), the target critic (t_*) and, in the cases the end-to-end test runs, the
live critic (c_*); the scalars discount and alpha (args_parse.py); and in float64, on all 130 rows as one minibatch: a_next, logp, y.
Arrays only.  Cases (obs + action -> critic hidden):
  mono 23+4->62 (actor 23,16,4)   dtde0 15+4->62 (actor 15,16,4)   dtde1 3+1->62 (actor 3,4,1)      — each with a live critic
  h64, h5: mono's actor and rows with a target critic 23+4 -> 64, 5
  w28 24+4->62: the widest input; no actor has obs_dim 24, so a_next and logp are INPUTS (a_next_in, logp_next_in)
  noeps: mono without eps
  clamp: mono with the log_std head's bias set so that >= 20 % of the components sit below -20 and >= 20 % above 2
  sat: mono with the mean head scaled so that >= 10 % of the components have |u| >= 9
A case with `base` stores only what differs from that case.
ReLU makes the gradients of the end-to-end test discontinuous where a pre-activation crosses 0, so the cases with a live critic keep
every pre-activation of its four gradient-pass layers at |z| >= 2e-5 in float64: the seeds are searched in order until that holds; the
seed and the achieved minimum are stored (seed, min_abs_z).
The archive is written with fixed zip time stamps: the same inputs give the same bytes.
"""
import copy
import io
import os
import sys
import zipfile
from types import SimpleNamespace

import numpy as np
import torch
from torch.distributions import Normal

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if len(sys.argv) < 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
sys.path.insert(0, REF)

from algos.sac.sac_mlp import MLP_Actor_SAC, epsilon  # noqa: E402
from algos.td3.td3_mlp import MLP_Critic  # noqa: E402

ROWS, MARGIN = 130, 2e-5
SCALARS = {"discount": 0.99, "alpha": 0.2}
# name: (obs_dim, action_dim, critic hidden, actor hidden or None, live critic, first seed)
CASES = {
    "mono": (23, 4, 62, 16, True, 100),
    "dtde0": (15, 4, 62, 16, True, 200),
    "dtde1": (3, 1, 62, 4, True, 300),
    "w28": (24, 4, 62, None, False, 700),
}
NAMES = tuple(f"fc{k}_{x}" for k in range(1, 7) for x in "wb")
ACTOR_NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std_w", "log_std_b")


def tanh64(x):
    """tanh of a float64 tensor, evaluated in long double and rounded once (tests/sac_ref.py: tanh64)."""
    return torch.from_numpy(np.tanh(x.numpy().astype(np.longdouble)).astype(np.float64))


def critic_tensors(net):
    return [t for k in range(1, 7) for t in (getattr(net, f"fc{k}").weight, getattr(net, f"fc{k}").bias)]


def actor_tensors(net):
    return [t for l in (net.fc1, net.fc2, net.mean_linear, net.log_std_linear) for t in (l.weight, l.bias)]


def min_abs_z(critic64, sa):
    with torch.no_grad():
        m = float("inf")
        for a, b in ((critic64.fc1, critic64.fc2), (critic64.fc4, critic64.fc5)):
            z1 = a(sa)
            z2 = b(torch.relu(z1))
            m = min(m, z1.abs().min().item(), z2.abs().min().item())
    return m


def target(critic_t, actor, d, eps, sc):
    """sac.py:146-153 in float64 on modules that already are float64; (out, u)."""
    f = lambda x: torch.as_tensor(x).double()
    rwd, obs_next, done = f(d["reward"])[:, None], f(d["obs_next"]), f(d["done"])[:, None]
    with torch.no_grad():
        if actor is not None:
            mean, log_std = actor.forward(obs_next)
            std = log_std.exp()
            normal = Normal(mean, std)
            x_t = mean + std * (f(eps) if eps is not None else torch.zeros_like(mean))
            action = tanh64(x_t)
            log_prob = normal.log_prob(x_t)
            log_prob -= torch.log((1 - action.pow(2)) + epsilon)
            log_prob = log_prob.sum(1, keepdim=True)
        else:
            action, log_prob, x_t, log_std = f(d["a_next_in"]), f(d["logp_next_in"])[:, None], None, None
        tq1, tq2 = critic_t(obs_next, action)
        y = torch.min(tq1, tq2) - sc["alpha"] * log_prob
        y = rwd + sc["discount"] * (1 - done) * y
    out = {"a_next": action.numpy().copy(), "logp": log_prob[:, 0].numpy().copy(), "y": y[:, 0].numpy().copy()}
    return out, (None if x_t is None else x_t.numpy()), (None if log_std is None else actor.log_std_linear(
        torch.relu(actor.fc2(torch.relu(actor.fc1(obs_next))))).detach().numpy())


def build(spec, seed):
    D, A, H, HA, live, _ = spec
    torch.manual_seed(seed)
    cargs = SimpleNamespace(obs_dim_n=[D], action_dim_n=[A], critic_hidden_dim=H, actor_hidden_dim=[HA])
    critic_t = MLP_Critic(cargs, 0)
    critic = MLP_Critic(cargs, 0) if live else None
    actor = MLP_Actor_SAC(cargs, 0) if HA else None
    if actor is not None:   # weights_init_ leaves every bias at 0: give the biases values, so that a dropped bias shows
        with torch.no_grad():
            for l in (actor.fc1, actor.fc2, actor.mean_linear, actor.log_std_linear):
                l.bias.uniform_(-0.3, 0.3)
    g = torch.Generator().manual_seed(10_000 + seed)
    d = {"obs": torch.rand(ROWS, D, generator=g) * 2 - 1, "obs_next": torch.rand(ROWS, D, generator=g) * 2 - 1,
         "action": torch.rand(ROWS, A, generator=g) * 2 - 1, "reward": torch.randn(ROWS, generator=g),
         "done": (torch.rand(ROWS, generator=g) < 0.3).float(), "eps": torch.randn(ROWS, A, generator=g)}
    if not HA:
        d["a_next_in"] = torch.tanh(torch.randn(ROWS, A, generator=g))
        d["logp_next_in"] = torch.randn(ROWS, generator=g) * 3
    return critic, critic_t, actor, {k: v.numpy() for k, v in d.items()}


def one_case(name, spec):
    seed = spec[5]
    while True:   # the seeds in order, until the margin of the live critic holds
        critic, critic_t, actor, d = build(spec, seed)
        m = float("inf")
        if critic is not None:
            sa = torch.cat([torch.as_tensor(d["obs"]).double(), torch.as_tensor(d["action"]).double()], 1)
            m = min_abs_z(copy.deepcopy(critic).double(), sa)
        if m >= MARGIN:
            break
        seed += 1
    out = dict(d)
    out.update({k: np.float64(v) for k, v in SCALARS.items()})
    out.update(seed=np.int64(seed), has_eps=np.int64(1), action_dim=np.int64(spec[1]))
    if critic is not None:
        out["min_abs_z"] = np.float64(m)
        for n, p in zip(NAMES, critic_tensors(critic)):
            out["c_" + n] = p.detach().numpy().copy()
    for n, p in zip(NAMES, critic_tensors(critic_t)):
        out["t_" + n] = p.detach().numpy().copy()
    if actor is not None:
        for n, p in zip(ACTOR_NAMES, actor_tensors(actor)):
            out["a_" + n] = p.detach().numpy().copy()
    res, u, ls = target(copy.deepcopy(critic_t).double(), None if actor is None else copy.deepcopy(actor).double(), d, d["eps"], SCALARS)
    out.update(res)
    report(name, out, u, ls)
    return out, {"critic_t": critic_t, "actor": actor, "data": d}


def report(name, out, u=None, ls=None):
    assert all(np.isfinite(a).all() for k, a in out.items() if k != "base")
    extra = ""
    if u is not None:
        extra = (f"  |u| >= 9: {np.mean(np.abs(u) >= 9):.3f}  ls < -20: {np.mean(ls < -20):.3f}  ls > 2: {np.mean(ls > 2):.3f}")
    print(f"{name}: |y| {np.linalg.norm(out['y']):.3f}  max|logp| {np.abs(out['logp']).max():.3f}  done {int(out['done'].sum()) if 'done' in out else '-'}{extra}")


def write_npz(path, arrays):
    """np.savez_compressed's format with fixed time stamps and the given order: equal arrays give equal bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    allout, mods = {}, {}
    for name, spec in CASES.items():
        out, mods[name] = one_case(name, spec)
        allout.update({f"{name}_{k}": a for k, a in out.items()})
    mm = mods["mono"]
    d, actor = mm["data"], mm["actor"]
    a64 = lambda a: copy.deepcopy(a).double()
    # h64, h5: mono's actor and rows with another target critic
    for name, H, seed in (("h64", 64, 400), ("h5", 5, 500)):
        torch.manual_seed(seed)
        ct = MLP_Critic(SimpleNamespace(obs_dim_n=[23], action_dim_n=[4], critic_hidden_dim=H), 0)
        res, u, ls = target(a64(ct), a64(actor), d, d["eps"], SCALARS)
        for n, p in zip(NAMES, critic_tensors(ct)):
            res["t_" + n] = p.detach().numpy().copy()
        res.update(base=np.array("mono"))
        report(name, res, u, ls)
        allout.update({f"{name}_{k}": a for k, a in res.items()})
    # noeps: mono without eps
    res, u, ls = target(a64(mm["critic_t"]), a64(actor), d, None, SCALARS)
    res.update(has_eps=np.int64(0), base=np.array("mono"))
    report("noeps", res, u, ls)
    allout.update({f"noeps_{k}": a for k, a in res.items()})
    # clamp: the log_std head's bias moves one component below -20, one above 2 and one onto the lower bound
    act = copy.deepcopy(actor)
    with torch.no_grad():
        act.log_std_linear.bias.copy_(torch.tensor([-24.0, 5.0, 0.0, -20.0]))
    res, u, ls = target(a64(mm["critic_t"]), a64(act), d, d["eps"], SCALARS)
    assert np.mean(ls < -20) >= 0.2 and np.mean(ls > 2) >= 0.2, (np.mean(ls < -20), np.mean(ls > 2))
    res.update(a_log_std_b=act.log_std_linear.bias.detach().numpy().copy(), base=np.array("mono"))
    report("clamp", res, u, ls)
    allout.update({f"clamp_{k}": a for k, a in res.items()})
    # sat: the mean head x 40
    act = copy.deepcopy(actor)
    with torch.no_grad():
        act.mean_linear.weight.mul_(40.0)
        act.mean_linear.bias.mul_(40.0)
    res, u, ls = target(a64(mm["critic_t"]), a64(act), d, d["eps"], SCALARS)
    assert np.mean(np.abs(u) >= 9) >= 0.1, np.mean(np.abs(u) >= 9)
    res.update(a_mean_w=act.mean_linear.weight.detach().numpy().copy(), a_mean_b=act.mean_linear.bias.detach().numpy().copy(),
               base=np.array("mono"))
    report("sat", res, u, ls)
    allout.update({f"sat_{k}": a for k, a in res.items()})
    allout["cases"] = np.array(["mono", "dtde0", "dtde1", "h64", "h5", "w28", "noeps", "clamp", "sat"])
    path = os.path.join(REPO, "tests", "golden", "sac_critic.npz")
    write_npz(path, allout)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
