#!/usr/bin/env python
"""Generate tests/golden/sac_ctde_actor.npz by RUNNING THE REFERENCE's SAC modules (fdcl-gwu/gym-rotor, algos/sac/sac_mlp.py:
MLP_Actor_SAC.forward for both agents; algos/td3/td3_mlp.py: MLP_Critic_CTDE, which SAC uses) and its algos/policy_regularization.py in
float64 autograd on the CPU with the CTDE branch of the actor half of SAC.train (algos/sac/sac.py:175-203, without the spectral-norm
term), like tools/gen_golden_sac_actor.py and tools/gen_golden_ctde_actor.py.

    python tools/gen_golden_sac_ctde_actor.py <path of the reference checkout>

MLP_Actor_SAC.sample draws its own noise (rsample), so each actor is a thin object whose sample(obs) calls the reference's forward and
restates the sample with the NEXT SUPPLIED draw, in the order the reference makes them: agent 0, agent 1, agent k's second sample (the
log-probability), then policy_regularization's reg, next, pert.  torch.normal is patched to record the one [obs_dim[k]] noise row.
Per case 130 transitions as one minibatch (64 + 64 + 2): obs0, obs1, obs_next0, obs_next1 uniform in [-1, 1]; the float32 weights of
the actors that exist (a0_*, a1_*: eight tensors each) and of the twin critic (c_*: twelve); `shared` = the name of the case whose
networks it uses; the draws eps0, eps1, eps_logp, eps_reg, eps_next, eps_pert that exist; action_other (the supplied form: uniform in
[-1, 1], by row); k; noise, nominal; coeffs = lam_T, lam_S, lam_M, max_action, alpha, target_entropy; and in float64 the six stats,
alpha_grad, agent k's eight gradients g_* and other_action, what the critics read for agent 1 - k.  Arrays only.
Cases (widths obs 0 + obs 1 / action 0 + action 1; critic hidden width; k):
  k0, k1: 15+3 / 4+1, 62   h64: k = 1, 64   h5: k = 0, 5
  on k0's networks, k = 0:  noreg (all lam = 0), noeps (every draw absent), onedraw (no eps_logp: logp from the first sample), alpha0
  clamp: k = 0, both actors' log_std_linear biases pushed so that components fall outside [-20, 2] for agent k AND the other agent
  sat0, sat1: ONE set of networks, max_action = 0.5 and BOTH actors' mean head x 4, k = 0 and k = 1
  w28: own (15,16,4) as agent 0, the other's obs 5 and action 4 supplied, no second actor: 15+5+4+4 = 28, critic 62
The seeds are searched in order until, in float64 over all 130 rows and all passes, every ReLU pre-activation (both actors, both
critics), raw log_std from -20 and 2, |a| from max_action in the reg passes (only where max_action < 1) and |Q1 - Q2| keep 2e-5
(tests/sac_ctde_actor_ref.py: margins), rows lie on both sides of the min, and the case's own conditions hold; the seed and the achieved
minima are stored.
"""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if len(sys.argv) < 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
sys.argv = ["gen_golden_sac_ctde_actor"]
sys.path.insert(0, os.path.join(HERE, "_gymnasium_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tests"))

import algos.policy_regularization as refreg  # noqa: E402
from algos.sac.sac_mlp import MLP_Actor_SAC, epsilon  # noqa: E402
from algos.td3.td3_mlp import MLP_Critic_CTDE  # noqa: E402
from gym_rotor.envs.quad import QuadEnv  # noqa: E402
import sac_ctde_actor_ref as R  # noqa: E402

LAM = (0.4, 0.3, 0.6)   # args_parse.py
DEC = ([15, 3], [4, 1], [16, 4])
ALL = ("eps0", "eps1", "eps_logp", "eps_reg", "eps_next", "eps_pert")
# group: (obs_dim_n, action_dim_n, actor hidden, critic hidden, networks of (None: own), lam, max_action, alpha, mean-head scale, the draws
#         that exist, first seed, ((case name, k), ...), the agents that have an actor)
GROUPS = {
    "k0": (*DEC, 62, None, LAM, 1.0, 0.2, 1.0, ALL, 100, (("k0", 0),), (0, 1)),
    "k1": (*DEC, 62, None, LAM, 1.0, 0.2, 1.0, ALL, 200, (("k1", 1),), (0, 1)),
    "h64": (*DEC, 64, None, LAM, 1.0, 0.2, 1.0, ALL, 300, (("h64", 1),), (0, 1)),
    "h5": (*DEC, 5, None, LAM, 1.0, 0.2, 1.0, ALL, 400, (("h5", 0),), (0, 1)),
    "noreg": (*DEC, 62, "k0", (0.0, 0.0, 0.0), 1.0, 0.2, 1.0, ALL, 500, (("noreg", 0),), (0, 1)),
    "noeps": (*DEC, 62, "k0", LAM, 1.0, 0.2, 1.0, (), 600, (("noeps", 0),), (0, 1)),
    "onedraw": (*DEC, 62, "k0", LAM, 1.0, 0.2, 1.0, tuple(n for n in ALL if n != "eps_logp"), 700, (("onedraw", 0),), (0, 1)),
    "alpha0": (*DEC, 62, "k0", LAM, 1.0, 0.0, 1.0, ALL, 800, (("alpha0", 0),), (0, 1)),
    "clamp": (*DEC, 62, None, LAM, 1.0, 0.2, 1.0, ALL, 900, (("clamp", 0),), (0, 1)),
    "sat": (*DEC, 62, None, LAM, 0.5, 0.2, 4.0, ALL, 1000, (("sat0", 0), ("sat1", 1)), (0, 1)),
    "w28": ([15, 5], [4, 4], [16, 4], 62, None, LAM, 1.0, 0.2, 1.0, tuple(n for n in ALL if n != "eps1"), 1100, (("w28", 0),), (0,)),
}
assert tuple(n for g in GROUPS.values() for n, _ in g[11]) == R.CASES
CLAMP_BIAS = ((-20.5, 2.3, 0.1, -19.7), (2.05,))   # log_std_linear's biases in `clamp`, per agent: components below -20, above 2, near a bound


def actor_tensors(net):
    return [t for l in (net.fc1, net.fc2, net.mean_linear, net.log_std_linear) for t in (l.weight, l.bias)]


def critic_tensors(net):
    return [t for k in range(1, 7) for t in (getattr(net, f"fc{k}").weight, getattr(net, f"fc{k}").bias)]


class Supplied:
    """An actor as sac.py:177-180 and policy_regularization see it: sample(obs) = the reference's forward, then MLP_Actor_SAC.sample's
    lines with rsample's draw taken from the supplied list (None: zeros)."""

    def __init__(self, actor64, eps):
        self.actor, self.eps = actor64, list(eps)

    def sample(self, x):
        mean, log_std = self.actor.forward(x)
        std = log_std.exp()
        e = self.eps.pop(0)
        x_t = mean + std * (torch.zeros_like(mean) if e is None else e)
        action = torch.tanh(x_t)
        log_prob = torch.distributions.Normal(mean, std).log_prob(x_t)
        log_prob = log_prob - torch.log((1 - action.pow(2)) + epsilon)
        return action, log_prob.sum(1, keepdim=True), torch.tanh(mean)


def one_group(gname, spec, env, nets):
    obs_dims, act_dims, hidden, HC, shared, lam, max_action, alpha, scale, have_eps, seed, members, have = spec
    args = SimpleNamespace(rl_algo="SAC", max_action=max_action, obs_dim_n=obs_dims, action_dim_n=act_dims, actor_hidden_dim=hidden,
                           critic_hidden_dim=HC, device="cpu", framework="MODUL", lam_T=lam[0], lam_S=lam[1], lam_M=lam[2])
    real_normal = torch.normal
    while True:   # the seeds in order, until the margins and the case's conditions hold for every member
        torch.set_default_dtype(torch.float32)
        torch.manual_seed(seed)
        if shared:
            actors, critic = nets[shared]
        else:
            actors = [MLP_Actor_SAC(args, m) if m in have else None for m in range(2)]
            critic = MLP_Critic_CTDE(args)   # fc1..fc3 and fc4..fc6 are initialised independently: Q2 is its own network
            with torch.no_grad():   # weights_init_ leaves every bias at 0: give the biases values, so that a dropped bias shows
                for m, a in enumerate(actors):
                    if a is None:
                        continue
                    for l in (a.fc1, a.fc2, a.mean_linear, a.log_std_linear):
                        l.bias.uniform_(-0.3, 0.3)
                    a.mean_linear.weight.mul_(scale)
                    a.mean_linear.bias.mul_(scale)
                    if gname == "clamp":
                        a.log_std_linear.bias.copy_(torch.tensor(CLAMP_BIAS[m]))
        g = torch.Generator().manual_seed(10_000 + seed)
        obs = [torch.rand(R.ROWS, d, generator=g) * 2 - 1 for d in obs_dims]
        obs_next = [torch.rand(R.ROWS, d, generator=g) * 2 - 1 for d in obs_dims]
        supplied = {m: torch.rand(R.ROWS, act_dims[m], generator=g) * 2 - 1 for m in range(2) if m not in have}
        w32 = [None if a is None else [p.detach().numpy().copy() for p in actor_tensors(a)] for a in actors]
        q32 = [p.detach().numpy().copy() for p in critic_tensors(critic)]

        torch.set_default_dtype(torch.float64)   # the reference builds its constants (torch.ones, torch.zeros) in the default dtype
        a64 = [None if a is None else copy.deepcopy(a).double() for a in actors]
        c64 = copy.deepcopy(critic).double()
        x, xn = [o.double() for o in obs], [o.double() for o in obs_next]
        outs, ok = {}, True
        for name, k in members:
            A = act_dims[k]
            target_entropy = -float(A)
            width = {"eps0": act_dims[0], "eps1": act_dims[1]}
            draws = {n: torch.randn(R.ROWS, width.get(n, A), generator=g, dtype=torch.float32) for n in ALL if n in have_eps}
            d64 = lambda n: draws[n].double() if n in draws else None
            own = ["eps_logp"] * ("eps_logp" in have_eps or not have_eps) + ["eps_reg", "eps_next", "eps_pert"]
            one = "eps_logp" not in have_eps and bool(have_eps)   # onedraw: the reference's second sample is not taken
            thin = [None if a64[m] is None else Supplied(a64[m], [d64(f"eps{m}")] + ([d64(n) for n in own] if m == k else [])) for m in range(2)]
            drawn = []

            def normal(*a, **kw):   # the one draw of policy_regularization: made in float32, recorded
                v = real_normal(*a, **kw, dtype=torch.float32)
                drawn.append(v.numpy().copy())
                return v.double()

            # sac.py:176-190 on the whole batch as one minibatch; a supplied action is a constant
            acts, logps = [], [None, None]
            for m in range(2):
                if m in have:
                    a_m, logps[m], _ = thin[m].sample(x[m])
                    acts.append(a_m)
                else:
                    acts.append(supplied[m].double())
            logp = logps[k] if one else thin[k].sample(x[k])[1]
            q1, q2 = c64(x, acts)
            qmin = torch.min(q1, q2)
            loss = -(qmin - alpha * logp).mean()
            torch.manual_seed(2000 + seed + k)
            refreg.torch.normal = normal
            try:
                total = refreg.policy_regularization(k, thin[k], loss, x[k], xn[k], env, args)
            finally:
                refreg.torch.normal = real_normal
            assert all(t is None or not t.eps for t in thin) and len(drawn) == 1 and drawn[0].shape == (1, obs_dims[k])
            for a in a64:
                if a is not None:
                    a.zero_grad()
            total.backward()
            noise = drawn[0].reshape(obs_dims[k])
            hover = float(np.interp(4. * env.hover_force, [4. * env.min_force, 4. * env.max_force], [-max_action, max_action]))
            nominal = np.array([0.0] if k == 1 else [hover, 0.0, 0.0, 0.0])
            ao = supplied[1 - k].numpy() if (1 - k) in supplied else None
            names = {"eps": f"eps{k}", "eps_other": f"eps{1 - k}", "eps_logp": "eps_logp", "eps_reg": "eps_reg", "eps_next": "eps_next", "eps_pert": "eps_pert"}
            eps_np = {a: draws[b].numpy() for a, b in names.items() if b in draws}
            kw = dict(noise=noise, nominal=nominal, lam=lam, max_action=max_action, alpha=alpha, target_entropy=target_entropy)
            pos = (w32, q32, [o.numpy() for o in obs], obs_next[k].numpy(), k, ao, eps_np)
            m = R.margins(*pos, **kw)
            stats, _, _, passes, _, pother = R.ctde_sac_actor_grad_f64(*pos, detail=True, **kw)
            ok = ok and all(v >= R.MARGIN for v in m.values()) and 0.1 <= stats[5] <= 0.9
            if gname == "clamp":
                lsr, lso = passes[0]["lsr"], pother["lsr"]
                ok = ok and (lsr < -20).any() and (lsr > 2).any() and 0.1 <= stats[4] <= 0.9 and ((lso < -20) | (lso > 2)).any()
            if gname == "sat":
                share = float(np.mean([(np.abs(p["a"]) > max_action).mean() for p in passes[2:]]))
                ok = ok and 0.2 <= share <= 0.8 and max(float(np.abs(p["u"]).max()) for p in passes) >= 4.0
            with torch.no_grad():
                lsr64 = a64[k].log_std_linear(torch.relu(a64[k].fc2(torch.relu(a64[k].fc1(x[k])))))
            out = {"k": np.int64(k), "noise": noise, "nominal": nominal,
                   "coeffs": np.array([*lam, max_action, alpha, target_entropy], dtype=np.float64), "seed": np.int64(seed),
                   "margins": np.array([m["relu"], m["ls"], m["clamp"], m["q"]], dtype=np.float64),
                   "stats": np.array([total.item(), qmin.mean().item(), logp.mean().item(), (total - loss).item(),
                                      ((lsr64 < -20) | (lsr64 > 2)).double().mean().item(), (q2 < q1).double().mean().item()], dtype=np.float64),
                   "alpha_grad": np.float64(-(target_entropy + logp.mean().item())), "other_action": acts[1 - k].detach().numpy().copy()}
            out.update({n: e.numpy() for n, e in draws.items()})
            for n, p in zip(R.ACTOR_NAMES, actor_tensors(a64[k])):
                out["g_" + n] = p.grad.numpy().copy()
            if ao is not None:
                out["action_other"] = ao
            outs[name] = out
        first = members[0][0]
        own_rows = {"obs0": obs[0].numpy(), "obs1": obs[1].numpy(), "obs_next0": obs_next[0].numpy(), "obs_next1": obs_next[1].numpy()}
        if shared:
            own_rows["shared"] = np.array(shared)
        else:
            for m in have:
                own_rows.update({f"a{m}_{n}": w for n, w in zip(R.ACTOR_NAMES, w32[m])})
            own_rows.update({"c_" + n: w for n, w in zip(R.CRITIC_NAMES, q32)})
        outs[first].update(own_rows)
        for name, _ in members[1:]:
            outs[name]["shared"] = np.array(first)
        if ok:
            break
        seed += 1
    for name, out in outs.items():
        assert all(np.isfinite(v).all() for k, v in out.items() if k not in ("shared", "margins"))   # (a clamp margin may be inf)
        mm = out["margins"]
        print(f"{name}: obs {obs_dims} act {act_dims} -> {HC}  k {int(out['k'])}  seed {seed}  margins relu {mm[0]:.2e} ls {mm[1]:.2e} clamp {mm[2]:.2e} "
              f"q {mm[3]:.2e}  loss {out['stats'][0]:+.6f}  logp {out['stats'][2]:+.4f}  reg {out['stats'][3]:.6f}  ls outside {out['stats'][4]:.3f}  "
              f"Q2 {out['stats'][5]:.3f}  max|g| {max(np.abs(out['g_' + n]).max() for n in R.ACTOR_NAMES):.3e}")
    return outs, (actors, critic)


def main():
    env = QuadEnv()
    allout, nets = {}, {}
    for gname, spec in GROUPS.items():
        outs, nets[gname] = one_group(gname, spec, env, nets)
        for name, out in outs.items():
            allout.update({f"{name}_{k}": v for k, v in out.items()})
    allout["cases"] = np.array(list(R.CASES))
    path = os.path.join(REPO, "tests", "golden", "sac_ctde_actor.npz")
    np.savez_compressed(path, **allout)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000   # the size limit of a committed file is 1 MiB


if __name__ == "__main__":
    main()
