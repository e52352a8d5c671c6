#!/usr/bin/env python
"""Generate tests/golden/ctde_actor.npz by RUNNING THE REFERENCE's TD3 modules (fdcl-gwu/gym-rotor, algos/td3/td3_mlp.py:
MLP_Actor_TD3 for both agents, MLP_Critic_CTDE.Q1) and its algos/policy_regularization.py in float64 autograd on the CPU with the
CTDE branch of the actor half of TD3.train (algos/td3/td3.py:180-196, without the equivariant term), like
tools/gen_golden_td3_actor.py.

    python tools/gen_golden_ctde_actor.py <path of the reference checkout>

Per case 130 transitions as one minibatch: obs0, obs1, obs_next0, obs_next1 uniform in [-1, 1]; the float32 weights of the actors that
exist (a0_*, a1_*) and of Q1 alone (c_*); `shared` = the name of the case whose networks and rows it uses; action_other (the supplied
form: uniform in [-1, 1], by row); k; noise = the one [obs_dim[k]] draw of policy_regularization (made in float32, recorded), nominal =
its hover action for agent k; coeffs = lam_T, lam_S, lam_M, max_action; and in float64: loss, q_mean, clamp_share, reg and agent k's six
gradients g_*.  Arrays only.
Cases (widths obs 0 + obs 1 / action 0 + action 1; critic hidden width; k):
  k0, k1: 15+3 / 4+1, 62   h64: k = 1, 64   h5: k = 0, 5   noreg: k0's networks, all lam = 0, k = 0
  sat0, sat1: ONE set of networks and rows, max_action = 0.5 and BOTH actors' last layer x 6, k = 0 and k = 1
  w28a: own (15,16,4) as agent 0, the other's obs 5 and action 4 supplied: 15+5+4+4 = 28, critic 62
  w28b: own (3,4,1) as agent 1, the other's obs 16 and action 8 supplied: 16+3+8+1 = 28, critic 62
ReLU makes the gradients discontinuous where a pre-activation crosses 0, so the seeds are searched in order until every
pre-activation — agent k's fc1 and fc2 on obs, obs_next and obs + noise, the other agent's fc1 and fc2 on obs, the critic's fc1 and fc2
on the concatenated row — keeps |z| >= 2e-5 in float64 over all 130 rows; for sat also until of each agent's components of pi_m(obs_m)
between 30 % and 90 % are clamped and none lies within 1e-4 of the bound.  The seed and the achieved minima are stored.
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
sys.argv = ["gen_golden_ctde_actor"]
sys.path.insert(0, os.path.join(HERE, "_gymnasium_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tests"))

import algos.policy_regularization as refreg  # noqa: E402
from algos.td3.td3_mlp import MLP_Actor_TD3, MLP_Critic_CTDE  # noqa: E402
from gym_rotor.envs.quad import QuadEnv  # noqa: E402
import ctde_actor_ref as R  # noqa: E402

LAM = (0.4, 0.3, 0.6)   # args_parse.py
DEC = ([15, 3], [4, 1], [16, 4])
# group: (obs_dim_n, action_dim_n, actor hidden, critic hidden, networks of (None: own), lam, max_action, last-layer scale, first seed,
#         ((case name, k), ...), the agents that have an actor)
GROUPS = {
    "k0": (*DEC, 62, None, LAM, 1.0, 1.0, 100, (("k0", 0),), (0, 1)),
    "k1": (*DEC, 62, None, LAM, 1.0, 1.0, 200, (("k1", 1),), (0, 1)),
    "h64": (*DEC, 64, None, LAM, 1.0, 1.0, 300, (("h64", 1),), (0, 1)),
    "h5": (*DEC, 5, None, LAM, 1.0, 1.0, 400, (("h5", 0),), (0, 1)),
    "noreg": (*DEC, 62, "k0", (0.0, 0.0, 0.0), 1.0, 1.0, 500, (("noreg", 0),), (0, 1)),
    "sat": (*DEC, 62, None, LAM, 0.5, 6.0, 800, (("sat0", 0), ("sat1", 1)), (0, 1)),
    "w28a": ([15, 5], [4, 4], [16, 4], 62, None, LAM, 1.0, 1.0, 600, (("w28a", 0),), (0,)),
    "w28b": ([16, 3], [8, 1], [16, 4], 62, None, LAM, 1.0, 1.0, 700, (("w28b", 1),), (1,)),
}
assert tuple(n for g in GROUPS.values() for n, _ in g[9]) == R.CASES


def tensors(net, n_layers=3):
    return [t for k in range(1, n_layers + 1) for t in (getattr(net, f"fc{k}").weight, getattr(net, f"fc{k}").bias)]


def one_group(gname, spec, env, nets):
    obs_dims, act_dims, hidden, HC, shared, lam, max_action, scale, seed, members, have = spec
    args = SimpleNamespace(rl_algo="TD3", max_action=max_action, obs_dim_n=obs_dims, action_dim_n=act_dims, actor_hidden_dim=hidden,
                           critic_hidden_dim=HC, device="cpu", framework="MODUL", lam_T=lam[0], lam_S=lam[1], lam_M=lam[2])
    real_normal = torch.normal
    while True:   # the seeds in order, until the margins (and sat's clamp conditions) hold for every member
        torch.set_default_dtype(torch.float32)
        torch.manual_seed(seed)
        if shared:
            actors, critic = nets[shared]
        else:
            actors = [MLP_Actor_TD3(args, m) if m in have else None for m in range(2)]
            critic = MLP_Critic_CTDE(args)
            with torch.no_grad():
                for a in actors:
                    if a is not None:
                        a.fc3.weight.mul_(scale)
        g = torch.Generator().manual_seed(10_000 + seed)
        obs = [torch.rand(R.ROWS, d, generator=g) * 2 - 1 for d in obs_dims]
        obs_next = [torch.rand(R.ROWS, d, generator=g) * 2 - 1 for d in obs_dims]
        supplied = {m: torch.rand(R.ROWS, act_dims[m], generator=g) * 2 - 1 for m in range(2) if m not in have}
        w32 = [None if a is None else [p.detach().numpy().copy() for p in tensors(a)] for a in actors]
        q32 = [p.detach().numpy().copy() for p in tensors(critic)]

        torch.set_default_dtype(torch.float64)   # the reference builds its constants (torch.ones, torch.zeros) in the default dtype
        a64 = [None if a is None else copy.deepcopy(a).double() for a in actors]
        c64 = copy.deepcopy(critic).double()
        x, xn = [o.double() for o in obs], [o.double() for o in obs_next]
        outs, ok = {}, True
        for name, k in members:
            drawn = []

            def normal(*a, **kw):   # the one draw of policy_regularization: made in float32, recorded
                v = real_normal(*a, **kw, dtype=torch.float32)
                drawn.append(v.numpy().copy())
                return v.double()

            # td3.py:181, 192-196 on the whole batch as one minibatch; a supplied action is a constant
            acts = [a64[m](x[m]).clamp(-max_action, max_action) if m in have else supplied[m].double() for m in range(2)]
            q1 = c64.Q1(x, acts)
            loss = -q1.mean()
            torch.manual_seed(2000 + seed + k)
            refreg.torch.normal = normal
            try:
                total = refreg.policy_regularization(k, a64[k], loss, x[k], xn[k], env, args)
            finally:
                refreg.torch.normal = real_normal
            for a in a64:
                if a is not None:
                    a.zero_grad()
            total.backward()
            assert len(drawn) == 1 and drawn[0].shape == (1, obs_dims[k])
            noise = drawn[0].reshape(obs_dims[k])
            hover = float(np.interp(4. * env.hover_force, [4. * env.min_force, 4. * env.max_force], [-max_action, max_action]))
            nominal = np.array([0.0] if k == 1 else [hover, 0.0, 0.0, 0.0])
            ao = supplied[1 - k].numpy() if (1 - k) in supplied else None
            m = R.margins(w32, q32, [o.numpy() for o in obs], obs_next[k].numpy(), k, ao, noise, max_action)
            ok = ok and m >= R.MARGIN
            with torch.no_grad():
                mu = a64[k](x[k])
            out = {"k": np.int64(k), "noise": noise, "nominal": nominal, "coeffs": np.array([*lam, max_action], dtype=np.float64),
                   "seed": np.int64(seed), "min_abs_z": np.float64(m), "loss": np.float64(total.item()), "q_mean": np.float64(q1.mean().item()),
                   "clamp_share": np.float64((mu.abs() > max_action).double().mean().item()), "reg": np.float64((total - loss).item())}
            for n, p in zip(R.ACTOR_NAMES, tensors(a64[k])):
                out["g_" + n] = p.grad.numpy().copy()
            if ao is not None:
                out["action_other"] = ao
            outs[name] = out
        first = members[0][0]
        own = {"obs0": obs[0].numpy(), "obs1": obs[1].numpy(), "obs_next0": obs_next[0].numpy(), "obs_next1": obs_next[1].numpy()}
        if shared:
            own["shared"] = np.array(shared)
        else:
            for m in have:
                own.update({f"a{m}_{n}": w for n, w in zip(R.ACTOR_NAMES, w32[m])})
            own.update({"c_" + n: w for n, w in zip(R.Q1_NAMES, q32)})
        outs[first].update(own)
        for name, _ in members[1:]:
            outs[name]["shared"] = np.array(first)
        shares = R.clamp_shares({**own, **{f"a{m}_{n}": w for m in have for n, w in zip(R.ACTOR_NAMES, w32[m])}, "max_action": max_action})
        if gname == "sat":
            ok = ok and all(0.3 <= s <= 0.9 and d >= 1e-4 for s, d in shares.values())
            for name, _ in members:
                outs[name]["clamp_shares"] = np.array([shares[m][0] for m in range(2)])
                outs[name]["clamp_distance"] = np.array([shares[m][1] for m in range(2)])
        if ok:
            break
        seed += 1
    for name, out in outs.items():
        assert all(np.isfinite(v).all() for k, v in out.items() if k != "shared")
        print(f"{name}: obs {obs_dims} act {act_dims} -> {HC}  k {int(out['k'])}  seed {seed}  min|z| {float(out['min_abs_z']):.3e}  "
              f"loss {float(out['loss']):+.6f}  reg {float(out['reg']):.6f}  clamped {[round(s, 2) for s, _ in shares.values()]}  "
              f"max|g| {max(np.abs(out['g_' + n]).max() for n in R.ACTOR_NAMES):.3e}")
    return outs, (actors, critic)


def main():
    env = QuadEnv()
    allout, nets = {}, {}
    for gname, spec in GROUPS.items():
        outs, nets[gname] = one_group(gname, spec, env, nets)
        for name, out in outs.items():
            allout.update({f"{name}_{k}": v for k, v in out.items()})
    allout["cases"] = np.array(list(R.CASES))
    path = os.path.join(REPO, "tests", "golden", "ctde_actor.npz")
    np.savez_compressed(path, **allout)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
