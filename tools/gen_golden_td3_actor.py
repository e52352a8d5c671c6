#!/usr/bin/env python
"""Generate tests/golden/td3_actor.npz by RUNNING THE REFERENCE's TD3 modules (fdcl-gwu/gym-rotor, algos/td3/td3_mlp.py:
MLP_Actor_TD3, MLP_Critic.Q1) and its algos/policy_regularization.py in float64 autograd on the CPU with the actor half of TD3.train
(algos/td3/td3.py:183-196, the non-CTDE branch, without the equivariant term), like tools/gen_golden_ppo_actor.py.

    python tools/gen_golden_td3_actor.py <path of the reference checkout>

Per case 130 transitions as one minibatch: obs, obs_next uniform in [-1, 1]; the float32 weights of the actor (a_*) and of Q1 (c_*, or
`critic` = the name of the case whose Q1 it shares); noise = the one [obs_dim] draw of policy_regularization (made in float32,
recorded), nominal = its hover action; coeffs = lam_T, lam_S, lam_M, max_action; and in float64: loss, q_mean, clamp_share, reg and
the actor's six gradients g_*.  Arrays only.
Cases (actor sizes; critic hidden width):
  mono (23,16,4) 62   dtde0 (15,16,4) 62   dtde1 (3,4,1) 62   h64, h5, h1: the mono sizes with critic width 64, 5, 1
  noreg: mono's sizes and critic with all lam = 0   sat: mono's critic, max_action = 0.5 and the actor's last layer x 6
ReLU makes the gradients discontinuous where a pre-activation crosses 0, so the seeds are searched in order until every
pre-activation — the actor's fc1 and fc2 on obs, obs_next and obs + noise, the critic's fc1 and fc2 on (obs, a) — keeps |z| >= 2e-5
in float64 over all 130 rows (and, for sat, until its clamp conditions hold); the seed and the achieved minimum are stored.
"""
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
sys.argv = ["gen_golden_td3_actor"]
sys.path.insert(0, os.path.join(HERE, "_gymnasium_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tests"))

import algos.policy_regularization as refreg  # noqa: E402
from algos.td3.td3_mlp import MLP_Actor_TD3, MLP_Critic  # noqa: E402
from gym_rotor.envs.quad import QuadEnv  # noqa: E402
import td3_actor_ref as R  # noqa: E402

LAM = (0.4, 0.3, 0.6)   # args_parse.py
# name: (framework, obs_dim_n, action_dim_n, actor hidden, agent, critic hidden, critic of (None: own), lam, max_action, last-layer scale, first seed)
CASES = {
    "mono": ("MONO", [23], [4], [16], 0, 62, None, LAM, 1.0, 1.0, 100),
    "dtde0": ("MODUL", [15, 3], [4, 1], [16, 4], 0, 62, None, LAM, 1.0, 1.0, 200),
    "dtde1": ("MODUL", [15, 3], [4, 1], [16, 4], 1, 62, None, LAM, 1.0, 1.0, 300),
    "h64": ("MONO", [23], [4], [16], 0, 64, None, LAM, 1.0, 1.0, 400),
    "h5": ("MONO", [23], [4], [16], 0, 5, None, LAM, 1.0, 1.0, 500),
    "h1": ("MONO", [23], [4], [16], 0, 1, None, LAM, 1.0, 1.0, 600),
    "noreg": ("MONO", [23], [4], [16], 0, 62, "mono", (0.0, 0.0, 0.0), 1.0, 1.0, 700),
    "sat": ("MONO", [23], [4], [16], 0, 62, "mono", LAM, 0.5, 6.0, 800),
}
assert tuple(CASES) == R.CASES


def tensors(net, n_layers):
    return [t for k in range(1, n_layers + 1) for t in (getattr(net, f"fc{k}").weight, getattr(net, f"fc{k}").bias)]


def one_case(name, spec, env, critics):
    framework, obs_dims, act_dims, hidden, agent, HC, shared, lam, max_action, scale, seed = spec
    D, A = obs_dims[agent], act_dims[agent]
    args = SimpleNamespace(rl_algo="TD3", max_action=max_action, obs_dim_n=obs_dims, action_dim_n=act_dims, actor_hidden_dim=hidden,
                           critic_hidden_dim=HC, device="cpu", framework=framework, lam_T=lam[0], lam_S=lam[1], lam_M=lam[2])
    real_normal = torch.normal
    while True:   # the seeds in order, until the margin (and sat's clamp conditions) hold
        torch.set_default_dtype(torch.float32)
        torch.manual_seed(seed)
        actor = MLP_Actor_TD3(args, agent)
        critic = critics[shared] if shared else MLP_Critic(args, agent)
        with torch.no_grad():
            actor.fc3.weight.mul_(scale)
        g = torch.Generator().manual_seed(10_000 + seed)
        obs, obs_next = torch.rand(R.ROWS, D, generator=g) * 2 - 1, torch.rand(R.ROWS, D, generator=g) * 2 - 1
        w32 = [p.detach().numpy().copy() for p in tensors(actor, 3)]
        q32 = [p.detach().numpy().copy() for p in tensors(critic, 3)]

        torch.set_default_dtype(torch.float64)   # the reference builds its constants (torch.ones, torch.zeros) in the default dtype
        import copy
        a64, c64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
        x, xn = obs.double(), obs_next.double()
        drawn = []

        def normal(*a, **kw):   # the one draw of policy_regularization: made in float32, recorded
            v = real_normal(*a, **kw, dtype=torch.float32)
            drawn.append(v.numpy().copy())
            return v.double()

        # td3.py:183, 192-196 on the whole batch as one minibatch
        act = a64(x).clamp(-max_action, max_action)
        q1 = c64.Q1(x, act)
        loss = -q1.mean()
        torch.manual_seed(2000 + seed)
        refreg.torch.normal = normal
        try:
            total = refreg.policy_regularization(agent, a64, loss, x, xn, env, args)
        finally:
            refreg.torch.normal = real_normal
        a64.zero_grad()
        total.backward()
        assert len(drawn) == 1 and drawn[0].shape == (1, D)
        noise = drawn[0].reshape(D)
        hover = float(np.interp(4. * env.hover_force, [4. * env.min_force, 4. * env.max_force], [-max_action, max_action]))
        nominal = np.array([0.0] if (framework == "MODUL" and agent == 1) else [hover, 0.0, 0.0, 0.0])
        m, _ = R.margins(w32, q32, obs.numpy(), obs_next.numpy(), noise, max_action)
        shares = R.clamp_shares(w32, obs.numpy(), obs_next.numpy(), max_action)
        ok = m >= R.MARGIN
        if name == "sat":
            ok = ok and all(0.2 <= s <= 0.8 and d >= 1e-4 for s, d in shares)
        if ok:
            break
        seed += 1
    with torch.no_grad():
        mu = a64(x)
    out = {"obs": obs.numpy(), "obs_next": obs_next.numpy(), "noise": noise, "nominal": nominal,
           "coeffs": np.array([*lam, max_action], dtype=np.float64), "seed": np.int64(seed), "min_abs_z": np.float64(m),
           "loss": np.float64(total.item()), "q_mean": np.float64(q1.mean().item()),
           "clamp_share": np.float64((mu.abs() > max_action).double().mean().item()), "reg": np.float64((total - loss).item())}
    for n, w, p in zip(R.ACTOR_NAMES, w32, tensors(a64, 3)):
        out["a_" + n] = w
        out["g_" + n] = p.grad.numpy().copy()
    if shared:
        out["critic"] = np.array(shared)
    else:
        for n, w in zip(R.Q1_NAMES, q32):
            out["c_" + n] = w
    assert all(np.isfinite(v).all() for k, v in out.items() if k != "critic")
    print(f"{name}: ({D},{hidden[agent]},{A}) -> {HC}  seed {seed}  min|z| {m:.3e}  loss {out['loss']:+.6f}  reg {out['reg']:.6f}  "
          f"clamped {shares[0][0]:.2f} / {shares[1][0]:.2f}  max|g| {max(np.abs(out['g_' + n]).max() for n in R.ACTOR_NAMES):.3e}")
    return out, critic


def main():
    env = QuadEnv()
    allout, critics = {}, {}
    for name, spec in CASES.items():
        out, critics[name] = one_case(name, spec, env, critics)
        allout.update({f"{name}_{k}": v for k, v in out.items()})
    allout["cases"] = np.array(list(CASES))
    path = os.path.join(REPO, "tests", "golden", "td3_actor.npz")
    np.savez_compressed(path, **allout)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
