#!/usr/bin/env python
"""Generate tests/golden/ppo_actor_grad.npz by RUNNING THE REFERENCE's actor module and policy regularisation (fdcl-gwu/gym-rotor,
algos/ppo/ppo_mlp.py: MLP_Actor_PPO; algos/policy_regularization.py) in float64 on the CPU, like tools/gen_golden_critic.py.

    python tools/gen_golden_ppo_actor.py <path of the reference checkout>

Per case, for one agent: a hand-built storage of T = 2, N = 65 (130 transitions) — obs [3, 65, D], final_obs [2, 65, D] (NaN in the
rows of envs that did not reset), done [2, 65, n_agents], truncated [2, 65], action / logp_old [2, 65, A], advantage [130] — the
module's weights (float32 values), the one torch.normal draw of the spatial term (the call is wrapped: drawn in float32, recorded),
the nominal action the reference forms from its own QuadEnv's constants, the coefficients, and in float64 the loss of
ppo.py:169-182 + policy_regularization on ALL 130 rows, its seven gradients from autograd, the mean surrogate, the number of rows
with rho outside the clip range and the mean of (rho - 1) - log rho.  Arrays only (np.load(..., allow_pickle=False)).
Cases:  mono (23,16,4)   modul0 (15,16,4)   modul1 (3,4,1)   mono_noreg: all lam = 0   mono_sat: weights x 8, max_action 0.9.
Branch safety, asserted here: every number finite; about a third of the rows outside the clip range, both signs of the advantage
among them; no |rho - (1 +- clip)| below 1e-3; no |mu| within 1e-3 of max_action in any of the three passes.
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
sys.argv = ["gen_golden_ppo_actor"]
sys.path.insert(0, os.path.join(HERE, "_gymnasium_shim"))
sys.path.insert(0, REF)

import algos.policy_regularization as refreg  # noqa: E402
from algos.ppo.ppo_mlp import MLP_Actor_PPO  # noqa: E402
from gym_rotor.envs.quad import QuadEnv  # noqa: E402

T, N = 2, 65
CLIP, ENT = 0.2, 0.01
# name: (framework, obs_dim_n, action_dim_n, hidden, agent, weight scale, max_action, (lam_T, lam_S, lam_M), seed)
CASES = {
    "mono": ("MONO", [23], [4], [16], 0, 1.0, 1.0, (0.4, 0.3, 0.6), 11),
    "modul0": ("MODUL", [15, 3], [4, 1], [16, 4], 0, 1.0, 1.0, (0.4, 0.3, 0.6), 12),
    "modul1": ("MODUL", [15, 3], [4, 1], [16, 4], 1, 1.0, 1.0, (0.4, 0.3, 0.6), 13),
    "mono_noreg": ("MONO", [23], [4], [16], 0, 1.0, 1.0, (0.0, 0.0, 0.0), 14),
    "mono_sat": ("MONO", [23], [4], [16], 0, 8.0, 0.9, (0.4, 0.3, 0.6), 18),   # (seeds 15-17: a |mu| within 1e-3 of max_action)
}
NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std")


def params(net):
    return (net.fc1.weight, net.fc1.bias, net.fc2.weight, net.fc2.bias, net.mean_linear.weight, net.mean_linear.bias, net.log_std)


def one_case(name, spec, env):
    framework, obs_dims, act_dims, hidden, agent, scale, max_action, lams, seed = spec
    D, A, n_agents = obs_dims[agent], act_dims[agent], len(obs_dims)
    torch.manual_seed(seed)
    torch.set_default_dtype(torch.float32)
    net = MLP_Actor_PPO(SimpleNamespace(obs_dim_n=obs_dims, actor_hidden_dim=hidden, action_dim_n=act_dims), agent)
    with torch.no_grad():
        for lin in (net.fc1, net.fc2, net.mean_linear):
            lin.weight.mul_(scale)
        net.mean_linear.bias.copy_(torch.rand(A) * 0.2 - 0.1)
        net.log_std.copy_(torch.linspace(-0.6, -0.3, A).reshape(1, A) if A > 1 else torch.tensor([[-0.45]]))
    w32 = [p.detach().numpy().copy() for p in params(net)]
    g = torch.Generator().manual_seed(1000 + seed)
    obs = torch.rand(T + 1, N, D, generator=g) * 2 - 1
    fin = torch.rand(T, N, D, generator=g) * 2 - 1
    done = torch.rand(T, N, n_agents, generator=g) < 0.05
    trunc = torch.rand(T, N, generator=g) < 0.05
    reset = done.any(-1) | trunc
    assert 3 <= int(reset.sum()) <= 40
    obs_next = torch.where(reset[..., None], fin, obs[1:])
    fin[~reset] = float("nan")
    adv = torch.randn(T * N, generator=g)
    eps = torch.randn(T * N, A, generator=g)
    u = torch.rand(T * N, generator=g)

    torch.set_default_dtype(torch.float64)   # the reference builds its constants (torch.ones, torch.zeros) in the default dtype
    net = net.double()
    x, xn = obs[:-1].reshape(T * N, D).double(), obs_next.reshape(T * N, D).double()
    with torch.no_grad():
        dist = net.get_dist(x)
        act = (dist.mean + dist.stddev * eps.double()).clamp(-max_action, max_action).float()
        lp = dist.log_prob(act.double())
        # the target ratio: every third row outside the clip range (alternately below and above), the others well inside
        rows = torch.arange(T * N)
        out_lo, out_hi = (rows % 3 == 0) & (rows % 2 == 0), (rows % 3 == 0) & (rows % 2 == 1)
        rho = 0.86 + 0.28 * u.double()
        rho = torch.where(out_lo, 0.5 + 0.27 * u.double(), rho)
        rho = torch.where(out_hi, 1.23 + 0.4 * u.double(), rho)
        logp_old = (lp - (rho.log() / A)[:, None]).float()

    drawn = []
    real_normal = torch.normal

    def normal(*a, **kw):   # the one draw of policy_regularization: made in float32, recorded
        v = real_normal(*a, **kw, dtype=torch.float32)
        drawn.append(v.numpy().copy())
        return v.double()

    args = SimpleNamespace(rl_algo="PPO", max_action=max_action, obs_dim_n=obs_dims, device="cpu", framework=framework,
                           lam_T=lams[0], lam_S=lams[1], lam_M=lams[2])
    a64, old64, adv64 = act.double(), logp_old.double(), adv.double()[:, None]
    # ppo.py:169-182 on the whole batch as one minibatch
    dist = net.get_dist(x)
    entropy = dist.entropy().sum(1, keepdim=True)
    ratio = torch.exp(dist.log_prob(a64).sum(1, keepdim=True) - old64.sum(1, keepdim=True))
    s1, s2 = ratio * adv64, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv64
    surr = torch.min(s1, s2)
    loss = -(surr + ENT * entropy).mean()
    torch.manual_seed(2000 + seed)
    refreg.torch.normal = normal
    try:
        loss = refreg.policy_regularization(agent, net, loss, x, xn, env, args)
    finally:
        refreg.torch.normal = real_normal
    net.zero_grad()
    loss.backward()
    assert len(drawn) == 1 and drawn[0].shape == (1, D)
    noise = drawn[0].reshape(D)
    # the nominal action as the reference forms it (policy_regularization.py:30-46)
    hover = float(np.interp(4. * env.hover_force, [4. * env.min_force, 4. * env.max_force], [-max_action, max_action]))
    nominal = np.array([0.0] if (framework == "MODUL" and agent == 1) else [hover, 0.0, 0.0, 0.0])

    # branch safety
    r = ratio.detach().reshape(-1)
    outside = (r < 1 - CLIP) | (r > 1 + CLIP)
    assert 0.25 < outside.double().mean() < 0.45, outside.double().mean()
    assert (adv[outside] > 0).sum() >= 8 and (adv[outside] < 0).sum() >= 8
    assert min((r - (1 - CLIP)).abs().min(), (r - (1 + CLIP)).abs().min()) > 1e-3
    clamped = 0.0
    with torch.no_grad():
        for rows_ in (x, xn, x + torch.from_numpy(noise).double()):
            mu = net(rows_)
            assert (mu.abs() - max_action).abs().min() > 1e-3, (name, (mu.abs() - max_action).abs().min())
            clamped = max(clamped, float((mu.abs() > max_action).double().mean()))
    out = {"obs": obs.numpy(), "final_obs": fin.numpy(), "done": done.numpy().astype(np.uint8), "truncated": trunc.numpy().astype(np.uint8),
           "action": act.numpy().reshape(T, N, A), "logp_old": logp_old.numpy().reshape(T, N, A), "advantage": adv.numpy(),
           "noise": noise, "nominal": nominal, "coeffs": np.array([CLIP, ENT, *lams, max_action], dtype=np.float64),
           "loss": np.float64(loss.item()), "surr": np.float64(surr.mean().item()), "n_clipped": np.int64(outside.sum().item()),
           "kl": np.float64(((ratio - 1) - ratio.log()).mean().item())}
    for n, w, p in zip(NAMES, w32, params(net)):
        out[n] = w.reshape(-1) if n == "log_std" else w
        out["g_" + n] = p.grad.numpy().reshape(-1).copy() if n == "log_std" else p.grad.numpy().copy()
        assert out["g_" + n].dtype == np.float64 and np.array_equal(p.detach().numpy().reshape(w.shape), w.astype(np.float64))
    assert all(np.isfinite(v).all() for k, v in out.items() if k != "final_obs") and np.isfinite(out["final_obs"][reset.numpy()]).all()
    print(f"{name}: ({D},{hidden[agent]},{A})  loss {out['loss']:+.6f}  clipped {int(out['n_clipped'])}/130  resets {int(reset.sum())}  "
          f"share of |mu| > max_action {clamped:.2f}  max|g| {max(np.abs(out['g_' + n]).max() for n in NAMES):.3e}")
    return {f"{name}_{k}": v for k, v in out.items()}


def main():
    env = QuadEnv()
    out = {}
    for name, spec in CASES.items():
        out.update(one_case(name, spec, env))
    out["cases"] = np.array(list(CASES))
    path = os.path.join(REPO, "tests", "golden", "ppo_actor_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
