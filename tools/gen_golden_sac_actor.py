#!/usr/bin/env python
"""Generate tests/golden/sac_actor.npz by RUNNING THE REFERENCE's SAC modules (fdcl-gwu/gym-rotor, algos/sac/sac_mlp.py:
MLP_Actor_SAC.forward; algos/td3/td3_mlp.py: MLP_Critic, which SAC uses) and its algos/policy_regularization.py in float64 autograd on
the CPU with the actor half of SAC.train (algos/sac/sac.py:182-211, the non-CTDE branch, without the spectral-norm term), like
tools/gen_golden_td3_actor.py and tools/gen_golden_sac_critic.py.

    python tools/gen_golden_sac_actor.py <path of the reference checkout>

MLP_Actor_SAC.sample draws its own noise (rsample), so the actor is handed to policy_regularization as a thin object whose sample(obs)
calls the reference's forward and restates the sample with the NEXT SUPPLIED eps, in the order the reference draws them: loss, reg,
next, pert.  torch.normal is patched to record the one [obs_dim] noise row (made in float32).  tanh is torch.tanh (autograd needs it).
Per case 130 transitions as one minibatch (three tiles: 64 + 64 + 2): obs, obs_next uniform in [-1, 1]; the float32 weights of the
actor (a_*) and of the twin critic (c_*, Q2 an independent network); the four eps; noise, nominal; coeffs = lam_T, lam_S, lam_M,
max_action, alpha, target_entropy; and in float64 the six stats, alpha_grad and the actor's eight gradients g_*.  Arrays only.
Cases (actor sizes; critic hidden width):
  mono (23,16,4) 62   dtde0 (15,16,4) 62   dtde1 (3,4,1) 62   h64, h5: the mono sizes with critic width 64, 5
  noreg: all lam = 0   noeps: all four eps absent   alpha0: alpha = 0
  clamp: log_std_linear's biases pushed so that components fall below -20 and above 2
  sat: max_action = 0.5 and the mean head scaled, so that both the action clamp and the tanh saturation bite
The seeds are searched in order until, in float64 over all 130 rows and all passes, every ReLU pre-activation (actor and both
critics), raw log_std from -20 and 2, |a| from max_action in the reg passes and |Q1 - Q2| keep 2e-5 (tests/sac_actor_ref.py: margins),
rows lie on both sides of the min, and the case's own conditions hold; the seed and the achieved minima are stored.
"""
import copy
import io
import os
import sys
import zipfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if len(sys.argv) < 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
sys.argv = ["gen_golden_sac_actor"]
sys.path.insert(0, os.path.join(HERE, "_gymnasium_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tests"))

import algos.policy_regularization as refreg  # noqa: E402
from algos.sac.sac_mlp import MLP_Actor_SAC, epsilon  # noqa: E402
from algos.td3.td3_mlp import MLP_Critic  # noqa: E402
from gym_rotor.envs.quad import QuadEnv  # noqa: E402
import sac_actor_ref as R  # noqa: E402

LAM = (0.4, 0.3, 0.6)   # args_parse.py
# name: (framework, obs_dim_n, action_dim_n, actor hidden, agent, critic hidden, lam, max_action, alpha, mean-head scale, eps, first seed)
CASES = {
    "mono": ("MONO", [23], [4], [16], 0, 62, LAM, 1.0, 0.2, 1.0, True, 100),
    "dtde0": ("MODUL", [15, 3], [4, 1], [16, 4], 0, 62, LAM, 1.0, 0.2, 1.0, True, 200),
    "dtde1": ("MODUL", [15, 3], [4, 1], [16, 4], 1, 62, LAM, 1.0, 0.2, 1.0, True, 300),
    "h64": ("MONO", [23], [4], [16], 0, 64, LAM, 1.0, 0.2, 1.0, True, 400),
    "h5": ("MONO", [23], [4], [16], 0, 5, LAM, 1.0, 0.2, 1.0, True, 500),
    "noreg": ("MONO", [23], [4], [16], 0, 62, (0.0, 0.0, 0.0), 1.0, 0.2, 1.0, True, 600),
    "noeps": ("MONO", [23], [4], [16], 0, 62, LAM, 1.0, 0.2, 1.0, False, 700),
    "alpha0": ("MONO", [23], [4], [16], 0, 62, LAM, 1.0, 0.0, 1.0, True, 800),
    "clamp": ("MONO", [23], [4], [16], 0, 62, LAM, 1.0, 0.2, 1.0, True, 900),
    "sat": ("MONO", [23], [4], [16], 0, 62, LAM, 0.5, 0.2, 4.0, True, 1000),
}
assert tuple(CASES) == R.CASES
CLAMP_BIAS = (-20.5, 2.3, 0.1, -19.7)   # log_std_linear's biases in `clamp`: one component below -20, one above 2, two near a bound


def actor_tensors(net):
    return [t for l in (net.fc1, net.fc2, net.mean_linear, net.log_std_linear) for t in (l.weight, l.bias)]


def critic_tensors(net):
    return [t for k in range(1, 7) for t in (getattr(net, f"fc{k}").weight, getattr(net, f"fc{k}").bias)]


class Supplied:
    """The actor as policy_regularization and sac.py:182 see it: sample(obs) = the reference's forward, then MLP_Actor_SAC.sample's
    lines with rsample's draw taken from the supplied list."""

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


def one_case(name, spec, env):
    framework, obs_dims, act_dims, hidden, agent, HC, lam, max_action, alpha, scale, has_eps, seed = spec
    D, A = obs_dims[agent], act_dims[agent]
    args = SimpleNamespace(rl_algo="SAC", max_action=max_action, obs_dim_n=obs_dims, action_dim_n=act_dims, actor_hidden_dim=hidden,
                           critic_hidden_dim=HC, device="cpu", framework=framework, lam_T=lam[0], lam_S=lam[1], lam_M=lam[2])
    real_normal = torch.normal
    target_entropy = -float(A)
    while True:   # the seeds in order, until the margins and the case's conditions hold
        torch.set_default_dtype(torch.float32)
        torch.manual_seed(seed)
        actor = MLP_Actor_SAC(args, agent)
        critic = MLP_Critic(args, agent)   # fc1..fc3 and fc4..fc6 are initialised independently: Q2 is its own network
        with torch.no_grad():   # weights_init_ leaves every bias at 0: give the biases values, so that a dropped bias shows
            for l in (actor.fc1, actor.fc2, actor.mean_linear, actor.log_std_linear):
                l.bias.uniform_(-0.3, 0.3)
            actor.mean_linear.weight.mul_(scale)
            actor.mean_linear.bias.mul_(scale)
            if name == "clamp":
                actor.log_std_linear.bias.copy_(torch.tensor(CLAMP_BIAS[:A]))
        g = torch.Generator().manual_seed(10_000 + seed)
        obs, obs_next = torch.rand(R.ROWS, D, generator=g) * 2 - 1, torch.rand(R.ROWS, D, generator=g) * 2 - 1
        eps32 = [torch.randn(R.ROWS, A, generator=g) if has_eps else None for _ in range(4)]
        w32 = [p.detach().numpy().copy() for p in actor_tensors(actor)]
        q32 = [p.detach().numpy().copy() for p in critic_tensors(critic)]

        torch.set_default_dtype(torch.float64)   # the reference builds its constants (torch.ones, torch.zeros) in the default dtype
        a64, c64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
        x, xn = obs.double(), obs_next.double()
        thin = Supplied(a64, [None if e is None else e.double() for e in eps32])
        drawn = []

        def normal(*a, **kw):   # the one draw of policy_regularization: made in float32, recorded
            v = real_normal(*a, **kw, dtype=torch.float32)
            drawn.append(v.numpy().copy())
            return v.double()

        # sac.py:182-195 on the whole batch as one minibatch
        act, logp, _ = thin.sample(x)
        q1, q2 = c64(x, act)
        qmin = torch.min(q1, q2)
        loss = -(qmin - alpha * logp).mean()
        torch.manual_seed(2000 + seed)
        refreg.torch.normal = normal
        try:
            total = refreg.policy_regularization(agent, thin, loss, x, xn, env, args)
        finally:
            refreg.torch.normal = real_normal
        assert not thin.eps and len(drawn) == 1 and drawn[0].shape == (1, D)
        a64.zero_grad()
        total.backward()
        noise = drawn[0].reshape(D)
        hover = float(np.interp(4. * env.hover_force, [4. * env.min_force, 4. * env.max_force], [-max_action, max_action]))
        nominal = np.array([0.0] if (framework == "MODUL" and agent == 1) else [hover, 0.0, 0.0, 0.0])
        eps_np = [None if e is None else e.numpy() for e in eps32]
        kw = dict(noise=noise, nominal=nominal, lam=lam, max_action=max_action, alpha=alpha, target_entropy=target_entropy)
        m = R.margins(w32, q32, obs.numpy(), obs_next.numpy(), eps_np, **kw)
        stats, _, _, passes, _ = R.sac_actor_grad_f64(w32, q32, obs.numpy(), obs_next.numpy(), eps_np, detail=True, **kw)
        ok = all(v >= R.MARGIN for v in m.values()) and 0.1 <= stats[5] <= 0.9
        if name == "clamp":
            lsr = passes[0]["lsr"]
            ok = ok and (lsr < -20).any() and (lsr > 2).any() and 0.1 <= stats[4] <= 0.9
        if name == "sat":
            share = float(np.mean([(np.abs(p["a"]) > max_action).mean() for p in passes[1:]]))
            ok = ok and 0.2 <= share <= 0.8 and max(float(np.abs(p["u"]).max()) for p in passes) >= 4.0
        if ok:
            break
        seed += 1
    with torch.no_grad():
        lsr = a64.log_std_linear(torch.relu(a64.fc2(torch.relu(a64.fc1(x)))))
    out = {"obs": obs.numpy(), "obs_next": obs_next.numpy(), "noise": noise, "nominal": nominal,
           "coeffs": np.array([*lam, max_action, alpha, target_entropy], dtype=np.float64), "seed": np.int64(seed),
           "margins": np.array([m["relu"], m["ls"], m["clamp"], m["q"]], dtype=np.float64),
           "stats": np.array([total.item(), qmin.mean().item(), logp.mean().item(), (total - loss).item(),
                              ((lsr < -20) | (lsr > 2)).double().mean().item(), (q2 < q1).double().mean().item()], dtype=np.float64),
           "alpha_grad": np.float64(-(target_entropy + logp.mean().item()))}
    if has_eps:
        out.update({k: e for k, e in zip(R.EPS, eps_np)})
    for n, w, p in zip(R.ACTOR_NAMES, w32, actor_tensors(a64)):
        out["a_" + n] = w
        out["g_" + n] = p.grad.numpy().copy()
    for n, w in zip(R.CRITIC_NAMES, q32):
        out["c_" + n] = w
    assert all(np.isfinite(v).all() for k, v in out.items() if k != "margins")   # (noreg: no reg pass, its clamp margin is inf)
    print(f"{name}: ({D},{hidden[agent]},{A}) -> {HC}  seed {seed}  margins relu {m['relu']:.2e} ls {m['ls']:.2e} clamp {m['clamp']:.2e} q {m['q']:.2e}  "
          f"loss {out['stats'][0]:+.6f}  reg {out['stats'][3]:.6f}  ls outside {out['stats'][4]:.3f}  Q2 {out['stats'][5]:.3f}  "
          f"max|u| {max(float(np.abs(p['u']).max()) for p in passes):.2f}  max|g| {max(np.abs(out['g_' + n]).max() for n in R.ACTOR_NAMES):.3e}")
    return out


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
    env = QuadEnv()
    allout = {}
    for name, spec in CASES.items():
        allout.update({f"{name}_{k}": v for k, v in one_case(name, spec, env).items()})
    allout["cases"] = np.array(list(CASES))
    path = os.path.join(REPO, "tests", "golden", "sac_actor.npz")
    write_npz(path, allout)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000   # the size limit of a committed file is 1 MiB


if __name__ == "__main__":
    main()
