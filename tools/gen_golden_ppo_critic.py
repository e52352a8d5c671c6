#!/usr/bin/env python
"""Generate tests/golden/ppo_critic_grad.npz by RUNNING THE REFERENCE's critic modules (fdcl-gwu/gym-rotor, algos/ppo/ppo_mlp.py:
MLP_Critic, MLP_Critic_CTDE) in float64 on the CPU with the critic loss of PPO.train (algos/ppo/ppo.py:193-204), like
tools/gen_golden_critic.py and tools/gen_golden_ppo_actor.py.

    python tools/gen_golden_ppo_critic.py <path of the reference checkout>

Per case, for one critic: a hand-built storage of T = 2, N = 65 (130 transitions) — the per-agent observation rows obs0 [3, 65, D_0]
(and obs1 [3, 65, D_1] for the MODUL cases), uniform in [-1, 1]; target [130] ~ 3 N(0, 1); `inputs`, the agents whose rows the
critic reads; the module's weights (float32 values); l2_reg — and in float64, on ALL 130 rows as one minibatch: the loss
(mse + l2_reg * the squared norms of every parameter whose name holds 'weight', ppo.py:202-204), the mse, the mean error, the
population variance of the target, and the six gradients from autograd.  Arrays only (np.load(..., allow_pickle=False)).
Cases (input width -> hidden width; l2_reg 1e-4 unless said):
  mono 23->62   dtde0 15->62   dtde1 3->62   ctde 15 + 3 -> 62 (MLP_Critic_CTDE: two row sources)
  h64 23->64   h5 23->5   h1 23->1   sat: the mono weights x 8 (saturated tanh)   mono_nol2: mono with l2_reg 0 (shares mono's inputs)
Asserted here: every number finite; in `sat` a share of the hidden units has |t| > 0.999, so 1 - t^2 is exercised near zero.
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
sys.path.insert(0, REF)

from algos.ppo.ppo_mlp import MLP_Critic, MLP_Critic_CTDE  # noqa: E402

T, N = 2, 65
# name: (class, obs_dim_n, agent_id, inputs, hidden, weight scale, l2_reg, seed)
CASES = {
    "mono": (MLP_Critic, [23], 0, (0,), 62, 1.0, 1e-4, 100),
    "dtde0": (MLP_Critic, [15, 3], 0, (0,), 62, 1.0, 1e-4, 101),
    "dtde1": (MLP_Critic, [15, 3], 1, (1,), 62, 1.0, 1e-4, 102),
    "ctde": (MLP_Critic_CTDE, [15, 3], 0, (0, 1), 62, 1.0, 1e-4, 103),
    "h64": (MLP_Critic, [23], 0, (0,), 64, 1.0, 1e-4, 104),
    "h5": (MLP_Critic, [23], 0, (0,), 5, 1.0, 1e-4, 105),
    "h1": (MLP_Critic, [23], 0, (0,), 1, 1.0, 1e-4, 106),
    "sat": (MLP_Critic, [23], 0, (0,), 62, 8.0, 1e-4, 100),      # the mono weights, scaled
    "mono_nol2": (MLP_Critic, [23], 0, (0,), 62, 1.0, 0.0, 100),  # the mono weights and inputs
}
NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")


def params(net):
    return (net.fc1.weight, net.fc1.bias, net.fc2.weight, net.fc2.bias, net.fc3.weight, net.fc3.bias)


def one_case(name, spec):
    cls, dims, agent, inputs, hidden, scale, l2_reg, seed = spec
    torch.manual_seed(seed)
    net = cls(SimpleNamespace(obs_dim_n=dims, critic_hidden_dim=hidden), agent)
    with torch.no_grad():
        for lin in (net.fc1, net.fc2, net.fc3):
            lin.weight.mul_(scale)
    w32 = [p.detach().numpy().copy() for p in params(net)]
    g = torch.Generator().manual_seed(1000 + seed)
    obs = [torch.rand(T + 1, N, d, generator=g) * 2 - 1 for d in dims]
    target = torch.randn(T * N, generator=g) * 3

    net = net.double()
    rows = [obs[k][:T].reshape(T * N, -1).double() for k in inputs]
    v = net(rows) if cls is MLP_Critic_CTDE else net(rows[0])
    err = v - target.double()[:, None]
    mse = err.pow(2).mean()
    loss = mse
    for pname, param in net.named_parameters():   # ppo.py:202-204
        if "weight" in pname:
            loss = loss + param.pow(2).sum() * l2_reg
    net.zero_grad()
    loss.backward()

    out = {"inputs": np.array(inputs, dtype=np.int64), "l2_reg": np.float64(l2_reg), "loss": np.float64(loss.item()), "mse": np.float64(mse.item()),
           "mean_err": np.float64(err.mean().item()), "target_var": np.float64(target.double().var(unbiased=False).item())}
    if name != "mono_nol2":
        out["target"] = target.numpy()
        for k, o in enumerate(obs):
            out[f"obs{k}"] = o.numpy()
    for n, w, p in zip(NAMES, w32, params(net)):
        if name != "mono_nol2":
            out[n] = w
        out["g_" + n] = p.grad.numpy().copy()
        assert out["g_" + n].dtype == np.float64 and np.array_equal(p.detach().numpy(), w.astype(np.float64))
    assert all(np.isfinite(a).all() for a in out.values())
    with torch.no_grad():
        x = torch.cat(rows, dim=1)
        t1 = torch.tanh(net.fc1(x))
        t2 = torch.tanh(net.fc2(t1))
        share = float(((t1.abs() > 0.999).double().mean() + (t2.abs() > 0.999).double().mean()) / 2)
    if name == "sat":
        assert share > 0.05, share
    print(f"{name}: {x.shape[1]}->{hidden}  loss {out['loss']:.6f}  mse {out['mse']:.6f}  share of |t| > 0.999 {share:.3f}  "
          f"max|g| {max(np.abs(out['g_' + n]).max() for n in NAMES):.3e}")
    return {f"{name}_{k}": a for k, a in out.items()}


def main():
    out = {}
    for name, spec in CASES.items():
        out.update(one_case(name, spec))
    out["cases"] = np.array(list(CASES))
    path = os.path.join(REPO, "tests", "golden", "ppo_critic_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
