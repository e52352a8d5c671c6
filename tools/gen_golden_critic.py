#!/usr/bin/env python
"""Generate tests/golden/critic_values.npz by RUNNING THE REFERENCE's critic modules (fdcl-gwu/gym-rotor,
algos/ppo/ppo_mlp.py: MLP_Critic, MLP_Critic_CTDE) on the CPU in the build container, like tools/gen_golden.py.

    python tools/gen_golden_critic.py [path of the reference checkout, default: the one tools/gen_golden.py uses]

Per case: the module's seeded weights (torch.nn.Linear layout), 130 input rows uniform in [-1, 1] (float32), the module's
float32 outputs and the outputs of its .double() copy on the same rows.  Arrays only (np.load(..., allow_pickle=False)).
Cases (input width -> hidden width):
  mono 23->62 (MONO)   dtde0 15->62, dtde1 3->62 (MODUL, DTDE)   ctde 18->62 (MODUL, CTDE: the module concatenates 15 + 3)
  h64 23->64   h5 23->5   h1 23->1   (the hidden widths at and off the kernel's 16-unit blocks)
  sat   the mono weights x 8: the tanh layers saturate
"""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, REF)

from algos.ppo.ppo_mlp import MLP_Critic, MLP_Critic_CTDE  # noqa: E402

N_ROWS = 130
# name: (class, obs_dim_n, agent_id, hidden, weight scale)
CASES = {
    "mono": (MLP_Critic, [23], 0, 62, 1.0),
    "dtde0": (MLP_Critic, [15, 3], 0, 62, 1.0),
    "dtde1": (MLP_Critic, [15, 3], 1, 62, 1.0),
    "ctde": (MLP_Critic_CTDE, [15, 3], 0, 62, 1.0),
    "h64": (MLP_Critic, [23], 0, 64, 1.0),
    "h5": (MLP_Critic, [23], 0, 5, 1.0),
    "h1": (MLP_Critic, [23], 0, 1, 1.0),
    "sat": (MLP_Critic, [23], 0, 62, 8.0),
}


def main():
    out = {}
    for i, (name, (cls, dims, agent, hidden, scale)) in enumerate(CASES.items()):
        torch.manual_seed(100 if name == "sat" else 100 + i)  # sat: the mono weights (i = 0), scaled
        net = cls(SimpleNamespace(obs_dim_n=dims, critic_hidden_dim=hidden), agent)
        with torch.no_grad():
            for lin in (net.fc1, net.fc2, net.fc3):
                lin.weight.mul_(scale)
        din = net.fc1.weight.shape[1]
        g = torch.Generator().manual_seed(1000 + i)
        x = torch.rand(N_ROWS, din, generator=g) * 2 - 1
        feed = (lambda t: list(torch.split(t, dims, dim=1))) if cls is MLP_Critic_CTDE else (lambda t: t)
        with torch.no_grad():
            v32 = net(feed(x))
            v64 = copy.deepcopy(net).double()(feed(x.double()))
        for lname in ("fc1", "fc2", "fc3"):
            lin = getattr(net, lname)
            out[f"{name}_{lname}_w"] = lin.weight.detach().numpy().copy()
            out[f"{name}_{lname}_b"] = lin.bias.detach().numpy().copy()
        out[f"{name}_x"] = x.numpy()
        out[f"{name}_v32"] = v32.numpy().reshape(-1)
        out[f"{name}_v64"] = v64.numpy().reshape(-1)
        assert out[f"{name}_v32"].dtype == np.float32 and out[f"{name}_v64"].dtype == np.float64
        print(f"{name}: {din}->{hidden}  max|V| {np.abs(out[f'{name}_v64']).max():.3f}  "
              f"max|v32 - v64| {np.abs(out[f'{name}_v32'] - out[f'{name}_v64']).max():.2e}")
    out["cases"] = np.array(list(CASES))
    path = os.path.join(REPO, "tests", "golden", "critic_values.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
