"""The PPO critic on the device (qr_critic_values / qr_critic_next_values, CriticParams, RolloutStorage.compute_values) without a
GPU: the float64 restatement the GPU tests compare against, checked against the reference's own outputs
(tests/golden/critic_values.npz, tools/gen_golden_critic.py); the C-ABI struct mirror and every argument error; CriticParams."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("mono", "dtde0", "dtde1", "ctde", "h64", "h5", "h1", "sat")
SIZES = {"mono": (23, 62), "dtde0": (15, 62), "dtde1": (3, 62), "ctde": (18, 62), "h64": (23, 64), "h5": (23, 5), "h1": (23, 1), "sat": (23, 62)}


def critic_f64(w, x):
    """MLP_Critic.forward (algos/ppo/ppo_mlp.py:90-93) in float64 NumPy: w = (fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b) in
    torch.nn.Linear layout, x [n, in] -> [n]."""
    w = [np.asarray(t, dtype=np.float64) for t in w]
    h = np.tanh(np.asarray(x, dtype=np.float64) @ w[0].T + w[1])
    h = np.tanh(h @ w[2].T + w[3])
    return (h @ w[4].T + w[5]).reshape(-1)


def case_weights(g, name):
    return tuple(g[f"{name}_{l}_{p}"] for l in ("fc1", "fc2", "fc3") for p in ("w", "b"))


def bar(v64):
    """The project's bar for float32 rows against float64, scaled by the size of the values."""
    return 2e-6 * max(1.0, float(np.abs(v64).max()))


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "critic_values.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def test_fixture_holds_the_cases(fixture):
    assert tuple(fixture["cases"]) == CASES
    for name in CASES:
        din, hidden = SIZES[name]
        w = case_weights(fixture, name)
        assert [t.shape for t in w] == [(hidden, din), (hidden,), (hidden, hidden), (hidden,), (1, hidden), (1,)]
        assert all(t.dtype == np.float32 for t in w)
        x = fixture[f"{name}_x"]
        assert x.shape == (130, din) and x.dtype == np.float32 and -1 <= x.min() and x.max() <= 1
        assert fixture[f"{name}_v32"].shape == (130,) and fixture[f"{name}_v64"].dtype == np.float64
    assert np.array_equal(fixture["sat_fc1_w"], 8 * fixture["mono_fc1_w"]) and np.array_equal(fixture["sat_fc1_b"], fixture["mono_fc1_b"])
    assert np.abs(fixture["sat_v64"]).max() > 5  # the saturating case: values well above 1, so its bar scales


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(fixture, name):
    v = critic_f64(case_weights(fixture, name), fixture[f"{name}_x"])
    v64, v32 = fixture[f"{name}_v64"], fixture[f"{name}_v32"].astype(np.float64)
    assert np.abs(v - v64).max() <= 1e-13
    assert np.abs(v - v32).max() <= 1e-6 * max(1.0, np.abs(v64).max())


def test_qr_critic_mirrors_the_header(tmp_path):
    """QrCritic in gym_rotor_amd/_lib.py against include/quadrotor_hip.h, compiled: size and offsets; the ABI version stays."""
    from gym_rotor_amd import _lib as L
    fl = [f[0] for f in L.QrCritic._fields_]
    lines = ['printf("QrCritic %zu\\n", sizeof(QrCritic));'] + [f'printf("{f} %zu\\n", offsetof(QrCritic, {f}));' for f in fl]
    lines.append('printf("abi %d\\n", QR_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert fl == ["fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b", "in0", "in1", "hidden_dim", "reserved0"]
    assert int(out["QrCritic"]) == C.sizeof(L.QrCritic) == 64
    for f in fl:
        assert int(out[f]) == getattr(L.QrCritic, f).offset, f
    lib = L.load()
    assert {"qr_critic_values", "qr_critic_next_values"} <= set(L.SYMBOLS)
    assert hasattr(lib, "qr_critic_values") and hasattr(lib, "qr_critic_next_values")
    assert int(out["abi"]) == L.ABI_VERSION == 16


def _fake_critic():
    """A QrCritic that passes every check, on fake device addresses (never touched: every case below returns before a launch)."""
    from gym_rotor_amd import _lib as L
    q = L.QrCritic()
    for k, n in enumerate(("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")):
        setattr(q, n, 0x10000 + 0x1000 * k)
    q.in0, q.in1, q.hidden_dim = 23, 0, 62
    return q


def test_abi_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()
    NULL, SIZE, ALIGN = -1, -3, -4
    OBS0, OBS1, VAL, NEXT, DONE, TRUNC = 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000

    def values(q, obs0=OBS0, obs1=None, n=0, value=VAL, stride=1):
        return lib.qr_critic_values(None if q is None else C.byref(q), obs0, obs1, n, value, stride, None)

    def nxt(q, f0=OBS0, f1=None, done=DONE, agents=1, trunc=TRUNC, T=5, N=0, value=VAL, nv=NEXT, stride=1):
        return lib.qr_critic_next_values(None if q is None else C.byref(q), f0, f1, done, agents, trunc, T, N, value, nv, stride, None)

    q = _fake_critic()
    assert values(q) == 0 and nxt(q) == 0                                    # n_rows = 0 / n_envs = 0: nothing launched
    assert nxt(q, trunc=None) == 0                                           # truncated is optional
    assert values(None) == NULL and nxt(None) == NULL
    assert values(q, value=None) == NULL and nxt(q, nv=None) == NULL and nxt(q, value=None) == NULL and nxt(q, done=None) == NULL
    assert values(q, obs0=None) == NULL and nxt(q, f0=None) == NULL          # in0 = 23 needs the obs0 rows
    for name in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b"):
        bad = _fake_critic()
        setattr(bad, name, None)
        assert values(bad) == NULL and nxt(bad) == NULL, name
    # an obs pointer whose in* is 0 may be NULL; one whose in* is not may not
    q1 = _fake_critic()
    q1.in0, q1.in1 = 0, 3
    assert values(q1, obs0=None, obs1=OBS1) == 0 and values(q1, obs0=None, obs1=None) == NULL
    q2 = _fake_critic()
    q2.in0, q2.in1 = 15, 3
    assert values(q2, obs1=OBS1) == 0 and values(q2, obs1=None) == NULL and nxt(q2, f1=None) == NULL and nxt(q2, f1=OBS1) == 0
    # sizes
    for in0, in1, hidden in ((0, 0, 62), (25, 0, 62), (0, 25, 62), (15, 10, 62), (-1, 3, 62), (3, -1, 62), (23, 0, 0), (23, 0, 65), (23, 0, -4)):
        bad = _fake_critic()
        bad.in0, bad.in1, bad.hidden_dim = in0, in1, hidden
        assert values(bad, obs1=OBS1) == SIZE and nxt(bad, f1=OBS1) == SIZE, (in0, in1, hidden)
    for in0, in1, hidden in ((24, 0, 64), (0, 24, 1), (1, 0, 1), (12, 12, 64)):
        ok = _fake_critic()
        ok.in0, ok.in1, ok.hidden_dim = in0, in1, hidden
        assert values(ok, obs1=OBS1) == 0, (in0, in1, hidden)
    assert values(q, n=-1) == SIZE and values(q, stride=0) == SIZE and values(q, stride=-2) == SIZE
    assert nxt(q, T=0) == SIZE and nxt(q, T=-1) == SIZE and nxt(q, N=-1) == SIZE and nxt(q, stride=0) == SIZE and nxt(q, agents=0) == SIZE
    # rows, values and weights are float arrays: 4-byte aligned
    assert values(q, obs0=OBS0 + 2) == ALIGN and values(q, value=VAL + 1) == ALIGN
    assert nxt(q, f0=OBS0 + 2) == ALIGN and nxt(q, value=VAL + 2) == ALIGN and nxt(q, nv=NEXT + 3) == ALIGN
    assert values(q2, obs1=OBS1 + 1) == ALIGN
    bad = _fake_critic()
    bad.fc2_w += 2
    assert values(bad) == ALIGN
    assert values(q, obs0=OBS0 + 4, value=VAL + 4) == 0                      # 4 bytes are enough (an AoS row of 23 floats)


class _Critic(torch.nn.Module):
    """Shaped like the reference's critics: fc1, fc2, fc3."""

    def __init__(self, din, hidden):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(din, hidden), torch.nn.Linear(hidden, hidden), torch.nn.Linear(hidden, 1)

    def forward(self, x):
        x = torch.cat(x, dim=1) if isinstance(x, (list, tuple)) else x
        return self.fc3(torch.tanh(self.fc2(torch.tanh(self.fc1(x)))))


def test_critic_params_from_module():
    from gym_rotor_amd import CriticParams
    # the three input selections, against the widths of the Decoupled wrapper's rows (15, 3) and the Coupled one's (23,)
    m0, m1, mc, mono = _Critic(15, 62), _Critic(3, 62), _Critic(18, 62), _Critic(23, 62)
    c = CriticParams.from_module(m0)
    assert c.inputs == (0,) and c.dims == (15, 62) and c.fc1_w.data_ptr() == m0.fc1.weight.data_ptr()    # the module's own storage
    q = c.as_c([15, 3])
    assert (q.in0, q.in1, q.hidden_dim, q.reserved0) == (15, 0, 62, 0)
    assert [getattr(q, n) for n in CriticParams.NAMES] == [t.data_ptr() for t in (m0.fc1.weight, m0.fc1.bias, m0.fc2.weight, m0.fc2.bias,
                                                                                 m0.fc3.weight, m0.fc3.bias)]
    q = CriticParams.from_module(m1, inputs=(1,)).as_c([15, 3])
    assert (q.in0, q.in1, q.hidden_dim) == (0, 3, 62)
    q = CriticParams.from_module(mc, inputs=(0, 1)).as_c([15, 3])
    assert (q.in0, q.in1, q.hidden_dim) == (15, 3, 62)
    q = CriticParams.from_module(mono).as_c([23])
    assert (q.in0, q.in1, q.hidden_dim) == (23, 0, 62)
    # the selection must add up to the module's input width
    with pytest.raises(ValueError, match="columns"):
        CriticParams.from_module(mc, inputs=(0,)).as_c([15, 3])
    with pytest.raises(ValueError, match="columns"):
        CriticParams.from_module(m1, inputs=(1,)).as_c([23])
    with pytest.raises(ValueError, match="inputs"):
        CriticParams.from_module(m0, inputs=(1, 0))
    with pytest.raises(ValueError, match="inputs"):
        CriticParams.from_module(m0, inputs=(2,))
    # sizes past the kernel's padded widths; weights that are not float32
    assert CriticParams.from_module(_Critic(24, 64)).dims == (24, 64) and CriticParams.from_module(_Critic(1, 1)).dims == (1, 1)
    with pytest.raises(ValueError, match="hidden = 65"):
        CriticParams.from_module(_Critic(23, 65))
    with pytest.raises(ValueError, match="in = 25"):
        CriticParams.from_module(_Critic(25, 62))
    with pytest.raises(ValueError, match="float32"):
        CriticParams.from_module(_Critic(23, 62).double())
    with pytest.raises(ValueError, match="float32"):
        CriticParams.from_module(_Critic(23, 62).half())
    # no CPU kernel behind the launches
    from gym_rotor_amd.policy import critic_values
    with pytest.raises(RuntimeError, match="GPU only"):
        critic_values(CriticParams.from_module(mono), [torch.zeros(4, 23)], torch.zeros(4))


def test_torch_ops_are_registered_and_refuse_cpu_tensors():
    import gym_rotor_amd  # noqa: F401
    assert hasattr(torch.ops.gym_rotor_amd, "qr_critic_values") and hasattr(torch.ops.gym_rotor_amd, "qr_critic_next_values")
    m = _Critic(23, 62)
    w = [m.fc1.weight.data, m.fc1.bias.data, m.fc2.weight.data, m.fc2.bias.data, m.fc3.weight.data, m.fc3.bias.data]
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_critic_values(w, [0], torch.zeros(4, 23), None, torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_critic_next_values(w, [0], torch.zeros(2, 4, 23), None, torch.zeros(2, 4, 1, dtype=torch.bool),
                                                      torch.zeros(2, 4, dtype=torch.bool), torch.zeros(3, 4), torch.zeros(2, 4))
