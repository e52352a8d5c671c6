"""PPO's critic loss and its gradients on the device (qr_ppo_critic_grad, policy.ppo_critic_grad, RolloutStorage.critic_grad,
critic_loss) without a GPU: the float64 restatement of the loss and its HAND-DERIVED gradients the GPU tests compare against,
checked against the reference's own autograd (tests/golden/ppo_critic_grad.npz, tools/gen_golden_ppo_critic.py); the C-ABI struct
mirrors and argument errors; the host-side argument checks."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_critic_host import _Critic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("mono", "dtde0", "dtde1", "ctde", "h64", "h5", "h1", "sat", "mono_nol2")
SIZES = {"mono": (23, 62), "dtde0": (15, 62), "dtde1": (3, 62), "ctde": (18, 62), "h64": (23, 64), "h5": (23, 5), "h1": (23, 1), "sat": (23, 62),
         "mono_nol2": (23, 62)}
ROW_WIDTHS = {"mono": (23,), "dtde0": (15, 3), "dtde1": (15, 3), "ctde": (15, 3), "h64": (23,), "h5": (23,), "h1": (23,), "sat": (23,), "mono_nol2": (23,)}
INPUTS = {"dtde1": (1,), "ctde": (0, 1)}
NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")
T, N = 2, 65


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ppo_critic_grad.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def case(g, name):
    """One case of the fixture as a dict; mono_nol2 takes mono's inputs and weights."""
    own = lambda prefix: {k[len(prefix) + 1:]: v for k, v in g.items() if k.startswith(prefix + "_") and not (prefix == "mono" and k.startswith("mono_nol2_"))}
    c = own("mono") if name == "mono_nol2" else {}
    c.update(own(name))
    c["obs"] = [c[f"obs{k}"] for k in range(len(ROW_WIDTHS[name]))]
    c["inputs"] = tuple(int(i) for i in c["inputs"])
    c["x"] = np.concatenate([c["obs"][k][:T].reshape(T * N, -1) for k in c["inputs"]], axis=1)    # the critic's input rows
    c["w"] = [c[n] for n in NAMES]
    c["l2_reg"] = float(c["l2_reg"])
    return c


def critic_grad_f64(w, x, y, l2_reg):
    """The loss of quadrotor_hip.h (qr_ppo_critic_grad) and its gradients, derived by hand, in float64 NumPy on B rows: x [B, D],
    y [B].  Returns (grads: 6 arrays in NAMES' order, stats: loss, mse, mean error, population variance of y)."""
    w = [np.asarray(t, dtype=np.float64) for t in w]
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1)
    B = x.shape[0]
    t1 = np.tanh(x @ w[0].T + w[1])
    t2 = np.tanh(t1 @ w[2].T + w[3])
    e = (t2 @ w[4].T + w[5]).reshape(-1) - y
    gv = (2.0 * e / B)[:, None]
    dz2 = (gv @ w[4]) * (1.0 - t2 * t2)
    dz1 = (dz2 @ w[2]) * (1.0 - t1 * t1)
    grads = [dz1.T @ x + 2 * l2_reg * w[0], dz1.sum(0), dz2.T @ t1 + 2 * l2_reg * w[2], dz2.sum(0), gv.T @ t2 + 2 * l2_reg * w[4], gv.sum(0)]
    mse = (e * e).mean()
    loss = mse + l2_reg * sum((w[k] * w[k]).sum() for k in (0, 2, 4))
    return grads, np.array([loss, mse, e.mean(), y.var()])


def f64_on_rows(c, idx=None, l2_reg=None):
    """The restatement on rows `idx` (None: all 130) of a case."""
    idx = np.arange(T * N) if idx is None else np.asarray(idx)
    return critic_grad_f64(c["w"], c["x"][idx], c["target"][idx], c["l2_reg"] if l2_reg is None else l2_reg)


def test_fixture_holds_the_cases(fixture):
    assert tuple(fixture["cases"]) == CASES
    for name in CASES:
        c, (D, H) = case(fixture, name), SIZES[name]
        assert [t.shape for t in c["w"]] == [(H, D), (H,), (H, H), (H,), (1, H), (1,)] and all(t.dtype == np.float32 for t in c["w"])
        assert [o.shape for o in c["obs"]] == [(T + 1, N, d) for d in ROW_WIDTHS[name]] and all(o.dtype == np.float32 for o in c["obs"])
        assert c["inputs"] == INPUTS.get(name, (0,)) and c["x"].shape == (T * N, D)
        assert c["target"].shape == (T * N,) and c["target"].dtype == np.float32 and 2.0 < c["target"].std() < 4.0
        assert np.abs(np.concatenate([o.reshape(-1) for o in c["obs"]])).max() <= 1.0
        for n in NAMES:
            assert c["g_" + n].dtype == np.float64 and c["g_" + n].shape == c[n].shape and np.isfinite(c["g_" + n]).all()
        assert all(np.isfinite(c[k]) and c[k].dtype == np.float64 for k in ("loss", "mse", "mean_err", "target_var"))
        assert c["l2_reg"] == (0.0 if name == "mono_nol2" else 1e-4)
    sat, mono = case(fixture, "sat"), case(fixture, "mono")
    assert all(np.array_equal(sat[n], mono[n] * (8 if n.endswith("_w") else 1)) for n in NAMES)
    t1 = np.tanh(sat["x"].astype(np.float64) @ sat["fc1_w"].T.astype(np.float64) + sat["fc1_b"])
    assert (np.abs(t1) > 0.999).mean() > 0.05                       # 1 - t^2 near zero on a measurable share of the units
    assert "mono_nol2_obs0" not in fixture and "mono_nol2_fc1_w" not in fixture
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ppo_critic_grad.npz")) <= 600_000


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(fixture, name):
    c = case(fixture, name)
    grads, stats = f64_on_rows(c)
    for n, got in zip(NAMES, grads):
        want = c["g_" + n]
        assert np.abs(got.reshape(want.shape) - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), n
    for q, k in enumerate(("loss", "mse", "mean_err", "target_var")):
        assert abs(stats[q] - c[k]) <= 1e-12 * max(1.0, abs(c[k])), k


def test_structs_mirror_the_header(tmp_path):
    from gym_rotor_amd import _lib as L
    lines = []
    for sname in ("QrCriticBatch", "QrCriticGrad"):
        lines.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        lines += [f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));' for f, _ in getattr(L, sname)._fields_]
    lines.append('printf("abi %d\\n", QR_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for sname in ("QrCriticBatch", "QrCriticGrad"):
        ct = getattr(L, sname)
        assert int(out[sname]) == C.sizeof(ct)
        for f, _ in ct._fields_:
            assert int(out[f"{sname}.{f}"]) == getattr(ct, f).offset, (sname, f)
    lib = L.load()
    assert {"qr_ppo_critic_grad", "qr_ppo_critic_workspace_bytes"} <= set(L.SYMBOLS) and hasattr(lib, "qr_ppo_critic_grad")
    assert L.PPO_CRITIC_GRAD_NAMES == NAMES and [f for f, _ in L.QrCriticGrad._fields_] == list(NAMES) + ["stats"]
    assert int(out["abi"]) == L.ABI_VERSION == 16


def _fake(in0=23, in1=0, hidden=62, batch=130):
    """(QrCritic, QrCriticBatch, QrCriticGrad) that pass every check, on fake device addresses (never touched: every case of the
    test below returns before a launch)."""
    from gym_rotor_amd import _lib as L
    q = L.QrCritic()
    for k, n in enumerate(NAMES):
        setattr(q, n, 0x10000 + 0x1000 * k)
    q.in0, q.in1, q.hidden_dim = in0, in1, hidden
    b = L.QrCriticBatch()
    for k, n in enumerate(("obs0", "obs1", "target", "index", "workspace")):
        setattr(b, n, 0x100000 + 0x10000 * k)
    b.batch, b.rows, b.target_stride, b.max_workgroups, b.l2_reg = batch, T * N, 1, 0, 1e-4
    b.workspace_bytes = L.load().qr_ppo_critic_workspace_bytes(in0 + in1, hidden, batch, 0) - 1    # one byte short: refused before any launch
    g = L.QrCriticGrad(*[0x800000 + 0x1000 * k for k in range(7)])
    return q, b, g


def test_abi_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()
    NULL, SIZE, ALIGN = -1, -3, -4

    def call(q, b, g):
        return lib.qr_ppo_critic_grad(None if q is None else C.byref(q), None if b is None else C.byref(b), None if g is None else C.byref(g), None)

    q, b, g = _fake()
    assert call(q, b, g) == SIZE                                   # every other check passes: only the workspace is one byte short
    assert call(None, b, g) == NULL and call(q, None, g) == NULL and call(q, b, None) == NULL

    def expect(code, what, fake=(), **edit):
        q, b, g = _fake(*fake)
        for k, v in edit.items():
            setattr({"q": q, "b": b, "g": g}[k[0]], k[2:], v)
        assert call(q, b, g) == code, (what, edit)

    for n in NAMES:
        expect(NULL, "weight", **{"q_" + n: None})
        expect(NULL, "gradient", **{"g_" + n: None})
    expect(NULL, "stats", g_stats=None)
    for n in ("obs0", "target", "workspace"):
        expect(NULL, n, **{"b_" + n: None})
    expect(NULL, "obs1 of a CTDE critic", fake=(15, 3), b_obs1=None)
    expect(NULL, "obs1 of agent 1's critic", fake=(0, 3), b_obs1=None)
    for fake, edit in (((), dict(b_obs1=None)), ((), dict(b_index=None)), ((0, 3), dict(b_obs0=None)), ((15, 3), {}), ((1, 0, 1, 1), {})):
        expect(SIZE, "optional pointers and legal sizes", fake=fake, **edit)     # (SIZE = reached the workspace check)
    for in0, in1, hidden in ((0, 0, 62), (25, 0, 62), (0, 25, 62), (23, 2, 62), (-1, 5, 62), (23, 0, 0), (23, 0, 65), (23, 0, -3)):
        expect(SIZE, "widths", q_in0=in0, q_in1=in1, q_hidden_dim=hidden)
    for edit in (dict(b_batch=0), dict(b_batch=-5), dict(b_rows=0), dict(b_target_stride=0), dict(b_target_stride=-1), dict(b_max_workgroups=-1)):
        expect(SIZE, "sizes", **edit)
    expect(ALIGN, "floats", b_obs0=0x100002)
    expect(ALIGN, "floats", b_target=0x120001)
    expect(ALIGN, "floats", g_fc2_w=0x800001)
    expect(ALIGN, "floats", q_fc3_b=0x15002)
    expect(ALIGN, "index", b_index=0x130004)
    expect(ALIGN, "workspace", b_workspace=0x140004)
    # the workspace size: the grid is min(tiles, max_workgroups or 1024) partial vectors of float64
    ws = lib.qr_ppo_critic_workspace_bytes
    np_mono = 62 * 23 + 62 + 62 * 62 + 62 + 62 + 1 + 4
    assert np_mono == 5461
    assert ws(23, 62, 130, 0) == 3 * np_mono * 8 and ws(23, 62, 130, 2) == 2 * np_mono * 8 and ws(23, 62, 1, 0) == np_mono * 8
    assert ws(23, 62, 64 * 5000, 0) == 1024 * np_mono * 8 and ws(3, 5, 200, 3) == 3 * (15 + 5 + 25 + 5 + 5 + 1 + 4) * 8
    assert ws(24, 64, 64, 0) == (64 * 24 + 64 + 64 * 64 + 64 + 64 + 1 + 4) * 8 and ws(1, 1, 1, 0) == 10 * 8
    for bad in ((23, 62, 0, 0), (23, 62, 10, -1), (0, 62, 10, 0), (25, 62, 10, 0), (23, 0, 10, 0), (23, 65, 10, 0)):
        assert ws(*bad) == SIZE, bad


def _critic_params(din=23, hidden=62, inputs=(0,)):
    from gym_rotor_amd import CriticParams
    return CriticParams.from_module(_Critic(din, hidden), inputs)


def test_host_side_argument_checks():
    from gym_rotor_amd import CriticParams, ppo_critic_grad
    from gym_rotor_amd.policy import ppo_critic_workspace_bytes
    critic = _critic_params()
    obs, target = [torch.zeros(4, 5, 23)], torch.zeros(3, 5)

    def run(critic=critic, obs=obs, target=target, index=None, **kw):
        return ppo_critic_grad(critic, obs, target, index, **kw)

    with pytest.raises(RuntimeError, match="GPU only"):             # every check passes (T+1 rows for T * N targets): no CPU kernel exists
        run()
    with pytest.raises(RuntimeError, match="GPU only"):             # a column of the storage's [T, N, n_agents] tensor; agent 1's rows
        run(critic=_critic_params(3, 62, (1,)), obs=[torch.zeros(4, 5, 15), torch.zeros(4, 5, 3)], target=torch.zeros(3, 5, 2)[..., 1])
    with pytest.raises(RuntimeError, match="GPU only"):             # a CTDE critic; an agent the critic does not read may be None
        run(critic=_critic_params(18, 62, (0, 1)), obs=[torch.zeros(4, 5, 15), torch.zeros(4, 5, 3)])
    with pytest.raises(RuntimeError, match="GPU only"):
        run(critic=_critic_params(3, 62, (1,)), obs=[None, torch.zeros(4, 5, 3)])
    with pytest.raises(ValueError, match="target must be float32"):
        run(target=torch.zeros(3, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="element stride"):
        run(target=torch.zeros(3, 10)[:, :5])
    with pytest.raises(ValueError, match="observation rows 0 must be contiguous float32"):
        run(obs=[torch.zeros(4, 5, 23, dtype=torch.float64)])
    with pytest.raises(ValueError, match="observation rows 0 must be contiguous float32"):
        run(obs=[torch.zeros(4, 23, 5).transpose(1, 2)])
    with pytest.raises(ValueError, match=r">= 15 rows"):           # fewer rows than targets
        run(obs=[torch.zeros(2, 5, 23)])
    with pytest.raises(ValueError, match="reads 23 columns"):
        run(obs=[torch.zeros(4, 5, 15)])
    with pytest.raises(ValueError, match="reads 23 columns"):
        run(critic=CriticParams.from_module(_Critic(23, 62), (0, 1)), obs=[torch.zeros(4, 5, 15), torch.zeros(4, 5, 3)])
    with pytest.raises(ValueError, match="index must be a contiguous int64"):
        run(index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="index must be a contiguous int64"):
        run(index=torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="at least one element"):
        run(obs=[torch.zeros(0, 23)], target=torch.zeros(0), index=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="grads\\['fc1_w'\\]"):
        run(grads={n: torch.zeros(3) for n in NAMES})
    with pytest.raises(ValueError, match="grads\\['fc3_b'\\]"):
        run(grads={n: torch.zeros_like(getattr(critic, n)) for n in NAMES[:5]})
    with pytest.raises(ValueError, match="stats must be a contiguous float32"):
        run(stats=torch.zeros(5))
    with pytest.raises(ValueError, match="critic sizes"):            # CriticParams refuses the sizes the kernel does not take
        CriticParams.from_module(_Critic(23, 65))
    assert ppo_critic_workspace_bytes((23, 62), 130) == 3 * 5461 * 8 and ppo_critic_workspace_bytes((18, 62), 128, 1) == (5461 - 5 * 62) * 8
    with pytest.raises(ValueError, match="QR_E_SIZE"):
        ppo_critic_workspace_bytes((23, 62), 0)
    with pytest.raises(ValueError, match="QR_E_SIZE"):
        ppo_critic_workspace_bytes((23, 62), 10, -1)


def _cpu_storage(kind="coupled", T_=3, N_=5):
    from gym_rotor_amd import RolloutStorage
    dims = {"coupled": [23], "decoupled": [15, 3]}[kind]
    env = SimpleNamespace(num_envs=N_, device=torch.device("cpu"), n_agents=len(dims), action_dim=4 if len(dims) == 1 else 5, obs_dims=dims,
                          auto_reset=False, kind=kind, obs_rows=True)
    return RolloutStorage(env, T_)


def test_storage_critic_grad_and_critic_loss_argument_checks():
    from gym_rotor_amd import CriticParams, critic_loss
    st = _cpu_storage()
    m = _Critic(23, 62)
    critic = CriticParams.from_module(m)
    with pytest.raises(RuntimeError, match="GPU only"):             # the default target, storage.obs with its T+1 rows as it is
        st.critic_grad(0, critic)
    assert list(st._critic_workspace) == [(0, 15, 0)] and st._critic_workspace[(0, 15, 0)].numel() == 5461 and not st._ppo_workspace
    with pytest.raises(RuntimeError, match="GPU only"):
        st.critic_grad(0, critic, torch.zeros(7, dtype=torch.int64), target=torch.zeros(3, 5), max_workgroups=2, l2_reg=1e-4)
    assert set(st._critic_workspace) == {(0, 15, 0), (0, 7, 2)}
    with pytest.raises(ValueError, match="agent 1 of 1"):
        st.critic_grad(1, critic)
    with pytest.raises(ValueError, match="target must be"):
        st.critic_grad(0, critic, target=torch.zeros(15))
    with pytest.raises(ValueError, match="target must be"):
        st.critic_grad(0, critic, target=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="target must be float32"):
        st.critic_grad(0, critic, target=torch.zeros(3, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="reads 15 columns"):
        st.critic_grad(0, CriticParams.from_module(_Critic(15, 62)))
    st2 = _cpu_storage("decoupled")
    with pytest.raises(RuntimeError, match="GPU only"):             # a CTDE critic for agent 1: both row sets, td_target's second column
        st2.critic_grad(1, CriticParams.from_module(_Critic(18, 62), (0, 1)))
    with pytest.raises(ValueError, match="reads 18 columns"):
        st2.critic_grad(1, CriticParams.from_module(_Critic(18, 62), (0,)))
    # critic_loss: allocates the .grad tensors it writes into, takes no grads of its own
    assert m.fc1.weight.grad is None
    with pytest.raises(RuntimeError, match="GPU only"):
        critic_loss(m, st, 0, l2_reg=1e-4)
    assert all(p.grad is not None and p.grad.shape == p.shape and p.grad.is_contiguous() for p in m.parameters())
    with pytest.raises(ValueError, match="takes no grads"):
        critic_loss(m, st, 0, grads={})
    with pytest.raises(ValueError, match="critic inputs must be"):
        critic_loss(m, st, 0, inputs=(2,))
    with pytest.raises(AttributeError):
        critic_loss(torch.nn.Linear(23, 1), st, 0)


def test_torch_op_is_registered_and_refuses_cpu_tensors():
    import gym_rotor_amd  # noqa: F401
    assert hasattr(torch.ops.gym_rotor_amd, "qr_ppo_critic_grad")
    m = _Critic(23, 62)
    w = [p.data for p in (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias)]
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_ppo_critic_grad(w, [0], torch.zeros(4, 5, 23), None, torch.zeros(3, 5), None, [torch.zeros_like(t) for t in w],
                                                   torch.zeros(4), 1e-4)
