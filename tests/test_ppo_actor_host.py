"""PPO's actor loss and its gradients on the device (qr_ppo_actor_grad, policy.ppo_actor_grad, RolloutStorage.actor_grad) without a
GPU: the float64 restatement of the loss and its HAND-DERIVED gradients the GPU tests compare against, checked against the
reference's own autograd (tests/golden/ppo_actor_grad.npz, tools/gen_golden_ppo_actor.py); the fixture's branch-safety conditions;
the C-ABI struct mirrors and argument errors; the host-side argument checks; nominal_action."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("mono", "modul0", "modul1", "mono_noreg", "mono_sat")
DIMS = {"mono": (23, 16, 4), "modul0": (15, 16, 4), "modul1": (3, 4, 1), "mono_noreg": (23, 16, 4), "mono_sat": (23, 16, 4)}
NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std")
COEFFS = ("clip", "entropy_coef", "lam_T", "lam_S", "lam_M", "max_action")
T, N = 2, 65


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ppo_actor_grad.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def case(g, name):
    """One case of the fixture as a dict, with the reference's obs_next rows built by the storage's rule."""
    c = {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "_") and not (name == "mono" and k.startswith(("mono_noreg_", "mono_sat_")))}
    reset = c["done"].any(-1) | (c["truncated"] != 0)
    c["reset"] = reset
    c["obs_next"] = np.where(reset[..., None], c["final_obs"], c["obs"][1:])
    c["w"] = [c[n] for n in NAMES]
    c["co"] = dict(zip(COEFFS, (float(v) for v in c["coeffs"])))
    return c


def _forward(w, x):
    h1 = np.maximum(x @ w[0].T + w[1], 0.0)
    h2 = np.maximum(h1 @ w[2].T + w[3], 0.0)
    return h1, h2, np.tanh(h2 @ w[4].T + w[5])


def _backward(w, x, h1, h2, mu, dmu, g):
    dp = dmu * (1.0 - mu * mu)
    g[4] += dp.T @ h2; g[5] += dp.sum(0)
    dz2 = (dp @ w[4]) * (h2 > 0)
    g[2] += dz2.T @ h1; g[3] += dz2.sum(0)
    dz1 = (dz2 @ w[2]) * (h1 > 0)
    g[0] += dz1.T @ x; g[1] += dz1.sum(0)


def ppo_f64(w, x, x_next, act, logp_old, adv, co, noise=None, nominal=None):
    """The loss of quadrotor_hip.h (qr_ppo_actor_grad) and its gradients, derived by hand, in float64 NumPy on B rows:
    x, x_next [B, D], act / logp_old [B, A], adv [B].  Returns (grads: 7 arrays in NAMES' order, stats: loss, mean S, number of rows
    outside the clip range, mean of (rho - 1) - log rho)."""
    w = [np.asarray(t, dtype=np.float64) for t in w]
    x, x_next, act, logp_old, adv = (np.asarray(t, dtype=np.float64) for t in (x, x_next, act, logp_old, adv))
    B, A = act.shape
    s = w[6].reshape(-1)
    clip, ent, lam_T, lam_S, lam_M, ma = (co[k] for k in COEFFS)
    g = [np.zeros_like(t) for t in w[:6]]
    h1, h2, mu = _forward(w, x)
    diff, ivar = act - mu, np.exp(-2.0 * s)
    lp = (-0.5 * diff * diff * ivar - s - 0.5 * np.log(2 * np.pi)).sum(1)
    rho = np.exp(lp - logp_old.sum(1))
    s1, s2 = rho * adv, np.clip(rho, 1 - clip, 1 + clip) * adv
    S = np.minimum(s1, s2)
    inside = (rho >= 1 - clip) & (rho <= 1 + clip)
    gS = np.where(inside | (s1 < s2), s1, 0.0)[:, None]          # dS / d(sum of log-probs): torch.min's and torch.clamp's routing
    dmu = -gS * diff * ivar / B
    g_ls = (-gS * (diff * diff * ivar - 1.0) / B).sum(0) - ent
    loss = -S.mean() - ent * (0.5 + 0.5 * np.log(2 * np.pi) + s).sum()
    m = np.clip(mu, -ma, ma)
    dm = np.zeros_like(mu)
    if lam_M != 0:
        d = m - np.asarray(nominal, dtype=np.float64)
        loss += lam_M * (d * d).mean(); dm += 2 * lam_M * d / (B * A)
    for lam, y in ((lam_S, None if noise is None else x + np.asarray(noise, dtype=np.float64)), (lam_T, x_next)):
        if lam == 0:
            continue
        g1, g2, mo = _forward(w, y)
        d = m - np.clip(mo, -ma, ma)
        loss += lam * (d * d).mean(); dm += 2 * lam * d / (B * A)
        _backward(w, y, g1, g2, mo, -2 * lam * d / (B * A) * (np.abs(mo) <= ma), g)
    _backward(w, x, h1, h2, mu, dmu + dm * (np.abs(mu) <= ma), g)
    return g + [g_ls], np.array([loss, S.mean(), float((~inside).sum()), ((rho - 1) - np.log(rho)).mean()])


def f64_on_rows(c, idx=None):
    """The restatement on rows `idx` (None: all 130) of a case."""
    idx = np.arange(T * N) if idx is None else np.asarray(idx)
    D, _, A = c["fc1_w"].shape[1], 0, c["mean_w"].shape[0]
    return ppo_f64(c["w"], c["obs"][:-1].reshape(-1, D)[idx], c["obs_next"].reshape(-1, D)[idx], c["action"].reshape(-1, A)[idx],
                   c["logp_old"].reshape(-1, A)[idx], c["advantage"][idx], c["co"], c["noise"], c["nominal"])


def test_fixture_holds_the_cases(fixture):
    assert tuple(fixture["cases"]) == CASES
    for name in CASES:
        c, (D, H, A) = case(fixture, name), DIMS[name]
        assert [t.shape for t in c["w"]] == [(H, D), (H,), (H, H), (H,), (A, H), (A,), (A,)] and all(t.dtype == np.float32 for t in c["w"])
        assert c["obs"].shape == (T + 1, N, D) and c["final_obs"].shape == (T, N, D) and c["action"].shape == (T, N, A)
        assert c["done"].shape == (T, N, 2 if name.startswith("modul") else 1) and c["truncated"].shape == (T, N)
        assert c["noise"].shape == (D,) and c["noise"].dtype == np.float32 and c["nominal"].shape == (A,)
        for n in NAMES:
            assert c["g_" + n].dtype == np.float64 and c["g_" + n].shape == c[n].shape
        assert np.isnan(c["final_obs"][~c["reset"]]).all() and np.isfinite(c["obs_next"]).all() and 3 <= c["reset"].sum() <= 40
    assert case(fixture, "mono_noreg")["co"]["lam_T"] == 0 and case(fixture, "mono_sat")["co"]["max_action"] == 0.9
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ppo_actor_grad.npz")) <= 220_000


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(fixture, name):
    c = case(fixture, name)
    grads, stats = f64_on_rows(c)
    for n, got in zip(NAMES, grads):
        want = c["g_" + n]
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), n
    assert abs(stats[0] - c["loss"]) <= 1e-12 * max(1.0, abs(c["loss"]))
    assert abs(stats[1] - c["surr"]) <= 1e-12 and stats[2] == c["n_clipped"] and abs(stats[3] - c["kl"]) <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_branch_safe(fixture, name):
    """Every number finite, about a third of the rows outside the clip range with both signs of the advantage, no ratio within 1e-3
    of a clip bound and no |mu| within 1e-3 of max_action in any pass: a float32 evaluation takes float64's branches."""
    c = case(fixture, name)
    D, A = c["fc1_w"].shape[1], c["mean_w"].shape[0]
    w = [t.astype(np.float64) for t in c["w"]]
    x = c["obs"][:-1].reshape(-1, D).astype(np.float64)
    assert all(np.isfinite(c[k]).all() for k in ("obs", "action", "logp_old", "advantage", "noise", "nominal") + tuple("g_" + n for n in NAMES))
    mu = _forward(w, x)[2]
    diff, s = c["action"].reshape(-1, A) - mu, w[6]
    rho = np.exp((-0.5 * diff * diff * np.exp(-2 * s) - s - 0.5 * np.log(2 * np.pi)).sum(1) - c["logp_old"].reshape(-1, A).astype(np.float64).sum(1))
    clip, ma = c["co"]["clip"], c["co"]["max_action"]
    out = (rho < 1 - clip) | (rho > 1 + clip)
    assert 0.25 < out.mean() < 0.45 and out.sum() == c["n_clipped"]
    assert (c["advantage"][out] > 0).sum() >= 8 and (c["advantage"][out] < 0).sum() >= 8
    assert (rho < 1 - clip).sum() >= 8 and (rho > 1 + clip).sum() >= 8
    assert min(np.abs(rho - (1 - clip)).min(), np.abs(rho - (1 + clip)).min()) > 1e-3
    share = 0.0
    for y in (x, c["obs_next"].reshape(-1, D).astype(np.float64), x + c["noise"]):
        mo = _forward(w, y)[2]
        assert np.abs(np.abs(mo) - ma).min() > 1e-3
        share = max(share, (np.abs(mo) > ma).mean())
    assert (share > 0.2) == (name == "mono_sat")     # the clamp acts on a measurable share of the elements there, and nowhere else


def test_structs_mirror_the_header(tmp_path):
    from gym_rotor_amd import _lib as L
    lines = []
    for sname in ("QrPpoBatch", "QrPpoGrad"):
        lines.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        lines += [f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));' for f, _ in getattr(L, sname)._fields_]
    lines.append('printf("abi %d\\n", QR_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for sname in ("QrPpoBatch", "QrPpoGrad"):
        ct = getattr(L, sname)
        assert int(out[sname]) == C.sizeof(ct)
        for f, _ in ct._fields_:
            assert int(out[f"{sname}.{f}"]) == getattr(ct, f).offset, (sname, f)
    lib = L.load()
    assert {"qr_ppo_actor_grad", "qr_ppo_actor_workspace_bytes"} <= set(L.SYMBOLS) and hasattr(lib, "qr_ppo_actor_grad")
    assert int(out["abi"]) == L.ABI_VERSION == 16


def _fake(dims=(23, 16, 4), batch=130):
    """(QrActor, QrPpoBatch, QrPpoGrad) that pass every check, on fake device addresses (never touched: every case of the test below
    returns before a launch)."""
    from gym_rotor_amd import _lib as L
    q = L.QrActor()
    for k, n in enumerate(NAMES):
        setattr(q, n, 0x10000 + 0x1000 * k)
    q.obs_dim, q.hidden_dim, q.action_dim, q.squash = *dims, L.ACTOR_TANH_MEAN
    b = L.QrPpoBatch()
    for k, n in enumerate(("obs", "final_obs", "done", "truncated", "action", "logp_old", "advantage", "index", "noise", "nominal", "workspace")):
        setattr(b, n, 0x100000 + 0x10000 * k)
    b.batch, b.n_envs, b.n_steps, b.n_agents, b.row_stride, b.col_offset, b.adv_stride = batch, N, T, 1, dims[2], 0, 1
    b.clip, b.entropy_coef, b.lam_T, b.lam_S, b.lam_M, b.max_action = 0.2, 0.01, 0.4, 0.3, 0.6, 1.0
    b.workspace_bytes = L.load().qr_ppo_actor_workspace_bytes(*dims, batch, 0) - 1      # one byte short: refused before any launch
    g = L.QrPpoGrad(*[0x800000 + 0x1000 * k for k in range(8)])
    return q, b, g


def test_abi_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()
    NULL, KIND, SIZE, ALIGN = -1, -2, -3, -4

    def call(q, b, g):
        return lib.qr_ppo_actor_grad(None if q is None else C.byref(q), None if b is None else C.byref(b), None if g is None else C.byref(g), None)

    q, b, g = _fake()
    assert call(q, b, g) == SIZE                                   # every other check passes: only the workspace is one byte short
    assert call(None, b, g) == NULL and call(q, None, g) == NULL and call(q, b, None) == NULL

    def expect(code, what, **edit):
        q, b, g = _fake()
        for k, v in edit.items():
            setattr({"q": q, "b": b, "g": g}[k[0]], k[2:], v)
        assert call(q, b, g) == code, (what, edit)

    for n in NAMES:
        expect(NULL, "weight", **{"q_" + n: None})
        expect(NULL, "gradient", **{"g_" + n: None})
    expect(NULL, "stats", g_stats=None)
    for n in ("obs", "action", "logp_old", "advantage", "workspace", "done", "noise", "nominal"):
        expect(NULL, n, **{"b_" + n: None})
    for edit in (dict(b_final_obs=None, b_done=None), dict(b_truncated=None), dict(b_index=None), dict(b_noise=None, b_lam_S=0.0),
                 dict(b_nominal=None, b_lam_M=0.0)):
        expect(SIZE, "optional pointers", **edit)                   # (SIZE = reached the workspace check)
    expect(KIND, "squash", q_squash=L.ACTOR_TANH_SAMPLE)
    expect(KIND, "log_std head", q_log_std_w=0x9000, q_log_std_b=0xA000)
    for dims in ((23, 16, 3), (22, 16, 4), (15, 4, 4), (3, 4, 4), (0, 0, 0)):
        expect(SIZE, "dims", q_obs_dim=dims[0], q_hidden_dim=dims[1], q_action_dim=dims[2])
    for edit in (dict(b_batch=0), dict(b_batch=-5), dict(b_n_steps=0), dict(b_n_envs=0), dict(b_row_stride=0), dict(b_adv_stride=0),
                 dict(b_max_workgroups=-1), dict(b_col_offset=-1), dict(b_col_offset=1), dict(b_n_agents=0)):
        expect(SIZE, "sizes", **edit)
    expect(ALIGN, "floats", b_obs=0x100002)
    expect(ALIGN, "floats", g_fc2_w=0x800001)
    expect(ALIGN, "index", b_index=0x170004)
    expect(ALIGN, "workspace", b_workspace=0x1A0004)
    # the workspace size: the grid is min(tiles, max_workgroups or 1024) partial vectors of float64
    ws = lib.qr_ppo_actor_workspace_bytes
    np_mono = 23 * 16 + 16 + 256 + 16 + 64 + 4 + 4 + 6
    assert ws(23, 16, 4, 130, 0) == 3 * np_mono * 8 and ws(23, 16, 4, 130, 2) == 2 * np_mono * 8 and ws(23, 16, 4, 1, 0) == np_mono * 8
    assert ws(23, 16, 4, 64 * 5000, 0) == 1024 * np_mono * 8 and ws(3, 4, 1, 200, 3) == 3 * (12 + 4 + 16 + 4 + 4 + 1 + 1 + 6) * 8
    assert ws(23, 16, 4, 0, 0) == SIZE and ws(23, 62, 4, 10, 0) == SIZE and ws(23, 16, 4, 10, -1) == SIZE


class _Actor(torch.nn.Module):
    """Shaped like the reference's MLP_Actor_PPO: fc1, fc2, mean_linear, log_std [1, A]."""

    def __init__(self, D, H, A, log_std=-0.5):
        super().__init__()
        self.fc1, self.fc2, self.mean_linear = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, A)
        self.log_std = torch.nn.Parameter(torch.ones(1, A) * log_std)

    def forward(self, x):
        return torch.tanh(self.mean_linear(torch.relu(self.fc2(torch.relu(self.fc1(x))))))


def _host_args(D=23, A=4, t=3, n=5):
    return dict(obs=torch.zeros(t + 1, n, D), action=torch.zeros(t, n, A), logp_old=torch.zeros(t, n, A), advantage=torch.zeros(t, n))


def test_host_side_argument_checks():
    from gym_rotor_amd import ActorParams, ppo_actor_grad
    from gym_rotor_amd.policy import random_actors
    actor = ActorParams.from_module(_Actor(23, 16, 4))

    def run(actor=actor, **edit):
        a = _host_args()
        kw = {k: edit.pop(k) for k in list(edit) if k not in a}
        a.update(edit)
        return ppo_actor_grad(actor, a["obs"], a["action"], a["logp_old"], a["advantage"], **kw)

    with pytest.raises(RuntimeError, match="GPU only"):             # every check passes: no CPU kernel exists
        run()
    with pytest.raises(ValueError, match="actor sizes"):
        run(actor=ActorParams.from_module(_Actor(23, 32, 4)))
    with pytest.raises(ValueError, match="actor sizes"):
        run(actor=ActorParams.from_module(_Actor(18, 16, 4)))
    with pytest.raises(ValueError, match="MLP_Actor_PPO's form"):
        run(actor=random_actors("coupled", "cpu", algo="sac")[0])
    with pytest.raises(ValueError, match="float32"):
        run(actor=ActorParams.from_module(_Actor(23, 16, 4).double()))
    with pytest.raises(ValueError, match="obs must be contiguous float32"):
        run(obs=torch.zeros(4, 5, 23, dtype=torch.float64))
    with pytest.raises(ValueError, match="obs must be contiguous float32"):
        run(obs=torch.zeros(4, 23, 5).transpose(1, 2))
    with pytest.raises(ValueError, match="obs must be contiguous float32"):
        run(obs=torch.zeros(4, 5, 15))
    with pytest.raises(ValueError, match="action must be float32"):
        run(action=torch.zeros(3, 5, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="action must be float32"):
        run(action=torch.zeros(3, 5, 3))
    with pytest.raises(ValueError, match="rows of a contiguous"):
        run(action=torch.zeros(3, 4, 5).transpose(1, 2))
    with pytest.raises(ValueError, match="same row stride"):
        run(logp_old=torch.zeros(3, 5, 5)[..., :4])
    with pytest.raises(ValueError, match="advantage must be float32"):
        run(advantage=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="element stride"):
        run(advantage=torch.zeros(3, 10)[:, :5])
    with pytest.raises(ValueError, match="index must be a contiguous int64"):
        run(index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="noise is required"):
        run(lam_S=0.3)
    with pytest.raises(ValueError, match="nominal is required"):
        run(lam_M=0.3)
    with pytest.raises(ValueError, match="noise must be a contiguous float32 tensor of 23"):
        run(lam_S=0.3, noise=torch.zeros(22))
    with pytest.raises(ValueError, match="final_obs needs done"):
        run(final_obs=torch.zeros(3, 5, 23))
    with pytest.raises(ValueError, match="done must be contiguous bool"):
        run(final_obs=torch.zeros(3, 5, 23), done=torch.zeros(3, 5, 1))
    with pytest.raises(ValueError, match="grads\\['fc1_w'\\]"):
        run(grads={n: torch.zeros(3) for n in NAMES})
    with pytest.raises(RuntimeError, match="GPU only"):             # the storage's shared rows with a column offset; log_std grads as [1, A]
        ppo_actor_grad(ActorParams.from_module(_Actor(3, 4, 1)), torch.zeros(4, 5, 3), torch.zeros(3, 5, 5), torch.zeros(3, 5, 5),
                       torch.zeros(3, 5, 2)[..., 1], col_offset=4)


def test_torch_op_is_registered_and_refuses_cpu_tensors():
    import gym_rotor_amd  # noqa: F401
    assert hasattr(torch.ops.gym_rotor_amd, "qr_ppo_actor_grad")
    m = _Actor(23, 16, 4)
    w = [p.data for p in (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.mean_linear.weight, m.mean_linear.bias, m.log_std)]
    a = _host_args()
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_ppo_actor_grad(w, a["obs"], None, None, None, a["action"], a["logp_old"], a["advantage"], None, None, None,
                                                  [torch.zeros_like(t) for t in w], torch.zeros(4), 0, 0.2, 0.01, 0.0, 0.0, 0.0, 1.0)


def test_nominal_action_reproduces_the_reference(fixture):
    from gym_rotor_amd import QuadConstants, RolloutStorage
    k = QuadConstants()
    for name, n_agents, agent in (("mono", 1, 0), ("modul0", 2, 0), ("modul1", 2, 1), ("mono_sat", 1, 0)):
        c = case(fixture, name)
        env = SimpleNamespace(n_agents=n_agents, hover_force=k.hover_force, min_force=k.min_force, max_force=k.max_force, device="cpu")
        got = RolloutStorage.nominal_action(env, agent, max_action=c["co"]["max_action"])
        assert got.dtype == torch.float32 and tuple(got.shape) == c["nominal"].shape
        assert np.array_equal(got.numpy(), c["nominal"].astype(np.float32)), name
    assert -1 < case(fixture, "mono")["nominal"][0] < 0 and case(fixture, "modul1")["nominal"][0] == 0
