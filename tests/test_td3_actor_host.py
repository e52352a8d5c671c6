"""The TD3 actor half on the device (qr_dpg_actor_grad, qr_soft_update, td3.dpg_actor_grad / td3_actor_loss / soft_update) without a
GPU: the float64 restatement of tests/td3_actor_ref.py against the reference's own autograd (tests/golden/td3_actor.npz,
tools/gen_golden_td3_actor.py), the ReLU margin and the clamp shares of the fixture, the C-ABI struct layouts, every argument error
of the three C entries and of the Python helpers, and the soft update's float32 rule against CPU torch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import td3_actor_ref as R  # noqa: E402
from td3_actor_ref import ACTOR_NAMES, CASES, Q1_NAMES  # noqa: E402
from test_td3_critic_host import _Actor, _Twin  # noqa: E402

SHAPES = {"mono": (23, 16, 4, 62), "dtde0": (15, 16, 4, 62), "dtde1": (3, 4, 1, 62), "h64": (23, 16, 4, 64), "h5": (23, 16, 4, 5),
          "h1": (23, 16, 4, 1), "noreg": (23, 16, 4, 62), "sat": (23, 16, 4, 62)}
NULL, KIND, SIZE, ALIGN = -1, -2, -3, -4


@pytest.fixture(scope="module")
def fixture():
    return R.load()


def _w(c):
    return [c["a_" + n] for n in ACTOR_NAMES], [c["c_" + n] for n in Q1_NAMES]


def test_fixture_holds_the_cases(fixture):
    assert tuple(str(n) for n in fixture["cases"]) == CASES
    assert os.path.getsize(R.GOLDEN) <= 1_000_000
    for name in CASES:
        c = R.case(fixture, name)
        D, H, A, HC = SHAPES[name]
        assert c["obs"].shape == (130, D) and c["obs_next"].shape == (130, D) and c["noise"].shape == (D,) and c["nominal"].shape == (A,)
        assert c["a_fc1_w"].shape == (H, D) and c["a_fc3_w"].shape == (A, H) and c["c_fc1_w"].shape == (HC, D + A) and c["c_fc3_w"].shape == (1, HC)
        assert c["g_fc1_w"].dtype == np.float64 and c["obs"].dtype == np.float32 and c["a_fc2_w"].dtype == np.float32
    assert R.case(fixture, "mono")["lam"] == (0.4, 0.3, 0.6) and R.case(fixture, "noreg")["lam"] == (0.0, 0.0, 0.0)
    assert R.case(fixture, "sat")["max_action"] == 0.5 and R.case(fixture, "mono")["max_action"] == 1.0


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(fixture, name):
    c = R.case(fixture, name)
    w, q = _w(c)
    stats, grads = R.dpg_actor_grad_f64(w, q, c["obs"], c["obs_next"], c["noise"], c["nominal"], c["lam"], c["max_action"])
    for n in ACTOR_NAMES:
        want = c["g_" + n]
        assert np.abs(grads[n] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), n
    for got, k in zip(stats, R.STATS):
        assert abs(got - float(c[k])) <= 1e-12 * max(1.0, abs(float(c[k]))), k


@pytest.mark.parametrize("name", CASES)
def test_every_case_keeps_the_relu_margin(fixture, name):
    c = R.case(fixture, name)
    w, q = _w(c)
    m, per_unit = R.margins(w, q, c["obs"], c["obs_next"], c["noise"], c["max_action"])
    assert m >= R.MARGIN == 2e-5
    assert abs(m - float(c["min_abs_z"])) <= 1e-12 * max(1.0, m)   # the helper returns the stored minimum
    # the device forms `a` with a tanh that is off by up to 2e-7: the critic's fc1 pre-activation of unit u moves by at most
    # 2e-7 sum_a |fc1_w[u, D + a]|, which must stay below a tenth of the stored margin
    D = c["obs"].shape[1]
    shift = R.TANH_FAST_ERR * np.abs(q[0].astype(np.float64)[:, D:]).sum(1)
    assert shift.shape == per_unit.shape and (shift < 0.1 * float(c["min_abs_z"])).all(), float(shift.max())


def test_sat_clamps_a_fifth_and_leaves_a_fifth(fixture):
    c = R.case(fixture, "sat")
    for share, dist in R.clamp_shares(_w(c)[0], c["obs"], c["obs_next"], c["max_action"]):
        assert 0.2 <= share <= 0.8 and dist >= 1e-4
    assert 0.2 <= float(c["clamp_share"]) <= 0.8
    for name in CASES[:-1]:
        assert float(R.case(fixture, name)["clamp_share"]) == 0.0


STRUCTS = ("QrDpgGrad", "QrSoftUpdate")


def test_structs_mirror_the_header(tmp_path):
    from gym_rotor_amd import _lib as L
    lines = []
    for sname in STRUCTS:
        lines.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        lines += [f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));' for f, _ in getattr(L, sname)._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for sname in STRUCTS:
        ct = getattr(L, sname)
        assert int(out[sname]) == C.sizeof(ct)
        for f, _ in ct._fields_:
            assert int(out[f"{sname}.{f}"]) == getattr(ct, f).offset, (sname, f)
    lib = L.load()
    assert {"qr_dpg_actor_grad", "qr_dpg_actor_workspace_bytes", "qr_soft_update"} <= set(L.SYMBOLS) and hasattr(lib, "qr_soft_update")
    assert L.DPG_GRAD_NAMES == ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b") and L.SOFT_UPDATE_MAX == 24


def _fake(actor=(23, 16, 4), hidden=62, batch=130):
    """(QrActor, QrQCritic, QrTransitions, QrDpgGrad) that pass every check but the last, on fake device addresses (never touched: the
    workspace is one byte short, so every case returns before a launch)."""
    from gym_rotor_amd import _lib as L
    p = L.QrActor()
    for k, n in enumerate(("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std")):
        setattr(p, n, 0x900000 + 0x1000 * k)
    p.obs_dim, p.hidden_dim, p.action_dim, p.squash = *actor, L.ACTOR_TANH_MEAN
    q = L.QrQCritic()
    for k, n in enumerate(L.TWINQ_GRAD_NAMES):
        setattr(q, n, 0x10000 + 0x1000 * k)
    q.obs_dim, q.action_dim, q.hidden_dim, q.reserved0 = actor[0], actor[2], hidden, 0
    b = L.QrTransitions()
    for k, n in enumerate(("obs", "obs_next", "action", "reward", "done", "index")):
        setattr(b, n, 0x100000 + 0x10000 * k)
    b.batch, b.rows, b.row_stride, b.col_offset, b.reward_stride, b.done_stride = batch, 130, 4, 0, 1, 1
    g = L.QrDpgGrad(*[0x800000 + 0x1000 * k for k in range(7)], 0x300000, 0x310000, 0x400000)
    g.workspace_bytes = L.load().qr_dpg_actor_workspace_bytes(*actor, hidden, batch, 0) - 1
    g.lam_T, g.lam_S, g.lam_M, g.max_action, g.max_workgroups, g.reserved0 = 0.4, 0.3, 0.6, 1.0, 0, 0
    return {"p": p, "q": q, "b": b, "g": g}


def _ref(x):
    return None if x is None else C.byref(x)


def test_dpg_actor_grad_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()

    def call(s):
        return lib.qr_dpg_actor_grad(_ref(s["p"]), _ref(s["q"]), _ref(s["b"]), _ref(s["g"]), None)

    assert call(_fake()) == SIZE                                   # every other check passes: only the workspace is one byte short
    for k in "pqbg":
        assert call({**_fake(), k: None}) == NULL

    def expect(code, what, fake=(), **edit):
        s = _fake(*fake)
        for k, v in edit.items():
            setattr(s[k[0]], k[2:], v)
        assert call(s) == code, (what, edit)

    for n in L.DPG_GRAD_NAMES:
        expect(NULL, "actor weight", **{"p_" + n: None})
        expect(NULL, "gradient", **{"g_" + n: None})
    for n in Q1_NAMES:
        expect(NULL, "Q1 weight", **{"q_" + n: None})
    for n in ("stats", "workspace", "noise", "nominal"):
        expect(NULL, n, **{"g_" + n: None})
    for n in ("obs", "obs_next"):
        expect(NULL, n, **{"b_" + n: None})
    # what is optional (SIZE = reached the workspace check): Q2, log_std, index, the unread tensors, and the inputs of a term whose lam is 0
    for edit in (dict(q_fc4_w=None, q_fc4_b=None, q_fc5_w=None, q_fc5_b=None, q_fc6_w=None, q_fc6_b=None), dict(p_log_std=None),
                 dict(b_index=None), dict(b_action=None, b_reward=None, b_done=None, b_row_stride=0, b_reward_stride=0),
                 dict(g_lam_T=0.0, b_obs_next=None), dict(g_lam_S=0.0, g_noise=None), dict(g_lam_M=0.0, g_nominal=None),
                 dict(g_lam_T=0.0, g_lam_S=0.0, g_lam_M=0.0, b_obs_next=None, g_noise=None, g_nominal=None), dict(g_max_action=0.0)):
        expect(SIZE, "optional pointers and legal values", **edit)
    for fake in (((15, 16, 4), 62), ((3, 4, 1), 62), ((23, 16, 4), 1), ((23, 16, 4), 64), ((3, 4, 1), 5, 1 << 33)):
        expect(SIZE, "legal sizes", fake=fake)
    expect(KIND, "SAC form", p_squash=L.ACTOR_TANH_SAMPLE)
    expect(KIND, "log_std head", p_log_std_w=0x990000, p_log_std_b=0x991000)
    big = dict(g_workspace_bytes=1 << 40)
    for dims in ((23, 16, 3), (23, 8, 4), (24, 16, 4), (15, 16, 4), (3, 4, 1), (0, 0, 0)):
        expect(SIZE, "actor sizes, or an actor that does not fit the critic", p_obs_dim=dims[0], p_hidden_dim=dims[1], p_action_dim=dims[2], **big)
    for D, A, H in ((15, 4, 62), (23, 1, 62), (23, 4, 0), (23, 4, 65), (23, 4, -1)):
        expect(SIZE, "critic widths, or a critic that does not fit the actor", q_obs_dim=D, q_action_dim=A, q_hidden_dim=H, **big)
    for edit in (dict(b_batch=0), dict(b_batch=-5), dict(b_rows=0), dict(g_max_workgroups=-1), dict(q_reserved0=1), dict(g_reserved0=1),
                 dict(g_max_action=-0.5), dict(g_max_action=float("nan")), dict(g_max_action=float("inf")), dict(g_lam_T=-0.1),
                 dict(g_lam_S=float("nan")), dict(g_lam_M=float("inf"))):
        expect(SIZE, "sizes and coefficients", **big, **edit)
    for edit in (dict(b_obs=0x100002), dict(b_obs_next=0x110001), dict(g_fc2_w=0x802001), dict(p_mean_b=0x905002), dict(q_fc3_b=0x15002),
                 dict(g_stats=0x806001), dict(g_noise=0x300002), dict(g_nominal=0x310003), dict(b_index=0x150004), dict(g_workspace=0x400004)):
        expect(ALIGN, "alignment", **big, **edit)
    # the workspace: min(tiles, max_workgroups or 1024) partial vectors of float64 — the six tensors, then five sums
    ws = lib.qr_dpg_actor_workspace_bytes
    np_mono, np_d0, np_d1 = 23 * 16 + 16 + 256 + 16 + 64 + 4 + 5, 15 * 16 + 16 + 256 + 16 + 64 + 4 + 5, 12 + 4 + 16 + 4 + 4 + 1 + 5
    assert ws(23, 16, 4, 62, 130, 0) == 3 * np_mono * 8 and ws(23, 16, 4, 62, 130, 2) == 2 * np_mono * 8 and ws(23, 16, 4, 1, 1, 0) == np_mono * 8
    assert ws(15, 16, 4, 64, 64 * 5000, 0) == 1024 * np_d0 * 8 and ws(3, 4, 1, 62, 200, 3) == 3 * np_d1 * 8
    for bad in ((23, 16, 4, 62, 0, 0), (23, 16, 4, 62, 10, -1), (23, 16, 4, 0, 10, 0), (23, 16, 4, 65, 10, 0), (24, 16, 4, 62, 10, 0), (3, 4, 4, 62, 10, 0)):
        assert ws(*bad) == SIZE, bad


def test_soft_update_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()

    def fake(n=18):
        u = L.QrSoftUpdate()
        u.n_tensors, u.reserved0, u.tau = n, 0, 0.005
        for k in range(n):
            u.target[k], u.param[k], u.count[k] = 0x100000 + 0x1000 * k, 0x200000 + 0x1000 * k, 10 + k
        return u

    assert lib.qr_soft_update(None, None) == NULL
    for n in (0, 25, -1):
        u = fake(1)
        u.n_tensors = n
        assert lib.qr_soft_update(C.byref(u), None) == SIZE, n
    for field, k, value, code in (("count", 3, 0, SIZE), ("count", 17, -2, SIZE), ("target", 5, None, NULL), ("param", 0, None, NULL),
                                  ("target", 2, 0x100001, ALIGN), ("param", 17, 0x200002, ALIGN), ("target", 4, 0x200000 + 0x4000, SIZE)):
        u = fake()
        getattr(u, field)[k] = value
        assert lib.qr_soft_update(C.byref(u), None) == code, (field, k, value)
    for tau in (-0.001, 1.001, float("nan"), float("inf")):
        u = fake()
        u.tau = tau
        assert lib.qr_soft_update(C.byref(u), None) == SIZE, tau
    u = fake()
    u.reserved0 = 1
    assert lib.qr_soft_update(C.byref(u), None) == SIZE
    u = fake()
    u.target[20], u.count[20] = None, 0                             # entries past n_tensors are not looked at: the only failure left is none
    u.n_tensors = 0
    assert lib.qr_soft_update(C.byref(u), None) == SIZE


# ---------------------------------------------------------------------------------------------------------------------------
# the Python helpers
# ---------------------------------------------------------------------------------------------------------------------------
def test_python_helpers_refuse_bad_arguments():
    from gym_rotor_amd import ActorParams, QCriticParams, ReplayBuffer, dpg_actor_grad, soft_update, td3_actor_loss
    from gym_rotor_amd import _lib as L
    q = QCriticParams.from_module(_Twin(), 4)
    actor = ActorParams.from_td3_module(_Actor(), 0.0)
    obs, nxt, noise, nominal = torch.zeros(130, 23), torch.zeros(130, 23), torch.zeros(23), torch.zeros(4)
    ok = dict(noise=noise, nominal=nominal)
    with pytest.raises(RuntimeError, match="GPU only"):             # every check passes on CPU tensors; there is no CPU kernel
        dpg_actor_grad(actor, q, obs, nxt, None, **ok)
    bad = [
        (dict(actor=ActorParams.from_td3_module(_Actor(15, 16, 4), 0.0)), "the critic reads"),
        (dict(actor=ActorParams.from_td3_module(_Actor(23, 8, 4), 0.0)), "not among"),
        (dict(actor=ActorParams(*[getattr(actor, n) for n in L.DPG_GRAD_NAMES], None, torch.zeros(4, 16), torch.zeros(4))), "MLP_Actor_TD3"),
        (dict(obs=torch.zeros(130, 22)), "obs must be"), (dict(obs=torch.zeros(130, 23, dtype=torch.float64)), "obs must be"),
        (dict(obs_next=None), "obs_next must be"), (dict(obs_next=torch.zeros(129, 23)), "130 rows"),
        (dict(noise=None), "noise"), (dict(nominal=None), "nominal"), (dict(noise=torch.zeros(22)), "noise must be"),
        (dict(nominal=torch.zeros(4, dtype=torch.float64)), "nominal must be"),
        (dict(index=torch.zeros(5, dtype=torch.int32)), "index must be"), (dict(lam_T=-1.0), "lam_T"), (dict(lam_S=float("nan")), "lam_S"),
        (dict(max_action=float("inf")), "max_action"), (dict(stats=torch.zeros(3)), "stats must be"),
        (dict(grads={n: torch.zeros(1) for n in L.DPG_GRAD_NAMES}), "grads"),
    ]
    for edit, match in bad:
        kw = dict(actor=actor, critic=q, obs=obs, obs_next=nxt, index=None, **ok)
        kw.update(edit)
        a, c, o, n, i = (kw.pop(k) for k in ("actor", "critic", "obs", "obs_next", "index"))
        with pytest.raises(ValueError, match=match):
            dpg_actor_grad(a, c, o, n, i, **kw)
    with pytest.raises(RuntimeError, match="GPU only"):             # a term whose lam is 0 needs none of its inputs
        dpg_actor_grad(actor, q, obs, None, None, lam_T=0.0, lam_S=0.0, lam_M=0.0)
    # td3_actor_loss: the module's .grad tensors are created, then the same checks
    m, tw = _Actor(), _Twin()
    buf = ReplayBuffer(130, [23], [4], "cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        td3_actor_loss(m, tw, buf, 0, None, noise=noise, nominal=nominal)
    assert all(p.grad is not None and p.grad.shape == p.shape for p in m.parameters()) and ("actor", 0, 130, 0) in buf._cache
    with pytest.raises(ValueError, match="noise"):
        td3_actor_loss(m, tw, buf, 0, None, nominal=nominal)
    # soft_update
    a, b = _Actor(), _Actor()
    with pytest.raises(RuntimeError, match="GPU only"):
        soft_update([_Twin(), a], [_Twin(), b], 0.005)
    for args, match in ((([a], [b, b]), "pairs"), (([_Twin(), _Twin(), a], [_Twin(), _Twin(), b]), "pairs"), (([], []), "pairs"),
                        ((a, b, 1.5), "tau"), ((a, b, -0.1), "tau"), ((a, b, float("nan")), "tau"), ((a, a), "its own param"),
                        (([torch.zeros(3)], [torch.zeros(4)]), "elements"), (([torch.zeros(3, dtype=torch.float64)], [torch.zeros(3)]), "float32"),
                        (([torch.zeros(4, 2).T], [torch.zeros(2, 4)]), "contiguous")):
        with pytest.raises(ValueError, match=match):
            soft_update(*args)


@pytest.mark.parametrize("tau", (0.0, 0.005, 0.5, 1.0))
def test_soft_update_rule_is_torch_float32_bit_for_bit(tau):
    g = torch.Generator().manual_seed(int(tau * 1000) + 3)
    for shape, scale in (((62, 27), 1.0), ((62, 62), 1e-3), ((1, 62), 1e3), ((4099,), 1.0)):
        p, t = torch.randn(shape, generator=g) * scale, torch.randn(shape, generator=g) * scale
        want = tau * p + (1 - tau) * t                                  # td3.py:207-211
        got = R.soft_update_f32(p.numpy(), t.numpy(), tau)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32)), (tau, shape)
    if tau == 0.0:
        assert np.array_equal(R.soft_update_f32(p.numpy(), t.numpy(), tau), t.numpy())
    if tau == 1.0:
        assert np.array_equal(R.soft_update_f32(p.numpy(), t.numpy(), tau), p.numpy())
