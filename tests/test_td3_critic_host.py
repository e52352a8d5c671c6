"""The TD3 critic half on the device (qr_twinq_target, qr_twinq_grad, td3.td3_target / twinq_grad / td3_critic_loss, ReplayBuffer)
without a GPU: the float64 restatement of tests/td3_ref.py against the reference's own autograd (tests/golden/td3_critic.npz,
tools/gen_golden_td3_critic.py), the ReLU margin of every fixture case, the C-ABI struct layouts, every argument error of the two C
entries and of the Python helpers, and the replay buffer's ring rule, order, obs_next rule, wrap-around and sampling."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import td3_ref  # noqa: E402
from td3_ref import ACTOR_NAMES, NAMES  # noqa: E402

CASES = ("mono", "dtde0", "dtde1", "h64", "h5", "h1", "w28", "sat", "nonoise")
SHAPES = {"mono": (23, 4, 62), "dtde0": (15, 4, 62), "dtde1": (3, 1, 62), "h64": (23, 4, 64), "h5": (23, 4, 5), "h1": (23, 4, 1),
          "w28": (24, 4, 62), "sat": (23, 4, 5), "nonoise": (23, 4, 5)}


@pytest.fixture(scope="module")
def fixture():
    return td3_ref.load()


def test_fixture_holds_the_cases(fixture):
    assert tuple(str(n) for n in fixture["cases"]) == CASES
    assert os.path.getsize(td3_ref.GOLDEN) <= 1_000_000
    for name in CASES:
        c = td3_ref.case(fixture, name)
        D, A, H = SHAPES[name]
        assert c["obs"].shape == (130, D) and c["obs_next"].shape == (130, D) and c["action"].shape == (130, A)
        assert c["c_fc1_w"].shape == (H, D + A) and c["c_fc5_w"].shape == (H, H) and c["g_fc6_w"].shape == (1, H)
        assert c["y"].dtype == np.float64 and c["g_fc1_w"].dtype == np.float64 and c["obs"].dtype == np.float32
        assert ("eps" in c) == (name != "nonoise") and ("a_fc1_w" in c) == (name != "w28")
    sat = td3_ref.case(fixture, "sat")
    raw = float(sat["target_noise"]) * sat["eps"].astype(np.float64)
    mean = td3_ref.actor_forward([sat["a_" + n].astype(np.float64) for n in ACTOR_NAMES], sat["obs_next"].astype(np.float64))
    assert (np.abs(raw) > sat["noise_clip"]).any(1).sum() >= 10                                              # the noise clamp is active
    assert (np.abs(mean + np.clip(raw, -0.5, 0.5)) > sat["max_action"]).any(1).sum() >= 10                   # the action clamp is active
    assert sat["done"].sum() >= 10 and np.abs(sat["a_next"]).max() == 1.0


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(fixture, name):
    c = td3_ref.case(fixture, name)
    a_next, y = td3_ref.td3_target_f64(c)
    for got, want, what in ((a_next, c["a_next"], "a_next"), (y, c["y"], "y")):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), what
    loss, m1, m2, grads = td3_ref.twinq_grad_f64([c["c_" + n] for n in NAMES], c["obs"], c["action"], c["y"])
    for n in NAMES:
        want = c["g_" + n]
        assert np.abs(grads[n].reshape(want.shape) - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), n
    for got, k in ((loss, "loss"), (m1, "mse1"), (m2, "mse2")):
        assert abs(got - float(c[k])) <= 1e-12 * max(1.0, abs(float(c[k]))), k


@pytest.mark.parametrize("name", CASES)
def test_every_case_keeps_the_relu_margin(fixture, name):
    c = td3_ref.case(fixture, name)
    m = td3_ref.margin([c["c_" + n] for n in NAMES], c["obs"], c["action"])
    assert m >= td3_ref.MARGIN == 2e-5
    assert abs(m - float(c["min_abs_z"])) <= 1e-12 * max(1.0, m)   # the helper returns the stored minimum


STRUCTS = ("QrQCritic", "QrTransitions", "QrTd3Target", "QrTwinQGrad")


def test_structs_mirror_the_header(tmp_path):
    from gym_rotor_amd import _lib as L
    lines = []
    for sname in STRUCTS:
        lines.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        lines += [f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));' for f, _ in getattr(L, sname)._fields_]
    lines.append('printf("abi %d\\n", QR_ABI_VERSION);')
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
    assert {"qr_twinq_target", "qr_twinq_grad", "qr_twinq_workspace_bytes"} <= set(L.SYMBOLS) and hasattr(lib, "qr_twinq_grad")
    assert L.TWINQ_GRAD_NAMES == NAMES and [f for f, _ in L.QrTwinQGrad._fields_][:13] == list(NAMES) + ["stats"]
    assert int(out["abi"]) == L.ABI_VERSION


def _fake(obs_dim=23, action_dim=4, hidden=62, batch=130, actor=(23, 16, 4)):
    """(QrActor, QrQCritic, QrTransitions, QrTd3Target, QrTwinQGrad) that pass every check, on fake device addresses (never touched:
    every case of the tests below returns before a launch — the twin-Q workspace is one byte short, the target's batch is refused
    last through y = NULL unless the case edits something else)."""
    from gym_rotor_amd import _lib as L
    p = L.QrActor()
    for k, n in enumerate(("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std")):
        setattr(p, n, 0x900000 + 0x1000 * k)
    p.obs_dim, p.hidden_dim, p.action_dim, p.squash = *actor, L.ACTOR_TANH_MEAN
    q = L.QrQCritic()
    for k, n in enumerate(NAMES):
        setattr(q, n, 0x10000 + 0x1000 * k)
    q.obs_dim, q.action_dim, q.hidden_dim, q.reserved0 = obs_dim, action_dim, hidden, 0
    b = L.QrTransitions()
    for k, n in enumerate(("obs", "obs_next", "action", "reward", "done", "index")):
        setattr(b, n, 0x100000 + 0x10000 * k)
    b.batch, b.rows, b.row_stride, b.col_offset, b.reward_stride, b.done_stride = batch, 130, action_dim, 0, 1, 1
    t = L.QrTd3Target(0x200000, 0x210000, 0x220000, 0.99, 0.2, 0.5, 1.0)
    g = L.QrTwinQGrad(*[0x800000 + 0x1000 * k for k in range(13)], 0x300000, 0x400000)
    g.workspace_bytes = L.load().qr_twinq_workspace_bytes(obs_dim + action_dim, hidden, batch, 0) - 1
    g.max_workgroups, g.reserved0 = 0, 0
    return {"p": p, "q": q, "b": b, "t": t, "g": g}


NULL, KIND, SIZE, ALIGN = -1, -2, -3, -4


def _ref(x):
    return None if x is None else C.byref(x)


def test_twinq_grad_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()

    def call(s):
        return lib.qr_twinq_grad(_ref(s["q"]), _ref(s["b"]), _ref(s["g"]), None)

    s = _fake()
    assert call(s) == SIZE                                         # every other check passes: only the workspace is one byte short
    for k in "qbg":
        assert call({**_fake(), k: None}) == NULL

    def expect(code, what, fake=(), **edit):
        s = _fake(*fake)
        for k, v in edit.items():
            setattr(s[k[0]], k[2:], v)
        assert call(s) == code, (what, edit)

    for n in NAMES:
        expect(NULL, "weight", **{"q_" + n: None})
        expect(NULL, "gradient", **{"g_" + n: None})
    for n in ("stats", "y", "workspace"):
        expect(NULL, n, **{"g_" + n: None})
    for n in ("obs", "action"):
        expect(NULL, n, **{"b_" + n: None})
    for edit in (dict(b_index=None), dict(b_obs_next=None, b_reward=None, b_done=None), dict(b_row_stride=9, b_col_offset=5)):
        expect(SIZE, "optional pointers and legal sizes", **edit)   # (SIZE = reached the workspace check)
    for fake in ((24, 4, 62), (3, 1, 62), (1, 1, 1), (23, 4, 64), (27, 1, 64)):
        expect(SIZE, "legal widths", fake=fake)
    for D, A, H in ((25, 4, 62), (23, 6, 62), (0, 4, 62), (23, 0, 62), (-1, 4, 62), (23, 4, 0), (23, 4, 65), (23, 4, -3)):
        expect(SIZE, "widths", q_obs_dim=D, q_action_dim=A, q_hidden_dim=H, g_workspace_bytes=1 << 40)   # 29 wide, hidden 65, ...
    for edit in (dict(b_batch=0), dict(b_batch=-5), dict(b_rows=0), dict(b_row_stride=0), dict(b_col_offset=-1), dict(b_col_offset=1),
                 dict(g_max_workgroups=-1), dict(q_reserved0=1), dict(g_reserved0=1)):
        expect(SIZE, "sizes", g_workspace_bytes=1 << 40, **edit)
    for edit in (dict(b_obs=0x100002), dict(b_action=0x120001), dict(g_fc5_w=0x800001), dict(q_fc6_b=0x15002), dict(g_y=0x300002),
                 dict(g_stats=0x80c001), dict(b_index=0x150004), dict(g_workspace=0x400004)):
        expect(ALIGN, "alignment", g_workspace_bytes=1 << 40, **edit)
    # the workspace size: two rows of min(tiles, max_workgroups or 512) partial vectors of float64
    ws = lib.qr_twinq_workspace_bytes
    np_mono = 62 * 27 + 62 + 62 * 62 + 62 + 62 + 1 + 2
    assert np_mono == 5707
    assert ws(27, 62, 130, 0) == 2 * 3 * np_mono * 8 and ws(27, 62, 130, 2) == 2 * 2 * np_mono * 8 and ws(27, 62, 1, 0) == 2 * np_mono * 8
    assert ws(27, 62, 64 * 5000, 0) == 2 * 512 * np_mono * 8 and ws(4, 5, 200, 3) == 2 * 3 * (20 + 5 + 25 + 5 + 5 + 1 + 2) * 8
    assert ws(28, 64, 64, 0) == 2 * (64 * 28 + 64 + 64 * 64 + 64 + 64 + 1 + 2) * 8 and ws(2, 1, 1, 0) == 2 * 9 * 8
    for bad in ((27, 62, 0, 0), (27, 62, 10, -1), (1, 62, 10, 0), (29, 62, 10, 0), (27, 0, 10, 0), (27, 65, 10, 0)):
        assert ws(*bad) == SIZE, bad


def test_td3_target_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()

    def call(s):
        return lib.qr_twinq_target(_ref(s["p"]), _ref(s["q"]), _ref(s["b"]), _ref(s["t"]), None)

    def expect(code, what, fake=(), **edit):
        s = _fake(*fake)
        s["t"].y = None                                            # the last pointer check: every legal case ends here, before a launch
        for k, v in edit.items():
            if k == "p":
                s["p"] = v
            else:
                setattr(s[k[0]], k[2:], v)
        assert call(s) == code, (what, edit)

    expect(NULL, "everything else is legal")
    for k in "qbt":
        assert call({**_fake(), k: None}) == NULL
    for fake in ((15, 4, 62, 130, (15, 16, 4)), (3, 1, 62, 130, (3, 4, 1)), (23, 4, 1, 1), (23, 4, 64, 1 << 33)):
        expect(NULL, "legal sizes", fake=fake)
    expect(NULL, "no actor: action_next", p=None)
    expect(NULL, "no actor and no action_next", p=None, t_action_next=None, t_y=0x220000)
    expect(NULL, "eps is optional", t_eps=None)
    expect(NULL, "log_std is unread", p_log_std=None)
    expect(NULL, "obs and action are unread", b_obs=None, b_action=None, b_row_stride=0)
    for n in NAMES:
        expect(NULL, "weight", t_y=0x220000, **{"q_" + n: None})
    for n in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b"):
        expect(NULL, "actor weight", t_y=0x220000, **{"p_" + n: None})
    for n in ("obs_next", "reward", "done"):
        expect(NULL, n, t_y=0x220000, **{"b_" + n: None})
    expect(KIND, "SAC form", p_squash=L.ACTOR_TANH_SAMPLE)
    expect(KIND, "log_std head", p_log_std_w=0x990000, p_log_std_b=0x991000)
    for D, A, H in ((25, 4, 62), (23, 6, 62), (0, 4, 62), (23, 0, 62), (23, 4, 0), (23, 4, 65)):
        expect(SIZE, "widths", q_obs_dim=D, q_action_dim=A, q_hidden_dim=H)
    for dims in ((23, 16, 3), (23, 8, 4), (24, 16, 4), (15, 16, 4), (3, 4, 1)):
        expect(SIZE, "actor sizes, or an actor that does not fit the critic", p_obs_dim=dims[0], p_hidden_dim=dims[1], p_action_dim=dims[2])
    expect(SIZE, "actor 15 -> 4 under a 15 + 1 critic", fake=(15, 1, 62, 130, (15, 16, 4)))
    for edit in (dict(b_batch=0), dict(b_rows=0), dict(b_reward_stride=0), dict(b_done_stride=-1), dict(q_reserved0=7),
                 dict(t_noise_clip=-0.5), dict(t_max_action=float("nan")), dict(t_max_action=float("inf"))):
        expect(SIZE, "sizes", **edit)
    for edit in (dict(b_obs_next=0x110002), dict(b_reward=0x130001), dict(b_done=0x140003), dict(t_eps=0x200002), dict(t_y=0x220001),
                 dict(q_fc4_w=0x13002), dict(p_mean_w=0x904001), dict(b_index=0x150004)):
        expect(ALIGN, "alignment", **{"t_y": 0x220000, **edit})


# ---------------------------------------------------------------------------------------------------------------------------
# the Python helpers
# ---------------------------------------------------------------------------------------------------------------------------
class _Twin(torch.nn.Module):
    def __init__(self, din=27, hidden=62):
        super().__init__()
        for k, (i, o) in enumerate(((din, hidden), (hidden, hidden), (hidden, 1)) * 2, 1):
            setattr(self, f"fc{k}", torch.nn.Linear(i, o))


class _Actor(torch.nn.Module):
    def __init__(self, D=23, H=16, A=4):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, A)


def test_qcritic_params_checks():
    from gym_rotor_amd import QCriticParams
    q = QCriticParams.from_module(_Twin(), 4)
    assert q.dims == (23, 4, 62) and q.shapes["fc4_w"] == (62, 27) and q.shapes["fc6_b"] == (1,) and tuple(q.shapes) == NAMES
    c = q.as_c()
    assert (c.obs_dim, c.action_dim, c.hidden_dim, c.reserved0) == (23, 4, 62, 0) and c.fc5_w == q.fc5_w.data_ptr()
    assert QCriticParams.from_module(_Twin(28, 64), 4).dims == (24, 4, 64) and QCriticParams.from_module(_Twin(4, 1), 1).dims == (3, 1, 1)
    for din, hidden, A in ((29, 62, 4), (27, 65, 4), (27, 62, 0), (27, 62, 27), (1, 62, 1)):
        with pytest.raises(ValueError):
            QCriticParams.from_module(_Twin(din, hidden), A)
    for name, bad in (("fc5_w", torch.zeros(62, 61)), ("fc2_b", torch.zeros(62, dtype=torch.float64)), ("fc6_w", torch.zeros(62, 2)[:, :1].T)):
        m = _Twin()
        args = {n: getattr(getattr(m, n[:3]), "weight" if n.endswith("w") else "bias").data for n in NAMES}
        args[name] = bad
        with pytest.raises(ValueError, match=name):
            QCriticParams(**args, action_dim=4)


def test_python_helpers_refuse_bad_arguments():
    from gym_rotor_amd import ActorParams, QCriticParams, td3_target, twinq_grad
    q = QCriticParams.from_module(_Twin(), 4)
    actor = ActorParams.from_td3_module(_Actor(), 0.0)
    t = {"obs": torch.zeros(10, 23), "act": torch.zeros(10, 4), "rwd": torch.zeros(10), "obs_next": torch.zeros(10, 23), "done": torch.zeros(10)}
    idx = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        td3_target(actor, q, t, 0, idx)
    with pytest.raises(RuntimeError, match="GPU only"):
        twinq_grad(q, t["obs"], t["act"], torch.zeros(5), idx)
    bad_t = [("obs_next", torch.zeros(10, 22)), ("obs_next", torch.zeros(10, 23, dtype=torch.float64)), ("rwd", torch.zeros(9)),
             ("done", torch.zeros(10, dtype=torch.bool)), ("rwd", torch.zeros(10, 2)), ("done", None)]
    for k, v in bad_t:
        with pytest.raises(ValueError, match=k):
            td3_target(actor, q, {**t, k: v}, 0, idx)
    for kw, pat in ((dict(index=idx.int()), "index"), (dict(index=idx, noise=torch.zeros(5, 3)), "noise"), (dict(index=idx, noise=torch.zeros(10, 4)), "noise"),
                    (dict(index=idx, out=torch.zeros(4)), "out"), (dict(index=idx, out=torch.zeros(5, dtype=torch.float64)), "out")):
        with pytest.raises(ValueError, match=pat):
            td3_target(actor, q, t, 0, **kw)
    with pytest.raises(ValueError, match="action_next"):
        td3_target(None, q, t, 0, idx)
    with pytest.raises(ValueError, match="action_next"):
        td3_target(None, q, t, 0, idx, action_next=torch.zeros(5, 3))
    with pytest.raises(ValueError, match="the critic reads"):
        td3_target(ActorParams.from_td3_module(_Actor(15, 16, 4), 0.0), q, t, 0, idx)
    with pytest.raises(ValueError, match="not among"):
        td3_target(ActorParams.from_td3_module(_Actor(23, 8, 4), 0.0), q, t, 0, idx)
    sac = ActorParams.from_td3_module(_Actor(), 0.0)
    sac.squash = 1
    with pytest.raises(ValueError, match="MLP_Actor_TD3"):
        td3_target(sac, q, t, 0, idx)
    half = ActorParams.from_td3_module(_Actor(), 0.0)
    half.fc2_w = half.fc2_w.double()
    with pytest.raises(ValueError, match="fc2_w"):
        td3_target(half, q, t, 0, idx)
    y = torch.zeros(5)
    for args, kw, pat in (((torch.zeros(10, 22), t["act"], y, idx), {}, "obs"), ((t["obs"], torch.zeros(9, 4), y, idx), {}, "action"),
                          ((t["obs"], torch.zeros(10, 3), y, idx), {}, "action"), ((t["obs"], torch.zeros(4, 10).T, y, idx), {}, "action"),
                          ((t["obs"], t["act"], torch.zeros(6), idx), {}, "y"), ((t["obs"], t["act"], y.double(), idx), {}, "y"),
                          ((t["obs"], t["act"], y, idx.float()), {}, "index"), ((t["obs"], t["act"], y, idx), dict(stats=torch.zeros(3)), "stats"),
                          ((t["obs"], t["act"], y, idx), dict(grads={}), "grads"),
                          ((t["obs"], t["act"], y, idx), dict(grads={n: torch.zeros(s) for n, s in q.shapes.items() if n != "fc4_b"}), "fc4_b")):
        with pytest.raises(ValueError, match=pat):
            twinq_grad(q, *args, **kw)
    from gym_rotor_amd.td3 import twinq_workspace_bytes
    assert twinq_workspace_bytes((23, 4, 62), 130) == 2 * 3 * 5707 * 8 and twinq_workspace_bytes((3, 1, 5), 200, 1) == 2 * 63 * 8
    with pytest.raises(ValueError):
        twinq_workspace_bytes((23, 4, 62), 0)
    with pytest.raises(ValueError):
        twinq_workspace_bytes((25, 4, 62), 10)
    assert hasattr(torch.ops.gym_rotor_amd, "qr_twinq_target") and hasattr(torch.ops.gym_rotor_amd, "qr_twinq_grad")
    w = [getattr(q, n) for n in NAMES]
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_twinq_grad(w, 4, t["obs"], t["act"], y, idx, [torch.zeros_like(x) for x in w], torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_twinq_target([], w, 4, t["obs_next"], t["rwd"], t["done"], idx, None, torch.zeros(5, 4), y, 0.99, 0.2, 0.5, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# ReplayBuffer
# ---------------------------------------------------------------------------------------------------------------------------
def cpu_storage(T=3, N=5, obs_dims=(23,), action_dims=(4,), seed=0, final_obs=True):
    """A hand-filled RolloutStorage on the CPU (the storage only reads these attributes of the env)."""
    from gym_rotor_amd import RolloutStorage
    env = SimpleNamespace(num_envs=N, device=torch.device("cpu"), n_agents=len(obs_dims), action_dim=sum(action_dims), obs_dims=list(obs_dims),
                          auto_reset=True, kind="coupled" if len(obs_dims) == 1 else "decoupled", obs_rows=True)
    st = RolloutStorage(env, T, list(action_dims), final_obs=final_obs)
    g = torch.Generator().manual_seed(seed)
    for o in st.obs:
        o.copy_(torch.rand(o.shape, generator=g))
    if st.final_obs is not None:
        for f in st.final_obs:
            f.copy_(torch.rand(f.shape, generator=g) + 10.0)   # recognisable
    st.act_all.copy_(torch.rand(st.act_all.shape, generator=g))
    st.reward.copy_(torch.rand(st.reward.shape, generator=g))
    return st


def test_replay_buffer_add_order_and_obs_next_rule():
    from gym_rotor_amd import ReplayBuffer
    st = cpu_storage(3, 5, (15, 3), (4, 1))
    st.done[1, 2, 0] = True        # env 2: agent 0 terminates in step 1 (agent 1 does not)
    st.truncated[0, 4] = True      # env 4: the time limit in step 0
    buf = ReplayBuffer(40, (15, 3), (4, 1), "cpu")
    buf.add(st)
    assert (buf.count, buf.current_size) == (15, 15)
    for k in range(2):
        for t in range(3):
            for n in range(5):
                i = t * 5 + n                                         # (t, n) order
                assert torch.equal(buf.obs[k][i], st.obs[k][t, n]) and torch.equal(buf.act[k][i], st.act[k][t, n])
                assert buf.rwd[k][i] == st.reward[t, n, k] and buf.done[k][i] == float(st.done[t, n, k])
                reset = (t, n) in ((1, 2), (0, 4))
                assert torch.equal(buf.obs_next[k][i], st.final_obs[k][t, n] if reset else st.obs[k][t + 1, n])
    assert buf.done[0].sum() == 1 and buf.done[1].sum() == 0 and buf.done[0].dtype == torch.float32   # agent k's own flag
    assert (buf.obs[0][15:] == 0).all()
    plain = cpu_storage(3, 5, (15, 3), (4, 1), final_obs=False)
    b2 = ReplayBuffer(15, (15, 3), (4, 1), "cpu")
    b2.add(plain)
    assert torch.equal(b2.obs_next[1], plain.obs[1][1:].reshape(15, 3)) and (b2.count, b2.current_size) == (0, 15)
    with pytest.raises(ValueError, match="does not fit"):
        ReplayBuffer(14, (15, 3), (4, 1), "cpu").add(st)
    with pytest.raises(ValueError, match="differ"):
        ReplayBuffer(40, (23,), (4,), "cpu").add(st)
    with pytest.raises(ValueError):
        ReplayBuffer(0, (23,), (4,), "cpu")


def test_replay_buffer_ring_rule_and_wrap_around():
    from gym_rotor_amd import ReplayBuffer
    cap = 40
    buf = ReplayBuffer(cap, (23,), (4,), "cpu")
    count, size = 0, 0
    mirror = torch.zeros(cap, 23)
    sts = [cpu_storage(3, 5, seed=seed) for seed in range(4)]
    for st in sts:                                                   # 4 x 15 transitions into 40 rows: the third wraps
        buf.add(st)
        for row in st.obs[0][:-1].reshape(15, 23):                   # the reference's store_transition, one transition at a time
            mirror[count] = row
            count = (count + 1) % cap
            size = min(size + 1, cap)
        assert (buf.count, buf.current_size) == (count, size)
    assert (count, size) == (20, 40) and torch.equal(buf.obs[0], mirror)
    a2, a3 = sts[2].act[0].reshape(15, 4), sts[3].act[0].reshape(15, 4)
    assert torch.equal(buf.act[0][30:40], a2[:10]) and torch.equal(buf.act[0][:5], a2[10:]) and torch.equal(buf.act[0][5:20], a3)


def test_replay_buffer_sample():
    from gym_rotor_amd import ReplayBuffer
    buf = ReplayBuffer(100, (23,), (4,), "cpu")
    buf.add(cpu_storage(3, 5))
    g = torch.Generator().manual_seed(3)
    idx = buf.sample(15, g)
    assert idx.dtype == torch.int64 and idx.shape == (15,) and sorted(idx.tolist()) == list(range(15))   # no repeats, below current_size
    idx = buf.sample(7, g)
    assert len(set(idx.tolist())) == 7 and int(idx.max()) < 15 and int(idx.min()) >= 0
    assert torch.equal(buf.sample(7, torch.Generator().manual_seed(5)), buf.sample(7, torch.Generator().manual_seed(5)))
    for bad in (0, 16):
        with pytest.raises(ValueError):
            buf.sample(bad)
