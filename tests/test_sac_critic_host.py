"""SAC's critic half on the device (qr_sac_target, sac.sac_target / sac_critic_loss) without a GPU: the float64 restatement of
tests/sac_ref.py against the reference's own modules (tests/golden/sac_critic.npz, tools/gen_golden_sac_critic.py), the properties the
fixture's cases are there for, the C-ABI struct layout, every argument error of the C entry and of the Python helpers, and the torch
op's registration.

The restatement is held to 1e-12 * max(1, |x|) in a', logp and y.  Measured on the committed fixture, worst |restatement - fixture|:
a' 1.1e-16, logp 7.1e-15 (sat; bound 5.1e-11), y 8.9e-16.  tanh is ONE function on both sides (sac_ref.tanh64: evaluated in long
double, rounded once): the reference's log(1 - a'^2 + 1e-6) multiplies one ulp of a' by 2e6 on a saturated component, and with
torch's tanh in the generator and NumPy's here, which differ by an ulp on some inputs, clamp and sat came out 2.2e-10 apart in logp."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sac_ref  # noqa: E402
from sac_ref import ACTOR_NAMES  # noqa: E402
from td3_ref import NAMES  # noqa: E402
import td3_ref  # noqa: E402

CASES = ("mono", "dtde0", "dtde1", "h64", "h5", "w28", "noeps", "clamp", "sat")
SHAPES = {"mono": (23, 4, 62), "dtde0": (15, 4, 62), "dtde1": (3, 1, 62), "h64": (23, 4, 64), "h5": (23, 4, 5), "w28": (24, 4, 62),
          "noeps": (23, 4, 62), "clamp": (23, 4, 62), "sat": (23, 4, 62)}
ACTORS = {"mono": (23, 16, 4), "dtde0": (15, 16, 4), "dtde1": (3, 4, 1)}
LIVE = ("mono", "dtde0", "dtde1")   # the cases with a live critic of their own: what sac_critic_loss's end-to-end test runs


@pytest.fixture(scope="module")
def fixture():
    return sac_ref.load()


def _heads(c):
    f = lambda x: np.asarray(x, dtype=np.float64)
    w = [f(c["a_" + n]) for n in ACTOR_NAMES]
    on = f(c["obs_next"])
    h = td3_ref.relu(td3_ref.relu(on @ w[0].T + w[1]) @ w[2].T + w[3])
    return h @ w[4].T + w[5], h @ w[6].T + w[7]     # mean, the UNCLAMPED log_std


def test_fixture_holds_the_cases(fixture):
    assert tuple(str(n) for n in fixture["cases"]) == CASES
    assert os.path.getsize(sac_ref.GOLDEN) <= 1_000_000
    for name in CASES:
        c = sac_ref.case(fixture, name)
        D, A, H = SHAPES[name]
        assert c["obs"].shape == (130, D) and c["obs_next"].shape == (130, D) and c["action"].shape == (130, A)
        assert c["t_fc1_w"].shape == (H, D + A) and c["t_fc5_w"].shape == (H, H) and c["t_fc6_w"].shape == (1, H)
        assert ("c_fc1_w" in c) == (name != "w28") and ("a_fc1_w" in c) == (name != "w28") and ("eps" in c) == (name != "noeps")
        assert c["y"].shape == (130,) and c["logp"].shape == (130,) and c["a_next"].shape == (130, A)
        assert c["y"].dtype == c["logp"].dtype == c["a_next"].dtype == np.float64
        assert all(c[k].dtype == np.float32 for k in c if k[:2] in ("a_", "c_", "t_") and k != "a_next") and c["obs"].dtype == np.float32
        assert 20 <= c["done"].sum() <= 110 and set(np.unique(c["done"])) == {0.0, 1.0}                      # done mixed 0 / 1
        assert float(c["discount"]) == 0.99 and float(c["alpha"]) == 0.2
        if "a_fc1_w" in c:
            assert c["a_fc1_w"].shape == (ACTORS.get(name, (23, 16, 4))[1], D) and c["a_log_std_w"].shape == (A, c["a_fc1_w"].shape[0])
        else:
            assert c["a_next_in"].shape == (130, A) and c["logp_next_in"].shape == (130,)
    for name in LIVE:
        c = sac_ref.case(fixture, name)
        m = td3_ref.margin([c["c_" + n] for n in NAMES], c["obs"], c["action"])
        assert m >= td3_ref.MARGIN and abs(m - float(c["min_abs_z"])) <= 1e-12 * max(1.0, m)


def test_clamp_and_sat_shares_of_the_fixture(fixture):
    c = sac_ref.case(fixture, "clamp")
    _, ls = _heads(c)
    assert np.mean(ls < -20) >= 0.2 and np.mean(ls > 2) >= 0.2                 # both bounds of the log_std clamp are active
    assert np.mean((ls >= -20) & (ls <= 2)) >= 0.2                              # ... and so is the range between them
    c = sac_ref.case(fixture, "sat")
    mean, ls = _heads(c)
    u = mean + np.exp(np.clip(ls, -20, 2)) * c["eps"].astype(np.float64)
    assert np.mean(np.abs(u) >= 9) >= 0.1
    assert np.mean(np.abs(u) < 3) >= 0.1                                        # ... next to unsaturated components
    for name in ("mono", "dtde0", "dtde1"):                                     # the plain cases are plain
        mean, ls = _heads(sac_ref.case(fixture, name))
        assert ls.min() > -20 and ls.max() < 2


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(fixture, name):
    c = sac_ref.case(fixture, name)
    a_next, logp, y = sac_ref.sac_target_f64(c)
    worst = {}
    for got, want, what in ((a_next, c["a_next"], "a_next"), (logp, c["logp"], "logp"), (y, c["y"], "y")):
        err, bound = float(np.abs(got - want).max()), 1e-12 * max(1.0, float(np.abs(want).max()))
        print(f"sac restatement {name} {what}: err {err:.3e}, bound {bound:.3e}")
        worst[what] = (err, bound)
    assert all(err <= bound for err, bound in worst.values()), (name, worst)


@pytest.mark.parametrize("name", CASES)
def test_done_rows_have_the_reward_as_target(fixture, name):
    c = sac_ref.case(fixture, name)
    done = c["done"] > 0
    assert np.array_equal(c["y"][done], c["reward"][done].astype(np.float64))
    assert not np.any(c["y"][~done] == c["reward"][~done])
    y = sac_ref.sac_target_f64(c)[2]
    assert np.array_equal(y[done], c["reward"][done].astype(np.float64))


def test_restatement_options(fixture):
    c = sac_ref.case(fixture, "mono")
    a0, l0, y0 = sac_ref.sac_target_f64(c, eps=None)
    n = sac_ref.case(fixture, "noeps")
    assert np.array_equal(a0, sac_ref.sac_target_f64(n)[0]) and np.array_equal(y0, sac_ref.sac_target_f64(n)[2])
    a, lp, y = sac_ref.sac_target_f64(c)
    a2, lp2, y2 = sac_ref.sac_target_f64(c, a_next=a, logp_next=lp)              # a' and logp fed back in
    assert np.array_equal(y2, y) and np.array_equal(lp2, lp)
    idx = np.array([5, 5, 129, 0])
    a3, lp3, y3 = sac_ref.sac_target_f64(c, idx, eps=c["eps"][idx])
    assert np.allclose(y3, y[idx], rtol=0, atol=1e-13)
    ya = sac_ref.sac_target_f64(c, alpha=0.0)[2]
    assert np.allclose(ya - y, 0.99 * (1 - c["done"].astype(np.float64)) * 0.2 * lp, rtol=0, atol=1e-12)


def test_struct_mirrors_the_header(tmp_path):
    from gym_rotor_amd import _lib as L
    sname = "QrSacTarget"
    lines = [f'printf("{sname} %zu\\n", sizeof({sname}));']
    lines += [f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));' for f, _ in L.QrSacTarget._fields_]
    lines.append('printf("abi %d\\n", QR_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out[sname]) == C.sizeof(L.QrSacTarget) == 64
    for f, _ in L.QrSacTarget._fields_:
        assert int(out[f"{sname}.{f}"]) == getattr(L.QrSacTarget, f).offset, f
    assert [f for f, _ in L.QrSacTarget._fields_] == ["eps", "action_next", "logp_next", "alpha_dev", "y", "action_out", "logp_out", "discount",
                                                      "alpha"]
    assert "qr_sac_target" in L.SYMBOLS and hasattr(L.load(), "qr_sac_target") and int(out["abi"]) == L.ABI_VERSION


def _fake(obs_dim=23, action_dim=4, hidden=62, batch=130, actor=(23, 16, 4)):
    """(QrActor, QrQCritic, QrTransitions, QrSacTarget) that pass every check, on fake device addresses (never touched: every case of
    the test below returns before a launch — a legal case is refused last through y = NULL)."""
    from gym_rotor_amd import _lib as L
    p = L.QrActor()
    for k, n in enumerate(("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std", "log_std_w", "log_std_b")):
        setattr(p, n, 0x900000 + 0x1000 * k)
    p.log_std = None
    p.obs_dim, p.hidden_dim, p.action_dim, p.squash = *actor, L.ACTOR_TANH_SAMPLE
    q = L.QrQCritic()
    for k, n in enumerate(NAMES):
        setattr(q, n, 0x10000 + 0x1000 * k)
    q.obs_dim, q.action_dim, q.hidden_dim, q.reserved0 = obs_dim, action_dim, hidden, 0
    b = L.QrTransitions()
    for k, n in enumerate(("obs", "obs_next", "action", "reward", "done", "index")):
        setattr(b, n, 0x100000 + 0x10000 * k)
    b.batch, b.rows, b.row_stride, b.col_offset, b.reward_stride, b.done_stride = batch, 130, action_dim, 0, 1, 1
    t = L.sac_target_args(eps=None, action_next=None, logp_next=None, alpha_dev=None, y=None, action_out=None, logp_out=None, discount=0.99,
                          alpha=0.2)
    t.eps, t.action_next, t.logp_next, t.alpha_dev, t.action_out, t.logp_out = 0x200000, 0x210000, 0x230000, 0x240000, 0x250000, 0x260000
    return {"p": p, "q": q, "b": b, "t": t}


NULL, KIND, SIZE, ALIGN = -1, -2, -3, -4
Y = 0x220000


def _ref(x):
    return None if x is None else C.byref(x)


def test_sac_target_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()

    def call(s):
        return lib.qr_sac_target(_ref(s["p"]), _ref(s["q"]), _ref(s["b"]), _ref(s["t"]), None)

    def expect(code, what, fake=(), **edit):
        s = _fake(*fake)                                           # y = NULL: the last pointer check, every legal case ends there
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
    expect(NULL, "no actor: action_next and logp_next", p=None)
    expect(NULL, "no actor and no action_next", p=None, t_action_next=None, t_y=Y)
    expect(NULL, "no actor and no logp_next", p=None, t_logp_next=None, t_y=Y)
    for n in ("eps", "alpha_dev", "action_out", "logp_out", "action_next", "logp_next"):
        expect(NULL, "optional with an actor", **{"t_" + n: None})
    expect(NULL, "log_std is unread", p_log_std=0x906000)
    expect(NULL, "obs and action are unread", b_obs=None, b_action=None, b_row_stride=0)
    expect(NULL, "alpha = 0, discount = 0", t_alpha=0.0, t_discount=0.0)
    for n in NAMES:
        expect(NULL, "weight", t_y=Y, **{"q_" + n: None})
    for n in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b"):
        expect(NULL, "actor weight", t_y=Y, **{"p_" + n: None})
    for n in ("obs_next", "reward", "done"):
        expect(NULL, n, t_y=Y, **{"b_" + n: None})
    expect(KIND, "TD3 / PPO form", p_squash=L.ACTOR_TANH_MEAN)
    expect(KIND, "no log_std head", p_log_std_w=None, p_log_std_b=None, p_log_std=0x906000)
    expect(KIND, "half a log_std head", p_log_std_b=None)
    expect(KIND, "half a log_std head", p_log_std_w=None)
    for D, A, H in ((25, 4, 62), (23, 6, 62), (0, 4, 62), (23, 0, 62), (23, 4, 0), (23, 4, 65)):
        expect(SIZE, "widths", q_obs_dim=D, q_action_dim=A, q_hidden_dim=H)
    for dims in ((23, 16, 3), (23, 8, 4), (24, 16, 4), (15, 16, 4), (3, 4, 1)):
        expect(SIZE, "actor sizes, or an actor that does not fit the critic", p_obs_dim=dims[0], p_hidden_dim=dims[1], p_action_dim=dims[2])
    expect(SIZE, "actor 15 -> 4 under a 15 + 1 critic", fake=(15, 1, 62, 130, (15, 16, 4)))
    for edit in (dict(b_batch=0), dict(b_batch=-3), dict(b_rows=0), dict(b_reward_stride=0), dict(b_done_stride=-1), dict(q_reserved0=7),
                 dict(t_discount=-0.5), dict(t_discount=float("nan")), dict(t_discount=float("inf")), dict(t_alpha=-0.2),
                 dict(t_alpha=float("nan")), dict(t_alpha=float("inf"))):
        expect(SIZE, "sizes", **edit)
    for edit in (dict(b_obs_next=0x110002), dict(b_reward=0x130001), dict(b_done=0x140003), dict(t_eps=0x200002), dict(t_y=0x220001),
                 dict(t_action_next=0x210002), dict(t_logp_next=0x230001), dict(t_alpha_dev=0x240002), dict(t_action_out=0x250003),
                 dict(t_logp_out=0x260002), dict(q_fc4_w=0x13002), dict(p_mean_w=0x904001), dict(p_log_std_w=0x907002),
                 dict(p_log_std_b=0x908001), dict(b_index=0x150004)):
        expect(ALIGN, "alignment", **{"t_y": Y, **edit})
    # the order of the classes: KIND before SIZE before NULL before ALIGN
    expect(KIND, "kind first", p_squash=0, q_hidden_dim=0, b_obs_next=None)
    expect(SIZE, "size before pointers", t_alpha=-1.0, b_obs_next=None, t_y=0x220001)
    expect(NULL, "pointers before alignment", b_obs_next=None, t_y=0x220001)


# ---------------------------------------------------------------------------------------------------------------------------
# the Python helpers
# ---------------------------------------------------------------------------------------------------------------------------
class _Twin(torch.nn.Module):
    def __init__(self, din=27, hidden=62):
        super().__init__()
        for k, (i, o) in enumerate(((din, hidden), (hidden, hidden), (hidden, 1)) * 2, 1):
            setattr(self, f"fc{k}", torch.nn.Linear(i, o))


class _SacActor(torch.nn.Module):
    def __init__(self, D=23, H=16, A=4):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(D, H), torch.nn.Linear(H, H)
        self.mean_linear, self.log_std_linear = torch.nn.Linear(H, A), torch.nn.Linear(H, A)


def test_python_helpers_refuse_bad_arguments():
    from gym_rotor_amd import ActorParams, QCriticParams, ReplayBuffer, sac_critic_loss, sac_target
    q = QCriticParams.from_module(_Twin(), 4)
    actor = ActorParams.from_sac_module(_SacActor())
    t = {"obs": torch.zeros(10, 23), "act": torch.zeros(10, 4), "rwd": torch.zeros(10), "obs_next": torch.zeros(10, 23), "done": torch.zeros(10)}
    idx = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        sac_target(actor, q, t, 0, idx)
    with pytest.raises(RuntimeError, match="GPU only"):
        sac_target(actor, q, t, 0, idx, alpha=torch.tensor([0.2]), noise=torch.zeros(5, 4), action_out=torch.zeros(5, 4), logp_out=torch.zeros(5))
    with pytest.raises(RuntimeError, match="GPU only"):
        sac_target(None, q, t, 0, idx, action_next=torch.zeros(5, 4), logp_next=torch.zeros(5))
    bad_t = [("obs_next", torch.zeros(10, 22)), ("obs_next", torch.zeros(10, 23, dtype=torch.float64)), ("rwd", torch.zeros(9)),
             ("done", torch.zeros(10, dtype=torch.bool)), ("rwd", torch.zeros(10, 2)), ("done", None)]
    for k, v in bad_t:
        with pytest.raises(ValueError, match=k):
            sac_target(actor, q, {**t, k: v}, 0, idx)
    for kw, pat in ((dict(index=idx.int()), "index"), (dict(index=idx, noise=torch.zeros(5, 3)), "noise"), (dict(index=idx, noise=torch.zeros(10, 4)), "noise"),
                    (dict(index=idx, out=torch.zeros(4)), "out"), (dict(index=idx, out=torch.zeros(5, dtype=torch.float64)), "out"),
                    (dict(index=idx, action_out=torch.zeros(5, 3)), "action_out"), (dict(index=idx, action_out=torch.zeros(4, 5).T), "action_out"),
                    (dict(index=idx, logp_out=torch.zeros(6)), "logp_out"), (dict(index=idx, logp_out=torch.zeros(5, dtype=torch.float64)), "logp_out"),
                    (dict(index=idx, alpha=-0.1), "alpha"), (dict(index=idx, alpha=float("nan")), "alpha"), (dict(index=idx, alpha=float("inf")), "alpha"),
                    (dict(index=idx, alpha=torch.zeros(2)), "alpha"), (dict(index=idx, alpha=torch.zeros(1, dtype=torch.float64)), "alpha"),
                    (dict(index=idx, discount=-1.0), "discount"), (dict(index=idx, discount=float("nan")), "discount")):
        with pytest.raises(ValueError, match=pat):
            sac_target(actor, q, t, 0, **kw)
    for kw in (dict(), dict(action_next=torch.zeros(5, 4)), dict(logp_next=torch.zeros(5))):
        with pytest.raises(ValueError, match="action_next .* and logp_next"):
            sac_target(None, q, t, 0, idx, **kw)
    with pytest.raises(ValueError, match="action_next"):
        sac_target(None, q, t, 0, idx, action_next=torch.zeros(5, 3), logp_next=torch.zeros(5))
    with pytest.raises(ValueError, match="logp_next"):
        sac_target(None, q, t, 0, idx, action_next=torch.zeros(5, 4), logp_next=torch.zeros(4))
    with pytest.raises(ValueError, match="the critic reads"):
        sac_target(ActorParams.from_sac_module(_SacActor(15, 16, 4)), q, t, 0, idx)
    with pytest.raises(ValueError, match="not among"):
        sac_target(ActorParams.from_sac_module(_SacActor(23, 8, 4)), q, t, 0, idx)
    td3 = ActorParams.from_sac_module(_SacActor())
    td3.squash = 0
    with pytest.raises(ValueError, match="MLP_Actor_SAC"):
        sac_target(td3, q, t, 0, idx)
    nohead = ActorParams.from_sac_module(_SacActor())
    nohead.log_std_w, nohead.log_std = None, torch.zeros(4)
    with pytest.raises(ValueError, match="MLP_Actor_SAC"):
        sac_target(nohead, q, t, 0, idx)
    half = ActorParams.from_sac_module(_SacActor())
    half.log_std_b = half.log_std_b.double()
    with pytest.raises(ValueError, match="log_std_b"):
        sac_target(half, q, t, 0, idx)
    # sac_critic_loss: its own check, and what it passes on
    buf = ReplayBuffer(10, [23], [4], "cpu")
    with pytest.raises(ValueError, match="ReplayBuffer"):
        sac_critic_loss(_Twin(), _Twin(), _SacActor(), t, 0, idx)
    with pytest.raises(ValueError, match="alpha"):
        sac_critic_loss(_Twin(), _Twin(), _SacActor(), buf, 0, idx, alpha=-1.0)
    with pytest.raises(ValueError, match="noise"):
        sac_critic_loss(_Twin(), _Twin(), _SacActor(), buf, 0, idx, noise=torch.zeros(5, 3))
    with pytest.raises(ValueError, match="the critic reads"):
        sac_critic_loss(_Twin(), _Twin(), _SacActor(15, 16, 4), buf, 0, idx)
    with pytest.raises(ValueError, match="critic tensor"):
        sac_critic_loss(_Twin(), _Twin(27, 61).double(), _SacActor(), buf, 0, idx)
    with pytest.raises(AttributeError):
        sac_critic_loss(_Twin(), _Twin(), torch.nn.Linear(3, 3), buf, 0, idx)     # not MLP_Actor_SAC's attributes
    with pytest.raises(RuntimeError, match="GPU only"):
        sac_critic_loss(_Twin(), _Twin(), _SacActor(), buf, 0, idx)
    assert ("sac", 0, 5, 0) in buf._cache and (0, 5, 0) not in buf._cache       # a key of its own


def test_torch_op_is_registered():
    from gym_rotor_amd import ActorParams, QCriticParams
    assert hasattr(torch.ops.gym_rotor_amd, "qr_sac_target")
    q = QCriticParams.from_module(_Twin(), 4)
    w = [getattr(q, n) for n in NAMES]
    a = ActorParams.from_sac_module(_SacActor())
    aw = [a.fc1_w, a.fc1_b, a.fc2_w, a.fc2_b, a.mean_w, a.mean_b, a.log_std_w, a.log_std_b]
    idx, y = torch.zeros(5, dtype=torch.int64), torch.zeros(5)
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_sac_target(aw, w, 4, torch.zeros(10, 23), torch.zeros(10), torch.zeros(10), idx, None, None, None, y, None, None, 0.99, 0.2)
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_sac_target([], w, 4, torch.zeros(10, 23), torch.zeros(10), torch.zeros(10), idx, None, torch.zeros(5, 4),
                                              torch.zeros(5), y, torch.zeros(5, 4), torch.zeros(5), 0.99, 0.0, torch.zeros(1))
