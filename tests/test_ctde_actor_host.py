"""Agent k's TD3 actor half under the centralized (CTDE) critic (qr_ctde_dpg_actor_grad; td3.dpg_actor_grad_ctde /
dpg_actor_workspace_bytes_ctde / td3_actor_loss_ctde) without a GPU: the float64 restatement of tests/ctde_actor_ref.py against the
reference's own autograd (tests/golden/ctde_actor.npz, tools/gen_golden_ctde_actor.py), the ReLU margin of every case, sat's clamp
conditions, the new struct's layout, every documented error of the two C entries in their order, and of the three Python functions."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctde_actor_ref as R  # noqa: E402
from ctde_actor_ref import ACTOR_NAMES, CASES  # noqa: E402
from td3_ref import NAMES  # noqa: E402
from test_ctde_critic_host import ACTOR_W, ALIGN, KIND, NULL, SIZE, _apply, _fake, _ref, _Td3Actor, _Twin  # noqa: E402

# name: (obs widths, action widths, critic hidden, k)
SHAPES = {"k0": ((15, 3), (4, 1), 62, 0), "k1": ((15, 3), (4, 1), 62, 1), "h64": ((15, 3), (4, 1), 64, 1), "h5": ((15, 3), (4, 1), 5, 0),
          "noreg": ((15, 3), (4, 1), 62, 0), "sat0": ((15, 3), (4, 1), 62, 0), "sat1": ((15, 3), (4, 1), 62, 1),
          "w28a": ((15, 5), (4, 4), 62, 0), "w28b": ((16, 3), (8, 1), 62, 1)}


@pytest.fixture(scope="module")
def fixture():
    return R.load()


def test_fixture_holds_the_cases(fixture):
    assert tuple(str(n) for n in fixture["cases"]) == CASES == tuple(SHAPES)
    assert os.path.getsize(R.GOLDEN) <= 1_000_000
    assert not any(k.split("_", 1)[1].startswith(("c_fc4", "c_fc5", "c_fc6")) for k in fixture.files if "_" in k)   # only Q1 is stored
    for name in CASES:
        c = R.case(fixture, name)
        od, ad, H, k = SHAPES[name]
        assert c["k"] == k and c["c_fc1_w"].shape == (H, sum(od) + sum(ad)) and c["c_fc2_w"].shape == (H, H) and c["c_fc1_w"].dtype == np.float32
        for m in (0, 1):
            assert c[f"obs{m}"].shape == (130, od[m]) and c[f"obs_next{m}"].shape == (130, od[m]) and c[f"obs{m}"].dtype == np.float32
        assert (R.actor_of(c, 1 - k) is None) == (name in R.SUPPLIED) == ("action_other" in c)
        if name in R.SUPPLIED:
            assert c["action_other"].shape == (130, ad[1 - k]) and c["action_other"].dtype == np.float32
        assert c["a%d_fc1_w" % k].shape == ((16, 15), (4, 3))[k] and c["g_fc3_w"].shape == ((4, 16), (1, 4))[k] and c["g_fc1_w"].dtype == np.float64
        assert c["noise"].shape == (od[k],) and c["nominal"].shape == (ad[k],)
        assert c["lam"] == ((0.0, 0.0, 0.0) if name == "noreg" else (0.4, 0.3, 0.6)) and c["max_action"] == (0.5 if name.startswith("sat") else 1.0)
    s0, s1, k0, nr = (R.case(fixture, n) for n in ("sat0", "sat1", "k0", "noreg"))
    assert all(np.array_equal(s0[key], s1[key]) for key in ("obs0", "obs1", "a0_fc1_w", "a1_fc3_w", "c_fc2_w"))   # one set of networks, both k
    assert all(np.array_equal(k0[key], nr[key]) for key in ("a0_fc1_w", "a1_fc3_w", "c_fc2_w")) and not np.array_equal(k0["obs0"], nr["obs0"])


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.abs(got.reshape(want.shape) - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), what


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(fixture, name):
    c = R.case(fixture, name)
    stats, grads = R.case_f64(c)
    for n in ACTOR_NAMES:
        _close(grads[n], c["g_" + n], (name, n))
    for got, key in zip(stats, R.STATS):
        _close(got, c[key], (name, key))
    # the other agent's action is a value: scaling its actor's last layer moves the gradients, its own obs_next does not enter at all
    if name == "k0":
        w1 = [t.copy() for t in R.actor_of(c, 1)]
        w1[4] = w1[4] * 2
        moved = R.ctde_dpg_actor_grad_f64([R.actor_of(c, 0), w1], R.q1_of(c), (c["obs0"], c["obs1"]), c["obs_next0"], 0, None, c["noise"], c["nominal"],
                                          c["lam"], c["max_action"])[1]
        assert np.abs(moved["fc1_w"] - grads["fc1_w"]).max() > 1e-6


@pytest.mark.parametrize("name", CASES)
def test_every_case_keeps_the_relu_margin(fixture, name):
    c = R.case(fixture, name)
    m = R.case_margin(c)
    assert m >= R.MARGIN == 2e-5
    assert abs(m - float(c["min_abs_z"])) <= 1e-12 * max(1.0, m)


def test_sat_clamps_both_agents(fixture):
    for name in ("sat0", "sat1"):
        c = R.case(fixture, name)
        shares = R.clamp_shares(c)
        assert set(shares) == {0, 1}
        for m, (share, dist) in shares.items():
            assert 0.3 <= share <= 0.9 and dist >= 1e-4, (name, m, share, dist)
            assert share == float(c["clamp_shares"][m]) and dist == float(c["clamp_distance"][m])
        assert float(c["clamp_share"]) == shares[c["k"]][0]
    assert all(s == 0.0 for s, _ in R.clamp_shares(R.case(fixture, "k0")).values())


def test_struct_mirrors_the_header(tmp_path):
    from gym_rotor_amd import _lib as L
    sname = "QrCtdeDpgGrad"
    lines = [f'printf("{sname} %zu\\n", sizeof({sname}));'] + [f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));' for f, _ in L.QrCtdeDpgGrad._fields_]
    lines += ['printf("base %zu\\n", sizeof(QrDpgGrad));', 'printf("abi %d\\n", QR_ABI_VERSION);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out[sname]) == C.sizeof(L.QrCtdeDpgGrad) == C.sizeof(L.QrDpgGrad) + 16 and int(out["base"]) == C.sizeof(L.QrDpgGrad)
    for fl, _ in L.QrCtdeDpgGrad._fields_:
        assert int(out[f"{sname}.{fl}"]) == getattr(L.QrCtdeDpgGrad, fl).offset, fl
    for fl, _ in L.QrDpgGrad._fields_:                                # QrDpgGrad's members first, at its offsets
        assert getattr(L.QrCtdeDpgGrad, fl).offset == getattr(L.QrDpgGrad, fl).offset
    lib = L.load()
    new = {"qr_ctde_dpg_actor_grad", "qr_ctde_dpg_actor_workspace_bytes"}
    assert new <= set(L.SYMBOLS) and all(hasattr(lib, s) for s in new)
    assert int(out["abi"]) == L.ABI_VERSION == 16 and lib.qr_abi_version() == 16


NP = {0: 16 * 15 + 16 + 256 + 16 + 64 + 4 + 5, 1: 4 * 3 + 4 + 16 + 4 + 4 + 1 + 5}   # a partial vector: the six tensors and five sums


def _fake_actor(k=0, od=(15, 3), ad=(4, 1), hidden=62, batch=130, supplied=False):
    """test_ctde_critic_host's fake structs plus a QrCtdeDpgGrad that passes every check with a workspace ONE BYTE SHORT: every legal
    case ends with the workspace's QR_E_SIZE, before any launch."""
    from gym_rotor_amd import _lib as L
    s = _fake(od, ad, hidden, batch)
    g = L.QrCtdeDpgGrad(*[0x800000 + 0x1000 * j for j in range(7)], 0x300000, 0x310000, 0x400000)
    g.workspace_bytes = L.load().qr_ctde_dpg_actor_workspace_bytes(k, hidden, batch, 0) - 1
    g.lam_T, g.lam_S, g.lam_M, g.max_action, g.max_workgroups, g.reserved0, g.agent, g.reserved1 = 0.4, 0.3, 0.6, 1.0, 0, 0, k, 0
    if supplied:
        s[f"p{1 - k}"], g.action_other = None, 0x320000
    s["g"] = g
    return s


def test_ctde_dpg_actor_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()
    call = lambda s: lib.qr_ctde_dpg_actor_grad(_ref(s["p0"]), _ref(s["p1"]), _ref(s["q"]), _ref(s["b"]), _ref(s["g"]), None)
    big = dict(g_workspace_bytes=1 << 40)

    def expect(code, what, fake={}, **edit):
        s = _fake_actor(**fake)
        _apply(s, edit)
        assert call(s) == code, (what, fake, edit)

    for k in (0, 1):
        F = dict(k=k)
        o = 1 - k
        expect(SIZE, "everything else is legal: the workspace is one byte short", fake=F)
        expect(SIZE, "the supplied form", fake=dict(k=k, supplied=True))
        for key in "qbg":
            assert call({**_fake_actor(k), key: None}) == NULL
        # KIND first: either actor's form, and both forms of the other action at once
        for m in (0, 1):
            expect(KIND, "the other form", fake=F, **big, **{f"p{m}_squash": L.ACTOR_TANH_SAMPLE, "b_batch": 0, "q_fc1_w": None})
            expect(KIND, "a log_std head", fake=F, **{f"p{m}_log_std_w": 0x990000, f"p{m}_log_std_b": 0x991000})
        expect(KIND, "both actors and action_other", fake=F, g_action_other=0x320000, g_agent=5)
        # SIZE next, before any NULL
        for edit in (dict(g_agent=2), dict(g_agent=-1), {"b_obs_dim@0": 14}, {"b_action_dim@1": 2}, {"b_obs_dim@1": 0, "b_obs_dim@0": 18}, dict(q_obs_dim=19),
                     dict(q_action_dim=6), dict(q_hidden_dim=0), dict(q_hidden_dim=65), dict(q_reserved0=7), dict(g_reserved0=1), dict(g_reserved1=1),
                     dict(p0_obs_dim=23), dict(p0_hidden_dim=8), dict(p1_hidden_dim=5), dict(p1_obs_dim=15, p1_hidden_dim=16, p1_action_dim=4),
                     dict(b_batch=0), dict(b_rows=0), dict(g_max_workgroups=-1), dict(g_max_action=-1.0), dict(g_max_action=float("nan")),
                     dict(g_lam_T=-0.1), dict(g_lam_S=float("inf")), dict(g_lam_M=float("nan"))):
            expect(SIZE, "sizes", fake=F, **big, g_stats=None, **edit)
        expect(SIZE, "actors beside other widths", fake=dict(k=k, od=(14, 4), ad=(4, 1)), **big)
        expect(SIZE, "actors in the other order", fake=dict(k=k, od=(3, 15), ad=(1, 4)), **big)
        expect(SIZE, "29 columns", fake=dict(k=k, supplied=True, od=((15, 6), (17, 3))[k], ad=((4, 4), (8, 1))[k]), **big)
        expect(SIZE, "the supplied form, its own actor's widths still bind", fake=dict(k=k, supplied=True, od=(14, 4), ad=(4, 1)), **big)
        expect(SIZE, "28 columns, supplied: legal", fake=dict(k=k, supplied=True, od=((15, 5), (16, 3))[k], ad=((4, 4), (8, 1))[k]))
        # NULL
        expect(NULL, "agent k's actor", fake=F, **big, **{f"p{k}": None})
        expect(NULL, "agent k's actor, supplied form", fake=dict(k=k, supplied=True), **big, **{f"p{k}": None})
        expect(NULL, "neither form", fake=F, **big, **{f"p{o}": None})
        for n in ACTOR_W:
            expect(NULL, "own actor weight", fake=F, **big, **{f"p{k}_{n}": None})
            expect(NULL, "other actor weight", fake=F, **big, **{f"p{o}_{n}": None})
            expect(NULL, "gradient", fake=F, **big, **{"g_" + n: None})
        for n in NAMES[:6]:
            expect(NULL, "Q1 weight", fake=F, **big, **{"q_" + n: None})
        for n in ("stats", "workspace", "noise", "nominal"):
            expect(NULL, n, fake=F, **big, **{"g_" + n: None})
        for m in (0, 1):
            expect(NULL, "obs", fake=F, **big, **{f"b_obs@{m}": None})
        expect(NULL, "obs_next[k]", fake=F, **big, **{f"b_obs_next@{k}": None})
        expect(SIZE, "what is not read may be NULL", fake=F, b_index=None, b_reward=None, b_done=None, p0_log_std=None, p1_log_std=None,
               **{f"b_obs_next@{o}": None, "b_action@0": None, "b_action@1": None, "b_row_stride@0": 0}, **{"q_" + n: None for n in NAMES[6:]})
        expect(SIZE, "zero coefficients read none of their inputs", fake=F, g_lam_T=0.0, g_lam_S=0.0, g_lam_M=0.0, g_noise=None, g_nominal=None,
               **{f"b_obs_next@{k}": None})
        # ALIGN, then the workspace's SIZE
        for edit in ({"b_obs@0": 0x100002}, {"b_obs@1": 0x108001}, {f"b_obs_next@{k}": 0x110002 + 0x8000 * k}, dict(g_noise=0x300001), dict(g_nominal=0x310002),
                     dict(g_fc2_w=0x802001), dict(g_stats=0x806002), dict(q_fc3_b=0x15002), {f"p{k}_mean_w": 0x904001 + 0x100000 * k},
                     {f"p{o}_fc2_b": 0x903002 + 0x100000 * o}, dict(b_index=0x150004), dict(g_workspace=0x400004)):
            expect(ALIGN, "alignment", fake=F, **big, **edit)
        expect(ALIGN, "action_other", fake=dict(k=k, supplied=True), **big, g_action_other=0x320002)
        expect(SIZE, "a short workspace comes last", fake=F, g_workspace_bytes=0)
    ws = lib.qr_ctde_dpg_actor_workspace_bytes
    for k in (0, 1):
        assert ws(k, 62, 130, 0) == 3 * NP[k] * 8 == lib.qr_dpg_actor_workspace_bytes(*((15, 16, 4), (3, 4, 1))[k], 62, 130, 0)
        assert ws(k, 1, 64 * 5000, 0) == 1024 * NP[k] * 8 and ws(k, 64, 64 * 5000, 7) == 7 * NP[k] * 8 and ws(k, 62, 1, 0) == NP[k] * 8
    for bad in ((2, 62, 10, 0), (-1, 62, 10, 0), (0, 0, 10, 0), (1, 65, 10, 0), (0, 62, 0, 0), (1, 62, 10, -1)):
        assert ws(*bad) == SIZE, bad


# ---------------------------------------------------------------------------------------------------------------------------
# the Python functions
# ---------------------------------------------------------------------------------------------------------------------------
def _pair(rows=10, od=(15, 3)):
    return [torch.zeros(rows, d) for d in od]


def test_python_functions_refuse_bad_arguments():
    from gym_rotor_amd import ActorParams, QCriticParams, ReplayBuffer, dpg_actor_grad_ctde, dpg_actor_workspace_bytes_ctde, td3_actor_loss_ctde
    q = QCriticParams.from_module(_Twin(), 5)
    actors = [ActorParams.from_td3_module(_Td3Actor(*d), 0.0) for d in ((15, 16, 4), (3, 4, 1))]
    obs, nxt, idx = _pair(), _pair(), torch.zeros(5, dtype=torch.int64)
    kw = dict(noise=torch.zeros(15), nominal=torch.zeros(4))
    kw1 = dict(noise=torch.zeros(3), nominal=torch.zeros(1))
    with pytest.raises(RuntimeError, match="GPU only"):
        dpg_actor_grad_ctde(actors, q, obs, nxt, idx, k=0, **kw)
    with pytest.raises(RuntimeError, match="GPU only"):
        dpg_actor_grad_ctde(actors, q, obs, (None, nxt[1]), idx, k=1, **kw1)
    with pytest.raises(RuntimeError, match="GPU only"):
        dpg_actor_grad_ctde([actors[0], None], q, obs, nxt, idx, k=0, action_other=torch.zeros(5, 1), **kw)
    with pytest.raises(RuntimeError, match="GPU only"):                                       # free widths in the supplied form: 16+3 / 8+1
        dpg_actor_grad_ctde([None, actors[1]], QCriticParams.from_module(_Twin(28), 9), _pair(od=(16, 3)), None, idx, k=1, action_other=torch.zeros(5, 8),
                            lam_T=0.0, **kw1)
    with pytest.raises(RuntimeError, match="GPU only"):                                       # zero coefficients need none of their inputs
        dpg_actor_grad_ctde(actors, q, obs, None, None, k=0, lam_T=0.0, lam_S=0.0, lam_M=0.0)

    def bad(match, a=actors, critic=q, o=obs, n=nxt, i=idx, **over):
        with pytest.raises(ValueError, match=match):
            dpg_actor_grad_ctde(a, critic, o, n, i, **{"k": 0, **kw, **over})
    bad("k must be", k=2)
    bad("pair", a=actors[:1])
    bad("agent 0's is required", a=[None, actors[1]])
    bad("not neither", a=[actors[0], None])
    bad("not both", action_other=torch.zeros(5, 1))
    bad("obs must be a pair", o=obs[:1])
    bad(r"obs\[1\]", o=[obs[0], None])
    bad(r"obs\[0\]", o=[obs[0].double(), obs[1]])
    bad(r"obs\[1\] must have", o=[obs[0], torch.zeros(9, 3)])
    bad("index", i=idx.int())
    bad("action_other", a=[actors[0], None], action_other=torch.zeros(6, 1))
    bad("action_other", a=[actors[0], None], action_other=torch.zeros(5, 1, dtype=torch.float64))
    bad("add up", critic=QCriticParams.from_module(_Twin(24), 5))
    bad("add up", a=[actors[0], None], action_other=torch.zeros(5, 2))
    bad("the actor maps", o=_pair(od=(14, 4)))
    bad("must have the sizes", a=[actors[1], actors[1]], o=_pair(od=(3, 15)), critic=QCriticParams.from_module(_Twin(20), 2), noise=torch.zeros(3),
        nominal=torch.zeros(1))
    sac = ActorParams.from_td3_module(_Td3Actor(3, 4, 1), 0.0)
    sac.squash = 1
    bad("MLP_Actor_TD3", a=[actors[0], sac])
    half = ActorParams.from_td3_module(_Td3Actor(15, 16, 4), 0.0)
    half.fc2_w = half.fc2_w.double()
    bad("fc2_w", a=[half, actors[1]])
    for name in ("lam_T", "lam_S", "lam_M", "max_action"):
        bad(name, **{name: -1.0})
        bad(name, **{name: float("inf")})
    bad("obs_next", n=None)
    bad("obs_next", n=(None, nxt[1]))
    bad(r"obs_next\[0\]", n=(torch.zeros(10, 14), nxt[1]))
    bad(r"obs_next\[0\] must have", n=(torch.zeros(9, 15), nxt[1]))
    bad("noise", noise=None)
    bad("nominal", nominal=None)
    bad("noise", noise=torch.zeros(3))
    bad("nominal", nominal=torch.zeros(1))
    bad("grads", grads={})
    bad("stats", stats=torch.zeros(5))
    for args in ((2, 62, 10), (0, 65, 10), (1, 62, 0), (0, 62, 10, -1)):
        with pytest.raises(ValueError, match="QR_E_SIZE"):
            dpg_actor_workspace_bytes_ctde(*args)
    assert dpg_actor_workspace_bytes_ctde(0, 62, 130) == 3 * NP[0] * 8 and dpg_actor_workspace_bytes_ctde(1, 62, 130, 2) == 2 * NP[1] * 8

    mods, critic = [_Td3Actor(15, 16, 4), _Td3Actor(3, 4, 1)], _Twin()
    buf = ReplayBuffer(8, (15, 3), (4, 1), "cpu")
    with pytest.raises(ValueError, match="two-agent"):
        td3_actor_loss_ctde(mods, critic, ReplayBuffer(8, (23,), (4,), "cpu"))
    with pytest.raises(ValueError, match="two-agent"):
        td3_actor_loss_ctde(mods, critic, {"obs": obs})
    with pytest.raises(ValueError, match="k must be"):
        td3_actor_loss_ctde(mods, critic, buf, 2)
    with pytest.raises(ValueError, match="pair"):
        td3_actor_loss_ctde(mods[:1], critic, buf)
    with pytest.raises(ValueError, match="noise"):
        td3_actor_loss_ctde(mods, critic, buf, 0, nominal=torch.zeros(4))


@pytest.mark.parametrize("k", (0, 1))
def test_td3_actor_loss_ctde_leaves_the_other_agent_alone(k, monkeypatch):
    """Up to the launch (which needs a GPU): agent k's six .grad tensors are made and handed over as they are, the cache key is its own,
    and the other actor's .grad objects — None, or tensors with values — are the objects and values they were."""
    from gym_rotor_amd import ReplayBuffer, td3, td3_actor_loss_ctde
    mods, critic = [_Td3Actor(15, 16, 4), _Td3Actor(3, 4, 1)], _Twin()
    buf = ReplayBuffer(8, (15, 3), (4, 1), "cpu")
    other = list(mods[1 - k].parameters())
    other[0].grad = torch.full_like(other[0], 3.5)
    held = [p.grad for p in other]
    seen = {}
    monkeypatch.setattr(td3, "dpg_actor_workspace_bytes_ctde", lambda k, H, B, mw=0: 8 * 11)

    def launch(actors, q, obs, obs_next, index, **kw):
        seen.update(kw, actors=actors, obs=obs, obs_next=obs_next)
        return kw["grads"], kw["stats"]
    monkeypatch.setattr(td3, "dpg_actor_grad_ctde", launch)
    kw = dict(noise=torch.zeros((15, 3)[k]), nominal=torch.zeros((4, 1)[k]))
    stats = td3_actor_loss_ctde(mods, critic, buf, k, torch.zeros(5, dtype=torch.int64), **kw)
    own = list(mods[k].parameters())
    assert all(p.grad is not None and p.grad.shape == p.shape for p in own)
    assert [g.data_ptr() for g in seen["grads"].values()] == [p.grad.data_ptr() for p in own] and seen["k"] == k and "action_other" not in seen
    assert all(a is b for a, b in zip(held, (p.grad for p in other))) and held[1] is None and bool((held[0] == 3.5).all())
    assert seen["obs"] is buf.obs and seen["obs_next"] is buf.obs_next and [a.dims for a in seen["actors"]] == [(15, 16, 4), (3, 4, 1)]
    assert ("actor_ctde", k, 5, 0) in buf._cache and seen["workspace"].numel() == 11 and stats is buf._cache[("actor_ctde", k, 5, 0)][1]
    again = td3_actor_loss_ctde(mods, critic, buf, k, torch.zeros(5, dtype=torch.int64), **kw)
    assert again is stats and len(buf._cache) == 1
