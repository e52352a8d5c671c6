"""The centralized-critic (CTDE) half of TD3 and SAC on the device (qr_ctde_twinq_target, qr_ctde_sac_target, qr_ctde_twinq_grad;
td3.td3_target_ctde / twinq_grad_ctde / td3_critic_loss_ctde, sac.sac_target_ctde / sac_critic_loss_ctde) without a GPU: the float64
restatement of tests/ctde_ref.py against the reference's own autograd (tests/golden/ctde_critic.npz, tools/gen_golden_ctde_critic.py),
the ReLU margin of every case, the C-ABI struct layouts, every documented error of the C entries and of the Python helpers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctde_ref  # noqa: E402
import td3_ref  # noqa: E402
from ctde_ref import CASES  # noqa: E402
from td3_ref import NAMES  # noqa: E402

SHAPES = {"ctde": ((15, 3), (4, 1), 62), "h64": ((15, 3), (4, 1), 64), "h5": ((15, 3), (4, 1), 5), "w28": ((16, 4), (5, 3), 20)}
GRAD_CASES = tuple(SHAPES)


@pytest.fixture(scope="module")
def fixture():
    return ctde_ref.load()


def test_fixture_holds_the_cases_and_their_active_clamps(fixture):
    assert tuple(str(n) for n in fixture["cases"]) == CASES
    assert os.path.getsize(ctde_ref.GOLDEN) <= 1_000_000
    for name in CASES:
        c = ctde_ref.case(fixture, name)
        od, ad, H = SHAPES.get(name, SHAPES["h5"])
        for m in (0, 1):
            assert c[f"obs{m}"].shape == (130, od[m]) and c[f"obsn{m}"].shape == (130, od[m]) and c[f"act{m}"].shape == (130, ad[m])
            assert c[f"td3_a{m}"].shape == (130, ad[m]) and c[f"sac_a{m}"].dtype == np.float64 and c[f"obs{m}"].dtype == np.float32
        assert c["rwd"].shape == (130, 2) and c["done"].shape == (130, 2) and tuple(c["obs_dims"]) == od and tuple(c["action_dims"]) == ad
        assert c["c_fc1_w"].shape == (H, sum(od) + sum(ad)) and c["t_fc5_w"].shape == (H, H)
        assert ("g0_fc1_w" in c) == (name in GRAD_CASES) == bool(c["has_grads"]) and ("p0_fc1_w" in c) == (name != "w28") == ("s1_mean_w" in c)
        assert ("eps0" in c) == (name != "noeps") and ("elp1" in c) == (name not in ("noeps", "onedraw"))
        for k in (0, 1):
            assert c[f"td3_y{k}"].shape == (130,) and c[f"sac_logp{k}"].shape == (130,) and c[f"sac_y{k}"].dtype == np.float64
    assert not np.array_equal(ctde_ref.case(fixture, "ctde")["td3_y0"], ctde_ref.case(fixture, "ctde")["td3_y1"])   # both agents' columns
    sat = ctde_ref.case(fixture, "sat")
    nc_rows, ma_rows = np.zeros(130, bool), np.zeros(130, bool)
    for m in (0, 1):
        raw = float(sat["target_noise"]) * sat[f"eps{m}"].astype(np.float64)
        mean = td3_ref.actor_forward([sat[f"p{m}_{n}"].astype(np.float64) for n in ctde_ref.TD3_ACTOR], sat[f"obsn{m}"].astype(np.float64))
        nc_rows |= (np.abs(raw) > sat["noise_clip"]).any(1)
        ma_rows |= (np.abs(mean + np.clip(raw, -0.5, 0.5)) > sat["max_action"]).any(1)
    assert nc_rows.sum() >= 10 and ma_rows.sum() >= 10 and sat["done"][:, 0].sum() >= 10 and sat["done"][:, 1].sum() >= 10
    clamp = ctde_ref.case(fixture, "clamp")
    for m in (0, 1):
        ls = ctde_ref.raw_log_std(clamp, m)
        assert ((ls < -20) | (ls > 2)).any(1).sum() >= 10, m
    two, one = ctde_ref.case(fixture, "twodraw"), ctde_ref.case(fixture, "onedraw")
    assert not np.array_equal(two["elp0"], two["eps0"]) and np.array_equal(two["sac_a0"], one["sac_a0"])
    assert not np.array_equal(two["sac_logp0"], one["sac_logp0"]) and not np.array_equal(two["sac_y1"], one["sac_y1"])


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.abs(got.reshape(want.shape) - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), what


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(fixture, name):
    c = ctde_ref.case(fixture, name)
    for k in (0, 1):
        a0, a1, y = ctde_ref.td3_target_f64(c, k)
        for got, key in ((a0, "td3_a0"), (a1, "td3_a1"), (y, f"td3_y{k}")):
            _close(got, c[key], (key, k))
        a0, a1, logp, ys = ctde_ref.sac_target_f64(c, k)
        for got, key in ((a0, "sac_a0"), (a1, "sac_a1"), (logp, f"sac_logp{k}"), (ys, f"sac_y{k}")):
            _close(got, c[key], (key, k))
        if name in GRAD_CASES:
            loss, m1, m2, grads = ctde_ref.twinq_grad_f64(c, c[f"td3_y{k}"])
            for n in NAMES:
                _close(grads[n], c[f"g{k}_{n}"], (n, k))
            for got, key in ((loss, "loss"), (m1, "mse1"), (m2, "mse2")):
                _close(got, c[f"g{k}_{key}"], (key, k))


@pytest.mark.parametrize("name", CASES)
def test_every_case_keeps_the_relu_margin(fixture, name):
    c = ctde_ref.case(fixture, name)
    m = ctde_ref.margin(c)
    assert m >= td3_ref.MARGIN == 2e-5
    assert abs(m - float(c["min_abs_z"])) <= 1e-12 * max(1.0, m)


STRUCTS = ("QrCtdeTransitions", "QrCtdeTd3Target", "QrCtdeSacTarget")


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
        for fl, _ in ct._fields_:
            assert int(out[f"{sname}.{fl}"]) == getattr(ct, fl).offset, (sname, fl)
    lib = L.load()
    new = {"qr_ctde_twinq_target", "qr_ctde_sac_target", "qr_ctde_twinq_grad", "qr_ctde_twinq_workspace_bytes"}
    assert new <= set(L.SYMBOLS) and all(hasattr(lib, s) for s in new)
    assert int(out["abi"]) == L.ABI_VERSION == 16 and lib.qr_abi_version() == 16


NULL, KIND, SIZE, ALIGN = -1, -2, -3, -4
ACTOR_W = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b")


def _fake(od=(15, 3), ad=(4, 1), hidden=62, batch=130, sac=False):
    """Structs that pass every check, on fake device addresses (never touched: every case below returns before a launch — the
    gradient's workspace is one byte short, a target is refused last through y = NULL unless the case edits something else)."""
    from gym_rotor_amd import _lib as L
    s = {}
    for m, dims in enumerate(((15, 16, 4), (3, 4, 1))):
        p = L.QrActor()
        for k, n in enumerate(ACTOR_W):
            setattr(p, n, 0x900000 + 0x100000 * m + 0x1000 * k)
        if sac:
            p.log_std_w, p.log_std_b = 0x980000 + 0x100000 * m, 0x981000 + 0x100000 * m
        p.obs_dim, p.hidden_dim, p.action_dim, p.squash = *dims, (L.ACTOR_TANH_SAMPLE if sac else L.ACTOR_TANH_MEAN)
        s[f"p{m}"] = p
    q = L.QrQCritic()
    for k, n in enumerate(NAMES):
        setattr(q, n, 0x10000 + 0x1000 * k)
    q.obs_dim, q.action_dim, q.hidden_dim, q.reserved0 = sum(od), sum(ad), hidden, 0
    b = L.QrCtdeTransitions()
    for m in (0, 1):
        b.obs[m], b.obs_next[m], b.action[m] = 0x100000 + 0x8000 * m, 0x110000 + 0x8000 * m, 0x120000 + 0x8000 * m
        b.obs_dim[m], b.action_dim[m], b.row_stride[m], b.col_offset[m] = od[m], ad[m], ad[m], 0
    b.reward, b.done, b.index, b.batch, b.rows, b.reward_stride, b.done_stride = 0x130000, 0x140000, 0x150000, batch, 130, 1, 1
    two = lambda a: (C.c_void_p * 2)(a, a + 0x8000)
    s.update(q=q, b=b, t=L.QrCtdeTd3Target(two(0x200000), two(0x210000), 0x220000, 0.99, 0.2, 0.5, 1.0),
             u=L.QrCtdeSacTarget(two(0x200000), 0x230000, two(0x210000), 0x240000, None, 0x220000, two(0x250000), 0x260000, 0.99, 0.2, 0, 0))
    g = L.QrTwinQGrad(*[0x800000 + 0x1000 * k for k in range(13)], 0x300000, 0x400000)
    g.workspace_bytes = L.load().qr_ctde_twinq_workspace_bytes(sum(od) + sum(ad), hidden, batch, 0) - 1
    g.max_workgroups, g.reserved0 = 0, 0
    s["g"] = g
    return s


def _ref(x):
    return None if x is None else C.byref(x)


def _apply(s, edit):
    """`<struct>_<field>` = value; `<field>@<m>` sets element m of an array member; the keys p0 / p1 replace an actor."""
    for k, v in edit.items():
        if k in ("p0", "p1"):
            s[k] = v
            continue
        key, name = (k[:2], k[3:]) if k[:2] in ("p0", "p1") else (k[0], k[2:])
        if "@" in name:
            name, m = name.split("@")
            getattr(s[key], name)[int(m)] = v
        else:
            setattr(s[key], name, v)


def test_ctde_twinq_grad_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()
    call = lambda s: lib.qr_ctde_twinq_grad(_ref(s["q"]), _ref(s["b"]), _ref(s["g"]), None)
    assert call(_fake()) == SIZE                                     # every other check passes: only the workspace is one byte short
    for k in "qbg":
        assert call({**_fake(), k: None}) == NULL

    def expect(code, what, fake={}, **edit):
        s = _fake(**fake)
        _apply(s, edit)
        assert call(s) == code, (what, edit)

    for n in NAMES:
        expect(NULL, "weight", **{"q_" + n: None})
        expect(NULL, "gradient", **{"g_" + n: None})
    for n in ("stats", "y", "workspace"):
        expect(NULL, n, **{"g_" + n: None})
    for m in (0, 1):
        expect(NULL, "obs", **{f"b_obs@{m}": None})
        expect(NULL, "action", **{f"b_action@{m}": None})
    expect(SIZE, "optional pointers", b_index=None, b_reward=None, b_done=None, **{"b_obs_next@0": None, "b_obs_next@1": None})
    expect(SIZE, "legal strides", **{"b_row_stride@0": 9, "b_col_offset@0": 5, "b_row_stride@1": 3, "b_col_offset@1": 2})
    for fake in (dict(od=(16, 4), ad=(5, 3)), dict(od=(1, 1), ad=(1, 1), hidden=1), dict(hidden=64), dict(od=(3, 15), ad=(1, 4))):
        expect(SIZE, "legal widths", fake=fake)
    big = dict(g_workspace_bytes=1 << 40)
    for edit in ({"b_obs_dim@0": 14}, {"b_obs_dim@1": 4}, {"b_action_dim@0": 5}, {"b_action_dim@1": 0}, {"b_obs_dim@0": 18, "b_obs_dim@1": 0},
                 {"b_obs_dim@0": 19, "b_obs_dim@1": -1}, dict(q_obs_dim=24), dict(q_hidden_dim=0), dict(q_hidden_dim=65), dict(q_reserved0=1),
                 dict(g_reserved0=1), dict(b_batch=0), dict(b_rows=0), {"b_row_stride@1": 0}, {"b_col_offset@0": -1}, {"b_col_offset@1": 1},
                 dict(g_max_workgroups=-1)):
        expect(SIZE, "sizes", **big, **edit)
    for edit in ({"b_obs@1": 0x108002}, {"b_action@0": 0x120001}, dict(g_fc5_w=0x800001), dict(q_fc6_b=0x15002), dict(g_y=0x300002),
                 dict(b_index=0x150004), dict(g_workspace=0x400004)):
        expect(ALIGN, "alignment", **big, **edit)
    ws, ws1 = lib.qr_ctde_twinq_workspace_bytes, lib.qr_twinq_workspace_bytes
    assert ws(23, 62, 130, 0) == ws1(23, 62, 130, 0) == 2 * 3 * (62 * 23 + 62 + 62 * 62 + 62 + 62 + 1 + 2) * 8
    assert ws(28, 64, 64 * 5000, 0) == ws1(28, 64, 64 * 5000, 0) and ws(4, 1, 1, 0) == 2 * (4 + 1 + 1 + 1 + 1 + 1 + 2) * 8
    for bad in ((3, 62, 10, 0), (29, 62, 10, 0), (23, 0, 10, 0), (23, 65, 10, 0), (23, 62, 0, 0), (23, 62, 10, -1)):
        assert ws(*bad) == SIZE, bad


@pytest.mark.parametrize("sac", (False, True))
def test_ctde_target_argument_errors_without_gpu(sac):
    from gym_rotor_amd import _lib as L
    lib = L.load()
    T = "u" if sac else "t"

    def call(s):
        fn = lib.qr_ctde_sac_target if sac else lib.qr_ctde_twinq_target
        return fn(_ref(s["p0"]), _ref(s["p1"]), _ref(s["q"]), _ref(s["b"]), _ref(s[T]), None)

    def expect(code, what, fake={}, **edit):
        s = _fake(sac=sac, **fake)
        setattr(s[T], "y", None)                                     # the last pointer check: every legal case ends here
        _apply(s, {(T + k[1:] if k[0] == "t" and k[1] == "_" else k): v for k, v in edit.items()})
        assert call(s) == code, (what, edit)

    Y = dict(t_y=0x220000)
    expect(NULL, "everything else is legal")
    for k in ("q", "b", T):
        assert call({**_fake(sac=sac), k: None}) == NULL
    expect(NULL, "legal sizes", fake=dict(hidden=1, batch=1 << 33))
    expect(NULL, "no actors: supplied a'", p0=None, p1=None, fake=dict(od=(16, 4), ad=(5, 3)))
    expect(NULL, "one actor only", p1=None, **Y)
    expect(NULL, "one actor only", p0=None, **Y)
    expect(NULL, "no actors and no action_next", p0=None, p1=None, **Y, **{"t_action_next@1": None})
    if sac:
        expect(NULL, "no actors and no logp_next", p0=None, p1=None, **Y, t_logp_next=None)
        expect(NULL, "optional", t_eps_logp=None, t_logp_out=None, t_alpha_dev=None, **{"t_action_out@0": None, "t_action_out@1": None})
    expect(NULL, "eps is optional", **{"t_eps@0": None, "t_eps@1": None})
    expect(NULL, "obs and action are unread", **{"b_obs@0": None, "b_action@1": None, "b_row_stride@0": 0})
    for n in NAMES:
        expect(NULL, "weight", **Y, **{"q_" + n: None})
    for m in (0, 1):
        for n in ACTOR_W:
            expect(NULL, "actor weight", **Y, **{f"p{m}_{n}": None})
        expect(NULL, "obs_next", **Y, **{f"b_obs_next@{m}": None})
    for n in ("reward", "done"):
        expect(NULL, n, **Y, **{"b_" + n: None})
    for m in (0, 1):
        expect(KIND, "the other form", **{f"p{m}_squash": L.ACTOR_TANH_MEAN if sac else L.ACTOR_TANH_SAMPLE})
        if sac:
            expect(KIND, "no log_std head", **{f"p{m}_log_std_w": None})
        else:
            expect(KIND, "log_std head", **{f"p{m}_log_std_w": 0x990000, f"p{m}_log_std_b": 0x991000})
    for edit in ({"b_obs_dim@0": 14}, {"b_action_dim@1": 2}, {"b_obs_dim@1": 0, "b_obs_dim@0": 18}, dict(q_obs_dim=19), dict(q_hidden_dim=0),
                 dict(q_hidden_dim=65), dict(q_reserved0=7), dict(p0_obs_dim=23), dict(p0_hidden_dim=8), dict(p1_obs_dim=15, p1_hidden_dim=16, p1_action_dim=4),
                 dict(p1_hidden_dim=5), dict(b_batch=0), dict(b_rows=0), dict(b_reward_stride=0), dict(b_done_stride=-1)):
        expect(SIZE, "sizes", **edit)
    expect(SIZE, "actors beside other widths", fake=dict(od=(14, 4), ad=(4, 1)))
    expect(SIZE, "actors in the other order", fake=dict(od=(3, 15), ad=(1, 4)))
    scalars = (dict(t_discount=-1.0), dict(t_alpha=float("nan")), dict(t_alpha=float("inf")), dict(t_agent=2), dict(t_agent=-1), dict(t_reserved0=1)) if sac \
        else (dict(t_noise_clip=-0.5), dict(t_max_action=float("nan")), dict(t_max_action=float("inf")))
    for edit in scalars:
        expect(SIZE, "scalars", **edit)
    if sac:
        expect(NULL, "agent 1", t_agent=1)
    align = [{"b_obs_next@1": 0x118002}, dict(b_reward=0x130001), dict(b_done=0x140003), {"t_eps@1": 0x208002}, dict(t_y=0x220001),
             dict(q_fc4_w=0x13002), dict(p1_mean_w=0xa04001), dict(b_index=0x150004)]
    align += [dict(t_eps_logp=0x230002), {"t_action_out@1": 0x258001}, dict(t_logp_out=0x260002), dict(t_alpha_dev=0x270001)] if sac else []
    for edit in align:
        expect(ALIGN, "alignment", **{**Y, **edit})


# ---------------------------------------------------------------------------------------------------------------------------
# the Python helpers
# ---------------------------------------------------------------------------------------------------------------------------
class _Twin(torch.nn.Module):
    def __init__(self, din=23, hidden=62):
        super().__init__()
        for k, (i, o) in enumerate(((din, hidden), (hidden, hidden), (hidden, 1)) * 2, 1):
            setattr(self, f"fc{k}", torch.nn.Linear(i, o))


class _Td3Actor(torch.nn.Module):
    def __init__(self, D, H, A):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(D, H), torch.nn.Linear(H, H), torch.nn.Linear(H, A)


class _SacActor(torch.nn.Module):
    def __init__(self, D, H, A):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(D, H), torch.nn.Linear(H, H)
        self.mean_linear, self.log_std_linear = torch.nn.Linear(H, A), torch.nn.Linear(H, A)


def _agents(rows=10, od=(15, 3), ad=(4, 1)):
    return [{"obs": torch.zeros(rows, od[m]), "act": torch.zeros(rows, ad[m]), "rwd": torch.zeros(rows), "obs_next": torch.zeros(rows, od[m]),
             "done": torch.zeros(rows)} for m in (0, 1)]


def test_python_helpers_refuse_bad_arguments():
    from gym_rotor_amd import (ActorParams, QCriticParams, ReplayBuffer, sac_critic_loss_ctde, sac_target_ctde, td3_critic_loss_ctde, td3_target_ctde,
                               twinq_grad_ctde)
    q = QCriticParams.from_module(_Twin(), 5)
    assert q.dims == (18, 5, 62)
    td3 = [ActorParams.from_td3_module(_Td3Actor(*d), 0.0) for d in ((15, 16, 4), (3, 4, 1))]
    sac = [ActorParams.from_sac_module(_SacActor(*d)) for d in ((15, 16, 4), (3, 4, 1))]
    t, idx = _agents(), torch.zeros(5, dtype=torch.int64)
    for fn, actors in ((td3_target_ctde, td3), (sac_target_ctde, sac)):
        what = fn.__name__
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(actors, q, t, 0, idx)
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(actors, q, t, 1, idx, noise=(torch.zeros(5, 4), None))

        def bad(match, *args, **kw):
            with pytest.raises(ValueError, match=match):
                fn(*args, **kw)
        bad("k must be", actors, q, t, 2, idx)
        bad("pair", actors, q, t[:1], 0, idx)
        bad("two agents", actors, q, ReplayBuffer(4, (23,), (4,), "cpu"), 0, idx)
        bad("add up", actors, QCriticParams.from_module(_Twin(24), 5), t, 0, idx)
        bad("add up", actors, QCriticParams.from_module(_Twin(23), 4), t, 0, idx)
        bad("obs_next", actors, q, [{**t[0], "obs_next": torch.zeros(10, 15, dtype=torch.float64)}, t[1]], 0, idx)
        bad("obs_next", actors, q, [t[0], {**t[1], "obs_next": torch.zeros(9, 3)}], 0, idx)
        bad("act", actors, q, [t[0], {**t[1], "act": None}], 0, idx)
        bad("rwd", actors, q, [{**t[0], "rwd": torch.zeros(9)}, t[1]], 0, idx)
        bad("done", actors, q, [t[0], {**t[1], "done": torch.zeros(10, dtype=torch.bool)}], 1, idx)
        bad("index", actors, q, t, 0, idx.int())
        bad("actors", actors[:1], q, t, 0, idx)
        bad("actors", (actors[0], None), q, t, 0, idx)
        bad(r"noise\[1\]", actors, q, t, 0, idx, noise=(None, torch.zeros(5, 4)))
        bad(r"noise\[0\]", actors, q, t, 0, idx, noise=(torch.zeros(10, 4), None))
        bad("noise", actors, q, t, 0, idx, noise=(torch.zeros(5, 4),))
        bad("action_next", None, q, t, 0, idx)
        bad("action_next", None, q, t, 0, idx, action_next=(torch.zeros(5, 4), None))
        bad(r"action_next\[1\]", None, q, t, 0, idx, action_next=(torch.zeros(5, 4), torch.zeros(5, 2)))
        bad("out", actors, q, t, 0, idx, out=torch.zeros(4))
        bad("MLP_Actor_TD3" if fn is td3_target_ctde else "MLP_Actor_SAC", sac if fn is td3_target_ctde else td3, q, t, 0, idx)
        bad("the critic reads", actors[::-1], q, t, 0, idx)
        half = list(actors)
        half[1] = ActorParams.from_td3_module(_Td3Actor(3, 4, 1), 0.0) if fn is td3_target_ctde else ActorParams.from_sac_module(_SacActor(3, 4, 1))
        half[1].fc2_w = half[1].fc2_w.double()
        bad("fc2_w", half, q, t, 0, idx)
        assert what in ("td3_target_ctde", "sac_target_ctde")
    # actors of a legal rollout size that are not the Decoupled pair
    t33 = _agents(od=(3, 3), ad=(1, 1))
    with pytest.raises(ValueError, match="actor 0 must have the sizes"):
        td3_target_ctde([td3[1], td3[1]], QCriticParams.from_module(_Twin(8, 8), 2), t33, 0, idx)
    an = (torch.zeros(5, 4), torch.zeros(5, 1))
    for kw, pat in ((dict(noise_logp=torch.zeros(5, 1)), "noise_logp"), (dict(action_out=(torch.zeros(5, 4), torch.zeros(5, 2))), r"action_out\[1\]"),
                    (dict(logp_out=torch.zeros(4)), "logp_out"), (dict(alpha=-1.0), "alpha"), (dict(alpha=torch.zeros(2)), "alpha"),
                    (dict(discount=float("inf")), "discount")):
        with pytest.raises(ValueError, match=pat):
            sac_target_ctde(sac, q, t, 0, idx, **kw)
    with pytest.raises(ValueError, match="logp_next"):
        sac_target_ctde(None, q, t, 0, idx, action_next=an)
    with pytest.raises(ValueError, match="logp_next"):
        sac_target_ctde(None, q, t, 0, idx, action_next=an, logp_next=torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        sac_target_ctde(None, q, t, 1, idx, action_next=an, logp_next=torch.zeros(5), noise_logp=None)
    # twinq_grad_ctde
    obs, act, y = (t[0]["obs"], t[1]["obs"]), (t[0]["act"], t[1]["act"]), torch.zeros(5)
    with pytest.raises(RuntimeError, match="GPU only"):
        twinq_grad_ctde(q, obs, act, y, idx)
    for args, kw, pat in (((obs[:1], act, y, idx), {}, "pairs"), (((obs[0], torch.zeros(10, 4)), act, y, idx), {}, "add up"),
                          ((obs, (act[0], torch.zeros(10, 2)), y, idx), {}, "add up"), (((obs[0], torch.zeros(9, 3)), act, y, idx), {}, r"obs\[1\]"),
                          (((obs[0].double(), obs[1]), act, y, idx), {}, r"obs\[0\]"), ((obs, (act[0], torch.zeros(9, 1)), y, idx), {}, r"action\[1\]"),
                          ((obs, (torch.zeros(4, 10).T, act[1]), y, idx), {}, r"action\[0\]"), ((obs, act, torch.zeros(6), idx), {}, "y"),
                          ((obs, act, y, idx.float()), {}, "index"), ((obs, act, y, idx), dict(stats=torch.zeros(3)), "stats"),
                          ((obs, act, y, idx), dict(grads={n: torch.zeros(s) for n, s in q.shapes.items() if n != "fc4_b"}), "fc4_b")):
        with pytest.raises(ValueError, match=pat):
            twinq_grad_ctde(q, *args, **kw)
    # the live-module forms
    for fn in (td3_critic_loss_ctde, sac_critic_loss_ctde):
        with pytest.raises(ValueError, match="ReplayBuffer"):
            fn(_Twin(), _Twin(), [], t, 0, idx)
    buf = ReplayBuffer(10, (15, 3), (4, 1), "cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        td3_critic_loss_ctde(_Twin(), _Twin(), [_Td3Actor(15, 16, 4), _Td3Actor(3, 4, 1)], buf, 1, idx)
    with pytest.raises(RuntimeError, match="GPU only"):
        sac_critic_loss_ctde(_Twin(), _Twin(), [_SacActor(15, 16, 4), _SacActor(3, 4, 1)], buf, 0, idx)
    assert ("td3_ctde", 1, 5, 0) in buf._cache and ("sac_ctde", 0, 5, 0) in buf._cache       # keys of their own
    with pytest.raises(ValueError):
        td3_critic_loss_ctde(_Twin(27), _Twin(27), [_Td3Actor(15, 16, 4), _Td3Actor(3, 4, 1)], buf, 0, idx)   # 27 != 18 + 5


def test_torch_ops_are_registered():
    ops = torch.ops.gym_rotor_amd
    assert all(hasattr(ops, n) for n in ("qr_ctde_twinq_target", "qr_ctde_sac_target", "qr_ctde_twinq_grad"))
    q = _Twin()
    w = [p.data for k in range(1, 7) for p in (getattr(q, f"fc{k}").weight, getattr(q, f"fc{k}").bias)]
    t, idx, y = _agents(), torch.zeros(5, dtype=torch.int64), torch.zeros(5)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.qr_ctde_twinq_grad(w, t[0]["obs"], t[1]["obs"], t[0]["act"], t[1]["act"], y, idx, [torch.zeros_like(x) for x in w], torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.qr_ctde_twinq_target([], w, t[0]["obs_next"], t[1]["obs_next"], t[0]["act"], t[1]["act"], t[0]["rwd"], t[0]["done"], idx, None, None,
                                 torch.zeros(5, 4), torch.zeros(5, 1), y, 0.99, 0.2, 0.5, 1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.qr_ctde_sac_target([], w, 1, t[0]["obs_next"], t[1]["obs_next"], t[0]["act"], t[1]["act"], t[1]["rwd"], t[1]["done"], idx, None, None, None,
                               torch.zeros(5, 4), torch.zeros(5, 1), torch.zeros(5), y, None, None, None, 0.99, 0.2)
