"""Agent k's SAC actor half under the centralized (CTDE) twin critic (qr_ctde_sac_actor_grad; sac.sac_actor_grad_ctde /
sac_actor_workspace_bytes_ctde / sac_actor_loss_ctde) without a GPU: the float64 restatement of tests/sac_ctde_actor_ref.py against the
reference's own autograd (tests/golden/sac_ctde_actor.npz, tools/gen_golden_sac_ctde_actor.py), the margins and conditions of every
case, the new struct's layout, every documented error of the two C entries in their order, and of the three Python functions."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sac_ctde_actor_ref as R  # noqa: E402
from sac_ctde_actor_ref import ACTOR_NAMES, CASES  # noqa: E402
from td3_ref import NAMES  # noqa: E402
from test_ctde_critic_host import ACTOR_W, ALIGN, KIND, NULL, SIZE, _apply, _fake, _ref, _SacActor, _Twin  # noqa: E402

# name: (obs widths, action widths, critic hidden, k)
DEC = ((15, 3), (4, 1))
SHAPES = {"k0": (*DEC, 62, 0), "k1": (*DEC, 62, 1), "h64": (*DEC, 64, 1), "h5": (*DEC, 5, 0), "noreg": (*DEC, 62, 0), "noeps": (*DEC, 62, 0),
          "onedraw": (*DEC, 62, 0), "alpha0": (*DEC, 62, 0), "clamp": (*DEC, 62, 0), "sat0": (*DEC, 62, 0), "sat1": (*DEC, 62, 1),
          "w28": ((15, 5), (4, 4), 62, 0)}
# The saturated cases: tanh and exp of NumPy (libm) against torch's differ in the last bits, and 1 / (1 - a^2 + 1e-6) and exp(ls)
# magnify that.  The bound is FOUR TIMES the largest relative difference measured on this fixture (DESIGN.md §8.14 has the
# measurements: clamp 2.73e-10, sat0 1.22e-13, sat1 2.36e-14), and has to stay below 1e-8.
SAT_TOL = {"clamp": 4 * 2.73e-10, "sat0": 4 * 1.22e-13, "sat1": 4 * 2.36e-14}


@pytest.fixture(scope="module")
def fixture():
    return R.load()


def test_fixture_holds_the_cases(fixture):
    assert tuple(str(n) for n in fixture["cases"]) == CASES == tuple(SHAPES)
    assert os.path.getsize(R.GOLDEN) <= 1_000_000
    for name in CASES:
        c = R.case(fixture, name)
        od, ad, H, k = SHAPES[name]
        assert c["k"] == k and c["c_fc1_w"].shape == (H, sum(od) + sum(ad)) and c["c_fc5_w"].shape == (H, H) and c["c_fc4_w"].dtype == np.float32
        for m in (0, 1):
            assert c[f"obs{m}"].shape == (130, od[m]) and c[f"obs_next{m}"].shape == (130, od[m]) and c[f"obs{m}"].dtype == np.float32
        assert (R.actor_of(c, 1 - k) is None) == (name in R.SUPPLIED) == ("action_other" in c)
        if name in R.SUPPLIED:
            assert c["action_other"].shape == (130, ad[1 - k]) and c["action_other"].dtype == np.float32 and "eps1" not in c
            assert np.array_equal(c["other_action"], c["action_other"].astype(np.float64))
        assert c["other_action"].shape == (130, ad[1 - k]) and c["other_action"].dtype == np.float64
        assert c["a%d_fc1_w" % k].shape == ((16, 15), (4, 3))[k] and c["g_log_std_w"].shape == ((4, 16), (1, 4))[k] and c["g_fc1_w"].dtype == np.float64
        assert c["noise"].shape == (od[k],) and c["nominal"].shape == (ad[k],) and c["stats"].shape == (6,)
        assert c["lam"] == ((0.0, 0.0, 0.0) if name == "noreg" else (0.4, 0.3, 0.6)) and c["max_action"] == (0.5 if name.startswith("sat") else 1.0)
        assert c["alpha"] == (0.0 if name == "alpha0" else 0.2) and c["target_entropy"] == -float(ad[k])
        have = [n for n in R.EPS if n in c]
        want = [] if name == "noeps" else [n for n in R.EPS if not (name == "onedraw" and n == "eps_logp") and not (name == "w28" and n == "eps1")]
        assert have == want
        for n in have:
            assert c[n].shape == (130, ad[int(n[3])] if n in ("eps0", "eps1") else ad[k]) and c[n].dtype == np.float32
    s0, s1, k0 = (R.case(fixture, n) for n in ("sat0", "sat1", "k0"))
    assert all(np.array_equal(s0[key], s1[key]) for key in ("obs0", "obs1", "a0_fc1_w", "a1_mean_w", "c_fc5_w"))   # one set of networks, both k
    for name in ("noreg", "noeps", "onedraw", "alpha0"):
        c = R.case(fixture, name)
        assert all(np.array_equal(k0[key], c[key]) for key in ("a0_fc1_w", "a1_log_std_w", "c_fc2_w")) and not np.array_equal(k0["obs0"], c["obs0"])


def _close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got.reshape(want.shape) - want).max() / max(1.0, np.abs(want).max())
    assert err <= tol, (what, err)
    return err


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(fixture, name):
    c = R.case(fixture, name)
    stats, grads, alpha_grad = R.case_f64(c)
    tol = SAT_TOL.get(name, 1e-12)
    assert tol < 1e-8 and set(SAT_TOL) == set(R.SATURATED)
    worst = max([_close(grads[n], c["g_" + n], tol, (name, n)) for n in ACTOR_NAMES] +
                [_close(stats[j], c["stats"][j], tol, (name, key)) for j, key in enumerate(R.STATS)] +
                [_close(alpha_grad, c["alpha_grad"], tol, (name, "alpha_grad"))])
    print(f"{name}: worst relative difference {worst:.2e} (bound {tol:.2e})")
    a, kw = R.case_args(c)
    ao = R.other_action(a[0], a[2], a[4], a[5], a[6].get("eps_other"))
    _close(ao, c["other_action"], tol, (name, "other_action"))
    if name == "k0":
        # the other agent's action is a value: scaling its mean head moves agent k's gradients; its own obs_next does not enter at all
        w1 = [t.copy() for t in R.actor_of(c, 1)]
        w1[4] = w1[4] * 2
        moved = R.ctde_sac_actor_grad_f64([R.actor_of(c, 0), w1], *a[1:], **kw)[1]
        assert np.abs(moved["fc1_w"] - grads["fc1_w"]).max() > 1e-6
        # the second sample carries the entropy term: without eps_logp, stats[2] is the first sample's logp, another number
        one = dict(a[6])
        del one["eps_logp"]
        s1 = R.ctde_sac_actor_grad_f64(*a[:6], one, **kw)[0]
        assert abs(s1[2] - stats[2]) > 1e-3 and s1[1] == stats[1]
        # ... and eps_logp given as the first draw IS the one-draw form
        same = dict(a[6], eps_logp=a[6]["eps"])
        s2, g2, _ = R.ctde_sac_actor_grad_f64(*a[:6], same, **kw)
        _close(s2, s1, 1e-12, "same draw")
        _close(g2["fc1_w"], R.ctde_sac_actor_grad_f64(*a[:6], one, **kw)[1]["fc1_w"], 1e-12, "same draw")


@pytest.mark.parametrize("name", CASES)
def test_every_case_keeps_its_margins_and_conditions(fixture, name):
    c = R.case(fixture, name)
    a, kw = R.case_args(c)
    m = R.margins(*a, **kw)
    got = np.array([m["relu"], m["ls"], m["clamp"], m["q"]])
    assert (got >= R.MARGIN).all() and R.MARGIN == 2e-5
    assert np.array_equal(np.isinf(got), np.isinf(c["margins"])) and np.isinf(got[2]) == (c["max_action"] >= 1.0 or name == "noreg")
    fin = np.isfinite(got)
    assert (np.abs(got[fin] - c["margins"][fin]) <= 1e-9 * np.maximum(1.0, got[fin])).all()
    stats, _, _, passes, (c1, c2), pother = R.ctde_sac_actor_grad_f64(*a, detail=True, **kw)
    assert 0.1 <= stats[5] <= 0.9 and 0 < int((c2[2] < c1[2]).sum()) < 130           # rows on both sides of the min
    assert (pother is None) == (name in R.SUPPLIED)
    if name == "clamp":
        lsr, lso = passes[0]["lsr"], pother["lsr"]
        assert (lsr < -20).any() and (lsr > 2).any() and 0.1 <= stats[4] <= 0.9 and ((lso < -20) | (lso > 2)).any()
    else:
        assert stats[4] == 0.0
    if name.startswith("sat"):
        share = float(np.mean([(np.abs(p["a"]) > c["max_action"]).mean() for p in passes[2:]]))
        assert 0.2 <= share <= 0.8 and max(float(np.abs(p["u"]).max()) for p in passes) >= 4.0
    assert len(passes) == {"noreg": 2, "noeps": 4, "onedraw": 4}.get(name, 5)


def test_struct_mirrors_the_header(tmp_path):
    from gym_rotor_amd import _lib as L
    sname = "QrCtdeSacActorGrad"
    lines = [f'printf("{sname} %zu\\n", sizeof({sname}));'] + [f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));' for f, _ in L.QrCtdeSacActorGrad._fields_]
    lines += ['printf("base %zu\\n", sizeof(QrSacActorGrad));', 'printf("abi %d\\n", QR_ABI_VERSION);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out[sname]) == C.sizeof(L.QrCtdeSacActorGrad) == C.sizeof(L.QrSacActorGrad) + 32 and int(out["base"]) == C.sizeof(L.QrSacActorGrad)
    for fl, _ in L.QrCtdeSacActorGrad._fields_:
        assert int(out[f"{sname}.{fl}"]) == getattr(L.QrCtdeSacActorGrad, fl).offset, fl
    for fl, _ in L.QrSacActorGrad._fields_:                             # QrSacActorGrad's members first, in order, at its offsets
        assert getattr(L.QrCtdeSacActorGrad, fl).offset == getattr(L.QrSacActorGrad, fl).offset
    assert [f for f, _ in L.QrCtdeSacActorGrad._fields_[len(L.QrSacActorGrad._fields_):]] == ["agent", "reserved1", "eps_logp", "eps_other", "action_other"]
    lib = L.load()
    new = {"qr_ctde_sac_actor_grad", "qr_ctde_sac_actor_workspace_bytes"}
    assert new <= set(L.SYMBOLS) and all(hasattr(lib, s) for s in new)
    assert int(out["abi"]) == L.ABI_VERSION == 16 and lib.qr_abi_version() == 16


# a partial vector: the eight tensors and seven sums
NP = {0: 16 * 15 + 16 + 256 + 16 + 2 * (64 + 4) + 7, 1: 4 * 3 + 4 + 16 + 4 + 2 * (4 + 1) + 7}
SAC_W = ACTOR_W + ("log_std_w", "log_std_b")


def _fake_actor(k=0, od=(15, 3), ad=(4, 1), hidden=62, batch=130, supplied=False):
    """test_ctde_critic_host's fake structs (SAC actors) plus a QrCtdeSacActorGrad that passes every check with a workspace ONE BYTE
    SHORT: every legal case ends with the workspace's QR_E_SIZE, before any launch."""
    from gym_rotor_amd import _lib as L
    s = _fake(od, ad, hidden, batch, sac=True)
    g = L.QrCtdeSacActorGrad(*[0x800000 + 0x1000 * j for j in range(9)], 0x500000, 0x510000, 0x520000, 0x530000, 0x300000, 0x310000, None, 0x330000,
                             0x400000)
    g.workspace_bytes = L.load().qr_ctde_sac_actor_workspace_bytes(k, hidden, batch, 0) - 1
    g.alpha, g.target_entropy, g.lam_T, g.lam_S, g.lam_M, g.max_action = 0.2, -4.0, 0.4, 0.3, 0.6, 1.0
    g.max_workgroups, g.reserved0, g.agent, g.reserved1, g.eps_logp, g.eps_other = 0, 0, k, 0, 0x540000, 0x550000
    if supplied:
        s[f"p{1 - k}"], g.action_other, g.eps_other = None, 0x320000, None
    s["g"] = g
    return s


def test_ctde_sac_actor_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()
    call = lambda s: lib.qr_ctde_sac_actor_grad(_ref(s["p0"]), _ref(s["p1"]), _ref(s["q"]), _ref(s["b"]), _ref(s["g"]), None)
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
            expect(KIND, "the other form", fake=F, **big, **{f"p{m}_squash": L.ACTOR_TANH_MEAN, "b_batch": 0, "q_fc1_w": None})
            expect(KIND, "no log_std head", fake=F, **{f"p{m}_log_std_w": None})
            expect(KIND, "half a log_std head", fake=F, **{f"p{m}_log_std_b": None, "g_agent": 7})
        expect(KIND, "both actors and action_other", fake=F, g_action_other=0x320000, g_agent=5)
        # SIZE next, before any NULL
        for edit in (dict(g_agent=2), dict(g_agent=-1), {"b_obs_dim@0": 14}, {"b_action_dim@1": 2}, {"b_obs_dim@1": 0, "b_obs_dim@0": 18}, dict(q_obs_dim=19),
                     dict(q_action_dim=6), dict(q_hidden_dim=0), dict(q_hidden_dim=65), dict(q_reserved0=7), dict(g_reserved0=1), dict(g_reserved1=1),
                     dict(p0_obs_dim=23), dict(p0_hidden_dim=8), dict(p1_hidden_dim=5), dict(p1_obs_dim=15, p1_hidden_dim=16, p1_action_dim=4),
                     dict(b_batch=0), dict(b_rows=0), dict(g_max_workgroups=-1), dict(g_max_action=-1.0), dict(g_max_action=float("nan")),
                     dict(g_lam_T=-0.1), dict(g_lam_S=float("inf")), dict(g_lam_M=float("nan")), dict(g_alpha=-0.1), dict(g_alpha=float("inf")),
                     dict(g_alpha=float("nan")), dict(g_target_entropy=float("nan")), dict(g_target_entropy=float("-inf"))):
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
        for n in SAC_W:
            expect(NULL, "gradient", fake=F, **big, **{"g_" + n: None})
        for n in NAMES:
            expect(NULL, "critic weight: both networks are read", fake=F, **big, **{"q_" + n: None})
        for n in ("stats", "workspace", "noise", "nominal"):
            expect(NULL, n, fake=F, **big, **{"g_" + n: None})
        for m in (0, 1):
            expect(NULL, "obs", fake=F, **big, **{f"b_obs@{m}": None})
        expect(NULL, "obs_next[k]", fake=F, **big, **{f"b_obs_next@{k}": None})
        expect(SIZE, "what is not read, and every draw, may be NULL", fake=F, b_index=None, b_reward=None, b_done=None, p0_log_std=None, p1_log_std=None,
               g_eps=None, g_eps_reg=None, g_eps_next=None, g_eps_pert=None, g_eps_logp=None, g_eps_other=None, g_alpha_grad=None,
               **{f"b_obs_next@{o}": None, "b_action@0": None, "b_action@1": None, "b_row_stride@0": 0})
        expect(SIZE, "zero coefficients read none of their inputs", fake=F, g_lam_T=0.0, g_lam_S=0.0, g_lam_M=0.0, g_noise=None, g_nominal=None,
               **{f"b_obs_next@{k}": None})
        # ALIGN, then the workspace's SIZE
        for edit in ({"b_obs@0": 0x100002}, {"b_obs@1": 0x108001}, {f"b_obs_next@{k}": 0x110002 + 0x8000 * k}, dict(g_noise=0x300001), dict(g_nominal=0x310002),
                     dict(g_fc2_w=0x802001), dict(g_log_std_b=0x807002), dict(g_stats=0x808002), dict(q_fc3_b=0x15002), dict(q_fc6_w=0x1a001),
                     {f"p{k}_mean_w": 0x904001 + 0x100000 * k}, {f"p{k}_log_std_w": 0x980002 + 0x100000 * k}, {f"p{o}_fc2_b": 0x903002 + 0x100000 * o},
                     {f"p{o}_log_std_b": 0x981001 + 0x100000 * o}, dict(g_eps=0x500001), dict(g_eps_reg=0x510002), dict(g_eps_next=0x520003),
                     dict(g_eps_pert=0x530001), dict(g_eps_logp=0x540002), dict(g_eps_other=0x550001), dict(g_alpha_dev=0x560002), dict(g_alpha_grad=0x330001),
                     dict(b_index=0x150004), dict(g_workspace=0x400004)):
            expect(ALIGN, "alignment", fake=F, **big, **edit)
        expect(ALIGN, "action_other", fake=dict(k=k, supplied=True), **big, g_action_other=0x320002)
        expect(SIZE, "a short workspace comes last", fake=F, g_workspace_bytes=0)
    ws = lib.qr_ctde_sac_actor_workspace_bytes
    for k in (0, 1):
        assert ws(k, 62, 130, 0) == 3 * NP[k] * 8 == lib.qr_sac_actor_workspace_bytes(*((15, 16, 4), (3, 4, 1))[k], 62, 130, 0)
        assert ws(k, 1, 64 * 5000, 0) == 1024 * NP[k] * 8 and ws(k, 64, 64 * 5000, 7) == 7 * NP[k] * 8 and ws(k, 62, 1, 0) == NP[k] * 8
    for bad in ((2, 62, 10, 0), (-1, 62, 10, 0), (0, 0, 10, 0), (1, 65, 10, 0), (0, 62, 0, 0), (1, 62, 10, -1)):
        assert ws(*bad) == SIZE, bad


# ---------------------------------------------------------------------------------------------------------------------------
# the Python functions
# ---------------------------------------------------------------------------------------------------------------------------
def _pair(rows=10, od=(15, 3)):
    return [torch.zeros(rows, d) for d in od]


def test_python_functions_refuse_bad_arguments():
    from gym_rotor_amd import ActorParams, QCriticParams, ReplayBuffer, sac_actor_grad_ctde, sac_actor_loss_ctde, sac_actor_workspace_bytes_ctde
    q = QCriticParams.from_module(_Twin(), 5)
    actors = [ActorParams.from_sac_module(_SacActor(*d)) for d in ((15, 16, 4), (3, 4, 1))]
    obs, nxt, idx = _pair(), _pair(), torch.zeros(5, dtype=torch.int64)
    kw = dict(noise=torch.zeros(15), nominal=torch.zeros(4))
    kw1 = dict(noise=torch.zeros(3), nominal=torch.zeros(1))
    e4, e1 = torch.zeros(5, 4), torch.zeros(5, 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        sac_actor_grad_ctde(actors, q, obs, nxt, idx, k=0, eps=e4, eps_logp=e4, eps_other=e1, eps_reg=e4, eps_next=e4, eps_pert=e4, **kw)
    with pytest.raises(RuntimeError, match="GPU only"):
        sac_actor_grad_ctde(actors, q, obs, (None, nxt[1]), idx, k=1, eps=e1, eps_logp=e1, eps_other=e4, alpha_grad=torch.zeros(1), **kw1)
    with pytest.raises(RuntimeError, match="GPU only"):
        sac_actor_grad_ctde([actors[0], None], q, obs, nxt, idx, k=0, action_other=torch.zeros(5, 1), **kw)
    with pytest.raises(RuntimeError, match="GPU only"):                                       # free widths in the supplied form: 16+3 / 8+1
        sac_actor_grad_ctde([None, actors[1]], QCriticParams.from_module(_Twin(28), 9), _pair(od=(16, 3)), None, idx, k=1, action_other=torch.zeros(5, 8),
                            lam_T=0.0, **kw1)
    with pytest.raises(RuntimeError, match="GPU only"):                                       # zero coefficients need none of their inputs
        sac_actor_grad_ctde(actors, q, obs, None, None, k=0, lam_T=0.0, lam_S=0.0, lam_M=0.0)

    def bad(match, a=actors, critic=q, o=obs, n=nxt, i=idx, **over):
        with pytest.raises(ValueError, match=match):
            sac_actor_grad_ctde(a, critic, o, n, i, **{"k": 0, **kw, **over})
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
    td3 = ActorParams.from_sac_module(_SacActor(3, 4, 1))
    td3.squash = 0
    bad("MLP_Actor_SAC", a=[actors[0], td3])
    half = ActorParams.from_sac_module(_SacActor(15, 16, 4))
    half.fc2_w = half.fc2_w.double()
    bad("fc2_w", a=[half, actors[1]])
    for name in ("lam_T", "lam_S", "lam_M", "max_action", "alpha"):
        bad(name, **{name: -1.0})
        bad(name, **{name: float("inf")})
    bad("alpha", alpha=torch.zeros(2))
    bad("alpha", alpha=torch.zeros(1, dtype=torch.float64))
    bad("target_entropy", target_entropy=float("nan"))
    bad("alpha_grad", alpha_grad=torch.zeros(2))
    bad("obs_next", n=None)
    bad("obs_next", n=(None, nxt[1]))
    bad(r"obs_next\[0\]", n=(torch.zeros(10, 14), nxt[1]))
    bad(r"obs_next\[0\] must have", n=(torch.zeros(9, 15), nxt[1]))
    bad("noise", noise=None)
    bad("nominal", nominal=None)
    bad("noise", noise=torch.zeros(3))
    bad("nominal", nominal=torch.zeros(1))
    for name in ("eps", "eps_logp", "eps_reg", "eps_next", "eps_pert"):
        bad(name + " must", **{name: torch.zeros(5, 1)})
        bad(name + " must", **{name: torch.zeros(6, 4)})
        bad(name + " must", **{name: e4.double()})
    bad("eps_other must", eps_other=torch.zeros(5, 4))
    bad("grads", grads={})
    bad("stats", stats=torch.zeros(5))
    for args in ((2, 62, 10), (0, 65, 10), (1, 62, 0), (0, 62, 10, -1)):
        with pytest.raises(ValueError, match="QR_E_SIZE"):
            sac_actor_workspace_bytes_ctde(*args)
    assert sac_actor_workspace_bytes_ctde(0, 62, 130) == 3 * NP[0] * 8 and sac_actor_workspace_bytes_ctde(1, 62, 130, 2) == 2 * NP[1] * 8

    mods, critic = [_SacActor(15, 16, 4), _SacActor(3, 4, 1)], _Twin()
    buf = ReplayBuffer(8, (15, 3), (4, 1), "cpu")
    with pytest.raises(ValueError, match="two-agent"):
        sac_actor_loss_ctde(mods, critic, ReplayBuffer(8, (23,), (4,), "cpu"))
    with pytest.raises(ValueError, match="two-agent"):
        sac_actor_loss_ctde(mods, critic, {"obs": obs})
    with pytest.raises(ValueError, match="k must be"):
        sac_actor_loss_ctde(mods, critic, buf, 2)
    with pytest.raises(ValueError, match="pair"):
        sac_actor_loss_ctde(mods[:1], critic, buf)
    with pytest.raises(ValueError, match="log_alpha"):
        sac_actor_loss_ctde(mods, critic, buf, 0, log_alpha=torch.zeros(2, requires_grad=True), **kw)
    with pytest.raises(ValueError, match="noise"):
        sac_actor_loss_ctde(mods, critic, buf, 0, nominal=torch.zeros(4))


def test_torch_op_is_registered():
    import gym_rotor_amd  # noqa: F401
    assert hasattr(torch.ops.gym_rotor_amd, "qr_ctde_sac_actor_grad")
    schema = str(torch.ops.gym_rotor_amd.qr_ctde_sac_actor_grad.default._schema)
    for arg in ("eps_logp", "eps_other", "action_other", "alpha_grad", "alpha_dev"):
        assert arg in schema


@pytest.mark.parametrize("k", (0, 1))
def test_sac_actor_loss_ctde_leaves_the_other_agent_alone(k, monkeypatch):
    """Up to the launch (which needs a GPU): agent k's eight .grad tensors and log_alpha's are made and handed over as they are, the cache
    key is its own, and the other actor — its attributes, its .grad objects (None, or tensors with values) — is what it was."""
    from gym_rotor_amd import ReplayBuffer, sac, sac_actor_loss_ctde
    mods, critic = [_SacActor(15, 16, 4), _SacActor(3, 4, 1)], _Twin()
    buf = ReplayBuffer(8, (15, 3), (4, 1), "cpu")
    other = list(mods[1 - k].parameters())
    other[0].grad = torch.full_like(other[0], 3.5)
    held = [p.grad for p in other]
    before = dict(vars(mods[1 - k]))
    children = dict(mods[1 - k].named_modules())
    seen = {}
    monkeypatch.setattr(sac, "sac_actor_workspace_bytes_ctde", lambda k, H, B, mw=0: 8 * 11)

    def launch(actors, q, obs, obs_next, index, **kw):
        seen.update(kw, actors=actors, obs=obs, obs_next=obs_next)
        return kw["grads"], kw["stats"]
    monkeypatch.setattr(sac, "sac_actor_grad_ctde", launch)
    log_alpha = torch.zeros(1, requires_grad=True)
    e = torch.zeros(5, (4, 1)[k])
    kw = dict(noise=torch.zeros((15, 3)[k]), nominal=torch.zeros((4, 1)[k]), log_alpha=log_alpha, eps_logp=e)
    stats = sac_actor_loss_ctde(mods, critic, buf, k, torch.zeros(5, dtype=torch.int64), **kw)
    m = mods[k]
    own = [t for l in (m.fc1, m.fc2, m.mean_linear, m.log_std_linear) for t in (l.weight, l.bias)]
    assert all(p.grad is not None and p.grad.shape == p.shape for p in own) and log_alpha.grad is not None
    assert [g.data_ptr() for g in seen["grads"].values()] == [p.grad.data_ptr() for p in own] and seen["k"] == k and "action_other" not in seen
    assert seen["alpha_grad"] is log_alpha.grad and seen["eps_logp"] is e and seen["eps_other"] is None
    assert all(a is b for a, b in zip(held, (p.grad for p in other))) and held[1] is None and bool((held[0] == 3.5).all())
    assert vars(mods[1 - k]).keys() == before.keys() and all(vars(mods[1 - k])[n] is v for n, v in before.items())
    assert dict(mods[1 - k].named_modules()).keys() == children.keys()
    assert seen["obs"] is buf.obs and seen["obs_next"] is buf.obs_next and [a.dims for a in seen["actors"]] == [(15, 16, 4), (3, 4, 1)]
    key = ("sac_actor_ctde", k, 5, 0)
    assert key in buf._cache and seen["workspace"].numel() == 11 and stats is buf._cache[key][1] and stats.numel() == 6
    again = sac_actor_loss_ctde(mods, critic, buf, k, torch.zeros(5, dtype=torch.int64), **kw)
    assert again is stats and len(buf._cache) == 1
