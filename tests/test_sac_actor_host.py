"""SAC's actor half without a GPU: the float64 restatement (tests/sac_actor_ref.py) against the fixture's autograd gradients and stats
(tests/golden/sac_actor.npz, tools/gen_golden_sac_actor.py), the margins and shares the seeds were searched for, the struct mirror, every
error code of qr_sac_actor_grad with a NULL stream (nothing is launched on an error), every ValueError of sac_actor_grad, the
workspace-bytes entry, the op's registration and sac_actor_loss's cache key.

The bound between the two float64 sides.  The generator must use torch.tanh (autograd), the restatement uses tanh64 (long double,
rounded once); log(1 - a^2 + 1e-6) turns one ulp of a into 2e-10 on a saturated component.  Where no component is
saturated the bound is 1e-12 * max(1, |x|).  For `clamp` and `sat` it is four times the worst difference measured when the fixture was
made (the factor allows for libm differences between machines), MEASURED below, which stays under 1e-8 * max(1, |x|): it cannot hide a
float32 error."""
import ctypes as C

import numpy as np
import pytest

import sac_actor_ref as R

G = R.load()
MEASURED = {"clamp": 4.341e-10, "sat": 2.454e-12}   # worst |restatement - autograd| / max(1, |x|) over gradients and stats


def _bound(name):
    b = 4.0 * MEASURED[name] if name in R.SATURATED else 1e-12
    assert b < 1e-8
    return b


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_matches_autograd(name):
    c = R.case(G, name)
    w, q, obs, obs_next, eps, kw = R.inputs(c)
    stats, grads, alpha_grad = R.sac_actor_grad_f64(w, q, obs, obs_next, eps, **kw)
    worst = 0.0
    for n in R.ACTOR_NAMES:
        ref = c["g_" + n]
        worst = max(worst, np.abs(grads[n] - ref).max() / max(1.0, np.abs(ref).max()))
    for k in range(4):
        worst = max(worst, abs(stats[k] - c["stats"][k]) / max(1.0, abs(c["stats"][k])))
    worst = max(worst, abs(alpha_grad - float(c["alpha_grad"])) / max(1.0, abs(float(c["alpha_grad"]))))
    print(f"{name}: worst |restatement - autograd| / max(1, |x|) = {worst:.3e}")
    assert worst <= _bound(name)
    assert stats[4] == c["stats"][4] and stats[5] == c["stats"][5]   # exact counts divided once


@pytest.mark.parametrize("name", R.CASES)
def test_margins_and_shares(name):
    c = R.case(G, name)
    w, q, obs, obs_next, eps, kw = R.inputs(c)
    m = R.margins(w, q, obs, obs_next, eps, **kw)
    assert all(v >= R.MARGIN for v in m.values()), m
    np.testing.assert_array_equal(np.array([m["relu"], m["ls"], m["clamp"], m["q"]]), c["margins"])
    assert len(obs) == R.ROWS == 130
    assert 0.0 < c["stats"][5] < 1.0                     # rows on both sides of the min
    assert ("eps" in c) == (name != "noeps")
    if name == "noreg":
        assert c["lam"] == (0.0, 0.0, 0.0) and c["stats"][3] == 0.0
    if name == "alpha0":
        assert c["alpha"] == 0.0
    if name == "clamp":
        stats, _, _, passes, _ = R.sac_actor_grad_f64(w, q, obs, obs_next, eps, detail=True, **kw)
        assert (passes[0]["lsr"] < -20).any() and (passes[0]["lsr"] > 2).any() and 0.1 <= stats[4] <= 0.9
    else:
        assert c["stats"][4] == 0.0 or name == "sat"
    if name == "sat":
        _, _, _, passes, _ = R.sac_actor_grad_f64(w, q, obs, obs_next, eps, detail=True, **kw)
        assert c["max_action"] == 0.5 and any((np.abs(p["a"]) > 0.5).any() for p in passes[1:]) and max(np.abs(p["u"]).max() for p in passes) >= 4.0
    # the critics are independent networks, not one scaled
    assert not np.allclose(c["c_fc1_w"] / np.abs(c["c_fc1_w"]).max(), c["c_fc4_w"] / np.abs(c["c_fc4_w"]).max())


def test_fixture_holds_arrays_only_and_is_small():
    import os
    assert os.path.getsize(R.GOLDEN) <= 1_000_000
    assert [str(n) for n in G["cases"]] == list(R.CASES)
    assert all(G[k].dtype != object for k in G.files)


def test_struct_mirror():
    from gym_rotor_amd import _lib
    S = _lib.QrSacActorGrad
    names = [n for n, _ in S._fields_]
    assert names == list(_lib.SAC_ACTOR_GRAD_NAMES) + ["stats", "eps", "eps_reg", "eps_next", "eps_pert", "noise", "nominal", "alpha_dev", "alpha_grad",
                                                       "workspace", "workspace_bytes", "alpha", "target_entropy", "lam_T", "lam_S", "lam_M",
                                                       "max_action", "max_workgroups", "reserved0"]
    assert _lib.SAC_ACTOR_GRAD_NAMES == R.ACTOR_NAMES
    assert C.sizeof(S) == 18 * 8 + 8 + 6 * 4 + 2 * 4 and S.workspace_bytes.offset == 18 * 8 and S.alpha.offset == 19 * 8
    assert "qr_sac_actor_grad" in _lib.SYMBOLS and "qr_sac_actor_workspace_bytes" in _lib.SYMBOLS


def _structs():
    """Valid arguments over host memory (the checks never dereference), kept alive by the returned list."""
    from gym_rotor_amd import _lib
    keep = [np.zeros(4096, dtype=np.float64) for _ in range(4)]
    addr = keep[0].ctypes.data
    p = _lib.QrActor()
    for n in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std_w", "log_std_b"):
        setattr(p, n, addr)
    p.obs_dim, p.hidden_dim, p.action_dim, p.squash = 23, 16, 4, _lib.ACTOR_TANH_SAMPLE
    q = _lib.QrQCritic()
    for n in _lib.TWINQ_GRAD_NAMES:
        setattr(q, n, addr)
    q.obs_dim, q.action_dim, q.hidden_dim, q.reserved0 = 23, 4, 62, 0
    b = _lib.QrTransitions()
    b.obs = b.obs_next = addr
    b.batch, b.rows, b.row_stride, b.reward_stride, b.done_stride = 130, 130, 1, 1, 1
    g = _lib.QrSacActorGrad()
    for n in _lib.SAC_ACTOR_GRAD_NAMES + ("stats", "noise", "nominal", "workspace"):
        setattr(g, n, addr)
    g.workspace_bytes = 1 << 20
    g.alpha, g.target_entropy, g.lam_T, g.lam_S, g.lam_M, g.max_action = 0.2, -4.0, 0.4, 0.3, 0.6, 1.0
    return p, q, b, g, keep


def _call(p, q, b, g):
    from gym_rotor_amd import _lib
    ref = lambda s: None if s is None else C.byref(s)
    return _lib.load().qr_sac_actor_grad(ref(p), ref(q), ref(b), ref(g), None)


E_NULL, E_KIND, E_SIZE, E_ALIGN = -1, -2, -3, -4


def test_error_codes():
    from gym_rotor_amd import _lib
    for k in range(4):
        s = list(_structs()[:4])
        s[k] = None
        assert _call(*s) == E_NULL
    cases = []

    def bad(code, **edits):
        cases.append((code, edits))

    bad(E_KIND, p_squash=_lib.ACTOR_TANH_MEAN)
    bad(E_KIND, p_log_std_w=None)
    bad(E_KIND, p_log_std_b=None)
    bad(E_SIZE, p_hidden_dim=8)
    bad(E_SIZE, q_hidden_dim=65)
    bad(E_SIZE, q_hidden_dim=0)
    bad(E_SIZE, q_obs_dim=15)
    bad(E_SIZE, q_action_dim=3)
    bad(E_SIZE, q_reserved0=1)
    bad(E_SIZE, g_reserved0=1)
    bad(E_SIZE, b_batch=0)
    bad(E_SIZE, b_rows=0)
    bad(E_SIZE, g_max_workgroups=-1)
    for f in ("alpha", "lam_T", "lam_S", "lam_M", "max_action"):
        bad(E_SIZE, **{"g_" + f: -0.5})
        bad(E_SIZE, **{"g_" + f: float("inf")})
        bad(E_SIZE, **{"g_" + f: float("nan")})
    bad(E_SIZE, g_target_entropy=float("inf"))
    bad(E_SIZE, g_target_entropy=float("nan"))
    bad(E_SIZE, g_workspace_bytes=8)
    for n in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b"):
        bad(E_NULL, **{"p_" + n: None})
    for n in _lib.TWINQ_GRAD_NAMES:
        bad(E_NULL, **{"q_" + n: None})
    for n in _lib.SAC_ACTOR_GRAD_NAMES + ("stats", "workspace", "noise", "nominal"):
        bad(E_NULL, **{"g_" + n: None})
    bad(E_NULL, b_obs=None)
    bad(E_NULL, b_obs_next=None)
    for code, edits in cases:
        p, q, b, g, keep = _structs()
        for k, v in edits.items():
            setattr({"p": p, "q": q, "b": b, "g": g}[k[0]], k[2:], v)
        assert _call(p, q, b, g) == code, edits
    # alignment: float pointers 4 bytes, index and workspace 8
    for owner, n, off in (("p", "fc2_w", 2), ("q", "fc5_b", 1), ("g", "mean_b", 2), ("g", "eps", 2), ("g", "eps_pert", 1), ("g", "alpha_dev", 2),
                          ("g", "alpha_grad", 2), ("b", "obs", 2), ("b", "index", 4), ("g", "workspace", 4)):
        p, q, b, g, keep = _structs()
        setattr({"p": p, "q": q, "b": b, "g": g}[owner], n, keep[1].ctypes.data + off)
        assert _call(p, q, b, g) == E_ALIGN, (owner, n)


def test_workspace_bytes_entry():
    from gym_rotor_amd import _lib
    f = _lib.load().qr_sac_actor_workspace_bytes
    np1 = 16 * 23 + 16 + 256 + 16 + 64 + 4 + 64 + 4 + 7
    assert f(23, 16, 4, 62, 130, 0) == 3 * np1 * 8 and f(23, 16, 4, 62, 130, 2) == 2 * np1 * 8
    assert f(23, 16, 4, 62, 1 << 22, 0) == 1024 * np1 * 8
    assert f(3, 4, 1, 5, 64, 0) == (12 + 4 + 16 + 4 + 4 + 1 + 4 + 1 + 7) * 8
    for bad in ((23, 16, 3, 62, 130, 0), (23, 16, 4, 0, 130, 0), (23, 16, 4, 65, 130, 0), (23, 16, 4, 62, 0, 0), (23, 16, 4, 62, 130, -1)):
        assert f(*bad) == E_SIZE


def test_value_errors():
    import torch
    from gym_rotor_amd import ActorParams, QCriticParams, _lib, sac_actor_grad
    c = R.case(G, "mono")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    w = [t(c["a_" + n]) for n in R.ACTOR_NAMES]
    actor = ActorParams(*w[:6], None, w[6], w[7], _lib.ACTOR_TANH_SAMPLE)
    critic = QCriticParams(*[t(c["c_" + n]) for n in R.CRITIC_NAMES], action_dim=4)
    obs, obs_next = t(c["obs"]), t(c["obs_next"])
    ok = dict(noise=t(c["noise"].astype(np.float32)), nominal=t(c["nominal"].astype(np.float32)))
    call = lambda a=actor, o=obs, on=obs_next, i=None, **kw: sac_actor_grad(a, critic, o, on, i, **{**ok, **kw})
    with pytest.raises(ValueError, match="MLP_Actor_SAC"):
        call(ActorParams(*w[:6], torch.zeros(4)))
    for name in ("lam_T", "lam_S", "lam_M", "max_action", "alpha"):
        with pytest.raises(ValueError, match=name):
            call(**{name: -1.0})
    with pytest.raises(ValueError, match="alpha"):
        call(alpha=torch.zeros(2))
    with pytest.raises(ValueError, match="target_entropy"):
        call(target_entropy=float("nan"))
    with pytest.raises(ValueError, match="alpha_grad"):
        call(alpha_grad=torch.zeros(2))
    with pytest.raises(ValueError, match="obs"):
        call(o=obs[:, :5])
    with pytest.raises(ValueError, match="obs_next"):
        call(on=obs_next[:7])
    with pytest.raises(ValueError, match="noise"):
        call(noise=None)
    with pytest.raises(ValueError, match="nominal"):
        call(nominal=torch.zeros(3))
    with pytest.raises(ValueError, match="index"):
        call(i=torch.zeros(4, dtype=torch.int32))
    for name in R.EPS:
        with pytest.raises(ValueError, match=name):
            call(**{name: torch.zeros(129, 4)})
    with pytest.raises(ValueError, match="stats"):
        call(stats=torch.zeros(4))
    with pytest.raises(ValueError, match="grads"):
        call(grads={})
    with pytest.raises(RuntimeError, match="GPU only"):
        call()


def test_op_registered():
    import torch
    import gym_rotor_amd  # noqa: F401
    op = torch.ops.gym_rotor_amd.qr_sac_actor_grad
    schema = str(op.default._schema)
    assert "Tensor(a" in schema and "alpha_grad" in schema and "max_workgroups" in schema


def test_sac_actor_loss_cache_key(monkeypatch):
    """sac_actor_loss caches (workspace, stats) on the buffer under ("sac_actor", k, B, max_workgroups) and hands them on."""
    import torch
    from gym_rotor_amd import ReplayBuffer, sac as S

    class L:
        def __init__(self, o, i):
            self.weight, self.bias = torch.nn.Parameter(torch.zeros(o, i)), torch.nn.Parameter(torch.zeros(o))

    class M:
        pass

    actor, critic = M(), M()
    actor.fc1, actor.fc2, actor.mean_linear, actor.log_std_linear = L(16, 23), L(16, 16), L(4, 16), L(4, 16)
    for k, (i, o) in enumerate(((27, 62), (62, 62), (62, 1)) * 2, 1):
        setattr(critic, f"fc{k}", L(o, i))
    buf = ReplayBuffer(256, [23], [4], torch.device("cpu"))
    seen = []
    monkeypatch.setattr(S, "sac_actor_grad", lambda *a, **kw: seen.append(kw) or (kw["grads"], kw["stats"]))
    index = torch.arange(130)
    log_alpha = torch.nn.Parameter(torch.zeros(1))
    s1 = S.sac_actor_loss(actor, critic, buf, 0, index, log_alpha=log_alpha, max_workgroups=2)
    s2 = S.sac_actor_loss(actor, critic, buf, 0, index, log_alpha=log_alpha, max_workgroups=2)
    key = ("sac_actor", 0, 130, 2)
    assert key in buf._cache and s1 is s2 is buf._cache[key][1] and s1.numel() == 6
    assert seen[0]["workspace"] is seen[1]["workspace"] is buf._cache[key][0]
    assert buf._cache[key][0].numel() * 8 == S.sac_actor_workspace_bytes((23, 16, 4), 62, 130, 2)
    assert seen[0]["alpha_grad"] is log_alpha.grad and set(seen[0]["grads"]) == set(R.ACTOR_NAMES)
    assert seen[0]["grads"]["log_std_w"] is actor.log_std_linear.weight.grad


def test_sac_actor_loss_value_errors():
    """The two checks sac_actor_loss makes itself, before anything reaches the device."""
    import torch
    from gym_rotor_amd import ReplayBuffer, sac_actor_loss

    class L:
        def __init__(self, o, i):
            self.weight, self.bias = torch.nn.Parameter(torch.zeros(o, i)), torch.nn.Parameter(torch.zeros(o))

    class M:
        pass

    actor, critic = M(), M()
    actor.fc1, actor.fc2, actor.mean_linear, actor.log_std_linear = L(16, 23), L(16, 16), L(4, 16), L(4, 16)
    with pytest.raises(ValueError, match="ReplayBuffer"):
        sac_actor_loss(actor, critic, {"obs": torch.zeros(4, 23)})
    buf = ReplayBuffer(8, [23], [4], torch.device("cpu"))
    with pytest.raises(ValueError, match="log_alpha"):
        sac_actor_loss(actor, critic, buf, log_alpha=torch.nn.Parameter(torch.zeros(2)))
