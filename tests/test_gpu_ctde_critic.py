"""The centralized-critic (CTDE) half of TD3 and SAC on the device (td3_target_kernel<15, 3> / <0, 0>, sac_target_kernel<15, 3> / <0, 0>,
ctde_twinq_kernel: qr_ctde_twinq_target, qr_ctde_sac_target, qr_ctde_twinq_grad; the Python functions, the live-module forms, the torch
ops) against the reference's float64 modules (tests/golden/ctde_critic.npz) and the float64 restatement of tests/ctde_ref.py.

The bar, per output: err <= max(2e-6 * max(1, |x64|), e32), e32 = the error of eager float32 torch — the reference's own lines — on
the same inputs on this device; no factor on e32.  Every case prints err / bar before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctde_ref  # noqa: E402
from ctde_ref import CASES, SAC_ACTOR, TD3_ACTOR  # noqa: E402
from td3_ref import NAMES  # noqa: E402
from test_ctde_critic_host import GRAD_CASES, _SacActor, _Td3Actor, _Twin  # noqa: E402
from twinq_gpu_util import _cuda, _idx, _np, _q, bar  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
STATS = ("loss", "mse1", "mse2", "mean_y")
PERM = np.random.default_rng(5).permutation(130)
REPEAT = np.random.default_rng(6).integers(0, 130, 97)


@pytest.fixture(scope="module")
def cases():
    g = ctde_ref.load()
    return {n: ctde_ref.case(g, n) for n in CASES}


def _critic(c, prefix="t_"):
    from gym_rotor_amd import QCriticParams
    return QCriticParams(*[_cuda(c[prefix + n]) for n in NAMES], int(c["action_dims"].sum()))


def _actors(c, sac):
    from gym_rotor_amd import ActorParams, _lib
    if "p0_fc1_w" not in c:
        return None
    out = []
    for m in (0, 1):
        if sac:
            w = [_cuda(c[f"s{m}_{n}"]) for n in SAC_ACTOR]
            out.append(ActorParams(*w[:6], None, w[6], w[7], _lib.ACTOR_TANH_SAMPLE))
        else:
            out.append(ActorParams(*[_cuda(c[f"p{m}_{n}"]) for n in TD3_ACTOR], None))
    return out


def _agents(c):
    """Both agents' tensors; rwd and done are the columns of ONE [130, 2] tensor each (element stride 2)."""
    rwd, done = _cuda(c["rwd"]), _cuda(c["done"])
    return [{"obs": _cuda(c[f"obs{m}"]), "act": _cuda(c[f"act{m}"]), "obs_next": _cuda(c[f"obsn{m}"]), "rwd": rwd[:, m], "done": done[:, m]} for m in (0, 1)]


def _draws(c, B, key):
    return [_cuda(c[f"{key}{m}"][:B]) for m in (0, 1)] if f"{key}0" in c else None


def run_td3(c, k, index=None, agents=None, **over):
    from gym_rotor_amd import td3_target_ctde
    B = 130 if index is None else len(index)
    kw = dict(discount=float(c["discount"]), target_noise=float(c["target_noise"]), noise_clip=float(c["noise_clip"]),
              max_action=float(c["max_action"]), noise=_draws(c, B, "eps"))
    if "p0_fc1_w" not in c:
        kw.update(action_next=[_cuda(c[f"an_in{m}"][:B]) for m in (0, 1)])
    kw.update(over)
    y = td3_target_ctde(_actors(c, False), _critic(c), agents or _agents(c), k, _idx(index), **kw)
    torch.cuda.synchronize()
    return y


def run_sac(c, k, index=None, agents=None, elp="own", outputs=True, **over):
    """(y, action_out 0, action_out 1, logp_out) of one sac_target_ctde call."""
    from gym_rotor_amd import sac_target_ctde
    B = 130 if index is None else len(index)
    ad = [int(a) for a in c["action_dims"]]
    if isinstance(elp, str):
        elp = _cuda(c[f"elp{k}"][:B]) if f"elp{k}" in c else None
    kw = dict(discount=float(c["discount"]), alpha=float(c["alpha"]), noise=_draws(c, B, "eps"), noise_logp=elp)
    if "p0_fc1_w" not in c:
        kw.update(action_next=[_cuda(c[f"an_in{m}"][:B]) for m in (0, 1)], logp_next=_cuda(c["logp_in"][:B]), noise_logp=None)
    if outputs:
        kw.update(action_out=[torch.full((B, a), SENTINEL, device="cuda") for a in ad], logp_out=torch.full((B,), SENTINEL, device="cuda"))
    kw.update(over)
    y = sac_target_ctde(_actors(c, True), _critic(c), agents or _agents(c), k, _idx(index), **kw)
    torch.cuda.synchronize()
    ao = kw.get("action_out") or (None, None)
    return y, ao[0], ao[1], kw.get("logp_out")


# ------------------------------------------------------------------------------------------------------------------------
# eager torch on the device, in a given dtype: what e32 is measured with (the reference's CTDE lines)
# ------------------------------------------------------------------------------------------------------------------------
def _twin(c, prefix, dtype):
    m = _Twin(c[prefix + "fc1_w"].shape[1], c[prefix + "fc1_w"].shape[0])
    with torch.no_grad():
        for n in NAMES:
            getattr(getattr(m, n[:3]), "weight" if n.endswith("w") else "bias").copy_(torch.from_numpy(c[prefix + n]))
    return m.to(dtype).cuda()


def _sample(w, x, e):
    h = torch.relu(torch.relu(x @ w[0].T + w[1]) @ w[2].T + w[3])
    mean, log_std = h @ w[4].T + w[5], torch.clamp(h @ w[6].T + w[7], min=-20, max=2)
    std = log_std.exp()
    x_t = mean + std * (e if e is not None else torch.zeros_like(mean))
    a = torch.tanh(x_t)
    logp = torch.distributions.Normal(mean, std).log_prob(x_t)
    logp -= torch.log((1 - a.pow(2)) + 1e-6)
    return a, logp.sum(1, keepdim=True)


def torch_targets(c, k, dtype, index=None, elp="own"):
    """{td3_y, sac_a0, sac_a1, sac_logp, sac_y} as float64 arrays, by eager torch in `dtype` on the device (td3.py:124-154, sac.py:136-153)."""
    idx = np.arange(130) if index is None else np.asarray(index)
    B = len(idx)
    on = [_cuda(c[f"obsn{m}"][idx], dtype) for m in (0, 1)]
    r, d = _cuda(c["rwd"][idx, k], dtype)[:, None], _cuda(c["done"][idx, k], dtype)[:, None]
    eps = [_cuda(c[f"eps{m}"][:B], dtype) for m in (0, 1)] if "eps0" in c else None
    if isinstance(elp, str):
        elp = c[f"elp{k}"][:B] if f"elp{k}" in c else None
    disc = float(c["discount"])
    with torch.no_grad():
        t = _twin(c, "t_", dtype)
        if "p0_fc1_w" in c:
            a = []
            for m in (0, 1):
                w = [_cuda(c[f"p{m}_{n}"], dtype) for n in TD3_ACTOR]
                mean = torch.tanh(torch.relu(torch.relu(on[m] @ w[0].T + w[1]) @ w[2].T + w[3]) @ w[4].T + w[5])
                noise = (eps[m] * float(c["target_noise"])).clamp(-float(c["noise_clip"]), float(c["noise_clip"])) if eps is not None else 0.0
                a.append((mean + noise).clamp(-float(c["max_action"]), float(c["max_action"])))
            ws = [[_cuda(c[f"s{m}_{n}"], dtype) for n in SAC_ACTOR] for m in (0, 1)]
            s = [_sample(ws[m], on[m], None if eps is None else eps[m])[0] for m in (0, 1)]
            own = None if eps is None else eps[k]
            logp = _sample(ws[k], on[k], own if elp is None else _cuda(elp, dtype))[1]
        else:
            a = s = [_cuda(c[f"an_in{m}"][:B], dtype) for m in (0, 1)]
            logp = _cuda(c["logp_in"][:B], dtype)[:, None]
        sa = torch.cat(on + a, 1)
        y = r + disc * (1 - d) * torch.min(_q(t, sa, 0), _q(t, sa, 1))
        sa = torch.cat(on + s, 1)
        ys = r + disc * (1 - d) * (torch.min(_q(t, sa, 0), _q(t, sa, 1)) - float(c["alpha"]) * logp)
    out = {"td3_y": y[:, 0], "sac_a0": s[0], "sac_a1": s[1], "sac_logp": logp[:, 0], "sac_y": ys[:, 0]}
    return {n: _np(v).astype(np.float64) for n, v in out.items()}


def torch_twinq(c, dtype, y, index=None):
    idx = np.arange(130) if index is None else np.asarray(index)
    m = _twin(c, "c_", dtype)
    sa = torch.cat([_cuda(c[n][idx], dtype) for n in ("obs0", "obs1", "act0", "act1")], 1)
    yt = _cuda(np.asarray(y), dtype)[:, None]
    m1, m2 = torch.nn.functional.mse_loss(_q(m, sa, 0), yt), torch.nn.functional.mse_loss(_q(m, sa, 1), yt)
    m.zero_grad()
    (m1 + m2).backward()
    grads = {n: _np(getattr(getattr(m, n[:3]), "weight" if n.endswith("w") else "bias").grad).astype(np.float64) for n in NAMES}
    return grads, np.array([(m1 + m2).item(), m1.item(), m2.item(), yt.mean().item()], dtype=np.float64)


def check(label, what, got, x64, x32):
    x64 = np.asarray(x64, dtype=np.float64)
    got = _np(got).astype(np.float64).reshape(x64.shape)
    assert np.isfinite(got).all(), (label, what)
    err, e32 = float(np.abs(got - x64).max()), float(np.abs(np.asarray(x32).reshape(x64.shape) - x64).max())
    b = bar(x64, e32)
    print(f"ctde {label} {what}: err / bar = {err / b:.3f} (err {err:.3e}, e32 {e32:.3e})")
    return err <= b, (label, what, err, b)


def check_targets(label, c, k, y_td3, sac, index=None, elp="own", want64=None):
    """TD3's y and SAC's (y, a'_0, a'_1, logp) against float64 (the fixture's where the call is the fixture's, ctde_ref's otherwise)."""
    x32 = torch_targets(c, k, torch.float32, index, elp)
    if want64 is None:
        e = None if not isinstance(elp, str) and elp is None else (c.get(f"elp{k}") if isinstance(elp, str) else elp)
        B = 130 if index is None else len(index)
        t = ctde_ref.td3_target_f64(c, k, index)
        s = ctde_ref.sac_target_f64(c, k, index, elp=None if e is None else e[:B])
        want64 = {"td3_y": t[2], "sac_a0": s[0], "sac_a1": s[1], "sac_logp": s[2], "sac_y": s[3]}
    got = {"td3_y": y_td3, "sac_y": sac[0], "sac_a0": sac[1], "sac_a1": sac[2], "sac_logp": sac[3]}
    res = [check(label, n, got[n], want64[n], x32[n]) for n in got if got[n] is not None]
    assert all(ok for ok, _ in res), [info for ok, info in res if not ok]


def run_grad(c, y, index=None, **kw):
    from gym_rotor_amd import twinq_grad_ctde
    t = _agents(c)
    grads, stats = twinq_grad_ctde(_critic(c, "c_"), (t[0]["obs"], t[1]["obs"]), (t[0]["act"], t[1]["act"]), y, _idx(index), **kw)
    torch.cuda.synchronize()
    return grads, stats


def check_grads(label, c, grads, stats, y32, index=None):
    """The twelve gradients and stats against float64 on the float32 y the kernel was given."""
    y64 = _np(y32).astype(np.float64)
    loss, m1, m2, g64 = ctde_ref.twinq_grad_f64(c, y64, index)
    g32, s32 = torch_twinq(c, torch.float32, _np(y32), index)
    res = [check(label, n, grads[n], g64[n].reshape(grads[n].shape), g32[n]) for n in NAMES]
    for j, (n, v) in enumerate(zip(STATS, (loss, m1, m2, float(y64.mean())))):
        res.append(check(label, n, stats[j:j + 1], np.array([v]), s32[j:j + 1]))
    assert all(ok for ok, _ in res), [info for ok, info in res if not ok]


def bits(t):
    return _np(t).view(np.int32) if t.dtype == torch.float32 else _np(t)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------------
# every fixture case against float64
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 1))
@pytest.mark.parametrize("name", CASES)
def test_targets_of_the_fixture_cases_against_the_reference_float64(cases, name, k):
    c = cases[name]
    y = run_td3(c, k)
    sac = run_sac(c, k)
    assert y.shape == (130,) and y.dtype == torch.float32
    want = {"td3_y": c[f"td3_y{k}"], "sac_a0": c["sac_a0"], "sac_a1": c["sac_a1"], "sac_logp": c[f"sac_logp{k}"], "sac_y": c[f"sac_y{k}"]}
    check_targets(f"{name} k={k}", c, k, y, sac, want64=want)


@pytest.mark.parametrize("k", (0, 1))
@pytest.mark.parametrize("name", CASES)
def test_regression_of_the_fixture_cases_against_the_reference_float64(cases, name, k):
    c = cases[name]
    y = _cuda(c[f"td3_y{k}"].astype(np.float32))
    grads, stats = run_grad(c, y)
    check_grads(f"{name} k={k}", c, grads, stats, y)
    if name in GRAD_CASES:   # the reference's own autograd, on its float64 y: the float32 rounding of y is inside the bar's 2e-6
        g32, _ = torch_twinq(c, torch.float32, c[f"td3_y{k}"])
        res = [check(f"{name} k={k} vs autograd", n, grads[n], c[f"g{k}_{n}"], g32[n]) for n in NAMES]
        assert all(ok for ok, _ in res), [info for ok, info in res if not ok]


# ------------------------------------------------------------------------------------------------------------------------
# index forms, tile edges, done rows, untouched memory
# ------------------------------------------------------------------------------------------------------------------------
def test_index_forms(cases):
    c = cases["ctde"]
    k = 1
    y0, s0 = run_td3(c, k), run_sac(c, k)
    ident = np.arange(130)
    assert same(y0, run_td3(c, k, ident)) and all(same(a, b) for a, b in zip(s0, run_sac(c, k, ident)))
    g0, st0 = run_grad(c, y0)
    g1, st1 = run_grad(c, y0, ident)
    assert same(st0, st1) and all(same(g0[n], g1[n]) for n in NAMES)
    for label, index in (("permuted", PERM), ("repeated", REPEAT)):
        y, sac = run_td3(c, k, index), run_sac(c, k, index)
        check_targets(label, c, k, y, sac, index)
        grads, stats = run_grad(c, y, index)
        check_grads(label, c, grads, stats, y, index)
    wild = PERM.copy()
    wild[::7], wild[3::11] = -5 - wild[::7], 130 + 9 * wild[3::11]
    clamped = np.clip(wild, 0, 129)
    assert (wild != clamped).sum() >= 20
    assert same(run_td3(c, k, wild), run_td3(c, k, clamped)) and all(same(a, b) for a, b in zip(run_sac(c, k, wild), run_sac(c, k, clamped)))
    ga, sa = run_grad(c, y0, wild)
    gb, sb = run_grad(c, y0, clamped)
    assert same(sa, sb) and all(same(ga[n], gb[n]) for n in NAMES)


def _guarded(shape):
    """A sentinel-filled buffer with 8 guard rows before and behind the view that is handed out."""
    buf = torch.full((shape[0] + 16,) + tuple(shape[1:]), SENTINEL, device="cuda")
    return buf, buf[8:8 + shape[0]]


@pytest.mark.parametrize("B", (1, 63, 64, 65, 130))
@pytest.mark.parametrize("name", ("ctde", "w28"))
def test_tile_edges_into_guarded_outputs(cases, name, B):
    c = cases[name]
    k = B % 2
    index = PERM[:B]
    ad = [int(a) for a in c["action_dims"]]
    (yb, y), (sb, ys), (a0b, a0), (a1b, a1), (lb, lp) = _guarded((B,)), _guarded((B,)), _guarded((B, ad[0])), _guarded((B, ad[1])), _guarded((B,))
    agents = _agents(c)
    before = [t.clone() for a in agents for t in a.values()]
    run_td3(c, k, index, agents, out=y)
    sac = run_sac(c, k, index, agents, out=ys, action_out=[a0, a1], logp_out=lp)
    for buf, view in ((yb, y), (sb, ys), (a0b, a0), (a1b, a1), (lb, lp)):
        assert (buf[:8] == SENTINEL).all() and (buf[8 + B:] == SENTINEL).all() and not (view == SENTINEL).any()   # fully written, nothing else
    assert all(torch.equal(t, b) for t, b in zip((t for a in agents for t in a.values()), before))
    check_targets(f"{name} B={B}", c, k, y, sac, index)
    grads, stats = run_grad(c, y, index)
    check_grads(f"{name} B={B}", c, grads, stats, y, index)


@pytest.mark.parametrize("name", ("sat", "ctde"))
def test_target_of_done_rows_is_the_reward_exactly(cases, name):
    c = cases[name]
    for k in (0, 1):
        done = c["done"][:, k] == 1.0
        assert done.sum() >= 5
        for y in (run_td3(c, k), run_sac(c, k)[0]):
            assert np.array_equal(_np(y)[done].view(np.int32), c["rwd"][done, k].view(np.int32))
            assert not np.array_equal(_np(y)[~done], c["rwd"][~done, k])


# ------------------------------------------------------------------------------------------------------------------------
# the four-source gather is the new code, the arithmetic is not: bit for bit against the one-agent kernels on concatenated rows
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ctde", "h64", "h5", "w28"))
def test_gradients_equal_twinq_grad_on_concatenated_rows_bit_for_bit(cases, name):
    from gym_rotor_amd import twinq_grad
    c = cases[name]
    t = _agents(c)
    obs, act = torch.cat([t[0]["obs"], t[1]["obs"]], 1).contiguous(), torch.cat([t[0]["act"], t[1]["act"]], 1).contiguous()
    y = _cuda(c["td3_y0"].astype(np.float32))
    for index, mw in ((None, 0), (REPEAT, 0), (PERM, 2), (None, 1)):
        B = 130 if index is None else len(index)
        ga, sa = run_grad(c, y[:B], index, max_workgroups=mw)
        gb, sb = twinq_grad(_critic(c, "c_"), obs, act, y[:B], _idx(index), max_workgroups=mw)
        torch.cuda.synchronize()
        assert same(sa, sb) and all(same(ga[n], gb[n]) for n in NAMES), (name, mw)


@pytest.mark.parametrize("name", ("ctde", "w28"))
def test_actorless_targets_equal_the_one_agent_kernels_bit_for_bit(cases, name):
    from gym_rotor_amd import sac_target, td3_target
    c = cases[name]
    t = _agents(c)
    for k, index in ((0, None), (1, REPEAT)):
        B = 130 if index is None else len(index)
        an = [_cuda(c[f"sac_a{m}"][:B].astype(np.float32)) for m in (0, 1)]
        lp = _cuda(c[f"sac_logp{k}"][:B].astype(np.float32))
        one = {"obs_next": torch.cat([t[0]["obs_next"], t[1]["obs_next"]], 1).contiguous(), "rwd": t[k]["rwd"], "done": t[k]["done"]}
        cat = torch.cat(an, 1).contiguous()
        kw = dict(discount=float(c["discount"]))
        from gym_rotor_amd import sac_target_ctde, td3_target_ctde
        ya = td3_target_ctde(None, _critic(c), t, k, _idx(index), action_next=an, **kw)
        yb = td3_target(None, _critic(c), one, 0, _idx(index), action_next=cat, **kw)
        ao = [torch.full_like(a, SENTINEL) for a in an]
        lo, lo1, ao1 = torch.full_like(lp, SENTINEL), torch.full_like(lp, SENTINEL), torch.full_like(cat, SENTINEL)
        sa = sac_target_ctde(None, _critic(c), t, k, _idx(index), action_next=an, logp_next=lp, alpha=0.2, action_out=ao, logp_out=lo, **kw)
        sb = sac_target(None, _critic(c), one, 0, _idx(index), action_next=cat, logp_next=lp, alpha=0.2, action_out=ao1, logp_out=lo1, **kw)
        torch.cuda.synchronize()
        assert same(ya, yb) and same(sa, sb) and same(torch.cat(ao, 1), ao1) and same(lo, lo1) and same(lo, lp), (name, k)


def test_same_inputs_and_grid_give_the_same_bits(cases):
    c = cases["ctde"]
    y = run_td3(c, 0)
    assert same(y, run_td3(c, 0)) and all(same(a, b) for a, b in zip(run_sac(c, 1), run_sac(c, 1)))
    for mw in (0, 1, 2):
        ga, sa = run_grad(c, y, max_workgroups=mw)
        gb, sb = run_grad(c, y, max_workgroups=mw)
        assert same(sa, sb) and all(same(ga[n], gb[n]) for n in NAMES)
    grads, stats = run_grad(c, y, max_workgroups=1)   # another grid: another order of the sums, inside the bar
    check_grads("max_workgroups=1", c, grads, stats, y)


def test_the_draw_of_the_log_probability(cases):
    c = cases["twodraw"]
    for k in (0, 1):
        eps_k = _cuda(c[f"eps{k}"])
        one = run_sac(c, k, elp=None)
        assert all(same(a, b) for a, b in zip(one, run_sac(c, k, elp=eps_k)))            # the same tensor: the bits of None
        noise = _draws(c, 130, "eps")
        assert all(same(a, b) for a, b in zip(one, run_sac(c, k, elp=noise[k], noise=noise)))   # the very tensor object passed as noise[k]
        two = run_sac(c, k)
        assert same(one[1], two[1]) and same(one[2], two[2])                               # a' does not depend on it
        assert not same(one[3], two[3]) and not same(one[0], two[0])                       # logp and y do
        check_targets(f"onedraw k={k}", c, k, None, one, elp=None)
    nz = cases["noeps"]
    zeros = [torch.zeros(130, a, device="cuda") for a in (4, 1)]
    assert all(same(a, b) for a, b in zip(run_sac(nz, 0), run_sac(nz, 0, noise=zeros)))     # NULL draws are zeros
    assert same(run_td3(nz, 1), run_td3(nz, 1, noise=zeros))


def test_outputs_on_or_off_and_alpha_on_the_device(cases):
    c = cases["ctde"]
    full = run_sac(c, 1)
    assert same(full[0], run_sac(c, 1, outputs=False)[0])
    assert same(full[0], run_sac(c, 1, alpha=torch.tensor([float(c["alpha"])], device="cuda"))[0])


# ------------------------------------------------------------------------------------------------------------------------
# live modules
# ------------------------------------------------------------------------------------------------------------------------
def _modules(c, sac):
    crit, targ = _twin(c, "c_", torch.float32), _twin(c, "t_", torch.float32)
    actors = []
    for m, dims in enumerate(((15, 16, 4), (3, 4, 1))):
        a = (_SacActor if sac else _Td3Actor)(*dims)
        layers = (a.fc1, a.fc2, a.mean_linear, a.log_std_linear) if sac else (a.fc1, a.fc2, a.fc3)
        names = SAC_ACTOR if sac else TD3_ACTOR
        with torch.no_grad():
            for j, l in enumerate(layers):
                l.weight.copy_(torch.from_numpy(c[f"{'s' if sac else 'p'}{m}_{names[2 * j]}"]))
                l.bias.copy_(torch.from_numpy(c[f"{'s' if sac else 'p'}{m}_{names[2 * j + 1]}"]))
        actors.append(a.cuda())
    return crit, targ, actors


def _buffer(c):
    from gym_rotor_amd import ReplayBuffer
    buf = ReplayBuffer(130, (15, 3), (4, 1), "cuda")
    for m in (0, 1):
        buf.obs[m].copy_(_cuda(c[f"obs{m}"])), buf.obs_next[m].copy_(_cuda(c[f"obsn{m}"])), buf.act[m].copy_(_cuda(c[f"act{m}"]))
        buf.rwd[m].copy_(_cuda(c["rwd"][:, m])), buf.done[m].copy_(_cuda(c["done"][:, m]))
    buf.count, buf.current_size = 0, 130
    return buf


@pytest.mark.parametrize("sac", (False, True))
def test_critic_loss_on_live_modules(cases, sac):
    from gym_rotor_amd import sac_critic_loss_ctde, td3_critic_loss_ctde
    c = cases["ctde"]
    k = 1
    crit, targ, actors = _modules(c, sac)
    buf = _buffer(c)
    index = _idx(REPEAT)
    noise = [_cuda(c[f"eps{m}"][:97]) for m in (0, 1)]
    elp = _cuda(c["elp1"][:97])

    def call():
        if sac:
            return sac_critic_loss_ctde(crit, targ, actors, buf, k, index, discount=float(c["discount"]), alpha=float(c["alpha"]), noise=noise, noise_logp=elp)
        return td3_critic_loss_ctde(crit, targ, actors, buf, k, index, noise=noise)

    stats = call()
    torch.cuda.synchronize()
    key = ("sac_ctde" if sac else "td3_ctde", k, 97, 0)
    y = buf._cache[key][0]
    y64 = (ctde_ref.sac_target_f64(c, k, REPEAT)[3] if sac else ctde_ref.td3_target_f64(c, k, REPEAT)[2])
    y32 = torch_targets(c, k, torch.float32, REPEAT)["sac_y" if sac else "td3_y"]
    ok, info = check("live", "y", y, y64, y32)
    assert ok, info
    grads = {n: getattr(getattr(crit, n[:3]), "weight" if n.endswith("w") else "bias").grad for n in NAMES}
    check_grads(f"live {'sac' if sac else 'td3'}", c, grads, stats, y, REPEAT)
    # the second call with an unchanged B allocates nothing
    ptrs = [g.data_ptr() for g in grads.values()]
    before = torch.cuda.memory_allocated()
    stats2 = call()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and stats2.data_ptr() == stats.data_ptr()
    assert ptrs == [getattr(getattr(crit, n[:3]), "weight" if n.endswith("w") else "bias").grad.data_ptr() for n in NAMES]
    # an optimiser step on the critic is seen by the next call without any copy
    g_before = {n: g.clone() for n, g in grads.items()}
    opt = torch.optim.AdamW(crit.parameters(), lr=1e-2)
    opt.step()
    call()
    torch.cuda.synchronize()
    assert not same(grads["fc1_w"], g_before["fc1_w"])
    c2 = dict(c)
    for n in NAMES:
        c2["c_" + n] = _np(getattr(getattr(crit, n[:3]), "weight" if n.endswith("w") else "bias").data)
    check_grads("live after AdamW", c2, grads, buf._cache[key][2], y, REPEAT)


def test_torch_ops_give_the_bits_of_the_python_functions(cases):
    ops = torch.ops.gym_rotor_amd
    c = cases["ctde"]
    k = 1
    t = _agents(c)
    index = _idx(PERM)
    noise = _draws(c, 130, "eps")
    elp = _cuda(c["elp1"])
    wt = [_cuda(c["t_" + n]) for n in NAMES]
    y = run_td3(c, k, PERM)
    y_op = torch.full_like(y, SENTINEL)
    pa = [_cuda(c[f"p{m}_{n}"]) for m in (0, 1) for n in TD3_ACTOR]
    ops.qr_ctde_twinq_target(pa, wt, t[0]["obs_next"], t[1]["obs_next"], t[0]["act"], t[1]["act"], t[k]["rwd"], t[k]["done"], index, noise[0], noise[1],
                             None, None, y_op, float(c["discount"]), float(c["target_noise"]), float(c["noise_clip"]), float(c["max_action"]))
    sac = run_sac(c, k, PERM)
    s_op = [torch.full_like(x, SENTINEL) for x in sac]
    sa = [_cuda(c[f"s{m}_{n}"]) for m in (0, 1) for n in SAC_ACTOR]
    ops.qr_ctde_sac_target(sa, wt, k, t[0]["obs_next"], t[1]["obs_next"], t[0]["act"], t[1]["act"], t[k]["rwd"], t[k]["done"], index, noise[0], noise[1], elp,
                           None, None, None, s_op[0], s_op[1], s_op[2], s_op[3], float(c["discount"]), float(c["alpha"]))
    grads, stats = run_grad(c, y, PERM)
    wc = [_cuda(c["c_" + n]) for n in NAMES]
    g_op, st_op = [torch.full_like(w, SENTINEL) for w in wc], torch.full((4,), SENTINEL, device="cuda")
    ops.qr_ctde_twinq_grad(wc, t[0]["obs"], t[1]["obs"], t[0]["act"], t[1]["act"], y, index, g_op, st_op)
    torch.cuda.synchronize()
    assert same(y, y_op) and all(same(a, b) for a, b in zip(sac, s_op))
    assert same(stats, st_op) and all(same(grads[n], g) for n, g in zip(NAMES, g_op))
