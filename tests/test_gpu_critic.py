"""The PPO critic on the device (critic_kernel: qr_critic_values, qr_critic_next_values; RolloutStorage.compute_values) against the
reference's critic modules (tests/golden/critic_values.npz: their float64 outputs), the float64 restatement of
tests/test_critic_host.py, and the torch-module path it replaces (RolloutStorage.next_values).

The bar everywhere is the project's bar for float32 rows against float64, 2e-6 * max(1, ||V||_inf); each test
prints the worst figure it saw before it asserts (pytest -s)."""
import numpy as np
import pytest
import torch

from test_critic_host import CASES, _Critic, bar, case_weights, critic_f64
from test_critic_host import fixture  # noqa: F401  (the module-scoped fixture file)

pytestmark = pytest.mark.gpu
INPUTS = {"dtde1": (1,), "ctde": (0, 1)}      # every other case reads agent 0's rows
SPLIT = {"ctde": (15, 3)}


def _np(t):
    return t.detach().cpu().numpy()


def _params(w, inputs=(0,)):
    from gym_rotor_amd import CriticParams
    return CriticParams(*[torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in w], inputs)


def _rows(name, x):
    """The per-agent row tensors of a case: its input rows as the obs0 / obs1 the critic's `inputs` select."""
    x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if name in SPLIT:
        a, b = torch.split(x, SPLIT[name], dim=1)
        return [a.contiguous(), b.contiguous()]
    return [None, x] if INPUTS.get(name) == (1,) else [x]


def _values(name, g, rows=slice(None), stride=1, guard=0, sentinel=-7.25):
    """qr_critic_values on rows `rows` of a fixture case into a [n + guard, stride] buffer of sentinels: (column 0 of the first n
    rows, the whole buffer)."""
    from gym_rotor_amd.policy import critic_values
    x = g[f"{name}_x"][rows]
    n = x.shape[0]
    buf = torch.full((n + guard, stride), sentinel, dtype=torch.float32, device="cuda")
    critic_values(_params(case_weights(g, name), INPUTS.get(name, (0,))), _rows(name, x), buf[:n, 0])
    torch.cuda.synchronize()
    return buf[:n, 0].clone(), buf


@pytest.mark.parametrize("name", CASES)
def test_values_match_the_reference_float64(fixture, name):  # noqa: F811
    v, _ = _values(name, fixture)
    v64 = fixture[f"{name}_v64"]
    err = float(np.abs(_np(v).astype(np.float64) - v64).max())
    print(f"critic {name}: max|V - V64| = {err:.3e}  (||V|| = {np.abs(v64).max():.3f}, bar {bar(v64):.3e})")
    assert np.isfinite(_np(v)).all()
    assert err <= bar(v64)


@pytest.mark.parametrize("name", ["mono", "ctde"])
def test_row_count_edges_and_guards(fixture, name):  # noqa: F811
    """n_rows around the 64-row tile, into column 0 of a [n + 70, 2] buffer: column 1 and the 70 rows behind keep their sentinel."""
    full, _ = _values(name, fixture)
    v64 = fixture[f"{name}_v64"]
    for n in (1, 63, 64, 65, 130, 0):
        v, buf = _values(name, fixture, rows=slice(0, n), stride=2, guard=70)
        assert v.shape == (n,)
        assert (buf[:, 1] == -7.25).all() and (buf[n:] == -7.25).all(), n
        if n:
            assert np.abs(_np(v).astype(np.float64) - v64[:n]).max() <= bar(v64), n
            assert torch.equal(v, full[:n]), n     # the same rows at the same tile positions: the same bits


@pytest.mark.parametrize("name", ["mono", "dtde1", "ctde", "sat"])
def test_position_independence_and_determinism(fixture, name):  # noqa: F811
    full, _ = _values(name, fixture)
    again, _ = _values(name, fixture)
    tail, _ = _values(name, fixture, rows=slice(64, 130))
    assert torch.equal(full, again)
    assert torch.equal(tail, full[64:130])


# ------------------------------------------------------------------------------------------------------------------------------
# next values: a hand-built storage
# ------------------------------------------------------------------------------------------------------------------------------
def _modules(kind, scheme, seed):
    """(torch modules on the GPU, their CriticParams, critic(rows) -> [n, n_agents] for RolloutStorage.next_values)."""
    from gym_rotor_amd import CriticParams
    torch.manual_seed(seed)
    if kind == "coupled":
        mods, inputs = [_Critic(23, 62)], [(0,)]
    elif scheme == "dtde":
        mods, inputs = [_Critic(15, 62), _Critic(3, 62)], [(0,), (1,)]
    else:
        mods, inputs = [_Critic(18, 62), _Critic(18, 62)], [(0, 1), (0, 1)]
    mods = [m.cuda() for m in mods]
    params = [CriticParams.from_module(m, i) for m, i in zip(mods, inputs)]

    def critic(rows):
        with torch.no_grad():
            return torch.cat([m([rows[j] for j in i] if len(i) > 1 else rows[i[0]]) for m, i in zip(mods, inputs)], 1)

    return mods, params, critic


def _f64(params, rows):
    """The float64 restatement for every agent: rows = per-agent NumPy [n, D_k] -> [n, n_agents]."""
    cols = []
    for p in params:
        w = [_np(getattr(p, n)) for n in p.NAMES]
        cols.append(critic_f64(w, np.concatenate([rows[j] for j in p.inputs], 1)))
    return np.stack(cols, 1)


SCHEMES = [("coupled", "mono"), ("decoupled", "dtde"), ("decoupled", "ctde")]


@pytest.mark.parametrize("kind,scheme", SCHEMES)
def test_next_values_on_a_hand_built_storage(kind, scheme):
    """T = 5, N = 70: 350 transitions = 6 tiles of 64 in the kernel's flat (t, n) order.  About 10 % random resets from every flag (each
    agent's done, truncated); tile 1 holds no reset (the copy-only path), tile 2 only resets (alternating flags).  final_obs rows of
    envs that did not reset are NaN."""
    from gym_rotor_amd import QuadVecEnv, RolloutStorage
    T, N = 5, 70
    env = QuadVecEnv(kind, N, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=100)
    st = RolloutStorage(env, T)
    assert st.final_obs is not None
    A = st.n_agents
    gen = torch.Generator("cuda").manual_seed(5)
    for o in st.obs:
        o.copy_(torch.rand(o.shape, device="cuda", generator=gen) * 2 - 1)
    done = torch.rand(T * N, A, device="cuda", generator=gen) < 0.04
    trunc = torch.rand(T * N, device="cuda", generator=gen) < 0.04
    done[64:128], trunc[64:128] = False, False
    lane = torch.arange(64, device="cuda")
    done[128:192], trunc[128:192] = False, lane % (A + 1) == A
    for k in range(A):
        done[128:192, k] = lane % (A + 1) == k
    st.done.copy_(done.view(T, N, A)); st.truncated.copy_(trunc.view(T, N))
    mask = st.reset_mask()
    flat = mask.view(-1)
    assert not flat[64:128].any() and flat[128:192].all() and 0.02 < flat[192:].float().mean() < 0.3
    for f in st.final_obs:
        f.copy_(torch.rand(f.shape, device="cuda", generator=gen) * 2 - 1)
        f[~mask] = float("nan")

    mods, params, critic = _modules(kind, scheme, seed=3)
    st.value.fill_(float("nan"))
    nv = st.compute_values(params)
    torch.cuda.synchronize()
    assert nv.shape == (T, N, A) and nv.dtype == torch.float32
    assert not torch.isnan(nv).any() and not torch.isnan(st.value).any()
    v64 = _f64(params, [_np(o).reshape((T + 1) * N, -1) for o in st.obs]).reshape(T + 1, N, A)
    b = bar(v64)
    e_val = float(np.abs(_np(st.value).astype(np.float64) - v64).max())
    m = _np(mask)
    assert torch.equal(nv[~mask], st.value[1:][~mask])                      # bit for bit where the env went on
    f64 = _f64(params, [_np(f)[m] for f in st.final_obs])
    e_fin = float(np.abs(_np(nv)[m].astype(np.float64) - f64).max())
    want = st.next_values(critic)                                           # the torch-module path on the same storage
    e_mod = float((nv - want).abs().max())
    print(f"next values {kind}/{scheme}: value {e_val:.3e}  reset rows {e_fin:.3e}  against next_values(module) {e_mod:.3e}  bar {b:.3e}")
    assert e_val <= b and e_fin <= b and e_mod <= b


def test_compute_values_without_final_obs_returns_the_shifted_values():
    from gym_rotor_amd import QuadVecEnv, RolloutStorage
    env = QuadVecEnv("coupled", 70, device="cuda", obs_rows=True)
    st = RolloutStorage(env, 3)
    assert st.final_obs is None
    st.obs[0].copy_(torch.rand(st.obs[0].shape, device="cuda") * 2 - 1)
    mods, params, critic = _modules("coupled", "mono", seed=4)
    nv = st.compute_values(params)
    assert nv.data_ptr() == st.value[1:].data_ptr() and nv.shape == (3, 70, 1)
    with torch.no_grad():
        want = mods[0](st.obs[0].reshape(-1, 23)).reshape(4, 70, 1)
    assert (st.value - want).abs().max() <= 2e-6
    with pytest.raises(ValueError, match="one CriticParams per agent"):
        st.compute_values(params + params)


# ------------------------------------------------------------------------------------------------------------------------------
# end to end: collect -> compute_values -> compute_gae
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,scheme", SCHEMES)
def test_collect_values_gae_against_the_torch_critic(kind, scheme):
    from gym_rotor_amd import QuadVecEnv, RolloutStorage, random_actors
    n, T = 128, 8
    env = QuadVecEnv(kind, n, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=6, seed=21)
    env.reset("train")
    env.get_norm_error_state()
    st = RolloutStorage(env, T)
    st.collect(env, random_actors(kind, "cuda", generator=torch.Generator("cuda").manual_seed(9), log_std=-0.5))
    assert st.reset_mask().any() and not st.reset_mask().all()
    mods, params, critic = _modules(kind, scheme, seed=6)

    nv = st.compute_values(params)
    adv, tgt = (t.clone() for t in st.compute_gae(0.99, 0.9, next_value=nv, want_stats=False))
    value = st.value.clone()

    st.value.copy_(critic([o.reshape((T + 1) * n, -1) for o in st.obs]).reshape(T + 1, n, st.n_agents))
    adv_t, tgt_t = st.compute_gae(0.99, 0.9, next_value=st.next_values(critic), want_stats=False)
    torch.cuda.synchronize()
    e_v, e_a, e_t = (float((a - b).abs().max()) for a, b in ((value, st.value), (adv, adv_t), (tgt, tgt_t)))
    print(f"collect + values + gae {kind}/{scheme}: value {e_v:.3e}  advantage {e_a:.3e}  td_target {e_t:.3e}")
    assert torch.isfinite(adv).all() and torch.isfinite(tgt).all()
    assert e_v <= 2e-6 * max(1.0, float(st.value.abs().max()))
    assert e_a <= 2e-5 and e_t <= 2e-5


# ------------------------------------------------------------------------------------------------------------------------------
# torch.ops
# ------------------------------------------------------------------------------------------------------------------------------
def test_torch_ops_return_the_bits_of_the_ctypes_path(fixture):  # noqa: F811
    from gym_rotor_amd.policy import critic_next_values, critic_values
    T, N = 3, 70
    p = _params(case_weights(fixture, "ctde"), (0, 1))
    w = [getattr(p, n) for n in p.NAMES]
    gen = torch.Generator("cuda").manual_seed(8)
    obs = [torch.rand(T + 1, N, d, device="cuda", generator=gen) * 2 - 1 for d in (15, 3)]
    fin = [torch.rand(T, N, d, device="cuda", generator=gen) * 2 - 1 for d in (15, 3)]
    done = torch.rand(T, N, 2, device="cuda", generator=gen) < 0.1
    trunc = torch.rand(T, N, device="cuda", generator=gen) < 0.1
    got = []
    for path in ("ctypes", "op"):
        value = torch.full((T + 1, N, 2), -3.0, device="cuda")
        nv = torch.full((T, N, 2), -3.0, device="cuda")
        if path == "ctypes":
            critic_values(p, obs, value[..., 1])
            critic_next_values(p, fin, done, trunc, value[..., 1], nv[..., 1])
        else:
            torch.ops.gym_rotor_amd.qr_critic_values(w, [0, 1], obs[0], obs[1], value[..., 1])
            torch.ops.gym_rotor_amd.qr_critic_next_values(w, [0, 1], fin[0], fin[1], done, trunc, value[..., 1], nv[..., 1])
        got.append((value, nv))
    (v0, n0), (v1, n1) = got
    assert torch.equal(v0, v1) and torch.equal(n0, n1)
    assert (v0[..., 0] == -3).all() and (n0[..., 0] == -3).all() and (v0[..., 1] != -3).all() and (n0[..., 1] != -3).all()
    reset = done.any(-1) | trunc
    assert torch.equal(n0[..., 1][~reset], v0[1:, :, 1][~reset]) and reset.any()
    # argument checks of the op: dtype, shape, stride
    with pytest.raises(ValueError, match="float32"):
        torch.ops.gym_rotor_amd.qr_critic_values(w, [0, 1], obs[0].double(), obs[1], v0[..., 1])
    with pytest.raises(ValueError, match="rows"):
        torch.ops.gym_rotor_amd.qr_critic_values(w, [0, 1], obs[0][1:], obs[1], v0[..., 1])
    with pytest.raises(ValueError, match="columns"):
        torch.ops.gym_rotor_amd.qr_critic_values(w, [0], obs[0], None, v0[..., 1])
    with pytest.raises(ValueError, match="element stride"):
        torch.ops.gym_rotor_amd.qr_critic_values(w, [0, 1], obs[0], obs[1], v0[:, :35, 1])
    with pytest.raises(ValueError, match="same element stride"):
        torch.ops.gym_rotor_amd.qr_critic_next_values(w, [0, 1], fin[0], fin[1], done, trunc, v0[..., 1], torch.zeros(T, N, device="cuda"))
