"""The time-limit "solved" done rule on the GPU (qr_replay_add_rule; td3.ReplayBuffer.append(storage, time_limit="solved")) against its
torch twin `add(storage, time_limit="solved")` on a twin buffer, bit for bit — the hand-made rows of tests/replay_rule_ref.py in every
tile, wraps and exact fits, a real rollout with truncations, more tiles than the grid — the device counters, a captured graph, the torch
op, the critic loss that shows the rule matters, and `OffPolicyCollector`."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_rule_ref as RR  # noqa: E402
from test_gpu_replay import SENTINEL, _assert_equal, _buffers, _same_bits  # noqa: E402
from test_replay_host import COUPLED, DECOUPLED, fake_storage  # noqa: E402
from test_replay_rule_host import rule_storage  # noqa: E402
from test_td3_critic_host import _Actor, _Twin  # noqa: E402

pytestmark = pytest.mark.gpu

T, N = 3, 65   # 195 transitions: 64-transition tiles, the last one partial; N crosses a wave


@pytest.mark.parametrize("dims,final", [(COUPLED, True), (DECOUPLED, True), (DECOUPLED, False), (COUPLED, False)])
@pytest.mark.parametrize("capacity,count", [(200, 190), (195, 0)])
def test_append_solved_is_add_solved_bit_for_bit(dims, final, capacity, count):
    s = rule_storage(dims, device="cuda", final_obs=final, seed=capacity + count)
    got, want = _buffers(dims, capacity, count)
    want.add(s, time_limit="solved")
    got.append(s, time_limit="solved")
    torch.cuda.synchronize()
    _assert_equal(got, want)
    written = (count + np.arange(T * N)) % capacity
    untouched = torch.from_numpy(np.setdiff1d(np.arange(capacity), written)).cuda()
    assert untouched.numel() == capacity - T * N
    for k in range(got.n_agents):
        for name, t in got.tensors(k).items():
            assert (t[untouched] == SENTINEL).all(), (k, name)
    # the hand-made rows hold what the cases say, in every tile they were planted in
    places = RR.places(T, N)
    for (t, n), exp in RR.expected(places, got.n_agents).items():
        row = (count + t * N + n) % capacity
        assert tuple(float(got.done[k][row]) for k in range(got.n_agents)) == tuple(exp), (t, n, places[(t, n)])
    # the rule changed rows in both directions, and only time-limit rows
    rows = torch.from_numpy(written).cuda()
    lim = s.truncated.reshape(-1)
    for k in range(got.n_agents):
        own, stored = s.done[..., k].reshape(-1).float(), got.done[k][rows]
        assert torch.equal(stored[~lim], own[~lim])
        assert bool(((stored == 1) & (own == 0)).any()) and bool(((stored == 0) & (own == 1)).any())


def test_append_solved_reads_the_storage_of_a_real_rollout():
    """max_episode_steps = 2 inside T = 3: every env meets its time limit (or crashes first)."""
    from gym_rotor_amd import ActorParams, QuadVecEnv, ReplayBuffer, RolloutStorage
    torch.manual_seed(3)
    env = QuadVecEnv("decoupled", 70, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=2, seed=4)
    env.reset("train")
    actors = [ActorParams.from_td3_module(_Actor(15, 16, 4).cuda(), 0.1), ActorParams.from_td3_module(_Actor(3, 4, 1).cuda(), 0.1)]
    storage = RolloutStorage(env, 3)
    storage.set_initial_obs(env.get_norm_error_state())
    env.rollout_actor(actors, 3, out=storage.horizon(), noise_seed=5)
    got, want, own = (ReplayBuffer(400, env.obs_dims, [4, 1], "cuda") for _ in range(3))
    for b in (got, want):
        b.time_limit_rule = b.time_limit_rule._replace(pos_tol=1.0, rot_tol=1.0)   # wide enough that freshly reset envs count as solved
    want.add(storage, time_limit="solved")
    got.append(storage, time_limit="solved")
    own.append(storage)
    torch.cuda.synchronize()
    assert storage.final_obs is not None and int(storage.truncated.sum()) >= 1
    _assert_equal(got, want)
    lim = storage.truncated.reshape(-1)
    assert bool((got.done[0][:210][lim] == 1).any()) and not torch.equal(got.done[0], own.done[0])
    for name in ("obs", "obs_next", "act", "rwd"):
        assert _same_bits(got.tensors(1)[name], own.tensors(1)[name])


def test_append_solved_with_more_tiles_than_the_grid():
    """140 000 transitions are 2188 tiles, the grid holds 2048 per tensor: the grid-stride walk, with a wrap inside."""
    t, n = 2, 70_000
    s = fake_storage(*DECOUPLED, t, n, device="cuda", seed=5)
    s.final_obs[0][:, ::3, :3] *= 0.02
    s.final_obs[1][:, ::3, 0] *= 0.01
    s.reward[:, ::5] = -1.0
    got, want = _buffers(DECOUPLED, 150_000, 100_000)
    want.add(s, time_limit="solved")
    got.append(s, time_limit="solved")
    torch.cuda.synchronize()
    _assert_equal(got, want)
    assert (got.done[0][90_000:100_000] == SENTINEL).all() and got.count == 90_000
    last = got.done[1][89_000:90_000]                 # rows of the tiles past the grid's first sweep
    assert 0.02 < float(last.mean()) < 0.98


@pytest.mark.parametrize("dims,final", [(COUPLED, True), (DECOUPLED, True), (DECOUPLED, False)])
def test_own_is_the_append_as_it_was(dims, final):
    s = rule_storage(dims, device="cuda", final_obs=final, seed=9)
    new, old = _buffers(dims, 200, 190)
    torch_twin = _buffers(dims, 200, 190)[0]
    new.append(s, time_limit="own")
    old.append(s)
    torch_twin.add(s)
    torch.cuda.synchronize()
    for k in range(new.n_agents):
        for name, t in new.tensors(k).items():
            assert torch.equal(t, old.tensors(k)[name]) and torch.equal(t, torch_twin.tensors(k)[name]), (k, name)
    assert (new.count, new.current_size) == (old.count, old.current_size) == (185, 200)


def test_device_state_equals_the_by_value_path():
    dev_buf, val_buf = _buffers(DECOUPLED, 300, 250, 250, seed=77)
    st = dev_buf.use_device_state()
    for seed in (1, 2):
        s = rule_storage(DECOUPLED, device="cuda", seed=seed)
        dev_buf.append(s, time_limit="solved")
        val_buf.append(s, time_limit="solved")
    dev_buf.count, dev_buf.current_size = 0, 300      # the kernels read the device's values, not these
    s = rule_storage(DECOUPLED, device="cuda", seed=3)
    dev_buf.append(s, time_limit="solved")
    val_buf.append(s, time_limit="solved")
    dev_buf.pull_device_state()
    torch.cuda.synchronize()
    _assert_equal(dev_buf, val_buf)
    assert st.tolist()[:2] == [(250 + 3 * T * N) % 300, 300]


def test_captured_append_solved_and_sample_replay_like_the_eager_sequence():
    graph_buf, eager_buf = _buffers(DECOUPLED, 500, 0, seed=31)
    s = rule_storage(DECOUPLED, device="cuda", seed=8)
    graph_buf.append(s, time_limit="solved")       # eager first: the code objects are loaded, current_size admits the batch
    eager_buf.append(s, time_limit="solved")
    st = graph_buf.use_device_state()
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graph_buf.append(s, time_limit="solved")
        graph_buf.sample_index(64, out=out)
    torch.cuda.synchronize()
    assert st.tolist() == [195, 195, 0]              # capturing ran nothing
    for step in range(3):
        s.final_obs[0].mul_(0.5)                     # more rows come within the tolerance with every replay
        s.final_obs[1].mul_(0.5)
        g.replay()
        eager_buf.append(s, time_limit="solved")
        want = eager_buf.sample_index(64)
        torch.cuda.synchronize()
        assert torch.equal(out, want), step
        assert st.tolist() == [eager_buf.count, eager_buf.current_size, eager_buf.draw], step
    graph_buf.pull_device_state()
    _assert_equal(graph_buf, eager_buf)
    assert (graph_buf.count, graph_buf.current_size, graph_buf.draw) == ((4 * 195) % 500, 500, 3)


def test_torch_op_gives_the_methods_result():
    import gym_rotor_amd  # noqa: F401
    ops = torch.ops.gym_rotor_amd
    for dims, final in ((COUPLED, True), (DECOUPLED, True), (DECOUPLED, False)):
        s = rule_storage(dims, device="cuda", final_obs=final, seed=12)
        got, want = _buffers(dims, 200, 190)
        want.time_limit_rule = want.time_limit_rule._replace(x_lim=1.25, pos_tol=0.04, rot_tol=0.02)
        want.append(s, time_limit="solved")
        flat = [got.tensors(k)[name] for k in range(got.n_agents) for name in ("obs", "obs_next", "act", "rwd", "done")]
        ops.qr_replay_add_rule(flat, s.obs, s.final_obs if final else [], s.act_all, s.reward, s.done, s.truncated, 190, None, 1.25, 0.04, 0.02)
        got.count, got.current_size = want.count, want.current_size
        torch.cuda.synchronize()
        _assert_equal(got, want, (dims, final))


def test_the_rule_reaches_the_critic_loss():
    """append("solved") -> sample_index -> td3_critic_loss: the stats of the add("solved")-fed buffer bit for bit, and not those of the
    "own"-fed buffer on a minibatch that holds solved time-limit rows (they are not bootstrapped)."""
    from gym_rotor_amd import td3_critic_loss
    torch.manual_seed(13)
    critic, critic_t, actor_t = _Twin().cuda(), _Twin().cuda(), _Actor().cuda()
    s = rule_storage(COUPLED, device="cuda", seed=21)
    got, want = _buffers(COUPLED, 400, 0, seed=3)
    own = _buffers(COUPLED, 400, 0, seed=3)[0]
    want.add(s, time_limit="solved")
    got.append(s, time_limit="solved")
    own.append(s)
    idx = got.sample_index(128)
    solved_rows = (got.done[0][idx] == 1) & (own.done[0][idx] == 0) & s.truncated.reshape(-1)[idx]
    assert int(solved_rows.sum()) >= 1
    eps = torch.randn(128, 4, device="cuda")
    stats = []
    for buf in (got, want, own):
        critic.zero_grad()
        stats.append(td3_critic_loss(critic, critic_t, actor_t, buf, 0, idx, noise=eps).clone())
    torch.cuda.synchronize()
    assert torch.isfinite(stats[0]).all() and _same_bits(stats[0], stats[1])
    assert not torch.equal(stats[0], stats[2])


# ---------------------------------------------------------------- OffPolicyCollector
def _twin_of(buffer):
    from gym_rotor_amd import ReplayBuffer
    twin = ReplayBuffer(buffer.capacity, buffer.obs_dims, buffer.action_dims, "cuda")
    twin.time_limit_rule = buffer.time_limit_rule
    return twin


def test_collector_warm_up_td3_and_sac_horizons():
    from gym_rotor_amd import OffPolicyCollector, QuadVecEnv, ReplayBuffer, random_actors
    n, t = 128, 3
    env = QuadVecEnv("decoupled", n, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=2, seed=6)
    env.reset("train")
    env.get_norm_error_state()
    buf = ReplayBuffer(5000, env.obs_dims, [4, 1], "cuda")
    col = OffPolicyCollector(env, buf, horizon=t, start_timesteps=2 * t, algo="td3", explor_noise_std_init=0.3, explor_noise_std_min=0.05,
                             decay_timesteps=12, time_limit="solved", generator=torch.Generator(device="cuda").manual_seed(2))
    buf.time_limit_rule = buf.time_limit_rule._replace(pos_tol=1.0, rot_tol=1.0)   # freshly reset envs count as solved
    assert buf.time_limit_rule.x_lim == float(env.x_lim)
    twin = _twin_of(buf)
    gen = torch.Generator(device="cuda").manual_seed(1)
    td3 = random_actors("decoupled", "cuda", gen, log_std=-9.0)
    sac = random_actors("decoupled", "cuda", gen, log_std=-1.0, algo="sac")
    std, decay = 0.3, (0.3 - 0.05) / 12
    mem = None
    for call in range(4):                            # warm-up, warm-up, TD3, TD3
        if call in (1, 3):                           # the second call of a kind allocates nothing
            torch.cuda.synchronize()
            mem = torch.cuda.memory_allocated()
        st = col.collect(td3)
        if call in (1, 3):
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == mem, call
        twin.add(st, time_limit="solved")
        torch.cuda.synchronize()
        _assert_equal(buf, twin, call)
        assert col.total_timesteps == (call + 1) * t and int(st.truncated.sum()) >= 1
        if call < 2:
            assert float(st.act_all.min()) >= -1.0 and float(st.act_all.max()) < 1.0 and float(st.act_all.std()) > 0.4
            assert torch.equal(st.act_all, col.random_actions)
        else:
            for a in td3:
                assert torch.equal(a.log_std, torch.full_like(a.log_std, math.log(std)))
        for _ in range(t):
            std = std - decay if std > 0.05 else 0.05
        assert col.explor_noise_std == std
    assert not torch.equal(buf.act[0][:t * n], buf.act[0][t * n:2 * t * n])          # the two warm-up horizons drew different actions
    assert bool((buf.done[0][:4 * t * n] == 1).any())
    sac_col = OffPolicyCollector(env, buf, horizon=t, algo="sac", time_limit="solved")
    for call in range(2):
        if call == 1:
            torch.cuda.synchronize()
            mem = torch.cuda.memory_allocated()
        st = sac_col.collect(sac)
        if call == 1:
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == mem
        twin.add(st, time_limit="solved")
        torch.cuda.synchronize()
        _assert_equal(buf, twin, ("sac", call))
        assert float(st.act_all.abs().max()) <= 1.0   # tanh of the sample
    assert buf.count == 6 * t * n and sac_col.total_timesteps == 2 * t
