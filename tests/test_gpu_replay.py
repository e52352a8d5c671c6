"""The replay buffer's two launches on the GPU (qr_replay_add, qr_replay_sample; td3.ReplayBuffer.append / sample_index /
use_device_state): `append` against `add` on a twin buffer bit for bit — wraps, exact fits, consecutive appends, sentinels outside the
written rows, more tiles than the grid holds — `sample_index` against tests/replay_ref.py bit for bit, the device counters against the
by-value path and under a captured graph, the two torch ops, and one append -> sample_index -> td3_critic_loss chain."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_ref as R  # noqa: E402
from test_replay_host import COUPLED, DECOUPLED, fake_storage  # noqa: E402
from test_td3_critic_host import _Actor, _Twin  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
T, N = 3, 65   # 195 transitions: four 64-transition tiles, the last one ragged; N crosses a wave


def _buffers(dims, capacity, count, size=None, **kw):
    """Twin buffers at the same position, every row pre-filled with the sentinel."""
    from gym_rotor_amd import ReplayBuffer
    pair = []
    for _ in range(2):
        b = ReplayBuffer(capacity, *dims, "cuda", **kw)
        for t in b.obs + b.obs_next + b.act + b.rwd + b.done:
            t.fill_(SENTINEL)
        b.count, b.current_size = count, count if size is None else size
        pair.append(b)
    return pair


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _assert_equal(got, want, label=""):
    assert (got.count, got.current_size) == (want.count, want.current_size), label
    for k in range(want.n_agents):
        for name, t in want.tensors(k).items():
            assert _same_bits(got.tensors(k)[name], t), (label, k, name)


@pytest.mark.parametrize("dims,final", [(COUPLED, True), (DECOUPLED, True), (DECOUPLED, False), (COUPLED, False)])
@pytest.mark.parametrize("capacity,count", [(200, 190), (195, 0), (195, 77), (1000, 0)])
def test_append_is_add_bit_for_bit(dims, final, capacity, count):
    s = fake_storage(*dims, T, N, device="cuda", final_obs=final, seed=capacity + count)
    got, want = _buffers(dims, capacity, count)
    want.add(s)
    got.append(s)
    torch.cuda.synchronize()
    _assert_equal(got, want)
    written = (count + np.arange(T * N)) % capacity
    untouched = torch.from_numpy(np.setdiff1d(np.arange(capacity), written)).cuda()
    assert untouched.numel() == capacity - T * N
    for k in range(got.n_agents):
        for name, t in got.tensors(k).items():
            assert (t[untouched] == SENTINEL).all(), (k, name)
    # the rows that came from final_obs are dense, and are not obs[t + 1]'s
    m = s.reset_mask().reshape(-1)
    assert 0.3 < float(m.float().mean()) < 0.9
    rows = torch.from_numpy(written).cuda()
    nxt = got.obs_next[0][rows]
    if final:
        assert torch.equal(nxt[m], s.final_obs[0].reshape(T * N, -1)[m]) and torch.equal(nxt[~m], s.obs[0][1:].reshape(T * N, -1)[~m])
    else:
        assert torch.equal(nxt, s.obs[0][1:].reshape(T * N, -1))
    for k in range(got.n_agents):   # done is the agent's own flag
        assert torch.equal(got.done[k][rows], s.done[..., k].reshape(-1).float())


@pytest.mark.parametrize("dims", [COUPLED, DECOUPLED])
def test_two_consecutive_appends(dims):
    got, want = _buffers(dims, 300, 250, 250)
    for seed in (1, 2):
        s = fake_storage(*dims, T, N, device="cuda", seed=seed)
        want.add(s)
        got.append(s)
    torch.cuda.synchronize()
    _assert_equal(got, want)
    assert (got.count, got.current_size) == ((250 + 2 * T * N) % 300, 300)


def test_append_with_more_tiles_than_the_grid():
    """140 000 transitions are 2188 tiles, the grid holds 2048 per tensor: the grid-stride walk, with a wrap inside."""
    t, n = 2, 70_000
    s = fake_storage(*COUPLED, t, n, device="cuda", seed=5)
    got, want = _buffers(COUPLED, 150_000, 100_000)
    want.add(s)
    got.append(s)
    torch.cuda.synchronize()
    _assert_equal(got, want)
    assert (got.obs[0][90_000:100_000] == SENTINEL).all() and got.count == 90_000


def test_append_reads_the_storage_of_a_real_rollout():
    from gym_rotor_amd import ActorParams, QuadVecEnv, ReplayBuffer, RolloutStorage
    torch.manual_seed(3)
    env = QuadVecEnv("decoupled", 70, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=2, seed=4)
    env.reset("train")
    actors = [ActorParams.from_td3_module(_Actor(15, 16, 4).cuda(), 0.1), ActorParams.from_td3_module(_Actor(3, 4, 1).cuda(), 0.1)]
    storage = RolloutStorage(env, 3)
    storage.set_initial_obs(env.get_norm_error_state())
    env.rollout_actor(actors, 3, out=storage.horizon(), noise_seed=5)
    got, want = ReplayBuffer(400, env.obs_dims, [4, 1], "cuda"), ReplayBuffer(400, env.obs_dims, [4, 1], "cuda")
    want.add(storage)
    got.append(storage)
    torch.cuda.synchronize()
    assert storage.final_obs is not None and bool(storage.truncated.any())
    _assert_equal(got, want)


# ---------------------------------------------------------------- sampling
SHAPES = [(1, 1), (5, 3), (64, 64), (65, 65), (1000, 64), (1000, 1000), (2 ** 20 + 1, 256), (1_000_000, 65_536)]
SEEDS = (12345, 2 ** 40 + 17)


@pytest.fixture(scope="module")
def expected():
    return {(n, B, seed): R.sample(n, B, seed, np.arange(3)) for n, B in SHAPES for seed in SEEDS}


@pytest.mark.parametrize("n,B", SHAPES)
def test_sample_index_is_the_restatement_bit_for_bit(expected, n, B):
    from gym_rotor_amd import ReplayBuffer, replay_sample
    for seed in SEEDS:
        buf = ReplayBuffer(8, [1], [1], "cuda", seed=seed)
        buf.current_size = n          # the sampler reads the fill level alone
        want = expected[(n, B, seed)]
        for d in range(3):
            idx = buf.sample_index(B)
            assert idx.dtype == torch.int64 and idx.shape == (B,) and buf.draw == d + 1
            assert np.array_equal(idx.cpu().numpy(), want[d]), (n, B, seed, d)
        assert np.array_equal(replay_sample(n, B, seed, 2).cpu().numpy(), want[2])   # the functional form, an explicit draw
        assert int(buf.status) == 0
        if B > 1:
            assert len(set(want[0].tolist())) == B and not np.array_equal(want[0], want[1])
        buf.seed(seed + 1)            # a new key; draw keeps counting
        assert np.array_equal(buf.sample_index(B).cpu().numpy(), R.sample(n, B, seed + 1, 3))


def test_sample_index_out_is_written_in_place_and_allocates_nothing():
    from gym_rotor_amd import ReplayBuffer
    buf = ReplayBuffer(8, [1], [1], "cuda", seed=9)
    buf.current_size = 100_000
    out = torch.full((256,), -1, dtype=torch.int64, device="cuda")
    assert buf.sample_index(256, out=out) is out
    torch.cuda.synchronize()
    first = out.clone()
    mem = torch.cuda.memory_allocated()
    assert buf.sample_index(256, out=out) is out
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem
    assert np.array_equal(first.cpu().numpy(), R.sample(100_000, 256, 9, 0)) and np.array_equal(out.cpu().numpy(), R.sample(100_000, 256, 9, 1))


# ---------------------------------------------------------------- device counters
def test_device_state_equals_the_by_value_path():
    dev_buf, val_buf = _buffers(DECOUPLED, 300, 250, 250, seed=77)
    st = dev_buf.use_device_state()
    assert st.is_cuda and st.tolist() == [250, 250, 0]
    for seed in (1, 2):
        s = fake_storage(*DECOUPLED, T, N, device="cuda", seed=seed)
        dev_buf.append(s)
        val_buf.append(s)
        for _ in range(2 - (seed == 1)):   # three samples in all
            assert torch.equal(dev_buf.sample_index(64), val_buf.sample_index(64))
    torch.cuda.synchronize()
    _assert_equal(dev_buf, val_buf)
    assert st.tolist() == [dev_buf.count, dev_buf.current_size, dev_buf.draw] == [(250 + 2 * T * N) % 300, 300, 3]
    # the device's values are what the kernels read: after the host's ints are spoilt, the results stay the by-value path's
    dev_buf.count, dev_buf.current_size, dev_buf.draw = 0, 300, 0
    s = fake_storage(*DECOUPLED, T, N, device="cuda", seed=3)
    dev_buf.append(s)
    val_buf.append(s)
    assert torch.equal(dev_buf.sample_index(64), val_buf.sample_index(64))
    dev_buf.pull_device_state()
    _assert_equal(dev_buf, val_buf)
    assert dev_buf.draw == val_buf.draw == 4
    # add after opting in leaves the tensor equal to the host's ints
    dev_buf.add(s)
    val_buf.add(s)
    torch.cuda.synchronize()
    assert st.tolist() == [dev_buf.count, dev_buf.current_size, dev_buf.draw] == [val_buf.count, 300, 4]
    _assert_equal(dev_buf, val_buf)
    assert int(dev_buf.status) == 0


def test_captured_append_and_sample_replay_like_the_eager_sequence():
    """One append + sample_index captured once; every replay appends at the advanced position and draws a fresh minibatch, like the
    eager sequence on a twin buffer.  The storage's contents change between replays.  (The default number of hardware queues.)"""
    graph_buf, eager_buf = _buffers(DECOUPLED, 500, 0, seed=31)
    s = fake_storage(*DECOUPLED, T, N, device="cuda", seed=8)
    graph_buf.append(s)       # eager first: the code objects are loaded, current_size admits the batch
    eager_buf.append(s)
    st = graph_buf.use_device_state()
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    host = (graph_buf.count, graph_buf.current_size, graph_buf.draw)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graph_buf.append(s)
        graph_buf.sample_index(64, out=out)
    torch.cuda.synchronize()
    assert st.tolist() == list(host) == [195, 195, 0]      # capturing ran nothing
    for step in range(3):
        for t in s.obs + s.final_obs + [s.act_all, s.reward]:
            t.add_(1.0)
        g.replay()
        eager_buf.append(s)
        want = eager_buf.sample_index(64)
        torch.cuda.synchronize()
        assert torch.equal(out, want), step
        assert st.tolist() == [eager_buf.count, eager_buf.current_size, eager_buf.draw], step
        assert np.array_equal(want.cpu().numpy(), R.sample(eager_buf.current_size, 64, 31, step)), step
    graph_buf.pull_device_state()
    _assert_equal(graph_buf, eager_buf)
    assert (graph_buf.count, graph_buf.current_size, graph_buf.draw) == ((4 * 195) % 500, 500, 3)


# ---------------------------------------------------------------- torch ops, end to end
def test_torch_ops_give_the_methods_results():
    import gym_rotor_amd  # noqa: F401
    ops = torch.ops.gym_rotor_amd
    for dims, final in ((COUPLED, True), (DECOUPLED, True), (DECOUPLED, False)):
        s = fake_storage(*dims, T, N, device="cuda", final_obs=final, seed=12)
        got, want = _buffers(dims, 200, 190)
        want.append(s)
        flat = [got.tensors(k)[name] for k in range(got.n_agents) for name in ("obs", "obs_next", "act", "rwd", "done")]
        ops.qr_replay_add(flat, s.obs, s.final_obs if final else [], s.act_all, s.reward, s.done, s.truncated, 190, None)
        got.count, got.current_size = want.count, want.current_size
        torch.cuda.synchronize()
        _assert_equal(got, want, (dims, final))
    buf = _buffers(COUPLED, 8, 0, seed=5)[0]
    buf.current_size = 1000
    want = buf.sample_index(64)
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    ops.qr_replay_sample(out, 1000, 5, 0, None, None)
    assert torch.equal(out, want)
    state = torch.tensor([0, 1000, 0], dtype=torch.int64, device="cuda")
    ops.qr_replay_sample(out, 1000, 5, 99, state, None)      # the state's draw wins, and advances
    assert torch.equal(out, want) and state.tolist() == [0, 1000, 1]


def test_append_sample_index_critic_loss_end_to_end():
    from gym_rotor_amd import td3_critic_loss
    torch.manual_seed(13)
    critic, critic_t, actor_t = _Twin().cuda(), _Twin().cuda(), _Actor().cuda()
    s = fake_storage(*COUPLED, T, N, device="cuda", seed=21)
    got, want = _buffers(COUPLED, 400, 0, seed=3)
    want.add(s)
    got.append(s)
    idx = got.sample_index(128)
    assert len(set(idx.tolist())) == 128 and int(idx.max()) < T * N and int(idx.min()) >= 0
    eps = torch.randn(128, 4, device="cuda")
    stats = []
    for buf in (got, want):
        critic.zero_grad()
        stats.append(td3_critic_loss(critic, critic_t, actor_t, buf, 0, idx, noise=eps).clone())
    torch.cuda.synchronize()
    assert torch.isfinite(stats[0]).all() and _same_bits(stats[0], stats[1])
