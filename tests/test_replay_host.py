"""The replay buffer's append and minibatch sampler (qr_replay_add, qr_replay_sample; td3.ReplayBuffer.append / sample_index /
use_device_state, td3.replay_add / replay_sample) without a GPU: the NumPy restatement of tests/replay_ref.py — that the sampler is a
permutation, its distinctness at the worst domain-to-n ratio, its keys, its uniformity as a chi-square condition, and the append rule
against `ReplayBuffer.add` on CPU tensors — the two new structs' layout, the C entries' errors and every ValueError of the Python side."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_ref as R  # noqa: E402

from gym_rotor_amd import _lib as L  # noqa: E402
from gym_rotor_amd.td3 import ReplayBuffer, replay_add, replay_sample  # noqa: E402

COUPLED, DECOUPLED = ((23,), (4,)), ((15, 3), (4, 1))   # (observation widths, action widths) of the two wrappers


def fake_storage(obs_dims, action_dims, T, N, device="cpu", final_obs=True, seed=0, p=0.3):
    """What `ReplayBuffer.add` / `append` read of a RolloutStorage, filled directly: random floats, done and truncated set in about
    `p` of their entries, so rows whose obs_next comes from final_obs are dense."""
    g = torch.Generator().manual_seed(seed)
    na = len(obs_dims)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(device)
    s = types.SimpleNamespace(T=T, N=N, n_agents=na, action_dims=list(action_dims), device=torch.device(device))
    s.obs = [rnd(T + 1, N, d) for d in obs_dims]
    s.final_obs = [rnd(T, N, d) for d in obs_dims] if final_obs else None
    s.act_all = rnd(T, N, sum(action_dims))
    s.act = list(torch.split(s.act_all, list(action_dims), dim=-1))
    s.reward = rnd(T, N, na)
    s.done = (torch.rand(T, N, na, generator=g) < p).to(device)
    s.truncated = (torch.rand(T, N, generator=g) < p).to(device)
    s.reset_mask = lambda: s.done.any(-1) | s.truncated
    return s


# ---------------------------------------------------------------- the sampler's restatement
@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 1000])
def test_full_batch_is_a_permutation(n):
    for seed, draw in ((0, 0), (12345, 7), (2 ** 40 + 3, 2 ** 33 + 1)):
        assert sorted(R.sample(n, n, seed, draw).tolist()) == list(range(n))


@pytest.mark.parametrize("n", [1_000_000, 2 ** 20 + 1])   # the second: the domain 4^11 is 4 n - 4, the worst ratio
def test_distinct_and_in_range_at_large_n(n):
    idx, walk = R.sample(n, 256, 12345, np.arange(8), return_walk=True)
    assert idx.shape == (8, 256) and idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < n
    assert all(len(set(row.tolist())) == 256 for row in idx)
    assert walk <= 1 << (2 * R.half_bits(n))
    assert R.half_bits(n) == (10 if n == 1_000_000 else 11)


def test_half_bits():
    assert [R.half_bits(n) for n in (1, 2, 4, 5, 16, 17, 64, 65, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1)] == [1, 1, 1, 2, 2, 3, 3, 4, 10, 11, 16]


def test_draws_and_seeds_differ():
    base = R.sample(1000, 64, 12345, 0)
    for seed, draw in ((12345, 1), (12346, 0), (12345 + 2 ** 32, 0), (2 ** 63 + 11, 0), (12345, 2 ** 32)):   # the high words are keyed too
        assert not np.array_equal(base, R.sample(1000, 64, seed, draw)), (seed, draw)
    assert np.array_equal(base, R.sample(1000, 64, 12345, 0))
    assert np.array_equal(R.sample(1000, 64, 12345, [0, 5])[1], R.sample(1000, 64, 12345, 5))
    assert np.array_equal(base[:16], R.sample(1000, 16, 12345, 0))   # index[j] depends on j alone, not on the batch


def test_sampler_refuses_bad_sizes():
    for n, B in ((5, 0), (5, 6), (0, 1), (2 ** 31, 4)):
        with pytest.raises(ValueError):
            R.sample(n, B, 0, 0)


@pytest.mark.parametrize("n,B,K", [(5, 3, 4000), (1000, 64, 16000)])
def test_uniformity(n, B, K):
    """Seed 12345, draws 0 .. K - 1 (deterministic).  Inclusion counts: every row is drawn K B / n times on average; without replacement
    within a draw the counts' variance is (1 - B / n) of the multinomial's, so the statistic is divided by that.  First index: index[0]
    is one uniform row per draw.  Both p-values (chi-square, n - 1 degrees of freedom) must be at least 1e-3."""
    from scipy.stats import chi2
    idx = R.sample(n, B, 12345, np.arange(K))
    inc, first = np.bincount(idx.ravel(), minlength=n), np.bincount(idx[:, 0], minlength=n)
    e = K * B / n
    p_inc = chi2.sf(((inc - e) ** 2 / e).sum() / (1.0 - B / n), n - 1)
    e = K / n
    p_first = chi2.sf(((first - e) ** 2 / e).sum(), n - 1)
    print(f"n={n} B={B} K={K}: p(inclusion)={p_inc:.3g} p(index[0])={p_first:.3g}")
    assert p_inc >= 1e-3 and p_first >= 1e-3


# ---------------------------------------------------------------- the append rule's restatement against ReplayBuffer.add (CPU tensors)
@pytest.mark.parametrize("dims,final", [(COUPLED, True), (DECOUPLED, True), (DECOUPLED, False)])
def test_append_restatement_is_add(dims, final):
    T, N, cap = 3, 65, 200
    s = fake_storage(*dims, T, N, final_obs=final, seed=3)
    buf = ReplayBuffer(cap, *dims, "cpu")
    for t in buf.obs + buf.obs_next + buf.act + buf.rwd + buf.done:
        t.fill_(-7.0)
    buf.count, buf.current_size = 190, 190
    ref = [{k: v.numpy().copy() for k, v in buf.tensors(a).items()} for a in range(buf.n_agents)]
    buf.add(s)
    nxt = R.append(ref, 190, [o.numpy() for o in s.obs], None if s.final_obs is None else [f.numpy() for f in s.final_obs], s.act_all.numpy(),
                   s.reward.numpy(), s.done.numpy(), s.truncated.numpy())
    assert nxt == buf.count == (190 + T * N) % cap and buf.current_size == cap
    for a in range(buf.n_agents):
        for name, got in buf.tensors(a).items():
            assert np.array_equal(got.numpy().view(np.uint32), ref[a][name].view(np.uint32)), (a, name)
    untouched = np.setdiff1d(np.arange(cap), (190 + np.arange(T * N)) % cap)
    assert untouched.size == 5 and (buf.obs[0][untouched] == -7.0).all()
    if final:   # the reset rows are dense and differ from obs[t + 1]
        m = s.reset_mask().reshape(-1).numpy()
        assert 0.3 < m.mean() < 0.9 and not np.array_equal(s.final_obs[0].numpy().reshape(T * N, -1)[m], s.obs[0][1:].numpy().reshape(T * N, -1)[m])


# ---------------------------------------------------------------- structs and the C entries' errors
def test_structs_mirror_the_header(tmp_path):
    names = ("QrReplayAdd", "QrReplaySample")
    lines = ['printf("abi %d\\n", QR_ABI_VERSION);']
    for sname in names:
        lines.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        lines += [f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));' for f, _ in getattr(L, sname)._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for sname in names:
        ct = getattr(L, sname)
        assert int(out[sname]) == C.sizeof(ct)
        for f, _ in ct._fields_:
            assert int(out[f"{sname}.{f}"]) == getattr(ct, f).offset, (sname, f)
    lib = L.load()
    assert {"qr_replay_add", "qr_replay_sample"} <= set(L.SYMBOLS) and hasattr(lib, "qr_replay_add") and hasattr(lib, "qr_replay_sample")
    assert int(out["abi"]) == L.ABI_VERSION == 16 and lib.qr_abi_version() == 16


NULL, SIZE, ALIGN = -1, -3, -4


def _fake_add(na=2):
    """A QrReplayAdd over made-up, aligned addresses that passes every check but for what a case changes: each case below fails one,
    so nothing is ever launched."""
    r = L.QrReplayAdd()
    p = iter(range(0x10000, 0x80000, 0x1000))
    for k in range(na):
        r.obs[k], r.final_obs[k] = next(p), next(p)
        r.buf_obs[k], r.buf_obs_next[k], r.buf_action[k], r.buf_reward[k], r.buf_done[k] = (next(p) for _ in range(5))
        r.obs_dim[k], r.action_dim[k], r.col_offset[k] = (15, 3)[k], (4, 1)[k], (0, 4)[k]
    r.action, r.reward, r.done, r.truncated = next(p), next(p), next(p), next(p)
    r.count, r.capacity, r.n_envs, r.n_steps, r.n_agents, r.action_row = 190, 200, 65, 3, na, 5
    return r


def _set(obj, name, value, k=None):
    if k is None:
        setattr(obj, name, value)
    else:
        getattr(obj, name)[k] = value


@pytest.mark.parametrize("name,value,k,want", [
    ("n_agents", 0, None, SIZE), ("n_agents", 3, None, SIZE), ("reserved0", 1, None, SIZE), ("capacity", 0, None, SIZE), ("n_steps", 0, None, SIZE),
    ("n_envs", 0, None, SIZE), ("capacity", 194, None, SIZE), ("count", 200, None, SIZE), ("count", -1, None, SIZE), ("obs_dim", 0, 1, SIZE),
    ("obs_dim", 4097, 0, SIZE), ("action_dim", 0, 0, SIZE), ("col_offset", 5, 1, SIZE), ("col_offset", -1, 0, SIZE), ("action_row", 4, None, SIZE),
    ("action", None, None, NULL), ("reward", None, None, NULL), ("done", None, None, NULL), ("obs", None, 1, NULL), ("buf_obs", None, 0, NULL),
    ("buf_obs_next", None, 1, NULL), ("buf_action", None, 0, NULL), ("buf_reward", None, 1, NULL), ("buf_done", None, 0, NULL),
    ("final_obs", None, 1, NULL), ("obs", 0x10002, 0, ALIGN), ("buf_done", 0x20001, 1, ALIGN), ("reward", 0x30002, None, ALIGN),
    ("state", 0x40004, None, ALIGN)])
def test_replay_add_errors(name, value, k, want):
    lib = L.load()
    r = _fake_add()
    if (name, value) == ("capacity", 194):
        r.count = 0
    _set(r, name, value, k)
    assert lib.qr_replay_add(C.byref(r), None) == want
    assert lib.qr_replay_add(None, None) == NULL


@pytest.mark.parametrize("name,value,want", [("batch", 0, SIZE), ("batch", 1001, SIZE), ("n", 2 ** 31, SIZE), ("index", None, NULL),
                                             ("index", 0x10004, ALIGN), ("state", 0x10004, ALIGN), ("status", 0x10002, ALIGN)])
def test_replay_sample_errors(name, value, want):
    lib = L.load()
    s = L.QrReplaySample(0x10000, 0x20000, 0x30000, 1000, 64, 5, 0)
    if name == "n":
        s.batch = 1
    setattr(s, name, value)
    assert lib.qr_replay_sample(C.byref(s), None) == want
    assert lib.qr_replay_sample(None, None) == NULL


# ---------------------------------------------------------------- the Python side's checks, all before a launch
def test_sample_index_checks():
    buf = ReplayBuffer(100, *COUPLED, "cpu", seed=2 ** 40)
    with pytest.raises(ValueError):
        buf.sample_index(1)                       # nothing stored yet
    buf.count = buf.current_size = 50
    for B in (0, -1, 51):
        with pytest.raises(ValueError):
            buf.sample_index(B)
    for out in (torch.zeros(8, dtype=torch.int32), torch.zeros(9, dtype=torch.int64), torch.zeros(8, 1, dtype=torch.int64),
                torch.zeros(16, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError):
            buf.sample_index(8, out=out)
    with pytest.raises(ValueError):                # another device than the buffer's
        buf.sample_index(8, out=torch.zeros(8, dtype=torch.int64, device="meta"))
    assert buf.draw == 0                           # a refused call draws nothing
    with pytest.raises(RuntimeError):              # all checks passed: there is no CPU kernel
        buf.sample_index(8, out=torch.zeros(8, dtype=torch.int64))
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            buf.seed(seed)
        with pytest.raises(ValueError):
            ReplayBuffer(10, *COUPLED, "cpu", seed=seed)
    out = torch.zeros(4, dtype=torch.int64)
    for args in ((2 ** 31, 4, 0, 0), (2 ** 31 + 5, 4, 0, 0), (10, 11, 0, 0), (10, 0, 0, 0), (10, 4, -1, 0), (10, 4, 0, 2 ** 64)):
        with pytest.raises(ValueError):
            replay_sample(*args, out)
    with pytest.raises(ValueError):
        replay_sample(10, 4, 0, 0, out, state=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        replay_sample(10, 4, 0, 0, out, state=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        replay_sample(10, 4, 0, 0, out, status=torch.zeros(1, dtype=torch.int64))


def test_append_checks():
    s = fake_storage(*DECOUPLED, 3, 65)
    with pytest.raises(ValueError):
        ReplayBuffer(194, *DECOUPLED, "cpu").append(s)                 # T * N > capacity
    with pytest.raises(ValueError):
        ReplayBuffer(200, *COUPLED, "cpu").append(s)                   # agent count
    with pytest.raises(ValueError):
        ReplayBuffer(200, (15, 4), (4, 1), "cpu").append(s)            # an observation width
    with pytest.raises(ValueError):
        ReplayBuffer(200, (15, 3), (3, 2), "cpu").append(s)            # an action width
    buf = ReplayBuffer(200, *DECOUPLED, "cpu")
    with pytest.raises(RuntimeError):                                   # all checks passed: there is no CPU kernel
        buf.append(s)
    assert (buf.count, buf.current_size) == (0, 0)
    t = [buf.tensors(k) for k in range(2)]
    good = dict(tensors=t, obs=s.obs, final_obs=s.final_obs, action=s.act_all, reward=s.reward, done=s.done, truncated=s.truncated, count=0)
    bad = [dict(tensors=t[:1]), dict(tensors=t + t[:1]), dict(obs=s.obs[:1]), dict(final_obs=s.final_obs[:1]), dict(count=200), dict(count=-1),
           dict(action=s.act_all[..., :4]), dict(action=s.act_all.double()), dict(reward=s.reward[..., 0]), dict(done=s.done.float()),
           dict(truncated=s.truncated[:2]), dict(obs=[s.obs[0][:3], s.obs[1]]), dict(final_obs=[s.final_obs[0], s.final_obs[1][..., :2]]),
           dict(tensors=[dict(t[0], rwd=t[0]["rwd"][:100]), t[1]]), dict(tensors=[dict(t[0], done=t[0]["done"].double()), t[1]]),
           dict(state=torch.zeros(3, dtype=torch.int32)), dict(state=torch.zeros(2, dtype=torch.int64))]
    for change in bad:
        with pytest.raises(ValueError):
            replay_add(**dict(good, **change))
    with pytest.raises(RuntimeError):
        replay_add(**good)


def test_device_state_follows_add():
    """use_device_state() on a buffer; `add` leaves the tensor equal to the host's ints (here on CPU tensors); a buffer that never
    opted in has no tensor and `add` does nothing new."""
    s = fake_storage(*COUPLED, 3, 65)
    buf = ReplayBuffer(200, *COUPLED, "cpu")
    buf.add(s)
    assert buf.state is None
    st = buf.use_device_state()
    assert st.dtype == torch.int64 and st.tolist() == [195, 195, 0] and buf.use_device_state() is st
    buf.add(s)
    assert st.tolist() == [buf.count, buf.current_size, buf.draw] == [190, 200, 0]
    st[2] = 9
    buf.pull_device_state()
    assert buf.draw == 9
    with pytest.raises(ValueError):
        ReplayBuffer(10, *COUPLED, "cpu").pull_device_state()
