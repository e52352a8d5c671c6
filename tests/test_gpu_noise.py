"""The library's noise source on the GPU (qr_noise_fill; noise_fill, DeviceNoise, the updaters' and the collector's
noise_source="device") against the NumPy restatement of tests/noise_ref.py: UNIFORM bit for bit, NORMAL under a derived bar; that a
value depends on (seed, draw, stream, element) alone; the device counter; the moments; and the updaters, their capture and the
collector's warm-up keyed as documented.  Every tensor filled here sits between sentinel words, which must survive."""
import copy

import numpy as np
import pytest
import torch

import noise_ref as NR
from test_gpu_offpolicy_update import FREQ, _buffer, _modules, _tensors, _updater

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD                                                  # a NaN pattern no draw produces
GUARD = 8                                                              # sentinel words on either side of a tensor
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4, 4, 7)
MISALIGNED = (5, 9)                                                    # the slots of 63 and 256 elements start one float past a 16-byte boundary
SEED, DRAW = 2 ** 40 + 3, 2 ** 33 + 5                                  # both high words in use

# The bar for a standard normal, absolute, at |z| <= R = 5.9 (u1 >= 2^-25 gives r <= sqrt(50 ln 2) = 5.887).  The device forms
# L = log(u1) as v_log_f32 times float32(ln 2), r = sqrtf(-2 L), (cs, sn) = sincos_small(angle) and z = r * cs in float32; the
# restatement takes the same float32 u1 and angle and does the rest in float64.  Relative to r, which bounds |z|:
#   the logarithm   v_log_f32 is accurate to 1 ulp (AMD Instinct CDNA3/CDNA4 ISA reference, V_LOG_F32), <= 2^-23 |L|; the constant
#                   float32(ln 2) is off by <= 2^-24 of itself and the product rounds by <= 2^-24 |L|: dL <= 2^-22 |L|.  The square root
#                   halves a relative error: dr <= 2^-23 r  (-2 L is exact)
#   sqrtf           correctly rounded (the compiler's default for HIP): <= 2^-24 r
#   sincos_small    ~1e-7 absolute (qr_rng.h), times r
#   the product     <= 2^-24 |z| <= 2^-24 r
# sum = r (2^-23 + 2^-24 + 1e-7 + 2^-24) = 3.38e-7 r <= 2.0e-6 at r = 5.9; with the factor 2 of margin: 4.0e-6.
R_MAX = 5.9
NORMAL_BAR = 2.0 * R_MAX * (2.0 ** -23 + 2.0 ** -24 + 1e-7 + 2.0 ** -24)


def normal_bar(a: float, b: float) -> float:
    """out = fmaf(b, z, a): the bar for z scaled by |b|, plus the fma's own rounding at the largest |out| — none where a = 0, b = 1,
    for which the fma is exact."""
    if (a, b) == (0.0, 1.0):
        return NORMAL_BAR
    return abs(b) * NORMAL_BAR + 2.0 ** -24 * (abs(a) + abs(b) * R_MAX)


def arena(counts, misaligned=()):
    """One int32-viewed float32 buffer of sentinel words and, carved from it, a contiguous float32 view per count — each at a 16-byte
    boundary (slot index in `misaligned`: one float past one) with at least GUARD sentinel words on either side.  Returns the whole
    buffer's int32 view, the views and the boolean mask of the words that belong to no view."""
    offs, at = [], GUARD
    for k, c in enumerate(counts):
        at = (at + 3) // 4 * 4 + (1 if k in misaligned else 0)
        offs.append(at)
        at += c + GUARD
    buf = torch.full((at + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    views = [buf.view(torch.float32)[o:o + c] for o, c in zip(offs, counts)]
    guard = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    for o, c in zip(offs, counts):
        guard[o:o + c] = False
    for k, v in enumerate(views):
        assert v.is_contiguous() and v.data_ptr() % 16 == (4 if k in misaligned else 0)
    return buf, views, guard


def sentinels_intact(buf, guard) -> bool:
    return bool((buf[guard] == SENTINEL).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def check_slot(t, kind, seed, draw, stream, a=0.0, b=1.0, label=""):
    """A filled tensor against the restatement; returns the NORMAL error (0.0 for UNIFORM, which must be equal)."""
    got = t.detach().cpu().numpy().reshape(-1)
    if kind == "uniform":
        want = NR.uniform(got.size, seed, draw, stream, a, b)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (label, "uniform differs from the restatement")
        return 0.0
    err = float(np.abs(got.astype(np.float64) - NR.normal(got.size, seed, draw, stream, a, b)).max())
    print(f"{label}: normal, {got.size} elements, a {a} b {b}: max err {err:.3e}, bar {normal_bar(a, b):.3e}")
    assert err <= normal_bar(a, b), (label, err, normal_bar(a, b))
    return err


def test_sixteen_slots_one_launch_against_the_restatement():
    """Every count of the walk in one launch, the kinds mixed, two misaligned views, some slots scaled and shifted."""
    from gym_rotor_amd import noise_fill
    buf, views, guard = arena(COUNTS, MISALIGNED)
    kinds = ["normal" if k % 3 != 1 else "uniform" for k in range(16)]
    a = [0.0] * 16
    b = [1.0] * 16
    a[8], b[8], a[9], b[9], a[11], b[11], a[12], b[12] = 0.25, 0.05, -1.5, 0.3, 0.0, 0.05, 2.0, -0.7   # slots 8, 11: normal; 9 normal, misaligned; 12: normal
    a[10], b[10], a[13], b[13] = 0.1, 0.3, -0.75, 2.5                                                    # slots 10, 13: uniform
    streams = [3 * k + 1 for k in range(16)]
    noise_fill(views, seed=SEED, draw=DRAW, streams=streams, kind=kinds, a=a, b=b)
    torch.cuda.synchronize()
    assert sentinels_intact(buf, guard)
    assert {kinds[k] for k in MISALIGNED} == {"normal"} and kinds[10] == kinds[13] == kinds[4] == "uniform"
    worst = max(check_slot(views[k], kinds[k], SEED, DRAW, streams[k], a[k], b[k], f"slot {k} ({COUNTS[k]})") for k in range(16))
    print(f"worst normal error over the sixteen slots: {worst:.3e}")
    # the same launch with the misaligned pair uniform: the element-by-element path bit for bit
    buf2, views2, guard2 = arena(COUNTS, MISALIGNED)
    noise_fill(views2, seed=SEED, draw=DRAW, streams=streams, kind=["uniform"] * 16, a=a, b=b)
    torch.cuda.synchronize()
    assert sentinels_intact(buf2, guard2)
    for k in range(16):
        check_slot(views2[k], "uniform", SEED, DRAW, streams[k], a[k], b[k])


@pytest.mark.parametrize("count", [1, 6, 2 ** 20 + 3])
def test_one_slot_and_the_grid_stride_path(count):
    """n_slots = 1; 2^20 + 3 elements are 262 145 quads, one more than the grid's 1024 x 256 threads: the loop's second trip.  The
    moments of the device's normals under the bounds tests/test_noise_host.py derives for the restatement's."""
    from gym_rotor_amd import noise_fill
    buf, (zn, zu), guard = arena((count, count), (1,))
    noise_fill([zn], seed=7, draw=11, streams=[5])
    noise_fill([zu], seed=7, draw=11, streams=[5], kind="uniform")
    torch.cuda.synchronize()
    assert sentinels_intact(buf, guard)
    err = check_slot(zn, "normal", 7, 11, 5, label=f"one slot of {count}")
    check_slot(zu, "uniform", 7, 11, 5)
    if count > 1000:
        n = count
        z = zn.double()
        mean, var = float(z.mean()), float(z.var(unbiased=False))
        print(f"device normals: mean {mean:.3e} (bound {5 / np.sqrt(n):.3e}), var - 1 {var - 1:.3e} (bound {5 * np.sqrt(2 / n):.3e}), worst error {err:.3e}")
        assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1.0) <= 5 * np.sqrt(2.0 / n) and float(z.abs().max()) <= R_MAX


@pytest.mark.parametrize("kind", ["normal", "uniform"])
def test_a_value_depends_on_its_key_alone(kind):
    """(seed, draw, stream) = (SEED, DRAW, 9) with 257 elements: alone; as the last of sixteen slots; as the first among others; through a
    misaligned view; as the seventeenth tensor of a call (the split's second launch); through the torch op — the same bits."""
    from gym_rotor_amd import noise_fill
    n, key = 257, dict(seed=SEED, draw=DRAW)
    buf, v, guard = arena((n, n, n, n, n, 33, 65) + (9,) * 14 + (n,) + (5,) * 16, (3,))
    alone, last, first, mis, op, o1, o2 = v[0], v[1], v[2], v[3], v[4], v[5], v[6]
    small, seventeenth, rest = v[7:21], v[21], v[22:38]
    noise_fill([alone], streams=[9], kind=kind, a=0.5, b=0.25, **key)
    others = list(range(100, 115))
    noise_fill(list(small) + [o1, last], streams=others + [9], kind=["uniform"] * 8 + ["normal"] * 7 + [kind], a=[0.0] * 15 + [0.5], b=[1.0] * 15 + [0.25], **key)
    noise_fill([first, o2], streams=[9, 200], kind=[kind, "normal"], a=[0.5, 0.0], b=[0.25, 1.0], **key)
    noise_fill([mis], streams=[9], kind=kind, a=0.5, b=0.25, **key)
    noise_fill(list(rest) + [seventeenth], streams=list(range(300, 316)) + [9], kind=["normal"] * 16 + [kind], a=[0.0] * 16 + [0.5], b=[1.0] * 16 + [0.25], **key)
    torch.ops.gym_rotor_amd.qr_noise_fill([o1, op], [0, NR.NORMAL if kind == "normal" else NR.UNIFORM], [0.0, 0.5], [1.0, 0.25], [100, 9], SEED, DRAW, None)
    torch.cuda.synchronize()
    assert sentinels_intact(buf, guard)
    for name, t in (("last of sixteen", last), ("first of two", first), ("misaligned", mis), ("seventeenth", seventeenth), ("torch op", op)):
        assert torch.equal(bits(t), bits(alone)), name
    check_slot(alone, kind, SEED, DRAW, 9, 0.5, 0.25, "alone")
    assert not torch.equal(bits(rest[0]), bits(rest[1]))        # the split's first launch ran, each tensor on its own stream


def test_the_device_counter():
    from gym_rotor_amd import DeviceNoise, noise_fill
    n = 130
    buf, v, guard = arena((n,) * 8)
    state = torch.tensor([3, 4, DRAW], dtype=torch.int64, device="cuda")
    noise_fill([v[0]], seed=SEED, draw=DRAW, streams=[2])
    noise_fill([v[1]], seed=SEED, draw=0, streams=[2], draw_dev=state[2:3])
    noise_fill([v[2]], seed=SEED, draw=DRAW + 1, streams=[2])
    noise_fill([v[3]], seed=SEED, draw=DRAW + 2 ** 32, streams=[2])
    noise_fill([v[4]], seed=SEED, draw=DRAW, streams=[3])
    noise_fill([v[5]], seed=SEED + 2 ** 32, draw=DRAW, streams=[2])
    src = DeviceNoise(SEED, "cuda").bind(state[2:3])
    src.fill([v[6]], streams=[2])
    state[2] += 1
    src.fill([v[7]], streams=[2])
    torch.cuda.synchronize()
    assert sentinels_intact(buf, guard) and state.tolist() == [3, 4, DRAW + 1] and src.draw == 2
    assert torch.equal(bits(v[1]), bits(v[0])) and torch.equal(bits(v[6]), bits(v[0])) and torch.equal(bits(v[7]), bits(v[2]))
    for k in (2, 3, 4, 5):
        assert not torch.equal(bits(v[k]), bits(v[0])), k
    host = DeviceNoise(SEED, "cuda")
    host.draw = DRAW
    a, b = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    host.fill([a], streams=[2])
    host.fill([b], streams=[2])
    assert host.draw == DRAW + 2 and torch.equal(bits(a), bits(v[0])) and torch.equal(bits(b), bits(v[2]))


def _by_hand(up, k, draw, seed):
    """Agent k's noise tensors filled by hand with the documented key: one tensor per call."""
    from gym_rotor_amd import noise_fill
    from gym_rotor_amd.offpolicy import NOISE_NAMES
    out = {}
    for name, t in up.noise[k].items():
        xs = []
        for j, x in enumerate(t if isinstance(t, tuple) else (t,)):
            y = torch.empty_like(x)
            noise_fill([y], seed=seed, draw=draw, streams=[(k << 8) | (NOISE_NAMES.index(name) << 2) | j], b=0.05 if name == "reg" else 1.0)
            xs.append(y)
        out[name] = tuple(xs) if isinstance(t, tuple) else xs[0]
    return out


@pytest.mark.parametrize("algo,mode", [("td3", "single"), ("sac", "ctde")])
def test_updater_draws_the_documented_stream(algo, mode):
    """update(buffer, 1) with the device source: noise[k] is noise_fill by hand under (noise_seed, the draw number sample_index left:
    k + 1, the stream id of the name), and the iteration equals a twin's that was handed those values (refill_noise=False)."""
    seed = 2 ** 50 + 9
    mods = _modules(algo, mode)
    twin_mods = copy.deepcopy(mods)
    up, buf = _updater(algo, mode, mods, noise_source="device", noise_seed=seed), _buffer(mode)
    up.policy_update_freq = 1
    up.update(buf, 1)
    n = up.n_agents
    assert buf.draw == n
    want = [_by_hand(up, k, k + 1, seed) for k in range(n)]
    flat = lambda d: [x for t in d.values() for x in (t if isinstance(t, tuple) else (t,))]
    for k in range(n):
        assert list(up.noise[k]) == list(want[k])
        for x, y in zip(flat(up.noise[k]), flat(want[k])):
            assert torch.equal(bits(x), bits(y)), (k, x.shape)
    twin, tbuf = _updater(algo, mode, twin_mods, refill_noise=False), _buffer(mode)
    twin.policy_update_freq = 1
    twin._prepare(tbuf)
    for k in range(n):
        for x, y in zip(flat(twin.noise[k]), flat(want[k])):
            x.copy_(y)
    twin.update(tbuf, 1)
    torch.cuda.synchronize()
    for j, (x, y) in enumerate(zip(_tensors(up), _tensors(twin))):
        assert torch.equal(x, y), j
    assert all(torch.equal(a, b) for a, b in zip(up.index, twin.index))


@pytest.mark.parametrize("algo", ["td3", "sac"])
def test_capture_draws_what_eager_iterations_draw(algo):
    """Three replays (device counters, the draw number read on the device) against an eager twin whose buffer keeps its counters on
    the host (the draw number passed by value): the same noise for the same minibatch number, so the same bits everywhere."""
    ups, bufs = [], []
    for dev_state in (True, False):
        up, buf = _updater(algo, "single", _modules(algo, "single"), noise_source="device", noise_seed=123), _buffer("single")
        if dev_state:
            buf.use_device_state()
        up.update(buf, FREQ)
        ups.append(up); bufs.append(buf)
    (a, b), (buf_a, buf_b) = ups, bufs
    replay = a.capture(buf_a)
    seen, mem = [[torch.empty_like(x) for x in a.noise[0].values()] for _ in range(3)], []
    for r in range(3):
        replay()
        for dst, src in zip(seen[r], a.noise[0].values()):
            dst.copy_(src)
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
    b.update(buf_b, 3 * FREQ)
    torch.cuda.synchronize()
    for j, (x, y) in enumerate(zip(_tensors(a), _tensors(b))):
        assert torch.equal(x, y), j
    for x, y in zip(a.noise[0].values(), b.noise[0].values()):
        assert torch.equal(bits(x), bits(y))
    assert all(not torch.equal(x, y) for x, y in zip(seen[0], seen[1])) and all(not torch.equal(x, y) for x, y in zip(seen[1], seen[2]))
    assert mem[0] == mem[1] == mem[2], mem                            # a replay allocates nothing
    buf_a.pull_device_state()
    assert buf_a.draw == buf_b.draw == 4 * FREQ and torch.equal(a.index[0], b.index[0])


def test_collector_warm_up_is_the_uniform_stream():
    from gym_rotor_amd import OffPolicyCollector, QuadVecEnv, ReplayBuffer, random_actors
    from gym_rotor_amd.offpolicy import COLLECTOR_STREAM
    n, t, seed = 128, 3, 2 ** 45 + 1
    env = QuadVecEnv("decoupled", n, device="cuda", obs_rows=True, auto_reset=True, max_episode_steps=2, seed=6)
    env.reset("train")
    env.get_norm_error_state()
    buf = ReplayBuffer(5000, env.obs_dims, [4, 1], "cuda")
    col = OffPolicyCollector(env, buf, horizon=t, start_timesteps=2 * t, algo="td3", noise_source="device", noise_seed=seed)
    actors = random_actors("decoupled", "cuda", torch.Generator(device="cuda").manual_seed(1), log_std=-9.0)
    for call in range(2):
        col.collect(actors)
        torch.cuda.synchronize()
        got = col.random_actions.cpu().numpy()
        want = NR.uniform(got.size, seed, call * t, COLLECTOR_STREAM).reshape(got.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), call
        assert np.abs(got).max() < 1.0
        rows = slice(call * t * n, (call + 1) * t * n)
        assert np.array_equal(buf.act[0][rows].cpu().numpy(), got.reshape(t * n, 5)[:, :4]) and np.array_equal(buf.act[1][rows].cpu().numpy(), got.reshape(t * n, 5)[:, 4:])
    assert col.total_timesteps == 2 * t
