"""The library's noise source (qr_noise_fill; gym_rotor_amd.noise_fill, DeviceNoise, the updaters' and the collector's
noise_source="device") without a GPU: the two structs' layout, every error code of the C entry, every ValueError of the Python side —
each before a launch — the stream numbering, and the NumPy restatement of tests/noise_ref.py: its Philox words against
tests/replay_ref.py, its single-rounding fma, and the moments of its normals."""
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
import noise_ref as NR  # noqa: E402
import replay_ref as RR  # noqa: E402

from gym_rotor_amd import DeviceNoise, _lib as L, noise_fill  # noqa: E402
from gym_rotor_amd import offpolicy as OP  # noqa: E402

NULL, SIZE, ALIGN = -1, -3, -4


# ---------------------------------------------------------------- structs and the C entry's errors
def test_structs_mirror_the_header(tmp_path):
    names = ("QrNoiseSlot", "QrNoiseFill")
    lines = ['printf("abi %d\\n", QR_ABI_VERSION);', 'printf("slots %d %d %d\\n", QR_NOISE_MAX_SLOTS, QR_NOISE_NORMAL, QR_NOISE_UNIFORM);']
    for sname in names:
        lines.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        lines += [f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));' for f, _ in getattr(L, sname)._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split(None, 1) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for sname in names:
        ct = getattr(L, sname)
        assert int(out[sname]) == C.sizeof(ct)
        for f, _ in ct._fields_:
            assert int(out[f"{sname}.{f}"]) == getattr(ct, f).offset, (sname, f)
    assert out["slots"].split() == [str(L.NOISE_MAX_SLOTS), str(L.NOISE_NORMAL), str(L.NOISE_UNIFORM)] == ["16", "0", "1"]
    lib = L.load()
    assert "qr_noise_fill" in L.SYMBOLS and hasattr(lib, "qr_noise_fill")
    assert int(out["abi"]) == L.ABI_VERSION == 16 and lib.qr_abi_version() == 16


def _fake_fill(n=3):
    """A QrNoiseFill over made-up, aligned addresses that passes every check: each case below breaks one, so nothing is launched."""
    f = L.QrNoiseFill()
    f.n_slots, f.seed, f.draw_dev, f.draw = n, 5, None, 7
    for k in range(n):
        s = f.slot[k]
        s.out, s.count, s.a, s.b, s.kind, s.stream = 0x10000 + 0x1000 * k, 10 + k, 0.0, 1.0, k % 2, k
    return f


@pytest.mark.parametrize("where,name,value,want", [
    ("fill", "n_slots", 0, SIZE), ("fill", "n_slots", 17, SIZE), ("fill", "n_slots", -1, SIZE), ("fill", "draw", -1, SIZE),
    ("slot", "count", 0, SIZE), ("slot", "count", -4, SIZE), ("slot", "count", 2 ** 33, SIZE), ("slot", "kind", 2, SIZE),
    ("slot", "stream", 2 ** 30, SIZE), ("slot", "a", float("nan"), SIZE), ("slot", "a", float("inf"), SIZE), ("slot", "b", float("-inf"), SIZE),
    ("slot", "b", float("nan"), SIZE), ("slot", "out", None, NULL), ("slot", "out", 0x10002, ALIGN), ("slot", "out", 0x10001, ALIGN),
    ("fill", "draw_dev", 0x20004, ALIGN)])
def test_noise_fill_errors(where, name, value, want):
    lib = L.load()
    for k in ((0, 2) if where == "slot" else (0,)):   # the first slot and the last one in use
        f = _fake_fill()
        setattr(f.slot[k] if where == "slot" else f, name, value)
        assert lib.qr_noise_fill(C.byref(f), None) == want
    assert lib.qr_noise_fill(None, None) == NULL


def test_draw_is_not_checked_with_a_device_counter_and_unused_slots_are_not_read():
    """A negative `draw` is refused only where it is used; slots behind n_slots may hold anything.  Both calls fail a later check,
    so nothing is launched."""
    lib = L.load()
    f = _fake_fill()
    f.draw, f.draw_dev = -1, 0x20004
    assert lib.qr_noise_fill(C.byref(f), None) == ALIGN      # past the SIZE checks
    f = _fake_fill()
    f.slot[3].count, f.slot[3].kind, f.slot[0].out = -1, 9, 0x10002
    assert lib.qr_noise_fill(C.byref(f), None) == ALIGN


# ---------------------------------------------------------------- the Python side's checks, all before a launch
def test_noise_fill_checks():
    t = [torch.zeros(8), torch.zeros(3, 4)]
    good = dict(seed=1, draw=0, streams=[0, 1])
    bad = [dict(streams=[0]), dict(streams=[0, 0]), dict(streams=[0, 2 ** 30]), dict(streams=[-1, 0]), dict(seed=-1), dict(seed=2 ** 64),
           dict(draw=-1), dict(draw=2 ** 63), dict(kind="gauss"), dict(kind=["normal"]), dict(a=[0.0]), dict(a=float("nan")), dict(b=float("inf")),
           dict(b=[1.0, 1e39]), dict(draw_dev=torch.zeros(1, dtype=torch.int32)), dict(draw_dev=torch.zeros(2, dtype=torch.int64)),
           dict(draw_dev=torch.zeros(1, dtype=torch.int64, device="meta"))]
    for change in bad:
        with pytest.raises(ValueError):
            noise_fill(t, **dict(good, **change))
    for tensors in ([], [torch.zeros(8), torch.zeros(8, dtype=torch.float64)], [torch.zeros(8), torch.zeros(4, 4)[:, :2]], [torch.zeros(8), torch.zeros(0)],
                    [torch.zeros(8), torch.zeros(8, device="meta")], [torch.zeros(8), None]):
        with pytest.raises(ValueError):
            noise_fill(tensors, seed=1, draw=0, streams=list(range(len(tensors))))
    with pytest.raises(RuntimeError):              # all checks passed: there is no CPU kernel
        noise_fill(t, **good)
    with pytest.raises(RuntimeError):
        noise_fill(t, **dict(good, draw=-5, draw_dev=torch.zeros(1, dtype=torch.int64)))   # draw is not read with a device counter
    assert all(bool((x == 0).all()) for x in t)
    with pytest.raises((ValueError, RuntimeError)):
        torch.ops.gym_rotor_amd.qr_noise_fill(t, [0, 2], [0.0, 0.0], [1.0, 1.0], [0, 1], 1, 0, None)


def test_device_noise_checks():
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            DeviceNoise(seed, "cpu")
    n = DeviceNoise(2 ** 64 - 1, "cpu")
    assert (n.seed, n.draw, n.draw_dev) == (2 ** 64 - 1, 0, None)
    for counter in (torch.zeros(1, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), torch.zeros(1, dtype=torch.int64, device="meta"), 3):
        with pytest.raises(ValueError):
            n.bind(counter)
    c = torch.zeros(3, dtype=torch.int64)
    assert n.bind(c[2:3]).draw_dev.data_ptr() == c.data_ptr() + 16 and n.bind(None).draw_dev is None
    with pytest.raises(ValueError):
        n.fill([torch.zeros(4, device="meta")])
    with pytest.raises(ValueError):
        n.fill([torch.zeros(4), torch.zeros(4)], streams=[3, 3])
    with pytest.raises(RuntimeError):
        n.fill([torch.zeros(4)])
    assert n.draw == 0                              # a refused call draws nothing


def test_updater_and_collector_noise_arguments():
    from test_sac_critic_host import _SacActor
    from test_td3_critic_host import _Actor, _Twin
    from gym_rotor_amd import OffPolicyCollector, ReplayBuffer, SacUpdater, Td3Updater
    a, c, at, ct, sa = _Actor(23, 16, 4), _Twin(27, 5), _Actor(23, 16, 4), _Twin(27, 5), _SacActor(23, 16, 4)
    nominal = [torch.zeros(4)]
    make = (lambda **kw: Td3Updater([a], [c], [at], [ct], nominal=nominal, **kw), lambda **kw: SacUpdater([sa], [c], [ct], nominal=nominal, **kw))
    for mk in make:
        up = mk()
        assert (up.noise_source, up.noise_seed) == ("torch", 0)
        up = mk(noise_source="device", noise_seed=2 ** 64 - 1)
        assert (up.noise_source, up.noise_seed) == ("device", 2 ** 64 - 1)
        for bad in (dict(noise_source="philox"), dict(noise_source="device", generator=torch.Generator()), dict(noise_source="device", noise_seed=-1),
                    dict(noise_seed=2 ** 64)):
            with pytest.raises(ValueError):
                mk(**bad)
    env = types.SimpleNamespace(auto_reset=True, n_agents=1, obs_dims=[23], action_dim=4, num_envs=4, x_lim=3.0, device=torch.device("cpu"))
    buf = ReplayBuffer(64, [23], [4], "cpu")
    for bad in (dict(noise_source="philox"), dict(noise_source="device", generator=torch.Generator()), dict(noise_source="device", noise_seed=-1)):
        with pytest.raises(ValueError):   # refused before the env is touched (the first checks)
            OffPolicyCollector(env, buf, 2, start_timesteps=4, **bad)


def test_stream_numbering_is_injective():
    ids = [OP.noise_stream(k, name, j) for k in (0, 1) for name in OP.NOISE_NAMES for j in (0, 1)]
    assert len(set(ids)) == len(ids) == 2 * len(OP.NOISE_NAMES) * 2 and 0 <= min(ids) and max(ids) < 2 ** 30
    assert OP.noise_stream(1, "reg", 0) == (1 << 8) | (OP.NOISE_NAMES.index("reg") << 2) and OP.noise_stream(0, "smooth", 1) == 1
    assert len(OP.NOISE_NAMES) << 2 <= 1 << 8       # the name's field does not reach the agent's
    assert max(ids) < OP.COLLECTOR_STREAM < 2 ** 30 # the collector's warm-up stream is no updater tensor's
    # SAC ctde, the most an agent fills in one launch: nine names, "next" a pair
    ctde = OP.SacUpdater._noise_shapes(types.SimpleNamespace(mode="ctde"), 0, 8, [15, 3], [4, 1])
    assert sum(len(s) if isinstance(s, list) else 1 for s in ctde.values()) == 10
    # every name a _noise_shapes returns is listed
    shapes = {}
    for cls in (OP.Td3Updater, OP.SacUpdater):
        for mode in OP.MODES:
            shapes.update(cls._noise_shapes(types.SimpleNamespace(mode=mode), 0, 8, [15, 3], [4, 1]))
    assert set(shapes) == set(OP.NOISE_NAMES)


# ---------------------------------------------------------------- the restatement
def test_philox_words_against_replay_ref():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, (4, 4096), dtype=np.uint64)
    for seed in (0, 12345, 2 ** 63 + 11):
        w = NR.philox4(c[0], c[1], c[2], c[3], seed)
        assert w.shape == (4, 4096) and int(w.max()) < 2 ** 32
        assert np.array_equal(w[0], RR.philox_word0(c[0], c[1], c[2], c[3], seed))
    # the known-answer vector of Random123 (philox4x32-10, counter and key all ones)
    w = NR.philox4(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF)
    assert [int(x) for x in w] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_stream_keys():
    base = NR.words(64, 5, 9, 3)
    assert base.shape == (16, 4) and np.array_equal(base, NR.words(61, 5, 9, 3)) and np.array_equal(base[4:], NR.words(48, 5, 9, 3, first_quad=4))
    for seed, draw, stream in ((6, 9, 3), (5 + 2 ** 32, 9, 3), (5, 10, 3), (5, 9 + 2 ** 32, 3), (5, 9, 4), (5, 9, 3 + 2 ** 29)):
        assert not np.array_equal(base, NR.words(64, seed, draw, stream)), (seed, draw, stream)
    # normal4's counter layout with gid = q, step = draw, block = 0x40000000 | stream
    q, draw = 2 ** 32 + 7, 2 ** 33 + 5
    w = NR.words(4, 11, draw, 3, first_quad=q)[0]
    assert np.array_equal(w, NR.philox4(q & 0xFFFFFFFF, (q >> 32) ^ (draw >> 32), draw & 0xFFFFFFFF, 0x80000000 | 0x40000000 | 3, 11))
    for bad in ((1, -1, 0, 0), (1, 0, 2 ** 64, 0), (1, 0, 0, 2 ** 30), (0, 0, 0, 0)):
        with pytest.raises(ValueError):
            NR.words(*bad)


def test_fma32_rounds_once():
    from fractions import Fraction
    rng = np.random.default_rng(1)
    b = rng.standard_normal(20000).astype(np.float32)
    x = NR.sym(rng.integers(0, 2 ** 32, 20000, dtype=np.uint64))
    a = (rng.standard_normal(20000) * np.float32(2.0) ** rng.integers(-30, 3, 20000)).astype(np.float32)
    got = NR.fma32(b, x, a)
    twice = (b.astype(np.float64) * x.astype(np.float64) + a.astype(np.float64)).astype(np.float32)   # two roundings
    differ = np.nonzero(got != twice)[0]
    for i in list(differ[:50]) + list(range(200)):
        exact = Fraction(float(b[i])) * Fraction(float(x[i])) + Fraction(float(a[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        d = abs(exact - Fraction(float(got[i])))
        assert d <= abs(exact - Fraction(float(lo))) and d <= abs(exact - Fraction(float(hi))), i
    s = NR.sym(np.array([0, 0xFF, 0x100, 2 ** 32 - 1], dtype=np.uint64))
    assert s.tolist() == [2.0 ** -24 - 1.0, 2.0 ** -24 - 1.0, 3 * 2.0 ** -24 - 1.0, 1.0 - 2.0 ** -24] and s.dtype == np.float32
    assert np.array_equal(NR.uniform(7, 1, 2, 3), NR.sym(NR.words(7, 1, 2, 3)).reshape(-1)[:7])   # a = 0, b = 1: the words' values themselves


def test_normal_moments_and_the_exact_zero():
    """2^20 draws of one stream.  The sample mean of n unit normals has standard deviation 1 / sqrt(n) and the sample variance
    sqrt(2 / n) (the fourth central moment of a unit normal is 3), so five standard deviations are 5 / sqrt(n) and 5 sqrt(2 / n): a
    correct stream misses either with probability 6e-7, and the truncation of the tails at |z| = 5.9 (u1 >= 2^-25) moves the
    variance by 1e-6 of that bound.  u1 rounds to 1 exactly where its word's top 24 bits are all ones: log gives 0 and the pair is
    (0, 0) whatever the angle."""
    n = 2 ** 20
    z = NR.normal(n, 2024, 3, 17)
    assert z.shape == (n,) and z.dtype == np.float64 and np.abs(z).max() <= 5.9
    mean, var = z.mean(), z.var()
    print(f"mean {mean:.3e} (bound {5 / np.sqrt(n):.3e}), var - 1 {var - 1:.3e} (bound {5 * np.sqrt(2 / n):.3e})")
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1.0) <= 5 * np.sqrt(2.0 / n)
    u = NR.uniform(n, 2024, 3, 18).astype(np.float64)
    assert abs(u.mean()) <= 5 * np.sqrt(1 / 3 / n) and abs(u.var() - 1 / 3) <= 5 * np.sqrt(4 / 45 / n) and np.abs(u).max() < 1.0
    w = np.array([[0xFFFFFF00, 123456789, 0xFFFFFFFF, 0x80000000], [0xFFFFFE00, 5, 0xFFFFFEFF, 77]], dtype=np.uint64)
    assert NR.u01(w[:, 0]).tolist() == [1.0, 1.0 - 2.0 ** -23]   # 1 - 2^-25 and 1 - 3 * 2^-25: both ties, to the even neighbour
    zz = NR.normals_from_words(w)
    assert (zz[0] == 0.0).all() and (zz[1] != 0.0).all()
    one = NR.u01(NR.words(n, 2024, 3, 17)[:, ::2]) == 1.0     # where u1 rounds to 1 in the sample itself (rare: 2^-24 per pair)
    assert np.array_equal(z.reshape(-1, 2)[one.reshape(-1)] == 0.0, np.ones((int(one.sum()), 2), dtype=bool))
    assert np.array_equal((z.reshape(-1, 2) == 0.0).all(-1), one.reshape(-1))
