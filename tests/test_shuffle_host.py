"""The keyed permutation (qr_shuffle; gym_rotor_amd.shuffle, ppo_stream) without a GPU: the NumPy restatement of tests/shuffle_ref.py — a
bijection at every size, slices, and its uniformity against numpy's own shuffle — the struct's layout, every error code of the C entry
and every ValueError of the Python side, each before a launch, and the stream numbering."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_ref as NR  # noqa: E402
import shuffle_ref as SR  # noqa: E402

from gym_rotor_amd import _lib as L, ppo_stream, shuffle  # noqa: E402
from gym_rotor_amd import es as ES, offpolicy as OP  # noqa: E402
from gym_rotor_amd.shuffle import PPO_STREAM_NAMES  # noqa: E402  (the package's `shuffle` is the function, not the module)

NULL, SIZE, ALIGN = -1, -3, -4
# three keys: a plain one, a seed with high bits and a draw beyond 32 bits, the updater's own stream of agent 1
KEYS = ((5, 9, 3), (2 ** 63 + 2 ** 40 + 3, 2 ** 32 + 1, 77), (12345, 6, (3 << 27) | (1 << 8)))


# ---------------------------------------------------------------- the restatement
def test_the_restatement_is_a_bijection_at_every_size():
    for n in list(range(1, 4101)) + [65535, 65536, 65537, 2 ** 20 + 1]:
        want = np.arange(n)
        for seed, draw, stream in KEYS:
            p = SR.shuffle_ref(n, seed, draw, stream)
            assert p.dtype == np.int64 and p.shape == (n,) and np.array_equal(np.sort(p), want), (n, seed, draw, stream)
    assert SR.shuffle_ref(1, 1, 2, 3).tolist() == [0]


def test_half_bits_and_keys():
    for n, w in ((1, 1), (2, 1), (4, 1), (5, 2), (16, 2), (17, 3), (210, 4), (256, 4), (257, 5), (65536, 8), (65537, 9), (2 ** 30 + 1, 16), (2 ** 32 - 1, 16)):
        assert SR.half_bits(n) == w and (n == 1 or n <= 4 ** w < 4 * n)
    for bad in (0, 2 ** 32):
        with pytest.raises(ValueError):
            SR.half_bits(bad)
    seed, draw, stream = KEYS[1]
    k = SR.keys(seed, draw, stream)
    assert k.shape == (8,) == (SR.ROUNDS,) and np.array_equal(k, NR.words(8, seed, draw, stream).reshape(-1))
    # quad k's counter: (k, draw_hi, draw_lo, 0xC0000000 | stream) under the seed
    assert np.array_equal(k[4:], NR.philox4(1, draw >> 32, draw & 0xFFFFFFFF, 0xC0000000 | stream, seed))
    assert (SR.ROUNDS, SR.MIX_M1, SR.MIX_M2) == (L.SHUFFLE_ROUNDS, L.SHUFFLE_MIX_M1, L.SHUFFLE_MIX_M2)
    assert int(SR.mix32(0)) == 0 and int(SR.mix32(1)) != 1 and len(set(SR.mix32(np.arange(4096)).tolist())) == 4096   # a bijection of the words


@pytest.mark.parametrize("n", [17, 210, 4097, 65537])
def test_a_slice_is_the_same_positions_of_the_whole(n):
    seed, draw, stream = KEYS[1]
    whole = SR.shuffle_ref(n, seed, draw, stream)
    for first, count in ((0, 1), (1, 7), (n // 3, n // 2 - 1), (n - 5, 5), (n, 0), (3, 0)):
        assert np.array_equal(SR.shuffle_ref(n, seed, draw, stream, first, count), whole[first:first + count])
    for key in ((seed + 1, draw, stream), (seed, draw + 1, stream), (seed, draw, stream + 1), (seed, draw + 2 ** 32, stream)):
        assert not np.array_equal(SR.shuffle_ref(n, *key), whole), key
    with pytest.raises(ValueError):
        SR.shuffle_ref(n, seed, draw, stream, n - 1, 2)


UNIFORMITY_KEY = (2 ** 40 + 3, (3 << 27) | 1)   # seed, stream; the draws are 0 .. 4095
DRAWS, RUNS = 4096, 200


@pytest.mark.parametrize("n", [2, 3, 5, 8, 17, 210])
def test_uniformity_against_numpy_permutations(n):
    """4096 consecutive draws of one stream: the chi-square statistic of the n x n table "element e at position p" against 4096 / n,
    and for n = 210 the number of pairs (i, i + 1) that stay adjacent and in order.  The bar of each is the largest value of the same
    statistic over 200 independently seeded numpy.random.Generator.permutation runs of the same size, computed here; the restatement
    must not exceed it.  (Measured with ROUNDS = 8: chi-square 2.13 / 3.71 / 33.38 / 80.62 / 274.45 / 44061.45 under bars of 20.72 /
    32.97 / 44.22 / 90.96 / 331.07 / 44705.49, and 4108 kept neighbours under a bar of 4285.)"""
    seed, stream = UNIFORMITY_KEY
    perms = np.stack([SR.shuffle_ref(n, seed, d, stream) for d in range(DRAWS)])
    chi, kept = SR.position_chi2(perms, n), SR.neighbours_kept(perms)
    bar_chi, bar_kept = 0.0, 0
    for run in range(RUNS):
        rng = np.random.default_rng(run)
        ref = np.stack([rng.permutation(n) for _ in range(DRAWS)])
        bar_chi, bar_kept = max(bar_chi, SR.position_chi2(ref, n)), max(bar_kept, SR.neighbours_kept(ref))
    print(f"n = {n}: chi-square {chi:.2f} (bar {bar_chi:.2f}), neighbours kept {kept} (bar {bar_kept})")
    assert chi <= bar_chi
    if n == 210:
        assert kept <= bar_kept


def test_the_statistics_see_a_structured_family():
    """What the two statistics are for: rotations of the identity fill the position table evenly and keep nearly every neighbour;
    a family that fixes element 0 keeps no more neighbours than chance and ruins the table."""
    n = 210
    rng = np.random.default_rng(0)
    rot = (np.arange(n)[None, :] + rng.integers(0, n, DRAWS)[:, None]) % n
    assert SR.neighbours_kept(rot) >= DRAWS * (n - 2)
    fixed = np.stack([np.concatenate([[0], 1 + rng.permutation(n - 1)]) for _ in range(DRAWS)])
    assert SR.position_chi2(fixed, n) > 10 * n * n


# ---------------------------------------------------------------- the struct and the C entry's errors
def test_struct_mirrors_the_header(tmp_path):
    lines = ['printf("abi %d\\n", QR_ABI_VERSION);', 'printf("consts %d %u %u\\n", QR_SHUFFLE_ROUNDS, QR_SHUFFLE_MIX_M1, QR_SHUFFLE_MIX_M2);',
             'printf("QrShuffle %zu\\n", sizeof(QrShuffle));']
    lines += [f'printf("QrShuffle.{f} %zu\\n", offsetof(QrShuffle, {f}));' for f, _ in L.QrShuffle._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split(None, 1) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["QrShuffle"]) == C.sizeof(L.QrShuffle)
    for f, _ in L.QrShuffle._fields_:
        assert int(out[f"QrShuffle.{f}"]) == getattr(L.QrShuffle, f).offset, f
    assert out["consts"].split() == [str(L.SHUFFLE_ROUNDS), str(L.SHUFFLE_MIX_M1), str(L.SHUFFLE_MIX_M2)]
    lib = L.load()
    assert {"qr_shuffle", "qr_ppo_actor_grad_dev"} <= set(L.SYMBOLS) and hasattr(lib, "qr_shuffle") and hasattr(lib, "qr_ppo_actor_grad_dev")
    assert int(out["abi"]) == L.ABI_VERSION == 16 and lib.qr_abi_version() == 16


def _fake():
    """A QrShuffle over made-up, aligned addresses that passes every check: each case below breaks one, so nothing is launched."""
    return L.QrShuffle(0x10000, 0x20000, 210, 3, 100, 5, 7, 9, 0)


@pytest.mark.parametrize("name,value,want", [
    ("n", 0, SIZE), ("n", -1, SIZE), ("n", 2 ** 32, SIZE), ("first", -1, SIZE), ("count", -1, SIZE), ("first", 111, SIZE), ("count", 208, SIZE),
    ("first", 2 ** 62, SIZE), ("count", 2 ** 63 - 1, SIZE), ("stream", 2 ** 30, SIZE), ("max_workgroups", -1, SIZE), ("out", None, NULL),
    ("out", 0x10004, ALIGN), ("out", 0x10001, ALIGN), ("draw_dev", 0x20004, ALIGN)])
def test_shuffle_errors(name, value, want):
    lib = L.load()
    s = _fake()
    setattr(s, name, value)
    assert lib.qr_shuffle(C.byref(s), None) == want
    assert lib.qr_shuffle(None, None) == NULL


def test_draw_is_checked_only_where_it_is_used_and_an_empty_slice_launches_nothing():
    lib = L.load()
    s = _fake()
    s.draw, s.draw_dev = -1, None
    assert lib.qr_shuffle(C.byref(s), None) == SIZE
    s = _fake()
    s.draw, s.out = -1, 0x10004                           # past the SIZE checks with a device counter
    assert lib.qr_shuffle(C.byref(s), None) == ALIGN
    for first in (0, 210):
        s = _fake()
        s.first, s.count, s.out, s.draw_dev = first, 0, None, 0x20004    # count = 0 returns before the pointers are looked at
        assert lib.qr_shuffle(C.byref(s), None) == 0
    s = _fake()
    s.count, s.n = 0, 0
    assert lib.qr_shuffle(C.byref(s), None) == SIZE       # ... but behind the sizes


# ---------------------------------------------------------------- the Python side's checks, all before a launch
def test_shuffle_checks():
    out = torch.zeros(100, dtype=torch.int64)
    good = dict(n=210, seed=1, draw=0, stream=4)
    bad = [dict(n=0), dict(n=2 ** 32), dict(n=99), dict(first=-1), dict(first=111), dict(seed=-1), dict(seed=2 ** 64), dict(draw=-1), dict(draw=2 ** 63),
           dict(stream=-1), dict(stream=2 ** 30), dict(max_workgroups=-1), dict(draw_dev=torch.zeros(1, dtype=torch.int32)),
           dict(draw_dev=torch.zeros(2, dtype=torch.int64)), dict(draw_dev=torch.zeros(1, dtype=torch.int64, device="meta")), dict(draw_dev=3)]
    for change in bad:
        with pytest.raises(ValueError):
            shuffle(out, **dict(good, **change))
    for o in (torch.zeros(100, dtype=torch.int32), torch.zeros(100, 2, dtype=torch.int64)[:, 0], None, torch.zeros(100)):
        with pytest.raises(ValueError):
            shuffle(o, **good)
    with pytest.raises(RuntimeError):              # all checks passed: there is no CPU kernel
        shuffle(out, **good)
    with pytest.raises(RuntimeError):
        shuffle(out, **dict(good, draw=-5, draw_dev=torch.zeros(1, dtype=torch.int64)))   # draw is not read with a device counter
    assert bool((out == 0).all())
    with pytest.raises((ValueError, RuntimeError)):
        torch.ops.gym_rotor_amd.qr_shuffle(out, 99, 0, 1, 0, 4, None)


def test_ppo_stream_is_disjoint_from_the_other_streams():
    ids = [ppo_stream(k, name) for k in (0, 1, 65535) for name in PPO_STREAM_NAMES]
    assert len(set(ids)) == 6 and ppo_stream(0, "shuffle") == 3 << 27 and ppo_stream(1, "noise") == (3 << 27) | (1 << 8) | 1
    es_max = max(ES.es_stream(k, n) for k in (0, 65535) for n in ES.NAMES)
    noise_max = max(OP.noise_stream(k, OP.NOISE_NAMES[-1], 3) for k in (0, 255, 65535))
    assert noise_max < ES.ES_STREAM and es_max < min(ids) and max(ids) < OP.COLLECTOR_STREAM < L.NOISE_MAX_STREAM
    for bad in ((-1, "noise"), (65536, "noise"), (0, "perm")):
        with pytest.raises(ValueError):
            ppo_stream(*bad)
