"""The keyed permutation on the GPU (qr_shuffle; gym_rotor_amd.shuffle): every value `==` the NumPy restatement of tests/shuffle_ref.py —
whole permutations at the sizes where the network's width changes, slices at the top of the range, guarded odd slices — and the
contract: the draw number read on the device, the grid, the stream."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shuffle_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
SEED, DRAW, STREAM = 2 ** 63 + 2 ** 40 + 3, 2 ** 32 + 1, (3 << 27) | (1 << 8)
KEY = dict(seed=SEED, draw=DRAW, stream=STREAM)
SENTINEL = -7


def _np(t):
    return t.detach().cpu().numpy()


def _run(n, first=0, count=None, guard=0, **kw):
    from gym_rotor_amd import shuffle
    count = n - first if count is None else count
    buf = torch.full((count + 2 * guard,), SENTINEL, dtype=torch.int64, device="cuda")
    out = shuffle(buf[guard:guard + count], n=n, first=first, **dict(KEY, **kw))
    torch.cuda.synchronize()
    assert count == 0 or out.data_ptr() == buf.data_ptr() + 8 * guard
    return _np(buf)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 210, 4096, 4097, 65536, 65537, 2 ** 20 + 1])
def test_whole_permutation_equals_the_restatement(n):
    got = _run(n)
    assert np.array_equal(got, SR.shuffle_ref(n, SEED, DRAW, STREAM))
    if n == 2 ** 20 + 1:
        assert np.array_equal(np.sort(got), np.arange(n))


@pytest.mark.parametrize("first", [0, 2 ** 32 - 1 - 1000])
def test_slices_at_the_largest_n(first):
    n = 2 ** 32 - 1
    got = _run(n, first, 1000)
    assert np.array_equal(got, SR.shuffle_ref(n, SEED, DRAW, STREAM, first, 1000)) and got.min() >= 0 and got.max() < n


@pytest.mark.parametrize("n,first,count", [(210, 1, 81), (210, 127, 83), (4097, 257, 3839), (65537, 65536, 1), (2 ** 20 + 1, 999999, 4097), (17, 5, 0)])
def test_odd_slices_between_sentinels(n, first, count):
    got = _run(n, first, count, guard=16)
    assert (got[:16] == SENTINEL).all() and (got[16 + count:] == SENTINEL).all() and got.size == count + 32
    assert np.array_equal(got[16:16 + count], SR.shuffle_ref(n, SEED, DRAW, STREAM, first, count))


def test_draw_on_the_device_equals_the_draw_by_value():
    from gym_rotor_amd import shuffle
    n = 4097
    state = torch.tensor([5, DRAW, 11], dtype=torch.int64, device="cuda")
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    shuffle(out, n=n, seed=SEED, draw=0, stream=STREAM, draw_dev=state[1:2])
    op = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.ops.gym_rotor_amd.qr_shuffle(op, n, 0, SEED - 2 ** 63, DRAW, STREAM, None)
    torch.cuda.synchronize()
    assert np.array_equal(_np(out), _run(n)) and state.tolist() == [5, DRAW, 11]          # the word is only read
    assert np.array_equal(_np(op), SR.shuffle_ref(n, SEED - 2 ** 63, DRAW, STREAM))       # (the op takes an int64 seed)
    state[1] += 1
    shuffle(out, n=n, seed=SEED, draw=0, stream=STREAM, draw_dev=state[1:2])
    torch.cuda.synchronize()
    assert np.array_equal(_np(out), _run(n, draw=DRAW + 1)) and not np.array_equal(_np(out), _run(n))


@pytest.mark.parametrize("n", [210, 65537, 2 ** 20 + 1])
def test_the_grid_cannot_change_a_value(n):
    want = _run(n)
    for cap in (1, 3, 2048):
        assert np.array_equal(_run(n, max_workgroups=cap), want), cap


def test_keys_give_different_permutations():
    base = _run(210)
    for change in (dict(stream=STREAM + 1), dict(seed=SEED + 1), dict(seed=SEED - 2 ** 40), dict(draw=DRAW + 1), dict(draw=DRAW - 2 ** 32)):
        other = _run(210, **change)
        assert not np.array_equal(other, base) and np.array_equal(np.sort(other), np.arange(210)), change
        k = dict(KEY, **change)
        assert np.array_equal(other, SR.shuffle_ref(210, k["seed"], k["draw"], k["stream"]))
