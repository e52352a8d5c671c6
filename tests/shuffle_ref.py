"""NumPy restatement of the library's keyed permutation (qr_shuffle; include/quadrotor_hip.h, gym_rotor_amd/csrc/qr_shuffle.h), on top of
tests/noise_ref.py's Philox.

perm is a bijection of [0, n) and a function of (seed, draw, stream, n) alone.  n = 1: [0].  Otherwise w is the smallest integer in
1..16 with 2^(2w) >= n (so 2^(2w) < 4n), and perm(i) walks a balanced Feistel network on 2w bits from x = i until the result is below n
(cycle walking).  ROUNDS rounds, round r: (L, R) -> (R, L ^ F_r(R)) with F_r(v) = mix32(v + key[r]) >> (32 - w); key[4k .. 4k + 3] are
the four raw Philox4x32-10 words of quad k of the qr_noise_fill stream (seed, draw, stream) — `noise_ref.words`, before they become
floats.  mix32 is the 32-bit multiply-xorshift finaliser x ^= x >> 16; x *= M1; x ^= x >> 15; x *= M2; x ^= x >> 16."""
import numpy as np

import noise_ref as NR

ROUNDS = 8
MIX_M1, MIX_M2 = 0x7FEB352D, 0x846CA68B
_U32 = np.uint64(0xFFFFFFFF)


def half_bits(n: int) -> int:
    """w: the smallest integer in 1..16 with 2^(2w) >= n."""
    if not 1 <= n < 2 ** 32:
        raise ValueError("need 1 <= n < 2^32")
    w = 1
    while (1 << (2 * w)) < n:
        w += 1
    return w


def mix32(x):
    """The finaliser on uint64 arrays holding 32-bit values."""
    x = np.asarray(x, dtype=np.uint64) & _U32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(MIX_M1)) & _U32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(MIX_M2)) & _U32
    return x ^ (x >> np.uint64(16))


def keys(seed: int, draw: int, stream: int, rounds: int = ROUNDS):
    """uint64 [rounds]: the raw words of quads 0 .. rounds / 4 - 1 of the noise stream (seed, draw, stream)."""
    return NR.words(rounds, seed, draw, stream).reshape(-1)[:rounds]


def network(x, key, w: int):
    """One application of the Feistel network on 2w bits to the uint64 array x."""
    mask, sh = np.uint64((1 << w) - 1), np.uint64(32 - w)
    L, R = x >> np.uint64(w), x & mask
    for k in key:
        L, R = R, L ^ (mix32(R + np.uint64(int(k))) >> sh)
    return (L << np.uint64(w)) | R


def shuffle_ref(n: int, seed: int, draw: int, stream: int, first: int = 0, count=None, rounds: int = ROUNDS):
    """int64 [count]: perm(first + i) for i < count (count None: the rest of [0, n))."""
    count = n - first if count is None else count
    if not (0 <= first and 0 <= count and first + count <= n):
        raise ValueError("need 0 <= first and first + count <= n")
    w = half_bits(n)
    if n == 1:
        return np.zeros(count, dtype=np.int64)
    key = keys(seed, draw, stream, rounds)
    x = np.arange(first, first + count, dtype=np.uint64)
    todo = np.ones(count, dtype=bool)
    while todo.any():
        x[todo] = network(x[todo], key, w)
        todo &= x >= np.uint64(n)
    return x.astype(np.int64)


def position_chi2(perms, n: int) -> float:
    """Chi-square statistic of the n x n table "element e at position p" over the rows of perms [draws, n] against draws / n."""
    perms = np.asarray(perms)
    draws = perms.shape[0]
    table = np.bincount((perms + n * np.arange(n)[None, :]).reshape(-1), minlength=n * n).astype(np.float64)
    e = draws / n
    return float(((table - e) ** 2).sum() / e)


def neighbours_kept(perms) -> int:
    """Over the rows of perms [draws, n]: how many pairs (i, i + 1) stay adjacent and in order (perm(i + 1) == perm(i) + 1)."""
    perms = np.asarray(perms)
    return int((perms[:, 1:] == perms[:, :-1] + 1).sum())
