"""NumPy restatement of the replay buffer's two launches (qr_replay_add, qr_replay_sample; include/quadrotor_hip.h): the sampler's
keyed permutation of [0, n) in unsigned integers — Philox4x32-10 as gym_rotor_amd/csrc/qr_rng.h writes it, the six-round balanced
Feistel network on 2 h bits, cycle walking — and the append rule on plain arrays.  Integer only, so the device gives these bits."""
import numpy as np

ROUNDS = 6
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)


def philox_word0(c0, c1, c2, c3, seed: int):
    """Word 0 of philox4x32_10 for arrays (or scalars) of counter words under the key (seed_lo, seed_hi); uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & U32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2   # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & U32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0


def half_bits(n: int) -> int:
    return max(1, -(-int(n - 1).bit_length() // 2))


def feistel(x, n: int, seed: int, draw):
    """One pass of the network over an array of points of [0, 4^h); draw: one draw counter, or an array of them of x's shape."""
    h = half_bits(n)
    mask = np.uint64((1 << h) - 1)
    x = np.asarray(x, dtype=np.uint64)
    draw = np.asarray(draw, dtype=np.uint64)
    L, R = x >> np.uint64(h), x & mask
    for r in range(ROUNDS):
        F = philox_word0(R, r, draw & U32, draw >> np.uint64(32), seed)
        L, R = R, L ^ (F & mask)
    return (L << np.uint64(h)) | R


def sample(n: int, batch: int, seed: int, draw, return_walk: bool = False):
    """index[j] = the first of P(j), P(P(j)), ... below n, j = 0 .. batch - 1: int64 [batch]; draw a sequence of K counters: int64
    [K, batch], row i drawn with draw[i].  Raises if a walk reaches its cap of 4^h steps (a permutation's cycle through j < n returns
    below n before that).  return_walk: also the longest walk."""
    n, batch = int(n), int(batch)
    if not 1 <= batch <= n < 2 ** 31:
        raise ValueError(f"need 1 <= batch <= n < 2^31, got batch {batch}, n {n}")
    cap = 1 << (2 * half_bits(n))
    draws = np.atleast_1d(np.asarray(draw, dtype=np.uint64))
    d = np.repeat(draws, batch)
    x = feistel(np.tile(np.arange(batch, dtype=np.uint64), draws.size), n, seed, d)
    steps = 1
    while True:
        out = np.nonzero(x >= np.uint64(n))[0]
        if out.size == 0:
            break
        if steps >= cap:
            raise RuntimeError(f"a walk did not return below n = {n} within {cap} steps")
        x[out] = feistel(x[out], n, seed, d[out])
        steps += 1
    idx = x.astype(np.int64).reshape(draws.size, batch)
    idx = idx[0] if np.ndim(draw) == 0 else idx
    return (idx, steps) if return_walk else idx


def append(buf, count: int, obs, final_obs, action, reward, done, truncated):
    """The append rule on arrays, in place.  buf: per agent a dict of obs, obs_next [capacity, D_k], act [capacity, A_k], rwd, done
    [capacity]; obs: per agent [T + 1, N, D_k]; final_obs: per agent [T, N, D_k] or None; action [T, N, sum A_k]; reward, done
    [T, N, n_agents]; truncated [T, N] or None.  Returns the next count."""
    capacity = buf[0]["obs"].shape[0]
    T, N = action.shape[:2]
    n = T * N
    assert n <= capacity
    rows = (count + np.arange(n)) % capacity
    reset = done.reshape(n, -1).any(-1)
    if truncated is not None:
        reset = reset | truncated.reshape(n)
    col = 0
    for k, b in enumerate(buf):
        D, A = b["obs"].shape[1], b["act"].shape[1]
        nxt = obs[k][1:].reshape(n, D)
        if final_obs is not None:
            nxt = np.where(reset[:, None], final_obs[k].reshape(n, D), nxt)
        b["obs"][rows] = obs[k][:-1].reshape(n, D)
        b["obs_next"][rows] = nxt
        b["act"][rows] = action.reshape(n, -1)[:, col:col + A]
        b["rwd"][rows] = reward.reshape(n, -1)[:, k]
        b["done"][rows] = done.reshape(n, -1)[:, k].astype(np.float32)
        col += A
    return (count + n) % capacity
