"""NumPy restatement of the library's noise stream (qr_noise_fill; include/quadrotor_hip.h, gym_rotor_amd/csrc/qr_noise.h).

Element e of a tensor is position e % 4 of quad q = e // 4, whose four words are Philox4x32-10 — as gym_rotor_amd/csrc/qr_rng.h
writes it, all four words here (tests/replay_ref.py restates word 0) — under the key (seed_lo, seed_hi) with the counter
(q_lo, q_hi ^ draw_hi, draw_lo, 0xC0000000 | stream).

UNIFORM is integer-to-float arithmetic with one rounding per fused multiply-add and is restated bit for bit (`fma32`).  NORMAL follows
the kernel's float32 inputs — u = float32(w >> 8) * 2^-24 + 2^-25 in one rounding, the float32 angle product — and takes sqrt, log,
cos and sin in float64 from them: what the device's float32 arithmetic is measured against."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)
NORMAL, UNIFORM = 0, 1
STREAM_BITS = 0x80000000 | 0x40000000
TWO_PI_F32 = np.float32(6.283185307179586)


def philox4(c0, c1, c2, c3, seed: int):
    """The four words of philox4x32_10 for arrays (or scalars) of counter words under the key (seed_lo, seed_hi): uint64 [4, ...]
    holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & U32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2   # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & U32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3])


def words(count: int, seed: int, draw: int, stream: int, first_quad: int = 0):
    """uint64 [n_quads, 4]: the words of the quads first_quad .. first_quad + ceil(count / 4) - 1 of (seed, draw, stream)."""
    if not (0 <= seed < 2 ** 64 and 0 <= draw < 2 ** 64 and 0 <= stream < 2 ** 30 and count >= 1):
        raise ValueError("need 0 <= seed, draw < 2^64, 0 <= stream < 2^30 and count >= 1")
    q = np.arange(first_quad, first_quad + (count + 3) // 4, dtype=np.uint64)
    return philox4(q & U32, (q >> np.uint64(32)) ^ np.uint64(draw >> 32), draw & 0xFFFFFFFF, STREAM_BITS | stream, seed).T


def fma32(b, x, a):
    """float32(b * x + a) with ONE rounding, for float32 arrays: the product of two float32 numbers is exact in float64; the sum is
    formed there with its rounding error (TwoSum) and, where it is inexact, nudged to an odd last bit (round to odd), after which
    the rounding to float32 is the correct one (53 >= 2 * 24 + 2 bits)."""
    b, x, a = (np.atleast_1d(np.asarray(v, dtype=np.float32)).astype(np.float64) for v in (b, x, a))
    p = b * x
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    up = (err > 0) == (s >= 0)          # move away from zero when the error has the sum's sign
    bits = np.where(fix, np.where(up, bits + 1, bits - 1), bits)
    # (s == 0 with err != 0 cannot happen: then s would be err itself)
    return bits.view(np.float64).astype(np.float32)


def u01(w):
    """fmaf((float)(w >> 8), 2^-24, 2^-25): 25 significant bits, exact in float64, rounded once."""
    return (np.asarray(w >> np.uint64(8), dtype=np.float64) * 2.0 ** -24 + 2.0 ** -25).astype(np.float32)


def sym(w):
    """fmaf((float)(w >> 8), 2^-23, 2^-24 - 1): a multiple of 2^-24 below 1 in magnitude — exact."""
    return (np.asarray(w >> np.uint64(8), dtype=np.float64) * 2.0 ** -23 + (2.0 ** -24 - 1.0)).astype(np.float32)


def normals_from_words(w):
    """float64 [n_quads, 4] from uint64 [n_quads, 4]: Box-Muller on the word pairs (0, 1) and (2, 3), the inputs rounded as the kernel
    rounds them (u1, u2 and the angle 2 pi u2 are float32 numbers), the functions in float64."""
    w = np.asarray(w, dtype=np.uint64)
    z = np.empty(w.shape, dtype=np.float64)
    for h in (0, 1):
        u1, u2 = u01(w[:, 2 * h]), u01(w[:, 2 * h + 1])
        r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
        ang = (TWO_PI_F32 * u2).astype(np.float32).astype(np.float64)   # the float32 product
        z[:, 2 * h], z[:, 2 * h + 1] = r * np.cos(ang), r * np.sin(ang)
    return z


def uniform(count: int, seed: int, draw: int, stream: int, a=0.0, b=1.0):
    """float32 [count]: the UNIFORM slot, bit for bit."""
    return fma32(np.float32(b), sym(words(count, seed, draw, stream)).reshape(-1)[:count], np.float32(a))


def normal(count: int, seed: int, draw: int, stream: int, a=0.0, b=1.0):
    """float64 [count]: the NORMAL slot, a + b z with a and b rounded to float32 and z, the product and the sum in float64."""
    z = normals_from_words(words(count, seed, draw, stream)).reshape(-1)[:count]
    return np.float64(np.float32(a)) + np.float64(np.float32(b)) * z
