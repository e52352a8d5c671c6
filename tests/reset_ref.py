"""NumPy restatement of the library's episode starts (gym_rotor_amd/csrc/qr_rng.h: draw20 / sample_start — qr_reset, qr_traj_start —
and make_pool / take_from_lds — the in-launch reset; qr_traj.h: traj_draws).  No torch, no GPU.

Both streams are Philox4x32-10 (tests/noise_ref.py: philox4, pinned to the published vectors) under the key (seed_lo, seed_hi):
    qr_reset / qr_traj_start   block b of an env      counter (gid_lo, gid_hi, episode, b)
    in-launch pool             block b of slot s      counter (gfirst_lo, gfirst_hi, count, 0x40000000 | s << 8 | b)
gid = env_offset + local index, gfirst = global id of the 64-env tile's first env, count = the tile's reset counter at that env-step,
s = 12 * pass + k = rank of the lane among the tile's lanes that reset in that step.  The 20 words of a start mean the same in both:
    0..5 m, d, J1, J3, c_tf, c_tw   6..8 x   9..11 v   12..14 W   15 zero-error branch   16 yaw   17 roll   18 pitch   19 goal generator

Parameters, x, v, W, the three angles and the goal generator's draws are float32 numbers with ONE rounding each and are restated bit
for bit.  The attitude goes through float32 half-angle polynomials on the device; here R = Rz(yaw) Ry(pitch) Rx(roll) (the
reference's Rotation.from_euler('xyz', (roll, pitch, yaw)), quad.py:197-199) is formed in float64 from the float32 angles, and
`R_f32`, the same composition in plain float32 NumPy, sizes the bar the device is held to (attitude_bar).

One difference between the two kernels' texts is restated, not hidden: sample_start forms x, v, W as the product scale * sym, the pool
as fmaf(scale, sym, +0).  With a zero scale (the zero-error branch, eval's v and W) the product of a negative sym is -0.0 and the
fused form +0.0 — equal numbers, different sign bits.  `pool=True` selects the fused form."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from noise_ref import U32, fma32, philox4, sym, u01  # noqa: E402

POOL_TAG = 0x40000000
F32 = np.float32
PI_F32, LIM_R_F32 = F32(np.pi), F32(50.0 * np.pi / 180.0)
THETA_B1D_F32, W_B1D_F32 = F32(25.0 * np.pi / 180.0), F32(0.15 * np.pi)
ATTITUDE_CEILING = 1e-5      # 2^-23 absolute in each of the six trig values, through the triple products and the quadratic form
F32_QUAT_STORAGE = 16 * 2.0 ** -24   # layout 'f32': the quaternion is stored as packed float32


def _u64(a):
    """uint64 array of 64-bit ids (Python ints of any size below 2^64, or arrays)."""
    return np.atleast_1d(np.asarray(a, dtype=np.uint64))


def _u32(a):
    """int32 counters as the kernels read them: the low 32 bits."""
    return (np.atleast_1d(np.asarray(a)).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)


def draw20_words(seed: int, gid, episode):
    """uint64 [n, 20]: draw20(seed, gid, episode) — block b (0..4) is philox4(gid_lo, gid_hi, episode, b, seed)."""
    gid = _u64(gid)
    gid, episode = np.broadcast_arrays(gid, _u32(episode))
    return np.concatenate([philox4(gid & U32, gid >> np.uint64(32), episode, b, seed) for b in range(5)]).T


def pool_words(seed: int, gfirst, count, slot):
    """uint64 [n, 20]: slot `slot` = 12 * pass + k of the pool of (gfirst, count) — block b is
    philox4(gfirst_lo, gfirst_hi, count, 0x40000000 | slot << 8 | b, seed)."""
    gfirst, count, slot = np.broadcast_arrays(_u64(gfirst), _u32(count), _u32(slot))
    return np.concatenate([philox4(gfirst & U32, gfirst >> np.uint64(32), count, np.uint64(POOL_TAG) | (slot << np.uint64(8)) | np.uint64(b), seed)
                           for b in range(5)]).T


def coeffs(constants=None, UDM_percentage: float = 10.0):
    """The float32 values the host hands the samplers (qr_launch.h: fill_coeffs): nom_f[6], udm, reset_v = v_lim / 2, reset_W = W_lim / 2.
    `constants`: anything with the fields of gym_rotor_amd.constants.QuadConstants (default: the reference's values)."""
    g = (lambda name, dflt: dflt) if constants is None else (lambda name, dflt: getattr(constants, name))
    nom = [g("m_nominal", 2.15), g("d_nominal", 0.23), g("J1_nominal", 0.022), g("J3_nominal", 0.035), g("c_tf_nominal", 0.0135), g("c_tw_nominal", 2.2)]
    return dict(nom=np.array(nom, dtype=np.float64).astype(F32), udm=F32(float(UDM_percentage) / 100.0),
                reset_v=F32(g("v_lim", 4.0) * 0.5), reset_W=F32(g("W_lim", 2.0 * np.pi) * 0.5))


def rotation_f64(yaw, roll, pitch):
    """float64 [n, 3, 3] = Rz(yaw) Ry(pitch) Rx(roll)."""
    y, r, p = (np.asarray(a, dtype=np.float64) for a in (yaw, roll, pitch))
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    R = np.empty(y.shape + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = -sp, cp * sr, cp * cr
    return R


def quat_to_R(q):
    """float64 [n, 3, 3] of quaternions [n, 4] (w, x, y, z), formed in float64."""
    w, x, y, z = (np.asarray(q[..., j], dtype=np.float64) for j in range(4))
    R = np.empty(w.shape + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def rotation_f32(yaw, roll, pitch):
    """The composition as sample_attitude writes it, q = qz(yaw) qy(pitch) qx(roll), in plain float32 NumPy: float32 sin / cos of the
    float32 half angles, every product and sum rounded to float32, normalised in float32; R of that quaternion (formed in float64,
    as qr_get_state forms it).  Not the device's arithmetic: its distance from rotation_f64 is what float32 costs here."""
    h = F32(0.5)
    y, r, p = (np.asarray(a, dtype=F32) for a in (yaw, roll, pitch))
    sr, cr, sp, cp, sy, cy = np.sin(h * r), np.cos(h * r), np.sin(h * p), np.cos(h * p), np.sin(h * y), np.cos(h * y)
    q = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1)
    assert q.dtype == F32
    q = q / np.sqrt((q * q).sum(-1, dtype=F32))[..., None]
    return quat_to_R(q)


def start_from_words(words, randomise: bool, eval: bool, coeffs: dict, pool: bool = False):
    """The episode start of each row of `words` (uint64 [n, 20]).  Returns a dict:
      params  float32 [n, 6]   fma32(float32(nom_j * p), sym_j, nom_j), row 5 with nom_5 * float32(0.5 p); nominal without `randomise` / with `eval`
      x, v, W float32 [n, 3]   scale * sym in one float32 rounding; scales 0.6, reset_v, reset_W — all zero in the zero-error branch
                               (u01(word 15) < float32(0.2)); eval: 0.4, 0, 0 and no zero-error branch
      yaw, roll, pitch float32 [n]   float32(pi) sym(16) in every branch (quad.py:339), iR sym(17), iR sym(18), iR = float32(50 pi / 180) or 0
      zero    bool [n]         the zero-error branch was taken
      R       float64 [n, 3, 3]  Rz(yaw) Ry(pitch) Rx(roll) in float64 from the float32 angles
      R_f32   float64 [n, 3, 3]  rotation_f32 of the same angles
    pool=True: the in-launch pool's fused form (a zero scale gives +0.0, never -0.0; see the module text)."""
    words = np.asarray(words, dtype=np.uint64)
    n = words.shape[0]
    s = sym(words)                                                  # float32 [n, 20]
    nom, p = coeffs["nom"], coeffs["udm"]
    if randomise and not eval:
        scale = np.array([nom[j] * p for j in range(5)] + [nom[5] * (F32(0.5) * p)], dtype=F32)   # float32 products
        params = np.stack([fma32(np.full(n, scale[j]), s[:, j], np.full(n, nom[j])) for j in range(6)], 1)
    else:
        params = np.tile(nom, (n, 1))
    zero = np.zeros(n, dtype=bool) if eval else (u01(words[:, 15]) < F32(0.2))
    z, one = F32(0.0), np.ones(n, dtype=F32)
    if eval:
        ix, iv, iW, iR = F32(0.4) * one, z * one, z * one, z * one
    else:
        ix, iv = np.where(zero, z, F32(0.6)), np.where(zero, z, coeffs["reset_v"])
        iW, iR = np.where(zero, z, coeffs["reset_W"]), np.where(zero, z, LIM_R_F32)
    plus0 = (lambda a: a + z) if pool else (lambda a: a)            # fmaf(scale, sym, +0): -0 + +0 = +0
    x, v, W = plus0(ix[:, None] * s[:, 6:9]), plus0(iv[:, None] * s[:, 9:12]), plus0(iW[:, None] * s[:, 12:15])
    yaw, roll, pitch = plus0(PI_F32 * s[:, 16]), plus0(iR * s[:, 17]), plus0(iR * s[:, 18])
    for a in (params, x, v, W, yaw, roll, pitch):
        assert a.dtype == F32
    return dict(params=params, x=x, v=v, W=W, yaw=yaw, roll=roll, pitch=pitch, zero=zero,
                R=rotation_f64(yaw, roll, pitch), R_f32=rotation_f32(yaw, roll, pitch))


def state_rows(start: dict, R=None):
    """float64 [n, 18]: the library's state row (x, v, vec_F(R) — column-major —, W) of a start_from_words result."""
    R = start["R"] if R is None else R
    f = lambda a: a.astype(np.float64)
    return np.concatenate([f(start["x"]), f(start["v"]), np.swapaxes(R, -1, -2).reshape(-1, 9), f(start["W"])], 1)


def rows_R(rows):
    """float64 [n, 3, 3] from state rows [n, 18]."""
    return np.swapaxes(np.asarray(rows, dtype=np.float64)[:, 6:15].reshape(-1, 3, 3), 1, 2)


def traj_draws(word19):
    """(theta_b1d, t_traj, w_b1d) float32 [n] of traj_draws(r19): float32(25 pi / 180) sym(w); 2 + 3 (float32(w >> 16) 2^-16 + 2^-17),
    exact in float32 however it is fused (20 significant bits); float32(0.15 pi) fma32(float32(w & 0xFFFF), 2^-15, 2^-16 - 1)."""
    w = np.asarray(word19, dtype=np.uint64)
    theta = THETA_B1D_F32 * sym(w)
    t_traj = (2.0 + 3.0 * ((w >> np.uint64(16)).astype(np.float64) * 2.0 ** -16 + 2.0 ** -17)).astype(F32)
    lo = (w & np.uint64(0xFFFF)).astype(F32)
    w_b1d = W_B1D_F32 * fma32(lo, np.full(lo.shape, F32(2.0 ** -15)), np.full(lo.shape, F32(2.0 ** -16 - 1.0))).reshape(lo.shape)
    assert theta.dtype == F32 and w_b1d.dtype == F32
    return theta, t_traj, w_b1d


def sincos_small_f32(x):
    """(sin, cos) float32 of qr_rng.h's sincos_small, bit for bit: every operation there is a single float32 product, an explicit
    fmaf or a select, so nothing is left to the compiler."""
    x = np.atleast_1d(np.asarray(x, dtype=F32))
    k = np.rint(x * F32(0.63661977236758134)).astype(F32)          # rintf: ties to even
    r = fma32(-k, F32(1.5707962512969971), x)
    r = fma32(-k, F32(7.5497894158615964e-08), r)
    r2 = r * r
    ps = fma32(r * r2, fma32(r2, fma32(r2, F32(-1.9515295891e-4), F32(8.3321608736e-3)), F32(-1.6666654611e-1)), r)
    pc = fma32(r2 * r2, fma32(r2, fma32(r2, F32(2.443315711809948e-5), F32(-1.388731625493765e-3)), F32(4.166664568298827e-2)),
               fma32(F32(-0.5), r2, F32(1.0)))
    q = k.astype(np.int64)
    odd = (q & 1) != 0
    s0, c0 = np.where(odd, pc, ps), np.where(odd, ps, pc)
    return np.where((q & 2) != 0, -s0, s0).astype(F32), np.where(((q + 1) & 2) != 0, -c0, c0).astype(F32)


def mode0_b1d(theta_init, word19):
    """The two values traj_start's mode 0 admits for (b1d_x, b1d_y) = (cos, sin)(theta_init + theta_b1d), theta_b1d = float32(25 pi / 180)
    sym(w): under -ffp-contract=fast the sum may take theta_b1d rounded (where the draw arrives as a number: qr_traj_start) or fuse
    its product (where traj_draws is inlined next to it: the step kernels) — one rounding apart in the ARGUMENT.  theta_init is the
    device's own float32 (atan2_fast goes through v_rcp_f32, which has no restatement).  Returns ((cos, sin) unfused, (cos, sin) fused)."""
    ti, s = np.atleast_1d(np.asarray(theta_init, dtype=F32)), sym(np.asarray(word19, dtype=np.uint64))
    sn0, cs0 = sincos_small_f32(ti + THETA_B1D_F32 * s)
    sn1, cs1 = sincos_small_f32(fma32(np.full(s.shape, THETA_B1D_F32), s, ti))
    return (cs0, sn0), (cs1, sn1)


def attitude_bar(start: dict, layout: str = "mixed"):
    """(e32, bar) for the rows of `start`: e32 = max |R_f32 - R|, the restatement's own float32 error on these words; bar = 4 e32 —
    a factor 2 for the device's freedom to fuse and order the products, a factor 2 for its polynomials' documented ~1e-7 against
    NumPy's correctly rounded functions — plus 16 * 2^-24 for layout 'f32' (the packed float32 quaternion in storage).  A bar above
    the 1e-5 ceiling is a mis-sized test and raises."""
    e32 = float(np.abs(start["R_f32"] - start["R"]).max())
    bar = 4.0 * e32 + (F32_QUAT_STORAGE if layout == "f32" else 0.0)
    if not 0.0 < bar <= ATTITUDE_CEILING:
        raise AssertionError(f"attitude bar {bar:.3e} mis-sized (e32 {e32:.3e}, ceiling {ATTITUDE_CEILING:.0e})")
    return e32, bar


def bits_equal(a, b):
    """Element-wise: the same bits (two arrays of one float dtype, 4 or 8 bytes wide).  -0.0 and +0.0 differ."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    it = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return a.view(it) == b.view(it)


def ranks_in_tile(rows):
    """Per env: its rank among the True rows of its 64-env tile (meaningful where `rows` is True) — the pool slot of a resetting lane."""
    rows = np.asarray(rows, dtype=bool)
    n = rows.shape[0]
    pad = np.zeros((n + 63) // 64 * 64, dtype=np.int64)
    pad[:n] = rows
    return (np.cumsum(pad.reshape(-1, 64), 1) - pad.reshape(-1, 64)).reshape(-1)[:n]


# ---------------------------------------------------------------------------------------------------------------------
# the keys of tests/test_gpu_reset_stream.py (shared with tests/test_reset_host.py, which checks the restatement on them)
# ---------------------------------------------------------------------------------------------------------------------
TEST_N = 64 * 6 + 17                              # whole tiles plus a ragged tail
TEST_SEED = 0x0123456789ABCDEF & (2 ** 63 - 1)    # a non-zero high word
TEST_OFFSETS = (0, 192, 2 ** 32 + 5 * 64)         # the last: a non-zero high word of the global env id
TEST_KILLS = (1, 12, 13, 64, 0, 5)                # lanes killed per whole tile (the tail: its last three)


def kill_rows(rng, n: int = TEST_N, counts=TEST_KILLS):
    """bool [n]: per whole tile `counts` lanes at random positions, plus the ragged tail's last three."""
    k = np.zeros(n, dtype=bool)
    for t, c in enumerate(counts):
        k[64 * t + rng.permutation(64)[:c]] = True
    k[n - 3:] = True
    return k


def pool_keys(rows, env_offset: int, reset_count):
    """(rows' indices, gfirst, count, slot) of the in-launch resets `rows` (bool [n]) of one env-step: reset_count is the per-tile counter
    AT that env-step (int [tiles])."""
    idx = np.flatnonzero(rows)
    tile = idx // 64
    gfirst = (np.asarray(tile, dtype=object) * 64 + int(env_offset)).astype(np.uint64)
    return idx, gfirst, np.asarray(reset_count)[tile], ranks_in_tile(rows)[idx]
