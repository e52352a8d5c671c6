"""tests/reset_ref.py without a GPU: the restated attitude against the reference's own scipy call, the branch logic and ranges of
start_from_words on hand-made words, traj_draws against its closed forms, the two streams' keying, the size of the attitude bar on
the keys tests/test_gpu_reset_stream.py uses — and that mutated restatements (the errors that test exists to catch) differ from
the true one on those keys by more than it tolerates."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reset_ref as RR  # noqa: E402
from noise_ref import philox4, sym, u01  # noqa: E402

F32 = np.float32
C = RR.coeffs()
# word 15 on either side of the zero-error threshold: u01(w) = ((w >> 8) + 0.5) 2^-24 rounded to float32 against float32(0.2)
W_BELOW = next(w for w in range(int(0.2 * 2 ** 24) + 4, 0, -1) if u01(np.uint64(w << 8)) < F32(0.2)) << 8
W_ABOVE = W_BELOW + (1 << 8)


def _words(rows):
    return np.array(rows, dtype=np.uint64)


def _test_words(stream: str):
    """The words of the GPU test's own keys: every env of the batch at episode 1 / every slot 0..63 of every tile at count 0."""
    gid = np.arange(RR.TEST_N, dtype=np.uint64) + np.uint64(RR.TEST_OFFSETS[1])
    if stream == "draw20":
        return RR.draw20_words(RR.TEST_SEED, gid, 1)
    return RR.pool_words(RR.TEST_SEED, (gid // np.uint64(64)) * np.uint64(64), 0, np.arange(RR.TEST_N) % 64)


def test_restated_attitude_is_the_references_from_euler():
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    rng = np.random.default_rng(0)
    n = 4000
    yaw, roll, pitch = rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n)
    yaw[:4], roll[:4], pitch[:4] = (0.0, np.pi, -np.pi, 1.0), (0.0, 0.0, 0.5, -0.5), (0.0, 0.3, 0.0, -0.5)
    want = Rotation.from_euler("xyz", np.stack([roll, pitch, yaw], 1), degrees=False).as_matrix()   # quad.py:197-199
    got = RR.rotation_f64(yaw, roll, pitch)
    assert np.abs(got - want).max() <= 1e-14
    # on sampled words too, and the 18-word row is column-major (quad.py:204: R.reshape(9, 1, order='F'))
    st = RR.start_from_words(_test_words("draw20"), True, False, C)
    want = Rotation.from_euler("xyz", np.stack([st["roll"], st["pitch"], st["yaw"]], 1).astype(np.float64)).as_matrix()
    assert np.abs(st["R"] - want).max() <= 1e-14
    rows = RR.state_rows(st)
    assert rows.shape == (RR.TEST_N, 18) and np.array_equal(rows[:, 6:15], np.stack([w.reshape(9, order="F") for w in st["R"]]))
    assert np.abs(rows[:, 6:15] - np.stack([w.reshape(9, order="F") for w in want])).max() <= 1e-14
    assert np.array_equal(RR.rows_R(rows), st["R"])
    assert np.abs(RR.quat_to_R(Rotation.from_matrix(want).as_quat()[:, [3, 0, 1, 2]]) - want).max() <= 1e-14


def test_branches_and_ranges_on_hand_made_words():
    ones, zeros = [0xFFFFFFFF] * 20, [0] * 20
    below, above = list(range(1000, 21000, 1000)), list(range(1000, 21000, 1000))
    below = [(w * 0x9E3779B1) & 0xFFFFFFFF for w in below]; above = list(below)
    below[15], above[15] = W_BELOW, W_ABOVE
    assert u01(np.uint64(W_BELOW)) < F32(0.2) <= u01(np.uint64(W_ABOVE))
    w = _words([zeros, ones, below, above])
    s = sym(w)
    assert s[0, 0] == F32(2.0 ** -24 - 1.0) and s[1, 0] == F32(1.0 - 2.0 ** -24)       # the ends of sym: never +-1
    st = RR.start_from_words(w, True, False, C)
    assert list(st["zero"]) == [True, False, True, False]                           # u01(0) = 2^-25 < 0.2; u01(all ones) ~ 1
    # parameters: nominal (1 -+ p (1 - 2^-24)), c_tw half the width; one rounding each
    nom = C["nom"].astype(np.float64)
    width = np.array([0.1] * 5 + [0.05])
    for row, sgn in ((0, -1.0), (1, 1.0)):
        assert np.allclose(st["params"][row], nom * (1 + sgn * width), rtol=3e-7, atol=0)
        assert (np.abs(st["params"][row] / nom - 1) < width * (1 + 1e-6)).all()
    assert st["params"].dtype == F32
    # full-error branch at the ends of the range; zero-error branch all zero, yaw random all the same (quad.py:339)
    assert np.array_equal(st["x"][1], np.full(3, F32(0.6) * s[1, 6])) and np.array_equal(st["v"][1], np.full(3, F32(2.0) * s[1, 9]))
    assert np.array_equal(st["W"][1], np.full(3, F32(np.pi) * s[1, 12]))
    assert st["roll"][1] == RR.LIM_R_F32 * s[1, 17] and abs(float(st["roll"][1]) - np.deg2rad(50)) < 1e-6 and st["pitch"][1] == st["roll"][1]
    for row in (0, 2):
        assert not np.any(st["x"][row]) and not np.any(st["v"][row]) and not np.any(st["W"][row]) and st["roll"][row] == 0 and st["pitch"][row] == 0
        assert st["yaw"][row] == RR.PI_F32 * s[row, 16] and st["yaw"][row] != 0
        assert np.abs(st["R"][row] - RR.rotation_f64(st["yaw"][row:row + 1], [0.0], [0.0])[0]).max() == 0
    assert abs(float(st["yaw"][0]) + np.pi) < 1e-6 and abs(float(st["yaw"][1]) - np.pi) < 1e-6
    # rows 2 and 3 differ in word 15 alone: same parameters and yaw, everything else switched on
    assert np.array_equal(st["params"][2], st["params"][3]) and st["yaw"][2] == st["yaw"][3]
    assert np.all(st["x"][3] != 0) and np.all(st["v"][3] != 0) and np.all(st["W"][3] != 0) and st["roll"][3] != 0 and st["pitch"][3] != 0
    assert np.abs(st["x"][3]).max() < 0.6 and np.abs(st["v"][3]).max() < 2.0 and np.abs(st["W"][3]).max() < np.pi
    # the sign of a zero: sample_start's product keeps sym's sign, the pool's fused form gives +0 (reset_ref's module text)
    assert np.signbit(st["x"][0]).all() and not np.signbit(RR.start_from_words(w, True, False, C, pool=True)["x"][0]).any()
    pl = RR.start_from_words(w, True, False, C, pool=True)
    for k in ("params", "x", "v", "W", "yaw", "roll", "pitch"):
        assert np.array_equal(pl[k], st[k])                                          # equal as numbers everywhere
        assert RR.bits_equal(pl[k][[1, 3]], st[k][[1, 3]]).all()                     # and in bits outside the zero-error branch
    # eval: x within 0.4, v = W = roll = pitch = 0, no zero-error branch, nominal parameters
    ev = RR.start_from_words(w, True, True, C)
    assert not ev["zero"].any() and np.array_equal(ev["x"], F32(0.4) * s[:, 6:9]) and not np.any(ev["v"]) and not np.any(ev["W"])
    assert not np.any(ev["roll"]) and not np.any(ev["pitch"]) and np.array_equal(ev["yaw"], st["yaw"])
    assert np.array_equal(ev["params"], np.tile(C["nom"], (4, 1)))
    # randomise off: nominal parameters, the state as before
    off = RR.start_from_words(w, False, False, C)
    assert np.array_equal(off["params"], np.tile(C["nom"], (4, 1)))
    for k in ("x", "v", "W", "yaw", "roll", "pitch"):
        assert RR.bits_equal(off[k], st[k]).all()
    # other coefficients reach the values they scale
    from gym_rotor_amd.constants import QuadConstants
    c2 = RR.coeffs(QuadConstants(v_lim=3.3, W_lim=5.1, m_nominal=1.83), UDM_percentage=13.0)
    assert c2["reset_v"] == F32(1.65) and c2["reset_W"] == F32(2.55) and c2["udm"] == F32(0.13) and c2["nom"][0] == F32(1.83)
    s2 = RR.start_from_words(w, True, False, c2)
    assert np.array_equal(s2["v"][1], np.full(3, F32(1.65) * s[1, 9])) and np.array_equal(s2["W"][3], F32(2.55) * s[3, 12:15])
    assert abs(float(s2["params"][1, 0]) / 1.83 - 1.13) < 1e-6 and abs(float(s2["params"][0, 5]) / 2.2 - 0.935) < 1e-6
    assert np.array_equal(s2["x"], st["x"])


def test_traj_draws_against_the_closed_forms():
    mixed = 0xA5C3_7E19
    th, tt, wb = RR.traj_draws(_words([0, 0xFFFFFFFF, mixed]))
    assert th.dtype == tt.dtype == wb.dtype == F32
    d25, w15 = np.deg2rad(25.0), 0.15 * np.pi
    for i, w in enumerate((0, 0xFFFFFFFF, mixed)):
        assert abs(float(th[i]) - d25 * (((w >> 8) + 0.5) * 2.0 ** -23 - 1.0)) < 2e-7 * d25 + 1e-9
        assert float(tt[i]) == 2.0 + 3.0 * (((w >> 16) + 0.5) * 2.0 ** -16)                     # exact in float32
        assert abs(float(wb[i]) - w15 * (((w & 0xFFFF) + 0.5) * 2.0 ** -15 - 1.0)) < 2e-7 * w15 + 1e-9
    assert 2.0 < float(tt[0]) < 2.0001 and 4.9999 < float(tt[1]) < 5.0 and -d25 < float(th[0]) < -d25 * 0.9999 and w15 * 0.9999 < float(wb[1]) < w15
    # word 19 is split 16 / 16: the high half moves t_traj (and theta's 24 bits), the low half w_b1d alone
    a, b = RR.traj_draws(_words([0x1234_0000, 0x1234_FFFF]))[1:], RR.traj_draws(_words([0x0000_8000, 0xFFFF_8000]))[1:]
    assert a[0][0] == a[0][1] and a[1][0] != a[1][1] and b[0][0] != b[0][1] and b[1][0] == b[1][1]


def test_streams_are_tagged_and_keyed_by_all_64_bits():
    seed, gid = RR.TEST_SEED, np.array([0, 1, 64, 2 ** 32 + 64], dtype=np.uint64)
    d, p = RR.draw20_words(seed, gid, 3), RR.pool_words(seed, gid, 3, 0)
    assert d.shape == p.shape == (4, 20) and d.dtype == np.uint64 and int(d.max()) < 2 ** 32
    assert not (d == p).any()                                             # equal arguments, slot 0: only the 0x40000000 tag differs
    # the blocks are what the text says, word 4 b + j = word j of block b
    assert np.array_equal(d[3, 8:12], philox4(64, 1, 3, 2, seed))
    assert np.array_equal(p[3, 16:20], philox4(64, 1, 3, 0x40000000 | 4, seed))
    assert np.array_equal(RR.pool_words(seed, gid, 3, 37)[2, 4:8], philox4(64, 0, 3, 0x40000000 | 37 << 8 | 1, seed))
    # the high word of the seed and of the id are part of the key, in both streams
    for f in (RR.draw20_words, lambda s_, g_, e_: RR.pool_words(s_, g_, e_, 5)):
        base = f(seed, gid, 3)
        assert not (f(seed ^ (1 << 40), gid, 3) == base).all(1).any() and not (f(seed, gid ^ np.uint64(1 << 35), 3) == base).all(1).any()
        assert not (f(seed & 0xFFFFFFFF, gid, 3) == base).all(1).any()
        assert not (f(seed, gid, 4) == base).all(1).any() and len({tuple(r) for r in base}) == 4
    assert not (RR.pool_words(seed, gid, 3, 6) == RR.pool_words(seed, gid, 3, 5)).all(1).any()
    # counters arrive as int32: their low 32 bits count
    assert np.array_equal(RR.draw20_words(seed, gid, np.int32(-1)), RR.draw20_words(seed, gid, 0xFFFFFFFF))


def test_ranks_and_pool_keys():
    rows = np.zeros(64 * 2 + 5, dtype=bool)
    rows[[3, 9, 63, 64, 70, 130, 132]] = True
    assert list(RR.ranks_in_tile(rows)[rows]) == [0, 1, 2, 0, 1, 0, 1]
    idx, gfirst, count, slot = RR.pool_keys(rows, 2 ** 32 + 128, np.array([7, 8, 9]))
    assert list(idx) == [3, 9, 63, 64, 70, 130, 132] and list(slot) == [0, 1, 2, 0, 1, 0, 1] and list(count) == [7, 7, 7, 8, 8, 9, 9]
    assert [int(g) for g in gfirst] == [2 ** 32 + 128] * 3 + [2 ** 32 + 192] * 2 + [2 ** 32 + 256] * 2
    k = RR.kill_rows(np.random.default_rng(1))
    assert [int(k[64 * t:64 * t + 64].sum()) for t in range(6)] == list(RR.TEST_KILLS) and k[-3:].all() and k[384:].sum() == 3
    assert RR.ranks_in_tile(k)[k].max() == 63                              # slots of passes 0..5


@pytest.mark.parametrize("stream", ["draw20", "pool"])
def test_attitude_bar_on_the_gpu_tests_keys(stream):
    """e32 = max |R_f32 - R| on the words the GPU test compares lies well under a quarter of the 1e-5 ceiling (so 4 e32 is a bar, not
    the ceiling), and well above float64 round-off (so it measures float32)."""
    st = RR.start_from_words(_test_words(stream), True, False, C, pool=stream == "pool")
    e32, bar = RR.attitude_bar(st)
    print(f"{stream}: e32 {e32:.3e} bar {bar:.3e}")
    assert 2e-8 < e32 < 1e-6 < 2.5e-6 and bar == 4 * e32
    assert RR.attitude_bar(st, "f32")[1] == bar + 16 * 2.0 ** -24
    assert np.abs(np.swapaxes(st["R_f32"], 1, 2) @ st["R_f32"] - np.eye(3)).max() < 1e-6
    with pytest.raises(AssertionError, match="mis-sized"):
        RR.attitude_bar(dict(R=st["R"], R_f32=st["R"] + 1e-5))


@pytest.mark.parametrize("stream", ["draw20", "pool"])
def test_mutated_restatements_miss_on_the_gpu_tests_keys(stream):
    """Each error the GPU test is there to catch, made in the RESTATEMENT: on the GPU test's own keys the mutant differs from the true
    start in bits (x, v, W, parameters, draws) on nearly every row, or in R by far more than the attitude bar — so a kernel with that
    error fails the comparison."""
    pool = stream == "pool"
    words = _test_words(stream)
    true = RR.start_from_words(words, True, False, C, pool=pool)
    live = ~true["zero"]
    e32, bar = RR.attitude_bar(true)
    gid = np.arange(RR.TEST_N, dtype=np.uint64) + np.uint64(RR.TEST_OFFSETS[1])
    gfirst, slot = (gid // np.uint64(64)) * np.uint64(64), np.arange(RR.TEST_N) % 64

    def start(w):
        return RR.start_from_words(w, True, False, C, pool=pool)

    def rows_differing(a, b, key):
        return ~RR.bits_equal(a[key], b[key]).reshape(RR.TEST_N, -1).all(1)

    # roll and pitch swapped (words 17 and 18): same x, v, W — only R tells
    m = start(words[:, list(range(17)) + [18, 17, 19]])
    assert RR.bits_equal(m["x"], true["x"]).all() and np.abs(m["R"] - true["R"])[live].max(axis=(1, 2)).min() > 100 * bar
    # the quaternion composed in the other order, Rx Ry Rz: within the same angle limits, another matrix
    other = RR.rotation_f64(0 * true["yaw"], true["roll"], 0 * true["yaw"]) @ RR.rotation_f64(0 * true["yaw"], 0 * true["yaw"], true["pitch"]) \
        @ RR.rotation_f64(true["yaw"], 0 * true["yaw"], 0 * true["yaw"])
    assert np.median(np.abs(other - true["R"])[live].max(axis=(1, 2))) > 1000 * bar
    # an error of 1e-5 in a half angle's sine: 2e-5 in the angle
    m = RR.rotation_f64(true["yaw"], true["roll"].astype(np.float64) + 2e-5, true["pitch"])
    assert np.abs(m - true["R"]).max(axis=(1, 2)).min() > 10 * bar
    # x2 reads the word v0 reads
    w9 = words.copy(); w9[:, 8] = w9[:, 9]
    assert rows_differing(start(w9), true, "x")[live].all()
    # a v component scaled by ix instead of reset_v
    m = dict(true); m["v"] = (np.where(true["zero"], F32(0), F32(0.6))[:, None] * sym(words[:, 9:12])).astype(F32)
    assert rows_differing(m, true, "v")[live].all()
    # a parameter row reading its neighbour's word
    wp = words.copy(); wp[:, 1] = wp[:, 2]
    assert rows_differing(start(wp), true, "params").all()
    # scl_z wrong for one role: W not zeroed in the zero-error branch
    wz = words.copy(); wz[:, 15] = 0xFFFFFFFF
    assert rows_differing(start(wz), true, "W")[~live].all() and (~live).sum() > 40
    # the wrong slot's quaternion / the wrong slot altogether, the high word of the seed or of the id dropped
    if pool:
        mutants = [RR.pool_words(RR.TEST_SEED, gfirst, 0, slot + 1), RR.pool_words(RR.TEST_SEED & 0xFFFFFFFF, gfirst, 0, slot),
                   RR.pool_words(RR.TEST_SEED, gfirst, 1, slot)]
        hi = RR.TEST_OFFSETS[2]
        assert not (RR.pool_words(RR.TEST_SEED, gfirst + np.uint64(hi), 0, slot) == RR.pool_words(RR.TEST_SEED, gfirst + np.uint64(hi & 0xFFFFFFFF), 0, slot)).all(1).any()
    else:
        mutants = [RR.draw20_words(RR.TEST_SEED, gid + np.uint64(1), 1), RR.draw20_words(RR.TEST_SEED & 0xFFFFFFFF, gid, 1),
                   RR.draw20_words(RR.TEST_SEED, gid, 2)]
        hi = RR.TEST_OFFSETS[2]
        assert not (RR.draw20_words(RR.TEST_SEED, gid + np.uint64(hi), 1) == RR.draw20_words(RR.TEST_SEED, gid + np.uint64(hi & 0xFFFFFFFF), 1)).all(1).any()
    for w in mutants:
        m = start(w)
        assert rows_differing(m, true, "params").all()
        both = live & ~m["zero"]
        assert rows_differing(m, true, "x")[both].all() and np.abs(m["R"] - true["R"]).max(axis=(1, 2)).min() > 100 * bar
        # slot + 1 with the true slot's x, v, W, parameters: the wrong slot's quaternion alone
        assert np.median(np.abs(m["R"] - true["R"]).max(axis=(1, 2))) > 1e4 * bar
    # word 19 split wrongly: the halves exchanged
    t_true = RR.traj_draws(words[:, 19])
    swapped = ((words[:, 19] >> np.uint64(16)) | (words[:, 19] << np.uint64(16))) & np.uint64(0xFFFFFFFF)
    t_mut = RR.traj_draws(swapped)
    assert all((~RR.bits_equal(a, b)).mean() > 0.99 for a, b in zip(t_true, t_mut))


def test_restated_sincos_small_and_mode0_b1d():
    x = np.concatenate([np.linspace(-4.0, 4.0, 20001), [0.0, np.pi / 4, -np.pi / 4, np.pi / 2, 3.0, -3.0]]).astype(F32)
    sn, cs = RR.sincos_small_f32(x)
    assert sn.dtype == cs.dtype == F32 and sn.shape == x.shape
    assert np.abs(sn - np.sin(x.astype(np.float64))).max() < 2e-7 and np.abs(cs - np.cos(x.astype(np.float64))).max() < 2e-7
    assert sn[-6] == 0 and cs[-6] == 1
    # the two admissible arguments are one rounding apart: mostly the same float, sometimes the neighbour
    w = _test_words("pool")[:, 19]
    ti = np.random.default_rng(2).uniform(-np.pi, np.pi, len(w)).astype(F32)
    (c0, s0), (c1, s1) = RR.mode0_b1d(ti, w)
    same = RR.bits_equal(c0, c1) & RR.bits_equal(s0, s1)
    assert 0.5 < same.mean() < 1.0 and max(np.abs(c0 - c1).max(), np.abs(s0 - s1).max()) < 6e-7
    th = RR.traj_draws(w)[0]
    assert np.abs(c0 - np.cos(ti.astype(np.float64) + th)).max() < 5e-7
