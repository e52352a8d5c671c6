"""CPU: the oracle with its constants moved off their defaults (oracle.quad_oracle.constants).

* pinned against the reference flown with the same values (tools/gen_golden.py coeffs -> tests/golden/onestep_coeffs_{A,B}.npz), at
  the bars test_oracle_golden.py uses for the default vectors: the same functions at the same converged integrator;
* the constants are read when a function is CALLED (dt was once bound when integrate_batch was defined);
* the power of tests/test_gpu_coeffs.py's single-field sweep, decided by the oracle alone: for every field and every output the
  GPU test compares for it, the oracle at the perturbed value and the oracle at the default differ by at least 10 bars, so a
  kernel that ignored the field would fail."""
import math

import numpy as np
import pytest

import coeff_cases as cc
from conftest import grouped_rel_err
from oracle import quad_oracle as orc
from oracle import traj_oracle as trj

KINDS = orc.KINDS
SETS = ("A", "B")


def _snapshot():
    return {k: getattr(orc, k) for k in orc.SETTABLE + orc.DERIVED} | {"NOMINAL_PARAMS": orc.NOMINAL_PARAMS.copy(), "EIGHT": dict(orc.EIGHT)}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a) and a.keys() == b.keys()


def test_constants_sets_derives_and_restores():
    before = _snapshot()
    with orc.constants(CX=5.0, CW12=0.9, CB1=4.0, M_NOM=1.83, J3_NOM=0.041, EIX_LIM=2.3, UDM_PERCENTAGE=17.0, DT=1 / 250, EIGHT=dict(T=7.0, count=0.5)):
        assert orc.CW == orc.CW12 == 0.9 and orc.EIX_LIM == 2.3 and orc.EIB1_LIM == 3.0 and orc.UDM_PERCENTAGE == 17.0
        assert orc.REWARD_MIN == -math.ceil(5.0 + 0.1 + 0.4 + 4.0 + 0.1 + 0.9) and orc.REWARD_MIN_1 == -math.ceil(5.0 + 0.1 + 0.4 + 0.9)
        assert orc.REWARD_MIN_2 == -math.ceil(4.0 + 0.1 + 0.1)
        assert orc.NOMINAL_PARAMS.tolist() == [1.83, 0.23, 0.022, 0.041, 0.0135, 2.2]
        assert trj.EIGHT is orc.EIGHT and trj.EIGHT["T"] == 7.0 and trj.EIGHT["count"] == 0.5 and trj.EIGHT["A1"] == 1.5
        with orc.constants(CW=0.8):   # nested: CW apart from CW12, the rest as the outer block left it
            assert (orc.CW, orc.CW12, orc.CX) == (0.8, 0.9, 5.0) and orc.REWARD_MIN == -math.ceil(5.0 + 0.1 + 0.4 + 4.0 + 0.1 + 0.8)
        assert orc.CW == 0.9
    assert _same(before, _snapshot())
    with pytest.raises(TypeError):
        with orc.constants(X_LIMIT=2.0):
            pass
    try:
        with orc.constants(G=3.71):
            raise RuntimeError
    except RuntimeError:
        pass
    assert _same(before, _snapshot()), "restored when the block raises"


def test_quad_constants_map_onto_the_oracle():
    """Every QuadConstants field reaches an oracle constant, and the defaults of the two tables agree."""
    import dataclasses
    from gym_rotor_amd.constants import QuadConstants
    c = QuadConstants()
    kw = orc.overrides_of(c)
    mapped = set(orc.FROM_QUAD_CONSTANTS) | {"freq"} | {"eight_" + k for k in orc.EIGHT}
    assert {f.name for f in dataclasses.fields(c)} - mapped == {"reward_alive"}    # (a constant 0 the reference never adds)
    before = _snapshot()
    with orc.constants(c):
        now = _snapshot()
    assert all(np.allclose(before[k], now[k], rtol=0, atol=0) if k != "EIGHT" else before[k] == now[k] for k in before), "defaults agree"
    assert kw["DT"] == orc.DT and (c.reward_min, c.reward_min_1, c.reward_min_2) == (orc.REWARD_MIN, orc.REWARD_MIN_1, orc.REWARD_MIN_2)


def test_dt_is_read_at_call_time():
    """Regression: `integrate_batch(..., dt=DT)` and `get_desired_batch(..., dt=DT)` bound DT when they were defined, so a patched DT
    changed the integrator words of the observation and left the ODE step and the goal clock where they were."""
    rng = np.random.default_rng(0)
    s = orc.sample_reset_state(rng, 8)
    a = rng.uniform(-1, 1, (8, 4))
    base = orc.step_batch("coupled", s, a)
    with orc.constants(DT=1 / 400):
        half = orc.step_batch("coupled", s, a)
        y = orc.integrate_batch(s, np.full(8, 20.0), np.zeros((8, 3)), np.full(8, 2.0), np.full(8, 0.02), np.full(8, 0.02), np.full(8, 0.03))
        assert np.array_equal(y, orc.integrate_batch(s, np.full(8, 20.0), np.zeros((8, 3)), np.full(8, 2.0), np.full(8, 0.02), np.full(8, 0.02),
                                                     np.full(8, 0.03), dt=1 / 400))
    v = s[:, 3:6]
    assert np.abs((half["state"][:, 0:3] - s[:, 0:3]) - v / 400).max() < 2e-4 and np.abs((base["state"][:, 0:3] - s[:, 0:3]) - v / 200).max() < 5e-4
    assert np.abs(base["state"][:, 0:3] - half["state"][:, 0:3]).max() > 1e-3
    # the goal generator's clock: 90 calls at 1/400 s are 45 at 1/200 s; the eight-curve table is read when called
    for mode, kw in ((1, dict(t_traj=3.0, w_b1d=0.3)), (6, {})):
        tr_a, tr_b = (trj.traj_start_batch(s, mode, **kw) for _ in range(2))
        for _ in range(45):
            ga = trj.get_desired_batch(tr_a, s)
        with orc.constants(DT=1 / 400):
            for _ in range(90):
                gb = trj.get_desired_batch(tr_b, s)
        assert all(np.allclose(x, y, rtol=0, atol=1e-12) for x, y in zip(ga, gb)), mode
    tr_a, tr_b = (trj.traj_start_batch(s, 6) for _ in range(2))
    with orc.constants(EIGHT=dict(T=7.0, A1=1.2)):
        ga = trj.get_desired_batch(tr_a, s)
    gb = trj.get_desired_batch(tr_b, s, eight=dict(T=7.0, A1=1.2))
    assert all(np.array_equal(x, y) for x, y in zip(ga, gb)) and not np.array_equal(ga[0], trj.get_desired_batch(trj.traj_start_batch(s, 6), s)[0])
    # RefEnv integrates over the DT of the call as well
    e = orc.RefEnv("coupled"); e.state = s[0].copy()
    with orc.constants(DT=1 / 400):
        e.step(a[0])
    assert np.abs(e.state - half["state"][0]).max() < 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# against the reference flown with the same values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SETS)
def test_step_batch_matches_the_reference_under_coefficient_sets(name, kind, golden):
    """test_step_batch_matches_reference_onestep at its own bars, on the sets' vectors."""
    g = golden(f"onestep_coeffs_{name}")
    d = cc.of_kind(g, kind)
    c, udm, cw, kw = cc.coeff_set(g)
    with orc.constants(**kw):
        o = orc.step_batch(kind, d["state"], d["action"], d["params"], d["goal"], d["integ"])
        # what the fixture promises of itself (tools/gen_golden.py): parameters within the set's UDM range of the set's nominals,
        # straddling rows at least 1e-4 from a threshold
        rel = d["params"] / orc.NOMINAL_PARAMS - 1.0
        assert (np.abs(rel) <= udm / 100 * np.array([1, 1, 1, 1, 1, 0.5]) + 1e-6).all() and np.abs(rel).max() > 0.8 * udm / 100
        assert cc.done_margin(kind, o).min() >= 1e-4
    assert np.abs(o["state"] - d["next_state"]).max() <= 1e-13
    assert np.abs(o["f"] - d["f"]).max() <= 1e-13 and np.abs(o["M"] - d["M"]).max() <= 1e-13
    for k, ob in enumerate(o["obs"]):
        ref = d[f"obs{k}"]
        if kind == "quad":
            assert np.abs(ob - ref).max() <= 1e-13
        else:
            assert ob.dtype == np.float32 and np.array_equal(ob, ref)
    assert np.abs(o["reward_raw"] - d["reward_raw"]).max() <= 4e-6
    assert np.abs(o["reward"] - d["reward"]).max() <= 3e-7
    assert np.array_equal(o["done"], d["done"]) and d["done"].any() and not d["done"].all()
    assert np.abs(o["integ"] - d["next_integ"]).max() <= 1e-14


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SETS)
def test_refenv_matches_the_reference_under_coefficient_sets(name, kind, golden):
    """test_refenv_single_matches_reference_onestep at its own bars, on the sets' vectors."""
    g = golden(f"onestep_coeffs_{name}")
    d = cc.of_kind(g, kind)
    with orc.constants(**cc.coeff_set(g)[3]):
        for i in range(0, 128, 5):
            e = orc.RefEnv(kind, d["params"][i])
            e.state = d["state"][i].copy(); e.set_goal(d["goal"][i]); e.set_integ(d["integ"][i])
            obs, r, dn, trunc, info = e.step(d["action"][i])
            assert np.abs(e.state - d["next_state"][i]).max() <= 1e-14
            assert np.allclose(r, d["reward"][i], atol=1e-15) and list(dn) == list(d["done"][i])
            assert np.allclose(e.last_raw, d["reward_raw"][i], atol=0, rtol=0)
            for k, ob in enumerate([obs] if kind == "quad" else obs):
                assert np.array_equal(np.asarray(ob, dtype=np.float64), d[f"obs{k}"][i].astype(np.float64))
            assert np.abs(e.get_integ() - d["next_integ"][i]).max() <= 1e-15


@pytest.mark.parametrize("name", SETS)
def test_error_obs_matches_the_reference_under_coefficient_sets(name, golden):
    """error_obs_batch in either format: float32 rows bit for bit, integrator words to 1e-14 (test_oracle_golden's bars)."""
    g = golden(f"onestep_coeffs_{name}")
    with orc.constants(**cc.coeff_set(g)[3]):
        for kind, fw, nk in (("coupled", "MONO", 1), ("decoupled", "MODUL", 2)):
            o = orc.error_obs_batch(kind, g["errobs_state"], g["errobs_goal"], g["errobs_integ"])
            for k in range(nk):
                assert np.array_equal(o["obs"][k], g[f"errobs_{fw}_obs{k}"]), (fw, k)
            assert np.abs(o["integ"] - g[f"errobs_{fw}_next_integ"]).max() <= 1e-14


@pytest.mark.parametrize("name", SETS)
def test_coefficient_sets_can_show_a_swap(name, golden):
    """No two neighbours of QrCoeffs hold the same value in a set, and no field is at its default."""
    from gym_rotor_amd import _lib
    from gym_rotor_amd.constants import QuadConstants
    c, udm, cw, _ = cc.coeff_set(golden(f"onestep_coeffs_{name}"))
    val = dict(CW=cw, dt=c.dt, euler_lim_deg=c.euler_lim, udm_fraction=udm / 100, w_adapt=16.0)
    order = [n for n, _ in _lib.QrCoeffs._fields_]
    vals = [val[n] if n in val else getattr(c, n) for n in order]
    assert all(a != b for a, b in zip(vals, vals[1:])), [(n, v) for n, v in zip(order, vals)]
    dflt = QuadConstants()
    dval = dict(CW=dflt.CW, dt=dflt.dt, euler_lim_deg=dflt.euler_lim, udm_fraction=0.1)
    assert all(v != (dval[n] if n in dval else getattr(dflt, n)) for n, v in zip(order, vals) if n != "w_adapt")
    down = name == "A"
    assert all((abs(v) < abs(dval[n] if n in dval else getattr(dflt, n))) == down for n, v in zip(order, vals) if n not in ("w_adapt", "dt", "udm_fraction"))


# ---------------------------------------------------------------------------------------------------------------------
# power of the GPU sweep
# ---------------------------------------------------------------------------------------------------------------------
def _difference(kind, out, a, b, c):
    """How far two oracle results are apart in `out`, in units of the bar the GPU test applies to it."""
    if out == "state":
        return grouped_rel_err(a["state"], b["state"]) / max(cc.ONESTEP_TOL.values())
    if out == "obs":
        return max((np.abs(x.astype(np.float64) - y.astype(np.float64)) / np.maximum(np.abs(y), 1.0) / bar).max()
                   for x, y, bar in zip(a["obs"], b["obs"], cc.obs_bars(kind, c)))
    if out == "integ":
        return np.abs(a["integ"] - b["integ"]).max() / cc.INTEG_TOL
    if out == "reward_raw":
        return np.abs(a["reward_raw"] - b["reward_raw"]).max() / (cc.RAW_TOL * max(1.0, np.abs(a["reward_raw"]).max()))
    if out == "reward":
        same = a["done"] == b["done"]
        return np.abs(a["reward"] - b["reward"])[same].max() / cc.REWARD_TOL
    assert out == "done"   # rows that decide differently OUTSIDE the window in which a difference is excused, against one such row
    differs = (a["done"] != b["done"]).any(1) & (a["margin"] >= 10 * cc.DONE_WINDOW)
    return 10.0 * differs.sum()


@pytest.mark.parametrize("name", list(cc.FIELDS))
def test_power_of_the_single_field_sweep(name):
    """For each field, each kind that reads it and each output listed for it: ignoring the field moves that output by >= 10 bars."""
    _, _, consumers = cc.FIELDS[name]
    c = cc.quad_constants(name)
    for kind, outs in consumers.items():
        for per_env in ((False,) if name in cc.NOMINAL_FIELDS else (False, True)):
            with orc.constants(**cc.oracle_kw(name)):
                d = cc.sweep_inputs(kind, name, per_env)
                a = orc.step_batch(kind, d["state"], d["action"], d["params"], d["goal"], d["integ"])
                a["margin"] = cc.done_margin(kind, a)
                assert (d["ulp"].sum() == len(cc.ULP_ROWS)) == (name in ("x_lim", "v_lim"))
                if d["ulp"].any():   # the ulp rows sit where they were put: inside the window, on both sides
                    col, lim = (0, orc.X_LIM) if name == "x_lim" else (3, orc.V_LIM)
                    off = (a["state"][d["ulp"], col] - lim) / float(np.spacing(np.float32(lim)))
                    assert np.abs(off - np.array(cc.ULP_ROWS)).max() <= 0.51 and (off > 0).any() and (off < 0).any()
            b = orc.step_batch(kind, d["state"], d["action"], d["params"], d["goal"], d["integ"])   # the field (alone) back at its default
            for out in outs:
                diff = _difference(kind, out, a, b, c)
                assert diff >= 10.0, f"{name} / {kind} / {out} / per-env params {per_env}: only {diff:.2f} bars"


@pytest.mark.parametrize("name", SETS)
def test_power_of_the_reset_and_goal_tests(name, golden):
    """udm_fraction and the eight-curve values are read by no single step: their consumers are the reset samplers and the goal
    generator, flown under sets A and B.  Decided by the oracle alone: each of these fields, put back to its default within the
    set, moves what those tests compare by >= 10 of their bars — the parameter spread (3 % of width / sqrt 3) and the goal words of
    the eight curve flown to 1.5 times its end (3e-6 relative to max(1, largest value of the word)); dt likewise."""
    c, udm, cw, kw = cc.coeff_set(golden(f"onestep_coeffs_{name}"))
    spread = lambda: (orc.sample_params(np.random.default_rng(1), 100000) / orc.NOMINAL_PARAMS - 1.0).std(0)
    with orc.constants(**kw):
        a = spread()
        with orc.constants(UDM_PERCENTAGE=10.0):
            b = spread()
    assert (np.abs(a / b - 1.0) >= 10 * 0.03).all(), a / b
    s = orc.sample_reset_state(np.random.default_rng(2), 16)

    def fly(calls, **back):
        with orc.constants(**dict(kw, **back)):
            tr = trj.traj_start_batch(s, 6)
            return np.stack([np.concatenate(trj.get_desired_batch(tr, s), 1) for _ in range(calls)])

    calls = int(1.5 * c.eight_count * c.eight_T * c.freq)
    want = fly(calls)
    scale = np.maximum(1.0, np.abs(want).max((0, 1)))
    for key, default in {**{"EIGHT." + k: v for k, v in orc.EIGHT.items()}, "DT": orc.DT}.items():
        back = {"DT": default} if key == "DT" else {"EIGHT": dict(kw["EIGHT"], **{key[6:]: default})}
        diff = (np.abs(fly(calls, **back) - want) / scale).max() / 3e-6
        assert diff >= 10.0, f"set {name}: {key} back at its default moves the goal by only {diff:.2f} bars"


def test_every_untested_field_is_in_the_sweep():
    """The cap on what may be left out: every field no GPU test moved before is listed for at least one consumer in the sweep;
    udm_fraction and the eight-curve values, which no single step reads: test_power_of_the_reset_and_goal_tests."""
    from gym_rotor_amd.constants import QuadConstants
    moved = set()
    for name, (kw, extra, consumers) in cc.FIELDS.items():
        if any(consumers.values()):
            moved |= {k for k, v in kw.items() if v != getattr(QuadConstants(), k)} | set(extra)
    assert {"freq", "v_lim", "W_lim", "euler_lim", "eIx_lim", "eIb1_lim", "beta", "CIx", "CIb1", "m_nominal", "d_nominal", "J1_nominal",
            "J3_nominal", "c_tf_nominal", "c_tw_nominal", "g", "min_force", "CW", "x_lim"} <= moved
