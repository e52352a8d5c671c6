"""Cases shared by tests/test_oracle_coeffs.py (CPU) and tests/test_gpu_coeffs.py (GPU): the single-field table, the inputs of a
case, the bars, and the two all-fields sets as tests/golden/onestep_coeffs_{A,B}.npz carries them.  Everything here is NumPy and
the oracle: no GPU, no reference."""
import dataclasses

import numpy as np

from oracle import quad_oracle as orc

KINDS = orc.KINDS
WRAPPERS = ("coupled", "decoupled")
f32r = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)   # float32-representable float64

# ---------------------------------------------------------------------------------------------------------------------
# bars (none of them new: test_gpu_parity.py)
# ---------------------------------------------------------------------------------------------------------------------
ONESTEP_TOL = {("f64", 1): 2e-8, ("mixed", 1): 2e-7, ("mixed", 2): 2e-7}   # ONESTEP_TOL / test_onestep_golden_magnus_substeps
VARIANTS = tuple(ONESTEP_TOL)          # (layout, substeps); ("mixed", 2) is the Magnus substep
OBS_TOL, INTEG_TOL, RAW_TOL, REWARD_TOL = 2e-6, 2e-6, 1e-5, 1e-5
DONE_WINDOW, DONE_CAP = 1e-6, 0.02     # a done flag may differ within 1e-6 (relative to its limit) of a threshold; at most 2 % of the rows

DEFAULT_LIMS = dict(x_lim=1.0, v_lim=4.0, W_lim=2.0 * np.pi, eIx_lim=3.0, eIb1_lim=3.0)


def obs_word_limits(kind):
    """Per observation row: which limit each word was divided by (wrapper_utils.py:3-29); None: a word with no limit in it."""
    x, ix, v, w, ib = ["x_lim"] * 3, ["eIx_lim"] * 3, ["v_lim"] * 3, ["W_lim"] * 3, ["eIb1_lim"]
    if kind == "coupled":
        return [x + ix + v + [None] * 9 + [None] + ib + w]
    return [x + ix + v + [None] * 3 + w, [None] + ib + ["W_lim"]]


def obs_bars(kind, c):
    """OBS_TOL per word.  A word is q / limit and q's own absolute error (float32 state, float32 integrator word) does not change
    with the limit, so under a smaller limit the word's error grows by default_limit / limit; a larger limit leaves the bar."""
    return [np.array([OBS_TOL * (1.0 if w is None else max(1.0, DEFAULT_LIMS[w] / getattr(c, w))) for w in row]) for row in obs_word_limits(kind)]


# ---------------------------------------------------------------------------------------------------------------------
# the single-field table: one field off its default per case
# ---------------------------------------------------------------------------------------------------------------------
# name -> (QuadConstants overrides, extra oracle overrides, {kind: outputs that must move by >= 10 bars when the field is ignored})
# A kind that does not read the field is absent (it is not flown for that field); `nominal` fields are read only by envs without a
# parameter buffer, so their power is judged on the nominal half of the cases.
_ALL = lambda outs: {k: outs for k in KINDS}
_WRAP = lambda outs: {k: outs for k in WRAPPERS}
_LIM = lambda: dict(quad=("done",), coupled=("obs", "reward_raw", "done"), decoupled=("obs", "reward_raw", "done"))
FIELDS = {
    "freq250": (dict(freq=250), {}, dict(quad=("state",), coupled=("state", "obs", "integ", "reward_raw"), decoupled=("state", "obs", "integ", "reward_raw"))),
    "freq400": (dict(freq=400), {}, dict(quad=("state",), coupled=("state", "obs", "integ", "reward_raw"), decoupled=("state", "obs", "integ", "reward_raw"))),
    "x_lim": (dict(x_lim=0.7), {}, _LIM()),
    "v_lim": (dict(v_lim=3.3), {}, _LIM()),
    "W_lim": (dict(W_lim=5.1), {}, _LIM()),
    "euler_lim": (dict(euler_lim=62.0), {}, dict(quad=("done",))),
    "eIx_lim": (dict(eIx_lim=2.3), {}, _WRAP(("obs", "reward_raw"))),
    "eIb1_lim": (dict(eIb1_lim=1.7), {}, _WRAP(("obs", "reward_raw"))),
    "beta": (dict(beta=0.11), {}, _WRAP(("obs", "integ"))),
    "CIx": (dict(CIx=0.35), {}, _WRAP(("reward_raw", "reward"))),
    "CIb1": (dict(CIb1=0.45), {}, _WRAP(("reward_raw", "reward"))),
    "m_nominal": (dict(m_nominal=1.83), {}, _ALL(("state",))),
    "d_nominal": (dict(d_nominal=0.19), {}, dict(quad=("state",))),
    "J1_nominal": (dict(J1_nominal=0.027), {}, _ALL(("state",))),
    "J3_nominal": (dict(J3_nominal=0.041), {}, _ALL(("state",))),
    "c_tf_nominal": (dict(c_tf_nominal=0.0171), {}, dict(quad=("state",))),
    "c_tw_nominal": (dict(c_tw_nominal=2.6), {}, _ALL(("state",))),
    "g": (dict(g=3.71), {}, _ALL(("state",))),
    "min_force": (dict(min_force=0.9), {}, _ALL(("state",))),
    # CW apart from Cw12 (the ABI allows it; QuadConstants ties them): set on env._cenv.coeffs.  Quad-v0 and the coupled wrapper read
    # CW, the decoupled one Cw12: it is flown too (a kernel reading CW there would miss), with no power claimed for it.
    "CW": (dict(Cw12=0.6), dict(CW=0.8), dict(quad=("reward_raw", "reward"), coupled=("reward_raw", "reward"), decoupled=())),
}
NOMINAL_FIELDS = ("m_nominal", "d_nominal", "J1_nominal", "J3_nominal", "c_tf_nominal", "c_tw_nominal")
UDM_SWEEP = 13.0   # the percentage the per-env parameters of the sweep are drawn with (udm_fraction off its default as well)


def quad_constants(name):
    from gym_rotor_amd.constants import QuadConstants
    return QuadConstants(**FIELDS[name][0])


def oracle_kw(name):
    return orc.overrides_of(quad_constants(name), UDM_PERCENTAGE=UDM_SWEEP, **FIELDS[name][1])


# ---------------------------------------------------------------------------------------------------------------------
# inputs of a case
# ---------------------------------------------------------------------------------------------------------------------
def state_in(s):
    """x, v, W float32-representable, R an exact float64 rotation (as tools/gen_golden.py: state_in)."""
    s = np.array(s, dtype=np.float64)
    R = np.swapaxes(s[:, 6:15].reshape(-1, 3, 3), 1, 2)
    U, _, Vt = np.linalg.svd(R)
    out = f32r(s)
    out[:, 6:15] = np.swapaxes(U @ Vt, 1, 2).reshape(-1, 9)
    return out


def _boundary(rng, n):
    """Starts straddling each termination threshold AS IT STANDS in the oracle (call under orc.constants), within +-2 %; the component
    and the side cycle with the row index, so that every threshold is met by each component on either side."""
    s = orc.sample_reset_state(rng, n, "train")
    for i in range(n):
        which, j, sgn = i % 5, (i // 5) % 3, rng.choice([-1.0, 1.0])
        eps = rng.uniform(0.001, 0.02) * (1.0 if (i // 15) % 2 == 0 else -1.0)
        if which < 3:
            s[i, (0, 3, 15)[which] + j] = sgn * (orc.X_LIM, orc.V_LIM, orc.W_LIM)[which] * (1.0 + eps)
        else:
            ang = np.deg2rad(orc.EULER_LIM_DEG * (1.0 + eps))
            roll, pitch = (sgn * ang, rng.uniform(-0.3, 0.3)) if which == 3 else (rng.uniform(-0.3, 0.3), sgn * ang)
            s[i, 6:15] = orc.euler_xyz_to_R(roll, pitch, rng.uniform(-np.pi, np.pi)).reshape(9, order="F")
            s[i, 15:18] *= 0.05
    return s


ULP_ROWS = (1, -1, 2, -2, 3, -3, 4, -4, 5, -5)   # float32 ulps off the limit, next state, one row each


def sweep_inputs(kind, name, per_env_params, n=192, seed=0):
    """Inputs of one single-field case, drawn under the perturbed constants (call under orc.constants(**oracle_kw(name))): starts
    scaled to the perturbed limits (a quarter straddling the thresholds), non-zero integrator words, random goals with non-zero Wd
    on half the rows, saturated commands on every seventh; per-env parameters around the perturbed nominals or None (nominal).
    For x_lim / v_lim the last len(ULP_ROWS) rows are moved so that the NEXT state's first position / velocity component sits a
    few float32 ulps on either side of the limit (x and v enter their own derivative nowhere: a shift of the start shifts the end)."""
    rng = np.random.default_rng(7000 + 13 * KINDS.index(kind) + 101 * list(FIELDS).index(name) + seed)
    A, nb = orc.ACTION_DIM[kind], n // 4
    state = state_in(np.concatenate([orc.sample_reset_state(rng, n - nb, "train"), _boundary(rng, nb)]))
    action = f32r(rng.uniform(-1, 1, (n, A)))
    action[::7] = f32r(np.sign(action[::7]))
    params = f32r(orc.sample_params(rng, n, "train")) if per_env_params else None
    goal = np.tile(orc.DEFAULT_GOAL, (n, 1))
    psi = rng.uniform(-np.pi, np.pi, n)
    rnd = np.concatenate([rng.uniform(-0.3, 0.3, (n, 3)) * orc.X_LIM, rng.uniform(-0.5, 0.5, (n, 3)), np.cos(psi)[:, None], np.sin(psi)[:, None],
                          np.zeros((n, 1)), rng.uniform(-0.5, 0.5, (n, 3))], 1)
    goal[::2] = f32r(rnd)[::2]
    goal[n - nb:] = orc.DEFAULT_GOAL      # (the straddling rows straddle the state's thresholds: no goal offset on them)
    integ = np.concatenate([rng.uniform(-1.0, 1.0, (n, 6)), rng.uniform(-2.0, 2.0, (n, 1)), rng.uniform(-3.0, 3.0, (n, 1))], 1)
    integ[::5, 0:3] = rng.uniform(-4.0, 4.0, (len(integ[::5]), 3)); integ[::9, 6] = rng.uniform(-4.0, 4.0, len(integ[::9]))
    integ = np.zeros((n, 8)) if kind == "quad" else f32r(integ)
    ulp = np.zeros(n, bool)
    if name in ("x_lim", "v_lim"):
        col, lim = (0, orc.X_LIM) if name == "x_lim" else (3, orc.V_LIM)
        rows = np.arange(n - nb - len(ULP_ROWS), n - nb)            # (in-regime starts, not the straddling quarter)
        goal[rows] = orc.DEFAULT_GOAL
        nxt = orc.step_batch(kind, state[rows], action[rows], None if params is None else params[rows], goal[rows], integ[rows])["state"]
        target = lim + np.array(ULP_ROWS) * float(np.spacing(np.float32(lim)))
        state[rows, col] = f32r(state[rows, col] + (target - nxt[:, col]))
        ulp[rows] = True
    return dict(state=state, action=action, params=params, goal=goal, integ=integ, ulp=ulp)


def done_margin(kind, out):
    """Per row: distance of the nearest deciding quantity of the done rule from its threshold, relative to its limit, on an oracle
    result (call under the constants it was made with).  _done_mismatch_ok of test_gpu_parity.py, at the limits as they stand."""
    s = out["state"]
    q = [s[:, 0:3] / orc.X_LIM, s[:, 3:6] / orc.V_LIM, s[:, 15:18] / orc.W_LIM]
    if kind == "quad":
        R = np.swapaxes(s[:, 6:15].reshape(-1, 3, 3), 1, 2)
        q.append(np.degrees(np.arctan2(R[:, 2, 1], R[:, 2, 2]))[:, None] / orc.EULER_LIM_DEG)
        q.append(np.degrees(-np.arcsin(np.clip(R[:, 2, 0], -1.0, 1.0)))[:, None] / orc.EULER_LIM_DEG)
    else:
        o = [x.astype(np.float64) for x in out["obs"]]
        q += [o[0][:, 0:3], o[0][:, 6:9], o[0][:, 20:23]] if kind == "coupled" else [o[0][:, 0:3], o[0][:, 6:9], o[0][:, 12:15], o[1][:, 2:3]]
    return np.abs(np.abs(np.concatenate(q, 1)) - 1.0).min(1)


# ---------------------------------------------------------------------------------------------------------------------
# the two all-fields sets, as the fixture carries them
# ---------------------------------------------------------------------------------------------------------------------
def coeff_set(d):
    """(QuadConstants, UDM percentage, CW, oracle overrides) from onestep_coeffs_*.npz: coeff_names / coeff_values."""
    from gym_rotor_amd.constants import QuadConstants
    v = dict(zip((str(k) for k in d["coeff_names"]), (float(x) for x in d["coeff_values"])))
    cw = v.pop("CW")
    fields = {f.name: f.type for f in dataclasses.fields(QuadConstants)}
    assert set(v) <= set(fields), set(v) - set(fields)
    v["freq"] = int(v["freq"])
    c = QuadConstants(**v)
    return c, c.UDM_percentage, cw, orc.overrides_of(c, CW=cw)


def of_kind(d, kind):
    """The `kind` block of onestep_coeffs_*.npz in the layout of onestep_{kind}.npz."""
    out = {k[len(kind) + 1:]: v for k, v in d.items() if k.startswith(kind + "_")}
    for k in ("action", "params", "goal", "integ"):     # (stored as float32: they are float32 numbers)
        out[k] = out[k].astype(np.float64)
    return out
