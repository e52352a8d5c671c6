"""NumPy restatement of in-loop action selection (qr_rollout_actor; gym_rotor_amd/csrc/qr_step.h, qr_actor.h): the exploration noise
the step kernel draws for itself, element by element, and the two action rules of `actor_sample` from given head outputs.

The noise of env i at step t of a launch is Philox4x32-10 (tests/noise_ref.py: `philox4`, all four words) under the key
(seed_lo, seed_hi) with the counter
    (gid_lo, gid_hi ^ step_hi, step_lo, 0x80000000 | block),   gid = env_offset + i,   step = step_base + t  (mod 2^64),
components 0..3 = Box-Muller on block 0's word pairs (0, 1) and (2, 3) (`noise_ref.normals_from_words`: the kernel's float32 inputs,
the functions in float64), component 4 (Decoupled) = position 0 of block 1.  The plain wave draws them where it needs them, the
helper wave one step ahead into a two-slot LDS buffer — the same values.

The rules are float64 and are the oracle's (oracle/actor_oracle.py: `choose_action`, `sac_sample`) with the network taken away:
tests/test_action_ref_host.py holds the two together to 1e-12 on random networks."""
import numpy as np

import noise_ref as NR

LOG_SQRT_2PI = 0.9189385332046727
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
ROLLOUT_BIT = 0x80000000
U64 = 2 ** 64 - 1


def rollout_words(seed: int, gid, step, block: int):
    """uint64 [..., 4] (32-bit values): the Philox words of `block` for arrays (or scalars, broadcast) of global env ids and global
    steps, both below 2^64."""
    gid, step = np.broadcast_arrays(np.asarray(gid, dtype=np.uint64), np.asarray(step, dtype=np.uint64))
    s32 = np.uint64(32)
    w = NR.philox4(gid & NR.U32, (gid >> s32) ^ (step >> s32), step & NR.U32, ROLLOUT_BIT | block, seed)
    return np.moveaxis(w, 0, -1)


def eps_from_blocks(w0, w1, A: int, fifth: int = 0):
    """float64 [..., A] from the words [..., 4] of blocks 0 and 1: four normals of block 0, then (A = 5) normal `fifth` of block 1."""
    shape = w0.shape[:-1]
    z = NR.normals_from_words(w0.reshape(-1, 4)).reshape(shape + (4,))
    if A == 4:
        return z
    z1 = NR.normals_from_words(w1.reshape(-1, 4)).reshape(shape + (4,))
    return np.concatenate([z, z1[..., fifth:fifth + 1]], -1)


def rollout_ids(env_offset: int, n: int, step_base: int, T: int):
    """(gid uint64 [1, n], step uint64 [T, 1]): the key's two 64-bit words for every element of a launch of T steps over n envs; the
    step wraps at 2^64 like the kernel's unsigned sum."""
    gid = np.array([(env_offset + i) & U64 for i in range(n)], dtype=np.uint64)[None, :]
    step = np.array([(step_base + t) & U64 for t in range(T)], dtype=np.uint64)[:, None]
    return gid, step


def rollout_eps(seed: int, env_offset: int, n: int, step_base: int, T: int, A: int):
    """float64 [T, n, A]: what rollout_actor(actors, T) draws for envs env_offset .. env_offset + n - 1 from stream position step_base."""
    if A not in (4, 5):
        raise ValueError("A must be 4 (coupled) or 5 (decoupled)")
    gid, step = rollout_ids(env_offset, n, step_base, T)
    return eps_from_blocks(rollout_words(seed, gid, step, 0), rollout_words(seed, gid, step, 1), A)


# ---------------------------------------------------------------------------------------------------------------------
# the two rules of actor_sample, from the heads' outputs (pre = the mean head before any squashing)
# ---------------------------------------------------------------------------------------------------------------------
def tanh_mean_rule(pre, log_std, eps, max_action=1.0, clamp_log_std=False):
    """QR_ACTOR_TANH_MEAN (PPO.choose_action, TD3.choose_action): mean = tanh(pre); a = clip(mean + exp(log_std) eps, +-max_action);
    logp = Normal(mean, std).log_prob of the CLAMPED action, per component.  eps None: the deterministic action clip(mean).
    clamp_log_std: log_std is a head's output and is clamped to [-20, 2] first.  Returns (action, logp, mean)."""
    mean = np.tanh(np.asarray(pre, dtype=np.float64))
    ls = np.asarray(log_std, dtype=np.float64)
    if clamp_log_std:
        ls = np.clip(ls, LOG_STD_MIN, LOG_STD_MAX)
    ls = np.broadcast_to(ls, mean.shape)
    std = np.exp(ls)
    raw = mean if eps is None else mean + std * np.asarray(eps, dtype=np.float64)
    action = np.clip(raw, -max_action, max_action)
    logp = -((action - mean) ** 2) / (2.0 * std ** 2) - ls - LOG_SQRT_2PI
    return action, logp, mean


def tanh_sample_rule(pre, log_std, eps):
    """QR_ACTOR_TANH_SAMPLE (MLP_Actor_SAC.sample): log_std clamped to [-20, 2]; u = pre + exp(log_std) eps; a = tanh(u);
    logp = Normal(pre, std).log_prob(u) - log(1 - a^2 + 1e-6).  eps None: a = tanh(pre), logp with z = 0.
    Returns (action, logp, u, clamped log_std)."""
    pre = np.asarray(pre, dtype=np.float64)
    ls = np.broadcast_to(np.clip(np.asarray(log_std, dtype=np.float64), LOG_STD_MIN, LOG_STD_MAX), pre.shape)
    std = np.exp(ls)
    u = pre if eps is None else pre + std * np.asarray(eps, dtype=np.float64)
    action = np.tanh(u)
    logp = -((u - pre) ** 2) / (2.0 * std ** 2) - ls - LOG_SQRT_2PI - np.log(1.0 - action ** 2 + 1e-6)
    return action, logp, u, ls


def sac_logp_from_action(log_std, eps, a):
    """The log-prob the kernel should report GIVEN the action it reported: -z^2 / 2 - ls - log sqrt(2 pi) - log(1 - a^2 + 1e-6), a the
    float32 number returned (widened exactly), everything else float64; log_std is the clamped one.  Unlike the rule's own logp this
    is well conditioned at |a| -> 1: the squash term is a function of the returned a, not of u."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    z = np.zeros_like(a) if eps is None else np.asarray(eps, dtype=np.float64)
    return -0.5 * z * z - np.asarray(log_std, dtype=np.float64) - LOG_SQRT_2PI - np.log(1.0 - a * a + 1e-6)


def normal_logp_from_action(mean, log_std, a):
    """TANH_MEAN's counterpart: Normal(mean, exp(log_std)).log_prob of the returned float32 action about the float64 mean."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    ls = np.asarray(log_std, dtype=np.float64)
    z = (a - np.asarray(mean, dtype=np.float64)) * np.exp(-ls)
    return -0.5 * z * z - ls - LOG_SQRT_2PI


# ---------------------------------------------------------------------------------------------------------------------
# the keys tests/test_gpu_action_noise.py runs (tests/test_action_ref_host.py shows that they tell every wrong key apart)
# ---------------------------------------------------------------------------------------------------------------------
NOISE_N = 64 * 2 + 5                      # two full tiles and a ragged one
NOISE_SEED = 2 ** 40 + 3                  # a seed with a high word
NOISE_OFFSET = 2 ** 32 + 192              # a global env id with a high word; a multiple of 64 (in-launch resets)
NOISE_STEPS = 2 ** 32 - 2                 # the loaded stream position: the step word's 32-bit boundary is crossed at t = 2
NOISE_SPLITS = (3, 2)                     # ... inside the first launch; the second starts beyond it
NOISE_OTHER_SEED = 2 ** 47 + 11           # the explicit noise_seed= case (the env's own seed stays NOISE_SEED)


# ---------------------------------------------------------------------------------------------------------------------
# the edge grids of tests/test_gpu_action_rules.py: head outputs (as the float32 biases the device reads) and injected eps
# ---------------------------------------------------------------------------------------------------------------------
RULE_N = 133
PRE = (0.0, 0.3, -0.3, 2.0, -2.0, 5.0, -5.0, 9.0, -9.0, 20.0, -20.0)       # tanh through 1 - 2^-24 (|pre| = 9), exactly 1.0f and beyond
SAC_LS = (-25.0, -20.0, -19.999, -5.0, 0.0, 1.999, 2.0, 3.0)               # the clamp acts at -20 and 2 and nowhere else
MEAN_LS = (-20.0, -5.0, -1.0, 0.0, 1.0)                                    # the parameter form: unclamped
MAX_ACTIONS = (1.0, 0.5, 0.05)
BASE_EPS = (0.0, 2.0 ** -20, -2.0 ** -20, 0.5, -0.5, 1.0, -1.0, 3.0, -3.0, 5.9, -5.9)
# where float32 tanh leaves the last values below one: tanh(u) = 1 - 2^-24 (the largest float32 below 1) and 1 - 2^-25 (the midpoint
# to 1.0f, beyond which the correctly rounded value IS 1.0f)
U_EDGES = tuple(s * float(np.arctanh(1.0 - 2.0 ** -k)) for k in (24, 25) for s in (1.0, -1.0))


def f32(x):
    return np.asarray(x, dtype=np.float32)


def _around(e):
    """A float64 value as the nearest float32 and that number's two neighbours: on, one ulp inside and one ulp outside."""
    e = np.float32(e)
    return [np.nextafter(e, np.float32(-np.inf)), e, np.nextafter(e, np.float32(np.inf))]


def combos(ls_values):
    """Every (log_std, pre) pair, log_std-major, as float32 numbers."""
    return [(np.float32(ls), np.float32(p)) for ls in ls_values for p in PRE]


def bias_sets(ls_values, A: int):
    """The launches of one grid: per launch A (log_std, pre) pairs, one per action component.  Components 0..3 (the MFMA actor) walk
    the whole product, four pairs a launch; component 4 (Decoupled's VALU / LDS actor) takes pair (j mod #log_std, j mod 11) in launch
    j — 11 is prime to 5 and to 8, and there are at least 11 launches, so it meets every log_std and every pre."""
    c = combos(ls_values)
    n_launch = (len(c) + 3) // 4
    assert n_launch >= len(PRE) and n_launch >= len(ls_values)
    sets = []
    for j in range(n_launch):
        row = [c[(4 * j + k) % len(c)] for k in range(4)]
        if A == 5:
            row.append(c[(j % len(ls_values)) * len(PRE) + j % len(PRE)])
        sets.append(row)
    return sets


def eps_column(rule: str, ls, pre, max_action=1.0, fill_seed=0):
    """float32 [RULE_N]: the injected draws of one component whose heads give (pre, ls): BASE_EPS, then the values that put
    u = pre + sd eps (rule 'sample': on each of U_EDGES) or mean + sd eps (rule 'mean': on +-max_action) on the boundary, one ulp
    inside and one ulp outside, then fixed standard normals up to RULE_N.  sd = exp of the CLAMPED log_std for 'sample' and for
    'mean_head', of the log_std as given for 'mean'."""
    ls, pre = float(ls), float(pre)
    if rule != "mean":
        ls = min(max(ls, LOG_STD_MIN), LOG_STD_MAX)
    sd = np.exp(ls)
    col = [np.float32(e) for e in BASE_EPS]
    if rule == "sample":
        for ue in U_EDGES:
            col += _around((ue - pre) / sd)
    else:
        for b in (float(np.float32(max_action)), -float(np.float32(max_action))):
            col += _around((b - np.tanh(pre)) / sd)
    rng = np.random.default_rng(1000 + fill_seed)
    col += list(rng.standard_normal(RULE_N - len(col)).astype(np.float32))
    out = np.array(col, dtype=np.float32)
    assert out.shape == (RULE_N,) and np.isfinite(out).all()
    return out


def rule_launch(rule: str, row, max_action=1.0, index=0):
    """One launch of a grid: (pre float32 [A], ls float32 [A], eps float32 [1, RULE_N, A]) for the bias set `row`."""
    ls = np.array([r[0] for r in row], dtype=np.float32)
    pre = np.array([r[1] for r in row], dtype=np.float32)
    eps = np.stack([eps_column(rule, l, p, max_action, fill_seed=17 * index + k) for k, (l, p) in enumerate(row)], 1)[None]
    return pre, ls, np.ascontiguousarray(eps)


# ---------------------------------------------------------------------------------------------------------------------
# bars: the kernel's float32 arithmetic (qr_actor.h: actor_sample, tanh_fast) against the float64 rules.  Everything below is a
# sum of roundings of documented size, evaluated per element from float64 quantities — nothing is fitted to a device result.
#   float32 rounding (add, multiply, fma: ONE rounding each)      <= 2^-24 relative to the result
#   a float32 constant (0.9189..f, 1e-6f, log2(e), ln 2)          <= 2^-24 relative to itself
#   v_exp_f32, v_log_f32, v_rcp_f32                               1 ulp <= 2^-23 relative (AMD Instinct CDNA3/CDNA4 ISA reference)
#   tanh_fast                                                     <= 2e-7 absolute (qr_actor.h, from v_exp_f32 + v_rcp_f32)
# ---------------------------------------------------------------------------------------------------------------------
EPS24, EPS23 = 2.0 ** -24, 2.0 ** -23
TANH_FAST_ERR = 2e-7


def exp_rel(x):
    """Relative error of __expf(x) = v_exp_f32(float32(log2 e) * x): the constant and the product put the exponent y = x log2(e) off
    by <= 2^-23 |y|, a factor 2^(2^-23 |y|) = 1 + 2^-23 |x| (ln 2 log2 e = 1); the instruction adds 1 ulp: 2^-23 (1 + |x|)."""
    return EPS23 * (1.0 + np.abs(x))


def _sech2(x):
    return 1.0 / np.cosh(np.minimum(np.abs(x), 300.0)) ** 2


def sac_action_bar(pre, ls, eps, pre_err=0.0, ls_err=0.0):
    """|a - tanh(u)|, u = pre + sd eps in float64, a = tanh_fast(fmaf(sd32, eps, pre)), ls the clamped log_std:
      du = pre_err                              (the head's own error: 0 where the weights are 0 and pre is the bias)
         + |sd eps| (exp_rel(ls) + ls_err)      (sd32 = __expf(ls); a head's error in ls scales sd by e^ls_err)
         + 2^-24 |u|                            (the fma's one rounding)
      bar = 2e-7 (tanh_fast) + du * max tanh' over [u - du, u + du],   tanh' = sech^2 <= 1, largest at the end nearer 0.
    Deterministic (eps None): fmaf(sd, 0, pre) = pre, du = pre_err."""
    pre, ls = np.asarray(pre, np.float64), np.asarray(ls, np.float64)
    z = np.zeros_like(pre) if eps is None else np.asarray(eps, np.float64)
    sd = np.exp(ls)
    u = pre + sd * z
    du = pre_err + np.abs(sd * z) * (exp_rel(ls) + np.expm1(ls_err)) + EPS24 * np.abs(u) * (z != 0)
    return TANH_FAST_ERR + du * _sech2(np.maximum(np.abs(u) - du, 0.0))


def sac_logp_bar(ls, eps, a, ls_err=0.0):
    """|logp - sac_logp_from_action(ls, eps, a)| for logp = fmaf(-z/2, z, -ls - c32) - __logf(fmaf(-a, a, 1) + 1e-6f):
      -ls - c32        2^-24 (|ls| + c) for the sum + 2^-24 c for the constant
      the fma          2^-24 t1,  t1 = z^2 / 2 + |ls| + c bounds its result (-z/2 is exact, the product is not rounded)
      the argument     s = (1 - a^2) + 1e-6: the fma's rounding, the constant's and the sum's, each <= 2^-24 s: log s moves by 3 * 2^-24
      __logf           v_log_f32 (2^-23 |L|) times float32(ln 2) (constant and product: 2^-23 |L|), L = log s  (tests/test_gpu_noise.py)
      the difference   2^-24 (t1 + |L|)
      + ls_err         a head's own error in ls (0 where ls is the bias)."""
    ls = np.asarray(ls, np.float64)
    a = np.asarray(a, np.float32).astype(np.float64)
    z = np.zeros_like(a) if eps is None else np.asarray(eps, np.float64)
    t1 = 0.5 * z * z + np.abs(ls) + LOG_SQRT_2PI
    L = np.abs(np.log(1.0 - a * a + 1e-6))
    return EPS24 * (np.abs(ls) + 2.0 * LOG_SQRT_2PI) + EPS24 * t1 + 3.0 * EPS24 + 2.0 * EPS23 * L + EPS24 * (t1 + L) + ls_err


def mean_action_bar(pre, ls, eps):
    """|a - clip(mean + sd eps)| for a = clamp(fmaf(sd32, eps, tanh_fast(pre))): 2e-7 (tanh_fast) + |sd eps| exp_rel(ls) (sd32) +
    2^-24 (|raw| + the two before) (the fma's one rounding); the clamp is 1-Lipschitz and exact.  Deterministic: 2e-7."""
    pre, ls = np.asarray(pre, np.float64), np.asarray(ls, np.float64)
    if eps is None:
        return np.full(np.broadcast(pre, ls).shape, TANH_FAST_ERR)
    sd, z = np.exp(ls), np.asarray(eps, np.float64)
    first = TANH_FAST_ERR + np.abs(sd * z) * exp_rel(ls)
    return first + EPS24 * (np.abs(np.tanh(pre) + sd * z) + first)


def mean_logp_bar(pre, ls, a):
    """|logp - normal_logp_from_action(tanh(pre), ls, a)| for z32 = (a - mean32) * __expf(-ls), logp = fmaf(-z32/2, z32, -ls - c32):
      d = a - mean     the kernel's mean32 is tanh_fast(pre): dd = 2e-7 + 2^-24 (|d| + 2e-7) (the subtraction's rounding)
      z = d e^-ls      dz = e^-ls dd (1 + r) + |z| r,  r = exp_rel(-ls) + 2^-24 (__expf and the product)
      z^2 / 2          |z| dz + dz^2 / 2 — proportional to |a - mean| e^-ls, and to its square: at log_std = -20 the 2e-7 of the
                       mean alone is dz = 97, so where the action is not clamped the float32 log-prob carries no information and
                       this bar says so; where it is, z ~ 1e8 and the bar is ~1e-5 of the value
      -ls - c32, the fma's rounding   2^-24 (|ls| + 2 c) + 2^-24 (z^2 / 2 + dq + |ls| + c)."""
    pre, ls = np.asarray(pre, np.float64), np.asarray(ls, np.float64)
    a = np.asarray(a, np.float32).astype(np.float64)
    einv = np.exp(-ls)
    d = a - np.tanh(pre)
    z = d * einv
    dd = TANH_FAST_ERR + EPS24 * (np.abs(d) + TANH_FAST_ERR)
    r = exp_rel(-ls) + EPS24
    dz = einv * dd * (1.0 + r) + np.abs(z) * r
    dq = np.abs(z) * dz + 0.5 * dz * dz
    return dq + EPS24 * (np.abs(ls) + 2.0 * LOG_SQRT_2PI) + EPS24 * (0.5 * z * z + dq + np.abs(ls) + LOG_SQRT_2PI)


def heads_with_error(p, obs, rounding=EPS24):
    """(pre, ls, pre_err, ls_err): the two heads of an MLP_Actor_SAC-shaped network in float64 (ls NOT clamped) and a running bound
    on what a float32 evaluation of it may differ by, whatever its summation order: a K-term dot product with its bias, accumulated
    by fmas and (the MFMA actor's transpose-reduce) a few adds, sees at most K + 3 roundings on any path, so
    |err| <= gamma (|W| (|x| + e_in) + |b|) + |W| e_in with gamma = (K + 3) 2^-24 / (1 - (K + 3) 2^-24); relu is 1-Lipschitz."""
    f = lambda k: np.asarray(p[k], dtype=np.float64)

    def layer(w, b, x, e_in):
        g = (w.shape[1] + 3) * rounding
        g = g / (1.0 - g)
        y = x @ w.T + b
        return y, g * ((np.abs(x) + e_in) @ np.abs(w).T + np.abs(b)) + e_in @ np.abs(w).T

    x = np.asarray(obs, dtype=np.float64)
    h, e = layer(f("fc1_w"), f("fc1_b"), x, np.zeros_like(x))
    h, e = layer(f("fc2_w"), f("fc2_b"), np.maximum(h, 0.0), e)
    h = np.maximum(h, 0.0)
    pre, pre_err = layer(f("mean_w"), f("mean_b"), h, e)
    ls, ls_err = layer(f("log_std_w"), f("log_std_b"), h, e)
    return pre, ls, pre_err, ls_err
