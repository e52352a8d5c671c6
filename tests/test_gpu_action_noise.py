"""The exploration noise qr_rollout_actor draws for itself, element by element, against the value its key must give
(tests/action_ref.py: `rollout_eps`; tests/test_action_ref_host.py shows that these keys tell every wrong key apart).

The action is made the noise: mean_w = 0 and mean_b = 0 give pre = +-0 and tanh_fast(+-0) = +-0; log_std = 0 gives __expf(0) = 1; so
raw = fmaf(1, eps, +-0) = eps exactly, and max_action = 1e6 clamps nothing.  Keys: a seed, a global env id and a global step with
non-zero high words — the stream position arrives through load_state_dict() two steps below 2^32 and five steps are drawn in
launches of 3 and 2, so the step word's 32-bit boundary is crossed inside the first launch and the second starts beyond it.

helper_rollout x auto_reset: the launcher gives a tile its helper wave — which samples the noise a step ahead into a two-slot LDS
buffer, between the pools of in-launch resets — only with in-launch resets (qr_launch.h: pick_shape; asserted below through
launch_plan); helper_rollout=True without them is the plain, rate-adaptive instantiation, =False with them the plain non-adaptive one.
QuadVecEnv takes an env_offset of 2^32 + 192 as it is."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import action_ref as AR  # noqa: E402
from test_gpu_noise import NORMAL_BAR, R_MAX  # noqa: E402  (the bar for one device normal against the restatement, derived there)

pytestmark = pytest.mark.gpu
LOG_SQRT_2PI = AR.LOG_SQRT_2PI
# logp = fmaf(-z/2, z, -0 - c32) with z = (a - 0) * __expf(-0) = a exactly: -z/2 is exact and the product is not rounded, so against
# -a^2 / 2 - log sqrt(2 pi) in float64 AT THE RETURNED a there are the fma's one rounding, <= 2^-24 of a result of at most
# R^2 / 2 + 0.92, and the float32 constant, <= 2^-24 * 0.92: together below 2^-23 (R^2 / 2 + 0.92) = 2.2e-6.
LOGP_BAR = 2.0 ** -23 * (R_MAX ** 2 / 2.0 + LOG_SQRT_2PI)


def _actors(kind):
    from gym_rotor_amd import random_actors
    actors = random_actors(kind, "cuda", generator=torch.Generator("cuda").manual_seed(1), log_std=0.0)
    for a in actors:
        a.mean_w.zero_(); a.mean_b.zero_()
    return actors


def _run(kind, helper, auto_reset, *, env_seed, noise_seed=None):
    """Five steps in launches of 3 and 2 from the loaded stream position: (action, logprob) as float32 [5, n, A]."""
    from gym_rotor_amd import QuadVecEnv
    env = QuadVecEnv(kind, AR.NOISE_N, device="cuda", obs_rows=True, seed=env_seed, env_offset=AR.NOISE_OFFSET, auto_reset=auto_reset,
                     helper_rollout=helper)
    env.reset("train")
    env.get_norm_error_state()
    sd = env.state_dict()
    assert sd["policy_steps"] == 0
    sd["policy_steps"] = AR.NOISE_STEPS
    env.load_state_dict(sd)
    assert env.launch_plan(AR.NOISE_SPLITS[0], "ppo")["help"] == int(helper and auto_reset)
    actors = _actors(kind)
    kw = {} if noise_seed is None else {"noise_seed": noise_seed}
    outs = [env.rollout_actor(actors, k, max_action=1e6, **kw) for k in AR.NOISE_SPLITS]
    torch.cuda.synchronize()
    assert env.state_dict()["policy_steps"] == AR.NOISE_STEPS + sum(AR.NOISE_SPLITS)
    cat = lambda key: torch.cat([o[key] for o in outs], 0).cpu().numpy()
    return cat("action"), cat("logprob")


def _check(label, act, logp, seed, A):
    want = AR.rollout_eps(seed, AR.NOISE_OFFSET, AR.NOISE_N, AR.NOISE_STEPS, sum(AR.NOISE_SPLITS), A)
    assert act.shape == logp.shape == want.shape and act.dtype == np.float32
    a64 = act.astype(np.float64)
    err = np.abs(a64 - want)
    lerr = np.abs(logp.astype(np.float64) - (-0.5 * a64 * a64 - LOG_SQRT_2PI))
    per_step = ", ".join(f"{e:.2e}" for e in err.reshape(err.shape[0], -1).max(1))
    print(f"[action noise] {label}: max |a - eps| {err.max():.3e} (bar {NORMAL_BAR:.3e}; per step {per_step}), component 4 "
          f"{err[..., 4:].max() if A == 5 else 0.0:.3e}, max logp error {lerr.max():.3e} (bar {LOGP_BAR:.3e}), max |a| {np.abs(act).max():.3f}")
    assert np.isfinite(act).all() and np.isfinite(logp).all()
    assert err.max() <= NORMAL_BAR, (label, float(err.max()), np.argwhere(err > NORMAL_BAR)[:5])
    assert np.abs(act).max() <= R_MAX
    assert lerr.max() <= LOGP_BAR, (label, float(lerr.max()))


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("helper", [True, False])
@pytest.mark.parametrize("kind", ["coupled", "decoupled"])
def test_every_draw_against_its_key(kind, helper, auto_reset):
    A = 4 if kind == "coupled" else 5
    act, logp = _run(kind, helper, auto_reset, env_seed=AR.NOISE_SEED)
    _check(f"{kind}, helper {helper}, auto_reset {auto_reset}", act, logp, AR.NOISE_SEED, A)


def test_the_keyword_not_the_envs_seed_keys_the_stream():
    """noise_seed= given and different from the env's seed: the draws are the keyword's, and not the env seed's."""
    act, logp = _run("decoupled", True, True, env_seed=AR.NOISE_SEED, noise_seed=AR.NOISE_OTHER_SEED)
    _check("decoupled, helper, auto_reset, noise_seed=", act, logp, AR.NOISE_OTHER_SEED, 5)
    other = AR.rollout_eps(AR.NOISE_SEED, AR.NOISE_OFFSET, AR.NOISE_N, AR.NOISE_STEPS, sum(AR.NOISE_SPLITS), 5)
    assert (np.abs(act.astype(np.float64) - other) > 100.0 * NORMAL_BAR).mean() >= 0.99
