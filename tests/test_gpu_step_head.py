"""The head of the one-step helper-wave launch (qr_step.h: kHeadOrder — the load queue ordered by first use, the attitude
unpack, the substep size and the action map pinned behind partial waits) against the plain launch of the same env-steps, bit for bit.

qr_step with in-launch resets, 40 steps, once with QR_FLAG_FORCE_HELPER and once with QR_FLAG_NO_HELPER: state, integrators, parameters,
reward, terminated and truncated must agree after every step.  Shapes: a single lane, ragged tails on either side of one tile, three
tiles, and 520 envs = 9 tiles, where both the quotient and the remainder of the XCD tile map are non-zero; env_offset 0 and 64; with and
without a params buffer; with and without a steps buffer.  At 520 envs the result must also equal the first 520 envs of a 1024-env batch
(the in-launch reset stream is keyed by tile, not by grid), and at least one env must have been re-sampled."""
import itertools

import pytest
import torch

KINDS = ("quad", "coupled", "decoupled")
SIZES = (1, 63, 64, 65, 129, 520)
STEPS = 40
LIMIT = 25      # max_episode_steps of the cases with a steps buffer: truncations inside the 40 steps


def _make(kind, n, helper, env_offset, params, steps):
    from gym_rotor_amd import QuadVecEnv
    env = QuadVecEnv(kind, n, device="cuda", seed=11, auto_reset=True, use_UDM=params, env_offset=env_offset,
                     max_episode_steps=LIMIT if steps else 0, helper=helper, autotune=False)
    env.reset("train")
    if kind != "quad":
        env.get_norm_error_state()
    return env


def _buffers(env, n):
    """Everything a step leaves behind, as stored: x, v | packed attitude, W | integrators | parameters | step counters."""
    out = {"pos_vel": env._pos_vel[:, :n], "att_rate": env._att_rate[:, :n]}
    for name in ("integ", "params", "steps"):
        b = getattr(env, "_" + name)
        if b is not None:
            out[name] = b[:, :n] if b.dim() == 2 else b[:n]
    return out


def _seed_from(dst, src, n):
    """Start `dst` (n envs) from the first n envs of `src` (integrators included: no second get_norm_error_state, which advances them)."""
    for name, b in _buffers(src, n).items():
        _buffers(dst, n)[name].copy_(b)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_helper_and_plain_launch_agree_bit_for_bit(kind, n):
    g = torch.Generator(device="cuda"); g.manual_seed(100 + n)
    for env_offset, params, steps in itertools.product((0, 64), (True, False), (True, False)):
        tag = f"{kind} n={n} env_offset={env_offset} params={params} steps={steps}"
        helper, plain = _make(kind, n, True, env_offset, params, steps), _make(kind, n, False, env_offset, params, steps)
        assert helper.kernel_info()[2] == 128 and plain.kernel_info()[2] == 64, tag
        big = _make(kind, 1024, None, env_offset, params, steps) if n == 520 else None
        if big is not None:
            _seed_from(helper, big, n); _seed_from(plain, big, n)
        m = 1024 if big is not None else n
        acts = torch.rand(STEPS, m, helper.action_dim, device="cuda", generator=g) * 2 - 1
        resets = 0
        for t in range(STEPS):
            a = acts[t, :n]
            oh, op = helper.step(a), plain.step(a)
            ob = big.step(acts[t]) if big is not None else None
            for name, i in (("reward", 1), ("terminated", 2), ("truncated", 3)):
                assert _same(oh[i], op[i]), f"{tag}: {name} differs at step {t}"
                if ob is not None:
                    assert _same(oh[i], ob[i][:n]), f"{tag}: {name} differs from the 1024-env batch at step {t}"
            bh, bp = _buffers(helper, n), _buffers(plain, n)
            for name in bh:
                assert _same(bh[name], bp[name]), f"{tag}: {name} differs at step {t}"
                if big is not None:
                    assert _same(bh[name], _buffers(big, n)[name]), f"{tag}: {name} differs from the 1024-env batch at step {t}"
            resets += int((oh[2].any(dim=-1) | oh[3].reshape(n, -1).any(dim=-1)).sum())
        if n == 520:
            assert resets >= 1, f"{tag}: no env was re-sampled in {STEPS} steps — the reset path was not exercised"
