#!/usr/bin/env python3
"""Do two builds of the library compute the same bits?  Each build (QR_LIB) steps the same batch (QR_AB_KIND, default quad; QR_AB_ENVS, default 65 536
envs) with in-launch resets in its own subprocess and prints a digest of state, integrators, parameters, observation rows, rewards,
dones, terminal observations, episode and tile counters — then the same for qr_rollout and (wrappers) qr_rollout_actor with a PPO and an SAC actor.
A third digest covers the update launches: ppo_critic_grad on every case of tests/golden/ppo_critic_grad.npz (gradients, stats), td3_target
and twinq_grad on every case of tests/golden/td3_critic.npz (y, the twelve gradients, stats), each at the default grid, at
max_workgroups 1 and 3, and once with a permuted index; sac_target on every case of tests/golden/sac_critic.npz (y, action_out,
logp_out), in order and with the permuted index; ppo_actor_grad on every case of tests/golden/ppo_actor_grad.npz (the seven gradients,
stats) and dpg_actor_grad on every case of tests/golden/td3_actor.npz (the six gradients, stats), each at the default grid, at
max_workgroups 1 and 3, and once with the permuted index.
A build whose child does not exit 0 within QR_AB_TIMEOUT seconds (default 900) ends the run: nothing more is started on the card.

    [QR_AB_KIND=coupled] python tools/ab_equal.py build/ab/A.so build/ab/B.so        (GPU box)
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import hashlib, sys, torch
sys.path.insert(0, %r)
from gym_rotor_amd import QuadVecEnv
import os
kind = os.environ.get("QR_AB_KIND", "quad")
NE = int(os.environ.get("QR_AB_ENVS", "65536"))
env = QuadVecEnv(kind, NE, device="cuda", seed=3, auto_reset=True, obs_rows=True, final_obs=True, want_raw_reward=True)
env.reset("train")
if kind != "quad":
    env.get_norm_error_state()
g = torch.Generator(device="cuda"); g.manual_seed(1)
h = hashlib.sha256()
for t in range(300):
    o, r, d, _, _ = env.step(torch.rand(NE, env.action_dim, device="cuda", generator=g) * 2 - 1)
    if t %% 10 == 9:
        obs = [o] if isinstance(o, torch.Tensor) else list(o)
        fin = env.final_observation()
        fin = [fin] if isinstance(fin, torch.Tensor) else list(fin)
        rows = d.reshape(NE, -1).any(dim=1)
        for x in [env.get_current_state(), env._params, r, env._reward_raw, d, env._episode, env._reset_count] + obs + [f[rows] for f in fin] + ([env._integ] if env._integ is not None else []):
            h.update(x.cpu().numpy().tobytes())
step_digest = h.hexdigest()
# the multi-step instantiations: qr_rollout (T = 24, twice) and, for the wrappers, qr_rollout_actor (PPO and SAC forms, T = 8)
h = hashlib.sha256()
def upd(d):
    for k in sorted(d):
        v = d[k]
        if k == "obs" or v is None:
            continue
        for x in (v if isinstance(v, (tuple, list)) else [v]):
            h.update(x.cpu().numpy().tobytes())
for rep in range(2):
    upd(env.rollout(torch.rand(24, NE, env.action_dim, device="cuda", generator=g) * 2 - 1))
h.update(env.get_current_state().cpu().numpy().tobytes()); h.update(env._reset_count.cpu().numpy().tobytes())
if kind != "quad":
    from gym_rotor_amd import random_actors
    for algo in ("ppo", "sac"):
        actors = random_actors(kind, "cuda", generator=torch.Generator(device="cuda").manual_seed(5), log_std=-0.5, algo=algo)
        env.get_norm_error_state()
        upd(env.rollout_actor(actors, 8))
    h.update(env.get_current_state().cpu().numpy().tobytes()); h.update(env._integ.cpu().numpy().tobytes())
rollout_digest = h.hexdigest()
# the update launches on the fixtures of their tests
import numpy as np
sys.path.insert(0, os.path.join(%r, "tests"))
import sac_ref, td3_actor_ref, td3_ref, test_ppo_actor_host as pah, test_ppo_critic_host as pch, test_sac_critic_host as sch, test_td3_critic_host as tch
from gym_rotor_amd import ActorParams, CriticParams, QCriticParams, _lib, dpg_actor_grad, ppo_actor_grad, ppo_critic_grad, sac_target, td3_target, twinq_grad
h = hashlib.sha256()
cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
perm = cuda(np.random.default_rng(0).permutation(130).astype(np.int64))
def put(*ts):
    for x in ts:
        h.update(x.cpu().numpy().tobytes())
g = dict(np.load(os.path.join(%r, "tests", "golden", "ppo_critic_grad.npz"), allow_pickle=False))
for name in pch.CASES:
    c = pch.case(g, name)
    critic, obs, tgt = CriticParams(*[cuda(t) for t in c["w"]], c["inputs"]), [cuda(o) for o in c["obs"]], cuda(c["target"])
    for index, mw in ((None, 0), (None, 1), (None, 3), (perm, 0)):
        grads, stats = ppo_critic_grad(critic, obs, tgt, index, l2_reg=c["l2_reg"], max_workgroups=mw)
        put(*[grads[n] for n in pch.NAMES], stats)
g = td3_ref.load()
for name in tch.CASES:
    c = td3_ref.case(g, name)
    critic, critic_t = (QCriticParams(*[cuda(c[p + n]) for n in td3_ref.NAMES], int(c["action_dim"])) for p in ("c_", "t_"))
    actor_t = ActorParams(*[cuda(c["a_" + n]) for n in td3_ref.ACTOR_NAMES], None) if "a_fc1_w" in c else None
    tens = {"obs": cuda(c["obs"]), "act": cuda(c["action"]), "rwd": cuda(c["reward"]), "obs_next": cuda(c["obs_next"]), "done": cuda(c["done"])}
    kw = {k: float(c[k]) for k in ("discount", "target_noise", "noise_clip", "max_action")}
    kw["noise"] = None if c.get("eps") is None else cuda(c["eps"])
    if actor_t is None:
        kw["action_next"] = cuda(c["a_next_in"])
    for index, mw in ((None, 0), (None, 1), (None, 3), (perm, 0)):
        y = td3_target(actor_t, critic_t, tens, 0, index, **kw)
        grads, stats = twinq_grad(critic, tens["obs"], tens["act"], y, index, max_workgroups=mw)
        put(y, *[grads[n] for n in td3_ref.NAMES], stats)
g = sac_ref.load()
for name in sch.CASES:
    c = sac_ref.case(g, name)
    critic_t = QCriticParams(*[cuda(c["t_" + n]) for n in td3_ref.NAMES], int(c["action_dim"]))
    w = [cuda(c["a_" + n]) for n in sac_ref.ACTOR_NAMES] if "a_fc1_w" in c else None
    actor = ActorParams(*w[:6], None, w[6], w[7], _lib.ACTOR_TANH_SAMPLE) if w else None
    tens = {"rwd": cuda(c["reward"]), "obs_next": cuda(c["obs_next"]), "done": cuda(c["done"])}
    kw = dict(discount=float(c["discount"]), alpha=float(c["alpha"]), noise=None if c.get("eps") is None else cuda(c["eps"]))
    if actor is None:
        kw.update(action_next=cuda(c["a_next_in"]), logp_next=cuda(c["logp_next_in"]))
    for index in (None, perm):
        a_out, logp_out = torch.zeros(130, int(c["action_dim"]), device="cuda"), torch.zeros(130, device="cuda")
        put(sac_target(actor, critic_t, tens, 0, index, action_out=a_out, logp_out=logp_out, **kw), a_out, logp_out)
g = dict(np.load(os.path.join(%r, "tests", "golden", "ppo_actor_grad.npz"), allow_pickle=False))
for name in pah.CASES:
    c = pah.case(g, name)
    actor, pos = ActorParams(*[cuda(t) for t in c["w"]]), [cuda(c[k]) for k in ("obs", "action", "logp_old", "advantage")]
    kw = dict(final_obs=cuda(c["final_obs"]), done=cuda(c["done"]), truncated=cuda(c["truncated"]), noise=cuda(c["noise"]),
              nominal=cuda(c["nominal"].astype(np.float32)), **c["co"])
    for index, mw in ((None, 0), (None, 1), (None, 3), (perm, 0)):
        grads, stats = ppo_actor_grad(actor, *pos, index, max_workgroups=mw, **kw)
        put(*[grads[n] for n in pah.NAMES], stats)
g = td3_actor_ref.load()
for name in td3_actor_ref.CASES:
    c = td3_actor_ref.case(g, name)
    q1 = [cuda(c["c_" + n]) for n in td3_actor_ref.Q1_NAMES]
    actor, critic = ActorParams(*[cuda(c["a_" + n]) for n in td3_actor_ref.ACTOR_NAMES], None), QCriticParams(*q1, *q1, c["a_fc3_w"].shape[0])
    kw = dict(zip(("lam_T", "lam_S", "lam_M"), c["lam"]), max_action=c["max_action"], noise=cuda(c["noise"]), nominal=cuda(c["nominal"].astype(np.float32)))
    for index, mw in ((None, 0), (None, 1), (None, 3), (perm, 0)):
        grads, stats = dpg_actor_grad(actor, critic, cuda(c["obs"]), cuda(c["obs_next"]), index, max_workgroups=mw, **kw)
        put(*[grads[n] for n in _lib.DPG_GRAD_NAMES], stats)
torch.cuda.synchronize()
print(step_digest, rollout_digest, h.hexdigest(), int(env._episode.sum()))
''' % (ROOT, ROOT, ROOT, ROOT)
out = []
for lib in sys.argv[1:3]:
    try:
        r = subprocess.run([sys.executable, "-c", CHILD], env=dict(os.environ, QR_LIB=os.path.abspath(lib)), capture_output=True, text=True,
                           timeout=float(os.environ.get("QR_AB_TIMEOUT", "900")))
    except subprocess.TimeoutExpired:
        sys.exit(f"{os.path.basename(lib)} FAILED: time limit; nothing more is started")
    if r.returncode != 0:
        sys.exit(f"{os.path.basename(lib)} FAILED (exit {r.returncode}); nothing more is started\n{r.stderr[-600:]}")
    out.append(r.stdout.strip().splitlines()[-1])
    print(os.path.basename(lib), out[-1])
print("IDENTICAL" if out[0] == out[1] else "DIFFERENT")
sys.exit(0 if out[0] == out[1] else 1)
