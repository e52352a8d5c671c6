"""`torch.ops.gym_rotor_amd.*` — every entry point of the C-ABI (include/quadrotor_hip.h) registered as a
PyTorch custom op, for callers that want the env step inside a torch program:
`torch.compile(fullgraph=True)`, export, CUDA-graph capture.  Tensors carry the device buffers, the op
body is one ctypes call into libquadrotor_hip.so on the current stream of the buffers' device; there is
no CPU kernel behind these ops (a CPU tensor raises).

Argument convention (the same for every env op):
    state   pos_vel [6, N] (x, v), att_rate [6, N] (the three smaller quaternion components k0 k1 k2, W)
                                                       SoA views (row stride = QrEnv.field_stride)
    per-env integ [8, N]?, params [6, N]?, goal [12, N]?, traj [8, N]?, episode [N] i32?, steps [N] i32?,
            reset_count [ceil(N/64)] i32?              None where the env has no such buffer
    cfg     List[int] = [kind, layout, flags, seed, env_offset, goal_mode, max_episode_steps]   (QrEnv scalars)
    coeffs  List[float] = the QrCoeffs fields in header order (`env_args(env)[2]` / `default_coeffs_list()`)
`env_args(env)` gives (state + per-env tensors, cfg, coeffs) of a QuadVecEnv; `step(env, action, out)` etc.
are thin functional wrappers that call the ops with the env's own buffers — what QuadVecEnv.step does, but
visible to torch's tracer as ONE opaque, mutating op.

Reference interface mirrored: QuadEnv.step / reset / set_goal_state(-> goal buffer) / get_norm_error_state /
get_current_state (gym_rotor/envs/quad.py:142, 171, 409, 413, 421).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch

from . import _lib
from .constants import OBS_DIMS

_NS = "gym_rotor_amd"
_COEFF_NAMES = [n for n, _ in _lib.QrCoeffs._fields_]
N_CFG = 7


_p = _lib.ptr


def _gpu(t: torch.Tensor):
    if t.device.type != "cuda":
        raise RuntimeError("gym_rotor_amd ops run on the GPU only (no CPU kernel exists)")


def default_coeffs_list() -> List[float]:
    c = _lib.default_coeffs()
    return [float(getattr(c, n)) for n in _COEFF_NAMES]


def env_args(env):
    """(tensors, cfg, coeffs) of a QuadVecEnv for the ops below: tensors = (pos_vel, att_rate, integ, params, goal, traj,
    episode, steps, reset_count); cfg / coeffs are the plain-Python copies the env keeps of its QrEnv scalars and
    QrCoeffs (so that torch.compile can trace through this function).  Seeds are passed as int64 (QuadVecEnv accepts
    0 <= seed < 2^63 only, so the op path and the env path draw the same streams)."""
    tensors = (env._pos_vel, env._att_rate, env._integ, env._params, env._goal, env._traj, env._episode, env._steps, env._reset_count)
    return tensors, env._op_cfg, env._op_coeffs


def _env_struct(pos_vel, att_rate, integ, params, goal, traj, episode, steps, reset_count, cfg: Sequence[int], coeffs: Sequence[float]):
    _gpu(pos_vel)
    if len(cfg) != N_CFG:
        raise ValueError(f"cfg must hold {N_CFG} ints: kind, layout, flags, seed, env_offset, goal_mode, max_episode_steps")
    if len(coeffs) != len(_COEFF_NAMES):
        raise ValueError(f"coeffs must hold the {len(_COEFF_NAMES)} QrCoeffs fields")
    e = _lib.QrEnv()
    e.kind, e.layout, e.flags = int(cfg[0]), int(cfg[1]), int(cfg[2])
    e.seed, e.env_offset, e.goal_mode, e.max_episode_steps = int(cfg[3]) & (2 ** 64 - 1), int(cfg[4]), int(cfg[5]), int(cfg[6])
    if pos_vel.shape[0] != 6 or att_rate.shape[0] != 6 or att_rate.shape[1] != pos_vel.shape[1] or att_rate.stride(0) != pos_vel.stride(0):
        raise ValueError("pos_vel and att_rate must be [6, N] SoA views with the same row stride (quadrotor_hip.h: field_stride)")
    e.num_envs, e.field_stride = pos_vel.shape[1], pos_vel.stride(0)
    e.pos_vel, e.att_rate, e.integ, e.params, e.goal, e.traj = _p(pos_vel), _p(att_rate), _p(integ), _p(params), _p(goal), _p(traj)
    e.episode, e.steps, e.reset_count = _p(episode), _p(steps), _p(reset_count)
    for n, v in zip(_COEFF_NAMES, coeffs):
        setattr(e.coeffs, n, float(v))
    return e


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _out_struct(*tensors):
    """QrStepOut of an op's positional output tensors, in _OUT_MUT's order (a None `truncated` is a null pointer either way)."""
    return _lib.step_out(dict(zip(_OUT_KEYS, tensors)), True)


# (goal: written by the fused goal generator's stateful modes 2-5, whose xd / vd / b1d / Wd persist there)
_ENV_MUT = ("pos_vel", "att_rate", "integ", "params", "goal", "traj", "episode", "steps", "reset_count")
_OUT_MUT = ("obs0", "obs1", "reward", "reward_raw", "done", "truncated", "final_obs0", "final_obs1")
_OUT_KEYS = tuple("terminated" if k == "done" else k for k in _OUT_MUT)   # the ops call QrStepOut.done by its member name


@torch.library.custom_op(f"{_NS}::qr_step", mutates_args=_ENV_MUT + _OUT_MUT)
def qr_step(pos_vel: torch.Tensor, att_rate: torch.Tensor, integ: Optional[torch.Tensor], params: Optional[torch.Tensor],
            goal: Optional[torch.Tensor], traj: Optional[torch.Tensor], episode: Optional[torch.Tensor], steps: Optional[torch.Tensor],
            reset_count: Optional[torch.Tensor], action: torch.Tensor,
            obs0: Optional[torch.Tensor], obs1: Optional[torch.Tensor], reward: torch.Tensor, reward_raw: Optional[torch.Tensor],
            done: torch.Tensor, truncated: Optional[torch.Tensor], final_obs0: Optional[torch.Tensor], final_obs1: Optional[torch.Tensor],
            substeps: int, cfg: List[int], coeffs: List[float]) -> None:
    """QuadEnv.step for all envs (qr_step).  action [N, A] float32 contiguous; outputs as in QrStepOut."""
    e = _env_struct(pos_vel, att_rate, integ, params, goal, traj, episode, steps, reset_count, cfg, coeffs)
    o = _out_struct(obs0, obs1, reward, reward_raw, done, truncated, final_obs0, final_obs1)
    with torch.cuda.device(pos_vel.device):
        _lib.check(_lib.load().qr_step(C.byref(e), action.data_ptr(), substeps, C.byref(o), _stream(pos_vel)), "qr_step")


@torch.library.custom_op(f"{_NS}::qr_rollout", mutates_args=_ENV_MUT + _OUT_MUT)
def qr_rollout(pos_vel: torch.Tensor, att_rate: torch.Tensor, integ: Optional[torch.Tensor], params: Optional[torch.Tensor],
               goal: Optional[torch.Tensor], traj: Optional[torch.Tensor], episode: Optional[torch.Tensor], steps: Optional[torch.Tensor],
               reset_count: Optional[torch.Tensor], action: torch.Tensor,
               obs0: Optional[torch.Tensor], obs1: Optional[torch.Tensor], reward: torch.Tensor, reward_raw: Optional[torch.Tensor],
               done: torch.Tensor, truncated: Optional[torch.Tensor], final_obs0: Optional[torch.Tensor], final_obs1: Optional[torch.Tensor],
               substeps: int, cfg: List[int], coeffs: List[float]) -> None:
    """T env-steps in one launch (qr_rollout).  action [T, N, A]; outputs [T, N, ...]."""
    e = _env_struct(pos_vel, att_rate, integ, params, goal, traj, episode, steps, reset_count, cfg, coeffs)
    o = _out_struct(obs0, obs1, reward, reward_raw, done, truncated, final_obs0, final_obs1)
    with torch.cuda.device(pos_vel.device):
        _lib.check(_lib.load().qr_rollout(C.byref(e), action.data_ptr(), action.shape[0], substeps, C.byref(o), _stream(pos_vel)), "qr_rollout")


@torch.library.custom_op(f"{_NS}::qr_rollout_actor", mutates_args=_ENV_MUT + _OUT_MUT + ("action_out", "logprob_out"))
def qr_rollout_actor(pos_vel: torch.Tensor, att_rate: torch.Tensor, integ: Optional[torch.Tensor], params: Optional[torch.Tensor],
                     goal: Optional[torch.Tensor], traj: Optional[torch.Tensor], episode: Optional[torch.Tensor], steps: Optional[torch.Tensor],
                     reset_count: Optional[torch.Tensor],
                     actor0: List[torch.Tensor], actor1: List[torch.Tensor], squash: List[int],
                     obs0_in: torch.Tensor, obs1_in: Optional[torch.Tensor], noise: Optional[torch.Tensor],
                     action_out: torch.Tensor, logprob_out: Optional[torch.Tensor],
                     obs0: Optional[torch.Tensor], obs1: Optional[torch.Tensor], reward: torch.Tensor, reward_raw: Optional[torch.Tensor],
                     done: torch.Tensor, truncated: Optional[torch.Tensor], final_obs0: Optional[torch.Tensor], final_obs1: Optional[torch.Tensor],
                     n_steps: int, substeps: int, noise_seed: int, step_base: int, max_action: float, deterministic: bool,
                     cfg: List[int], coeffs: List[float]) -> None:
    """The collection loop with the reference's MLP actor(s) inside the step kernel (qr_rollout_actor).  actorK = the agent's
    tensors in the order fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, then EITHER log_std OR log_std_w, log_std_b (7 or 8
    tensors; actor1 = [] for COUPLED); squash = QR_ACTOR_* per agent."""
    from .policy import c_actor_array
    e = _env_struct(pos_vel, att_rate, integ, params, goal, traj, episode, steps, reset_count, cfg, coeffs)
    arr = c_actor_array(_actor_params(actor0, actor1, squash))   # (kept alive here: the struct only points at it)
    pol = _lib.policy_rollout(arr, (obs0_in, obs1_in), action_out=action_out, logprob_out=logprob_out, noise=noise, noise_seed=noise_seed,
                              step_base=step_base, max_action=max_action, deterministic=deterministic)
    o = _out_struct(obs0, obs1, reward, reward_raw, done, truncated, final_obs0, final_obs1)
    with torch.cuda.device(pos_vel.device):
        _lib.check(_lib.load().qr_rollout_actor(C.byref(e), C.byref(pol), n_steps, substeps, C.byref(o), _stream(pos_vel)), "qr_rollout_actor")


def _actor_params(actor0, actor1, squash):
    from .policy import ActorParams
    actors = []
    for k, ts in enumerate((actor0, actor1)):
        if not ts:
            continue
        if len(ts) == 7:
            actors.append(ActorParams(*ts[:6], ts[6], None, None, int(squash[k])))
        elif len(ts) == 8:
            actors.append(ActorParams(*ts[:6], None, ts[6], ts[7], int(squash[k])))
        else:
            raise ValueError("an actor is 7 tensors (.., log_std) or 8 (.., log_std_w, log_std_b)")
    return actors


@torch.library.custom_op(f"{_NS}::qr_evaluate_actor",
                         mutates_args=("pos_vel", "att_rate", "integ", "goal", "traj", "steps", "action_out", "episode_return", "benchmark",
                                       "length", "terminated", "success", "final_error", "obs0", "obs1"))
def qr_evaluate_actor(pos_vel: torch.Tensor, att_rate: torch.Tensor, integ: Optional[torch.Tensor], params: Optional[torch.Tensor],
                      goal: Optional[torch.Tensor], traj: Optional[torch.Tensor], episode: Optional[torch.Tensor], steps: Optional[torch.Tensor],
                      reset_count: Optional[torch.Tensor],
                      actor0: List[torch.Tensor], actor1: List[torch.Tensor], squash: List[int],
                      obs0_in: torch.Tensor, obs1_in: Optional[torch.Tensor], action_out: Optional[torch.Tensor],
                      episode_return: torch.Tensor, benchmark: torch.Tensor, length: torch.Tensor, terminated: torch.Tensor,
                      success: torch.Tensor, final_error: Optional[torch.Tensor], obs0: torch.Tensor, obs1: Optional[torch.Tensor],
                      max_steps: int, substeps: int, max_action: float, cfg: List[int], coeffs: List[float]) -> None:
    """Learner.eval_policy for every env in one launch (qr_evaluate_actor): the deterministic actor(s) from each env's current state
    until its first done or max_steps; per-env results as in QrEvalOut.  Actors as in qr_rollout_actor."""
    _evaluate_op(None, _env_struct(pos_vel, att_rate, integ, params, goal, traj, episode, steps, reset_count, cfg, coeffs),
                 _actor_params(actor0, actor1, squash), (obs0_in, obs1_in), action_out,
                 (episode_return, benchmark, length, terminated, success, final_error, obs0, obs1), max_steps, substeps, max_action, pos_vel)


@torch.library.custom_op(f"{_NS}::qr_evaluate_population",
                         mutates_args=("pos_vel", "att_rate", "integ", "goal", "traj", "steps", "action_out", "episode_return", "benchmark",
                                       "length", "terminated", "success", "final_error", "obs0", "obs1"))
def qr_evaluate_population(pos_vel: torch.Tensor, att_rate: torch.Tensor, integ: Optional[torch.Tensor], params: Optional[torch.Tensor],
                           goal: Optional[torch.Tensor], traj: Optional[torch.Tensor], episode: Optional[torch.Tensor],
                           steps: Optional[torch.Tensor], reset_count: Optional[torch.Tensor],
                           actor0: List[torch.Tensor], actor1: List[torch.Tensor], squash: List[int],
                           obs0_in: torch.Tensor, obs1_in: Optional[torch.Tensor], action_out: Optional[torch.Tensor],
                           episode_return: torch.Tensor, benchmark: torch.Tensor, length: torch.Tensor, terminated: torch.Tensor,
                           success: torch.Tensor, final_error: Optional[torch.Tensor], obs0: torch.Tensor, obs1: Optional[torch.Tensor],
                           envs_per_policy: int, max_steps: int, substeps: int, max_action: float, cfg: List[int],
                           coeffs: List[float]) -> None:
    """qr_evaluate_actor for P policies in one launch (qr_evaluate_population).  Actors as in qr_evaluate_actor with every tensor
    STACKED [P, ...] (contiguous; P is read off actor0[0]); the env holds P * roundup(envs_per_policy, 64) envs, policy p owns
    [p Epad, p Epad + E); rows are per env, padding rows untouched."""
    _evaluate_op(int(envs_per_policy), _env_struct(pos_vel, att_rate, integ, params, goal, traj, episode, steps, reset_count, cfg, coeffs),
                 _actor_params(actor0, actor1, squash), (obs0_in, obs1_in), action_out,
                 (episode_return, benchmark, length, terminated, success, final_error, obs0, obs1), max_steps, substeps, max_action, pos_vel)


def _evaluate_op(envs_per_policy: Optional[int], e, actors, obs, action_out, outs, max_steps, substeps, max_action, pos_vel):
    """The body of qr_evaluate_actor (envs_per_policy None: `actors` are one policy's) and qr_evaluate_population (`actors` hold
    stacked [P, ...] tensors); outs: the result tensors in QrEvalOut's member order.  One library call on pos_vel's device."""
    from .policy import ActorPopulation, c_actor_array
    if envs_per_policy is None:
        arr, call, tail = c_actor_array(actors), _lib.load().qr_evaluate_actor, ()
    else:
        population = ActorPopulation(actors)
        if e.kind in (_lib.KIND_COUPLED, _lib.KIND_DECOUPLED):  # (Quad-v0: the library answers QR_E_KIND)
            population.check(_lib.KIND_NAME[e.kind], pos_vel.device)
        pop = _lib.QrPopulation(len(population), envs_per_policy)
        arr, call, tail = population.c_array(), _lib.load().qr_evaluate_population, (C.byref(pop),)
    pol = _lib.policy_rollout(arr, obs, action_out=action_out, max_action=max_action, deterministic=True)   # (arr stays alive here)
    o = _lib.eval_out(dict(zip((n for n, _ in _lib.QrEvalOut._fields_), outs)))
    with torch.cuda.device(pos_vel.device):
        _lib.check(call(C.byref(e), C.byref(pol), *tail, max_steps, substeps, C.byref(o), _stream(pos_vel)), call.__name__)


@torch.library.custom_op(f"{_NS}::qr_error_obs", mutates_args=("integ", "obs0", "obs1"))
def qr_error_obs(pos_vel: torch.Tensor, att_rate: torch.Tensor, integ: torch.Tensor, goal: Optional[torch.Tensor],
                 obs0: torch.Tensor, obs1: Optional[torch.Tensor], cfg: List[int], coeffs: List[float], fmt: int = -1) -> None:
    """QuadEnv.get_norm_error_state(framework) for all envs (qr_error_obs / qr_error_obs_format): advances the integral terms like
    the reference.  fmt = -1: the env's own format; 1 (= QR_KIND_COUPLED): MONO rows [N,23]; 2 (= QR_KIND_DECOUPLED): MODUL rows
    [N,15] + [N,3] — on either wrapper kind (quad.py:452-466)."""
    e = _env_struct(pos_vel, att_rate, integ, None, goal, None, None, None, None, cfg, coeffs)
    e.goal_mode = 0
    with torch.cuda.device(pos_vel.device):
        if fmt < 0:
            _lib.check(_lib.load().qr_error_obs(C.byref(e), obs0.data_ptr(), _p(obs1), _stream(pos_vel)), "qr_error_obs")
        else:
            _lib.check(_lib.load().qr_error_obs_format(C.byref(e), int(fmt), obs0.data_ptr(), _p(obs1), _stream(pos_vel)), "qr_error_obs_format")


@torch.library.custom_op(f"{_NS}::qr_reset", mutates_args=("pos_vel", "att_rate", "integ", "params", "episode", "steps"))
def qr_reset(pos_vel: torch.Tensor, att_rate: torch.Tensor, integ: Optional[torch.Tensor], params: Optional[torch.Tensor],
             episode: torch.Tensor, steps: Optional[torch.Tensor], mask: Optional[torch.Tensor], cfg: List[int], coeffs: List[float]) -> None:
    """QuadEnv.reset for masked envs (qr_reset); cfg's flags select train / eval (QR_FLAG_EVAL_RESET) and UDM."""
    e = _env_struct(pos_vel, att_rate, integ, params, None, None, episode, steps, None, cfg, coeffs)
    e.goal_mode = 0
    with torch.cuda.device(pos_vel.device):
        _lib.check(_lib.load().qr_reset(C.byref(e), _p(mask), _stream(pos_vel)), "qr_reset")


@torch.library.custom_op(f"{_NS}::qr_traj_start", mutates_args=("traj", "goal"))
def qr_traj_start(pos_vel: torch.Tensor, att_rate: torch.Tensor, traj: torch.Tensor, goal: Optional[torch.Tensor], episode: Optional[torch.Tensor],
                  mask: Optional[torch.Tensor], draws: Optional[torch.Tensor], cfg: List[int], coeffs: List[float]) -> None:
    """TrajectoryGenerator.mark_traj_start for masked envs from the current state (qr_traj_start); draws [3, N] injects
    theta_b1d, t_traj, w_b1d, default: the env's stream (seed, global env id, episode).  goal: the env's goal buffer — required
    (and reset to a fresh generator's xd = vd = Wd = 0, b1d = e1) in the stateful modes 2-5, untouched otherwise."""
    e = _env_struct(pos_vel, att_rate, None, None, goal, traj, episode, None, None, cfg, coeffs)
    with torch.cuda.device(pos_vel.device):
        _lib.check(_lib.load().qr_traj_start(C.byref(e), _p(mask), _p(draws), _stream(pos_vel)), "qr_traj_start")


@torch.library.custom_op(f"{_NS}::qr_get_state", mutates_args=("rows",))
def qr_get_state(pos_vel: torch.Tensor, att_rate: torch.Tensor, rows: torch.Tensor, cfg: List[int], coeffs: List[float]) -> None:
    """QuadEnv.get_current_state: float64 rows [N, 18] = (x, v, vec_F(R(q)), W) (qr_get_state)."""
    e = _env_struct(pos_vel, att_rate, None, None, None, None, None, None, None, cfg, coeffs)
    e.goal_mode = 0
    with torch.cuda.device(pos_vel.device):
        _lib.check(_lib.load().qr_get_state(C.byref(e), rows.data_ptr(), _stream(pos_vel)), "qr_get_state")


@torch.library.custom_op(f"{_NS}::qr_set_state", mutates_args=("pos_vel", "att_rate", "rejected"))
def qr_set_state(pos_vel: torch.Tensor, att_rate: torch.Tensor, rows: torch.Tensor, mask: Optional[torch.Tensor],
                 rejected: Optional[torch.Tensor], cfg: List[int], coeffs: List[float]) -> None:
    """Assignment to QuadEnv.state from float64 rows [N, 18] (qr_set_state); `rejected` (int32 [1], zeroed by the caller)
    counts rows whose attitude block has no nearest rotation."""
    e = _env_struct(pos_vel, att_rate, None, None, None, None, None, None, None, cfg, coeffs)
    e.goal_mode = 0
    with torch.cuda.device(pos_vel.device):
        _lib.check(_lib.load().qr_set_state(C.byref(e), rows.data_ptr(), _p(mask), _p(rejected), _stream(pos_vel)), "qr_set_state")


@torch.library.custom_op(f"{_NS}::qr_gae", mutates_args=("advantage", "td_target"))
def qr_gae(reward: torch.Tensor, done: torch.Tensor, value: torch.Tensor, gamma: float, lam: float,
           advantage: torch.Tensor, td_target: torch.Tensor, next_value: Optional[torch.Tensor] = None) -> None:
    """GAE reverse scan (qr_gae): reward/done [T, M]; value [T+1, M] (row T = bootstrap) — or, with next_value [T, M]
    (the reference's V(obs_next)), value [T, M]."""
    _gpu(reward)
    T, M = reward.shape[0], reward[0].numel()
    with torch.cuda.device(reward.device):
        rc = _lib.load().qr_gae(reward.data_ptr(), done.data_ptr(), value.data_ptr(), _p(next_value), T, M, gamma, lam,
                                advantage.data_ptr(), td_target.data_ptr(), None, _stream(reward))
    _lib.check(rc, "qr_gae")


def _critic_params(critic: Sequence[torch.Tensor], inputs: Sequence[int]):
    from .policy import CriticParams
    if len(critic) != 6:
        raise ValueError("a critic is 6 tensors: fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b")
    return CriticParams(*critic, tuple(inputs))


@torch.library.custom_op(f"{_NS}::qr_critic_values", mutates_args=("value",))
def qr_critic_values(critic: List[torch.Tensor], inputs: List[int], obs0: Optional[torch.Tensor], obs1: Optional[torch.Tensor],
                     value: torch.Tensor) -> None:
    """V(row) of the reference's MLP critic for every observation row (qr_critic_values).  critic = fc1_w, fc1_b, fc2_w, fc2_b, fc3_w,
    fc3_b; inputs = [0], [1] or [0, 1]: the row tensors it reads (obsK: contiguous float32 [.., D_k]); value: float32, one element
    per row with one element stride (`values[..., k]` of a contiguous [.., n_agents] tensor)."""
    from .policy import critic_values
    _gpu(value)
    critic_values(_critic_params(critic, inputs), (obs0, obs1), value)


@torch.library.custom_op(f"{_NS}::qr_critic_next_values", mutates_args=("next_value",))
def qr_critic_next_values(critic: List[torch.Tensor], inputs: List[int], final_obs0: Optional[torch.Tensor], final_obs1: Optional[torch.Tensor],
                          done: torch.Tensor, truncated: Optional[torch.Tensor], value: torch.Tensor, next_value: torch.Tensor) -> None:
    """The reference's V(obs_next) of a [T, N] horizon (qr_critic_next_values): V(final_obs) where the env was re-sampled (any agent's
    done [T, N, n_agents], or truncated [T, N]), value[t+1] elsewhere.  value [T+1, N], next_value [T, N]: float32, the same single
    element stride.  Critic as in qr_critic_values."""
    from .policy import critic_next_values
    _gpu(next_value)
    critic_next_values(_critic_params(critic, inputs), (final_obs0, final_obs1), done, truncated, value, next_value)


@torch.library.custom_op(f"{_NS}::qr_ppo_actor_grad", mutates_args=("grads", "stats"))
def qr_ppo_actor_grad(actor: List[torch.Tensor], obs: torch.Tensor, final_obs: Optional[torch.Tensor], done: Optional[torch.Tensor],
                      truncated: Optional[torch.Tensor], action: torch.Tensor, logp_old: torch.Tensor, advantage: torch.Tensor,
                      index: Optional[torch.Tensor], noise: Optional[torch.Tensor], nominal: Optional[torch.Tensor],
                      grads: List[torch.Tensor], stats: torch.Tensor, col_offset: int, clip: float, entropy_coef: float, lam_T: float,
                      lam_S: float, lam_M: float, max_action: float, max_workgroups: int = 0) -> None:
    """PPO's actor loss and its gradients for one agent and one minibatch (qr_ppo_actor_grad).  actor = fc1_w, fc1_b, fc2_w, fc2_b,
    mean_w, mean_b, log_std; grads = seven float32 tensors of those sizes, overwritten; stats float32 [4].  Everything else as
    policy.ppo_actor_grad."""
    from .policy import ActorParams, ppo_actor_grad
    _gpu(obs)
    if len(actor) != 7 or len(grads) != 7:
        raise ValueError("the actor and its gradients are 7 tensors each: fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, log_std")
    ppo_actor_grad(ActorParams(*actor[:6], actor[6].reshape(-1)), obs, action, logp_old, advantage, index, final_obs=final_obs, done=done,
                   truncated=truncated, clip=clip, entropy_coef=entropy_coef, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M, noise=noise,
                   nominal=nominal, max_action=max_action, col_offset=col_offset, grads=dict(zip(_lib.PPO_GRAD_NAMES, grads)), stats=stats,
                   max_workgroups=max_workgroups)


@torch.library.custom_op(f"{_NS}::qr_ppo_actor_grad_dev", mutates_args=("grads", "stats"))
def qr_ppo_actor_grad_dev(actor: List[torch.Tensor], obs: torch.Tensor, final_obs: Optional[torch.Tensor], done: Optional[torch.Tensor],
                          truncated: Optional[torch.Tensor], action: torch.Tensor, logp_old: torch.Tensor, advantage: torch.Tensor,
                          index: Optional[torch.Tensor], noise: Optional[torch.Tensor], nominal: Optional[torch.Tensor],
                          grads: List[torch.Tensor], stats: torch.Tensor, entropy_coef_dev: torch.Tensor, col_offset: int, clip: float,
                          lam_T: float, lam_S: float, lam_M: float, max_action: float, max_workgroups: int = 0) -> None:
    """qr_ppo_actor_grad with the entropy coefficient read from the float32 device tensor of one element `entropy_coef_dev`
    (qr_ppo_actor_grad_dev); everything else as that op."""
    from .policy import ActorParams, ppo_actor_grad
    _gpu(obs)
    if len(actor) != 7 or len(grads) != 7:
        raise ValueError("the actor and its gradients are 7 tensors each: fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, log_std")
    ppo_actor_grad(ActorParams(*actor[:6], actor[6].reshape(-1)), obs, action, logp_old, advantage, index, final_obs=final_obs, done=done,
                   truncated=truncated, clip=clip, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M, noise=noise, nominal=nominal, max_action=max_action,
                   col_offset=col_offset, grads=dict(zip(_lib.PPO_GRAD_NAMES, grads)), stats=stats, max_workgroups=max_workgroups,
                   entropy_coef_dev=entropy_coef_dev)


@torch.library.custom_op(f"{_NS}::qr_ppo_critic_grad", mutates_args=("grads", "stats"))
def qr_ppo_critic_grad(critic: List[torch.Tensor], inputs: List[int], obs0: Optional[torch.Tensor], obs1: Optional[torch.Tensor],
                       target: torch.Tensor, index: Optional[torch.Tensor], grads: List[torch.Tensor], stats: torch.Tensor,
                       l2_reg: float, max_workgroups: int = 0) -> None:
    """PPO's critic loss and its gradients for one critic and one minibatch (qr_ppo_critic_grad).  Critic and inputs as in
    qr_critic_values; grads = six float32 tensors of the critic's sizes, overwritten; stats float32 [4].  Everything else as
    policy.ppo_critic_grad."""
    from .policy import ppo_critic_grad
    _gpu(target)
    if len(grads) != 6:
        raise ValueError("a critic's gradients are 6 tensors: fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b")
    ppo_critic_grad(_critic_params(critic, inputs), (obs0, obs1), target, index, l2_reg=l2_reg, grads=dict(zip(_lib.PPO_CRITIC_GRAD_NAMES, grads)),
                    stats=stats, max_workgroups=max_workgroups)


@torch.library.custom_op(f"{_NS}::qr_adamw_step", mutates_args=("params", "exp_avg", "exp_avg_sq", "step", "stats"))
def qr_adamw_step(params: List[torch.Tensor], grads: List[torch.Tensor], exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: torch.Tensor,
                  stats: Optional[torch.Tensor], lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, max_norm: float,
                  t0: int, eta_min: float) -> None:
    """Gradient-norm clipping, one AdamW step and the cosine schedule for one parameter group (qr_adamw_step): params updated in place
    from grads (read only), the moments and the int64 step counter in place, stats float32 [4] or None.  Everything else as
    optim.adamw_step."""
    from .optim import adamw_step
    _gpu(exp_avg)
    adamw_step(params, grads, exp_avg, exp_avg_sq, step, stats, lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=weight_decay,
               max_norm=max_norm, t0=t0, eta_min=eta_min)


@torch.library.custom_op(f"{_NS}::qr_adamw_polyak_step", mutates_args=("params", "targets", "exp_avg", "exp_avg_sq", "step", "stats", "exp_out"))
def qr_adamw_polyak_step(params: List[torch.Tensor], grads: List[torch.Tensor], targets: List[torch.Tensor], target_slots: List[int],
                         exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: torch.Tensor, stats: Optional[torch.Tensor],
                         exp_out: Optional[torch.Tensor], tau: float, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
                         max_norm: float, t0: int, eta_min: float) -> None:
    """qr_adamw_step for one group of up to 16 tensors with the soft target update and exp_out in the same launch
    (qr_adamw_polyak_step).  targets[j] is the target of params[target_slots[j]] (both empty: no targets); exp_out float32 [1] or
    None.  Everything else as optim.adamw_polyak_step."""
    from .optim import adamw_polyak_step
    _gpu(exp_avg)
    if len(targets) != len(target_slots) or len(set(target_slots)) != len(target_slots) or any(not 0 <= k < len(params) for k in target_slots):
        raise ValueError("target_slots names one distinct parameter per target")
    per_param: List[Optional[torch.Tensor]] = [None] * len(params)
    for k, t in zip(target_slots, targets):
        per_param[k] = t
    adamw_polyak_step(params, grads, per_param if targets else None, exp_avg, exp_avg_sq, step, stats, exp_out, tau=tau, lr=lr,
                      betas=(beta1, beta2), eps=eps, weight_decay=weight_decay, max_norm=max_norm, t0=t0, eta_min=eta_min)


def _qcritic_params(critic: Sequence[torch.Tensor], action_dim: int):
    from .policy import QCriticParams
    if len(critic) != 12:
        raise ValueError("a twin critic is 12 tensors: fc1_w, fc1_b, ..., fc6_w, fc6_b")
    return QCriticParams(*critic, int(action_dim))


@torch.library.custom_op(f"{_NS}::qr_twinq_target", mutates_args=("y",))
def qr_twinq_target(actor: List[torch.Tensor], critic: List[torch.Tensor], action_dim: int, obs_next: torch.Tensor, reward: torch.Tensor,
                  done: torch.Tensor, index: Optional[torch.Tensor], noise: Optional[torch.Tensor], action_next: Optional[torch.Tensor],
                  y: torch.Tensor, discount: float, target_noise: float, noise_clip: float, max_action: float) -> None:
    """TD3's target values of one minibatch (qr_twinq_target).  actor: the target actor's six tensors fc1_w, fc1_b, fc2_w, fc2_b, fc3_w,
    fc3_b, or an empty list with action_next; critic: the target critic's twelve tensors.  Everything else as td3.td3_target."""
    from .policy import ActorParams
    from .td3 import td3_target
    _gpu(y)
    if len(actor) not in (0, 6):
        raise ValueError("a TD3 actor is 6 tensors: fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b")
    td3_target(ActorParams(*actor, None) if actor else None, _qcritic_params(critic, action_dim),
               {"obs_next": obs_next, "rwd": reward, "done": done}, 0, index, discount=discount, target_noise=target_noise,
               noise_clip=noise_clip, max_action=max_action, noise=noise, action_next=action_next, out=y)


@torch.library.custom_op(f"{_NS}::qr_twinq_grad", mutates_args=("grads", "stats"))
def qr_twinq_grad(critic: List[torch.Tensor], action_dim: int, obs: torch.Tensor, action: torch.Tensor, y: torch.Tensor,
                  index: Optional[torch.Tensor], grads: List[torch.Tensor], stats: torch.Tensor, max_workgroups: int = 0) -> None:
    """The twin-Q loss against y and its twelve gradients for one minibatch (qr_twinq_grad).  critic and grads: twelve tensors each, fc1_w,
    fc1_b, ..., fc6_w, fc6_b; stats float32 [4].  Everything else as td3.twinq_grad."""
    from .td3 import twinq_grad
    _gpu(stats)
    if len(grads) != 12:
        raise ValueError("grads is 12 tensors: fc1_w, fc1_b, ..., fc6_w, fc6_b")
    twinq_grad(_qcritic_params(critic, action_dim), obs, action, y, index, grads=dict(zip(_lib.TWINQ_GRAD_NAMES, grads)), stats=stats,
               max_workgroups=max_workgroups)


@torch.library.custom_op(f"{_NS}::qr_dpg_actor_grad", mutates_args=("grads", "stats"))
def qr_dpg_actor_grad(actor: List[torch.Tensor], critic: List[torch.Tensor], action_dim: int, obs: torch.Tensor, obs_next: Optional[torch.Tensor],
                      index: Optional[torch.Tensor], noise: Optional[torch.Tensor], nominal: Optional[torch.Tensor], grads: List[torch.Tensor],
                      stats: torch.Tensor, lam_T: float, lam_S: float, lam_M: float, max_action: float, max_workgroups: int = 0) -> None:
    """TD3's actor loss and its six gradients for one minibatch (qr_dpg_actor_grad).  actor and grads: six tensors each, fc1_w, fc1_b,
    fc2_w, fc2_b, fc3_w, fc3_b; critic: the twin critic's twelve; stats float32 [4].  Everything else as td3.dpg_actor_grad."""
    from .policy import ActorParams
    from .td3 import dpg_actor_grad
    _gpu(stats)
    if len(actor) != 6 or len(grads) != 6:
        raise ValueError("a TD3 actor and its gradients are 6 tensors each: fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b")
    dpg_actor_grad(ActorParams(*actor, None), _qcritic_params(critic, action_dim), obs, obs_next, index, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M,
                   max_action=max_action, noise=noise, nominal=nominal, grads=dict(zip(_lib.DPG_GRAD_NAMES, grads)), stats=stats,
                   max_workgroups=max_workgroups)


@torch.library.custom_op(f"{_NS}::qr_soft_update", mutates_args=("targets",))
def qr_soft_update(params: List[torch.Tensor], targets: List[torch.Tensor], tau: float) -> None:
    """target = tau * param + (1 - tau) * target for up to 24 tensor pairs in one launch (qr_soft_update), as td3.soft_update."""
    from .td3 import soft_update
    _gpu(targets[0])
    soft_update(list(params), list(targets), tau)


@torch.library.custom_op(f"{_NS}::qr_replay_add", mutates_args=("buffers", "state"))
def qr_replay_add(buffers: List[torch.Tensor], obs: List[torch.Tensor], final_obs: List[torch.Tensor], action: torch.Tensor, reward: torch.Tensor,
                  done: torch.Tensor, truncated: Optional[torch.Tensor], count: int, state: Optional[torch.Tensor]) -> None:
    """One horizon into the ring of a flat transition buffer in one launch (qr_replay_add), as td3.replay_add.  buffers: per agent (one
    or two) its five tensors obs, obs_next, act, rwd, done, one agent after the other; obs: one [T + 1, N, D_k] tensor per agent;
    final_obs: one [T, N, D_k] per agent, or an empty list; state: the int64 [3] device counters, which win over count."""
    from .td3 import replay_add
    _gpu(action)
    if len(buffers) not in (5, 10):
        raise ValueError("a replay buffer is 5 tensors per agent: obs, obs_next, act, rwd, done")
    tensors = [dict(zip(_lib.REPLAY_BUFFER_NAMES, buffers[5 * k:5 * k + 5])) for k in range(len(buffers) // 5)]
    replay_add(tensors, list(obs), list(final_obs) if final_obs else None, action, reward, done, truncated, count, state=state)


@torch.library.custom_op(f"{_NS}::qr_replay_add_rule", mutates_args=("buffers", "state"))
def qr_replay_add_rule(buffers: List[torch.Tensor], obs: List[torch.Tensor], final_obs: List[torch.Tensor], action: torch.Tensor, reward: torch.Tensor,
                       done: torch.Tensor, truncated: torch.Tensor, count: int, state: Optional[torch.Tensor], x_lim: float, pos_tol: float,
                       rot_tol: float) -> None:
    """qr_replay_add with the reference's time-limit "solved" rule in the done it stores (qr_replay_add_rule), as td3.replay_add with
    time_limit_rule=(x_lim, pos_tol, rot_tol); the other arguments as qr_replay_add's, truncated required."""
    from .td3 import TimeLimitRule, replay_add
    _gpu(action)
    if len(buffers) not in (5, 10):
        raise ValueError("a replay buffer is 5 tensors per agent: obs, obs_next, act, rwd, done")
    tensors = [dict(zip(_lib.REPLAY_BUFFER_NAMES, buffers[5 * k:5 * k + 5])) for k in range(len(buffers) // 5)]
    replay_add(tensors, list(obs), list(final_obs) if final_obs else None, action, reward, done, truncated, count, state=state,
               time_limit_rule=TimeLimitRule(x_lim, pos_tol, rot_tol))


@torch.library.custom_op(f"{_NS}::qr_replay_sample", mutates_args=("out", "state", "status"))
def qr_replay_sample(out: torch.Tensor, n: int, seed: int, draw: int, state: Optional[torch.Tensor], status: Optional[torch.Tensor]) -> None:
    """out.numel() pairwise distinct rows below n in one O(B) launch (qr_replay_sample), as td3.replay_sample; seed and draw are passed as
    int64 here (0 <= seed, draw < 2^63).  state: the int64 [3] device counters, whose current_size and draw win over n and draw."""
    from .td3 import replay_sample
    _gpu(out)
    replay_sample(n, out.numel(), seed, draw, out, state=state, status=status)


@torch.library.custom_op(f"{_NS}::qr_noise_fill", mutates_args=("tensors",))
def qr_noise_fill(tensors: List[torch.Tensor], kinds: List[int], a: List[float], b: List[float], streams: List[int], seed: int, draw: int,
                  draw_dev: Optional[torch.Tensor]) -> None:
    """Fill float32 tensors with normal (kind 0) or uniform (kind 1) draws of the library's counter-based stream (qr_noise_fill), as
    noise.noise_fill: one kind, a, b and stream id per tensor; seed and draw are passed as int64 here (0 <= seed, draw < 2^63).
    draw_dev: an int64 device tensor of one element that is read as the draw number instead of `draw`, or None."""
    from .noise import KINDS, noise_fill
    _gpu(tensors[0])
    if any(k not in (0, 1) for k in kinds):
        raise ValueError("kinds are 0 (normal) or 1 (uniform)")
    noise_fill(list(tensors), seed=seed, draw=draw, streams=list(streams), kind=[KINDS[k] for k in kinds], a=list(a), b=list(b), draw_dev=draw_dev)


@torch.library.custom_op(f"{_NS}::qr_shuffle", mutates_args=("out",))
def qr_shuffle(out: torch.Tensor, n: int, first: int, seed: int, draw: int, stream: int, draw_dev: Optional[torch.Tensor],
               max_workgroups: int = 0) -> None:
    """out[i] = perm(first + i), the keyed permutation of [0, n) (qr_shuffle), as shuffle.shuffle; seed and draw are passed as int64
    here (0 <= seed, draw < 2^63).  draw_dev: an int64 device tensor of one element that is read as the draw number, or None."""
    from .shuffle import shuffle
    _gpu(out)
    shuffle(out, n=n, seed=seed, draw=draw, stream=stream, first=first, draw_dev=draw_dev, max_workgroups=max_workgroups)


@torch.library.custom_op(f"{_NS}::qr_es_perturb", mutates_args=("out", "copy_dst"))
def qr_es_perturb(base: List[torch.Tensor], out: List[torch.Tensor], copy_src: List[torch.Tensor], copy_dst: List[torch.Tensor], streams: List[int],
                  sigma: float, seed: int, generation: int, generation_dev: Optional[torch.Tensor], max_workgroups: int) -> None:
    """The antithetic evolution-strategy population around `base` in one launch (qr_es_perturb), as es.es_perturb_tensors: out[i]
    [P, ...] gets base[i] +- sigma eps in its even / odd rows, copy_dst[c] [P, ...] gets copy_src[c] in every row; one stream id per
    base tensor; seed and generation are passed as int64 here.  generation_dev: an int64 device tensor of one element that is read as
    the generation instead of `generation`, or None."""
    from .es import es_perturb_tensors
    _gpu(out[0])
    if len(copy_src) != len(copy_dst):
        raise ValueError("copy_src and copy_dst must pair up")
    es_perturb_tensors(list(base), list(out), sigma=sigma, seed=seed, generation=generation if generation_dev is None else generation_dev,
                       streams=list(streams), copies=list(zip(copy_src, copy_dst)), max_workgroups=max_workgroups)


@torch.library.custom_op(f"{_NS}::qr_es_gradient", mutates_args=("grads", "stats", "workspace"))
def qr_es_gradient(fitness: torch.Tensor, grads: List[torch.Tensor], stats: torch.Tensor, workspace: torch.Tensor, streams: List[int], sigma: float,
                   seed: int, generation: int, generation_dev: Optional[torch.Tensor], shaping: int, max_workgroups: int) -> None:
    """The shaped fitness and the evolution-strategy gradient estimate in one C call (qr_es_gradient), as es.es_gradient on a flat
    list of gradient tensors: shaping 0 = centered ranks, 1 = standardised fitness; stats float64 [4]; workspace float64
    [es.es_workspace_numel(P)]."""
    from .es import SHAPINGS, es_gradient
    _gpu(fitness)
    if shaping not in (0, 1):
        raise ValueError("shaping is 0 (centered_rank) or 1 (standardize)")
    es_gradient(fitness, list(grads), sigma=sigma, seed=seed, generation=generation if generation_dev is None else generation_dev,
                streams=list(streams), shaping=SHAPINGS[shaping], stats=stats, workspace=workspace, max_workgroups=max_workgroups)


@torch.library.custom_op(f"{_NS}::qr_episode_scan", mutates_args=("run_return", "run_length", "last", "total", "ep_return", "ep_length", "ep_flags",
                                                                  "ep_final_error", "workspace"))
def qr_episode_scan(reward: torch.Tensor, done: torch.Tensor, truncated: torch.Tensor, final_obs: List[torch.Tensor], run_return: torch.Tensor,
                    run_length: torch.Tensor, last: torch.Tensor, total: torch.Tensor, ep_return: Optional[torch.Tensor],
                    ep_length: Optional[torch.Tensor], ep_flags: Optional[torch.Tensor], ep_final_error: Optional[torch.Tensor],
                    workspace: torch.Tensor, x_lim: float, pos_tol: float, rot_tol: float, record: bool) -> None:
    """One collected horizon's rows into per-episode records and statistics in one C call (qr_episode_scan), as episodes.episode_scan:
    final_obs one [T, N, D_k] tensor per agent, or an empty list; the four dense outputs optional; workspace float64
    [episodes.episode_workspace_numel(N)]."""
    from .episodes import episode_scan
    from .td3 import TimeLimitRule
    _gpu(reward)
    episode_scan(reward, done, truncated, run_return, run_length, last, total, final_obs=list(final_obs) if final_obs else None,
                 rule=TimeLimitRule(x_lim, pos_tol, rot_tol), record=record, ep_return=ep_return, ep_length=ep_length, ep_flags=ep_flags,
                 ep_final_error=ep_final_error, workspace=workspace)


@torch.library.custom_op(f"{_NS}::qr_gae_rule", mutates_args=("advantage", "td_target", "done_eff", "stats", "normalized", "workspace"))
def qr_gae_rule(reward: torch.Tensor, done: torch.Tensor, truncated: Optional[torch.Tensor], term_obs: List[torch.Tensor], value: torch.Tensor,
                next_value: Optional[torch.Tensor], advantage: torch.Tensor, td_target: torch.Tensor, done_eff: Optional[torch.Tensor],
                stats: Optional[torch.Tensor], normalized: Optional[torch.Tensor], workspace: Optional[torch.Tensor], gamma: float, lam: float,
                rule: bool, x_lim: float, pos_tol: float, rot_tol: float, norm_eps: float) -> None:
    """PPO's advantages over the done flag the reference stores, their per-agent statistics and their normalisation in one C call
    (qr_gae_rule), as rollout.gae_rule: term_obs one [T, N, D_k] tensor per agent, or an empty list with rule=False (x_lim, pos_tol and
    rot_tol are then not read); done_eff, stats, normalized optional; workspace float64 [rollout.gae_rule_workspace_numel(N, n_agents)],
    needed with stats."""
    from .rollout import gae_rule
    from .td3 import TimeLimitRule
    _gpu(reward)
    gae_rule(reward, done, value, advantage, td_target, gamma=gamma, lam=lam, next_value=next_value, truncated=truncated,
             term_obs=list(term_obs) if term_obs else None, rule=TimeLimitRule(x_lim, pos_tol, rot_tol) if rule else None, done_eff=done_eff,
             stats=stats, normalized=normalized, workspace=workspace, norm_eps=norm_eps)


@torch.library.custom_op(f"{_NS}::qr_sac_target", mutates_args=("y", "action_out", "logp_out"))
def qr_sac_target(actor: List[torch.Tensor], critic: List[torch.Tensor], action_dim: int, obs_next: torch.Tensor, reward: torch.Tensor,
                  done: torch.Tensor, index: Optional[torch.Tensor], noise: Optional[torch.Tensor], action_next: Optional[torch.Tensor],
                  logp_next: Optional[torch.Tensor], y: torch.Tensor, action_out: Optional[torch.Tensor], logp_out: Optional[torch.Tensor],
                  discount: float, alpha: float, alpha_dev: Optional[torch.Tensor] = None) -> None:
    """SAC's target values of one minibatch (qr_sac_target).  actor: the live actor's eight tensors fc1_w, fc1_b, fc2_w, fc2_b, mean_w,
    mean_b, log_std_w, log_std_b, or an empty list with action_next and logp_next; critic: the target critic's twelve tensors; alpha_dev:
    the temperature as a device tensor of one element, which wins over alpha.  Everything else as sac.sac_target."""
    from .policy import ActorParams
    from .sac import sac_target
    _gpu(y)
    if len(actor) not in (0, 8):
        raise ValueError("a SAC actor is 8 tensors: fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, log_std_w, log_std_b")
    sac_target(ActorParams(*actor[:6], None, actor[6], actor[7], _lib.ACTOR_TANH_SAMPLE) if actor else None, _qcritic_params(critic, action_dim),
               {"obs_next": obs_next, "rwd": reward, "done": done}, 0, index, discount=discount, alpha=alpha if alpha_dev is None else alpha_dev,
               noise=noise, action_next=action_next, logp_next=logp_next, out=y, action_out=action_out, logp_out=logp_out)


def _ctde_agents(obs_next0, obs_next1, act0, act1, reward, done, k: int):
    """The pair of per-agent dicts the centralized helpers take; reward and done are agent k's."""
    t = [{"obs_next": obs_next0, "act": act0}, {"obs_next": obs_next1, "act": act1}]
    if k in (0, 1):
        t[k].update(rwd=reward, done=done)
    return t


@torch.library.custom_op(f"{_NS}::qr_ctde_twinq_target", mutates_args=("y",))
def qr_ctde_twinq_target(actors: List[torch.Tensor], critic: List[torch.Tensor], obs_next0: torch.Tensor, obs_next1: torch.Tensor,
                         action0: torch.Tensor, action1: torch.Tensor, reward: torch.Tensor, done: torch.Tensor, index: Optional[torch.Tensor],
                         noise0: Optional[torch.Tensor], noise1: Optional[torch.Tensor], action_next0: Optional[torch.Tensor],
                         action_next1: Optional[torch.Tensor], y: torch.Tensor, discount: float, target_noise: float, noise_clip: float,
                         max_action: float) -> None:
    """TD3's target values for the centralized critic of two agents (qr_ctde_twinq_target).  actors: both target actors' six tensors each
    (twelve: agent 0's fc1_w .. fc3_b, then agent 1's), or an empty list with action_next0 / action_next1; critic: the target critic's
    twelve; action0, action1: the agents' action tensors (their widths are read); reward, done: the columns of the agent whose target
    this is.  Everything else as td3.td3_target_ctde."""
    from .policy import ActorParams
    from .td3 import td3_target_ctde
    _gpu(y)
    if len(actors) not in (0, 12):
        raise ValueError("two TD3 actors are 12 tensors: fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b of agent 0, then of agent 1")
    pair = [ActorParams(*actors[6 * m:6 * m + 6], None) for m in range(2)] if actors else None
    td3_target_ctde(pair, _qcritic_params(critic, action0.shape[-1] + action1.shape[-1]),
                    _ctde_agents(obs_next0, obs_next1, action0, action1, reward, done, 0), 0, index, discount=discount, target_noise=target_noise,
                    noise_clip=noise_clip, max_action=max_action, noise=(noise0, noise1),
                    action_next=None if action_next0 is None and action_next1 is None else (action_next0, action_next1), out=y)


@torch.library.custom_op(f"{_NS}::qr_ctde_sac_target", mutates_args=("y", "action_out0", "action_out1", "logp_out"))
def qr_ctde_sac_target(actors: List[torch.Tensor], critic: List[torch.Tensor], agent: int, obs_next0: torch.Tensor, obs_next1: torch.Tensor,
                       action0: torch.Tensor, action1: torch.Tensor, reward: torch.Tensor, done: torch.Tensor, index: Optional[torch.Tensor],
                       noise0: Optional[torch.Tensor], noise1: Optional[torch.Tensor], noise_logp: Optional[torch.Tensor],
                       action_next0: Optional[torch.Tensor], action_next1: Optional[torch.Tensor], logp_next: Optional[torch.Tensor], y: torch.Tensor,
                       action_out0: Optional[torch.Tensor], action_out1: Optional[torch.Tensor], logp_out: Optional[torch.Tensor], discount: float,
                       alpha: float, alpha_dev: Optional[torch.Tensor] = None) -> None:
    """SAC's target values for the centralized critic of two agents (qr_ctde_sac_target).  actors: both live actors' eight tensors each
    (sixteen: agent 0's fc1_w .. log_std_b, then agent 1's), or an empty list with action_next0 / action_next1 and logp_next; agent: whose
    reward, done and log-probability.  Everything else as qr_ctde_twinq_target's and sac.sac_target_ctde."""
    from .policy import ActorParams
    from .sac import sac_target_ctde
    _gpu(y)
    if len(actors) not in (0, 16):
        raise ValueError("two SAC actors are 16 tensors: fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, log_std_w, log_std_b of agent 0, then of agent 1")
    pair = [ActorParams(*actors[8 * m:8 * m + 6], None, actors[8 * m + 6], actors[8 * m + 7], _lib.ACTOR_TANH_SAMPLE) for m in range(2)] if actors else None
    sac_target_ctde(pair, _qcritic_params(critic, action0.shape[-1] + action1.shape[-1]),
                    _ctde_agents(obs_next0, obs_next1, action0, action1, reward, done, agent), agent, index, discount=discount,
                    alpha=alpha if alpha_dev is None else alpha_dev, noise=(noise0, noise1), noise_logp=noise_logp,
                    action_next=None if action_next0 is None and action_next1 is None else (action_next0, action_next1), logp_next=logp_next,
                    out=y, action_out=(action_out0, action_out1), logp_out=logp_out)


@torch.library.custom_op(f"{_NS}::qr_ctde_twinq_grad", mutates_args=("grads", "stats"))
def qr_ctde_twinq_grad(critic: List[torch.Tensor], obs0: torch.Tensor, obs1: torch.Tensor, action0: torch.Tensor, action1: torch.Tensor,
                       y: torch.Tensor, index: Optional[torch.Tensor], grads: List[torch.Tensor], stats: torch.Tensor, max_workgroups: int = 0) -> None:
    """The twin-Q loss of the centralized critic against y and its twelve gradients (qr_ctde_twinq_grad); as qr_twinq_grad, with the row
    formed from obs0, obs1, action0, action1 in the kernel.  Everything else as td3.twinq_grad_ctde."""
    from .td3 import twinq_grad_ctde
    _gpu(stats)
    if len(grads) != 12:
        raise ValueError("grads is 12 tensors: fc1_w, fc1_b, ..., fc6_w, fc6_b")
    twinq_grad_ctde(_qcritic_params(critic, action0.shape[-1] + action1.shape[-1]), (obs0, obs1), (action0, action1), y, index,
                    grads=dict(zip(_lib.TWINQ_GRAD_NAMES, grads)), stats=stats, max_workgroups=max_workgroups)


@torch.library.custom_op(f"{_NS}::qr_ctde_dpg_actor_grad", mutates_args=("grads", "stats"))
def qr_ctde_dpg_actor_grad(actor0: List[torch.Tensor], actor1: List[torch.Tensor], critic: List[torch.Tensor], agent: int, obs0: torch.Tensor,
                           obs1: torch.Tensor, obs_next: Optional[torch.Tensor], index: Optional[torch.Tensor], action_other: Optional[torch.Tensor],
                           noise: Optional[torch.Tensor], nominal: Optional[torch.Tensor], grads: List[torch.Tensor], stats: torch.Tensor, lam_T: float,
                           lam_S: float, lam_M: float, max_action: float, max_workgroups: int = 0) -> None:
    """Agent `agent`'s TD3 actor loss under the centralized critic of two agents and its six gradients (qr_ctde_dpg_actor_grad).  actor0,
    actor1: six tensors each, fc1_w .. fc3_b; the other agent's may be an empty list with action_other.  critic: the centralized twin
    critic's twelve; obs_next: agent `agent`'s own; grads: that agent's six.  Everything else as td3.dpg_actor_grad_ctde."""
    from .policy import ActorParams
    from .td3 import dpg_actor_grad_ctde
    _gpu(stats)
    if len(actor0) not in (0, 6) or len(actor1) not in (0, 6) or len(grads) != 6:
        raise ValueError("a TD3 actor and its gradients are 6 tensors each: fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b")
    pair = [ActorParams(*a, None) if a else None for a in (actor0, actor1)]
    if agent not in (0, 1) or pair[agent] is None:
        raise ValueError("agent must be 0 or 1 and that agent's actor given")
    a_other = action_other.shape[-1] if action_other is not None else (pair[1 - agent].dims[2] if pair[1 - agent] is not None else 0)
    dpg_actor_grad_ctde(pair, _qcritic_params(critic, pair[agent].dims[2] + a_other), (obs0, obs1), (obs_next, None) if agent == 0 else (None, obs_next),
                        index, k=agent, action_other=action_other, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M, max_action=max_action, noise=noise,
                        nominal=nominal, grads=dict(zip(_lib.DPG_GRAD_NAMES, grads)), stats=stats, max_workgroups=max_workgroups)


@torch.library.custom_op(f"{_NS}::qr_sac_actor_grad", mutates_args=("grads", "stats", "alpha_grad"))
def qr_sac_actor_grad(actor: List[torch.Tensor], critic: List[torch.Tensor], action_dim: int, obs: torch.Tensor, obs_next: Optional[torch.Tensor],
                      index: Optional[torch.Tensor], eps: Optional[torch.Tensor], eps_reg: Optional[torch.Tensor], eps_next: Optional[torch.Tensor],
                      eps_pert: Optional[torch.Tensor], noise: Optional[torch.Tensor], nominal: Optional[torch.Tensor], grads: List[torch.Tensor],
                      stats: torch.Tensor, alpha_grad: Optional[torch.Tensor], alpha: float, target_entropy: float, lam_T: float, lam_S: float,
                      lam_M: float, max_action: float, alpha_dev: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> None:
    """SAC's actor loss and its eight gradients for one minibatch (qr_sac_actor_grad).  actor and grads: eight tensors each, fc1_w, fc1_b,
    fc2_w, fc2_b, mean_w, mean_b, log_std_w, log_std_b; critic: the twin critic's twelve; stats float32 [6]; alpha_dev: the temperature
    as a device tensor of one element, which wins over alpha.  Everything else as sac.sac_actor_grad."""
    from .policy import ActorParams
    from .sac import sac_actor_grad
    _gpu(stats)
    if len(actor) != 8 or len(grads) != 8:
        raise ValueError("a SAC actor and its gradients are 8 tensors each: fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, log_std_w, log_std_b")
    sac_actor_grad(ActorParams(*actor[:6], None, actor[6], actor[7], _lib.ACTOR_TANH_SAMPLE), _qcritic_params(critic, action_dim), obs, obs_next,
                   index, alpha=alpha if alpha_dev is None else alpha_dev, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M, max_action=max_action,
                   eps=eps, eps_reg=eps_reg, eps_next=eps_next, eps_pert=eps_pert, noise=noise, nominal=nominal, alpha_grad=alpha_grad,
                   target_entropy=target_entropy, grads=dict(zip(_lib.SAC_ACTOR_GRAD_NAMES, grads)), stats=stats, max_workgroups=max_workgroups)


@torch.library.custom_op(f"{_NS}::qr_ctde_sac_actor_grad", mutates_args=("grads", "stats", "alpha_grad"))
def qr_ctde_sac_actor_grad(actor0: List[torch.Tensor], actor1: List[torch.Tensor], critic: List[torch.Tensor], agent: int, obs0: torch.Tensor,
                           obs1: torch.Tensor, obs_next: Optional[torch.Tensor], index: Optional[torch.Tensor], action_other: Optional[torch.Tensor],
                           eps: Optional[torch.Tensor], eps_logp: Optional[torch.Tensor], eps_other: Optional[torch.Tensor],
                           eps_reg: Optional[torch.Tensor], eps_next: Optional[torch.Tensor], eps_pert: Optional[torch.Tensor],
                           noise: Optional[torch.Tensor], nominal: Optional[torch.Tensor], grads: List[torch.Tensor], stats: torch.Tensor,
                           alpha_grad: Optional[torch.Tensor], alpha: float, target_entropy: float, lam_T: float, lam_S: float, lam_M: float,
                           max_action: float, alpha_dev: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> None:
    """Agent `agent`'s SAC actor loss under the centralized twin critic of two agents and its eight gradients (qr_ctde_sac_actor_grad).
    actor0, actor1: eight tensors each, fc1_w .. log_std_b; the other agent's may be an empty list with action_other.  critic: the
    centralized twin critic's twelve; obs_next: agent `agent`'s own; grads: that agent's eight; stats float32 [6]; alpha_dev wins over
    alpha.  Everything else as sac.sac_actor_grad_ctde."""
    from .policy import ActorParams
    from .sac import sac_actor_grad_ctde
    _gpu(stats)
    if len(actor0) not in (0, 8) or len(actor1) not in (0, 8) or len(grads) != 8:
        raise ValueError("a SAC actor and its gradients are 8 tensors each: fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, log_std_w, log_std_b")
    pair = [ActorParams(*a[:6], None, a[6], a[7], _lib.ACTOR_TANH_SAMPLE) if a else None for a in (actor0, actor1)]
    if agent not in (0, 1) or pair[agent] is None:
        raise ValueError("agent must be 0 or 1 and that agent's actor given")
    a_other = action_other.shape[-1] if action_other is not None else (pair[1 - agent].dims[2] if pair[1 - agent] is not None else 0)
    sac_actor_grad_ctde(pair, _qcritic_params(critic, pair[agent].dims[2] + a_other), (obs0, obs1), (obs_next, None) if agent == 0 else (None, obs_next),
                        index, k=agent, action_other=action_other, alpha=alpha if alpha_dev is None else alpha_dev, lam_T=lam_T, lam_S=lam_S,
                        lam_M=lam_M, max_action=max_action, eps=eps, eps_logp=eps_logp, eps_other=eps_other, eps_reg=eps_reg, eps_next=eps_next,
                        eps_pert=eps_pert, noise=noise, nominal=nominal, alpha_grad=alpha_grad, target_entropy=target_entropy,
                        grads=dict(zip(_lib.SAC_ACTOR_GRAD_NAMES, grads)), stats=stats, max_workgroups=max_workgroups)


# ----------------------------------------------------------------------------------------------------------------
# functional wrappers over a QuadVecEnv's own buffers
# ----------------------------------------------------------------------------------------------------------------
def _outs(env, out):
    if out is None:
        out = {"obs0": env._obs0, "obs1": env._obs1, "reward": env._reward, "reward_raw": env._reward_raw, "terminated": env._done,
               "truncated": env._trunc if env._steps is not None else None, "final_obs0": env._final0, "final_obs1": env._final1}
    return tuple(out.get(k) if k != "truncated" or env._steps is not None else None for k in _OUT_KEYS)


def step(env, action: torch.Tensor, out: Optional[dict] = None) -> None:
    """`env.step(action)` as ONE torch op (same buffers, same bits): results land in the env's output tensors (or `out`)."""
    t, cfg, co = env_args(env)
    torch.ops.gym_rotor_amd.qr_step(*t, action, *_outs(env, out), env.substeps, cfg, co)


def rollout(env, actions: torch.Tensor, out: dict) -> None:
    t, cfg, co = env_args(env)
    torch.ops.gym_rotor_amd.qr_rollout(*t, actions, *_outs(env, out), env.substeps, cfg, co)


def rollout_actor(env, actors, n_steps: int, obs, out: dict, noise: Optional[torch.Tensor] = None, noise_seed: Optional[int] = None,
                  step_base: int = 0, max_action: float = 1.0, deterministic: bool = False) -> None:
    t, cfg, co = env_args(env)
    obs = [obs] if isinstance(obs, torch.Tensor) else list(obs)
    lists, squash = _actor_lists(actors)
    torch.ops.gym_rotor_amd.qr_rollout_actor(*t, lists[0], lists[1], squash, obs[0], obs[1] if len(obs) > 1 else None, noise,
                                             out["action"], out.get("logprob"), *_outs(env, out), n_steps, env.substeps,
                                             (env.seed if noise_seed is None else noise_seed) & (2 ** 63 - 1), step_base, max_action,
                                             deterministic, cfg, co)


def _actor_lists(actors):
    lists, squash = [], []
    for a in actors:
        ts = [a.fc1_w, a.fc1_b, a.fc2_w, a.fc2_b, a.mean_w, a.mean_b]
        ts += [a.log_std] if a.log_std_w is None else [a.log_std_w, a.log_std_b]
        lists.append(ts); squash.append(int(a.squash))
    while len(lists) < 2:
        lists.append([]); squash.append(0)
    return lists, squash


def _evaluate_args(env, agents, obs, out, steps, max_action):
    """Positional arguments of the two evaluate ops; steps = ([envs_per_policy,] max_steps), the only part in which they differ."""
    t, cfg, co = env_args(env)
    obs = [obs] if isinstance(obs, torch.Tensor) else list(obs)
    lists, squash = _actor_lists(agents)
    return (*t, lists[0], lists[1], squash, obs[0], obs[1] if len(obs) > 1 else None, out.get("action"), out["episode_return"],
            out["benchmark"], out["length"], out["terminated"], out["success"], out.get("final_error"), out["obs0"], out.get("obs1"),
            *(int(v) for v in steps), env.substeps, float(max_action), cfg, co)


def evaluate(env, actors, max_steps: int, obs, out: dict, max_action: float = 1.0) -> None:
    """`env.evaluate(actors, max_steps, obs)` as ONE torch op on the env's buffers: results land in `out` (the keys of the dict
    QuadVecEnv.evaluate returns; "action" and "final_error" optional)."""
    torch.ops.gym_rotor_amd.qr_evaluate_actor(*_evaluate_args(env, actors, obs, out, (max_steps,), max_action))


def evaluate_population(env, population, envs_per_policy: int, max_steps: int, obs, out: dict, max_action: float = 1.0) -> None:
    """`env.evaluate_population(population, envs_per_policy, max_steps, obs)` as ONE torch op on the env's buffers: results land in
    `out`, per env [N, ...] as QuadVecEnv.evaluate_population returns them ("action" and "final_error" optional)."""
    torch.ops.gym_rotor_amd.qr_evaluate_population(*_evaluate_args(env, population.agents, obs, out, (envs_per_policy, max_steps), max_action))


def error_obs(env, framework: Optional[str] = None, out=None) -> None:
    """get_norm_error_state through the op: the env's own format into its own buffers, or (framework = "MONO" | "MODUL", out = the
    row tensor(s) to fill) the format the argument names."""
    t, cfg, co = env_args(env)
    if framework is None or framework == env.framework:
        torch.ops.gym_rotor_amd.qr_error_obs(t[0], t[1], env._integ, env._goal, env._obs0, env._obs1, cfg, co)
        return
    if framework not in ("MONO", "MODUL"):
        raise ValueError(f"framework must be 'MONO' or 'MODUL', got {framework!r}")
    dims = OBS_DIMS["coupled" if framework == "MONO" else "decoupled"]
    if out is None:
        raise ValueError(f"error_obs(framework={framework!r}) on a {env.framework} env writes the OTHER format: pass out= the row tensor(s) "
                         f"to fill, float32 {[(env.num_envs, d) for d in dims]}")
    rows = [out] if isinstance(out, torch.Tensor) else list(out)
    if len(rows) != len(dims):
        raise ValueError(f"framework {framework!r} has {len(dims)} row tensor(s), got {len(rows)}")
    for r, d in zip(rows, dims):
        if tuple(r.shape) != (env.num_envs, d) or r.dtype != torch.float32 or r.device != env.device or not r.is_contiguous():
            raise ValueError(f"out rows must be contiguous float32 [{env.num_envs}, {d}] on {env.device}")
    fmt = _lib.KIND_ID["coupled" if framework == "MONO" else "decoupled"]
    torch.ops.gym_rotor_amd.qr_error_obs(t[0], t[1], env._integ, env._goal, rows[0], rows[1] if len(rows) > 1 else None, cfg, co, fmt)


def reset(env, env_type: str = "train", mask: Optional[torch.Tensor] = None) -> None:
    """What QuadVecEnv.reset launches: qr_reset, then (fused goal generator) qr_traj_start for the same envs — main.py:226-227;
    the previous episode's observation rows stop being the env's current observation."""
    t, cfg, co = env_args(env)
    rcfg = list(cfg)
    rcfg[2] = (rcfg[2] & ~3) | (2 if env_type == "eval" else 0)  # clear QR_FLAG_AUTO_RESET, select QR_FLAG_EVAL_RESET
    torch.ops.gym_rotor_amd.qr_reset(t[0], t[1], env._integ, env._params, env._episode, env._steps, mask, rcfg, co)
    if env.goal_mode is not None:
        torch.ops.gym_rotor_amd.qr_traj_start(t[0], t[1], env._traj, env._goal, env._episode, mask, None, cfg, co)
    env._last_obs = None


def get_state(env, rows: torch.Tensor) -> None:
    t, cfg, co = env_args(env)
    torch.ops.gym_rotor_amd.qr_get_state(t[0], t[1], rows, cfg, co)


def set_state(env, rows: torch.Tensor, mask: Optional[torch.Tensor] = None, rejected: Optional[torch.Tensor] = None) -> None:
    t, cfg, co = env_args(env)
    torch.ops.gym_rotor_amd.qr_set_state(t[0], t[1], rows, mask, rejected, cfg, co)
