"""ctypes binding of the C-ABI in include/quadrotor_hip.h (libquadrotor_hip.so).

The library is built in-tree by `__graft_entry__.build()` / `make -C gym_rotor_amd/csrc`.
There is deliberately NO fallback: if the shared library is missing or a symbol is absent
the import of the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# QR_LIB overrides the path for measurement builds (the span build, tools/build_ab.sh A/B builds) only.
LIB_PATH = os.environ.get("QR_LIB", os.path.join(_HERE, "libquadrotor_hip.so"))

KIND_QUAD, KIND_COUPLED, KIND_DECOUPLED = 0, 1, 2
KIND_ID = {"quad": KIND_QUAD, "coupled": KIND_COUPLED, "decoupled": KIND_DECOUPLED}
FLAG_AUTO_RESET, FLAG_EVAL_RESET, FLAG_NO_UDM = 1, 2, 4
FLAG_FORCE_HELPER, FLAG_NO_HELPER = 8, 16   # launch-rule overrides of the one-step launch (speed only)
FLAG_CALLER_RESETS = 32                     # the caller resets every done env before stepping it again (one-step launches)
FLAG_FORCE_HELPER_ROLLOUT, FLAG_NO_HELPER_ROLLOUT = 64, 128   # the same overrides for qr_rollout / qr_rollout_actor
ABI_VERSION = 16
GOAL_EXTERNAL, GOAL_MODE0, GOAL_MODE1, GOAL_MODE6, GOAL_MODE2, GOAL_MODE3, GOAL_MODE4, GOAL_MODE5 = 0, 1, 2, 3, 4, 5, 6, 7
GOAL_ID = {None: 0, 0: 1, 1: 2, 6: 3, 2: 4, 3: 5, 4: 6, 5: 7}  # TrajectoryGenerator mode -> QR_GOAL_*
LAYOUT_ID = {"mixed": 0, "f64": 1, "f32": 2}

ERRORS = {-1: "QR_E_NULL: a required pointer is NULL", -2: "QR_E_KIND: bad env kind",
          -3: "QR_E_SIZE: bad num_envs / substeps / n_steps / max_steps / actor sizes / coefficients", -4: "QR_E_ALIGN: buffer not 16-byte aligned"}

# every symbol include/quadrotor_hip.h declares
SYMBOLS = ("qr_step", "qr_rollout", "qr_rollout_actor", "qr_error_obs", "qr_error_obs_format", "qr_reset", "qr_get_state", "qr_set_state", "qr_check_state",
           "qr_traj_start", "qr_get_desired", "qr_gae",
           "qr_default_coeffs", "qr_abi_version", "qr_step_kernel_info", "qr_launch_thresholds",
           "qr_launch_plan", "qr_launch_stats", "qr_instance_table", "qr_touch", "qr_evaluate_actor", "qr_evaluate_population",
           "qr_critic_values", "qr_critic_next_values", "qr_ppo_actor_grad", "qr_ppo_actor_workspace_bytes",
           "qr_ppo_critic_grad", "qr_ppo_critic_workspace_bytes", "qr_adamw_step", "qr_adamw_polyak_step",
           "qr_twinq_target", "qr_twinq_grad", "qr_twinq_workspace_bytes",
           "qr_dpg_actor_grad", "qr_dpg_actor_workspace_bytes", "qr_soft_update", "qr_sac_target",
           "qr_sac_actor_grad", "qr_sac_actor_workspace_bytes",
           "qr_ctde_twinq_target", "qr_ctde_sac_target", "qr_ctde_twinq_grad", "qr_ctde_twinq_workspace_bytes",
           "qr_ctde_dpg_actor_grad", "qr_ctde_dpg_actor_workspace_bytes",
           "qr_ctde_sac_actor_grad", "qr_ctde_sac_actor_workspace_bytes",
           "qr_replay_add", "qr_replay_add_rule", "qr_replay_sample", "qr_noise_fill",
           "qr_episode_scan", "qr_episode_workspace_bytes", "qr_gae_rule", "qr_gae_rule_workspace_bytes",
           "qr_es_perturb", "qr_es_gradient", "qr_es_workspace_bytes", "qr_shuffle", "qr_ppo_actor_grad_dev")


class QrCoeffs(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "Cx", "CIx", "Cv", "Cb1", "CIb1", "CW", "Cw12", "CW3", "alpha", "beta", "dt",
        "x_lim", "v_lim", "W_lim", "eIx_lim", "eIb1_lim", "euler_lim_deg", "udm_fraction",
        "eight_T", "eight_A1", "eight_A2", "eight_w_b1d", "eight_alt_d", "eight_eps", "eight_count", "w_adapt",
        "m_nominal", "d_nominal", "J1_nominal", "J3_nominal", "c_tf_nominal", "c_tw_nominal", "g", "min_force")]


class QrEnv(C.Structure):
    _fields_ = [("kind", C.c_int32), ("layout", C.c_int32), ("num_envs", C.c_int64), ("field_stride", C.c_int64),
                ("env_offset", C.c_int64), ("seed", C.c_uint64),
                ("pos_vel", C.c_void_p), ("att_rate", C.c_void_p),
                ("integ", C.c_void_p), ("params", C.c_void_p), ("goal", C.c_void_p),
                ("traj", C.c_void_p), ("goal_mode", C.c_int32), ("reserved0", C.c_int32),
                ("episode", C.c_void_p), ("steps", C.c_void_p), ("reset_count", C.c_void_p),
                ("max_episode_steps", C.c_int32), ("flags", C.c_uint32), ("coeffs", QrCoeffs)]


class QrStepOut(C.Structure):
    _fields_ = [("obs0", C.c_void_p), ("obs1", C.c_void_p), ("reward", C.c_void_p),
                ("reward_raw", C.c_void_p), ("done", C.c_void_p), ("truncated", C.c_void_p),
                ("final_obs0", C.c_void_p), ("final_obs1", C.c_void_p)]


class QrActor(C.Structure):
    _fields_ = [("fc1_w", C.c_void_p), ("fc1_b", C.c_void_p), ("fc2_w", C.c_void_p), ("fc2_b", C.c_void_p),
                ("mean_w", C.c_void_p), ("mean_b", C.c_void_p), ("log_std", C.c_void_p),
                ("log_std_w", C.c_void_p), ("log_std_b", C.c_void_p),
                ("obs_dim", C.c_int32), ("hidden_dim", C.c_int32), ("action_dim", C.c_int32), ("squash", C.c_int32)]


ACTOR_TANH_MEAN, ACTOR_TANH_SAMPLE = 0, 1


class QrPolicyRollout(C.Structure):
    _fields_ = [("actors", C.POINTER(QrActor)), ("obs0_in", C.c_void_p), ("obs1_in", C.c_void_p), ("noise", C.c_void_p),
                ("noise_seed", C.c_uint64), ("step_base", C.c_uint64), ("max_action", C.c_float), ("deterministic", C.c_int32),
                ("action_out", C.c_void_p), ("logprob_out", C.c_void_p)]


class QrEvalOut(C.Structure):
    _fields_ = [("episode_return", C.c_void_p), ("benchmark", C.c_void_p), ("length", C.c_void_p), ("terminated", C.c_void_p),
                ("success", C.c_void_p), ("final_error", C.c_void_p), ("obs0", C.c_void_p), ("obs1", C.c_void_p)]


class QrPopulation(C.Structure):
    _fields_ = [("n_policies", C.c_int32), ("envs_per_policy", C.c_int32)]


class QrCritic(C.Structure):
    _fields_ = [("fc1_w", C.c_void_p), ("fc1_b", C.c_void_p), ("fc2_w", C.c_void_p), ("fc2_b", C.c_void_p),
                ("fc3_w", C.c_void_p), ("fc3_b", C.c_void_p),
                ("in0", C.c_int32), ("in1", C.c_int32), ("hidden_dim", C.c_int32), ("reserved0", C.c_int32)]


CRITIC_MAX_IN, CRITIC_MAX_HIDDEN = 24, 64   # qr_critic_values: padded input width, padded hidden width


class QrPpoBatch(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("final_obs", C.c_void_p), ("done", C.c_void_p), ("truncated", C.c_void_p),
                ("action", C.c_void_p), ("logp_old", C.c_void_p), ("advantage", C.c_void_p), ("index", C.c_void_p),
                ("noise", C.c_void_p), ("nominal", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("batch", C.c_int64), ("n_envs", C.c_int64), ("n_steps", C.c_int32), ("n_agents", C.c_int32),
                ("row_stride", C.c_int32), ("col_offset", C.c_int32), ("adv_stride", C.c_int32), ("max_workgroups", C.c_int32),
                ("clip", C.c_float), ("entropy_coef", C.c_float), ("lam_T", C.c_float), ("lam_S", C.c_float), ("lam_M", C.c_float),
                ("max_action", C.c_float)]


PPO_GRAD_NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b", "log_std")   # qr_ppo_actor_grad: the gradient tensors, in order


class QrPpoGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PPO_GRAD_NAMES + ("stats",)]


class QrCriticBatch(C.Structure):
    _fields_ = [("obs0", C.c_void_p), ("obs1", C.c_void_p), ("target", C.c_void_p), ("index", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("batch", C.c_int64), ("rows", C.c_int64), ("target_stride", C.c_int32),
                ("max_workgroups", C.c_int32), ("l2_reg", C.c_float), ("reserved0", C.c_int32)]


PPO_CRITIC_GRAD_NAMES = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")   # qr_ppo_critic_grad: the gradient tensors, in order


class QrCriticGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PPO_CRITIC_GRAD_NAMES + ("stats",)]


def ppo_batch_args(obs, action, logp_old, advantage, workspace, *, final_obs=None, done=None, truncated=None, index=None, noise=None, nominal=None,
                   batch, n_envs, n_steps, n_agents, row_stride, col_offset, adv_stride, max_workgroups, clip, entropy_coef, lam_T, lam_S, lam_M,
                   max_action) -> QrPpoBatch:
    """QrPpoBatch of one qr_ppo_actor_grad launch; final_obs, done, truncated, index, noise, nominal: tensors or None."""
    b = QrPpoBatch()
    b.obs, b.final_obs, b.done, b.truncated = ptr(obs), ptr(final_obs), ptr(done), ptr(truncated)
    b.action, b.logp_old, b.advantage, b.index = ptr(action), ptr(logp_old), ptr(advantage), ptr(index)
    b.noise, b.nominal = ptr(noise), ptr(nominal)
    b.workspace, b.workspace_bytes = ptr(workspace), workspace.numel() * workspace.element_size()
    b.batch, b.n_envs, b.n_steps, b.n_agents = int(batch), int(n_envs), int(n_steps), int(n_agents)
    b.row_stride, b.col_offset, b.adv_stride, b.max_workgroups = int(row_stride), int(col_offset), int(adv_stride), int(max_workgroups)
    b.clip, b.entropy_coef, b.lam_T, b.lam_S, b.lam_M, b.max_action = (float(v) for v in (clip, entropy_coef, lam_T, lam_S, lam_M, max_action))
    return b


def ppo_grad_args(grads, stats) -> QrPpoGrad:
    """QrPpoGrad of one qr_ppo_actor_grad launch: grads = {name: tensor} over PPO_GRAD_NAMES."""
    return QrPpoGrad(*[grads[n].data_ptr() for n in PPO_GRAD_NAMES], stats.data_ptr())


def critic_batch_args(obs0, obs1, target, workspace, *, index=None, batch, rows, target_stride, max_workgroups, l2_reg) -> QrCriticBatch:
    """QrCriticBatch of one qr_ppo_critic_grad launch; obs0 / obs1: the row tensors the critic reads, None for one it does not."""
    b = QrCriticBatch()
    b.obs0, b.obs1, b.target, b.index = ptr(obs0), ptr(obs1), ptr(target), ptr(index)
    b.workspace, b.workspace_bytes = ptr(workspace), workspace.numel() * workspace.element_size()
    b.batch, b.rows, b.target_stride, b.max_workgroups, b.l2_reg = int(batch), int(rows), int(target_stride), int(max_workgroups), float(l2_reg)
    return b


def critic_grad_args(grads, stats) -> QrCriticGrad:
    """QrCriticGrad of one qr_ppo_critic_grad launch: grads = {name: tensor} over PPO_CRITIC_GRAD_NAMES."""
    return QrCriticGrad(*[grads[n].data_ptr() for n in PPO_CRITIC_GRAD_NAMES], stats.data_ptr())


QCRITIC_MAX_IN, QCRITIC_MAX_HIDDEN = 28, 64   # qr_twinq_target / qr_twinq_grad: widest obs_dim + action_dim, widest hidden layer
TWINQ_GRAD_NAMES = tuple(f"fc{k}_{x}" for k in range(1, 7) for x in "wb")   # qr_twinq_grad: the gradient tensors, in order


class QrQCritic(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TWINQ_GRAD_NAMES] + [("obs_dim", C.c_int32), ("action_dim", C.c_int32), ("hidden_dim", C.c_int32),
                                                              ("reserved0", C.c_int32)]


class QrTransitions(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("obs_next", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("index", C.c_void_p), ("batch", C.c_int64), ("rows", C.c_int64), ("row_stride", C.c_int32), ("col_offset", C.c_int32),
                ("reward_stride", C.c_int32), ("done_stride", C.c_int32)]


class QrTd3Target(C.Structure):
    _fields_ = [("eps", C.c_void_p), ("action_next", C.c_void_p), ("y", C.c_void_p), ("discount", C.c_float), ("target_noise", C.c_float),
                ("noise_clip", C.c_float), ("max_action", C.c_float)]


class QrTwinQGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TWINQ_GRAD_NAMES + ("stats", "y", "workspace")] + [("workspace_bytes", C.c_int64),
                                                                                           ("max_workgroups", C.c_int32), ("reserved0", C.c_int32)]


DPG_GRAD_NAMES = PPO_GRAD_NAMES[:6]   # qr_dpg_actor_grad: the gradient tensors, in order
SOFT_UPDATE_MAX = 24                  # qr_soft_update: tensors per launch


class QrDpgGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in DPG_GRAD_NAMES + ("stats", "noise", "nominal", "workspace")] + [
        ("workspace_bytes", C.c_int64), ("lam_T", C.c_float), ("lam_S", C.c_float), ("lam_M", C.c_float), ("max_action", C.c_float),
        ("max_workgroups", C.c_int32), ("reserved0", C.c_int32)]


class QrSoftUpdate(C.Structure):
    _fields_ = [("target", C.c_void_p * 24), ("param", C.c_void_p * 24), ("count", C.c_int64 * 24), ("n_tensors", C.c_int32),
                ("reserved0", C.c_int32), ("tau", C.c_double)]


class QrSacTarget(C.Structure):
    _fields_ = [("eps", C.c_void_p), ("action_next", C.c_void_p), ("logp_next", C.c_void_p), ("alpha_dev", C.c_void_p), ("y", C.c_void_p),
                ("action_out", C.c_void_p), ("logp_out", C.c_void_p), ("discount", C.c_float), ("alpha", C.c_float)]


SAC_ACTOR_GRAD_NAMES = DPG_GRAD_NAMES + ("log_std_w", "log_std_b")   # qr_sac_actor_grad: the gradient tensors, in order
SAC_ACTOR_STATS = 6                                                    # ... and the length of its stats


class QrSacActorGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SAC_ACTOR_GRAD_NAMES + ("stats", "eps", "eps_reg", "eps_next", "eps_pert", "noise", "nominal", "alpha_dev",
                                                                  "alpha_grad", "workspace")] + [
        ("workspace_bytes", C.c_int64), ("alpha", C.c_float), ("target_entropy", C.c_float), ("lam_T", C.c_float), ("lam_S", C.c_float),
        ("lam_M", C.c_float), ("max_action", C.c_float), ("max_workgroups", C.c_int32), ("reserved0", C.c_int32)]


def transitions(*, obs=None, obs_next=None, action=None, reward=None, done=None, index=None, batch, rows, row_stride=1, col_offset=0,
                reward_stride=1, done_stride=1) -> QrTransitions:
    """QrTransitions of one minibatch of a flat transition buffer; a tensor the entry point does not read stays None."""
    b = QrTransitions()
    b.obs, b.obs_next, b.action, b.reward, b.done, b.index = ptr(obs), ptr(obs_next), ptr(action), ptr(reward), ptr(done), ptr(index)
    b.batch, b.rows = int(batch), int(rows)
    b.row_stride, b.col_offset, b.reward_stride, b.done_stride = int(row_stride), int(col_offset), int(reward_stride), int(done_stride)
    return b


def td3_target_args(*, eps, action_next, y, discount, target_noise, noise_clip, max_action) -> QrTd3Target:
    """QrTd3Target of one qr_twinq_target launch."""
    return QrTd3Target(ptr(eps), ptr(action_next), ptr(y), float(discount), float(target_noise), float(noise_clip), float(max_action))


def sac_target_args(*, eps, action_next, logp_next, alpha_dev, y, action_out, logp_out, discount, alpha) -> QrSacTarget:
    """QrSacTarget of one qr_sac_target launch; alpha_dev: the device scalar that wins over `alpha`, or None."""
    return QrSacTarget(ptr(eps), ptr(action_next), ptr(logp_next), ptr(alpha_dev), ptr(y), ptr(action_out), ptr(logp_out), float(discount),
                       float(alpha))


def twinq_grad_args(grads, stats, y, workspace, max_workgroups) -> QrTwinQGrad:
    """QrTwinQGrad of one qr_twinq_grad launch: grads = {name: tensor} over TWINQ_GRAD_NAMES."""
    g = QrTwinQGrad(*[grads[n].data_ptr() for n in TWINQ_GRAD_NAMES], stats.data_ptr(), y.data_ptr(), workspace.data_ptr())
    g.workspace_bytes, g.max_workgroups, g.reserved0 = workspace.numel() * workspace.element_size(), int(max_workgroups), 0
    return g


def dpg_grad_args(grads, stats, noise, nominal, workspace, *, lam_T, lam_S, lam_M, max_action, max_workgroups) -> QrDpgGrad:
    """QrDpgGrad of one qr_dpg_actor_grad launch: grads = {name: tensor} over DPG_GRAD_NAMES."""
    g = QrDpgGrad(*[grads[n].data_ptr() for n in DPG_GRAD_NAMES], stats.data_ptr(), ptr(noise), ptr(nominal), workspace.data_ptr())
    g.workspace_bytes = workspace.numel() * workspace.element_size()
    g.lam_T, g.lam_S, g.lam_M, g.max_action = float(lam_T), float(lam_S), float(lam_M), float(max_action)
    g.max_workgroups, g.reserved0 = int(max_workgroups), 0
    return g


def sac_actor_grad_args(grads, stats, workspace, *, eps, eps_reg, eps_next, eps_pert, noise, nominal, alpha_dev, alpha_grad, alpha, target_entropy,
                        lam_T, lam_S, lam_M, max_action, max_workgroups) -> QrSacActorGrad:
    """QrSacActorGrad of one qr_sac_actor_grad launch: grads = {name: tensor} over SAC_ACTOR_GRAD_NAMES; alpha_dev: the device scalar that
    wins over `alpha`, or None."""
    g = QrSacActorGrad(*[grads[n].data_ptr() for n in SAC_ACTOR_GRAD_NAMES], stats.data_ptr(), ptr(eps), ptr(eps_reg), ptr(eps_next), ptr(eps_pert),
                       ptr(noise), ptr(nominal), ptr(alpha_dev), ptr(alpha_grad), workspace.data_ptr())
    g.workspace_bytes = workspace.numel() * workspace.element_size()
    g.alpha, g.target_entropy = float(alpha), float(target_entropy)
    g.lam_T, g.lam_S, g.lam_M, g.max_action = float(lam_T), float(lam_S), float(lam_M), float(max_action)
    g.max_workgroups, g.reserved0 = int(max_workgroups), 0
    return g


class QrCtdeTransitions(C.Structure):
    _fields_ = [("obs", C.c_void_p * 2), ("obs_next", C.c_void_p * 2), ("action", C.c_void_p * 2), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("index", C.c_void_p), ("batch", C.c_int64), ("rows", C.c_int64), ("obs_dim", C.c_int32 * 2), ("action_dim", C.c_int32 * 2),
                ("row_stride", C.c_int32 * 2), ("col_offset", C.c_int32 * 2), ("reward_stride", C.c_int32), ("done_stride", C.c_int32)]


class QrCtdeTd3Target(C.Structure):
    _fields_ = [("eps", C.c_void_p * 2), ("action_next", C.c_void_p * 2), ("y", C.c_void_p), ("discount", C.c_float), ("target_noise", C.c_float),
                ("noise_clip", C.c_float), ("max_action", C.c_float)]


class QrCtdeSacTarget(C.Structure):
    _fields_ = [("eps", C.c_void_p * 2), ("eps_logp", C.c_void_p), ("action_next", C.c_void_p * 2), ("logp_next", C.c_void_p),
                ("alpha_dev", C.c_void_p), ("y", C.c_void_p), ("action_out", C.c_void_p * 2), ("logp_out", C.c_void_p), ("discount", C.c_float),
                ("alpha", C.c_float), ("agent", C.c_int32), ("reserved0", C.c_int32)]


class QrCtdeDpgGrad(C.Structure):
    _fields_ = QrDpgGrad._fields_ + [("agent", C.c_int32), ("reserved1", C.c_int32), ("action_other", C.c_void_p)]


class QrCtdeSacActorGrad(C.Structure):
    _fields_ = QrSacActorGrad._fields_ + [("agent", C.c_int32), ("reserved1", C.c_int32), ("eps_logp", C.c_void_p), ("eps_other", C.c_void_p),
                                          ("action_other", C.c_void_p)]


def _pair(x):
    x = (None, None) if x is None else x
    return (C.c_void_p * 2)(ptr(x[0]), ptr(x[1]))


def ctde_transitions(*, obs=None, obs_next=None, action=None, reward=None, done=None, index=None, batch, rows, obs_dims, action_dims,
                     row_strides=(1, 1), col_offsets=(0, 0), reward_stride=1, done_stride=1) -> QrCtdeTransitions:
    """QrCtdeTransitions of one minibatch of a two-agent buffer: obs, obs_next, action are pairs of tensors (or None where the entry point
    does not read them); reward, done: the columns of the agent whose target this is."""
    b = QrCtdeTransitions()
    b.obs, b.obs_next, b.action = _pair(obs), _pair(obs_next), _pair(action)
    b.reward, b.done, b.index = ptr(reward), ptr(done), ptr(index)
    b.batch, b.rows = int(batch), int(rows)
    for m in range(2):
        b.obs_dim[m], b.action_dim[m], b.row_stride[m], b.col_offset[m] = int(obs_dims[m]), int(action_dims[m]), int(row_strides[m]), int(col_offsets[m])
    b.reward_stride, b.done_stride = int(reward_stride), int(done_stride)
    return b


def ctde_td3_target_args(*, eps, action_next, y, discount, target_noise, noise_clip, max_action) -> QrCtdeTd3Target:
    """QrCtdeTd3Target of one qr_ctde_twinq_target launch; eps, action_next: pairs (or None)."""
    return QrCtdeTd3Target(_pair(eps), _pair(action_next), ptr(y), float(discount), float(target_noise), float(noise_clip), float(max_action))


def ctde_sac_target_args(*, eps, eps_logp, action_next, logp_next, alpha_dev, y, action_out, logp_out, discount, alpha, agent) -> QrCtdeSacTarget:
    """QrCtdeSacTarget of one qr_ctde_sac_target launch; eps, action_next, action_out: pairs (or None)."""
    return QrCtdeSacTarget(_pair(eps), ptr(eps_logp), _pair(action_next), ptr(logp_next), ptr(alpha_dev), ptr(y), _pair(action_out), ptr(logp_out),
                           float(discount), float(alpha), int(agent), 0)


def ctde_dpg_grad_args(grads, stats, noise, nominal, workspace, *, agent, action_other, lam_T, lam_S, lam_M, max_action, max_workgroups) -> QrCtdeDpgGrad:
    """QrCtdeDpgGrad of one qr_ctde_dpg_actor_grad launch: dpg_grad_args' fields, the agent k and the other agent's action (or None)."""
    d = dpg_grad_args(grads, stats, noise, nominal, workspace, lam_T=lam_T, lam_S=lam_S, lam_M=lam_M, max_action=max_action, max_workgroups=max_workgroups)
    g = QrCtdeDpgGrad(*[getattr(d, n) for n, _ in QrDpgGrad._fields_])
    g.agent, g.reserved1, g.action_other = int(agent), 0, ptr(action_other)
    return g


def ctde_sac_actor_grad_args(grads, stats, workspace, *, agent, action_other, eps_logp, eps_other, **kw) -> QrCtdeSacActorGrad:
    """QrCtdeSacActorGrad of one qr_ctde_sac_actor_grad launch: sac_actor_grad_args' fields (kw; eps = agent k's first draw), the agent k,
    its second draw, the other agent's draw and the other agent's action (each or None)."""
    d = sac_actor_grad_args(grads, stats, workspace, **kw)
    g = QrCtdeSacActorGrad(*[getattr(d, n) for n, _ in QrSacActorGrad._fields_])
    g.agent, g.reserved1, g.eps_logp, g.eps_other, g.action_other = int(agent), 0, ptr(eps_logp), ptr(eps_other), ptr(action_other)
    return g


REPLAY_MAX_WIDTH = 4096   # qr_replay_add: widest observation or action row
REPLAY_BUFFER_NAMES = ("obs", "obs_next", "act", "rwd", "done")   # an agent's five buffer tensors (ReplayBuffer.tensors), in QrReplayAdd's order


class QrReplayAdd(C.Structure):
    _fields_ = [("obs", C.c_void_p * 2), ("final_obs", C.c_void_p * 2), ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("truncated", C.c_void_p), ("buf_obs", C.c_void_p * 2), ("buf_obs_next", C.c_void_p * 2), ("buf_action", C.c_void_p * 2),
                ("buf_reward", C.c_void_p * 2), ("buf_done", C.c_void_p * 2), ("state", C.c_void_p), ("count", C.c_int64), ("capacity", C.c_int64),
                ("n_envs", C.c_int64), ("n_steps", C.c_int32), ("n_agents", C.c_int32), ("obs_dim", C.c_int32 * 2), ("action_dim", C.c_int32 * 2),
                ("col_offset", C.c_int32 * 2), ("action_row", C.c_int32), ("reserved0", C.c_int32)]


class QrReplayAddRule(C.Structure):
    _fields_ = [("add", QrReplayAdd), ("x_lim", C.c_double), ("pos_tol", C.c_double), ("rot_tol", C.c_double)]


class QrReplaySample(C.Structure):
    _fields_ = [("index", C.c_void_p), ("status", C.c_void_p), ("state", C.c_void_p), ("n", C.c_int64), ("batch", C.c_int64),
                ("seed", C.c_uint64), ("draw", C.c_uint64)]


def replay_add_args(buffers, obs, final_obs, action, reward, done, truncated, *, state, count, capacity, n_steps, n_envs, obs_dims, action_dims,
                    col_offsets, action_row) -> QrReplayAdd:
    """QrReplayAdd of one qr_replay_add launch: buffers = one {name: tensor} over REPLAY_BUFFER_NAMES per agent (one or two); obs a list
    per agent, final_obs one or None; state: the device counters or None."""
    r = QrReplayAdd()
    for k, b in enumerate(buffers):
        r.obs[k], r.final_obs[k] = ptr(obs[k]), (None if final_obs is None else ptr(final_obs[k]))
        r.buf_obs[k], r.buf_obs_next[k], r.buf_action[k], r.buf_reward[k], r.buf_done[k] = (ptr(b[n]) for n in REPLAY_BUFFER_NAMES)
        r.obs_dim[k], r.action_dim[k], r.col_offset[k] = int(obs_dims[k]), int(action_dims[k]), int(col_offsets[k])
    r.action, r.reward, r.done, r.truncated, r.state = ptr(action), ptr(reward), ptr(done), ptr(truncated), ptr(state)
    r.count, r.capacity, r.n_envs, r.n_steps, r.n_agents = int(count), int(capacity), int(n_envs), int(n_steps), len(buffers)
    r.action_row, r.reserved0 = int(action_row), 0
    return r


def replay_add_rule_args(add: QrReplayAdd, *, x_lim, pos_tol, rot_tol) -> QrReplayAddRule:
    """QrReplayAddRule of one qr_replay_add_rule launch: replay_add_args' struct and the time-limit rule's three numbers."""
    return QrReplayAddRule(add, float(x_lim), float(pos_tol), float(rot_tol))


def replay_sample_args(index, status, state, *, n, batch, seed, draw) -> QrReplaySample:
    """QrReplaySample of one qr_replay_sample launch; status, state: device tensors or None."""
    return QrReplaySample(ptr(index), ptr(status), ptr(state), int(n), int(batch), int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1))


NOISE_MAX_SLOTS = 16                     # qr_noise_fill: tensors per launch
NOISE_NORMAL, NOISE_UNIFORM = 0, 1
NOISE_KIND_ID = {"normal": NOISE_NORMAL, "uniform": NOISE_UNIFORM}
NOISE_MAX_STREAM = 2 ** 30               # stream ids lie below it


class QrNoiseSlot(C.Structure):
    _fields_ = [("out", C.c_void_p), ("count", C.c_int64), ("a", C.c_float), ("b", C.c_float), ("kind", C.c_uint32), ("stream", C.c_uint32)]


class QrNoiseFill(C.Structure):
    _fields_ = [("slot", QrNoiseSlot * 16), ("n_slots", C.c_int32), ("seed", C.c_uint64), ("draw_dev", C.c_void_p), ("draw", C.c_int64)]


def noise_fill_args(tensors, kinds, a, b, streams, *, seed, draw, draw_dev) -> QrNoiseFill:
    """QrNoiseFill of one qr_noise_fill launch over 1..16 tensors; kinds, a, b, streams: one per tensor; draw_dev: a device int64
    tensor of one element or None."""
    f = QrNoiseFill()
    f.n_slots, f.seed, f.draw_dev, f.draw = len(tensors), int(seed) & (2 ** 64 - 1), ptr(draw_dev), int(draw)
    for k, t in enumerate(tensors):
        s = f.slot[k]
        s.out, s.count, s.a, s.b, s.kind, s.stream = t.data_ptr(), t.numel(), float(a[k]), float(b[k]), int(kinds[k]), int(streams[k])
    return f


SHUFFLE_ROUNDS, SHUFFLE_MIX_M1, SHUFFLE_MIX_M2 = 8, 0x7FEB352D, 0x846CA68B   # qr_shuffle: Feistel rounds, the finaliser's multipliers
SHUFFLE_MAX_N = 2 ** 32                  # n lies below it


class QrShuffle(C.Structure):
    _fields_ = [("out", C.c_void_p), ("draw_dev", C.c_void_p), ("n", C.c_int64), ("first", C.c_int64), ("count", C.c_int64),
                ("seed", C.c_uint64), ("draw", C.c_int64), ("stream", C.c_uint32), ("max_workgroups", C.c_int32)]


def shuffle_args(out, *, n, first, seed, draw, draw_dev, stream, max_workgroups=0) -> QrShuffle:
    """QrShuffle of one qr_shuffle launch: out an int64 tensor (its numel is the count); draw_dev: a device int64 tensor of one
    element or None."""
    return QrShuffle(ptr(out) if out.numel() else None, ptr(draw_dev), int(n), int(first), out.numel(), int(seed) & (2 ** 64 - 1), int(draw),
                     int(stream), int(max_workgroups))


# qr_episode_scan: the QR_EP_* indices of `last` / `total` (agent g's field at index + g), the flag bits of ep_flags
EP_COUNT, EP_RETURN_SUM, EP_RETURN_SQ, EP_RETURN_MIN, EP_RETURN_MAX, EP_LENGTH_SUM, EP_LENGTH_MAX = 0, 1, 3, 5, 7, 9, 10
EP_DONE, EP_TRUNCATED, EP_SOLVED, EP_EX_SUM, EP_EB1_SUM, EP_FIELDS, EP_STEPS_SEEN, EP_TOTAL_FIELDS = 11, 13, 14, 16, 17, 18, 18, 19
EP_FLAG_DONE0, EP_FLAG_SOLVED0, EP_FLAG_TRUNCATED = 0x01, 0x10, 0x80
EP_INDEX = {"COUNT": EP_COUNT, "RETURN_SUM": EP_RETURN_SUM, "RETURN_SQ": EP_RETURN_SQ, "RETURN_MIN": EP_RETURN_MIN, "RETURN_MAX": EP_RETURN_MAX,
            "LENGTH_SUM": EP_LENGTH_SUM, "LENGTH_MAX": EP_LENGTH_MAX, "DONE": EP_DONE, "TRUNCATED": EP_TRUNCATED, "SOLVED": EP_SOLVED,
            "EX_SUM": EP_EX_SUM, "EB1_SUM": EP_EB1_SUM, "FIELDS": EP_FIELDS, "STEPS_SEEN": EP_STEPS_SEEN, "TOTAL_FIELDS": EP_TOTAL_FIELDS}
EP_MIN_FIELDS, EP_MAX_FIELDS = (5, 6), (7, 8, 10)   # the fields that fold as a minimum / a maximum; the others add


def episode_empty() -> list:
    """The QR_EP_TOTAL_FIELDS values of a `total` over no episodes (its first QR_EP_FIELDS: of a `last`)."""
    inf = float("inf")
    return [inf if k in EP_MIN_FIELDS else -inf if k in (7, 8) else 0.0 for k in range(EP_TOTAL_FIELDS)]


class QrEpisodeScan(C.Structure):
    _fields_ = [("reward", C.c_void_p), ("done", C.c_void_p), ("truncated", C.c_void_p), ("final_obs0", C.c_void_p), ("final_obs1", C.c_void_p),
                ("run_return", C.c_void_p), ("run_length", C.c_void_p), ("ep_return", C.c_void_p), ("ep_length", C.c_void_p),
                ("ep_flags", C.c_void_p), ("ep_final_error", C.c_void_p), ("last", C.c_void_p), ("total", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("n_envs", C.c_int64), ("n_steps", C.c_int32), ("n_agents", C.c_int32),
                ("d0", C.c_int32), ("d1", C.c_int32), ("record", C.c_int32), ("reserved0", C.c_int32),
                ("x_lim", C.c_double), ("pos_tol", C.c_double), ("rot_tol", C.c_double)]


def episode_scan_args(reward, done, truncated, final_obs, run_return, run_length, dense, last, total, workspace, *, n_steps, n_envs, n_agents,
                      x_lim, pos_tol, rot_tol, record) -> QrEpisodeScan:
    """QrEpisodeScan of one qr_episode_scan call; final_obs: None or one tensor per agent; dense: the four optional outputs (ep_return,
    ep_length, ep_flags, ep_final_error), tensors or None."""
    e = QrEpisodeScan()
    e.reward, e.done, e.truncated = ptr(reward), ptr(done), ptr(truncated)
    if final_obs is not None:
        e.final_obs0, e.d0 = ptr(final_obs[0]), final_obs[0].shape[-1]
        if n_agents == 2:
            e.final_obs1, e.d1 = ptr(final_obs[1]), final_obs[1].shape[-1]
    else:
        e.d0, e.d1 = 3, 1
    e.run_return, e.run_length, e.last, e.total = ptr(run_return), ptr(run_length), ptr(last), ptr(total)
    e.ep_return, e.ep_length, e.ep_flags, e.ep_final_error = (ptr(t) for t in dense)
    e.workspace, e.workspace_bytes = ptr(workspace), workspace.numel() * workspace.element_size()
    e.n_envs, e.n_steps, e.n_agents, e.record, e.reserved0 = int(n_envs), int(n_steps), int(n_agents), int(bool(record)), 0
    e.x_lim, e.pos_tol, e.rot_tol = float(x_lim), float(pos_tol), float(rot_tol)
    return e


class QrGaeRule(C.Structure):
    _fields_ = [("reward", C.c_void_p), ("done", C.c_void_p), ("truncated", C.c_void_p), ("term_obs0", C.c_void_p), ("term_obs1", C.c_void_p),
                ("value", C.c_void_p), ("next_value", C.c_void_p), ("advantage", C.c_void_p), ("td_target", C.c_void_p), ("done_eff", C.c_void_p),
                ("stats", C.c_void_p), ("normalized", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("n_envs", C.c_int64), ("n_steps", C.c_int32), ("n_agents", C.c_int32), ("d0", C.c_int32), ("d1", C.c_int32),
                ("rule", C.c_int32), ("reserved0", C.c_int32), ("gamma", C.c_float), ("lam", C.c_float),
                ("x_lim", C.c_double), ("pos_tol", C.c_double), ("rot_tol", C.c_double), ("norm_eps", C.c_double)]


GAE_NORM_EPS = 1e-4   # ppo.py:146


def gae_rule_args(reward, done, truncated, term_obs, value, next_value, advantage, td_target, done_eff, stats, normalized, workspace, *,
                  n_steps, n_envs, n_agents, gamma, lam, rule, norm_eps=GAE_NORM_EPS) -> QrGaeRule:
    """QrGaeRule of one qr_gae_rule call; term_obs: None or one tensor per agent (the transitions' obs_next rows); rule: None (each
    agent's own done flag) or the time-limit rule's three numbers (x_lim, pos_tol, rot_tol); next_value, done_eff, stats, normalized,
    workspace: tensors or None."""
    e = QrGaeRule()
    e.reward, e.done, e.truncated, e.value, e.next_value = ptr(reward), ptr(done), ptr(truncated), ptr(value), ptr(next_value)
    if term_obs is not None:
        e.term_obs0, e.d0 = ptr(term_obs[0]), term_obs[0].shape[-1]
        if n_agents == 2:
            e.term_obs1, e.d1 = ptr(term_obs[1]), term_obs[1].shape[-1]
    e.advantage, e.td_target, e.done_eff, e.stats, e.normalized = ptr(advantage), ptr(td_target), ptr(done_eff), ptr(stats), ptr(normalized)
    e.workspace, e.workspace_bytes = ptr(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size()
    e.n_envs, e.n_steps, e.n_agents, e.reserved0 = int(n_envs), int(n_steps), int(n_agents), 0
    e.gamma, e.lam, e.norm_eps = float(gamma), float(lam), float(norm_eps)
    e.rule = 0 if rule is None else 1
    if rule is not None:
        e.x_lim, e.pos_tol, e.rot_tol = (float(v) for v in rule)
    return e


ES_MAX_TENSORS, ES_MAX_COPIES, ES_MAX_POLICIES, ES_STATS = 16, 8, 8192, 4   # qr_es_perturb / qr_es_gradient
ES_CENTERED_RANK, ES_STANDARDIZE = 0, 1
ES_SHAPING_ID = {"centered_rank": ES_CENTERED_RANK, "standardize": ES_STANDARDIZE}


class QrEsTensor(C.Structure):
    _fields_ = [("base", C.c_void_p), ("out", C.c_void_p), ("count", C.c_int64), ("stream", C.c_uint32), ("reserved0", C.c_uint32)]


class QrEsCopy(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("count", C.c_int64)]


class QrEsPerturb(C.Structure):
    _fields_ = [("tensor", QrEsTensor * ES_MAX_TENSORS), ("copy", QrEsCopy * ES_MAX_COPIES), ("n_tensors", C.c_int32), ("n_copies", C.c_int32),
                ("n_policies", C.c_int32), ("max_workgroups", C.c_int32), ("sigma", C.c_float), ("reserved0", C.c_float), ("seed", C.c_uint64),
                ("generation_dev", C.c_void_p), ("generation", C.c_int64)]


class QrEsGradient(C.Structure):
    _fields_ = [("tensor", QrEsTensor * ES_MAX_TENSORS), ("fitness", C.c_void_p), ("stats", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("n_tensors", C.c_int32), ("n_policies", C.c_int32), ("shaping", C.c_int32),
                ("max_workgroups", C.c_int32), ("sigma", C.c_float), ("reserved0", C.c_float), ("seed", C.c_uint64),
                ("generation_dev", C.c_void_p), ("generation", C.c_int64)]


def _es_key(s, *, n_policies, sigma, seed, generation, generation_dev, max_workgroups):
    s.n_policies, s.max_workgroups, s.sigma, s.reserved0 = int(n_policies), int(max_workgroups), float(sigma), 0.0
    s.seed, s.generation_dev, s.generation = int(seed) & (2 ** 64 - 1), ptr(generation_dev), int(generation)


def es_perturb_args(base, out, copies, streams, **key) -> QrEsPerturb:
    """QrEsPerturb of one qr_es_perturb launch: base / out 1..16 tensors each (out the stacked [P, ...] ones), copies up to 8 (src, dst)
    pairs, streams one id per tensor; key: n_policies, sigma, seed, generation, generation_dev (a device int64 tensor or None),
    max_workgroups."""
    p = QrEsPerturb()
    p.n_tensors, p.n_copies = len(base), len(copies)
    for k, (b, o) in enumerate(zip(base, out)):
        t = p.tensor[k]
        t.base, t.out, t.count, t.stream, t.reserved0 = b.data_ptr(), o.data_ptr(), b.numel(), int(streams[k]), 0
    for k, (src, dst) in enumerate(copies):
        c = p.copy[k]
        c.src, c.dst, c.count = src.data_ptr(), dst.data_ptr(), src.numel()
    _es_key(p, **key)
    return p


def es_gradient_args(fitness, grads, stats, workspace, streams, *, shaping, **key) -> QrEsGradient:
    """QrEsGradient of one qr_es_gradient call: grads 1..16 tensors, streams one id per tensor, shaping an ES_* id; key as above."""
    g = QrEsGradient()
    g.n_tensors, g.shaping = len(grads), int(shaping)
    for k, t_ in enumerate(grads):
        t = g.tensor[k]
        t.base, t.out, t.count, t.stream, t.reserved0 = None, t_.data_ptr(), t_.numel(), int(streams[k]), 0
    g.fitness, g.stats, g.workspace = ptr(fitness), ptr(stats), ptr(workspace)
    g.workspace_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    _es_key(g, **key)
    return g


def soft_update_args(params, targets, tau) -> QrSoftUpdate:
    """QrSoftUpdate of one qr_soft_update launch: 1..24 (param, target) tensor pairs."""
    u = QrSoftUpdate()
    u.n_tensors, u.reserved0, u.tau = len(params), 0, float(tau)
    for k, (p, t) in enumerate(zip(params, targets)):
        u.param[k], u.target[k], u.count[k] = p.data_ptr(), t.data_ptr(), t.numel()
    return u


ADAMW_MAX_GROUPS, ADAMW_MAX_TENSORS, ADAMW_MAX_ENTRIES = 8, 8, 65536   # qr_adamw_step: groups per launch, tensors and entries per group


class QrAdamWGroup(C.Structure):
    _fields_ = [("param", C.c_void_p * 8), ("grad", C.c_void_p * 8), ("count", C.c_int32 * 8), ("n_tensors", C.c_int32),
                ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("step", C.c_void_p), ("stats", C.c_void_p),
                ("lr", C.c_double), ("eta_min", C.c_double), ("t0", C.c_int64),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float), ("max_norm", C.c_float)]


def ptr(t):
    return None if t is None else t.data_ptr()


def adamw_group(g: Optional[QrAdamWGroup], params, grads, exp_avg, exp_avg_sq, step, stats, *, lr, eta_min, t0, betas, eps, weight_decay, max_norm):
    """Fill the QrAdamWGroup `g` of one optimiser step: the parameter tensors and their gradients (1..8 of each, in the order of the
    flat moment buffers), the state tensors, the hyperparameters.  g None: a fresh struct.  Returns g."""
    g = QrAdamWGroup() if g is None else g
    g.n_tensors = len(params)
    for k, (p, d) in enumerate(zip(params, grads)):
        g.param[k], g.grad[k], g.count[k] = p.data_ptr(), d.data_ptr(), p.numel()
    for k in range(len(params), 8):
        g.param[k], g.grad[k], g.count[k] = None, None, 0
    g.exp_avg, g.exp_avg_sq, g.step, g.stats = exp_avg.data_ptr(), exp_avg_sq.data_ptr(), step.data_ptr(), ptr(stats)
    g.lr, g.eta_min, g.t0 = float(lr), float(eta_min), int(t0)
    g.beta1, g.beta2, g.eps, g.weight_decay, g.max_norm = float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(max_norm)
    return g


POLYAK_MAX_GROUPS, POLYAK_MAX_TENSORS = 7, 16   # qr_adamw_polyak_step: groups per launch, tensors per group (entries: ADAMW_MAX_ENTRIES)


class QrAdamWPolyakGroup(C.Structure):
    _fields_ = [("param", C.c_void_p * 16), ("grad", C.c_void_p * 16), ("target", C.c_void_p * 16), ("count", C.c_int32 * 16),
                ("n_tensors", C.c_int32), ("reserved0", C.c_int32),
                ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("step", C.c_void_p), ("stats", C.c_void_p), ("exp_out", C.c_void_p),
                ("lr", C.c_double), ("eta_min", C.c_double), ("t0", C.c_int64),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float), ("max_norm", C.c_float),
                ("tau", C.c_double)]


def adamw_polyak_group(g: Optional[QrAdamWPolyakGroup], params, grads, targets, exp_avg, exp_avg_sq, step, stats, exp_out, *, tau, lr, eta_min, t0, betas,
                       eps, weight_decay, max_norm):
    """Fill the QrAdamWPolyakGroup `g` of one step: as adamw_group with 1..16 tensors, plus per parameter its target tensor or None
    (targets = None: none at all), the exp output (or None) and tau.  g None: a fresh struct.  Returns g."""
    g = QrAdamWPolyakGroup() if g is None else g
    g.n_tensors, g.reserved0 = len(params), 0
    for k, (p, d) in enumerate(zip(params, grads)):
        g.param[k], g.grad[k], g.count[k] = p.data_ptr(), d.data_ptr(), p.numel()
        g.target[k] = None if targets is None else ptr(targets[k])
    for k in range(len(params), 16):
        g.param[k], g.grad[k], g.target[k], g.count[k] = None, None, None, 0
    g.exp_avg, g.exp_avg_sq, g.step, g.stats, g.exp_out = exp_avg.data_ptr(), exp_avg_sq.data_ptr(), step.data_ptr(), ptr(stats), ptr(exp_out)
    g.lr, g.eta_min, g.t0, g.tau = float(lr), float(eta_min), int(t0), float(tau)
    g.beta1, g.beta2, g.eps, g.weight_decay, g.max_norm = float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(max_norm)
    return g


def step_out(out, truncated: bool) -> QrStepOut:
    """QrStepOut over a mapping of output tensors keyed by the member names, `terminated` for the member `done`; a missing or
    None entry is a null pointer.  truncated=False: the env has no step counter, the `truncated` member stays null."""
    o = QrStepOut(*(ptr(out.get("terminated" if name == "done" else name)) for name, _ in QrStepOut._fields_))
    if not truncated:
        o.truncated = None
    return o


def eval_out(out) -> QrEvalOut:
    """QrEvalOut over a mapping keyed by the member names (the keys of QuadVecEnv.evaluate's dict); missing or None: null."""
    return QrEvalOut(*(ptr(out.get(name)) for name, _ in QrEvalOut._fields_))


def policy_rollout(actors_c, obs, *, action_out, logprob_out=None, noise=None, noise_seed=0, step_base=0, max_action=1.0, deterministic=False):
    """QrPolicyRollout of one policy launch.  actors_c: the QrActor array (policy.c_actor_array / ActorPopulation.c_array) — the
    struct only points at it, so the caller keeps `actors_c` alive until the library call has returned.  obs: the one or two
    observation tensors the first action is computed from (the second may be None)."""
    p = QrPolicyRollout()
    p.actors = actors_c
    p.obs0_in, p.obs1_in, p.noise = ptr(obs[0]), (ptr(obs[1]) if len(obs) > 1 else None), ptr(noise)
    p.noise_seed, p.step_base = int(noise_seed) & (2 ** 64 - 1), int(step_base)
    p.max_action, p.deterministic = float(max_action), int(bool(deterministic))
    p.action_out, p.logprob_out = ptr(action_out), ptr(logprob_out)
    return p


class QrLaunchPlan(C.Structure):
    _fields_ = [("grid", C.c_int32), ("block", C.c_int32), ("launches", C.c_int32),
                ("traj", C.c_int32), ("adapt", C.c_int32), ("policy", C.c_int32), ("single", C.c_int32), ("help", C.c_int32), ("hrew", C.c_int32),
                ("mag", C.c_int32), ("key", C.c_uint32), ("name", C.c_char * 96)]


class QuadrotorLibError(RuntimeError):
    pass


_lib = None


def load():
    """Load libquadrotor_hip.so (once) and type its entry points.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QuadrotorLibError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C gym_rotor_amd/csrc`.  gym_rotor_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for s in SYMBOLS:
        if not hasattr(lib, s):
            raise QuadrotorLibError(f"{LIB_PATH} does not export {s}")
    P = C.POINTER
    lib.qr_abi_version.restype = C.c_int
    lib.qr_abi_version.argtypes = []
    lib.qr_default_coeffs.restype = None
    lib.qr_default_coeffs.argtypes = [P(QrCoeffs)]
    lib.qr_step.restype = C.c_int
    lib.qr_step.argtypes = [P(QrEnv), C.c_void_p, C.c_int32, P(QrStepOut), C.c_void_p]
    lib.qr_rollout.restype = C.c_int
    lib.qr_rollout.argtypes = [P(QrEnv), C.c_void_p, C.c_int32, C.c_int32, P(QrStepOut), C.c_void_p]
    lib.qr_rollout_actor.restype = C.c_int
    lib.qr_rollout_actor.argtypes = [P(QrEnv), P(QrPolicyRollout), C.c_int32, C.c_int32, P(QrStepOut), C.c_void_p]
    lib.qr_evaluate_actor.restype = C.c_int
    lib.qr_evaluate_actor.argtypes = [P(QrEnv), P(QrPolicyRollout), C.c_int32, C.c_int32, P(QrEvalOut), C.c_void_p]
    lib.qr_evaluate_population.restype = C.c_int
    lib.qr_evaluate_population.argtypes = [P(QrEnv), P(QrPolicyRollout), P(QrPopulation), C.c_int32, C.c_int32, P(QrEvalOut), C.c_void_p]
    lib.qr_error_obs.restype = C.c_int
    lib.qr_error_obs.argtypes = [P(QrEnv), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.qr_error_obs_format.restype = C.c_int
    lib.qr_error_obs_format.argtypes = [P(QrEnv), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.qr_reset.restype = C.c_int
    lib.qr_reset.argtypes = [P(QrEnv), C.c_void_p, C.c_void_p]
    lib.qr_get_state.restype = C.c_int
    lib.qr_get_state.argtypes = [P(QrEnv), C.c_void_p, C.c_void_p]
    lib.qr_set_state.restype = C.c_int
    lib.qr_set_state.argtypes = [P(QrEnv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.qr_check_state.restype = C.c_int
    lib.qr_check_state.argtypes = [P(QrEnv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.qr_traj_start.restype = C.c_int
    lib.qr_traj_start.argtypes = [P(QrEnv), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.qr_get_desired.restype = C.c_int
    lib.qr_get_desired.argtypes = [P(QrEnv), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.qr_gae.restype = C.c_int
    lib.qr_gae.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_float,
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.qr_critic_values.restype = C.c_int
    lib.qr_critic_values.argtypes = [P(QrCritic), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    lib.qr_critic_next_values.restype = C.c_int
    lib.qr_critic_next_values.argtypes = [P(QrCritic), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.qr_ppo_actor_grad.restype = C.c_int
    lib.qr_ppo_actor_grad.argtypes = [P(QrActor), P(QrPpoBatch), P(QrPpoGrad), C.c_void_p]
    lib.qr_ppo_actor_grad_dev.restype = C.c_int
    lib.qr_ppo_actor_grad_dev.argtypes = [P(QrActor), P(QrPpoBatch), P(QrPpoGrad), C.c_void_p, C.c_void_p]
    lib.qr_ppo_actor_workspace_bytes.restype = C.c_int64
    lib.qr_ppo_actor_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    lib.qr_ppo_critic_grad.restype = C.c_int
    lib.qr_ppo_critic_grad.argtypes = [P(QrCritic), P(QrCriticBatch), P(QrCriticGrad), C.c_void_p]
    lib.qr_ppo_critic_workspace_bytes.restype = C.c_int64
    lib.qr_ppo_critic_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    lib.qr_adamw_step.restype = C.c_int
    lib.qr_adamw_step.argtypes = [P(QrAdamWGroup), C.c_int32, C.c_void_p]
    lib.qr_adamw_polyak_step.restype = C.c_int
    lib.qr_adamw_polyak_step.argtypes = [P(QrAdamWPolyakGroup), C.c_int32, C.c_void_p]
    lib.qr_twinq_target.restype = C.c_int
    lib.qr_twinq_target.argtypes = [P(QrActor), P(QrQCritic), P(QrTransitions), P(QrTd3Target), C.c_void_p]
    lib.qr_twinq_grad.restype = C.c_int
    lib.qr_twinq_grad.argtypes = [P(QrQCritic), P(QrTransitions), P(QrTwinQGrad), C.c_void_p]
    lib.qr_twinq_workspace_bytes.restype = C.c_int64
    lib.qr_twinq_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    lib.qr_dpg_actor_grad.restype = C.c_int
    lib.qr_dpg_actor_grad.argtypes = [P(QrActor), P(QrQCritic), P(QrTransitions), P(QrDpgGrad), C.c_void_p]
    lib.qr_dpg_actor_workspace_bytes.restype = C.c_int64
    lib.qr_dpg_actor_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    lib.qr_soft_update.restype = C.c_int
    lib.qr_soft_update.argtypes = [P(QrSoftUpdate), C.c_void_p]
    lib.qr_sac_target.restype = C.c_int
    lib.qr_sac_target.argtypes = [P(QrActor), P(QrQCritic), P(QrTransitions), P(QrSacTarget), C.c_void_p]
    lib.qr_sac_actor_grad.restype = C.c_int
    lib.qr_sac_actor_grad.argtypes = [P(QrActor), P(QrQCritic), P(QrTransitions), P(QrSacActorGrad), C.c_void_p]
    lib.qr_sac_actor_workspace_bytes.restype = C.c_int64
    lib.qr_sac_actor_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    lib.qr_ctde_twinq_target.restype = C.c_int
    lib.qr_ctde_twinq_target.argtypes = [P(QrActor), P(QrActor), P(QrQCritic), P(QrCtdeTransitions), P(QrCtdeTd3Target), C.c_void_p]
    lib.qr_ctde_sac_target.restype = C.c_int
    lib.qr_ctde_sac_target.argtypes = [P(QrActor), P(QrActor), P(QrQCritic), P(QrCtdeTransitions), P(QrCtdeSacTarget), C.c_void_p]
    lib.qr_ctde_twinq_grad.restype = C.c_int
    lib.qr_ctde_twinq_grad.argtypes = [P(QrQCritic), P(QrCtdeTransitions), P(QrTwinQGrad), C.c_void_p]
    lib.qr_ctde_twinq_workspace_bytes.restype = C.c_int64
    lib.qr_ctde_twinq_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    lib.qr_ctde_dpg_actor_grad.restype = C.c_int
    lib.qr_ctde_dpg_actor_grad.argtypes = [P(QrActor), P(QrActor), P(QrQCritic), P(QrCtdeTransitions), P(QrCtdeDpgGrad), C.c_void_p]
    lib.qr_ctde_dpg_actor_workspace_bytes.restype = C.c_int64
    lib.qr_ctde_dpg_actor_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    lib.qr_ctde_sac_actor_grad.restype = C.c_int
    lib.qr_ctde_sac_actor_grad.argtypes = [P(QrActor), P(QrActor), P(QrQCritic), P(QrCtdeTransitions), P(QrCtdeSacActorGrad), C.c_void_p]
    lib.qr_ctde_sac_actor_workspace_bytes.restype = C.c_int64
    lib.qr_ctde_sac_actor_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    lib.qr_replay_add.restype = C.c_int
    lib.qr_replay_add.argtypes = [P(QrReplayAdd), C.c_void_p]
    lib.qr_replay_add_rule.restype = C.c_int
    lib.qr_replay_add_rule.argtypes = [P(QrReplayAddRule), C.c_void_p]
    lib.qr_replay_sample.restype = C.c_int
    lib.qr_replay_sample.argtypes = [P(QrReplaySample), C.c_void_p]
    lib.qr_noise_fill.restype = C.c_int
    lib.qr_noise_fill.argtypes = [P(QrNoiseFill), C.c_void_p]
    lib.qr_shuffle.restype = C.c_int
    lib.qr_shuffle.argtypes = [P(QrShuffle), C.c_void_p]
    lib.qr_episode_scan.restype = C.c_int
    lib.qr_episode_scan.argtypes = [P(QrEpisodeScan), C.c_void_p]
    lib.qr_episode_workspace_bytes.restype = C.c_int64
    lib.qr_episode_workspace_bytes.argtypes = [C.c_int64]
    lib.qr_gae_rule.restype = C.c_int
    lib.qr_gae_rule.argtypes = [P(QrGaeRule), C.c_void_p]
    lib.qr_gae_rule_workspace_bytes.restype = C.c_int64
    lib.qr_gae_rule_workspace_bytes.argtypes = [C.c_int64, C.c_int32]
    lib.qr_es_perturb.restype = C.c_int
    lib.qr_es_perturb.argtypes = [P(QrEsPerturb), C.c_void_p]
    lib.qr_es_gradient.restype = C.c_int
    lib.qr_es_gradient.argtypes = [P(QrEsGradient), C.c_void_p]
    lib.qr_es_workspace_bytes.restype = C.c_int64
    lib.qr_es_workspace_bytes.argtypes = [C.c_int32]
    lib.qr_step_kernel_info.restype = C.c_char_p
    lib.qr_step_kernel_info.argtypes = [P(QrEnv), C.c_int32, P(C.c_int32), P(C.c_int32)]
    lib.qr_launch_plan.restype = C.c_int
    lib.qr_launch_plan.argtypes = [P(QrEnv), C.c_int32, C.c_int32, C.c_int32, P(QrLaunchPlan)]
    lib.qr_launch_stats.restype = C.c_int32
    lib.qr_launch_stats.argtypes = [P(C.c_uint32), P(C.c_uint32), C.c_int32, C.c_int32]
    lib.qr_instance_table.restype = C.c_int32
    lib.qr_instance_table.argtypes = [P(C.c_uint32), C.c_int32]
    lib.qr_touch.restype = C.c_int
    lib.qr_touch.argtypes = [P(QrEnv), C.c_void_p, P(QrStepOut), C.c_void_p]
    lib.qr_launch_thresholds.restype = None
    lib.qr_launch_thresholds.argtypes = [P(C.c_int32), P(C.c_int32), P(C.c_int32)]
    if lib.qr_abi_version() != ABI_VERSION:
        raise QuadrotorLibError(f"ABI mismatch: library {lib.qr_abi_version()} vs binding {ABI_VERSION}")
    _lib = lib
    return lib


def default_coeffs() -> QrCoeffs:
    c = QrCoeffs()
    load().qr_default_coeffs(C.byref(c))
    return c


def check(rc: int, what: str):
    if rc == 0:
        return
    if rc < 0:
        raise ValueError(f"{what}: {ERRORS.get(rc, rc)}")
    raise QuadrotorLibError(f"{what}: hipError_t {rc}")


_byref, _Structure = C.byref, C.Structure


def launch(dev, name: str, *args) -> None:
    """One library launch outside the env's hot path: entry `name` on `dev`'s current stream, under torch.cuda.device(dev).  A
    ctypes.Structure goes by reference; None, ints, floats, pointers and ctypes arrays go as they are; the stream is appended.
    The return code goes through `check`."""
    args = [_byref(a) if isinstance(a, _Structure) else a for a in args]
    with torch.cuda.device(dev):
        rc = getattr(load(), name)(*args, torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        check(rc, name)


def workspace_bytes(name: str, *ints) -> int:
    """The size query `name` (a qr_*_workspace_bytes entry) of the given integers; a refusal (negative) goes through `check`."""
    n = getattr(load(), name)(*(int(i) for i in ints))
    check(n if n < 0 else 0, name)
    return int(n)


def launch_thresholds() -> dict:
    """The launch rule's helper-wavefront thresholds of this process, in 64-env tiles (qr_launch_thresholds)."""
    q, w, r = C.c_int32(), C.c_int32(), C.c_int32()
    load().qr_launch_thresholds(C.byref(q), C.byref(w), C.byref(r))
    return {"step_quad": q.value, "step_wrappers": w.value, "rollout": r.value}


LAYOUT_NAME = {v: k for k, v in LAYOUT_ID.items()}
KIND_NAME = {v: k for k, v in KIND_ID.items()}


def describe_key(key: int) -> str:
    """'layout/kind TRAJ=.. ADAPT=.. POLICY=.. SINGLE=.. HELP=.. HREW=.. MAG=..' of a qr_launch_stats / qr_instance_table key."""
    b = key & 0xFF
    return (f"{LAYOUT_NAME[key >> 16]}/{KIND_NAME[(key >> 8) & 0xF]} TRAJ={b & 3} ADAPT={(b >> 2) & 1} POLICY={(b >> 3) & 3} "
            f"SINGLE={(b >> 5) & 1} HELP={(b >> 6) & 1} HREW={(b >> 7) & 1} MAG={(key >> 12) & 1}")


def launch_stats(reset: bool = False) -> dict:
    """{key: launches} of every step-kernel instantiation this process has launched (qr_launch_stats)."""
    lib = load()
    cap = 512
    keys, counts = (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
    n = lib.qr_launch_stats(keys, counts, cap, int(reset))
    return {int(keys[i]): int(counts[i]) for i in range(min(n, cap))}


def instance_table() -> list:
    """Keys of every step-kernel instantiation the library holds (qr_instance_table)."""
    lib = load()
    cap = 512
    keys = (C.c_uint32 * cap)()
    n = lib.qr_instance_table(keys, cap)
    return [int(keys[i]) for i in range(min(n, cap))]
