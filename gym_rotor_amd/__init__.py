"""gym_rotor_amd — MI355X-native batched quadrotor dynamics engine.

Drop-in for the env.step() hot path of fdcl-gwu/gym-rotor (Quad-v0, CoupledWrapper,
DecoupledWrapper), executed by hand-written HIP kernels for gfx950 behind a C-ABI
(include/quadrotor_hip.h).  See DESIGN.md / INTEGRATION.md.
"""
from .constants import ACTION_DIM, ALGO_BYTES, FRAMEWORK, KINDS, N_AGENTS, OBS_DIMS, QuadConstants  # noqa: F401
from .spaces import Box  # noqa: F401
from .sharding import shard_range, make_sharded_env, all_gather_rows  # noqa: F401
from .vec_env import CapturedStep, QuadVecEnv, as_gymnasium_vector_env  # noqa: F401
from .compat import QuadEnv, CoupledWrapper, DecoupledWrapper  # noqa: F401
from .rollout import RolloutStorage, gae_rule, gae_rule_workspace_numel  # noqa: F401
from .policy import ActorParams, ActorPopulation, CriticParams, QCriticParams, actor_loss, critic_loss, ppo_actor_grad, ppo_critic_grad, random_actors  # noqa: F401
from .optim import DeviceAdamW, PolyakAdamW, PpoUpdater, adamw_polyak_step, adamw_step, minibatch_slices  # noqa: F401
from .td3 import ReplayBuffer, dpg_actor_grad, soft_update, td3_actor_loss, td3_critic_loss, td3_target, twinq_grad  # noqa: F401
from .td3 import td3_critic_loss_ctde, td3_target_ctde, twinq_grad_ctde  # noqa: F401
from .td3 import dpg_actor_grad_ctde, dpg_actor_workspace_bytes_ctde, td3_actor_loss_ctde  # noqa: F401
from .td3 import TimeLimitRule, replay_add, replay_sample  # noqa: F401
from .sac import sac_actor_grad, sac_actor_loss, sac_actor_workspace_bytes, sac_critic_loss, sac_target  # noqa: F401
from .sac import sac_critic_loss_ctde, sac_target_ctde  # noqa: F401
from .sac import sac_actor_grad_ctde, sac_actor_loss_ctde, sac_actor_workspace_bytes_ctde  # noqa: F401
from .noise import DeviceNoise, noise_fill  # noqa: F401
from .shuffle import ppo_stream, shuffle  # noqa: F401
from .episodes import EpisodeTracker, episode_scan, episode_workspace_numel  # noqa: F401
from .offpolicy import OffPolicyCollector, SacUpdater, Td3Updater  # noqa: F401
from .ppo import PpoCollector  # noqa: F401
from .evaluate import EvalResult, PopulationResult, evaluate_policy, evaluate_population  # noqa: F401
from .es import EvolutionStrategy, es_gradient, es_perturb, es_stream  # noqa: F401  (the module's other helpers stay in gym_rotor_amd.es)
from . import torch_ops  # noqa: F401  (registers torch.ops.gym_rotor_amd.*)

__all__ = ["QuadVecEnv", "QuadEnv", "CoupledWrapper", "DecoupledWrapper", "QuadConstants", "Box",
           "shard_range", "make_sharded_env", "all_gather_rows", "RolloutStorage"]
