"""ctypes binding of libdppo_hip.so (C ABI: include/dppo_hip.h).

The shared library is built in-tree by ``dppo_amd/csrc/build.sh`` (hipcc, gfx950) into
``dppo_amd/lib/``.  There is NO fallback: if the library cannot be loaded every compute entry point
raises, by design -- the product path is the HIP path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

# DPPO_HIP_LIB names another build of the same library (debug variants such as libdppo_hip_stamps.so); never a CPU path
LIB_PATH = os.environ.get("DPPO_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                          "libdppo_hip.so")

PREC_F32, PREC_BF16 = 0, 1
ACT_RELU, ACT_MISH = 0, 1
STAT_PG_LOSS, STAT_V_LOSS, STAT_APPROX_KL, STAT_CLIPFRAC, STAT_RATIO, STAT_ADV_MEAN, STAT_ADV_STD = range(7)
STAT_COUNT = 8

PREC_BY_NAME = {"fp32": PREC_F32, "f32": PREC_F32, "float32": PREC_F32, "bf16": PREC_BF16, "bfloat16": PREC_BF16}


class NetDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("kind", "in_dim", "hidden", "n_blocks", "out_dim", "act", "time_dim", "act_flat", "cond_dim",
                 "cond_hidden", "cond_out", "use_layernorm", "plain")]


class DiffusionCfg(C.Structure):
    _fields_ = [("use_ddim", C.c_int32), ("has_denoised_clip", C.c_int32), ("has_eps_clip", C.c_int32),
                ("has_final_clip", C.c_int32), ("denoised_clip", C.c_float), ("eps_clip", C.c_float),
                ("randn_clip", C.c_float), ("final_clip", C.c_float), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32)]


class AdamwSlot(C.Structure):  # struct dppo_adamw_slot
    _fields_ = [("params", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("n", C.c_int64), ("step_dev", C.c_void_p), ("lr_dev", C.c_void_p), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double), ("sq_norm", C.c_void_p),
                ("max_norm", C.c_double)]


class PpoCfg(C.Structure):
    _fields_ = [("ft_denoising_steps", C.c_int32), ("horizon_steps", C.c_int32), ("action_dim", C.c_int32),
                ("reward_horizon", C.c_int32), ("norm_adv", C.c_int32), ("has_adv_clip", C.c_int32),
                ("has_vclip", C.c_int32), ("pad", C.c_int32),
                ("gamma_denoising", C.c_double), ("clip_ploss_coef", C.c_double),
                ("clip_ploss_coef_base", C.c_double), ("clip_ploss_coef_rate", C.c_double),
                ("clip_vloss_coef", C.c_double), ("adv_clip_lo", C.c_float), ("adv_clip_hi", C.c_float)]


class GaussianCfg(C.Structure):  # struct dppo_gaussian_cfg
    _fields_ = [("horizon_steps", C.c_int32), ("action_dim", C.c_int32), ("tanh_mean", C.c_int32), ("std_mode", C.c_int32),
                ("norm_adv", C.c_int32), ("has_vclip", C.c_int32), ("deterministic", C.c_int32), ("pad", C.c_int32),
                ("fixed_std", C.c_float), ("logvar_min", C.c_float), ("logvar_max", C.c_float), ("randn_clip", C.c_float),
                ("clip_ploss_coef", C.c_double), ("clip_vloss_coef", C.c_double), ("seed_lo", C.c_uint32),
                ("seed_hi", C.c_uint32)]


GAUSS_STAT_ENTROPY, GAUSS_STAT_STD, GAUSS_STAT_COUNT = 7, 8, 9


class UnetDesc(C.Structure):  # struct dppo_unet_desc
    _fields_ = [("action_dim", C.c_int32), ("cond_dim", C.c_int32), ("horizon_steps", C.c_int32), ("time_dim", C.c_int32),
                ("dim", C.c_int32), ("n_levels", C.c_int32), ("mults", C.c_int32 * 4), ("kernel_size", C.c_int32),
                ("n_groups", C.c_int32), ("larger_encoder", C.c_int32), ("cond_predict_scale", C.c_int32),
                ("act", C.c_int32), ("groupnorm_eps", C.c_float)]

class VisDesc(C.Structure):  # struct dppo_vis_desc
    _fields_ = [("in_ch", C.c_int32), ("img_h", C.c_int32), ("img_w", C.c_int32), ("embed_dim", C.c_int32),
                ("num_heads", C.c_int32), ("depth", C.c_int32), ("embed_norm", C.c_int32), ("prop_dim", C.c_int32),
                ("spatial_emb", C.c_int32), ("num_img", C.c_int32)]


class GmmCfg(C.Structure):  # struct dppo_gmm_cfg
    _fields_ = [("horizon_steps", C.c_int32), ("action_dim", C.c_int32), ("num_modes", C.c_int32), ("std_mode", C.c_int32),
                ("norm_adv", C.c_int32), ("has_vclip", C.c_int32), ("deterministic", C.c_int32), ("pad", C.c_int32),
                ("fixed_std", C.c_float), ("logvar_min", C.c_float), ("logvar_max", C.c_float), ("ent_coef", C.c_float),
                ("clip_ploss_coef", C.c_double), ("clip_vloss_coef", C.c_double), ("seed_lo", C.c_uint32),
                ("seed_hi", C.c_uint32)]


class GemmNTDesc(C.Structure):  # struct dppo_gemm_nt_desc (tests and tools only)
    _fields_ = [("X", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("M", C.c_int64), ("N", C.c_int32),
                ("Kp", C.c_int32), ("ldx", C.c_int32), ("ldw", C.c_int32), ("dsrc", C.c_void_p), ("dsrc_kind", C.c_int32),
                ("dsrc_ld", C.c_int32), ("dact", C.c_int32), ("ldres", C.c_int32), ("res", C.c_void_p), ("add", C.c_void_p),
                ("out_f32", C.c_void_p), ("out_pre", C.c_void_p), ("out_act", C.c_void_p), ("ldadd", C.c_int32),
                ("ldo32", C.c_int32), ("ldo", C.c_int32), ("act", C.c_int32)]


class GemmTNJob(C.Structure):  # struct dppo_gemm_tn_job (tests and tools only)
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("slab", C.c_void_p), ("M", C.c_int64), ("lda", C.c_int32),
                ("N1", C.c_int32), ("ldb", C.c_int32), ("N2", C.c_int32), ("rows_per_split", C.c_int32),
                ("ncol_a", C.c_int32), ("ncol_b", C.c_int32), ("pad", C.c_int32)]


class IdqlBatch(C.Structure):  # struct dppo_idql_batch
    _fields_ = [("obs", C.c_void_p), ("next_obs", C.c_void_p), ("actions", C.c_void_p), ("reward", C.c_void_p),
                ("terminated", C.c_void_p), ("inds", C.c_void_p), ("cap", C.c_int64), ("n_envs", C.c_int64),
                ("head", C.c_int64), ("count", C.c_int64)]


class SacCfg(C.Structure):  # struct dppo_sac_cfg
    _fields_ = [("horizon_steps", C.c_int32), ("action_dim", C.c_int32), ("deterministic", C.c_int32), ("squash", C.c_int32),
                ("logvar_min", C.c_float), ("logvar_max", C.c_float), ("randn_clip", C.c_float), ("pad", C.c_float),
                ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32)]


class CalqlCfg(C.Structure):  # struct dppo_calql_cfg
    _fields_ = [("n_random", C.c_int32), ("n_next", C.c_int32), ("per_row_logpi", C.c_int32), ("pad", C.c_int32),
                ("min_q_weight", C.c_float), ("clip_diff_min", C.c_float), ("clip_diff_max", C.c_float), ("log_rand_pi", C.c_float),
                ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32)]


class Dropout(C.Structure):  # struct dppo_dropout
    _fields_ = [("p", C.c_float), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("pad", C.c_int32), ("mask", C.c_void_p),
                ("mask_out", C.c_void_p)]


IDQL_STAT_COUNT = 3
RLPD_MAX_E = 16  # csrc/rlpd.h
CALQL_STAT_COUNT = 6
DQL_STAT_COUNT = 5
SAC_STAT_COUNT = 4

DP_HOOK_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)  # void (*)(void* user, dppo_stream_t side)


class DpHook(C.Structure):  # struct dppo_dp_hook
    _fields_ = [("critic_grads_enqueued", DP_HOOK_FN), ("user", C.c_void_p)]


class ObsIO(C.Structure):  # struct dppo_obs_io
    _fields_ = [("obs_critic", C.c_void_p), ("d_obs_actor", C.c_void_p), ("d_obs_critic", C.c_void_p)]


# numpy mirror of `dppo_step` (40 bytes) so schedules are built vectorised on the host
STEP_DTYPE = np.dtype([("net", "<i4"), ("t", "<i4"), ("chain_slot", "<i4"), ("final_clip", "<i4"),
                       ("c0", "<f4"), ("c1", "<f4"), ("c2", "<f4"), ("c3", "<f4"), ("std", "<f4"), ("pad", "<f4")])
assert STEP_DTYPE.itemsize == 40

# every symbol include/dppo_hip.h declares: name -> (restype, argtypes)
_P, _I, _L, _D = C.c_void_p, C.c_int, C.c_int64, C.c_double
_ND = C.POINTER(NetDesc)
SYMBOLS = {
    "dppo_version": (C.c_int, []),
    "dppo_last_error": (C.c_char_p, []),
    "dppo_net_param_count": (_L, [_ND]),
    "dppo_packed_bytes": (_L, [_ND, _I, _I]),
    "dppo_pack_net": (_I, [_ND, _I, _I, _P, _P, _P]),
    "dppo_mlp_forward_workspace_bytes": (_L, [_ND, _I, _L]),
    "dppo_actor_forward": (_I, [_ND, _I, _P, _P, _P, _P, _P, _L, _P, _P, _L, _P]),
    "dppo_critic_forward": (_I, [_ND, _I, _P, _P, _P, _L, _P, _P, _L, _P]),
    "dppo_sample_chain_workspace_bytes": (_L, [_ND, _I, _L]),
    "dppo_sample_chain_exchange_bytes": (_L, [_ND, _I, _L]),
    "dppo_sample_chain": (_I, [_ND, _I, _P, _P, _P, _P, C.POINTER(DiffusionCfg), _P, _I, _P, _P, _L, _P, _P, _I, _I,
                               _P, _L, _P]),
    "dppo_plain_sample_workspace_bytes": (_L, [_ND, _I, _L]),
    "dppo_plain_sample_chain": (_I, [_ND, _I, _P, _P, _P, _P, C.POINTER(DiffusionCfg), _P, _I, _P, _P, _L, _P, _P, _I, _I, _P,
                                     _L, _P]),
    "dppo_chain_logprob_workspace_bytes": (_L, [_ND, _I, _L, _I]),
    "dppo_chain_logprob": (_I, [_ND, _I, _P, _P, C.POINTER(DiffusionCfg), _P, _I, _P, _P, _L, _P, _P, _L, _P]),
    "dppo_bc_loss_workspace_bytes": (_L, [_ND, _I, _L, _I]),
    "dppo_bc_loss_fwd_bwd": (_I, [_ND, _I, _P, _P, C.POINTER(DiffusionCfg), _P, _I, _P, _P, _L, _P, _P, _P, _L, _P]),
    "dppo_axpy": (_I, [_P, _P, _D, _L, _P]),
    "dppo_denoise_mse_workspace_bytes": (_L, [_ND, _I, _L]),
    "dppo_denoise_mse_fwd_bwd": (_I, [_ND, _I, _P, _P, _P, _I, _P, _P, _P, _L, _P, _P, _P, _L, _P]),
    "dppo_gae": (_I, [_P, _P, _P, _P, _I, _I, _D, _D, _D, _P, _P, _P, _P, _P]),
    "dppo_ppo_workspace_bytes": (_L, [_ND, _ND, _I, _L]),
    "dppo_ppo_loss_fwd_bwd": (_I, [_ND, _ND, _I, _P, _P, _P, _P, C.POINTER(DiffusionCfg), C.POINTER(PpoCfg), _P,
                                   _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _L, _P]),
    "dppo_ppo_loss_fwd_bwd_dp": (_I, [_ND, _ND, _I, _P, _P, _P, _P, C.POINTER(DiffusionCfg), C.POINTER(PpoCfg), _P,
                                      _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _L, _P, C.POINTER(DpHook)]),
    "dppo_gaussian_workspace_bytes": (_L, [_ND, _ND, _I, _L]),
    "dppo_gaussian_sample": (_I, [_ND, _I, _P, _P, C.POINTER(GaussianCfg), _P, _P, _P, _L, _P, _P, _P, _L, _P]),
    "dppo_gaussian_logprob": (_I, [_ND, _I, _P, _P, C.POINTER(GaussianCfg), _P, _P, _P, _L, _P, _P, _L, _P]),
    "dppo_gaussian_ppo_loss_fwd_bwd": (_I, [_ND, _ND, _I, _P, _P, _P, _P, C.POINTER(GaussianCfg), _P, _P, _P, _P, _P, _P,
                                            _P, _L, _P, _P, _P, _P, _P, _P, _L, _P]),
    "dppo_unet_param_count": (_L, [C.POINTER(UnetDesc)]),
    "dppo_unet_packed_bytes": (_L, [C.POINTER(UnetDesc), _I, _I]),
    "dppo_gmm_workspace_bytes": (_L, [_ND, _ND, _ND, _I, _L]),
    "dppo_gmm_sample": (_I, [_ND, _ND, _I, _P, _P, _P, _P, C.POINTER(GmmCfg), _P, _P, _P, _P, _L, _P, _P, _L, _P]),
    "dppo_gmm_logprob": (_I, [_ND, _ND, _I, _P, _P, _P, _P, C.POINTER(GmmCfg), _P, _P, _P, _L, _P, _P, _L, _P]),
    "dppo_gmm_ppo_loss_fwd_bwd": (_I, [_ND, _ND, _ND, _I, _P, _P, _P, _P, _P, _P, C.POINTER(GmmCfg), _P, _P, _P, _P, _P, _P, _P,
                                       _L, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    # behaviour-cloning pre-training of the Gaussian / mixture policies (GaussianModel.loss, GMMModel.loss)
    "dppo_gaussian_bc_workspace_bytes": (_L, [_ND, _I, _L]),
    "dppo_gaussian_bc_loss_fwd_bwd": (_I, [_ND, _I, _P, _P, C.POINTER(GaussianCfg), _P, _P, _P, _L, _D, _P, _P, _P, _P, _L, _P]),
    "dppo_gmm_bc_workspace_bytes": (_L, [_ND, _ND, _I, _L]),
    "dppo_gmm_bc_loss_fwd_bwd": (_I, [_ND, _ND, _I, _P, _P, _P, _P, C.POINTER(GmmCfg), _P, _P, _P, _L, _P, _P, _P, _P, _P, _L,
                                      _P]),
    # IDQL: twin-Q / expectile-V losses over the device replay ring, best-of-N selection, Polyak target (csrc/idql.hip)
    "dppo_idql_v_loss_workspace_bytes": (_L, [_ND, _ND, _I, _L, _I]),
    "dppo_idql_v_loss_fwd_bwd": (_I, [_ND, _ND, _I, _P, _P, _P, _P, _P, C.POINTER(IdqlBatch), _L, _D, _I, _P, _P, _P, _P, _L, _P]),
    "dppo_idql_q_loss_workspace_bytes": (_L, [_ND, _ND, _I, _L, _I]),
    "dppo_idql_q_loss_fwd_bwd": (_I, [_ND, _ND, _I, _P, _P, _P, _P, _P, C.POINTER(IdqlBatch), _L, _D, _I, _P, _P, _P, _L, _P]),
    "dppo_idql_q_forward_workspace_bytes": (_L, [_ND, _I, _L, _I]),
    "dppo_idql_q_forward": (_I, [_ND, _I, _P, _P, _P, _P, _I, _L, _P, _L, _I, _P, _P, _P, _L, _P]),
    "dppo_idql_select": (_I, [_P, _P, _P, _I, _P, _P, _L, _I, _I, _I, _D, C.c_uint64, _P, _P, _P]),
    "dppo_polyak": (_I, [_P, _P, _D, _L, _P]),
    # QSM: the twin critic's action gradient as the actor's regression target, TD loss on the target twin (csrc/qsm.hip)
    "dppo_qsm_actor_target_workspace_bytes": (_L, [_ND, _I, _I, _L]),
    "dppo_qsm_actor_target": (_I, [_ND, _I, _P, _P, _P, C.POINTER(IdqlBatch), _I, _L, _P, _P, _P, _P, _I, _D, _P, _P, _P, _P, _L,
                                   _P]),
    "dppo_qsm_q_loss_workspace_bytes": (_L, [_ND, _I, _I, _L]),
    "dppo_qsm_q_loss_fwd_bwd": (_I, [_ND, _I, _P, _P, _P, _P, _P, _P, C.POINTER(IdqlBatch), _I, _P, _L, _D, _P, _P, _P, _L, _P]),
    # DQL: the actor loss differentiated through the K-step sampling chain (csrc/dql.hip)
    "dppo_dql_actor_workspace_bytes": (_L, [_ND, _ND, _I, _I, _L, _I]),
    "dppo_dql_actor_fwd_bwd": (_I, [_ND, _ND, _I, _P, _P, _P, _P, _P, C.POINTER(DiffusionCfg), _P, _I, C.POINTER(IdqlBatch), _I, _L,
                                    _P, _P, _P, _P, _P, _D, _I, _P, _P, _P, _P, _P, _L, _P]),
    # SAC: the two-headed tanh-Gaussian epilogue, the entropy-regularised TD loss, the actor loss through min(Q1, Q2), the
    # temperature loss (csrc/sac.hip)
    "dppo_sac_sample_workspace_bytes": (_L, [_ND, _I, _L]),
    "dppo_sac_sample": (_I, [_ND, _I, _P, _P, C.POINTER(SacCfg), _P, _P, _L, _P, _P, _P, _P, _L, _P]),
    "dppo_sac_q_loss_workspace_bytes": (_L, [_ND, _I, _I, _L]),
    "dppo_sac_q_loss_fwd_bwd": (_I, [_ND, _I, _P, _P, _P, _P, _P, _P, C.POINTER(IdqlBatch), _I, _P, _P, _P, _L, _D, _P, _P, _P, _L,
                                     _P]),
    "dppo_sac_actor_workspace_bytes": (_L, [_ND, _ND, _I, _I, _L]),
    "dppo_sac_actor_fwd_bwd": (_I, [_ND, _ND, _I, _P, _P, _P, _P, _P, C.POINTER(SacCfg), C.POINTER(IdqlBatch), _I, _L, _P, _P, _P,
                                    _P, _P, _P, _P, _P, _P, _L, _P]),
    "dppo_sac_alpha_loss": (_I, [_P, _L, _P, _D, _P, _P]),
    # RLPD: the TD loss of an ensemble of LayerNorm Q trunks (csrc/rlpd.hip)
    "dppo_rlpd_q_loss_workspace_bytes": (_L, [_ND, _I, _I, _L, _I]),
    "dppo_rlpd_q_loss_fwd_bwd": (_I, [_ND, _I, _I, _P, C.POINTER(C.c_void_p), _P, C.POINTER(C.c_void_p), _I, _I, C.POINTER(IdqlBatch), _I,
                                      _P, _P, _P, _L, _D, _P, _P, _P, _L, _P]),
    # ... and the actor loss through the mean of the members' Q
    "dppo_rlpd_actor_workspace_bytes": (_L, [_ND, _ND, _I, _I, _L, _I]),
    "dppo_rlpd_actor_fwd_bwd": (_I, [_ND, _ND, _I, _I, _P, _P, _P, C.POINTER(C.c_void_p), C.POINTER(SacCfg), C.POINTER(IdqlBatch), _I,
                                     _L, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    # Cal-QL: the conservative critic loss on a twin of LayerNorm Q trunks (csrc/calql.hip)
    "dppo_calql_q_loss_workspace_bytes": (_L, [_ND, _I, _I, _L, _I, _I]),
    "dppo_calql_q_loss_fwd_bwd": (_I, [_ND, _I, _P, _P, _P, _P, _P, _P, C.POINTER(CalqlCfg), C.POINTER(IdqlBatch), _I, _P, _P, _P, _P,
                                       _P, _P, _P, _L, _D, _P, _P, _P, _P, _P, _L, _P]),
    # ... and the actor loss through the min of that twin (dppo_sac_actor_fwd_bwd's argument list)
    "dppo_calql_actor_workspace_bytes": (_L, [_ND, _ND, _I, _I, _L]),
    "dppo_calql_actor_fwd_bwd": (_I, [_ND, _ND, _I, _P, _P, _P, _P, _P, C.POINTER(SacCfg), C.POINTER(IdqlBatch), _I, _L, _P, _P, _P,
                                      _P, _P, _P, _P, _P, _P, _L, _P]),
    # IBRL: dropout in a plain actor, the Q-guided choice between two proposals, the ensemble's TD loss (csrc/ibrl.hip)
    "dppo_gaussian_sample_drop": (_I, [_ND, _I, _P, _P, C.POINTER(GaussianCfg), _P, _P, _P, _L, _P, _P, C.POINTER(Dropout), _P, _L,
                                       _P]),
    "dppo_ibrl_act_workspace_bytes": (_L, [_ND, _ND, _I, _L]),
    "dppo_ibrl_act": (_I, [_ND, _ND, _I, _I, _P, _P, _P, _P, C.POINTER(GaussianCfg), C.POINTER(GaussianCfg), C.POINTER(Dropout),
                           C.POINTER(Dropout), _P, C.POINTER(C.c_void_p), _I, _I, _P, _P, _P, _L, _I, _D, _P, C.c_uint32, C.c_uint32,
                           _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    "dppo_ibrl_q_loss_workspace_bytes": (_L, [_ND, _I, _I, _L, _I]),
    "dppo_ibrl_q_loss_fwd_bwd": (_I, [_ND, _I, _I, _P, C.POINTER(C.c_void_p), _P, C.POINTER(C.c_void_p), _I, _I, C.POINTER(IdqlBatch), _I,
                                      _P, _P, _L, _D, _P, _P, _P, _P, _P, _L, _P]),
    # ... and the actor loss through the min of the members' Q, backwards through the actor's dropout
    "dppo_ibrl_actor_workspace_bytes": (_L, [_ND, _ND, _I, _I, _L, _I]),
    "dppo_ibrl_actor_fwd_bwd": (_I, [_ND, _ND, _I, _I, _P, _P, _P, C.POINTER(C.c_void_p), C.POINTER(GaussianCfg), C.POINTER(Dropout),
                                     C.POINTER(IdqlBatch), _I, _L, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    # the *_obs entries: pre-gathered mode only (no `inds`), + dppo_obs_io* / d_obs
    "dppo_ppo_loss_fwd_bwd_obs": (_I, [_ND, _ND, _I, _P, _P, _P, _P, C.POINTER(DiffusionCfg), C.POINTER(PpoCfg), _P,
                                       _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _L, _P, C.POINTER(ObsIO)]),
    "dppo_unet_ppo_loss_fwd_bwd_obs": (_I, [C.POINTER(UnetDesc), _ND, _I, _P, _P, _P, _P, C.POINTER(DiffusionCfg),
                                            C.POINTER(PpoCfg), _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _L, _P,
                                            C.POINTER(ObsIO)]),
    "dppo_gaussian_ppo_loss_fwd_bwd_obs": (_I, [_ND, _ND, _I, _P, _P, _P, _P, C.POINTER(GaussianCfg), _P, _P, _P, _P, _P, _P,
                                            _P, _L, _P, _P, _P, _P, _P, _P, _L, _P, C.POINTER(ObsIO)]),
    "dppo_denoise_mse_fwd_bwd_obs": (_I, [_ND, _I, _P, _P, _P, _I, _P, _P, _P, _L, _P, _P, _P, _L, _P, _P]),
    "dppo_unet_denoise_mse_fwd_bwd_obs": (_I, [C.POINTER(UnetDesc), _I, _P, _P, _P, _I, _P, _P, _P, _L, _P, _P, _P, _L, _P, _P]),
    "dppo_vis_param_count": (_L, [C.POINTER(VisDesc)]),
    "dppo_vis_packed_bytes": (_L, [C.POINTER(VisDesc), _I]),
    "dppo_vis_pack": (_I, [C.POINTER(VisDesc), _I, _P, _P, _P]),
    "dppo_vis_workspace_bytes": (_L, [C.POINTER(VisDesc), _I, _L, _I]),
    "dppo_vis_encode": (_I, [C.POINTER(VisDesc), _I, _P, _P, _P, _I, _P, _L, _P, _I, _I, _P, _L, _P]),
    "dppo_vis_backward": (_I, [C.POINTER(VisDesc), _I, _P, _P, _P, _I, _L, _P, _P, _L, _P]),
    "dppo_unet_pack": (_I, [C.POINTER(UnetDesc), _I, _I, _P, _P, _P]),
    "dppo_unet_workspace_bytes": (_L, [C.POINTER(UnetDesc), _I, _L]),
    "dppo_unet_sample_workspace_bytes": (_L, [C.POINTER(UnetDesc), _I, _L, _I]),
    "dppo_unet_forward": (_I, [C.POINTER(UnetDesc), _I, _P, _P, _P, _P, _P, _L, _P, _P, _L, _P]),
    "dppo_unet_sample_chain": (_I, [C.POINTER(UnetDesc), _I, _P, _P, _P, _P, C.POINTER(DiffusionCfg), _P, _I, _P, _P, _L, _P,
                                    _P, _I, _I, _P, _L, _P]),
    "dppo_unet_chain_logprob": (_I, [C.POINTER(UnetDesc), _I, _P, _P, C.POINTER(DiffusionCfg), _P, _P, _I, _P, _P, _L, _P, _P,
                                     _L, _P]),
    "dppo_unet_ppo_workspace_bytes": (_L, [C.POINTER(UnetDesc), _ND, _I, _L]),
    "dppo_unet_ppo_loss_fwd_bwd": (_I, [C.POINTER(UnetDesc), _ND, _I, _P, _P, _P, _P, C.POINTER(DiffusionCfg),
                                        C.POINTER(PpoCfg), _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _L, _P]),
    "dppo_unet_denoise_mse_workspace_bytes": (_L, [C.POINTER(UnetDesc), _I, _L]),
    "dppo_unet_denoise_mse_fwd_bwd": (_I, [C.POINTER(UnetDesc), _I, _P, _P, _P, _I, _P, _P, _P, _L, _P, _P, _P, _L, _P]),
    "dppo_grad_sq_norm": (_I, [_P, _L, _P, _P, _P]),
    "dppo_adamw_step": (_I, [_P, _P, _P, _P, _L, _I, _D, _D, _D, _D, _D, _P, _D, _P]),
    "dppo_adamw_step_dev": (_I, [_P, _P, _P, _P, _L, _P, _P, _D, _D, _D, _D, _P, _D, _P]),
    "dppo_adamw_step_multi": (_I, [_P, _I, _P]),
    "dppo_pack_nets": (_I, [_ND, _I, _P, _P, _ND, _I, _P, _P, _I, _P]),
    "dppo_stats_split": (_I, [_P, _P, _P]),
    "dppo_stats_merge": (_I, [_P, _P, _I, _P]),
    "dppo_stats_merge_n": (_I, [_P, _P, _I, _I, _P]),
    "dppo_probe_arm": (_I, [_I, _I]),
    "dppo_probe_collect": (_I, [C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "dppo_probe_collect_bytes": (_I, [C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double)]),
    "dppo_tune_set": (_I, [_I, _I]),
    "dppo_backward_route": (_I, [_ND, _I, _L, _I, _I, C.POINTER(C.c_int)]),
    "dppo_ppo_loss_route": (_I, [_ND, _ND, _I, _L, _I]),
    "dppo_gemm_nt_raw": (_I, [_I, _P, _P, _P, _L, _I, _I, _P, _P, _I, _I, _P]),
    "dppo_gemm_tn_raw": (_I, [_I, _P, _I, _I, _P, _I, _I, _L, _I, _P, _P, _P]),
    "dppo_gemm_nt_desc_raw": (_I, [_I, C.POINTER(GemmNTDesc), _P]),
    "dppo_gemm_tn_group_raw": (_I, [_I, C.POINTER(GemmTNJob), _I, C.POINTER(C.c_void_p), _P]),
    "dppo_gemm_tn_job_raw": (_I, [_I, C.POINTER(GemmTNJob), _P, _P]),
}

_lib: Optional[C.CDLL] = None


class DppoHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the HIP library (once).  Raises DppoHipError when it is missing -- there is no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DppoHipError(
                f"{LIB_PATH} not found: build it with dppo_amd/csrc/build.sh (or __graft_entry__.build()). "
                "dppo_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        for kv in filter(None, os.environ.get("DPPO_TUNE", "").split(",")):  # e.g. DPPO_TUNE=2=0,7=1 (dppo_tune_set knobs)
            k, v = kv.split("=")
            if lib.dppo_tune_set(int(k), int(v)) != 0:
                raise DppoHipError(f"DPPO_TUNE: bad knob {kv!r}: {lib.dppo_last_error().decode()}")
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().dppo_last_error().decode()
        raise DppoHipError(f"{what} failed (rc={rc}): {msg}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_contiguous(), "dppo_amd kernels take contiguous tensors"
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream() -> int:
    """hipStream_t of torch's current stream on the current device (called once per library call: the raw getter costs
    0.3 us where ``torch.cuda.current_stream().cuda_stream`` costs 10)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise DppoHipError(f"{what}: tensor is on {t.device}; the DPPO hot path runs on an MI355X only "
                           "(no CPU fallback)")


class Workspace:
    """Grow-only device scratch buffer (one per purpose, reused across calls)."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int, device, what: Optional[str] = None) -> torch.Tensor:
        """``nbytes`` as the library's ``<entry>_workspace_bytes`` returned it: a negative one is that query's refusal, raised
        under the name ``what``."""
        if nbytes < 0:
            check(int(nbytes), what)
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            # zero-filled: a sampling workspace begins with the sticky time-out word (include/dppo_hip.h, dppo_sample_chain)
            self.buf = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        return self.buf
