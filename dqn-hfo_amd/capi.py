"""ctypes declarations of include/dqnhip.h (one entry per exported symbol)."""
import ctypes as C
import os

from ._build import LIB, build

MAX_HIDDEN = 8
NSTEP_MAX = 64           # DQNHIP_NSTEP_MAX
DP_ID_BYTES = 128        # DQNHIP_DP_ID_BYTES
DP_PER_LAYER, DP_HALF_GRADS, DP_SHARD_OPT = 1, 2, 4    # dqnhip_dp_init flags
DP_UNVERIFIED_OK = 256   # lets DP_PER_LAYER / DP_SHARD_OPT through for dp_world > 1 (never run on real links)
TUNE_FP16_WGRAD_PER_LAYER = 1                       # dqnhip_config.tuning_flags bits
TUNE_SEPARATE_HEAD_SEED = 2
TUNE_BWD_UNSHIFTED = 4
TUNE_SEPARATE_ACTOR_HEAD_BWD = 8
TUNE_SEPARATE_Q_TRAIN = 16
TUNE_SEPARATE_FIRST_LAYER = 32
TUNE_SEPARATE_CRITIC_FIRST_LAYERS = 64
TUNE_LATE_GATHER = 128
TUNE_NO_KERNARG_PRELOAD = 256
# dqnhip_update_plan.forms bits (DQNHIP_PLAN_*), in bit order
PLAN_FORMS = ("fp16", "data_parallel", "bwd_shifted_critic", "bwd_shifted_actor", "head_wgrad_rides_critic", "head_wgrad_rides_actor",
              "q_train_in_dgrad", "head_seed_fused", "dqda_head_bwd", "critic_l0_rides", "first_layers_merged", "early_gather_l0", "dp_tails_ride", "prioritized", "n_step", "target_smoothing")
LOSS_SCALE_STATIC, LOSS_SCALE_DYNAMIC = 0, 1        # dqnhip_config.loss_scale_mode
FP32, FP16 = 0, 1                                   # DQNHIP_FP32 / DQNHIP_FP16: dqnhip_config.precision, dqnhip_set_act_precision
ACTOR, CRITIC, ACTOR_TARGET, CRITIC_TARGET = 0, 1, 2, 3
KIND_W, KIND_M, KIND_V, KIND_G = 0, 1, 2, 3       # (KIND_M / KIND_V: solver history 1 / 2)
SOLVERS = ("Adam", "SGD", "Nesterov", "AdaGrad", "RMSProp", "AdaDelta")      # DQNHIP_SOLVER_*, by value: Caffe's type strings


LR_POLICIES = ("fixed", "step", "exp", "inv", "multistep", "poly", "sigmoid")      # DQNHIP_LR_*, by value: Caffe's lr_policy strings
LR_MAX_STEPVALUES = 16                                                           # DQNHIP_LR_MAX_STEPVALUES
REGULARIZATIONS = ("L2", "L1")                                                   # DQNHIP_REG_*, by value: Caffe's regularization_type strings


class Config(C.Structure):
    """struct dqnhip_config (include/dqnhip.h)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("minibatch", C.c_int32), ("state_size", C.c_int32),
        ("num_hidden", C.c_int32), ("hidden", C.c_int32 * MAX_HIDDEN),
        ("replay_capacity", C.c_int32), ("soft_update_freq", C.c_int32),
        ("gamma", C.c_double), ("beta", C.c_double), ("tau", C.c_double),
        ("actor_lr", C.c_float), ("critic_lr", C.c_float), ("momentum", C.c_float),
        ("momentum2", C.c_float), ("delta", C.c_float), ("clip_gradients", C.c_float),
        ("device", C.c_int32), ("dp_world", C.c_int32), ("dp_rank", C.c_int32), ("use_graph", C.c_int32),
        ("seed", C.c_uint64), ("stream", C.c_void_p), ("grad_arena", C.c_void_p),
        ("grad_arena_bytes", C.c_size_t), ("precision", C.c_int32), ("loss_scale", C.c_float),
        ("solver_type", C.c_int32), ("rms_decay", C.c_float),
        ("lr_policy", C.c_int32), ("lr_gamma", C.c_float), ("lr_power", C.c_float), ("lr_stepsize", C.c_int32), ("lr_max_iter", C.c_int32),
        ("lr_n_stepvalue", C.c_int32), ("lr_stepvalue", C.c_int32 * LR_MAX_STEPVALUES), ("weight_decay", C.c_float), ("regularization_type", C.c_int32),
        ("tuning_flags", C.c_int32),
        ("loss_scale_mode", C.c_int32), ("loss_scale_growth_interval", C.c_int32),
        ("loss_scale_min_mult", C.c_float), ("loss_scale_max_mult", C.c_float),
    ]


class LossScaleState(C.Structure):
    """struct dqnhip_loss_scale_state (include/dqnhip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("mode", C.c_int32), ("mult_critic", C.c_float), ("mult_actor", C.c_float),
                ("good_critic", C.c_int32), ("good_actor", C.c_int32), ("backoffs_critic", C.c_int32), ("backoffs_actor", C.c_int32),
                ("growths_critic", C.c_int32), ("growths_actor", C.c_int32), ("skipped_steps", C.c_int32), ("reserved", C.c_int32)]


class UpdatePlan(C.Structure):
    """struct dqnhip_update_plan (include/dqnhip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("forms", C.c_int32), ("launches_single", C.c_int32), ("launches_graph_first", C.c_int32),
                ("launches_in_graph", C.c_int32), ("updates_per_graph", C.c_int32), ("collectives", C.c_int32), ("solver_type", C.c_int32),
                ("lr_policy", C.c_int32), ("regularised", C.c_int32)]


class PerConfig(C.Structure):
    """struct dqnhip_per_config (include/dqnhip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("alpha", C.c_float), ("beta0", C.c_float), ("beta_anneal_iters", C.c_int32),
                ("eps", C.c_float), ("seed", C.c_uint64)]


class PerState(C.Structure):
    """struct dqnhip_per_state (include/dqnhip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("enabled", C.c_int32), ("levels", C.c_int32), ("size", C.c_int32),
                ("total", C.c_float), ("p_max", C.c_float), ("beta_now", C.c_float), ("reserved", C.c_float),
                ("next_counter", C.c_uint64), ("syncs", C.c_int64)]


class StateInfo(C.Structure):
    """struct dqnhip_state_info / dqnhip_state_info_t (include/dqnhip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("version", C.c_int32), ("flags", C.c_int32), ("precision", C.c_int32), ("minibatch", C.c_int32),
                ("state_size", C.c_int32), ("num_hidden", C.c_int32), ("hidden", C.c_int32 * MAX_HIDDEN), ("replay_capacity", C.c_int32),
                ("memory_size", C.c_int32), ("actor_iter", C.c_int32), ("critic_iter", C.c_int32), ("has_memory", C.c_int32),
                ("has_per", C.c_int32), ("has_loss_scale", C.c_int32), ("seed", C.c_uint64), ("update_counter", C.c_uint64),
                ("user_bytes", C.c_uint64), ("file_bytes", C.c_uint64), ("solver_type", C.c_int32), ("rms_decay", C.c_float)]


STATE_NO_MEMORY = 1      # DQNHIP_STATE_NO_MEMORY

DIAG_BINS = 64                                      # DQNHIP_DIAG_BINS
DIAG_MAX_BLOBS = 2 * (2 * MAX_HIDDEN + 4)           # DQNHIP_DIAG_MAX_BLOBS
DIAG_MAX_PANELS = 5 * MAX_HIDDEN                    # DQNHIP_DIAG_MAX_PANELS


class DiagMoments(C.Structure):
    """struct dqnhip_diag_moments (include/dqnhip.h)."""
    _fields_ = [("count", C.c_int64), ("n_zero", C.c_int64), ("n_nonfinite", C.c_int64), ("sum_abs", C.c_double), ("sum_sq", C.c_double),
                ("max_abs", C.c_float), ("reserved", C.c_float)]


class DiagBlob(C.Structure):
    """struct dqnhip_diag_blob (include/dqnhip.h)."""
    _fields_ = [("net", C.c_int32), ("layer", C.c_int32), ("is_bias", C.c_int32), ("reserved", C.c_int32),
                ("w", DiagMoments), ("g", DiagMoments), ("lag", DiagMoments), ("step", DiagMoments), ("g_hist", C.c_int32 * DIAG_BINS)]


class DiagPanel(C.Structure):
    """struct dqnhip_diag_panel (include/dqnhip.h)."""
    _fields_ = [("pass_", C.c_int32), ("layer", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("n_negative", C.c_int64),
                ("dead_units", C.c_int32), ("reserved", C.c_int32), ("a", DiagMoments), ("hist", C.c_int32 * DIAG_BINS)]


class DiagRow(C.Structure):
    """struct dqnhip_diag_row (include/dqnhip.h)."""
    _fields_ = [("min", C.c_float), ("max", C.c_float), ("sum", C.c_double), ("sum_sq", C.c_double), ("n_nonfinite", C.c_int64)]


class DiagAction(C.Structure):
    """struct dqnhip_diag_action (include/dqnhip.h)."""
    _fields_ = [("min", C.c_float), ("max", C.c_float), ("sum", C.c_double), ("n_out_of_bounds", C.c_int64)]


class DiagReport(C.Structure):
    """struct dqnhip_diag_report (include/dqnhip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("n_blobs", C.c_int32), ("n_panels", C.c_int32), ("has_per", C.c_int32),
                ("blobs", DiagBlob * DIAG_MAX_BLOBS), ("panels", DiagPanel * DIAG_MAX_PANELS),
                ("q_target", DiagRow), ("y", DiagRow), ("q_train", DiagRow), ("q_policy", DiagRow), ("td", DiagRow),
                ("n_terminal", C.c_int64), ("actor_out", DiagAction * 10),
                ("dq_da_sum_abs", C.c_double), ("dq_da_max_abs", C.c_float), ("per_w_min", C.c_float), ("per_w_sum", C.c_double),
                ("per_prob_min", C.c_float), ("per_td_abs_max", C.c_float), ("actor_iter", C.c_int32), ("critic_iter", C.c_int32),
                ("critic_loss", C.c_float), ("avg_q", C.c_float), ("grad_norm", C.c_double * 2), ("clip_scale", C.c_double * 2),
                ("fp16", C.c_int32), ("loss_scale_mode", C.c_int32), ("loss_scale_critic", C.c_float), ("loss_scale_dqda", C.c_float),
                ("loss_scale_actor", C.c_float), ("mult_critic", C.c_float), ("mult_actor", C.c_float), ("reserved", C.c_int32)]


class SweepReport(C.Structure):
    """struct dqnhip_sweep_report (include/dqnhip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("first", C.c_int32), ("n", C.c_int32), ("n_chunks", C.c_int32),
                ("n_terminal", C.c_int64), ("n_action_match", C.c_int64),
                ("q", DiagRow), ("y", DiagRow), ("td", DiagRow), ("q_policy", DiagRow), ("mc", DiagRow), ("q_minus_mc", DiagRow),
                ("reward", DiagRow), ("td_hist", C.c_int32 * DIAG_BINS), ("actor_iter", C.c_int32), ("critic_iter", C.c_int32)]


class SweepRows(C.Structure):
    """struct dqnhip_sweep_rows (include/dqnhip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("q", C.POINTER(C.c_float)), ("y", C.POINTER(C.c_float)), ("td", C.POINTER(C.c_float)),
                ("q_policy", C.POINTER(C.c_float)), ("action_match", C.POINTER(C.c_int32))]


fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int32)
up = C.POINTER(C.c_uint8)
H = C.c_void_p

# name -> (restype, argtypes): every function include/dqnhip.h declares
SIGNATURES = {
    "dqnhip_default_config": (None, [C.POINTER(Config), C.c_int32]),
    "dqnhip_solver_name": (C.c_char_p, [C.c_int32]),
    "dqnhip_lr_policy_name": (C.c_char_p, [C.c_int32]),
    "dqnhip_get_learning_rate": (C.c_int, [H, C.c_int32, fp]),
    "dqnhip_grad_arena_bytes": (C.c_size_t, [C.POINTER(Config)]),
    "dqnhip_last_error": (C.c_char_p, []),
    "dqnhip_create": (C.c_int, [C.POINTER(Config), C.POINTER(H)]),
    "dqnhip_destroy": (C.c_int, [H]),
    "dqnhip_update": (C.c_int, [H, ip, fp, fp]),
    "dqnhip_update_chained": (C.c_int, [H, ip, ip, fp, fp]),
    "dqnhip_update_async": (C.c_int, [H, ip]),
    "dqnhip_update_async_n": (C.c_int, [H, C.c_int32]),
    "dqnhip_update_pipelined": (C.c_int, [H, ip, fp, fp]),
    "dqnhip_update_indexed_n": (C.c_int, [H, ip, C.c_int32]),
    "dqnhip_collect_stats": (C.c_int, [H, fp, fp, C.c_int32, ip]),
    "dqnhip_benchmark_blocking": (C.c_int, [H, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, fp]),
    "dqnhip_update_phase": (C.c_int, [H, C.c_int32, ip]),
    "dqnhip_update_abort": (C.c_int, [H]),
    "dqnhip_apply_update": (C.c_int, [H, C.c_int32]),
    "dqnhip_apply_update_sharded": (C.c_int, [H, C.c_int32, C.c_int32]),
    "dqnhip_get_update_plan": (C.c_int, [H, C.POINTER(UpdatePlan)]),
    "dqnhip_grad_buffer": (C.c_int, [H, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "dqnhip_read_stats": (C.c_int, [H, fp, fp]),
    "dqnhip_dp_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "dqnhip_dp_init": (C.c_int, [H, C.c_void_p, C.c_size_t, C.c_int32]),
    "dqnhip_dp_init_file": (C.c_int, [H, C.c_char_p, C.c_int32, C.c_int32]),
    "dqnhip_dp_rendezvous_file": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]),
    "dqnhip_dp_rendezvous_cleanup": (C.c_int, [C.c_char_p, C.c_int32]),
    "dqnhip_dp_graph_active": (C.c_int, [H, ip]),
    "dqnhip_dp_broadcast_params": (C.c_int, [H, C.c_int32]),
    "dqnhip_dp_update": (C.c_int, [H, ip]),
    "dqnhip_dp_update_n": (C.c_int, [H, C.c_int32]),
    "dqnhip_dp_gather_state": (C.c_int, [H]),
    "dqnhip_dp_destroy": (C.c_int, [H]),
    "dqnhip_dp_info": (C.c_int, [ip, C.c_char_p, C.c_size_t]),
    "dqnhip_skipped_steps": (C.c_int, [H, C.POINTER(C.c_int64)]),
    "dqnhip_get_loss_scale": (C.c_int, [H, C.POINTER(LossScaleState)]),
    "dqnhip_set_loss_scale": (C.c_int, [H, C.c_float, C.c_float]),
    "dqnhip_reduce_gradients_local": (C.c_int, [C.POINTER(H), C.c_int32, C.c_int32]),
    "dqnhip_sample_states": (C.c_int, [H, ip, C.c_int32, fp]),
    "dqnhip_get_actor_output": (C.c_int, [H, C.c_int32, C.c_int32, fp]),
    "dqnhip_files_matching_regexp": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, ip]),
    "dqnhip_remove_snapshots": (C.c_int, [C.c_char_p, C.c_int32]),
    "dqnhip_benchmark": (C.c_int, [H, C.c_int32, C.c_int32, fp]),
    "dqnhip_select_actions": (C.c_int, [H, fp, C.c_int32, fp]),
    "dqnhip_select_actions_device": (C.c_int, [H, C.c_void_p, C.c_int32, C.c_void_p]),
    "dqnhip_select_actions_net": (C.c_int, [H, C.c_int32, fp, C.c_int32, fp]),
    "dqnhip_critic_forward": (C.c_int, [H, C.c_int32, fp, fp, C.c_int32, fp]),
    "dqnhip_set_act_precision": (C.c_int, [H, C.c_int32]),
    "dqnhip_get_act_precision": (C.c_int, [H, ip]),
    "dqnhip_add_transitions": (C.c_int, [H, fp, fp, fp, fp, fp, up, C.c_int32]),
    "dqnhip_add_transition": (C.c_int, [H, fp, fp, C.c_float, C.c_float, fp, C.c_uint8]),
    "dqnhip_add_transitions_device": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int32]),
    "dqnhip_label_transitions": (C.c_int, [C.c_double, fp, C.c_int32, fp]),
    "dqnhip_memory_size": (C.c_int, [H, ip]),
    "dqnhip_clear_memory": (C.c_int, [H]),
    "dqnhip_read_memory": (C.c_int, [H, C.c_int32, C.c_int32, fp, fp, fp, fp, fp, up]),
    "dqnhip_snapshot_replay_memory": (C.c_int, [H, C.c_char_p]),
    "dqnhip_load_replay_memory": (C.c_int, [H, C.c_char_p]),
    "dqnhip_get_config": (C.c_int, [H, C.POINTER(Config)]),
    "dqnhip_save_caffemodel": (C.c_int, [H, C.c_int32, C.c_char_p]),
    "dqnhip_load_caffemodel": (C.c_int, [H, C.c_int32, C.c_char_p]),
    "dqnhip_solver_snapshot": (C.c_int, [H, C.c_int32, C.c_char_p, ip]),
    "dqnhip_solver_restore": (C.c_int, [H, C.c_int32, C.c_char_p]),
    "dqnhip_snapshot": (C.c_int, [H, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32]),
    "dqnhip_snapshot_async": (C.c_int, [H, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32]),
    "dqnhip_snapshot_wait": (C.c_int, [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "dqnhip_snapshot_poll": (C.c_int, [H, C.POINTER(C.c_int32)]),
    "dqnhip_find_latest_snapshot": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "dqnhip_find_hiscore": (C.c_int, [C.c_char_p, ip]),
    "dqnhip_remove_files_matching_regexp": (C.c_int, [C.c_char_p]),
    "dqnhip_param_count": (C.c_int, [H, C.c_int32, C.POINTER(C.c_size_t)]),
    "dqnhip_get_params": (C.c_int, [H, C.c_int32, C.c_int32, fp, C.c_size_t]),
    "dqnhip_set_params": (C.c_int, [H, C.c_int32, C.c_int32, fp, C.c_size_t]),
    "dqnhip_clone_to_target": (C.c_int, [H, C.c_int32]),
    "dqnhip_share_parameters": (C.c_int, [H, H, C.c_int32, C.c_int32]),
    "dqnhip_share_replay_memory": (C.c_int, [H, H]),
    "dqnhip_get_iters": (C.c_int, [H, ip, ip]),
    "dqnhip_set_iters": (C.c_int, [H, C.c_int32, C.c_int32]),
    "dqnhip_debug_read": (C.c_int, [H, C.c_char_p, fp, C.c_size_t]),
    "dqnhip_get_stream": (C.c_int, [H, C.POINTER(C.c_void_p)]),
    "dqnhip_set_kernel_timing": (C.c_int, [H, C.c_int32]),
    "dqnhip_get_kernel_timing": (C.c_int, [H, C.c_char_p, fp, C.POINTER(C.c_int64), C.c_int32]),
    "dqnhip_diag_collect": (C.c_int, [H, C.POINTER(DiagReport)]),
    "dqnhip_per_default_config": (None, [C.POINTER(PerConfig)]),
    "dqnhip_per_enable": (C.c_int, [H, C.POINTER(PerConfig)]),
    "dqnhip_per_get_state": (C.c_int, [H, C.POINTER(PerState)]),
    "dqnhip_per_get_priorities": (C.c_int, [H, C.c_int32, C.c_int32, fp]),
    "dqnhip_per_set_priorities": (C.c_int, [H, C.c_int32, C.c_int32, fp]),
    "dqnhip_per_sample": (C.c_int, [H, C.c_uint64, C.c_int32, ip, fp]),
    "dqnhip_per_debug_read": (C.c_int, [H, C.c_char_p, fp, C.c_size_t]),
    "dqnhip_nstep_enable": (C.c_int, [H, C.c_int32]),
    "dqnhip_nstep_get": (C.c_int, [H, ip]),
    "dqnhip_nstep_debug_read": (C.c_int, [H, C.c_char_p, fp, C.c_size_t]),
    "dqnhip_nstep_debug_read_f64": (C.c_int, [H, C.c_char_p, C.POINTER(C.c_double), C.c_size_t]),
    "dqnhip_nstep_validate": (C.c_int, [H, C.c_int32, C.c_int32, C.POINTER(C.c_int64), ip]),
    "dqnhip_evaluate_memory": (C.c_int, [H, C.c_int32, C.c_int32, C.POINTER(SweepReport), C.POINTER(SweepRows)]),
    "dqnhip_per_refresh": (C.c_int, [H, C.c_int32, C.c_int32, C.POINTER(SweepReport)]),
    "dqnhip_save_state": (C.c_int, [H, C.c_char_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "dqnhip_load_state": (C.c_int, [H, C.c_char_p]),
    "dqnhip_state_info": (C.c_int, [C.c_char_p, C.POINTER(StateInfo)]),
    "dqnhip_state_read_user": (C.c_int, [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dqnhip_save_state_async": (C.c_int, [H, C.c_char_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "dqnhip_save_state_wait": (C.c_int, [H]),
    "dqnhip_save_state_poll": (C.c_int, [H, C.POINTER(C.c_int32)]),
    "dqnhip_state_crc32_device": (C.c_int, [H, C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_uint32)]),
}

class EnvConfig(C.Structure):
    """struct dqnhip_env_config (include/dqnhip_env.h)."""
    _fields_ = [("struct_size", C.c_int32), ("workers", C.c_int32), ("max_steps", C.c_int32), ("unum", C.c_int32),
                ("p_end", C.c_float), ("p_goal", C.c_float), ("seed", C.c_uint64)]


SIGNATURES.update({
    "dqnhip_env_create": (C.c_int, [H, C.POINTER(EnvConfig), C.POINTER(C.c_void_p)]),
    "dqnhip_env_destroy": (C.c_int, [C.c_void_p]),
    "dqnhip_env_step": (C.c_int, [C.c_void_p, C.c_float, C.c_int32]),
    "dqnhip_env_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int64)]),
    "dqnhip_env_debug_read": (C.c_int, [C.c_void_p, C.c_char_p, fp, C.c_size_t]),
})

ENV_NO_RECORD = 1        # DQNHIP_ENV_NO_RECORD
NOISE_EXPLORE, NOISE_TARGET = 0, 1   # DQNHIP_NOISE_*


class NoiseConfig(C.Structure):
    """struct dqnhip_noise_config (include/dqnhip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("clamp", C.c_int32), ("sigma_logits", C.c_float), ("sigma_params", C.c_float),
                ("theta", C.c_float), ("clip", C.c_float), ("seed", C.c_uint64)]


SIGNATURES.update({
    "dqnhip_noise_default_config": (C.c_int, [C.POINTER(NoiseConfig), C.c_int32]),
    "dqnhip_noise_explore_host": (C.c_int, [C.POINTER(NoiseConfig), C.c_uint64, C.c_int32, fp, fp]),
    "dqnhip_env_set_noise": (C.c_int, [C.c_void_p, C.POINTER(NoiseConfig)]),
    "dqnhip_target_noise_enable": (C.c_int, [H, C.POINTER(NoiseConfig)]),
    "dqnhip_target_noise_get": (C.c_int, [H, ip, C.POINTER(NoiseConfig)]),
})


class EnvEpisode(C.Structure):
    """struct dqnhip_env_episode (include/dqnhip_env.h)."""
    _fields_ = [("total_reward", C.c_double), ("extrinsic_reward", C.c_double), ("steps", C.c_int32), ("status", C.c_int32),
                ("worker", C.c_int32), ("reserved", C.c_int32), ("step_index", C.c_int64)]


SIGNATURES.update({
    "dqnhip_env_create_external": (C.c_int, [H, C.POINTER(EnvConfig), C.c_int32, fp, C.POINTER(C.c_void_p)]),
    "dqnhip_env_act": (C.c_int, [C.c_void_p, C.c_float, ip, fp, fp]),
    "dqnhip_env_act_device": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dqnhip_env_observe": (C.c_int, [C.c_void_p, fp, ip, ip]),
    "dqnhip_env_observe_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dqnhip_env_read_episodes": (C.c_int, [C.c_void_p, C.POINTER(EnvEpisode), C.c_int32, ip, C.POINTER(C.c_int64)]),
})

_lib = None


def load(rebuild=False):
    """dlopen the in-tree libdqnhip.so (building it first if needed).  There is no
    fallback: a missing or unloadable HIP library is a hard error."""
    global _lib
    if _lib is None or rebuild:
        build()
        if not os.path.exists(LIB):
            raise RuntimeError("libdqnhip.so is missing: the HIP extension is mandatory")
        lib = C.CDLL(LIB)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
