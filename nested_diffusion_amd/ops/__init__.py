"""Thin torch-tensor wrappers over the standalone operators of libnd_hip.so.
Every function launches HIP kernels on torch's current stream; inputs must live on the GPU.

One module per job, following the csrc/ units and the sections of include/nested_diffusion.h; each module's docstring names what it
binds.  Callers reach every wrapper as ops.name: this file only gathers the names."""
from .._lib import ND_ACT_GELU, ND_ACT_NONE, ND_ACT_RELU, ND_ACT_SOFTPLUS
from ._base import ACT, _f32, _stream, _workspace, _ws_cache
from .apgd_l2 import apgd_l2_random_start, apgd_l2_step, eot_add
from .attack_l2 import (L2_MAX_PARTS, CwState, cw_attack_space, cw_b_half, cw_control, cw_model_space, cw_update, l2_random_start, l2_step,
                        margin_head_grad)
from .attack_linf import (APGD_IMPROVED, APGD_NOT_PRED, APGD_RESTORE, ApgdState, apgd_control, apgd_random_start, apgd_update,
                          linf_random_start, linf_step)
from .diffusion_train import (BN_EPS, BN_MOMENTUM, SUMSQ_CHUNK, bn_train_backward, bn_train_forward, clip_adam, mse_grad, qsample, sumsq,
                              sumsq_plan)
from .ensemble_grad import (AGGREGATE_MAX_C, RSTEP_INIT, RSTEP_LAST, RSTEP_UPDATE, aggregate_xent_grad, cond_act_grad, cond_mul, reverse_step,
                            reverse_step_coef, reverse_step_grad, softmax_grad)
from .gemm import SplitMatrix, gemm_bias_act, gemm_split, join_rows, split_rows
from .optim import (COLSUM_CHUNK, adam_step, adamw_step, bias_grad_adam, colsum_adamw, ema_step, ensemble_xent_grad, gemm_tn_adamw,
                    gemm_tn_plan, layernorm_wgrad_adamw, linear_wgrad_adam, linear_wgrad_plan)
from .packed_linear import LINEAR_BWD_MAX_M, PackedWeight, linear, linear_grad_input
from .report_tail import aggregate, report, sample_stats, softmax_rows
from .square import SQUARE_ACCEPT, SQUARE_ACTIVE, SquareState, square_accept, square_commit, square_init, square_propose
from .square_l2 import SQUARE_L2_SUMS, SquareL2State, square_l2_commit, square_l2_init, square_l2_propose, square_l2_ws_floats
from .vit import (attention, attention_images, attention_split, gemm_split_qkv, layernorm, layernorm_split, patchify, patchify_split,
                  qkv_images_supported)
from .vit_grad import (ATTENTION_BWD_MAX_TOKENS, attention_grad, gelu_grad_split, gelu_split, layernorm_grad, unpatchify,
                       xent_head_grad)
