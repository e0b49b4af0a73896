// The host code's view of the bf16-operand twins (common.h "operand type": gemm.hip, attention.hip, elementwise.hip and train.hip compiled a second time with
// -DGTAV_BF16_OPERANDS -Dgtav=gtav_bf16, csrc/build.sh), and the one list of launchers that api_dit.hip / api_vae.hip / api_train.hip dispatch per operand type.
// The twins' declarations are the text of gemm.h / ops.h itself, read again with f16 = __bf16: structs with the same fields, launchers with the same arguments.
// Included by api_internal.h only.
#pragma once
#include "ops.h"

namespace gtav_bf16 {
typedef __bf16 f16;
using gtav_shared::PrefetchDesc;
#include "gemm_typed.inc"
#include "ops_typed.inc"
}  // namespace gtav_bf16

namespace gtav {

// F(field of OperandOps, launcher): every launcher that exists once per operand type.  The fields of OperandOps and both of its instances (api.hip) are generated
// from this list; a new entry needs its prototype in gemm_typed.inc / ops_typed.inc and nothing else.
#define GTAV_OPERAND_OPS(F)                                 \
    F(gemm, launch_gemm)                                    \
    F(ln_modulate, launch_ln_modulate)                      \
    F(ln_affine, launch_ln_affine)                          \
    F(patchify, launch_patchify)                            \
    F(convert_pad, launch_convert_pad_f16)                  \
    F(unpad, launch_unpad_f16_to_f32)                       \
    F(attn_spatial, launch_attn_spatial)                    \
    F(attn_temporal, launch_attn_temporal)                  \
    /* the training step (api_train.hip) */                 \
    F(gemm_tn, launch_gemm_tn)                              \
    F(gemm_dw_grouped, launch_gemm_dw_grouped)              \
    F(transpose_tiled, launch_transpose_tiled_f16)          \
    F(convert_T, launch_convert_T_f16)                      \
    F(gelu_tiled, launch_gelu_tiled)                        \
    F(gelu_bwd_tiled, launch_gelu_bwd_tiled)                \
    F(gelu_bwd_tiled_colsum, launch_gelu_bwd_tiled_colsum)  \
    F(gate_bwd, launch_gate_bwd)                            \
    F(frame_reduce_gate, launch_frame_reduce_gate)          \
    F(gate_bwd_fused, launch_gate_bwd_fused)                \
    F(colsum_tiled, launch_colsum_tiled_f16)                \
    F(to_tiled, launch_to_tiled_f16)                        \
    F(mse_bwd_patch, launch_mse_bwd_patch)                  \
    F(attn_spatial_bwd, launch_attn_spatial_bwd)            \
    F(attn_temporal_bwd, launch_attn_temporal_bwd)          \
    F(adamw_multi, launch_adamw_multi)                      \
    F(adamw_multi_ema, launch_adamw_multi_ema)              \
    F(adamw_swap_ema, launch_adamw_swap_ema)                \
    F(lora_merge, launch_lora_merge)                        \
    F(lora_merge_one, launch_lora_merge_one)                \
    F(lora_grads, launch_lora_grads)                        \
    F(branch_rows, launch_branch_rows)

// One set of launchers per operand type; the signatures are the fp16 ones (the bf16 set casts 2-byte pointers and parameter structs: api.hip twin_call).
struct OperandOps {
#define GTAV_OPS_FIELD(field, launcher) decltype(&launcher) field;
    GTAV_OPERAND_OPS(GTAV_OPS_FIELD)
#undef GTAV_OPS_FIELD
    bool bf16;
};
const OperandOps& operand_ops(bool bf16);   // api.hip

}  // namespace gtav
