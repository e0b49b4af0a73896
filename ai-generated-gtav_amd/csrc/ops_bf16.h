// The bf16-operand twins of the launchers api_dit.hip / api_vae.hip / api_train.hip dispatch per operand type (common.h "operand type"): gemm.hip, attention.hip, elementwise.hip and
// train.hip compiled a second time with -DGTAV_BF16_OPERANDS -Dgtav=gtav_bf16 (csrc/build.sh).  Same kernels, same argument meaning as gemm.h / ops.h; `f16*` there is `__bf16*` here and the
// parameter structs are the twin namespace's own (identical layout, asserted by every translation unit against struct_layout.h: api.hip passes its gtav::GemmParams /
// LnPending / GemmDwGroup / AdamParam / AdamItem through a reference cast).
// Keep the signatures in step with ops.h / gemm.h: a mismatch is a link error, never a silent one.
#pragma once
#include "ops.h"

namespace gtav_bf16 {
struct GemmParams;
struct LnPending;
int launch_gemm(const GemmParams& p, int epi, hipStream_t stream);
int launch_ln_modulate(float* x, int ldx, __bf16* out, int ldo, int M, int D, const float* shift, const float* scale, int mod_stride, const int* rows,
                       int rows_per_mod, const LnPending* pend, int* err_flag, hipStream_t stream);
int launch_ln_affine(float* x, int ldx, __bf16* out, int ldo, int M, int D, const float* gamma, const float* beta, const LnPending* pend, int* err_flag,
                     hipStream_t stream);
int launch_patchify(const float* img, const int* frame_index, int NB, int C, int H, int W, int p, __bf16* out, int ldo, float a, float b, int* err_flag,
                    hipStream_t stream);
int launch_convert_pad_f16(const float* src, int lds, int R, int C, __bf16* dst, int Rp, int Cp, float scale, int tiled, hipStream_t stream, int* err_flag);
int launch_unpad_f16_to_f32(const __bf16* src, int lds, int R, int C, float* dst, int tiled, hipStream_t stream);
int launch_attn_spatial(const __bf16* Q, const __bf16* K, const __bf16* Vt, __bf16* O, int NB, int heads, int S, hipStream_t stream, bool q_prescaled);
int launch_attn_temporal(const __bf16* q, const __bf16* kv, __bf16* O, int B, int P, int D, int Tq, int t0, int Tmax, hipStream_t stream);
// the training step of a bf16 handle (train.hip and the GEMM's weight-gradient launches compiled as twins; api_train.hip through gtav::TrainOps)
struct GemmDwGroup;
struct AdamParam;
struct AdamItem;
int launch_gemm_tn(const GemmParams& p, hipStream_t stream);
int launch_gemm_dw_grouped(const GemmDwGroup* g, int n, int K, int* err_flag, hipStream_t stream, bool tn);
int launch_transpose_tiled_f16(const __bf16* src, int R, int C, __bf16* dst, hipStream_t stream);
int launch_convert_T_f16(const float* src, int lds, int R, int C, __bf16* dst, hipStream_t stream);
int launch_gelu_tiled(const __bf16* u, __bf16* h, size_t n, hipStream_t stream);
int launch_gelu_bwd_tiled(const __bf16* dh, const __bf16* u, __bf16* du, size_t n, int* err_flag, hipStream_t stream);
int launch_gelu_bwd_tiled_colsum(const __bf16* dh, const __bf16* u, __bf16* du, int M, int N, float* db, float* ws, int* err_flag, hipStream_t stream);
int launch_gate_bwd(const float* dres, const float* gate, int mod_stride, int rows_per_mod, int M, int D, __bf16* dy_tiled, int* err_flag, hipStream_t stream);
int launch_frame_reduce_gate(const float* dres, const __bf16* y, int frames, int P, int D, float* dgate, int mod_stride, hipStream_t stream);
int launch_gate_bwd_fused(const float* dres, const __bf16* y, const float* gate, int mod_stride, int frames, int P, int D, __bf16* dy_tiled, float* dgate,
                          float* db, float* ws, int* err_flag, hipStream_t stream);
int launch_colsum_tiled_f16(const __bf16* dy, int M, int N, float* db, float* ws, hipStream_t stream);
int launch_to_tiled_f16(const float* a, int M, int D, __bf16* out, int* err_flag, hipStream_t stream);
int launch_mse_bwd_patch(const float* vpred, const float* vtarget, int B, int T, int C, int H, int W, int p, float scale, __bf16* dfo, int ldf, int* err_flag,
                         hipStream_t stream);
int launch_attn_spatial_bwd(const __bf16* Q, const __bf16* K, const __bf16* Vt, const __bf16* dO, int NB, int heads, int S, int D, const float* rope_cs,
                            __bf16* dqkv, int* err_flag, hipStream_t stream);
int launch_attn_temporal_bwd(const __bf16* q, const __bf16* kv, const __bf16* dO, int B, int P, int D, int T, int Tmax, const float* rope_cs, __bf16* dqkv,
                             int* err_flag, hipStream_t stream);
int launch_adamw_multi(const AdamParam* params, const AdamItem* items, int n_items, const float* ctl, float lr, float beta1, float beta2, float eps, float wd,
                       hipStream_t stream);
void set_error(const char* fmt, ...);     // defined in api.hip: forwards to gtav::set_error (the twin objects report through the same thread-local string)
const char* last_error();
}  // namespace gtav_bf16

namespace gtav {

// One set of launchers per operand type; the signatures are the fp16 ones (the bf16 set casts the 2-byte pointers).
struct OperandOps {
    int (*gemm)(const GemmParams& p, int epi, hipStream_t stream);
    int (*ln_modulate)(float* x, int ldx, f16* out, int ldo, int M, int D, const float* shift, const float* scale, int mod_stride, const int* rows, int rows_per_mod,
                       const LnPending* pend, int* err_flag, hipStream_t stream);
    int (*ln_affine)(float* x, int ldx, f16* out, int ldo, int M, int D, const float* gamma, const float* beta, const LnPending* pend, int* err_flag, hipStream_t stream);
    int (*patchify)(const float* img, const int* frame_index, int NB, int C, int H, int W, int p, f16* out, int ldo, float a, float b, int* err_flag, hipStream_t stream);
    int (*convert_pad)(const float* src, int lds, int R, int C, f16* dst, int Rp, int Cp, float scale, int tiled, hipStream_t stream, int* err_flag);
    int (*unpad)(const f16* src, int lds, int R, int C, float* dst, int tiled, hipStream_t stream);
    int (*attn_spatial)(const f16* Q, const f16* K, const f16* Vt, f16* O, int NB, int heads, int S, hipStream_t stream, bool q_prescaled);
    int (*attn_temporal)(const f16* q, const f16* kv, f16* O, int B, int P, int D, int Tq, int t0, int Tmax, hipStream_t stream);
    bool bf16;
};
const OperandOps& operand_ops(bool bf16);   // api.hip

// The training step's launchers that read or write 2-byte tensors, one set per operand type like OperandOps (the forward's GEMM / LayerNorm / patchify /
// attention launches are OperandOps' own).  The structs GemmParams / GemmDwGroup / AdamParam / AdamItem reach the bf16 set through a reference cast
// (struct_layout.h keeps the two layouts equal).
struct TrainOps {
    int (*gemm_tn)(const GemmParams& p, hipStream_t stream);
    int (*gemm_dw_grouped)(const GemmDwGroup* g, int n, int K, int* err_flag, hipStream_t stream, bool tn);
    int (*transpose_tiled)(const f16* src, int R, int C, f16* dst, hipStream_t stream);
    int (*convert_T)(const float* src, int lds, int R, int C, f16* dst, hipStream_t stream);
    int (*gelu_tiled)(const f16* u, f16* h, size_t n, hipStream_t stream);
    int (*gelu_bwd_tiled)(const f16* dh, const f16* u, f16* du, size_t n, int* err_flag, hipStream_t stream);
    int (*gelu_bwd_tiled_colsum)(const f16* dh, const f16* u, f16* du, int M, int N, float* db, float* ws, int* err_flag, hipStream_t stream);
    int (*gate_bwd)(const float* dres, const float* gate, int mod_stride, int rows_per_mod, int M, int D, f16* dy_tiled, int* err_flag, hipStream_t stream);
    int (*frame_reduce_gate)(const float* dres, const f16* y, int frames, int P, int D, float* dgate, int mod_stride, hipStream_t stream);
    int (*gate_bwd_fused)(const float* dres, const f16* y, const float* gate, int mod_stride, int frames, int P, int D, f16* dy_tiled, float* dgate, float* db,
                          float* ws, int* err_flag, hipStream_t stream);
    int (*colsum_tiled)(const f16* dy, int M, int N, float* db, float* ws, hipStream_t stream);
    int (*to_tiled)(const float* a, int M, int D, f16* out, int* err_flag, hipStream_t stream);
    int (*mse_bwd_patch)(const float* vpred, const float* vtarget, int B, int T, int C, int H, int W, int p, float scale, f16* dfo, int ldf, int* err_flag,
                         hipStream_t stream);
    int (*attn_spatial_bwd)(const f16* Q, const f16* K, const f16* Vt, const f16* dO, int NB, int heads, int S, int D, const float* rope_cs, f16* dqkv,
                            int* err_flag, hipStream_t stream);
    int (*attn_temporal_bwd)(const f16* q, const f16* kv, const f16* dO, int B, int P, int D, int T, int Tmax, const float* rope_cs, f16* dqkv, int* err_flag,
                             hipStream_t stream);
    int (*adamw_multi)(const AdamParam* params, const AdamItem* items, int n_items, const float* ctl, float lr, float beta1, float beta2, float eps, float wd,
                       hipStream_t stream);
    bool bf16;
};
const TrainOps& train_ops(bool bf16);       // api.hip

}  // namespace gtav
