// Big-M fp16 MFMA GEMM with fused epilogues:  Y[m][n] = sum_k X[m][k] * W[n][k]  (+ epilogue)
// X (activations, logical [M][K]) and W (torch-Linear [N][K]) are both fp16 in the TILE-MAJOR layout of
// common.h `tiled_off` (rows padded to 128, K to 64).  fp16 outputs that feed another GEMM are written tile-major too.
#pragma once
#include "common.h"
#include "gemm_plan.h"

namespace gtav {

enum GemmEpi : int {
    EPI_F32 = 0,        // out_f32[m][n] = acc + bias
    EPI_F16 = 1,        // out_f16[m][n] = acc + bias
    EPI_GELU_TANH = 2,  // out_f16[m][n] = gelu_tanh(acc + bias)   (DiT Mlp, model/dit.py:161)
    EPI_GELU_ERF = 3,   // out_f16[m][n] = gelu_erf(acc + bias)    (VAE Mlp, model/vae.py:128)
    EPI_RESID = 4,      // resid_f32[m][n] += gate[row(m)][n] * (acc + bias)   (model/dit.py:207-223)
    EPI_QKV = 5,        // bias, RoPE on q/k, scatter to attention layouts (model/attention.py:50-58,109-118)
    EPI_PARTIAL = 6,    // split-K: out_f32[ks][m][n] = raw partial sums (no bias); the following LayerNorm kernel
                        // reduces the slabs and applies bias + gate + residual (ops.h: LnPending)
    EPI_F16_TILED = 7,  // out_f16 = acc + bias, TILE-MAJOR like the GELU epilogues (no activation): training keeps the MLP's
                        // pre-activation, and the backward pass's activation gradients are GEMM operands themselves
    // ---- LayerNorm fold (docs/LABNOTES.md 4.7): the LayerNorm + adaLN modulate between a residual GEMM and the GEMM that consumes its
    // output is split over the two epilogues instead of being a launch of its own (model/dit.py:19-27,200-225) ----
    EPI_RESID_FOLD = 8,      // producer (out-proj, fc2; full K): x = resid[m][n] += gate (acc + bias) in place, AND the next GEMM's operand
                             // A[m][n] = fp16(x (1 + scale_next + 1e-6)) tile-major, AND per-row partial sums (sum x, sum x^2) per 64-feature slot
    EPI_QKV_FOLD = 9,        // consumers: X = A; y = (acc - mean c1[frame][n]) rstd + c2[frame][n], then as EPI_QKV / EPI_GELU_TANH / EPI_F32
    EPI_GELU_TANH_FOLD = 10, //   with mean / rstd from the producer's partial sums and c1 = sum_k (1 + scale_k) W[n][k],
    EPI_F32_FOLD = 11,       //   c2 = sum_k shift_k W[n][k] + bias[n] from the per-frame tables (gemm_grouped: one launch per forward)
};
constexpr bool epi_is_fold_consumer(int e) { return e == EPI_QKV_FOLD || e == EPI_GELU_TANH_FOLD || e == EPI_F32_FOLD; }
constexpr int epi_base(int e) { return e == EPI_QKV_FOLD ? EPI_QKV : e == EPI_GELU_TANH_FOLD ? EPI_GELU_TANH : e == EPI_F32_FOLD ? EPI_F32 : e; }

enum QkvMode : int {
    QKV_SPATIAL = 0,   // Q,K -> [nb][head][S][64], V -> Vt [nb][head][64][S]   (nb = m / S)
    QKV_TEMPORAL = 1,  // q -> [m][D]; k,v -> kv cache [b][Tmax][P][2][D]
};

constexpr int GEMM_SK_MAX_SPLIT = 128;   // split tiles per launch (half the CUs)
constexpr size_t gemm_sk_ws_bytes() { return (size_t)GEMM_SK_MAX_SPLIT * 256 * 256 * 4; }
constexpr size_t gemm_sk_flag_bytes() { return (size_t)GEMM_SK_MAX_SPLIT * 4; }

// GemmParams, GemmGroup, GemmDwGroup and the launchers that take them: the declarations that name `f16` (one text for both operand types)
#include "gemm_typed.inc"
// Which block shape a launch runs on, its K slices and tile-group width: the planner (gemm_plan.h, namespace gtav_shared — ONE copy for both operand types).
using gtav_shared::gemm_pp_ok, gtav_shared::gemm_resid_inplace_ok, gtav_shared::gemm_choose_splitk;
#ifdef GTAV_EXPERIMENTS
// per-block timeline: 8 x u64 per block {s_memtime at entry, first K-tile landed, main loop done, epilogue done (end);
// s_memrealtime at entry and end (100 MHz); XCC id; 0}; buf must hold 8 * grid u64 (null switches it off)
void gemm_set_stamps(unsigned long long* buf, int max_blocks);
#endif

}  // namespace gtav
