/* gtav_amd — test hooks of libgtav_amd.so.  NOT part of the product interface (include/gtav_amd.h): nothing in a binding of the
 * reference's API needs them.  tests/ use them to run every GEMM block shape the launch heuristic can pick through every epilogue.
 *
 * All settings are PER THREAD (thread_local in csrc/gemm_plan.hip, one set for both operand types), like the handles: forcing a shape on one thread never
 * changes what another thread's handle launches.  Every choice computes the same result.  0 restores the heuristic.
 *   gtav_op_gemm_set_stages   LDS ring depth of the 128 x 128 tiles: 2 or 4
 *   gtav_op_gemm_set_wm       block shape, an id of the shape table GEMM_SHAPES in csrc/gemm_plan.h — the ONE place where a shape's tile, waves and ring are
 *                             defined; gtav_op_gemm_plan (gtav_amd.h) reports them, and tests/test_host_gemm_plan.py holds this list against the table:
 *                                id   features x tokens   compute [+ loader] waves
 *     2     128 x 128     4 waves
 *     3     128 x 128     8 waves
 *     7     256 x 256     8 waves
 *     11    64 x 48       6 waves
 *     12    128 x 192     8 waves
 *     13    128 x 96      4 waves
 *     14    64 x 96       6 waves
 *     20    128 x 96      8 + 4 waves   (loader-wave kernel, as 24 / 26 / 29)
 *     24    64 x 48       6 + 2 waves
 *     26    64 x 96       6 + 2 waves
 *     29    128 x 144     12 + 4 waves
 *     31    128 x 192     8 + 4 waves   (persistent loader-wave kernel, 3-stage ring; its 4-stage / 256 x 128 / 128 x 256 forms 30 / 32 / 33 and the
 *                             other laboratory shapes exist in the experiments build only: a product library refuses them by name)
 *                             Plus GTAV_GEMM_WM_NT_WEIGHT_FILLS (0x100; with a shape or with 0 = heuristic): every loader-wave
 *                             launch of the thread (shapes 20 / 24 / 26 / 29 and the two fused to_qkv + attention launches) fills its weight operand with the
 *                             non-temporal cache policy (GemmParams::wfill, the kernel side of gtav_dit_set_weight_fill_policy): the same bits again
 *                             (tests/test_gpu_launch_head.py)
 *
 * gtav_op_set_operand_dtype   operand type of the kernel-level entry points (gtav_op_*) that have no _bf16 sibling: GTAV_OPERAND_F16 (0, the default) or
 *                             GTAV_OPERAND_BF16 (1), PER THREAD like the two above.  With bf16 set, gtav_op_gemm_f16, gtav_op_gemm_qkv, gtav_op_ln_modulate,
 *                             gtav_op_ln_affine, gtav_op_attn_spatial[_prescaled], gtav_op_gemm_tn, gtav_op_gemm_dw_grouped, gtav_op_gemm_splitk_ln and
 *                             gtav_op_convert_f16 launch the bf16 twins (the objects a bf16 layer group of a handle runs) and every 2-byte buffer they read or
 *                             write holds bf16.  Entry points with a _bf16 sibling (attn_temporal, attn_spatial_bwd, attn_temporal_bwd) keep their fixed type, the
 *                             type-free ones (skinny_f32, rope_interleave, the elementwise math) are unaffected, and the fused fp16-only launches
 *                             (gtav_op_gemm_qkvt_attn, gtav_op_gemm_qkvs_attn, gtav_op_qkv_head_major[_spatial]) refuse by name.  At the default every entry point
 *                             launches what it launched before the hook existed.  gtav_op_gemm_set_stages / _set_wm set the forced shape of BOTH operand types.
 * gtav_op_attn_spatial_prescaled   gtav_op_attn_spatial on a q that already carries 1/8 log2 e (the form the VAE's flash attention runs, GemmParams::rope_cs_q);
 *                             refused at the sequence lengths whose kernel takes plain q.  Honours the operand type above.
 * tests/test_gpu_ops_typed.py runs every one of these in both operand types against fp64 math with per-element bounds.
 *
 * gtav_op_train_*             the backward-only kernels of the training step (csrc/train.hip), each a thin call of the launcher(s) a training handle runs.  The 2-byte
 *                             ones dispatch per gtav_op_set_operand_dtype like gtav_op_gemm_tn (with bf16 set, every 2-byte buffer holds bf16); the fp32 conditioning
 *                             path (colsum_f32, colsum_reduce_multi, silu, silu_bwd, gemm_tn_f32, gemm_nn_f32, ada_bwd_dx) ignores it.  The caller owns EVERY
 *                             buffer — workspaces and the device error word `err` (may be null) included; a hook allocates nothing and never synchronises.  A
 *                             workspace comes with its size in floats and the hook refuses by name when the launcher's own *_workspace / *_splits function asks
 *                             for more.  `fused` picks between the one-pass launch a handle normally runs (1) and the separate launches it replaces (0):
 *   ln_mod_bwd            1: launch_ln_mod_bwd_fused (D = 256 / 512 / 1024 / 2048, ws = ln_bwd_fused_workspace(frames, P, D));  0: launch_ln_mod_bwd +
 *                             launch_frame_reduce_ln (any D % 4 == 0 up to 2048, ws = the 2 frames P floats of row statistics)
 *   gate_bwd              1: launch_gate_bwd_fused (ws = frames x D; db null leaves the per-frame bias partial sums in ws for colsum_reduce_multi);
 *                             0: launch_gate_bwd + launch_frame_reduce_gate + launch_colsum_tiled_f16 (ws = colsum_workspace(frames P, D), db required)
 *   gelu_bwd              1: launch_gelu_bwd_tiled_colsum (ws = gelu_bwd_colsum_splits(M) x N; db null leaves the per-split partial sums in ws);
 *                             0: launch_gelu_bwd_tiled over the whole 128-row-padded image + launch_colsum_tiled_f16 (ws = colsum_workspace(M, N), db required)
 *   colsum_tiled, colsum_f32   db[n] += column sums (ws = colsum_workspace(M, N));  colsum_reduce_multi: 1 .. 4 jobs, host arrays of device pointers
 *   mse_bwd_patch, to_tiled, transpose_tiled, convert_t (launch_convert_T_f16)   the loss gradient and the layout converters
 *   silu, silu_bwd, gemm_tn_f32 (dW += dY^T X), gemm_nn_f32 (dX = dY W), ada_bwd_dx (part = ada_bwd_dx_workspace(MODW, D, R))
 * tests/test_gpu_ops_train.py runs them against fp64 math with the bounds of tests/parity_bounds.py.
 *   attn_spatial_bwd, attn_temporal_bwd   launch_attn_spatial_bwd / launch_attn_temporal_bwd as a training handle makes them: the arguments of
 *                             gtav_op_attn_spatial_bwd / gtav_op_attn_temporal_bwd (gtav_amd.h), which run "without an error word", plus the caller's `err`, in the
 *                             thread's operand type.  The resident and the streaming kernel of each are chosen by the launcher (S <= 160 with S % 16 == 0; T <= 8).
 *                             On fp16 operands a dS, dq, dk or dv beyond 65504 is stored clamped and raises ERR_F16_SAT (2) in `err` — the bit on which a training
 *                             step skips its optimizer step; bf16 operands never raise it.  tests/test_gpu_ops_attn_bwd_bounds.py holds every output element to the
 *                             derived bounds of tests/parity_bounds.py on flat AND peaked softmax rows, and the bit.
 *   sumsq_parts, sumsq, clip_coef, adamw_multi, overflow_publish   the optimizer step as gtav_dit_adamw_step launches it: launch_sumsq (part = sumsq_parts(n) floats, its
 *                             size in part_floats, refused by name when short), launch_clip_coef (ctl = the caller's 8 device floats of csrc/ops_typed.inc: the hook
 *                             reads ctl[2], ctl[4] and writes ctl[0 .. 7] as the kernel does; err may be null), launch_overflow_publish, and
 *   adamw_multi               mode 0 / 1 / 2 = launch_adamw_multi / _multi_ema / _swap_ema in the thread's operand type, over n_params parameters given as HOST arrays
 *                             of n_params entries each: p, ldp, R, C (the fp32 master and its leading dimension), g, m, v, e (contiguous [R][C]; e may hold nulls in
 *                             mode 0), w16, Cp16, wT, RpT (the two 2-byte images of a GEMM weight: w16 null = an fp32 parameter trained in place, wT null = no
 *                             transposed image).  The work items — one per 64 x 64 tile of a GEMM weight, one per 4096-element run of an fp32 parameter — are cut by
 *                             the function gtav_dit_train_enable cuts them with (csrc/api_internal.h adam_plan_items).  `desc` is a caller-owned DEVICE buffer of
 *                             desc_bytes for the AdamParam [n_params] and AdamItem [items] tables (88 and 8 bytes each), refused by name when too small.  Unlike every
 *                             other hook this one SYNCHRONISES: it fills `desc` with two blocking hipMemcpy, as gtav_dit_train_enable fills the handle's tables.
 *                             It validates nothing else: pointers, shapes and alignment (16-byte rows for a GEMM weight with C % 4 == 0) are the caller's.
 *                             A documented property of the design: clip_coef computes the bias corrections ctl[5] / ctl[6] = 1 - powf(beta, t) in fp32, so at small t
 *                             they inherit the cancellation — |ctl[5 | 6] - (1 - beta^t)| <= 2 ulp(beta^t) + 2^-24 (1 - beta^t), which at beta2 = 0.999 and t = 2, 3 is
 *                             about 2000 x 2^-24 of the correction and half of that on the update; below 8 x 2^-24 from t = 1000 on.
 *                             tests/test_gpu_ops_optimizer.py holds, in both operand types and between NaN guard words: every element of w, m, v (and the shadow e)
 *                             to a derived bound against fp64 AdamW (tests/parity_bounds.py, last section) at t = 1, 2, 3, 1000 and 100000; exact zeros; BOTH images,
 *                             pads included, bit for bit equal to gtav_op_convert_f16 / gtav_op_train_convert_t of the master the launch wrote; a skipped step and a
 *                             swap writing exactly what they should; equal bits from the kernel's three code paths; the sum of squares, every field of clip_coef, and
 *                             the published overflow.
 *
 * gtav_op_ln_pending          ONE launch_ln_modulate (mode 0: p0 = shift, p1 = scale tables of row length mod_stride, indexed by rows / rows_per_mod) or
 *                             launch_ln_affine (mode 1: p0 = gamma, p1 = beta; rows, rows_per_mod and mod_stride unused) with a deferred residual update
 *                             (csrc/ops_typed.inc LnPending) whose EVERY field is an argument: parts .. k_load.  x has the leading dimension ldx, out is the
 *                             tile-major 2-byte operand of row length D.  Dispatches per gtav_op_set_operand_dtype (out and y_save then hold bf16).
 * gtav_op_branch_rows         launch_branch_rows, the launch of its own that writes what LnPending::y_save keeps, in the thread's operand type.
 *                             Both: the caller owns every buffer and the device error word `err` (may be null); the hooks allocate nothing, never synchronise and
 *                             validate NOTHING themselves — a bad descriptor meets the launchers' own refusals, which is what tests/test_gpu_ops_ln_pending.py
 *                             holds, next to the fp64 references and bounds of tests/parity_bounds.py.
 * (Timing experiments that change results, and the block shapes that measured slower than these, exist only in the separate
 * -DGTAV_EXPERIMENTS build: csrc/build.sh exp -> libgtav_amd_exp.so, loaded by tools/ only.) */
#ifndef GTAV_AMD_TESTING_H
#define GTAV_AMD_TESTING_H

#include <stdint.h>

#define GTAV_GEMM_WM_NT_WEIGHT_FILLS 0x100

#ifdef __cplusplus
extern "C" {
#endif

void gtav_op_gemm_set_stages(int32_t ns);
void gtav_op_gemm_set_wm(int32_t wm);
void gtav_op_set_operand_dtype(int32_t dtype);   /* GTAV_OPERAND_F16 (default) / GTAV_OPERAND_BF16, per thread */
int gtav_op_attn_spatial_prescaled(const void* q, const void* k, const void* vt, void* o, int32_t NB, int32_t heads, int32_t S, void* stream);

/* ---- backward-only training kernels (see above); M = frames x P token rows, 2-byte buffers in the thread's operand type ---- */
int gtav_op_train_ln_mod_bwd(int32_t fused, const float* dxn, const float* x, const float* scale, int32_t mod_stride, int32_t frames, int32_t P, int32_t D,
                             float* dres, int32_t accumulate, float* dshift, float* dscale, float* ws, int64_t ws_floats, void* stream);
int gtav_op_train_gate_bwd(int32_t fused, const float* dres, const void* y, const float* gate, int32_t mod_stride, int32_t frames, int32_t P, int32_t D,
                           void* dy_tiled, float* dgate, float* db, float* ws, int64_t ws_floats, int32_t* err, void* stream);
int gtav_op_train_gelu_bwd(int32_t fused, const void* dh, const void* u, void* du, int32_t M, int32_t N, float* db, float* ws, int64_t ws_floats, int32_t* err,
                           void* stream);
int gtav_op_train_colsum_tiled(const void* dy, int32_t M, int32_t N, float* db, float* ws, int64_t ws_floats, void* stream);
int gtav_op_train_colsum_f32(const float* a, int32_t lda, int32_t M, int32_t N, float* db, float* ws, int64_t ws_floats, void* stream);
int gtav_op_train_colsum_reduce_multi(const float* const* ws, float* const* db, const int32_t* splits, const int32_t* N, int32_t njobs, void* stream);
int gtav_op_train_mse_bwd_patch(const float* vpred, const float* vtarget, int32_t B, int32_t T, int32_t C, int32_t H, int32_t W, int32_t p, float scale, void* dfo,
                                int32_t ldf, int32_t* err, void* stream);
int gtav_op_train_to_tiled(const float* a, int32_t M, int32_t D, void* out, int32_t* err, void* stream);
int gtav_op_train_transpose_tiled(const void* src, int32_t R, int32_t C, void* dst, void* stream);
int gtav_op_train_convert_t(const float* src, int32_t lds, int32_t R, int32_t C, void* dst, void* stream);
int gtav_op_train_silu(const float* x, int32_t ldx, float* y, int32_t ldy, int32_t R, int32_t C, void* stream);
int gtav_op_train_silu_bwd(const float* dy, int32_t lddy, const float* x, int32_t ldx, float* dx, int32_t lddx, int32_t R, int32_t C, void* stream);
int gtav_op_train_gemm_tn_f32(const float* dY, int32_t lddy, const float* X, int32_t ldx, int32_t R, int32_t N, int32_t K, float* dW, int32_t lddw, void* stream);
int gtav_op_train_gemm_nn_f32(const float* dY, int32_t lddy, const float* W, int32_t ldw, int32_t R, int32_t N, int32_t K, float* dX, int32_t lddx, void* stream);
int gtav_op_train_ada_bwd_dx(const float* dmod, int32_t MODW, const float* W, int32_t D, int32_t R, float* dSc, float* part, int64_t part_floats, void* stream);
int gtav_op_train_attn_spatial_bwd(const void* q, const void* k, const void* vt, const void* d_o, int32_t NB, int32_t heads, int32_t S, const float* rope_cs,
                                   void* dqkv, int32_t* err, void* stream);
int gtav_op_train_attn_temporal_bwd(const void* q, const void* kv, const void* d_o, int32_t B, int32_t P, int32_t D, int32_t T, int32_t Tmax, const float* rope_cs,
                                    void* dqkv, int32_t* err, void* stream);

/* ---- the optimizer step (see above); host arrays of n_params entries, desc / ctl / part on the device ---- */
int gtav_op_train_sumsq_parts(int64_t n);
int gtav_op_train_sumsq(const float* g, int64_t n, float* part, int64_t part_floats, void* stream);
int gtav_op_train_clip_coef(float* ctl, const float* part, int32_t nparts, float inv_scale, float max_norm, float beta1, float beta2, float ema_decay,
                            int32_t ema_warmup, int32_t* err, void* stream);
int gtav_op_train_adamw_multi(int32_t mode, int32_t n_params, float* const* p, const int32_t* ldp, const int32_t* R, const int32_t* C, const float* const* g,
                              float* const* m, float* const* v, float* const* e, void* const* w16, const int32_t* Cp16, void* const* wT, const int32_t* RpT,
                              void* desc, int64_t desc_bytes, const float* ctl, float lr, float beta1, float beta2, float eps, float wd, void* stream);
int gtav_op_train_overflow_publish(const int32_t* err, float* g, void* stream);

/* ---- the deferred-residual LayerNorm (see above) ---- */
int gtav_op_ln_pending(int32_t mode, float* x, int32_t ldx, void* out, int32_t M, int32_t D, const float* p0, const float* p1, int32_t mod_stride,
                       const int32_t* rows, int32_t rows_per_mod, const float* parts, int32_t nsplit, int64_t slab_stride, int32_t ld, const float* bias,
                       const float* gate, int32_t gate_stride, const int32_t* gate_rows, int32_t rows_per_gate, float* x_out, void* y_save, int32_t tperm_T,
                       int32_t tperm_P, float* k_save, const float* k_load, int32_t* err, void* stream);
int gtav_op_branch_rows(const float* parts, int32_t nsplit, int64_t slab_stride, int32_t ld, const float* bias, void* y, int32_t M, int32_t N, int32_t* err,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GTAV_AMD_TESTING_H */
