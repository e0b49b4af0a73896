// Launchers of the non-GEMM kernels (all enqueue on `stream`, return 0 on success, never sync).
#pragma once
#include "common.h"
#include "gemm.h"
#include "launch_plan.h"

namespace gtav {

// LnPending, AdamParam / AdamItem and every launcher with an `f16*` or one of those structs in its signature: one text for both operand types
#include "ops_typed.inc"

// ---- skinny.hip --------------------------------------------------------------------------
int launch_skinny_f32(const float* X, int ldx, const float* W, const float* bias, float* Y, int ldy, int M, int N,
                      int K, int act_silu, hipStream_t stream);
// What a launch of problem a[] would run, as gtav_op_launch_plan reports it (include/gtav_amd.h: the kinds, their integers and the twelve outputs): the launcher's
// own validation and plan, no device touched.  One per kernel file; attention.hip and train.hip hold several kinds.
int skinny_launch_plan(const int* a, int* out12);
int ln_launch_plan(const int* a, int* out12);
int attn_launch_plan(int kind, const int* a, int* out12);
int train_launch_plan(int kind, const int* a, int* out12);

// ---- elementwise.hip ---------------------------------------------------------------------
// Per-noise-step scalars of the fused sampler step, kept in device memory so that a captured hipGraph of the
// step can be replayed with new values (written by a one-thread kernel ahead of the graph launch).
struct StepParams {
    int first;      // first frame of the window inside the latent buffer
    int cur;        // frame being denoised
    int t_ctx;      // timestep of the context frames (stabilization level)
    int t_cur;      // timestep of frame `cur`
    int is_final;   // noise_idx == 0: return x_start (train_dit.py:119-120)
    float alpha_t, alpha_next;
    int cond_step;  // >= 0: row set of the per-frame conditioning table prepared by gtav_dit_prepare_frame; -1: inline
    float guidance; // classifier-free guidance scale s of a guided step (gtav_dit_set_guidance): on the device, so one captured step replays for any s
};
// One launch ahead of the (possibly graph-replayed) step: *dst = v, frame_idx[b*Tq+tl] = b*F + (first + tl) % F
// (first = use_cur ? v.cur : v.first) and, when v.cond_step >= 0, the conditioning-table row of every processed frame:
// context frame (b, tl < T-1) -> b*(T-1)+tl, frame `cur` of sample b -> B*(T-1) + cond_step*B + b.
// Guided step (Bc < B, B = 2 Bc internal samples): sample Bc + b is the unconditional twin of sample b — the same frames of x (no copy), and the same row
// numbers over Bc samples plus `uncond_row0`, where the unconditional half of the prepared table starts.  Bc == B: today's numbering, uncond_row0 unused.
int launch_step_setup(StepParams* dst, const StepParams& v, int* frame_idx, int* mod_rows, int* last_rows, int* changed, int B, int Tq, int T, int F,
                      int use_cur, int Bc, int uncond_row0, hipStream_t stream);
// current-step conditioning table: cur[slot] <- table[rows[slot]] (W floats) for the slots step_setup flagged in `changed`
// (table2 / cur2 / W2: optional second table gathered by the same launch — the c1 / c2 tables of the LayerNorm fold)
int launch_gather_rows(const float* table, const int* rows, const int* changed, float* cur, int slots, int W, const float* table2, float* cur2, int W2,
                       hipStream_t stream);
// Conditioning inputs for a whole generated frame (rows laid out as above, n_steps row sets for frame `cur`).  rows_cond < rows (guided: rows = 2 rows_cond):
// row rows_cond + r repeats row r without its actions (zero action columns).
int launch_cond_inputs_frame(int rows, int rows_cond, int B, int T, int F, int start, int cur, int t_ctx, const int* t_steps, const float* sincos,
                             float* E, const float* actions, int A, float* HC, int ldhc, int D, int Apad, int* err_flag,
                             hipStream_t stream);

// Inverse scatter of the projection output.  order 0: features (ph, pw, c) (DiT, model/dit.py:328-341);
// order 1: features (c, ph, pw) (VAE, model/vae.py:279-304).  out (NB, C, H, W) f32 = a * y + b.
int launch_unpatchify(const float* y, int ldy, float* img, int NB, int C, int H, int W, int p, int order, float a,
                      float b, hipStream_t stream);

int launch_copy_f32_strided(const float* src, int lds, int R, int C, float* dst, int ldd, hipStream_t stream);
int launch_copy_rows_f32(const float* src, size_t src_stride, float* dst, size_t dst_stride, int rows, size_t n, hipStream_t stream);
// buf[m][c] = clamp(buf[m][c], lo, hi) for c in [c0, c1)
int launch_clamp_cols(float* buf, int M, int ld, int c0, int c1, float lo, float hi, hipStream_t stream);
int launch_frames_to_u8(const float* img, uint8_t* out, int N, int H, int W, hipStream_t stream);
int launch_moments_to_latents(const float* mom, float* lat, int N, int hw, int latent, int mom_ch, float scale, hipStream_t stream);
int launch_latents_to_tokens(const float* lat, float* z, int N, int hw, int latent, hipStream_t stream);
// Frame ingest: antialiased bilinear resize to (OH, OW) of n frames, either from a uint8 HWC strip (H, n*W, 3) with /255 (ToTensor +
// SplitImages + Resize of the dataset step) or from float NCHW (n, 3, H, W).  dst (n, 3, OH, OW) f32.
int launch_resize_aa(const void* src, int src_is_u8_strip, float* dst, int n, int H, int W, int OH, int OW, hipStream_t stream);
// fp32 strided copy with padding (used to build concatenated fp32 weights): dst[r][c0 + c] = src[r][c]
int launch_copy_f32(const float* src, int lds, int R, int C, float* dst, int ldd, int c0, hipStream_t stream);
int launch_fill_f32(float* dst, size_t n, float v, hipStream_t stream);
// cs[pos][k] = (cos[pos][2k], sin[pos][2k]) for k < 32: the GEMM epilogue's interleaved RoPE table
int launch_rope_interleave(const float* cos_t, const float* sin_t, float* cs, int npos, hipStream_t stream);
int launch_add_f32(const float* a, const float* b, float* out, size_t n, hipStream_t stream);
// timer calibration: one wave spins `ticks` ticks of s_memrealtime (100 MHz) and stores the ticks it really ran in dev_ticks[0]; launched through GTAV_LAUNCH
int launch_calib_spin(unsigned long long ticks, unsigned long long* dev_ticks, hipStream_t stream);
int launch_axpy_f32(float* y, const float* x, float alpha, size_t n, hipStream_t stream);   // y += alpha x (x may alias y)

// Conditioning inputs (model/dit.py:96-118,359-364) for `rows` (b, frame) pairs, row r = (r / Tq, r % Tq):
//   E[r][0:256] = sincos_table[t_r],  t_r = t64 ? t64[r] : (r % Tq == Tq - 1 ? t_cur : t_ctx)   (train_dit.py:64-91)
//   HC[r][D : D+Apad] = actions[(r / Tq) * act_outer + (r % Tq) * act_inner + 0:A]  (zeros when actions == nullptr)
// With `sp` (sampler step): t_ctx / t_cur come from *sp and the action row of (b, tl) is
// actions[b * act_outer + ((use_cur ? sp->cur : sp->first) + tl) * act_inner], the offset inside the sample taken modulo act_outer (ring window).
// Outer indices from `n_cond_outer` on (the unconditional half of a guided step) get zero action columns.
int launch_cond_inputs(const int64_t* t64, int rows, int Tq, const StepParams* sp, int use_cur, const float* sincos /*[1000][256]*/,
                       float* E, const float* actions, int64_t act_outer, int64_t act_inner, int n_cond_outer, int A, float* HC, int ldhc,
                       int D, int Apad, int* err_flag, hipStream_t stream);

// DDIM-style v-prediction update of the newest frame (train_dit.py:110-125), per sample b:
//   x0 = sqrt(a_t) x - sqrt(1 - a_t) v;  eps = (sqrt(1/a_t) x - x0) / sqrt(1/a_t - 1);
//   out = final ? x0 : sqrt(a_n) x0 + sqrt(1 - a_n) eps
// x, v, out: n elements per sample with given sample strides (floats).
int launch_ddim_update(const float* x, size_t x_stride, const float* v, size_t v_stride, float* out, size_t out_stride,
                       int B, int n, const float* alpha_t, const float* alpha_next, int is_final, hipStream_t stream);
// sampler form: frame sp->cur of x (B, F, n) is updated in place from v (row stride v_stride); alphas / is_final from *sp
int launch_ddim_update_step(float* x, size_t frames_per_sample, const float* v, size_t v_stride, int B, int n,
                            const StepParams* sp, hipStream_t stream);
// guided sampler form: v_g = v_c + (s - 1) (v_c - v_u) with s = sp->guidance, as three separately rounded fp32 operations (d = v_c - v_u, m = (s - 1) d,
// v_g = v_c + m: never an fma, so numpy float32 gives the same bits and s = 1 gives v_c itself); frame sp->cur of x is updated from v_g, and v_out
// (B, n; optional) receives v_g.  v_c / v_u: row b at b * v_stride.
int launch_ddim_update_guided_step(float* x, size_t frames_per_sample, const float* v_c, const float* v_u, size_t v_stride, int B, int n,
                                   const StepParams* sp, float* v_out, hipStream_t stream);

// Training-side noising, v-target and squared-error partial sums (train_dit.py:621-650).
int launch_add_noise(const float* x, const float* noise, const float* alpha /*[rows]*/, float* out, int rows, int n,
                     float clamp_abs, hipStream_t stream);
int launch_vtarget(const float* x, const float* noise, const float* alpha /*[rows]*/, float* vt, int rows, int n,
                   float clamp_abs, hipStream_t stream);
int launch_mse(const float* a, size_t a_stride, const float* b, size_t b_stride, int rows, int n, float* out_scalar,
               hipStream_t stream);

// Counter-based noise (DESIGN.md "Noise streams"): Philox4x32-10, key = the two halves of `seed`, counter (element >> 2, slot, sample, draw).  Row r of a call is
// frame slot slot0 + r % slots_per_sample of sample sample0 + r / slots_per_sample.  fp32 only: defined in the fp16 object of elementwise.hip, no bf16 twin.
// n % 4 == 0, rows <= 65535 and 16-byte aligned rows are the callers' to check (api.hip).
struct RngDraw {
    uint64_t seed;
    uint32_t draw, sample0, slot0, slots_per_sample;
};
int launch_rng_bits(uint32_t* out, int rows, int n, const RngDraw& d, hipStream_t stream);                                       // raw words, rows contiguous
// clamp(N(0,1), +-clamp_abs) into rows of n floats; the rows of a sample are contiguous, samples sample_stride floats apart
int launch_rng_normal(float* out, size_t sample_stride, int rows, int n, const RngDraw& d, float clamp_abs, hipStream_t stream);
// launch_add_noise over x (B, W, n) + launch_vtarget of its last slot with the noise of (sample0 + b, slot w) drawn in the launch (d.slot0 = 0, d.slots_per_sample = W)
int launch_noise_window_rng(const float* x, const float* alpha /*[B][W]*/, float* x_noisy, float* v_target /*[B][n]*/, int B, int W, int n, const RngDraw& d,
                            float clamp_abs, hipStream_t stream);
// z (frames, tokens, L) = mean + exp(0.5 clamp(logvar, -30, 20)) N from moments (frames, tokens, 2 L); a row of the stream is one frame
int launch_vae_posterior_sample(const float* moments, float* z, int frames, int tokens, int L, const RngDraw& d, hipStream_t stream);

// ---- train.hip (backward pass + optimizer) ---------------------------------------------
int launch_ln_mod_bwd(const float* dxn, const float* x, const float* scale, int mod_stride, int rows_per_mod, int M, int D, float* dres, int accumulate,
                      float* stats, hipStream_t stream);
int launch_frame_reduce_ln(const float* dxn, const float* x, const float* stats, int frames, int P, int D, float* dshift, float* dscale, int mod_stride,
                           hipStream_t stream);
int gelu_bwd_colsum_splits(int M);
int launch_colsum_reduce_multi(const float* const* ws, float* const* db, const int* splits, const int* N, int njobs, hipStream_t stream);
// launch_ln_mod_bwd + launch_frame_reduce_ln in one pass over dxn and x (M = frames x P rows); ln_bwd_fused_ok: D = 256, 512, 1024 or 2048
bool ln_bwd_fused_ok(int D);
size_t ln_bwd_fused_workspace(int frames, int P, int D);
int launch_ln_mod_bwd_fused(const float* dxn, const float* x, const float* scale, int mod_stride, int frames, int P, int D, float* dres, int accumulate,
                            float* dshift, float* dscale, float* part, hipStream_t stream);
// column sums in a fixed order (no float atomics): ws = colsum_workspace(M, N) floats of scratch for the per-row-split partial sums
size_t colsum_workspace(int M, int N);
int launch_colsum_f32(const float* a, int lda, int M, int N, float* db, float* ws, hipStream_t stream);   // db[n] += sum_m a[m][n]
// per-sample action dropout of the training forward (gtav_dit_train_forward_keep): row m belongs to sample m / rows_per_keep, keep[sample] == 0 = dropped
int launch_colsum_f32_keep(const float* a, int lda, int M, int N, const int* keep, int rows_per_keep, float* db, float* ws, hipStream_t stream);   // db[n] += sum over kept rows
int launch_keep_mask_cols(float* a, int lda, int M, int C, int rows_per_keep, const int* keep, hipStream_t stream);   // a[m][0:C] = 0 in dropped rows
int launch_keep_add_bias(float* y, int ldy, int M, int N, int rows_per_keep, const int* keep, const float* bias_keep, const float* bias_drop, hipStream_t stream);
int launch_silu(const float* x, int ldx, float* y, int ldy, int R, int C, hipStream_t stream);
int launch_silu_bwd(const float* dy, int lddy, const float* x, int ldx, float* dx, int lddx, int R, int C, hipStream_t stream);
int launch_gemm_tn_f32(const float* dY, int lddy, const float* X, int ldx, int R, int N, int K, float* dW, int lddw, hipStream_t stream);   // dW += dY^T X
int launch_gemm_nn_f32(const float* dY, int lddy, const float* W, int ldw, int R, int N, int K, float* dX, int lddx, hipStream_t stream);   // dX = dY W
// dSc [R][D] = dmod [R][MODW] x W_ada [MODW][D].  `part` = workspace of ada_bwd_dx_workspace(MODW, D, R) floats, REQUIRED (nullptr is refused by name): both
// kernels store per-chunk partial sums there and a second launch adds the chunks in a fixed order.  The fp32 MFMA kernel runs where D % 64 == 0, D <= 1024 and
// R <= 80; every other shape takes the VALU kernel.  No atomics on either path.  dSc is overwritten.
size_t ada_bwd_dx_workspace(int MODW, int D, int R);
int launch_ada_bwd_dx(const float* dmod, int MODW, const float* W, int D, int R, float* dSc, float* part, hipStream_t stream);                         // dSc = dmod W_ada
int sumsq_parts(size_t n);                                                         // per-block partial sums written by launch_sumsq
int launch_sumsq(const float* g, size_t n, float* part, hipStream_t stream);
// adds the partial sums in order (ctl[0]); err_flag (optional): ERR_F16_SAT / ERR_NONFINITE in the handle's error word count as overflow
// (step skipped) and are cleared
// Data-parallel training: the overflow decision of the optimizer step must be the SAME on every rank.  A rank whose fp16 gradient stores saturated
// (ERR_F16_SAT / ERR_NONFINITE in its error word) writes +inf into one element `g` of its gradient arena at the end of its backward pass, before the
// gradient all-reduce (SUM): every rank then sees a non-finite norm and skips the step (train.hip clip_coef_kernel).
int launch_overflow_publish(const int* err_flag, float* g, hipStream_t stream);
// clears `bits` of the device error word (stream-ordered)
int launch_err_clear(int* err_flag, int bits, hipStream_t stream);
// Mixed-type training handles (gtav_dit_train_allow_mixed): moves the bits of the per-group error words words[4 .. 4 + n_groups) (stream-ordered) into
// words[dst_word] and, where `sticky` is given, into sticky[g] as well; the group words are cleared.  (sticky, 0) is the fold at the end of a training forward:
// the optimizer's skip decision and launch_overflow_publish see in word 0 what they see on a default handle, and the sticky words remember WHICH group
// saturated until gtav_dit_train_range_words / gtav_dit_train_autorange read them.  (nullptr, 1) is gtav_dit_zero_grad's: bits an inference forward left in
// the group words are not this step's, and wait in word 1 for gtav_dit_check.
int launch_err_fold(int* words, int* sticky, int dst_word, int n_groups, hipStream_t stream);
// ema_decay > 0 (a handle with averaged weights): ctl[7] = the decay of the step being applied, ema_decay or with ema_warmup min(ema_decay, (1 + t) / (10 + t))
int launch_clip_coef(float* ctl, const float* part, int nparts, float inv_scale, float max_norm, float beta1, float beta2, float ema_decay, int ema_warmup,
                     int* err_flag, hipStream_t stream);
// Low-rank adapters (ops_typed.inc launch_lora_grads): the planning of the gradient launches, pure host arithmetic.  The contraction over the M token rows is
// cut into at most LORA_MAX_SPLITS runs of whole 128-row tiles; every run stores a partial [N + K][r] result which a second pass adds in run order.
// Workspace, in floats: t^T and u^T as 2-byte [r][round_up(M, 128)] each (r * round_up(M, 128) floats together), the adapters rounded to the operand type, A^ [r][K]
// and B^^T [r][N] (r (N + K) / 2 floats), then splits x (N + K) x r partial sums.
constexpr int LORA_MAX_SPLITS = 16;
inline bool lora_rank_ok(int r) { return r == 16 || r == 32 || r == 64; }
inline int lora_grads_splits(int M) {
    const int tiles = cdiv(M, 128), s0 = tiles < LORA_MAX_SPLITS ? tiles : LORA_MAX_SPLITS;
    return cdiv(tiles, cdiv(tiles, s0));   // (no run is empty)
}
inline size_t lora_grads_workspace(int M, int N, int K, int r) {
    return (size_t)r * round_up(M, 128) + (size_t)r * (N + K) / 2 + (size_t)lora_grads_splits(M) * (size_t)(N + K) * r;
}
// ... of a handle that serves every M <= Mmax (the run count is not monotonic in M: 16 tiles are 16 runs, 17 tiles 6 runs of 3)
inline size_t lora_grads_workspace_upto(int Mmax, int N, int K, int r) {
    return (size_t)r * round_up(Mmax, 128) + (size_t)r * (N + K) / 2 + (size_t)LORA_MAX_SPLITS * (size_t)(N + K) * r;
}

// ---- attention.hip -----------------------------------------------------------------------
bool attn_spatial_wants_prescaled_q(int S);
constexpr float kAttnQScale = 0.125f * 1.4426950408889634f;   // 1 / sqrt(64) * log2(e)

}  // namespace gtav
