// The non-GEMM declarations that name the operand type `f16`: parameter structs and launcher prototypes, grouped by the source that defines them.  Read like
// gemm_typed.inc (see there): by ops.h inside namespace gtav and by ops_bf16.h inside namespace gtav_bf16; no include guard, no preprocessor directive.

// ---- elementwise.hip ---------------------------------------------------------------------
// LayerNorm fold (gemm.h EPI_*_FOLD): fp16 tile-major X operands [n_groups][Rp][D] of the grouped table GEMM from the fp32 modulation table:
// group g = columns [col[g], col[g] + D) of mod [R][MODW]; is_scale[g] != 0 stores 1 + (scale + 1e-6).  col / is_scale are device arrays.
int launch_ctab_inputs(const float* mod, int MODW, int R, int Rp, int D, const int* col, const int* is_scale, int n_groups, f16* sx, size_t group_stride,
                       hipStream_t stream);

// Deferred residual update executed by the LayerNorm that follows a residual GEMM (model/dit.py:207-223):
//   x[m] += gate[row(m)] * (sum_s parts[s][m] + bias)      (gate == nullptr -> 1, i.e. the VAE's plain residual)
// `parts` are the split-K slabs written by gemm EPI_PARTIAL: slab s at parts + s * slab_stride, rows of ld floats.
struct LnPending {
    const float* parts;
    int nsplit;
    size_t slab_stride;
    int ld;
    const float* bias;
    const float* gate;
    int gate_stride;
    const int* gate_rows;
    int rows_per_gate;
    int flags;   // set by the launcher: bit 0 = residual write-back as sc1 stores, bit 1 = fp16 output as paired 16-byte sc1 stores, bit 2 = row and slabs by non-temporal loads
    int* err_flag;   // device error word (common.h ERR_F16_SAT is raised when the fp16 output saturated); may be null
    // training forward (api_train.hip gtav_dit_train_forward): the backward pass needs every intermediate residual state and every
    // branch output, so the updated row goes to x_out (same leading dimension as x) instead of in place, and the branch output
    // y = sum_s parts[s] + bias (before the gate) is kept as fp16 rows of ld elements in y_save.  Both may be null.
    float* x_out;
    f16* y_save;
    // Row order of the fp16 output (row-block kernel only).  tperm_T > 0: token row m = (b * tperm_T + t) * tperm_P + p is written
    // to row ((b * (tperm_P / 16) + p / 16) * tperm_T + t) * 16 + p % 16 — 16 positions x all frames of the window contiguous, the
    // X-tile order of the fused temporal QKV + attention GEMM (gemm.hip gemm_qkvt_attn_kernel).  0 = identity.
    int tperm_T, tperm_P;
    // Shift K of the one-pass statistics (row-block kernel only; one float per row; both null: K = the row's first element before the pending update).
    // k_save: the launch also stores its K there (needs `parts`).  k_load: the launch reads K from there and has no pending update: a training handle in
    // recompute mode re-runs a block from its stored input state, which already holds the update the forward's launch applied, and gets the forward's
    // bits only with the forward's K and the forward's reduction order (api_train.hip train_rerun_block).
    float* k_save;
    const float* k_load;
};
static_assert(sizeof(LnPending) == 120, "LnPending: every build and both operand types must see the same struct");

// LayerNorm outputs are GEMM A-operands: fp16 TILE-MAJOR with logical row length D (buffer rows padded to 128).
// LayerNorm(eps=1e-6, no affine) + adaLN modulate -> fp16  (model/dit.py:19-27,163-181)
//   out[m] = LN(x[m]) * (1 + (scale[row] + 1e-6)) + shift[row],  row = rows ? rows[m / rows_per_mod] : m / rows_per_mod
// (pend->tperm_T / tperm_P select a permuted OUTPUT row order, see LnPending)
int launch_ln_modulate(float* x, int ldx, f16* out, int ldo, int M, int D, const float* shift, const float* scale,
                       int mod_stride, const int* rows, int rows_per_mod, const LnPending* pend, int* err_flag, hipStream_t stream);
// LayerNorm(eps=1e-6) with affine weight/bias -> fp16   (model/vae.py:139,146,174)
int launch_ln_affine(float* x, int ldx, f16* out, int ldo, int M, int D, const float* gamma, const float* beta,
                     const LnPending* pend, int* err_flag, hipStream_t stream);
// The branch image of a pending update, y[m] = sum_s parts[s][m] + bias as 2-byte rows of ld elements: LnPending::y_save written by a launch of its own, in the
// operand type of the set it is called on, bit for bit what the LayerNorm launch would have kept (mixed-type training handles: api_train.hip train_branch_seam)
int launch_branch_rows(const float* parts, int nsplit, size_t slab_stride, int ld, const float* bias, f16* y, int M, int N, int* err_flag, hipStream_t stream);

// Non-overlapping patch gather (im2col of a k = s = p conv):  img (NB, C, H, W) f32 -> A fp16 TILE-MAJOR, logical [M][ldo],
// token m = (nb, gh, gw), column k = (c, ph, pw); value = a * img + b.  Columns [C p p, ldo) are zeroed.
// `frame_index` (optional, length NB) picks frame f = frame_index[nb] out of the source buffer (frame stride =
// C*H*W floats), which is how the sampler reads its sliding window in place.
int launch_patchify(const float* img, const int* frame_index, int NB, int C, int H, int W, int p, f16* out, int ldo,
                    float a, float b, int* err_flag, hipStream_t stream);

// fp32 -> fp16 with zero padding: src [R][C] (ld = lds) -> dst [Rp][Cp]
// tiled != 0: dst is tile-major (common.h tiled_off) with Rp % 128 == 0, Cp % 64 == 0
// err_flag (optional device word): ERR_F16_SAT is raised when a finite value beyond the operand type's range was clamped
int launch_convert_pad_f16(const float* src, int lds, int R, int C, f16* dst, int Rp, int Cp, float scale, int tiled,
                           hipStream_t stream, int* err_flag = nullptr);
// inverse of the above without padding (state_dict round trip): dst[r][c] = (float)src[r][c]
int launch_unpad_f16_to_f32(const f16* src, int lds, int R, int C, float* dst, int tiled, hipStream_t stream);
// tile-major to_qkv weight [3 D][D] -> head-major row order [head][q 64 | k 64 | v 64] (the fused temporal QKV + attention GEMM's W)
int launch_qkv_head_major(const f16* src, f16* dst, int D, hipStream_t stream, int mode = 0);   // mode 1: the fused spatial kernel's wave-interleaved order (elementwise.hip)

// ---- train.hip (backward pass + optimizer) --------------------------------------------------
// src tile-major logical [R][C] (C % 64 == 0) -> dst tile-major logical [C][round_up(R, 64)], zero K padding
int launch_transpose_tiled_f16(const f16* src, int R, int C, f16* dst, hipStream_t stream);
// fp32 row-major [R][C] -> fp16 tile-major of the transpose, logical [C][round_up(R, 64)] inside [round_up(C, 128)][...]
int launch_convert_T_f16(const float* src, int lds, int R, int C, f16* dst, hipStream_t stream);
int launch_gelu_tiled(const f16* u, f16* h, size_t n, hipStream_t stream);
int launch_gelu_bwd_tiled(const f16* dh, const f16* u, f16* du, size_t n, int* err_flag, hipStream_t stream);
// launch_gelu_bwd_tiled + the column sums of its output (db[n] += sum_m du[m][n]) in one pass
int launch_gelu_bwd_tiled_colsum(const f16* dh, const f16* u, f16* du, int M, int N, float* db, float* ws, int* err_flag, hipStream_t stream);
// db == nullptr in the two fused launchers: the per-split / per-frame partial sums stay in ws and the caller adds them later, several bias gradients per launch
int launch_gate_bwd(const float* dres, const float* gate, int mod_stride, int rows_per_mod, int M, int D, f16* dy_tiled, int* err_flag, hipStream_t stream);
int launch_frame_reduce_gate(const float* dres, const f16* y, int frames, int P, int D, float* dgate, int mod_stride, hipStream_t stream);
// the two above + db[n] += sum_m dy[m][n] in one pass over dres (M = frames x P rows; ws: frames x D floats)
int launch_gate_bwd_fused(const float* dres, const f16* y, const float* gate, int mod_stride, int frames, int P, int D, f16* dy_tiled, float* dgate, float* db,
                          float* ws, int* err_flag, hipStream_t stream);
// ws: colsum_workspace(M, N) floats of scratch (ops.h)
int launch_colsum_tiled_f16(const f16* dy, int M, int N, float* db, float* ws, hipStream_t stream);     // db[n] += sum_m dy[m][n]
int launch_to_tiled_f16(const float* a, int M, int D, f16* out, int* err_flag, hipStream_t stream);
int launch_mse_bwd_patch(const float* vpred, const float* vtarget, int B, int T, int C, int H, int W, int p, float scale, f16* dfo, int ldf, int* err_flag,
                         hipStream_t stream);
int launch_attn_spatial_bwd(const f16* Q, const f16* K, const f16* Vt, const f16* dO, int NB, int heads, int S, int D, const float* rope_cs, f16* dqkv,
                            int* err_flag, hipStream_t stream);
int launch_attn_temporal_bwd(const f16* q, const f16* kv, const f16* dO, int B, int P, int D, int T, int Tmax, const float* rope_cs, f16* dqkv, int* err_flag,
                             hipStream_t stream);
// multi-tensor AdamW: one descriptor per parameter, one work item per 64 x 64 weight tile / 4096-element run (train.hip)
struct AdamParam {
    float* p; int ldp, R, C;               // fp32 master (GEMM weights: contiguous [R][C]; fp32 parameters: in place, leading dimension ldp)
    const float* g; float *m, *v;          // gradient (scaled), AdamW moments, contiguous [R][C]
    float* e;                              // averaged weights (the fp32 shadow, contiguous [R][C] like m and v), or null on a handle without them
    f16* w16; int Cp16;                    // GEMM weights: tile-major fp16 W (logical row length Cp16), else null
    f16* wT; int RpT;                      // tile-major fp16 W^T (logical row length RpT = round_up(R, 64)), or null
};
static_assert(sizeof(AdamParam) == 88, "AdamParam: every build and both operand types must see the same struct");
struct AdamItem { int param; unsigned start; };   // GEMM weight: tile index (row-major over 64 x 64 tiles); fp32 parameter: first element
static_assert(sizeof(AdamItem) == 8, "AdamItem: every build and both operand types must see the same struct");
// ctl [8] floats: [0] sum of squares of the scaled gradients, [1] step coefficient (0 = step skipped), [2] skipped steps, [3] unscaled gradient
// norm, [4] applied steps (the Adam step count), [5] / [6] bias corrections of the step being applied (written by clip_coef on the device),
// [7] decay of the averaged weights for the step being applied (handles with a shadow only)
int launch_adamw_multi(const AdamParam* params, const AdamItem* items, int n_items, const float* ctl, float lr, float beta1, float beta2, float eps, float wd,
                       hipStream_t stream);
// the same step, then e = fmaf(ctl[7], e, (1 - ctl[7]) * w_new) on every element's shadow (AdamParam::e, not null) in the same launch; a skipped step leaves it alone
int launch_adamw_multi_ema(const AdamParam* params, const AdamItem* items, int n_items, const float* ctl, float lr, float beta1, float beta2, float eps, float wd,
                           hipStream_t stream);
// no step: w <-> e on every element, both 2-byte images of the GEMM weights rewritten from the new w as the step writes them
int launch_adamw_swap_ema(const AdamParam* params, const AdamItem* items, int n_items, hipStream_t stream);
// Low-rank adapters (train.hip, DESIGN.md 7 "Low-rank adapters"): W = W0 + s B A for every adapted Linear, one work item per 64 x 64 tile of W (N, K % 64 == 0).
struct LoraMergeParam {
    const float* w0; const float* a; const float* b;   // frozen fp32 master [N][K], A [r][K], B [N][r]
    int N, K, r; float s;
    f16* w16; int Cp16;                    // tile-major 2-byte W (logical row length Cp16)
    f16* wT; int RpT;                      // tile-major 2-byte W^T (logical row length RpT = round_up(N, 64)), or null
    float* w32;                            // launch_lora_merge_one(export_f32): the fp32 sum itself, contiguous [N][K]
};
static_assert(sizeof(LoraMergeParam) == 80, "LoraMergeParam: every build and both operand types must see the same struct");
struct LoraMergeItem { int param; unsigned tile; };   // tile index, row-major over 64 x 64 tiles
static_assert(sizeof(LoraMergeItem) == 8, "LoraMergeItem: every build and both operand types must see the same struct");
// (f16)clamp(W0 + s B A) into both images of every item's tile / the fp32 sum into w32: one device function, the same fp32 value (train.hip has the contract)
int launch_lora_merge(const LoraMergeParam* params, const LoraMergeItem* items, int n_items, hipStream_t stream);
// one Linear by value: its two images (export_f32 == 0) or the fp32 sum into P.w32
int launch_lora_merge_one(const LoraMergeParam& P, int export_f32, hipStream_t stream);
// dB [N][r] += s dY^T (X A^T), dA [r][K] += s (dY B)^T X over the M token rows of the tile-major X [M][K], dY [M][N] (pad rows up to 128 are never used);
// ws: lora_grads_workspace(M, N, K, r) floats (ops.h).  Fixed-order sums, no atomics; err_flag: ERR_F16_SAT when t = X A^T or u = dY B saturated.
int launch_lora_grads(const f16* X, const f16* dY, const float* A, const float* B, int M, int N, int K, int r, float s, float* dA, float* dB, float* ws,
                      size_t ws_floats, int* err_flag, hipStream_t stream);

// ---- attention.hip -----------------------------------------------------------------------
// Full (non-causal) attention over S tokens per (nb, head), head_dim 64 (model/attention.py:127-129, model/vae.py:101).
// Q,K [nb][heads][S][64], Vt [nb][heads][64][S] fp16 (layouts written by the QKV GEMM epilogue);
// O logical [nb*S][heads*64] fp16, TILE-MAJOR (A-operand of the out-projection GEMM).
// q_prescaled: Q already carries the softmax scale in the exponent's unit, q / 8 * log2 e (written that way by the to_qkv epilogue through
// GemmParams::rope_cs_q); only sequences that run the flash kernel take it — attn_spatial_wants_prescaled_q(S) says which
int launch_attn_spatial(const f16* Q, const f16* K, const f16* Vt, f16* O, int NB, int heads, int S, hipStream_t stream, bool q_prescaled = false);
// Causal attention over the frames of a window per (b, p, head) (model/attention.py:62-64).
// q [B*Tq*P][D] row-major for frames t0 .. t0+Tq-1; kv cache [B][Tmax][P][2][D]; O logical like q but TILE-MAJOR.
int launch_attn_temporal(const f16* q, const f16* kv, f16* O, int B, int P, int D, int Tq, int t0, int Tmax,
                         hipStream_t stream);
