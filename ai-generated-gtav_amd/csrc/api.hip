// C-ABI of gtav_amd (see include/gtav_amd.h): handles own repacked weights + workspace in HBM and
// enqueue the kernel sequence of each reference entry point on the caller's stream.
#include "api_internal.h"

#include <type_traits>

namespace gtav_shared {   // common.h: shared by the fp16 objects and their bf16 twins
thread_local hipEvent_t g_launch_ev[2] = {nullptr, nullptr};   // GTAV_LAUNCH: the profiler's event pair for the next launch of this thread
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }
}  // namespace gtav_shared

// ---- the two sets of launchers (ops_bf16.h GTAV_OPERAND_OPS): fp16 operands (default) and their bf16 twins ----
namespace {
// The type the twin declares where the fp16 signature has T: 2-byte pointers and the parameter structs that name `f16` change namespace, the rest is itself.
template <class T> struct twin_arg { typedef T type; };
template <> struct twin_arg<const f16*> { typedef const __bf16* type; };
template <> struct twin_arg<f16*> { typedef __bf16* type; };
// The two views of a struct are one text (gemm_typed.inc / ops_typed.inc) that differs in the pointee of 2-byte pointers only; checked here all the same.
#define GTAV_TWIN_STRUCT(S)                                                                                                                     \
    static_assert(sizeof(S) == sizeof(gtav_bf16::S) && alignof(S) == alignof(gtav_bf16::S) && std::is_standard_layout<S>::value &&             \
                      std::is_standard_layout<gtav_bf16::S>::value, #S ": the fp16 and the bf16 view differ");                                  \
    template <> struct twin_arg<const S&> { typedef const gtav_bf16::S& type; };                                                                \
    template <> struct twin_arg<const S*> { typedef const gtav_bf16::S* type; };
GTAV_TWIN_STRUCT(GemmParams)
GTAV_TWIN_STRUCT(LnPending)
GTAV_TWIN_STRUCT(GemmDwGroup)
GTAV_TWIN_STRUCT(AdamParam)
GTAV_TWIN_STRUCT(AdamItem)
GTAV_TWIN_STRUCT(LoraMergeParam)
GTAV_TWIN_STRUCT(LoraMergeItem)
#undef GTAV_TWIN_STRUCT
// twin_call<fp16 signature, twin's signature, twin>::call has the fp16 signature and calls the twin with every argument cast to the type the twin declares.
// A twin whose signature is not the mapped fp16 one does not compile.
template <class Sig, class TwinSig, TwinSig* Fn> struct twin_call;
template <class... A, class... B, int (*Fn)(B...)> struct twin_call<int(A...), int(B...), Fn> {
    static_assert((std::is_same<typename twin_arg<A>::type, B>::value && ...), "a bf16 twin's signature differs from its fp16 launcher's");
    template <class To, class From> static To cast(From a) {
        if constexpr (std::is_same<To, From>::value) return a;
        else return reinterpret_cast<To>(a);
    }
    static int call(A... a) { return Fn(cast<B, A>(a)...); }
};
#define GTAV_OPS_F16(field, launcher) &launcher,
#define GTAV_OPS_BF16(field, launcher) &twin_call<decltype(launcher), decltype(gtav_bf16::launcher), &gtav_bf16::launcher>::call,
const OperandOps OPS_F16 = {GTAV_OPERAND_OPS(GTAV_OPS_F16) false};
const OperandOps OPS_BF16 = {GTAV_OPERAND_OPS(GTAV_OPS_BF16) true};
#undef GTAV_OPS_F16
#undef GTAV_OPS_BF16
}  // namespace
const OperandOps& gtav::operand_ops(bool bf16) { return bf16 ? OPS_BF16 : OPS_F16; }

// Operand type of the kernel-level entry points below that have no _bf16 sibling (include/gtav_amd_testing.h gtav_op_set_operand_dtype): per thread, fp16 unless
// a test says otherwise.  op_ops() is the set of launchers they dispatch through; the fp16 set holds the launchers they called directly before the hook existed.
static thread_local bool g_op_bf16 = false;
static const OperandOps& op_ops() { return operand_ops(g_op_bf16); }
// the fused launches exist for fp16 operands only (the handle never runs them on a bf16 layer group)
#define GTAV_OP_F16_ONLY(name) GTAV_REQUIRE(!g_op_bf16, name ": fp16 operands only, there is no bf16 twin of this launch (gtav_op_set_operand_dtype)")

extern "C" {

const char* gtav_last_error(void) { return last_error(); }
int gtav_abi_version(void) { return 4; }   // 3: training step (gtav_dit_train_*), collectives (gtav_comm_*); 4: LayerNorm fold switch, optimizer state (gtav_dit_{get,set}_opt_state)

// ------------------------------------------------------------------------------------------------
// elementwise entry points
// ------------------------------------------------------------------------------------------------
int gtav_clamp_frames(float* x, int32_t B, int32_t F, int32_t first, int32_t n, float lo, float hi, void* stream) {
    GTAV_REQUIRE(x && B >= 1 && first >= 0 && first <= F && n >= 1, "clamp_frames: bad arguments");
    if (first == F) return 0;
    GTAV_REQUIRE((int64_t)F * n < (int64_t)1 << 31, "clamp_frames: sample of %d x %d floats too large", F, n);
    return launch_clamp_cols(x, B, F * n, first * n, F * n, lo, hi, (hipStream_t)stream);
}
int gtav_ddim_update(const float* x, const float* v, float* out, int32_t rows, int32_t n, const float* alpha_t,
                     const float* alpha_next, int32_t is_final, void* stream) {
    GTAV_REQUIRE(x && v && out && alpha_t && (alpha_next || is_final), "ddim_update: null argument");
    return launch_ddim_update(x, n, v, n, out, n, rows, n, alpha_t, alpha_next, is_final, (hipStream_t)stream);
}
int gtav_add_noise(const float* x, const float* noise, const float* alpha, float* out, int32_t rows, int32_t n, float clamp_abs,
                   void* stream) {
    return launch_add_noise(x, noise, alpha, out, rows, n, clamp_abs, (hipStream_t)stream);
}
int gtav_vtarget(const float* x, const float* noise, const float* alpha, float* vt, int32_t rows, int32_t n, float clamp_abs,
                 void* stream) {
    return launch_vtarget(x, noise, alpha, vt, rows, n, clamp_abs, (hipStream_t)stream);
}
// ---- counter-based noise (DESIGN.md "Noise streams"): everything is validated before a launch, a bad call touches no device ----
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// rows of n floats on grid.y, four elements per thread
#define GTAV_RNG_ROWS(name, rows, n)                                                                                                    \
    GTAV_REQUIRE((n) >= 4 && (n) % 4 == 0, name ": a row of %d floats (a multiple of 4: one generator call makes four elements)", (int)(n)); \
    GTAV_REQUIRE((rows) >= 1 && (rows) <= 65535, name ": %d rows (1 .. 65535)", (int)(rows))
int gtav_rng_normal(float* out, int64_t sample_stride, int32_t rows, int32_t n, uint64_t seed, uint32_t draw, uint32_t sample0, uint32_t slot0,
                    uint32_t slots_per_sample, float clamp_abs, void* stream) {
    GTAV_REQUIRE(out, "rng_normal: null pointer");
    GTAV_RNG_ROWS("rng_normal", rows, n);
    GTAV_REQUIRE(slots_per_sample >= 1, "rng_normal: slots_per_sample 0");
    GTAV_REQUIRE(clamp_abs >= 0.0f, "rng_normal: clamp_abs %g (>= 0; infinity for no clamp)", (double)clamp_abs);
    GTAV_REQUIRE(aligned16(out) && sample_stride >= 0 && sample_stride % 4 == 0, "rng_normal: out and sample_stride (%lld floats) must keep every row 16-byte aligned",
                 (long long)sample_stride);
    GTAV_REQUIRE((uint32_t)rows <= slots_per_sample || sample_stride >= (int64_t)slots_per_sample * n,
                 "rng_normal: sample_stride %lld is less than the %u x %d floats of a sample's rows", (long long)sample_stride, slots_per_sample, n);
    return launch_rng_normal(out, (size_t)sample_stride, rows, n, RngDraw{seed, draw, sample0, slot0, slots_per_sample}, clamp_abs, (hipStream_t)stream);
}
int gtav_noise_window_rng(const float* x, const float* alpha, float* x_noisy, float* v_target, int32_t B, int32_t W, int32_t n, uint64_t seed, uint32_t draw,
                          uint32_t sample0, float clamp_abs, void* stream) {
    GTAV_REQUIRE(x && alpha && x_noisy && v_target, "noise_window_rng: null pointer");
    GTAV_REQUIRE(B >= 1 && W >= 1, "noise_window_rng: B=%d W=%d", B, W);
    GTAV_RNG_ROWS("noise_window_rng", (int64_t)B * W, n);
    GTAV_REQUIRE(clamp_abs >= 0.0f, "noise_window_rng: clamp_abs %g (>= 0; infinity for no clamp)", (double)clamp_abs);
    GTAV_REQUIRE(aligned16(x) && aligned16(x_noisy) && aligned16(v_target), "noise_window_rng: x, x_noisy and v_target must be 16-byte aligned");
    return launch_noise_window_rng(x, alpha, x_noisy, v_target, B, W, n, RngDraw{seed, draw, sample0, 0u, (uint32_t)W}, clamp_abs, (hipStream_t)stream);
}
int gtav_vae_posterior_sample(const float* moments, float* z, int32_t frames, int32_t tokens, int32_t latent_dim, uint64_t seed, uint32_t draw,
                              uint32_t sample0, uint32_t slot0, uint32_t slots_per_sample, void* stream) {
    GTAV_REQUIRE(moments && z, "vae_posterior_sample: null pointer");
    GTAV_REQUIRE(latent_dim >= 4 && latent_dim % 4 == 0, "vae_posterior_sample: latent_dim %d (a multiple of 4: one generator call makes four elements)", latent_dim);
    GTAV_REQUIRE(tokens >= 1 && (int64_t)tokens * latent_dim < (int64_t)1 << 30, "vae_posterior_sample: %d tokens x %d", tokens, latent_dim);
    GTAV_RNG_ROWS("vae_posterior_sample", frames, tokens * latent_dim);
    GTAV_REQUIRE(slots_per_sample >= 1, "vae_posterior_sample: slots_per_sample 0");
    GTAV_REQUIRE(aligned16(moments) && aligned16(z), "vae_posterior_sample: moments and z must be 16-byte aligned");
    return launch_vae_posterior_sample(moments, z, frames, tokens, latent_dim, RngDraw{seed, draw, sample0, slot0, slots_per_sample}, (hipStream_t)stream);
}
int gtav_op_rng_bits(uint32_t* out, int32_t rows, int32_t n, uint64_t seed, uint32_t draw, uint32_t sample0, uint32_t slot0, uint32_t slots_per_sample,
                     void* stream) {
    GTAV_REQUIRE(out && aligned16(out), "op_rng_bits: null or unaligned pointer");
    GTAV_RNG_ROWS("op_rng_bits", rows, n);
    GTAV_REQUIRE(slots_per_sample >= 1, "op_rng_bits: slots_per_sample 0");
    return launch_rng_bits(out, rows, n, RngDraw{seed, draw, sample0, slot0, slots_per_sample}, (hipStream_t)stream);
}
#undef GTAV_RNG_ROWS
int gtav_axpy_f32(float* y, const float* x, float alpha, int64_t n, void* stream) {
    GTAV_REQUIRE(y && x && n > 0, "axpy_f32: bad argument");
    return launch_axpy_f32(y, x, alpha, (size_t)n, (hipStream_t)stream);
}
int gtav_mse(const float* a, int64_t a_stride, const float* b, int64_t b_stride, int32_t rows, int32_t n, float* out, void* stream) {
    return launch_mse(a, (size_t)a_stride, b, (size_t)b_stride, rows, n, out, (hipStream_t)stream);
}
int gtav_frames_to_u8(const float* img, uint8_t* out, int32_t N, int32_t H, int32_t W, void* stream) {
    return launch_frames_to_u8(img, out, N, H, W, (hipStream_t)stream);
}
int gtav_moments_to_latents(const float* mom, float* lat, int32_t N, int32_t hw, int32_t latent, int32_t mom_ch, float scale,
                            void* stream) {
    return launch_moments_to_latents(mom, lat, N, hw, latent, mom_ch, scale, (hipStream_t)stream);
}
int gtav_strip_to_frames(const uint8_t* strip, int32_t H, int32_t W, int32_t n_frames, float* out, int32_t OH, int32_t OW, void* stream) {
    return launch_resize_aa(strip, 1, out, n_frames, H, W, OH, OW, (hipStream_t)stream);
}
int gtav_resize_frames(const float* src, float* dst, int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, void* stream) {
    return launch_resize_aa(src, 0, dst, N, H, W, OH, OW, (hipStream_t)stream);
}
int gtav_latents_to_tokens(const float* lat, float* z, int32_t N, int32_t hw, int32_t latent, void* stream) {
    return launch_latents_to_tokens(lat, z, N, hw, latent, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// kernel-level entry points
// ------------------------------------------------------------------------------------------------
// split workspace of the persistent 256-token-tile kernel for the kernel-level entry points (a handle owns its own): allocated on first use per device —
// these test / tool entry points are never called under stream capture
static int op_sk_workspace(GemmParams& g) {
#ifndef GTAV_EXPERIMENTS
    (void)g;
    return 0;      // (the kernel that splits tiles lives in the experiments build)
#else
    static float* ws[64] = {nullptr};
    static int* flags[64] = {nullptr};
    int dev = 0;
    GTAV_CHECK_HIP(hipGetDevice(&dev));
    dev &= 63;
    if (!ws[dev]) {
        GTAV_CHECK_HIP(hipMalloc((void**)&ws[dev], gemm_sk_ws_bytes()));
        GTAV_CHECK_HIP(hipMalloc((void**)&flags[dev], gemm_sk_flag_bytes()));
        GTAV_CHECK_HIP(hipMemset(flags[dev], 0, gemm_sk_flag_bytes()));
    }
    g.sk_ws = ws[dev];
    g.sk_flags = flags[dev];
    return 0;
#endif
}
int gtav_op_gemm_f16(const void* x, int32_t ldx, const void* w, const float* bias, void* out, int32_t ldo, int32_t M, int32_t N,
                     int32_t K, int32_t epilogue, const float* gate, int32_t gate_stride, int32_t rows_per_gate, void* stream) {
    GTAV_REQUIRE((epilogue >= 0 && epilogue <= 4) || epilogue == EPI_PARTIAL || epilogue == EPI_F16_TILED, "op_gemm_f16: epilogue %d", epilogue);
    GemmParams g = gemm_params((const f16*)x, ldx, (const f16*)w, M, N, K);
    RET_IF(op_sk_workspace(g));
    if (epilogue == EPI_PARTIAL) g.splitk = gate_stride > 0 ? gate_stride : 1;  // split-K factor travels in gate_stride
    g.bias = bias; g.out = out; g.ldo = ldo;
    g.gate = gate; g.gate_stride = gate_stride; g.rows_per_gate = rows_per_gate;
    return op_ops().gemm(g, epilogue, (hipStream_t)stream);
}
int gtav_op_gemm_qkv(const void* x, int32_t ldx, const void* w, const float* bias, int32_t M, int32_t D, int32_t mode, void* q,
                     void* k, void* v, int32_t S, int32_t Tq, int32_t t0, int32_t Tmax, const float* rope_cs, void* stream) {
    GemmParams g = gemm_params((const f16*)x, ldx, (const f16*)w, M, 3 * D, D);
    g.bias = bias; g.D = D; g.S = S;
    g.qkv_mode = mode; g.q = (f16*)q; g.k = (f16*)k; g.v = (f16*)v; g.Tq = Tq; g.t0 = t0; g.Tmax = Tmax;
    g.rope_cs = rope_cs;
    return op_ops().gemm(g, EPI_QKV, (hipStream_t)stream);
}
#ifdef GTAV_EXPERIMENTS   // csrc/experiments.h
int gtav_op_gemm_fold_producer(const void* x, const void* w, const float* bias, float* resid, int32_t M, int32_t N, int32_t K, const float* gate,
                               const float* next_scale, int32_t mod_stride, int32_t tokens_per_frame, void* a_out, float* stats_out, void* stream) {
    GemmParams g = gemm_params((const f16*)x, K, (const f16*)w, M, N, K);
    g.bias = bias; g.out = resid; g.ldo = N;
    g.gate = gate; g.gate_stride = mod_stride; g.rows_per_gate = tokens_per_frame;
    g.f_P = tokens_per_frame; g.f_scale = next_scale; g.f_stats_out = stats_out; g.f_a = (f16*)a_out;
    return launch_gemm(g, EPI_RESID_FOLD, (hipStream_t)stream);
}
int gtav_op_gemm_fold_consumer(const void* a, const void* w, int32_t M, int32_t N, int32_t K, int32_t epi, const float* stats, const float* c1, const float* c2,
                               int32_t ldc, int32_t tokens_per_frame, void* out, int32_t ldo, void* stream) {
    GTAV_REQUIRE(epi == EPI_F32 || epi == EPI_GELU_TANH, "gemm_fold_consumer: epilogue %d (0 = f32 row-major, 2 = GELU-tanh fp16 tile-major)", epi);
    GemmParams g = gemm_params((const f16*)a, K, (const f16*)w, M, N, K);
    g.out = out; g.ldo = ldo;
    g.f_P = tokens_per_frame; g.f_stats = stats; g.f_nslot = K / 64; g.f_c1 = c1; g.f_c2 = c2; g.f_ldc = ldc;
    return launch_gemm(g, epi == EPI_F32 ? EPI_F32_FOLD : EPI_GELU_TANH_FOLD, (hipStream_t)stream);
}
#endif
int gtav_op_skinny_f32(const float* x, int32_t ldx, const float* w, const float* bias, float* y, int32_t ldy, int32_t M,
                       int32_t N, int32_t K, int32_t act_silu, void* stream) {
    return launch_skinny_f32(x, ldx, w, bias, y, ldy, M, N, K, act_silu, (hipStream_t)stream);
}
int gtav_op_ln_modulate(const float* x, void* out, int32_t M, int32_t D, const float* shift, const float* scale,
                        int32_t mod_stride, int32_t rows_per_mod, void* stream) {
    return op_ops().ln_modulate((float*)x, D, (f16*)out, D, M, D, shift, scale, mod_stride, nullptr, rows_per_mod, nullptr, nullptr, (hipStream_t)stream);
}
int gtav_op_ln_affine(const float* x, void* out, int32_t M, int32_t D, const float* gamma, const float* beta, void* stream) {
    return op_ops().ln_affine((float*)x, D, (f16*)out, D, M, D, gamma, beta, nullptr, nullptr, (hipStream_t)stream);
}
int gtav_op_attn_spatial(const void* q, const void* k, const void* vt, void* o, int32_t NB, int32_t heads, int32_t S, void* stream) {
    return op_ops().attn_spatial((const f16*)q, (const f16*)k, (const f16*)vt, (f16*)o, NB, heads, S, (hipStream_t)stream, false);
}
// the form the VAE runs: q carries 1/8 log2 e (GemmParams::rope_cs_q); launch_attn_spatial refuses the sequence lengths whose kernel takes plain q
int gtav_op_attn_spatial_prescaled(const void* q, const void* k, const void* vt, void* o, int32_t NB, int32_t heads, int32_t S, void* stream) {
    GTAV_REQUIRE(attn_spatial_wants_prescaled_q(S), "op_attn_spatial_prescaled: S=%d runs a kernel that takes plain q", S);
    return op_ops().attn_spatial((const f16*)q, (const f16*)k, (const f16*)vt, (f16*)o, NB, heads, S, (hipStream_t)stream, true);
}
static int op_attn_temporal(bool bf16, const void* q, const void* kv, void* o, int32_t B, int32_t P, int32_t D, int32_t Tq, int32_t t0, int32_t Tmax, void* stream) {
    return operand_ops(bf16).attn_temporal((const f16*)q, (const f16*)kv, (f16*)o, B, P, D, Tq, t0, Tmax, (hipStream_t)stream);
}
int gtav_op_attn_temporal(const void* q, const void* kv, void* o, int32_t B, int32_t P, int32_t D, int32_t Tq, int32_t t0,
                          int32_t Tmax, void* stream) {
    return op_attn_temporal(false, q, kv, o, B, P, D, Tq, t0, Tmax, stream);
}
int gtav_op_attn_temporal_bf16(const void* q, const void* kv, void* o, int32_t B, int32_t P, int32_t D, int32_t Tq, int32_t t0,
                               int32_t Tmax, void* stream) {
    return op_attn_temporal(true, q, kv, o, B, P, D, Tq, t0, Tmax, stream);
}
int gtav_op_qkv_head_major(const void* w, void* w_hm, int32_t D, void* stream) {
    GTAV_OP_F16_ONLY("op_qkv_head_major");
    return launch_qkv_head_major((const f16*)w, (f16*)w_hm, D, (hipStream_t)stream);
}
int gtav_op_gemm_qkvt_attn(const void* x_tperm, const void* w_hm, int32_t M, int32_t D, int32_t P, int32_t Tq, int32_t t0,
                           int32_t Tmax, const float* rope_cs, void* kv, void* o, void* stream) {
    GTAV_OP_F16_ONLY("op_gemm_qkvt_attn");
    GemmParams g = gemm_params((const f16*)x_tperm, D, (const f16*)w_hm, M, 3 * D, D);
    g.D = D; g.S = P;
    g.qkv_mode = QKV_TEMPORAL; g.k = (f16*)kv; g.v = (f16*)kv; g.out = o; g.ldo = D; g.Tq = Tq; g.t0 = t0; g.Tmax = Tmax;
    g.rope_cs = rope_cs;
    return launch_gemm_qkvt_attn(g, (hipStream_t)stream);
}
int gtav_op_qkv_head_major_spatial(const void* w, void* w_hm, int32_t D, void* stream) {
    GTAV_OP_F16_ONLY("op_qkv_head_major_spatial");
    return launch_qkv_head_major((const f16*)w, (f16*)w_hm, D, (hipStream_t)stream, 1);
}
int gtav_op_gemm_qkvs_attn(const void* x, const void* w_hm, int32_t M, int32_t D, int32_t P, const float* rope_cs, void* o, void* stream) {
    GTAV_OP_F16_ONLY("op_gemm_qkvs_attn");
    GemmParams g = gemm_params((const f16*)x, D, (const f16*)w_hm, M, 3 * D, D);
    g.D = D; g.S = P;
    g.qkv_mode = QKV_SPATIAL; g.out = o; g.ldo = D; g.rope_cs = rope_cs;
    return launch_gemm_qkvs_attn(g, (hipStream_t)stream);
}
static int op_attn_spatial_bwd(bool bf16, const void* q, const void* k, const void* vt, const void* d_o, int32_t NB, int32_t heads, int32_t S, const float* rope_cs,
                               void* dqkv, void* stream) {
    return operand_ops(bf16).attn_spatial_bwd((const f16*)q, (const f16*)k, (const f16*)vt, (const f16*)d_o, NB, heads, S, heads * 64, rope_cs, (f16*)dqkv, nullptr,
                                              (hipStream_t)stream);
}
int gtav_op_attn_spatial_bwd(const void* q, const void* k, const void* vt, const void* d_o, int32_t NB, int32_t heads, int32_t S,
                             const float* rope_cs, void* dqkv, void* stream) {
    return op_attn_spatial_bwd(false, q, k, vt, d_o, NB, heads, S, rope_cs, dqkv, stream);
}
int gtav_op_attn_spatial_bwd_bf16(const void* q, const void* k, const void* vt, const void* d_o, int32_t NB, int32_t heads, int32_t S,
                                  const float* rope_cs, void* dqkv, void* stream) {
    return op_attn_spatial_bwd(true, q, k, vt, d_o, NB, heads, S, rope_cs, dqkv, stream);
}
static int op_attn_temporal_bwd(bool bf16, const void* q, const void* kv, const void* d_o, int32_t B, int32_t P, int32_t D, int32_t T, int32_t Tmax, const float* rope_cs,
                                void* dqkv, void* stream) {
    GTAV_REQUIRE(q && kv && d_o && rope_cs && dqkv, "op_attn_temporal_bwd: null argument");
    return operand_ops(bf16).attn_temporal_bwd((const f16*)q, (const f16*)kv, (const f16*)d_o, B, P, D, T, Tmax, rope_cs, (f16*)dqkv, nullptr, (hipStream_t)stream);
}
int gtav_op_attn_temporal_bwd(const void* q, const void* kv, const void* d_o, int32_t B, int32_t P, int32_t D, int32_t T, int32_t Tmax,
                              const float* rope_cs, void* dqkv, void* stream) {
    return op_attn_temporal_bwd(false, q, kv, d_o, B, P, D, T, Tmax, rope_cs, dqkv, stream);
}
int gtav_op_attn_temporal_bwd_bf16(const void* q, const void* kv, const void* d_o, int32_t B, int32_t P, int32_t D, int32_t T, int32_t Tmax,
                                   const float* rope_cs, void* dqkv, void* stream) {
    return op_attn_temporal_bwd(true, q, kv, d_o, B, P, D, T, Tmax, rope_cs, dqkv, stream);
}
int gtav_op_gemm_tn(const void* x, const void* w, int32_t M, int32_t N, int32_t K, float* out, int32_t ldo, void* stream) {
    GemmParams q = gemm_params((const f16*)x, M, (const f16*)w, M, N, K);
    q.out = out; q.ldo = ldo;
    return op_ops().gemm_tn(q, (hipStream_t)stream);
}
int gtav_op_gemm_dw_grouped(int32_t n, const void* const* x, const void* const* w, float* const* out, const int32_t* M, const int32_t* N, const int32_t* ldo,
                            int32_t K, void* stream) {
    GTAV_REQUIRE(n >= 1 && n <= GEMM_DW_MAX_GROUPS && x && w && out && M && N && ldo, "op_gemm_dw_grouped: 1 .. %d groups", GEMM_DW_MAX_GROUPS);
    GemmDwGroup g[GEMM_DW_MAX_GROUPS];
    for (int i = 0; i < n; ++i) g[i] = GemmDwGroup{(const f16*)x[i], (const f16*)w[i], out[i], M[i], N[i], ldo[i]};
    return op_ops().gemm_dw_grouped(g, n, K, nullptr, (hipStream_t)stream, false);
}
int gtav_op_gemm_splitk_ln(const void* x, int32_t ldx, const void* w, const float* bias, int32_t M, int32_t N, int32_t K,
                           int32_t splitk, float* parts, float* resid, const float* gate, int32_t gate_stride,
                           int32_t rows_per_gate, void* out_f16, const float* shift, const float* scale, int32_t mod_stride,
                           void* stream) {
    GemmParams g = gemm_params((const f16*)x, ldx, (const f16*)w, M, N, K);
    g.out = parts; g.ldo = N;
    g.splitk = splitk > 0 ? splitk : gemm_choose_splitk(M, N, K);
    RET_IF(op_ops().gemm(g, EPI_PARTIAL, (hipStream_t)stream));
    LnPending pd;
    memset(&pd, 0, sizeof(pd));
    pd.parts = parts; pd.nsplit = g.splitk; pd.slab_stride = (size_t)M * N; pd.ld = N; pd.bias = bias; pd.gate = gate;
    pd.gate_stride = gate_stride; pd.rows_per_gate = rows_per_gate;
    return op_ops().ln_modulate(resid, N, (f16*)out_f16, N, M, N, shift, scale, mod_stride, nullptr, rows_per_gate, &pd, nullptr, (hipStream_t)stream);
}
// Test hooks (include/gtav_amd_testing.h): ONE launch_ln_modulate (mode 0: p0 = shift, p1 = scale) or launch_ln_affine (mode 1: p0 = gamma, p1 = beta; rows,
// rows_per_mod and mod_stride unused) with every LnPending field passed flat, and launch_branch_rows.  Nothing is validated here: the launchers' own
// refusals are what the tests hold.
int gtav_op_ln_pending(int32_t mode, float* x, int32_t ldx, void* out, int32_t M, int32_t D, const float* p0, const float* p1, int32_t mod_stride,
                       const int32_t* rows, int32_t rows_per_mod, const float* parts, int32_t nsplit, int64_t slab_stride, int32_t ld,
                       const float* bias, const float* gate, int32_t gate_stride, const int32_t* gate_rows, int32_t rows_per_gate, float* x_out, void* y_save,
                       int32_t tperm_T, int32_t tperm_P, float* k_save, const float* k_load, int32_t* err, void* stream) {
    LnPending pd;
    memset(&pd, 0, sizeof(pd));
    pd.parts = parts; pd.nsplit = nsplit; pd.slab_stride = (size_t)slab_stride; pd.ld = ld; pd.bias = bias; pd.gate = gate;
    pd.gate_stride = gate_stride; pd.gate_rows = gate_rows; pd.rows_per_gate = rows_per_gate; pd.x_out = x_out; pd.y_save = (f16*)y_save;
    pd.tperm_T = tperm_T; pd.tperm_P = tperm_P; pd.k_save = k_save; pd.k_load = k_load;
    if (mode == 0) return op_ops().ln_modulate(x, ldx, (f16*)out, D, M, D, p0, p1, mod_stride, rows, rows_per_mod, &pd, err, (hipStream_t)stream);
    return op_ops().ln_affine(x, ldx, (f16*)out, D, M, D, p0, p1, &pd, err, (hipStream_t)stream);
}
int gtav_op_branch_rows(const float* parts, int32_t nsplit, int64_t slab_stride, int32_t ld, const float* bias, void* y, int32_t M, int32_t N, int32_t* err,
                        void* stream) {
    return op_ops().branch_rows(parts, nsplit, (size_t)slab_stride, ld, bias, (f16*)y, M, N, err, (hipStream_t)stream);
}
int gtav_op_rope_interleave(const float* cos_t, const float* sin_t, float* cs, int32_t npos, void* stream) {
    return launch_rope_interleave(cos_t, sin_t, cs, npos, (hipStream_t)stream);
}
int gtav_op_gemm_choose_splitk(int32_t M, int32_t N, int32_t K) { return gemm_choose_splitk(M, N, K); }
int gtav_op_gemm_resid_inplace(int32_t M, int32_t N, int32_t K) { return gemm_resid_inplace_ok(M, N, K, 0) ? 1 : 0; }
int gtav_op_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t qkv_mode, int32_t S, int32_t splitk, int32_t rows_per_gate, int32_t* plan8) {
    static_assert(sizeof(gtav_shared::GemmPlan) == 8 * sizeof(int32_t), "plan8 is the GemmPlan");
    GTAV_REQUIRE(plan8, "op_gemm_plan: null argument");
    return gtav_shared::gemm_plan(gtav_shared::GemmProblem{M, N, K, epilogue, qkv_mode, S, splitk, rows_per_gate}, (gtav_shared::GemmPlan*)plan8);
}
int gtav_op_launch_plan(int32_t kind, int32_t a0, int32_t a1, int32_t a2, int32_t a3, int32_t a4, int32_t a5, int32_t a6, int32_t* plan12) {
    GTAV_REQUIRE(plan12 && kind >= 0 && kind <= 9, "op_launch_plan: null argument or unknown kind %d", kind);
    const int a[7] = {a0, a1, a2, a3, a4, a5, a6};
    return kind == 0 ? ln_launch_plan(a, plan12) : kind <= 2 ? attn_launch_plan(kind, a, plan12) : kind == 5 ? skinny_launch_plan(a, plan12) : train_launch_plan(kind, a, plan12);
}
// the forced ring depth / block shape are thread_locals of the planner (gemm_plan.hip), one set for both operand types
void gtav_op_gemm_set_stages(int32_t ns) { gtav_shared::gemm_set_stages(ns); }
#ifdef GTAV_EXPERIMENTS
void gtav_op_gemm_set_debug(int32_t bits) { gtav_shared::gemm_set_debug(bits); }   // libgtav_amd_exp.so only (csrc/experiments.h)
void gtav_op_gemm_set_stamps(void* buf_dev, int32_t max_blocks) { gemm_set_stamps((unsigned long long*)buf_dev, max_blocks); }
#endif
void gtav_op_gemm_set_wm(int32_t wm) { gtav_shared::gemm_set_wm(wm); }
void gtav_op_set_operand_dtype(int32_t dtype) { g_op_bf16 = dtype == GTAV_OPERAND_BF16; }

// Calibration of the in-situ profiler (gtav_dit_profile / gtav_vae_profile): `reps` launches of a one-wave kernel that spins `spin_us` microseconds on the
// device's own 100 MHz clock, enqueued back to back, each with an event pair attached to its dispatch exactly like a profiled kernel.  Returns the mean event-pair
// reading and the mean duration the kernel measured itself; their difference is what an attached event pair adds to a kernel's time.
int gtav_timer_calibrate(int32_t spin_us, int32_t reps, double* event_us_mean, double* device_us_mean, void* stream) {
    GTAV_REQUIRE(spin_us >= 0 && spin_us <= 1000 && reps >= 1 && reps <= 256 && event_us_mean && device_us_mean, "timer_calibrate: bad argument");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* dev = nullptr;
    GTAV_CHECK_HIP(hipMalloc(&dev, sizeof(unsigned long long) * reps));
    std::vector<hipEvent_t> ev(2 * reps, nullptr);
    int rc = 0;
    for (int i = 0; i < 2 * reps && !rc; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) { set_error("timer_calibrate: hipEventCreate failed"); rc = 1; }
    if (!rc) rc = launch_calib_spin((unsigned long long)spin_us * 100ull, dev, s);   // warm-up (module load), no events
    if (!rc && hipStreamSynchronize(s) != hipSuccess) { set_error("timer_calibrate: synchronize failed"); rc = 1; }
    for (int i = 0; i < reps && !rc; ++i) {
        g_launch_ev[0] = ev[2 * i];
        g_launch_ev[1] = ev[2 * i + 1];
        rc = launch_calib_spin((unsigned long long)spin_us * 100ull, dev + i, s);
        g_launch_ev[0] = nullptr;
    }
    std::vector<unsigned long long> ticks(reps, 0);
    if (!rc && (hipStreamSynchronize(s) != hipSuccess ||
                hipMemcpy(ticks.data(), dev, sizeof(unsigned long long) * reps, hipMemcpyDeviceToHost) != hipSuccess)) { set_error("timer_calibrate: read-back failed"); rc = 1; }
    double e = 0, d = 0;
    for (int i = 0; i < reps && !rc; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) != hipSuccess) { set_error("timer_calibrate: hipEventElapsedTime failed"); rc = 1; break; }
        e += ms * 1e3;
        d += (double)ticks[i] * 0.01;
    }
    for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
    (void)hipFree(dev);
    if (rc) return rc;
    *event_us_mean = e / reps;
    *device_us_mean = d / reps;
    return 0;
}

int gtav_op_convert_f16(const float* src, int32_t lds, int32_t R, int32_t C, void* dst, int32_t Rp, int32_t Cp, int32_t tiled,
                        void* stream) {
    return op_ops().convert_pad(src, lds, R, C, (f16*)dst, Rp, Cp, 1.0f, tiled, (hipStream_t)stream, nullptr);
}

// ------------------------------------------------------------------------------------------------
// Test hooks over the backward-only training launchers (include/gtav_amd_testing.h gtav_op_train_*): what api_train.hip launches, one launcher (or the fused /
// unfused group of them) per hook.  The caller owns every buffer; nothing is allocated and nothing synchronises.  A workspace that is too small is refused by name.
// ------------------------------------------------------------------------------------------------
#define GTAV_OP_WS(name, ws, have, need)                                                                                                         \
    GTAV_REQUIRE((ws) && (have) >= (int64_t)(need), name ": workspace of %lld floats, %lld needed", (long long)((ws) ? (have) : 0), (long long)(need))
int gtav_op_train_ln_mod_bwd(int32_t fused, const float* dxn, const float* x, const float* scale, int32_t mod_stride, int32_t frames, int32_t P, int32_t D,
                             float* dres, int32_t accumulate, float* dshift, float* dscale, float* ws, int64_t ws_floats, void* stream) {
    GTAV_REQUIRE(dxn && x && scale && dres && dshift && dscale, "op_train_ln_mod_bwd: null argument");
    GTAV_REQUIRE(frames >= 1 && P >= 1 && D >= 4 && D % 4 == 0 && D <= 2048 && mod_stride >= D && mod_stride % 4 == 0 && aligned16(scale) && aligned16(dxn) &&
                     aligned16(x) && aligned16(dres),
                 "op_train_ln_mod_bwd: frames=%d P=%d D=%d mod_stride=%d (D a multiple of 4 up to 2048, rows read as aligned 16-byte vectors)", frames, P, D, mod_stride);
    if (fused) {
        GTAV_REQUIRE(ln_bwd_fused_ok(D), "op_train_ln_mod_bwd: the fused launch exists at D = 256, 512, 1024 and 2048 only, not at D=%d", D);
        GTAV_OP_WS("op_train_ln_mod_bwd (fused)", ws, ws_floats, ln_bwd_fused_workspace(frames, P, D));
        return launch_ln_mod_bwd_fused(dxn, x, scale, mod_stride, frames, P, D, dres, accumulate, dshift, dscale, ws, (hipStream_t)stream);
    }
    GTAV_OP_WS("op_train_ln_mod_bwd (row statistics)", ws, ws_floats, (int64_t)2 * frames * P);
    RET_IF(launch_ln_mod_bwd(dxn, x, scale, mod_stride, P, frames * P, D, dres, accumulate, ws, (hipStream_t)stream));
    return launch_frame_reduce_ln(dxn, x, ws, frames, P, D, dshift, dscale, mod_stride, (hipStream_t)stream);
}
int gtav_op_train_gate_bwd(int32_t fused, const float* dres, const void* y, const float* gate, int32_t mod_stride, int32_t frames, int32_t P, int32_t D,
                           void* dy_tiled, float* dgate, float* db, float* ws, int64_t ws_floats, int32_t* err, void* stream) {
    GTAV_REQUIRE(dres && y && dy_tiled && dgate, "op_train_gate_bwd: null argument");
    GTAV_REQUIRE(frames >= 1 && P >= 1 && D >= 64 && D % 64 == 0 && mod_stride >= D && mod_stride % 4 == 0 && aligned16(dres) && (!gate || aligned16(gate)),
                 "op_train_gate_bwd: frames=%d P=%d D=%d mod_stride=%d", frames, P, D, mod_stride);
    const int M = frames * P;
    if (fused) {
        GTAV_OP_WS("op_train_gate_bwd (fused)", ws, ws_floats, (int64_t)frames * D);
        return op_ops().gate_bwd_fused(dres, (const f16*)y, gate, mod_stride, frames, P, D, (f16*)dy_tiled, dgate, db, ws, err, (hipStream_t)stream);
    }
    GTAV_REQUIRE(db, "op_train_gate_bwd: the unfused form adds its column sums to db, which is null");
    GTAV_OP_WS("op_train_gate_bwd (column sums)", ws, ws_floats, colsum_workspace(M, D));
    RET_IF(op_ops().gate_bwd(dres, gate, mod_stride, P, M, D, (f16*)dy_tiled, err, (hipStream_t)stream));
    RET_IF(op_ops().frame_reduce_gate(dres, (const f16*)y, frames, P, D, dgate, mod_stride, (hipStream_t)stream));
    return op_ops().colsum_tiled((const f16*)dy_tiled, M, D, db, ws, (hipStream_t)stream);
}
int gtav_op_train_gelu_bwd(int32_t fused, const void* dh, const void* u, void* du, int32_t M, int32_t N, float* db, float* ws, int64_t ws_floats, int32_t* err,
                           void* stream) {
    GTAV_REQUIRE(dh && u && du && M >= 1 && N >= 64 && N % 64 == 0, "op_train_gelu_bwd: M=%d N=%d (N a multiple of 64)", M, N);
    if (fused) {
        GTAV_OP_WS("op_train_gelu_bwd (fused)", ws, ws_floats, (int64_t)gelu_bwd_colsum_splits(M) * N);
        return op_ops().gelu_bwd_tiled_colsum((const f16*)dh, (const f16*)u, (f16*)du, M, N, db, ws, err, (hipStream_t)stream);
    }
    GTAV_REQUIRE(db, "op_train_gelu_bwd: the unfused form adds its column sums to db, which is null");
    GTAV_OP_WS("op_train_gelu_bwd (column sums)", ws, ws_floats, colsum_workspace(M, N));
    RET_IF(op_ops().gelu_bwd_tiled((const f16*)dh, (const f16*)u, (f16*)du, (size_t)round_up(M, 128) * N, err, (hipStream_t)stream));
    return op_ops().colsum_tiled((const f16*)du, M, N, db, ws, (hipStream_t)stream);
}
int gtav_op_train_colsum_tiled(const void* dy, int32_t M, int32_t N, float* db, float* ws, int64_t ws_floats, void* stream) {
    GTAV_REQUIRE(dy && db && M >= 1 && N >= 64, "op_train_colsum_tiled: M=%d N=%d", M, N);
    GTAV_OP_WS("op_train_colsum_tiled", ws, ws_floats, colsum_workspace(M, N));
    return op_ops().colsum_tiled((const f16*)dy, M, N, db, ws, (hipStream_t)stream);
}
int gtav_op_train_colsum_f32(const float* a, int32_t lda, int32_t M, int32_t N, float* db, float* ws, int64_t ws_floats, void* stream) {
    GTAV_REQUIRE(a && db && M >= 1 && N >= 1 && lda >= N, "op_train_colsum_f32: M=%d N=%d lda=%d", M, N, lda);
    GTAV_OP_WS("op_train_colsum_f32", ws, ws_floats, colsum_workspace(M, N));
    return launch_colsum_f32(a, lda, M, N, db, ws, (hipStream_t)stream);
}
int gtav_op_train_colsum_reduce_multi(const float* const* ws, float* const* db, const int32_t* splits, const int32_t* N, int32_t njobs, void* stream) {
    GTAV_REQUIRE(ws && db && splits && N, "op_train_colsum_reduce_multi: null argument");
    GTAV_REQUIRE(njobs >= 1 && njobs <= 4, "op_train_colsum_reduce_multi: %d jobs (1 .. 4)", njobs);
    for (int j = 0; j < njobs; ++j)
        GTAV_REQUIRE(ws[j] && db[j] && splits[j] >= 1 && N[j] >= 1, "op_train_colsum_reduce_multi: job %d: splits=%d N=%d or a null pointer", j, splits[j], N[j]);
    return launch_colsum_reduce_multi(ws, db, splits, N, njobs, (hipStream_t)stream);
}
int gtav_op_train_mse_bwd_patch(const float* vpred, const float* vtarget, int32_t B, int32_t T, int32_t C, int32_t H, int32_t W, int32_t p, float scale, void* dfo,
                                int32_t ldf, int32_t* err, void* stream) {
    GTAV_REQUIRE(vpred && vtarget && dfo && B >= 1 && T >= 1 && C >= 1 && p >= 1 && H >= p && W >= p && H % p == 0 && W % p == 0,
                 "op_train_mse_bwd_patch: B=%d T=%d C=%d H=%d W=%d p=%d", B, T, C, H, W, p);
    return op_ops().mse_bwd_patch(vpred, vtarget, B, T, C, H, W, p, scale, (f16*)dfo, ldf, err, (hipStream_t)stream);
}
int gtav_op_train_to_tiled(const float* a, int32_t M, int32_t D, void* out, int32_t* err, void* stream) {
    GTAV_REQUIRE(a && out && M >= 1 && D >= 64 && aligned16(a), "op_train_to_tiled: M=%d D=%d", M, D);
    return op_ops().to_tiled(a, M, D, (f16*)out, err, (hipStream_t)stream);
}
int gtav_op_train_transpose_tiled(const void* src, int32_t R, int32_t C, void* dst, void* stream) {
    GTAV_REQUIRE(src && dst, "op_train_transpose_tiled: null argument");
    return op_ops().transpose_tiled((const f16*)src, R, C, (f16*)dst, (hipStream_t)stream);
}
int gtav_op_train_convert_t(const float* src, int32_t lds, int32_t R, int32_t C, void* dst, void* stream) {
    GTAV_REQUIRE(src && dst && R >= 1 && C >= 1 && lds >= C, "op_train_convert_T: R=%d C=%d lds=%d", R, C, lds);
    return op_ops().convert_T(src, lds, R, C, (f16*)dst, (hipStream_t)stream);
}
// The two attention backward launches as a training handle makes them (api_train.hip): the thread's operand type and the caller's error word, where the product
// entries gtav_op_attn_*_bwd[_bf16] above pass none.
int gtav_op_train_attn_spatial_bwd(const void* q, const void* k, const void* vt, const void* d_o, int32_t NB, int32_t heads, int32_t S, const float* rope_cs,
                                   void* dqkv, int32_t* err, void* stream) {
    GTAV_REQUIRE(q && k && vt && d_o && rope_cs && dqkv, "op_train_attn_spatial_bwd: null argument");
    return op_ops().attn_spatial_bwd((const f16*)q, (const f16*)k, (const f16*)vt, (const f16*)d_o, NB, heads, S, heads * 64, rope_cs, (f16*)dqkv, err,
                                     (hipStream_t)stream);
}
int gtav_op_train_attn_temporal_bwd(const void* q, const void* kv, const void* d_o, int32_t B, int32_t P, int32_t D, int32_t T, int32_t Tmax, const float* rope_cs,
                                    void* dqkv, int32_t* err, void* stream) {
    GTAV_REQUIRE(q && kv && d_o && rope_cs && dqkv, "op_train_attn_temporal_bwd: null argument");
    return op_ops().attn_temporal_bwd((const f16*)q, (const f16*)kv, (const f16*)d_o, B, P, D, T, Tmax, rope_cs, (f16*)dqkv, err, (hipStream_t)stream);
}
// Low-rank adapters, kernel level (include/gtav_amd.h): the gradient of one Linear as a LoRA training handle launches it, and the merge of one Linear (both images,
// then the fp32 sum where w_f32 is given).  The launchers validate the shapes and the workspace by name.
int gtav_op_lora_grads(const void* x, const void* dy, const float* a_f32, const float* b_f32, int32_t M, int32_t N, int32_t K, int32_t r, float s, float* dA,
                       float* dB, float* ws, int64_t ws_floats, int32_t* err, void* stream) {
    GTAV_REQUIRE(ws_floats >= 0, "op_lora_grads: ws_floats=%lld", (long long)ws_floats);
    return op_ops().lora_grads((const f16*)x, (const f16*)dy, a_f32, b_f32, M, N, K, r, s, dA, dB, ws, (size_t)ws_floats, err, (hipStream_t)stream);
}
int gtav_op_lora_merge(const float* w0_f32, const float* a_f32, const float* b_f32, int32_t N, int32_t K, int32_t r, float s, void* w_img, void* wT_img,
                       float* w_f32, void* stream) {
    GTAV_REQUIRE(w_img, "op_lora_merge: null image");
    LoraMergeParam P;
    memset(&P, 0, sizeof(P));
    P.w0 = w0_f32; P.a = a_f32; P.b = b_f32; P.N = N; P.K = K; P.r = r; P.s = s;
    P.w16 = (f16*)w_img; P.Cp16 = K; P.wT = (f16*)wT_img; P.RpT = round_up(N, 64); P.w32 = w_f32;
    RET_IF(op_ops().lora_merge_one(P, 0, (hipStream_t)stream));
    return w_f32 ? op_ops().lora_merge_one(P, 1, (hipStream_t)stream) : 0;
}
int gtav_op_train_silu(const float* x, int32_t ldx, float* y, int32_t ldy, int32_t R, int32_t C, void* stream) {
    GTAV_REQUIRE(x && y && R >= 1 && C >= 1 && ldx >= C && ldy >= C, "op_train_silu: R=%d C=%d ldx=%d ldy=%d", R, C, ldx, ldy);
    return launch_silu(x, ldx, y, ldy, R, C, (hipStream_t)stream);
}
int gtav_op_train_silu_bwd(const float* dy, int32_t lddy, const float* x, int32_t ldx, float* dx, int32_t lddx, int32_t R, int32_t C, void* stream) {
    GTAV_REQUIRE(dy && x && dx && R >= 1 && C >= 1 && lddy >= C && ldx >= C && lddx >= C, "op_train_silu_bwd: R=%d C=%d lddy=%d ldx=%d lddx=%d", R, C, lddy, ldx, lddx);
    return launch_silu_bwd(dy, lddy, x, ldx, dx, lddx, R, C, (hipStream_t)stream);
}
int gtav_op_train_gemm_tn_f32(const float* dY, int32_t lddy, const float* X, int32_t ldx, int32_t R, int32_t N, int32_t K, float* dW, int32_t lddw, void* stream) {
    GTAV_REQUIRE(dY && X && dW && R >= 1 && N >= 1 && K >= 1 && lddy >= N && ldx >= K && lddw >= K, "op_train_gemm_tn_f32: R=%d N=%d K=%d lddy=%d ldx=%d lddw=%d", R, N, K,
                 lddy, ldx, lddw);
    // the matrix-core kernel (N % 64 == 0 and K % 64 == 0) updates dW by 16-byte vectors
    GTAV_REQUIRE(N % 64 || K % 64 || (lddw % 4 == 0 && aligned16(dW)), "op_train_gemm_tn_f32: dW rows must be 16-byte aligned at N=%d K=%d (lddw=%d)", N, K, lddw);
    return launch_gemm_tn_f32(dY, lddy, X, ldx, R, N, K, dW, lddw, (hipStream_t)stream);
}
int gtav_op_train_gemm_nn_f32(const float* dY, int32_t lddy, const float* W, int32_t ldw, int32_t R, int32_t N, int32_t K, float* dX, int32_t lddx, void* stream) {
    GTAV_REQUIRE(dY && W && dX && R >= 1 && N >= 1 && K >= 1 && lddy >= N && ldw >= K && lddx >= K && aligned16(dY), "op_train_gemm_nn_f32: R=%d N=%d K=%d lddy=%d ldw=%d lddx=%d",
                 R, N, K, lddy, ldw, lddx);
    return launch_gemm_nn_f32(dY, lddy, W, ldw, R, N, K, dX, lddx, (hipStream_t)stream);
}
int gtav_op_train_ada_bwd_dx(const float* dmod, int32_t MODW, const float* W, int32_t D, int32_t R, float* dSc, float* part, int64_t part_floats, void* stream) {
    GTAV_REQUIRE(dmod && W && dSc && MODW >= 1 && D >= 1 && R >= 1, "op_train_ada_bwd_dx: MODW=%d D=%d R=%d", MODW, D, R);
    GTAV_OP_WS("op_train_ada_bwd_dx", part, part_floats, ada_bwd_dx_workspace(MODW, D, R));
    return launch_ada_bwd_dx(dmod, MODW, W, D, R, dSc, part, (hipStream_t)stream);
}
// The optimizer step, kernel level (include/gtav_amd_testing.h): the norm's partial sums, the step coefficient, the multi-tensor AdamW launch in its three modes
// over work items cut by the handle's own planner (api_internal.h adam_plan_items), and the overflow publisher — each the launcher gtav_dit_adamw_step runs.
int gtav_op_train_sumsq_parts(int64_t n) { return sumsq_parts((size_t)n); }
int gtav_op_train_sumsq(const float* g, int64_t n, float* part, int64_t part_floats, void* stream) {
    GTAV_OP_WS("op_train_sumsq", part, part_floats, sumsq_parts((size_t)n));
    return launch_sumsq(g, (size_t)n, part, (hipStream_t)stream);
}
int gtav_op_train_clip_coef(float* ctl, const float* part, int32_t nparts, float inv_scale, float max_norm, float beta1, float beta2, float ema_decay,
                            int32_t ema_warmup, int32_t* err, void* stream) {
    return launch_clip_coef(ctl, part, nparts, inv_scale, max_norm, beta1, beta2, ema_decay, ema_warmup, err, (hipStream_t)stream);
}
int gtav_op_train_adamw_multi(int32_t mode, int32_t n_params, float* const* p, const int32_t* ldp, const int32_t* R, const int32_t* C, const float* const* g,
                              float* const* m, float* const* v, float* const* e, void* const* w16, const int32_t* Cp16, void* const* wT, const int32_t* RpT,
                              void* desc, int64_t desc_bytes, const float* ctl, float lr, float beta1, float beta2, float eps, float wd, void* stream) {
    GTAV_REQUIRE(mode >= 0 && mode <= 2 && n_params >= 1, "op_train_adamw_multi: mode=%d (0 step, 1 step + averaged weights, 2 swap), %d parameters", mode, n_params);
    std::vector<AdamParam> ap((size_t)n_params);
    std::vector<AdamItem> ai;
    for (int pi = 0; pi < n_params; ++pi) {
        AdamParam& d = ap[pi];
        memset(&d, 0, sizeof(d));
        d.p = p[pi]; d.ldp = ldp[pi]; d.R = R[pi]; d.C = C[pi]; d.g = g[pi]; d.m = m[pi]; d.v = v[pi]; d.e = e[pi];
        d.w16 = (f16*)w16[pi]; d.Cp16 = Cp16[pi]; d.wT = (f16*)wT[pi]; d.RpT = RpT[pi];
        adam_plan_items(d, pi, ai);
    }
    const size_t pb = ap.size() * sizeof(AdamParam), ib = ai.size() * sizeof(AdamItem);
    GTAV_REQUIRE(desc && desc_bytes >= (int64_t)(pb + ib), "op_train_adamw_multi: descriptor buffer of %lld bytes, %lld needed (%d parameters, %zu work items)",
                 (long long)(desc ? desc_bytes : 0), (long long)(pb + ib), n_params, ai.size());
    GTAV_REQUIRE(!ai.empty(), "op_train_adamw_multi: no work item");
    // (blocking copies, as gtav_dit_train_enable fills its tables: the one hook that synchronises)
    GTAV_CHECK_HIP(hipMemcpy(desc, ap.data(), pb, hipMemcpyHostToDevice));
    GTAV_CHECK_HIP(hipMemcpy((char*)desc + pb, ai.data(), ib, hipMemcpyHostToDevice));
    const AdamParam* dp = (const AdamParam*)desc;
    const AdamItem* di = (const AdamItem*)((char*)desc + pb);
    if (mode == 0) return op_ops().adamw_multi(dp, di, (int)ai.size(), ctl, lr, beta1, beta2, eps, wd, (hipStream_t)stream);
    if (mode == 1) return op_ops().adamw_multi_ema(dp, di, (int)ai.size(), ctl, lr, beta1, beta2, eps, wd, (hipStream_t)stream);
    return op_ops().adamw_swap_ema(dp, di, (int)ai.size(), (hipStream_t)stream);
}
int gtav_op_train_overflow_publish(const int32_t* err, float* g, void* stream) { return launch_overflow_publish(err, g, (hipStream_t)stream); }
#undef GTAV_OP_WS

}  // extern "C"
