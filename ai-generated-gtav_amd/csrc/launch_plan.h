// Which kernel instantiation a non-GEMM launcher runs, on which grid: the instantiation lists and the planner (launch_plan.hip), after the model of gemm_plan.h.
// Pure host code in namespace gtav_shared, compiled ONCE: the fp16 objects and their bf16 twins call the same functions.  Nothing here calls HIP or names the
// operand type; a launcher (attention.hip, elementwise.hip, skinny.hip, train.hip) validates, asks its *_plan() and dispatches over the same list.
#pragma once
#include <cstddef>
#include <type_traits>

namespace gtav_shared {

// GTAV_LAB_BUILD (common.h): true in a translation unit built with -DGTAV_EXPERIMENTS — the planner's environment knobs apply to its calls; false in the
// product objects and in the bf16 twins of BOTH libraries: the measured rules only
constexpr bool LAUNCH_LAB_BUILD = GTAV_LAB_BUILD;

// Geometry the kernels and the planner's LDS formulas share (train.hip)
constexpr int AB_MAXS = 160;   // bound of the two LDS-resident kernels (DiT: 144); longer frames and S % 16 == 8 run attn_spatial_bwd_stream_kernel
constexpr int ABM_LP = 72, ABM_DQP = 68, ABM_NW = 9, ABM_MAXT = AB_MAXS / 16;   // 9 waves: one query / key tile each at S = 144 (3 waves: 170 us per launch of 1280 items, 9 waves: 99 us)
constexpr int ABS_LP = 72, ABS_NW = 8, ABS_CH = 64;
constexpr int ADA_KC = 1024, ADA_RT = 5, ADA_PITCH = 68, ADA_VALU_KC = 2048;   // MODW chunk of the MFMA kernel, its row tiles and LDS pitch; chunk of the VALU kernel
constexpr int LAUNCH_LDS_MAX = 160 * 1024;   // what a kernel with dynamic LDS opts in to (common.h lds_opt_in)

// Kernel template of an instantiation; a .. d below are its template arguments in the template's own order (bool as 0 / 1, unused ones 0).
enum LaunchFamily : int {
    LF_LN_WAVE_ROW,          // ln_wave_row_kernel<MODE, NV>
    LF_LN_ROW_BLOCK,         // ln_row_block_kernel<MODE, PEND, KS>
    LF_ATTN_1P,              // attn_spatial_1p_kernel<NW, NK>
    LF_ATTN_FLASH,           // attn_flash_kernel<NQT, OCC, RAGGED, PRESCALED>
    LF_ATTN_T,               // attn_temporal_kernel<TM>
    LF_ATTN_T_STREAM,        // attn_temporal_stream_kernel<QG, FB>
    LF_ATTN_S_BWD_MFMA,      // attn_spatial_bwd_mfma_kernel<DBG>
    LF_ATTN_S_BWD_STREAM,    // attn_spatial_bwd_stream_kernel
    LF_ATTN_T_BWD,           // attn_temporal_bwd_kernel<TT>
    LF_ATTN_T_BWD_STREAM,    // attn_temporal_bwd_stream_kernel
    LF_SKINNY,               // skinny_f32_kernel<ACT, FT, RT, KC>
    LF_GEMM_TN_MFMA,         // gemm_tn_f32_mfma_kernel
    LF_GEMM_TN_VALU,         // gemm_tn_f32_kernel
    LF_GEMM_NN,              // gemm_nn_f32_kernel<ROWS>
    LF_ADA_MFMA,             // ada_bwd_dx_mfma_kernel (+ ada_reduce_kernel)
    LF_ADA_VALU,             // ada_bwd_dx_kernel (+ ada_reduce_kernel)
    LF_LN_BWD_FUSED,         // ln_mod_bwd_fused_kernel<NV> (+ frame_partials_reduce_kernel)
};
struct KernelInst {
    int family, a, b, c, d;
    bool product;   // false: compiled into the experiments build only (csrc/build.sh exp)
};

// ---- every instantiation, once: a planner returns an index into its launcher's list, the launcher's dispatch and LDS opt-in iterate over the same list ----
constexpr KernelInst LN_KERNELS[] = {
    {LF_LN_WAVE_ROW, 0, 1, 0, 0, true},  {LF_LN_WAVE_ROW, 0, 2, 0, 0, true},  {LF_LN_WAVE_ROW, 0, 4, 0, 0, true},  {LF_LN_WAVE_ROW, 0, 8, 0, 0, true},
    {LF_LN_WAVE_ROW, 1, 1, 0, 0, true},  {LF_LN_WAVE_ROW, 1, 2, 0, 0, true},  {LF_LN_WAVE_ROW, 1, 4, 0, 0, true},  {LF_LN_WAVE_ROW, 1, 8, 0, 0, true},
    {LF_LN_ROW_BLOCK, 0, 1, 1, 0, true}, {LF_LN_ROW_BLOCK, 0, 0, 2, 0, true}, {LF_LN_ROW_BLOCK, 0, 1, 0, 0, true}, {LF_LN_ROW_BLOCK, 0, 0, 0, 0, true},
    {LF_LN_ROW_BLOCK, 1, 1, 1, 0, true}, {LF_LN_ROW_BLOCK, 1, 0, 2, 0, true}, {LF_LN_ROW_BLOCK, 1, 1, 0, 0, true}, {LF_LN_ROW_BLOCK, 1, 0, 0, 0, true},
};
constexpr KernelInst ATTN_SPATIAL_KERNELS[] = {
    {LF_ATTN_1P, 4, 2, 0, 0, true}, {LF_ATTN_1P, 4, 4, 0, 0, true}, {LF_ATTN_1P, 4, 6, 0, 0, true}, {LF_ATTN_1P, 4, 8, 0, 0, true}, {LF_ATTN_1P, 4, 10, 0, 0, true},
    {LF_ATTN_1P, 3, 10, 0, 0, false}, {LF_ATTN_1P, 5, 10, 0, 0, false}, {LF_ATTN_1P, 9, 10, 0, 0, false},   // waves per block at NK = 10 (A/B runs)
    {LF_ATTN_FLASH, 2, 3, 0, 0, true}, {LF_ATTN_FLASH, 2, 3, 0, 1, true}, {LF_ATTN_FLASH, 2, 3, 1, 0, true}, {LF_ATTN_FLASH, 2, 3, 1, 1, true},
    {LF_ATTN_FLASH, 3, 3, 0, 0, true}, {LF_ATTN_FLASH, 3, 3, 0, 1, true}, {LF_ATTN_FLASH, 3, 3, 1, 0, true}, {LF_ATTN_FLASH, 3, 3, 1, 1, true},
    {LF_ATTN_FLASH, 3, 2, 0, 0, true}, {LF_ATTN_FLASH, 3, 2, 0, 1, true}, {LF_ATTN_FLASH, 3, 2, 1, 0, true}, {LF_ATTN_FLASH, 3, 2, 1, 1, true},
    {LF_ATTN_FLASH, 4, 2, 0, 0, true}, {LF_ATTN_FLASH, 4, 2, 0, 1, true}, {LF_ATTN_FLASH, 4, 2, 1, 0, true}, {LF_ATTN_FLASH, 4, 2, 1, 1, true},
};
constexpr KernelInst ATTN_TEMPORAL_KERNELS[] = {{LF_ATTN_T, 5, 0, 0, 0, true}, {LF_ATTN_T, 8, 0, 0, 0, true}, {LF_ATTN_T_STREAM, 1, 8, 0, 0, true}, {LF_ATTN_T_STREAM, 8, 4, 0, 0, true}};
constexpr KernelInst ATTN_SPATIAL_BWD_KERNELS[] = {
    {LF_ATTN_S_BWD_STREAM, 0, 0, 0, 0, true}, {LF_ATTN_S_BWD_MFMA, 0, 0, 0, 0, true},
    {LF_ATTN_S_BWD_MFMA, 1, 0, 0, 0, false}, {LF_ATTN_S_BWD_MFMA, 3, 0, 0, 0, false}, {LF_ATTN_S_BWD_MFMA, 7, 0, 0, 0, false},   // timing variants (wrong results)
};
constexpr KernelInst ATTN_TEMPORAL_BWD_KERNELS[] = {
    {LF_ATTN_T_BWD, 1, 0, 0, 0, true}, {LF_ATTN_T_BWD, 2, 0, 0, 0, true}, {LF_ATTN_T_BWD, 3, 0, 0, 0, true}, {LF_ATTN_T_BWD, 4, 0, 0, 0, true}, {LF_ATTN_T_BWD, 5, 0, 0, 0, true},
    {LF_ATTN_T_BWD, 6, 0, 0, 0, true}, {LF_ATTN_T_BWD, 7, 0, 0, 0, true}, {LF_ATTN_T_BWD, 8, 0, 0, 0, true}, {LF_ATTN_T_BWD_STREAM, 0, 0, 0, 0, true},
};
// (FT, RT) variants: (1, 1) small projections; (4, 1) many features, tens of rows (the adaLN table at batch 1); (4, 2) / (8, 2) hundreds of rows; KC = 128: the K-chunked form
constexpr KernelInst SKINNY_KERNELS[] = {
    {LF_SKINNY, 0, 1, 1, 0, true}, {LF_SKINNY, 1, 1, 1, 0, true}, {LF_SKINNY, 0, 4, 1, 0, true}, {LF_SKINNY, 1, 4, 1, 0, true}, {LF_SKINNY, 0, 4, 2, 0, true},
    {LF_SKINNY, 1, 4, 2, 0, true}, {LF_SKINNY, 0, 8, 2, 0, true}, {LF_SKINNY, 0, 4, 5, 128, true}, {LF_SKINNY, 0, 4, 6, 128, true}, {LF_SKINNY, 0, 4, 7, 128, true},
};
constexpr KernelInst GEMM_TN_F32_KERNELS[] = {{LF_GEMM_TN_MFMA, 0, 0, 0, 0, true}, {LF_GEMM_TN_VALU, 0, 0, 0, 0, true}};
constexpr KernelInst GEMM_NN_F32_KERNELS[] = {{LF_GEMM_NN, 16, 0, 0, 0, true}, {LF_GEMM_NN, 8, 0, 0, 0, true}, {LF_GEMM_NN, 4, 0, 0, 0, true}};
constexpr KernelInst ADA_BWD_DX_KERNELS[] = {{LF_ADA_MFMA, 0, 0, 0, 0, true}, {LF_ADA_VALU, 0, 0, 0, 0, true}};
constexpr KernelInst LN_BWD_FUSED_KERNELS[] = {{LF_LN_BWD_FUSED, 1, 0, 0, 0, true}, {LF_LN_BWD_FUSED, 2, 0, 0, 0, true}, {LF_LN_BWD_FUSED, 4, 0, 0, 0, true}, {LF_LN_BWD_FUSED, 8, 0, 0, 0, true}};

// index of an instantiation in its list, -1 where the list has none
template <int N>
constexpr int kernel_index(const KernelInst (&list)[N], int family, int a = 0, int b = 0, int c = 0, int d = 0) {
    for (int i = 0; i < N; ++i)
        if (list[i].family == family && list[i].a == a && list[i].b == b && list[i].c == c && list[i].d == d) return i;
    return -1;
}
template <int N>
constexpr int kernel_count(const KernelInst (&)[N]) { return N; }
// f(std::integral_constant<int, i>) for the list member i == idx: the launchers' dispatch and nothing else instantiates a family's kernels
template <int N, int I = 0, class F>
inline int dispatch_kernel(int idx, F&& f) {
    if constexpr (I < N) return idx == I ? f(std::integral_constant<int, I>{}) : dispatch_kernel<N, I + 1>(idx, f);
    else return (gtav_shared::set_error("launch: kernel index %d is not in its list of %d", idx, N), 2);
}

// ---- problems (plain integers) and plans.  kernel: index into the launcher's list; grid (gx, gy), block threads and dynamic LDS bytes of the launch ----
struct LaunchGeom { int kernel, gx, gy, block; size_t lds; };
// slabs: a pending update with split-K slabs; perm: an output row permutation; k_save / k_load: the statistics' shift kept / given (LnPending)
struct LnProblem { int mode, M, D; bool slabs, perm, k_save, k_load; };
struct AttnSpatialProblem { int NB, heads, S; bool q_prescaled; };
struct AttnSpatialPlan : LaunchGeom { int qsplit, nqb; };        // one-pass kernel: query splits (grid y); flash kernel: query blocks per (frame, head)
struct AttnTemporalProblem { int BP, D, Tq, t0; };               // BP = B * P columns
struct AttnTemporalPlan : LaunchGeom { int split; };             // one block per (column group, query frame)
struct AttnSpatialBwdProblem { int NB, heads, S; };
struct AttnTemporalBwdProblem { int B, P, D, T; };
struct SkinnyProblem { int M, N, K; bool act_silu; };
struct GemmF32Problem { int R, N, K; };                          // gemm_tn_f32: dW [N][K] += dY^T X over R rows; gemm_nn_f32: dX [R][K] = dY [R][N] W
struct AdaBwdProblem { int MODW, D, R; };
struct AdaBwdPlan : LaunchGeom { int nchunk, reduce_gx; };       // chunks of MODW in the workspace; grid of the ada_reduce_kernel launch behind it
struct LnBwdFusedProblem { int frames, P, D; };
struct LnBwdFusedPlan : LaunchGeom { int reduce_gx, reduce_gy; };   // grid of the frame_partials_reduce_kernel launch behind it

// Each returns 0 and the plan, or 2 with the error string set where the problem has no instantiation (no valid input does: tests/test_host_launch_plan.py).
// The callers have validated the geometry; the planners only select.
int ln_plan(const LnProblem& g, LaunchGeom* plan, bool lab = LAUNCH_LAB_BUILD);
int attn_spatial_plan(const AttnSpatialProblem& g, AttnSpatialPlan* plan, bool lab = LAUNCH_LAB_BUILD);
int attn_temporal_plan(const AttnTemporalProblem& g, AttnTemporalPlan* plan, bool lab = LAUNCH_LAB_BUILD);
int attn_spatial_bwd_plan(const AttnSpatialBwdProblem& g, LaunchGeom* plan, bool lab = LAUNCH_LAB_BUILD);
int attn_temporal_bwd_plan(const AttnTemporalBwdProblem& g, LaunchGeom* plan);
int skinny_plan(const SkinnyProblem& g, LaunchGeom* plan, bool lab = LAUNCH_LAB_BUILD);
int gemm_tn_f32_plan(const GemmF32Problem& g, LaunchGeom* plan);
int gemm_nn_f32_plan(const GemmF32Problem& g, LaunchGeom* plan);
int ada_bwd_dx_plan(const AdaBwdProblem& g, AdaBwdPlan* plan);
int ln_bwd_fused_plan(const LnBwdFusedProblem& g, LnBwdFusedPlan* plan);

// gtav_op_launch_plan's twelve integers: the instantiation (family, a, b, c, d), the geometry (gx, gy, block, lds) and up to three numbers of the family's own
inline void launch_plan_report(const KernelInst& k, const LaunchGeom& p, int x0, int x1, int x2, int* out12) {
    const int v[12] = {k.family, k.a, k.b, k.c, k.d, p.gx, p.gy, p.block, (int)p.lds, x0, x1, x2};
    for (int i = 0; i < 12; ++i) out12[i] = v[i];
}

}  // namespace gtav_shared
