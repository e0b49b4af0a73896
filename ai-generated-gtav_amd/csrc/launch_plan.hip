// The launch planner of the non-GEMM kernels (launch_plan.h): the measured rules that pick an instantiation and its grid.  Host code only, built once per library.
#include "ops.h"   // launch_plan.h, cdiv, round_up, GTAV_REQUIRE

#include <cstdlib>

namespace gtav_shared {
using namespace gtav;   // cdiv, round_up

// ---- laboratory overrides: the one place where the environment reaches these selections (experiments build, callers with lab = true) ----
struct LaunchKnobs {
    int ln_wave_row_min = 0;            // GTAV_LN_WAVE_ROW_MIN: ln_wave_row_kernel from this many rows on when there is no pending update
    int attn_force_flash = 0;           // GTAV_ATTN_FORCE_FLASH: the flash kernel for short sequences too (A/B runs)
    int attn_s_blocks = 512;            // GTAV_ATTN_S_BLOCKS: blocks the one-pass kernel's query split aims at
    int attn_1p_nw = 4;                 // GTAV_ATTN_1P_NW: waves per block of the one-pass kernel at NK = 10 (A/B runs: 3, 5 or 9; the product runs 4)
    int attn_flash_nqt = 0;             // GTAV_ATTN_FLASH_NQT: 2 .. 4 forces the query tiles per wave (A/B runs)
    int attn_flash_occ3 = 1;            // GTAV_ATTN_FLASH_OCC3: 0 = three query tiles per wave at two blocks per CU (A/B runs)
    int attn_t_split_max = 1024;        // GTAV_ATTN_T_SPLIT_MAX
    int skinny_ft_min_blocks = 1024;    // GTAV_SKINNY_FT_MIN_BLOCKS: a huge value = one tile per wave everywhere (A/B)
    int skinny_variant = 0;             // GTAV_SKINNY_VARIANT: 41 / 42 / 82 force (FT, RT)
    int skinny_chunked = 1;             // GTAV_SKINNY_CHUNKED: 0 = the whole-K slabs (A/B)
    int attn_bwd_dbg = 0;               // GTAV_ATTN_BWD_DBG: timing variants of the MFMA kernel (wrong results)
};
static const LaunchKnobs g_lab_off = {};
#ifdef GTAV_EXPERIMENTS
static const LaunchKnobs g_lab = {GTAV_ENV_INT("GTAV_LN_WAVE_ROW_MIN", 0), GTAV_ENV_INT("GTAV_ATTN_FORCE_FLASH", 0), GTAV_ENV_INT("GTAV_ATTN_S_BLOCKS", 512),
                                  GTAV_ENV_INT("GTAV_ATTN_1P_NW", 4), GTAV_ENV_INT("GTAV_ATTN_FLASH_NQT", 0), GTAV_ENV_INT("GTAV_ATTN_FLASH_OCC3", 1),
                                  GTAV_ENV_INT("GTAV_ATTN_T_SPLIT_MAX", 1024), GTAV_ENV_INT("GTAV_SKINNY_FT_MIN_BLOCKS", 1024), GTAV_ENV_INT("GTAV_SKINNY_VARIANT", 0),
                                  GTAV_ENV_INT("GTAV_SKINNY_CHUNKED", 1), GTAV_ENV_INT("GTAV_ATTN_BWD_DBG", 0)};
static const LaunchKnobs& knobs(bool lab) { return lab ? g_lab : g_lab_off; }
#else
static const LaunchKnobs& knobs(bool) { return g_lab_off; }
#endif

// the plan's kernel is a member of the list: anything else is refused by name, never launched as nothing
#define GTAV_PLAN_KERNEL(plan, list, what, lab, ...)                                                             \
    do {                                                                                                         \
        (plan)->kernel = kernel_index(list, __VA_ARGS__);                                                        \
        GTAV_REQUIRE((plan)->kernel >= 0 && ((list)[(plan)->kernel].product || ((lab) && LAUNCH_LAB_BUILD)), what ": no kernel instantiation for this problem"); \
    } while (0)

// ---- LayerNorm (elementwise.hip launch_ln_modulate / launch_ln_affine) ----
// ln_wave_row_kernel when there is no pending update (every such launch: 3.4 vs 3.6 us at 720 rows, 7.1 vs 8.9 at 5 760, 45 vs 67 at 46 080).
// (Round 2 had tried one wave per row for the batch-1 forward's launches WITH a pending update: 5.2-5.3 us per launch against 4.9 for the row-block
// kernel at M = 720 in a one-process A/B, profiles/round2/forward_ab_B1_ln_wave_row.txt; round 5 measured the same again.)
int ln_plan(const LnProblem& g, LaunchGeom* plan, bool lab) {
    const bool wave_d = g.D == 256 || g.D == 512 || g.D == 1024 || g.D == 2048;
    if (g.k_save || g.k_load) {   // the statistics' shift kept / given: always one block per row (LnPending::k_save)
        GTAV_PLAN_KERNEL(plan, LN_KERNELS, "ln", lab, LF_LN_ROW_BLOCK, g.mode, g.k_save ? 1 : 0, g.k_save ? 1 : 2);
    } else if (!g.slabs && !g.perm && g.M >= knobs(lab).ln_wave_row_min && wave_d) {
        GTAV_PLAN_KERNEL(plan, LN_KERNELS, "ln", lab, LF_LN_WAVE_ROW, g.mode, g.D / 256);
        plan->gx = cdiv(g.M, 4), plan->gy = 1, plan->block = 256, plan->lds = 0;
        return 0;
    } else {   // one block per row
        GTAV_PLAN_KERNEL(plan, LN_KERNELS, "ln", lab, LF_LN_ROW_BLOCK, g.mode, g.slabs ? 1 : 0, 0);
    }
    plan->gx = g.M, plan->gy = 1, plan->block = round_up(g.D / 4, 64), plan->lds = 0;
    return 0;
}

// ---- spatial attention (attention.hip launch_attn_spatial) ----
int attn_spatial_plan(const AttnSpatialProblem& g, AttnSpatialPlan* plan, bool lab) {
    const LaunchKnobs& k = knobs(lab);
    const int NB = g.NB, heads = g.heads, S = g.S;
    const int S_pad = round_up(S, 32), nqt = cdiv(S, 16);
    if (S_pad <= 160 && !k.attn_force_flash) {   // short sequences (the DiT's frames): one pass per query tile, scores in registers
        plan->lds = (size_t)S_pad * 128 + (size_t)64 * (S_pad + 8) * 2;
        plan->nqb = 0;
        const int nk = S_pad / 16;
        if (nk == 10 && (k.attn_1p_nw == 3 || k.attn_1p_nw == 5 || k.attn_1p_nw == 9)) {   // experiments build: A/B of the waves per block
            GTAV_PLAN_KERNEL(plan, ATTN_SPATIAL_KERNELS, "attn_spatial", lab, LF_ATTN_1P, k.attn_1p_nw, 10);
            plan->gx = NB * heads, plan->gy = 1, plan->block = 64 * k.attn_1p_nw, plan->qsplit = 1;
            return 0;
        }
        // enough blocks to fill 256 CUs when there are few (frame, head) pairs; each block re-stages K / Vt from L2
        int qsplit = 1;
        const int max_split = cdiv(nqt, 4);
        while (NB * heads * qsplit < k.attn_s_blocks && qsplit < max_split) ++qsplit;
        GTAV_PLAN_KERNEL(plan, ATTN_SPATIAL_KERNELS, "attn_spatial", lab, LF_ATTN_1P, 4, nk);
        plan->gx = NB * heads, plan->gy = qsplit, plan->block = 256, plan->qsplit = qsplit;
        return 0;
    }
    // long sequences (the VAE's 576 tokens): flash form, K / Vt streamed through a 3-slot LDS ring (48 KiB whatever S is), 4 waves x NQT query tiles per block.
    // NQT by the fewest padded query tiles; on a tie the larger tile once the grid fills the chip, else the smaller (more blocks)
    int best = 0, best_pad = 1 << 30, best_nqb = 0;
    for (int c = 2; c <= 4; ++c) {
        const int nqb_c = cdiv(nqt, 4 * c), pad = nqb_c * c;
        const bool better = pad < best_pad || (pad == best_pad && NB * heads * best_nqb >= 512);
        if (better) best = c, best_pad = pad, best_nqb = nqb_c;
    }
    if (k.attn_flash_nqt >= 2 && k.attn_flash_nqt <= 4) best = k.attn_flash_nqt, best_nqb = cdiv(nqt, 4 * k.attn_flash_nqt);
    const int occ = best == 2 || (best == 3 && k.attn_flash_occ3) ? 3 : 2;
    GTAV_PLAN_KERNEL(plan, ATTN_SPATIAL_KERNELS, "attn_spatial", lab, LF_ATTN_FLASH, best, occ, S % 64 != 0 ? 1 : 0, g.q_prescaled ? 1 : 0);
    plan->gx = (int)((long long)NB * heads * best_nqb), plan->gy = 1, plan->block = 256, plan->lds = 0;   // (the launcher refuses a grid beyond 2^31)
    plan->qsplit = 0, plan->nqb = best_nqb;
    return 0;
}

// ---- temporal attention (attention.hip launch_attn_temporal) ----
// The kernel is chosen by the number of VISIBLE frames, never by the cache stride Tmax: a window of <= 8 frames runs the same
// kernel, and gives the same bits, whatever capacity its handle was built for.
int attn_temporal_plan(const AttnTemporalProblem& g, AttnTemporalPlan* plan, bool lab) {
    const int tpc = g.D / 8, cpb = tpc >= 256 ? 1 : 256 / tpc;  // threads per column, columns per block
    const int Tvis = g.t0 + g.Tq;
    plan->gx = cdiv(g.BP, cpb), plan->gy = 1, plan->block = tpc * cpb, plan->lds = 0, plan->split = 0;
    if (Tvis > 8) {
        if (g.Tq == 1) {
            GTAV_PLAN_KERNEL(plan, ATTN_TEMPORAL_KERNELS, "attn_temporal", lab, LF_ATTN_T_STREAM, 1, 8);
        } else {
            GTAV_PLAN_KERNEL(plan, ATTN_TEMPORAL_KERNELS, "attn_temporal", lab, LF_ATTN_T_STREAM, 8, 4);
            plan->gy = cdiv(g.Tq, 8);
        }
        return 0;
    }
    plan->split = (g.Tq > 1 && g.BP < knobs(lab).attn_t_split_max) ? 1 : 0;   // few columns: one block per (column group, query frame)
    if (plan->split) plan->gy = g.Tq;
    GTAV_PLAN_KERNEL(plan, ATTN_TEMPORAL_KERNELS, "attn_temporal", lab, LF_ATTN_T, Tvis <= 5 ? 5 : 8);
    return 0;
}

// ---- attention backward (train.hip) ----
int attn_spatial_bwd_plan(const AttnSpatialBwdProblem& g, LaunchGeom* plan, bool lab) {
    const int S = g.S;
    plan->gx = g.NB * g.heads, plan->gy = 1;
    if (S > AB_MAXS || S % 16 != 0) {   // the streaming kernel; S <= 160 with S % 16 == 0 stays on the resident kernel below, bit for bit
        GTAV_PLAN_KERNEL(plan, ATTN_SPATIAL_BWD_KERNELS, "attn_spatial_bwd", lab, LF_ATTN_S_BWD_STREAM);
        plan->block = 64 * ABS_NW;
        plan->lds = (size_t)2 * ABS_CH * ABS_LP * 2 + (size_t)ABS_NW * 16 * ABS_LP * 2 + (size_t)ABS_NW * 256 * 2 + (size_t)2 * round_up(S, 16) * 4;
        return 0;
    }
    const int dbg = knobs(lab).attn_bwd_dbg;
    GTAV_PLAN_KERNEL(plan, ATTN_SPATIAL_BWD_KERNELS, "attn_spatial_bwd", lab, LF_ATTN_S_BWD_MFMA, dbg == 1 || dbg == 3 || dbg == 7 ? dbg : 0);
    plan->block = 64 * ABM_NW;
    plan->lds = (size_t)4 * S * ABM_LP * 2 + (size_t)S * ABM_DQP * 4 + (size_t)2 * S * 4 + (size_t)ABM_NW * 256 * 2;
    return 0;
}
int attn_temporal_bwd_plan(const AttnTemporalBwdProblem& g, LaunchGeom* plan) {
    const size_t threads = (size_t)g.B * g.P * (g.D / 64) * 16;
    plan->gx = (int)((threads + 255) / 256), plan->gy = 1, plan->block = 256, plan->lds = 0;
    if (g.T > 8) GTAV_PLAN_KERNEL(plan, ATTN_TEMPORAL_BWD_KERNELS, "attn_temporal_bwd", false, LF_ATTN_T_BWD_STREAM);   // T <= 8 stays on the register-resident kernel, bit for bit
    else GTAV_PLAN_KERNEL(plan, ATTN_TEMPORAL_BWD_KERNELS, "attn_temporal_bwd", false, LF_ATTN_T_BWD, g.T);
    return 0;
}

// ---- skinny fp32 GEMM (skinny.hip launch_skinny_f32) ----
int skinny_plan(const SkinnyProblem& g, LaunchGeom* plan, bool lab) {
    const LaunchKnobs& k = knobs(lab);
    const int M = g.M, N = g.N, K = g.K, act = g.act_silu ? 1 : 0;
    // four (eight) feature tiles per wave where that still leaves the chip full, 32-row slabs as soon as there are two of them: the adaLN table of a frame
    // 1.52 -> 0.92 ms at 101 rows (batch 1), 11.3 -> 5.0 ms at 808 rows (batch 8)
    int ft = 1, rt = 1;
    if ((long long)cdiv(N, 256) * cdiv(M, 16) >= k.skinny_ft_min_blocks) {
        ft = 4;
        if (M > 32 && (size_t)32 * (K + 8) * sizeof(float) <= 150 * 1024) {
            rt = 2;
            if (!act && (long long)cdiv(N, 512) * cdiv(M, 32) >= k.skinny_ft_min_blocks) ft = 8;
        }
    }
    plan->block = 256;
    // many features, more than two row tiles, no activation (the adaLN table): 80-112 rows per block on K chunks of 128 (44-61 KiB of LDS: two or three blocks per CU) — W is streamed once per 5-7 row tiles
    if (k.skinny_chunked && !act && M > 32 && K % 128 == 0 && (long long)cdiv(N, 256) >= 256 && k.skinny_variant == 0) {
        const int tiles = cdiv(M, 16);
        const int rtc = tiles <= 5 ? 5 : tiles == 6 ? 6 : tiles == 7 ? 7 : 6;   // one block of rows up to 112 rows, 96-row blocks beyond
        GTAV_PLAN_KERNEL(plan, SKINNY_KERNELS, "skinny", lab, LF_SKINNY, 0, 4, rtc, 128);
        plan->gx = cdiv(N, 256), plan->gy = cdiv(M, 16 * rtc);
        plan->lds = (size_t)16 * rtc * (128 + 8) * sizeof(float);
        return 0;
    }
    if (k.skinny_variant == 41) ft = 4, rt = 1;
    if (k.skinny_variant == 42) ft = 4, rt = 2;
    if (k.skinny_variant == 82 && !act) ft = 8, rt = 2;
    GTAV_PLAN_KERNEL(plan, SKINNY_KERNELS, "skinny", lab, LF_SKINNY, act, ft, rt, 0);
    plan->gx = cdiv(N, 64 * ft), plan->gy = cdiv(M, 16 * rt);
    plan->lds = (size_t)16 * rt * (K + 8) * sizeof(float);
    return 0;
}

// ---- fp32 training launchers (train.hip) ----
int gemm_tn_f32_plan(const GemmF32Problem& g, LaunchGeom* plan) {
    plan->block = 256, plan->lds = 0;
    if (g.N % 64 == 0 && g.K % 64 == 0) {
        GTAV_PLAN_KERNEL(plan, GEMM_TN_F32_KERNELS, "gemm_tn_f32", false, LF_GEMM_TN_MFMA);
        plan->gx = g.K / 64, plan->gy = cdiv(g.N, 256);
    } else {
        GTAV_PLAN_KERNEL(plan, GEMM_TN_F32_KERNELS, "gemm_tn_f32", false, LF_GEMM_TN_VALU);
        plan->gx = cdiv(g.K, 256), plan->gy = cdiv(g.N, 8);
    }
    return 0;
}
int gemm_nn_f32_plan(const GemmF32Problem& g, LaunchGeom* plan) {
    const size_t row = (size_t)g.N * sizeof(float);
    const int rows = 16 * row <= 64 * 1024 ? 16 : 8 * row <= 64 * 1024 ? 8 : 4;   // rows of dY per block: as many of 16 / 8 / 4 as fit 64 KiB of LDS
    GTAV_PLAN_KERNEL(plan, GEMM_NN_F32_KERNELS, "gemm_nn_f32", false, LF_GEMM_NN, rows);
    plan->gx = cdiv(g.K, 64), plan->gy = cdiv(g.R, rows), plan->block = 64, plan->lds = rows * row;
    return 0;
}
int ada_bwd_dx_plan(const AdaBwdProblem& g, AdaBwdPlan* plan) {
    plan->lds = 0;
    if (g.D % 64 == 0 && g.D <= 1024 && g.R <= 16 * ADA_RT) {
        GTAV_PLAN_KERNEL(plan, ADA_BWD_DX_KERNELS, "ada_bwd_dx", false, LF_ADA_MFMA);
        plan->nchunk = cdiv(g.MODW, ADA_KC);
        plan->gx = plan->nchunk, plan->gy = 1, plan->block = g.D;
    } else {
        // shapes the matrix-core kernel does not take (hidden % 64 != 0, more than 80 conditioning rows): the VALU kernel, same fixed-order reduction
        GTAV_PLAN_KERNEL(plan, ADA_BWD_DX_KERNELS, "ada_bwd_dx", false, LF_ADA_VALU);
        plan->nchunk = cdiv(g.MODW, ADA_VALU_KC);    // (<= cdiv(MODW, ADA_KC) chunks: the workspace covers it)
        plan->gx = cdiv(g.D, 256), plan->gy = plan->nchunk, plan->block = 256;
    }
    plan->reduce_gx = (int)(((long long)g.R * g.D + 255) / 256);
    return 0;
}
int ln_bwd_fused_plan(const LnBwdFusedProblem& g, LnBwdFusedPlan* plan) {
    GTAV_PLAN_KERNEL(plan, LN_BWD_FUSED_KERNELS, "ln_mod_bwd_fused", false, LF_LN_BWD_FUSED, g.D % 256 == 0 ? g.D / 256 : 0);
    plan->gx = cdiv(g.P, 16), plan->gy = g.frames, plan->block = 256, plan->lds = 0;
    plan->reduce_gx = cdiv(g.D, 256), plan->reduce_gy = g.frames;
    return 0;
}

}  // namespace gtav_shared
