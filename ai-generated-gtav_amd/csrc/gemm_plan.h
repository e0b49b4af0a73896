// Which block shape a GEMM runs on, and how big that shape's tile is: the shape table and the planner (gemm_plan.hip).
// Pure host code in namespace gtav_shared, compiled ONCE: the fp16 gemm.hip and its bf16 twin call the same functions and see the same per-thread test
// overrides.  Nothing here calls HIP, names the operand type or reads GemmParams; launch_gemm (gemm.hip) validates, asks gemm_plan() and dispatches.
#pragma once

namespace gtav_shared {

constexpr int GEMM_TK = 64;   // K step of every kernel

// Kernel family of a block shape: which kernel template its row's numbers instantiate (gemm.hip launch_epi, gemm_experiments.inc launch_experiment_shape).
enum GemmFamily : int {
    GF_K128,   // gemm_kernel<EPI, ring, WM, FJ>: 128 x 128, all waves fill; the ring depth (2 or 4) is picked at run time
    GF_G,      // gemm_g_kernel<EPI, NS, FI, FJ, WM>: piece-granular tiles, all waves fill
    GF_T256,   // gemm256_kernel<EPI>: 256 x 256, K-tile in four quadrant phases (laboratory: gemm256_pp_kernel, the same tile with two wave groups in antiphase)
    GF_L,      // gemm_l_kernel<EPI, NS, FI, FJ, WN, WM, NL>: compute waves + NL loader waves
    GF_LP,     // gemm_lp_kernel<EPI, NS, FI, FJ, WN, WM>: persistent loader-wave kernel, one block per CU
    GF_LW,     // laboratory: gemm_lw_kernel<EPI, NS, FI, FJ, WN, WM, NL, D>, the weight operand straight into registers
    GF_LAB,    // laboratory kernels written for one geometry: gemm_pp_kernel (persistent ping-pong), gemm_p256_kernel<EPI, FI>, gemm_s16_kernel (persistent 256-token tiles)
};

// One block shape.  A wave computes 16 FI features x 16 FJ tokens; WN x WM compute waves (+ NL loader waves) make a block.  Where the kernel is a template over
// these numbers the launchers instantiate it FROM this row (gemm.hip launch_k128 / launch_g / launch_l / launch_lp), so tile, thread count, token span and LDS
// ring cannot drift apart; for the kernels that are written for one geometry the row is where that geometry is stated for the host.
struct GemmShape {
    int id, family;
    int ns;            // LDS ring depth the kernel is instantiated with (GF_K128: 0, the plan's ring depth picks between its two instantiations)
    int fi, fj, wn, wm, nl;
    bool product;      // false: compiled into the experiments build only (csrc/build.sh exp)
    constexpr int tokens() const { return 16 * fj * wm; }        // tile rows (M)
    constexpr int features() const { return 16 * fi * wn; }      // tile columns (N)
    constexpr int threads() const { return 64 * (wn * wm + nl); }
    constexpr int span() const { return 16 * fj; }               // tokens of one wave: a LayerNorm-fold epilogue needs frames at least this long
    constexpr int ring_bytes() const { return ns * (2 * fi * wn + 2 * fj * wm) * 1024; }   // GF_L: ns stages of the W and the X tile at 128 bytes per row
};

constexpr GemmShape GEMM_SHAPES[] = {
    //  id family      ns fi fj wn wm nl product
    {2,  GF_K128,   0, 4, 4, 2, 2, 0, true},    // 128 x 128, 4 waves of 64 x 64, two blocks per CU
    {3,  GF_K128,   0, 4, 2, 2, 4, 0, true},    // 128 x 128, 8 waves of 64 x 32 (two staggered waves per SIMD)
    {7,  GF_T256,   2, 8, 4, 2, 4, 0, true},    // 256 x 256, 8 waves, one block per CU
    {8,  GF_G,      4, 3, 2, 2, 3, 0, false},   // 96 x 96, 6 waves
    {9,  GF_G,      4, 4, 2, 2, 3, 0, false},   // 128 features x 96 tokens, 6 waves (3 stages 1-3 % and 5 stages 4-5 % slower)
    {11, GF_G,      4, 2, 1, 2, 3, 0, true},    // 64 features x 48 tokens, 6 waves: skinny M (context-cached sampling, M = 144); 6 stages measured 6-8 % slower
    {12, GF_G,      2, 4, 3, 2, 4, 0, true},    // 128 features x 192 tokens, 8 waves of 64 x 48, two blocks per CU (4 waves per SIMD)
    {13, GF_G,      2, 4, 3, 2, 2, 0, true},    // 128 features x 96 tokens, 4 waves of 64 x 48, two-stage ring, two blocks per CU: long-K N = 1024 GEMMs at a few thousand
                                                // tokens in ONE K slice (480 tiles at M = 5760 fill the 512 block slots; 128 x 128 has 360, 128 x 192 only 240)
    {14, GF_G,      4, 2, 2, 2, 3, 0, true},    // 64 features x 96 tokens, 6 waves: a few hundred tokens (M = 288-320)
    {16, GF_LAB,    3, 4, 3, 2, 4, 8, false},   // 128 x 192, persistent ping-pong: two groups of eight waves
    {17, GF_T256,   2, 8, 4, 2, 4, 0, false},   // shape 7's tile, two wave groups in antiphase
    {18, GF_LW,     4, 1, 6, 8, 1, 4, false},   // shape 20's tile, eight compute waves side by side along the features
    {20, GF_L,      4, 2, 3, 4, 2, 4, true},    // 128 x 96, 8 compute + 4 loader waves
    {21, GF_L,      3, 4, 4, 4, 2, 4, false},   // 256 x 128, 8 compute + 4 loader waves
    {22, GF_LW,     4, 2, 3, 4, 2, 4, false},   // shape 20's tile, the weight operand straight into registers
    {23, GF_L,      4, 4, 3, 2, 2, 4, false},   // 128 x 96, 4 compute waves of 64 x 48 + 4 loader waves
    {24, GF_L,      4, 2, 1, 2, 3, 2, true},    // 64 x 48, 6 compute + 2 loader waves (the skinny shape 11 on the loader-wave kernel)
    {25, GF_L,      5, 2, 3, 4, 2, 4, false},   // shape 20 with a 5-stage ring (140 KiB)
    {26, GF_L,      4, 2, 2, 2, 3, 2, true},    // 64 x 96, 6 compute + 2 loader waves (shape 14 likewise)
    {27, GF_L,      8, 2, 1, 2, 3, 2, false},   // shape 24 with an 8-stage ring (112 KiB): seven K-steps of W in flight per CU
    {28, GF_L,      8, 2, 1, 2, 3, 4, false},   // ... and four loader waves
    // 128 x 144 (nine 16-token groups: one 144-token frame per row tile), 12 compute waves of 32 x 48 + 4 loader waves (round 4): M = 1152, the context-cached
    // step at batch 8, is 8 x 32 = 256 tiles for fc1 / 4-slice fc2 where the 128 x 128 grid has 288 (1.1 rounds)
    {29, GF_L,      4, 2, 3, 4, 3, 4, true},
    {30, GF_LP,     4, 4, 3, 2, 4, 4, false},   // shape 31 with a 4-stage ring
    {31, GF_LP,     3, 4, 3, 2, 4, 4, true},    // persistent loader-wave kernel: 128 x 192 tiles, 3-stage ring, 8 compute + 4 loader waves
    {32, GF_LP,     3, 4, 4, 4, 2, 4, false},   // 256 x 128
    {33, GF_LP,     3, 4, 4, 2, 4, 4, false},   // 128 x 256
    {40, GF_LAB,    2, 8, 4, 2, 4, 0, false},   // persistent 256 x 256 tiles
    {41, GF_LAB,    2, 6, 4, 2, 4, 0, false},   // persistent 192 x 256 (N x M)
    {42, GF_LAB,    2, 4, 4, 4, 4, 0, false},   // persistent 256 x 256 tiles on sixteen waves of 64 x 64
};
// (Shapes 4, 5, 6, 10 of round 1 — 128x256, loader-wave variants, 4-wave 128x192 — measured slower and were removed.)

// the row of a shape, nullptr for an unknown id (as a template argument that does not compile)
constexpr const GemmShape* gemm_shape(int id) {
    for (const GemmShape& s : GEMM_SHAPES)
        if (s.id == id) return &s;
    return nullptr;
}
inline int gemm_tiles(int shape, int M, int N) {   // of a shape that exists
    const GemmShape& s = *gemm_shape(shape);
    return ((M + s.tokens() - 1) / s.tokens()) * ((N + s.features() - 1) / s.features());
}

// What launch_gemm asks about: plain integers.
// epi: extended epilogue code (gemm.h GemmEpi, the LayerNorm-fold ones included); qkv_mode, S: EPI_QKV; splitk: the caller's K slices (honoured for EPI_PARTIAL
// only, like launch_gemm); rows_per_gate: EPI_RESID, tokens per gate vector, 0 = no gate
struct GemmProblem { int M, N, K, epi, qkv_mode, S, splitk, rows_per_gate; };
// shape: GEMM_SHAPES id; ns: ring depth request, the forced stages, else 2 or 4 (GF_K128 picks its instantiation by it; the other kernels carry theirs in the
// row); splitk: K slices of the grid; gn: width in n-panels of the tile groups of the block -> tile map; blocks: tiles x K slices (a persistent kernel launches
// min(blocks, CUs)).  The eight integers gtav_op_gemm_plan reports, in this order.
struct GemmPlan { int shape, ns, splitk, gn, tile_tokens, tile_features, blocks, threads; };

// GTAV_LAB_BUILD (common.h): true in a translation unit built with -DGTAV_EXPERIMENTS — the planner's environment knobs and debug bits apply to its calls;
// false in the product objects and in the bf16 twins of BOTH libraries (never built with it): the heuristic and the test overrides only
constexpr bool GEMM_LAB_BUILD = GTAV_LAB_BUILD;

// Returns 0 and the plan, or 2 with the error string set: an unknown forced shape, one that exists in the experiments build only (product library, or a
// caller with lab = false), or spatial QKV on the 96-feature tile.
int gemm_plan(const GemmProblem& g, GemmPlan* plan, bool lab = GEMM_LAB_BUILD);
// Width (in n-panels) of the tile groups for a tmb x tnb (tokens x features) tile; the launchers outside the plan (fused to_qkv + attention, gemm_tn) ask too.
int gemm_choose_gn(int M, int N, int K, int tmb, int tnb, int splitk, bool lab = GEMM_LAB_BUILD);
// True when launch_gemm would run this shape on the persistent ping-pong kernel (large M): residual GEMMs then use the in-place
// EPI_RESID epilogue (hidden under the other wave group's main loop) instead of split-K slabs.  Always false in the product library.
bool gemm_pp_ok(int M, int N, int K, int epi, bool lab = GEMM_LAB_BUILD);
// True when launch_gemm runs a residual GEMM of this shape on the persistent loader-wave kernel (shape 31, large M), whose in-place gated residual epilogue
// (EPI_RESID: the residual tile is requested at the head of the tile's K loop) replaces slab + LayerNorm reduction.
bool gemm_resid_inplace_ok(int M, int N, int K, int rows_per_gate, bool lab = GEMM_LAB_BUILD);
// Split-K factor used for a residual GEMM of this shape (1 = no split): fills the 256 CUs when M is small.
int gemm_choose_splitk(int M, int N, int K, bool lab = GEMM_LAB_BUILD);

// Test overrides, PER THREAD like the handles and ONE set for both operand types: a test that forces a shape does not change what another thread's handle launches.
// Pipeline depth override (0 = heuristic, else 2 or 4 LDS stages).
void gemm_set_stages(int ns);
// Block shape override (0 = heuristic; GEMM_SHAPES ids).  Every shape computes the same result.  Bit 8 (+ 0x100, with any shape or with 0):
// every loader-wave launch of the thread fills its W operand non-temporally (GemmParams::wfill), whatever the caller's params say.  The same result again.
void gemm_set_wm(int wm);
bool gemm_forced_wfill();
// Debug bits of the laboratory (skip fills / skip MFMA: WRONG results, timing only; selection A/B bits): 0 in the product library and for callers with lab = false.
int gemm_debug(bool lab = GEMM_LAB_BUILD);
void gemm_set_debug(int bits);   // experiments library only: timing experiments, WRONG results

}  // namespace gtav_shared
