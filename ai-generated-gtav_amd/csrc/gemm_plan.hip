// The GEMM planner (gemm_plan.h): the measured rules that pick a block shape, its K slices and its tile-group width.  Host code only, built once per library.
#include "gemm.h"   // gemm_plan.h, the epilogue codes, cdiv, GTAV_REQUIRE

#include <cstdlib>

namespace gtav_shared {
using namespace gtav;   // EPI_*, QKV_*, cdiv

// ---- per-thread test overrides ----
static thread_local int t_force_stages = 0, t_force_shape = 0, t_force_wfill = 0;
// GTAV_GEMM_SHAPE (experiments build; 0 in the product): a forced shape for whole-bench A/B runs, until gemm_set_wm replaces it; never handed to a caller that is not a laboratory build
static thread_local int t_env_shape = GTAV_ENV_INT("GTAV_GEMM_SHAPE", 0);
void gemm_set_stages(int ns) { t_force_stages = ns; }
void gemm_set_wm(int wm) { t_force_shape = wm & 0xFF; t_force_wfill = wm >> 8 & 1; t_env_shape = 0; }
bool gemm_forced_wfill() { return t_force_wfill != 0; }
static int forced_shape(bool lab) { return t_force_shape ? t_force_shape : lab ? t_env_shape : 0; }

// ---- laboratory overrides: the one place where the environment and the debug bits reach the selection (experiments build, callers with lab = true) ----
struct LabKnobs {
    int debug = 0;           // GTAV_GEMM_DEBUG / gemm_set_debug.  Selection bits: 6 = round-1 shapes, 7 = shape 25 for 20, 8 = full-K residual GEMMs, 10 = round-1 group width,
                             // 21 / 22 = persistent 128 x 256 / 256 x 128 tiles for fc1, 24 / 25 = shapes 22 / 18 for 20
    int lp = 1;              // GTAV_LP: 0 = round-2 selection, for A/B runs
    int resid_inplace = 1;   // GTAV_RESID_INPLACE: 0 = slab + LayerNorm reduction at every M (A/B runs)
    int splitk_old = 0;      // GTAV_SPLITK_OLD: A/B
    int l_for_8 = 1;         // GTAV_L_FOR_8: 0 keeps the 96 x 96 tile (shape 8) where the cost model picks it
    int gn = 0;              // GTAV_GEMM_GN: > 0 forces the group width, < 0 = round-1 rule (A/B runs)
    int pp = 0;              // GTAV_PP: 1 = the ping-pong kernel (shape 16) where gemm_pp_ok
};
static const LabKnobs g_lab_off = {};
#ifdef GTAV_EXPERIMENTS
static LabKnobs g_lab = {GTAV_ENV_INT("GTAV_GEMM_DEBUG", 0), GTAV_ENV_INT("GTAV_LP", 1), GTAV_ENV_INT("GTAV_RESID_INPLACE", 1), GTAV_ENV_INT("GTAV_SPLITK_OLD", 0),
                         GTAV_ENV_INT("GTAV_L_FOR_8", 1), GTAV_ENV_INT("GTAV_GEMM_GN", 0), GTAV_ENV_INT("GTAV_PP", 0)};
static const LabKnobs& knobs(bool lab) { return lab ? g_lab : g_lab_off; }
void gemm_set_debug(int bits) { g_lab.debug = bits; }
// Round-2 measurement (profiles/round2/pp_stamps_v1.txt): correct and bit-identical to the one-shot kernels, the overlap works (MAIN
// phases run back to back), but with only 8 of the 16 waves computing, a K-step costs 1.15-1.25 us against 0.68 us of fill time: the
// barrier-synchronised waves serialise into fill / read / MFMA phases, where two independent co-resident blocks interleave them.
// fc1 at M = 5760: 71-76 us against 57 us for shape 12.  Not selected by the heuristic (GTAV_PP=1 in the experiments build or a
// forced shape 16 run it); the de-phased shape 12 above gets the same overlap with 16 computing waves.
bool gemm_pp_ok(int M, int N, int K, int epi, bool lab) {
    if (!(epi == EPI_GELU_TANH || epi == EPI_GELU_ERF || epi == EPI_QKV || epi == EPI_RESID)) return false;
    if (K % GEMM_TK != 0 || K / GEMM_TK < 14 || M % 8 != 0 || N % 8 != 0) return false;
    // worth it when most CUs get a tile and, beyond one tile per CU, the epilogue of one tile hides under the next tile's main
    // loop (otherwise the one-shot kernels with smaller tiles cover the chip better)
    return knobs(lab).pp && gemm_tiles(16, M, N) >= 224;
}
// the laboratory's stand-ins for shape 20, wherever the heuristic picks it
static int lab_shape_for_20(const LabKnobs& k, bool foldish, int ksteps) {
    int wm = (k.debug & 128) ? 25 : 20;
    // round 6 A/B (debug bit 24): the 128 x 96 loader-wave tile with the weight operand straight into registers (shape 22) wherever the heuristic picks shape 20
    if (wm == 20 && (k.debug & 0x1000000) && !foldish && ksteps % 4 == 0) wm = 22;
    if (wm == 20 && (k.debug & 0x2000000) && !foldish && ksteps % 8 == 0) wm = 18;   // debug bit 25: shape 18
    return wm;
}
// A/B of the persistent 128 x 256 / 256 x 128 tiles for fc1 (debug bits 21 / 22)
static int lab_shape_for_fc1(const LabKnobs& k, int wm, int epi_x, int M, int N) {
    if (epi_x == EPI_GELU_TANH && (k.debug & 0x600000) && cdiv(M, 128) * cdiv(N, 256) >= 512) return (k.debug & 0x200000) ? 33 : 32;
    return wm;
}
#else
static const LabKnobs& knobs(bool) { return g_lab_off; }
bool gemm_pp_ok(int, int, int, int, bool) { return false; }   // the ping-pong kernel (shape 16) is compiled into the experiments build only (gemm_experiments.inc)
static int lab_shape_for_20(const LabKnobs&, bool, int) { return 20; }
static int lab_shape_for_fc1(const LabKnobs&, int wm, int, int, int) { return wm; }
#endif
int gemm_debug(bool lab) { return knobs(lab).debug; }

// The persistent loader-wave kernel (shape 31) takes the narrow residual GEMMs (N <= 2048: out-proj, fc2) in ONE K slice once its 128 x 192 tiles cover
// most of the chip (>= 160 tiles): measured against the heuristic's own choice, split-K included (profiles/round3/persistent_loader_kernel_vs_heuristic_*.txt) —
// M = 4320: out-proj 17.2 -> 13.2 us, fc2 47.1 -> 36.3 us; M = 5760: 17.5 -> 14.3, 51.0 -> 45.1; M = 8640: 27.5 -> 24.0, 78.6 -> 75.0; M = 11 520: 27.9 -> 25.1,
// 87.6 -> 84.5; at 120 tiles (M = 2880) it loses (12.0 -> 12.8, 31.7 -> 34.0) and the split-K shapes stay.  One slab also halves what the LayerNorm behind fc2 reads.
static bool lp_takes(int M, int N, int K, bool lab) { return knobs(lab).lp && N <= 2048 && N % 8 == 0 && K >= 512 && gemm_tiles(31, M, N) >= 160; }
// (rows_per_gate: tokens per gate vector — the persistent kernel stages at most LP_MAXF gate rows per 192-token tile; 0 = no gate.  A forced block shape
// other than 31 (tests) runs the one-shot kernels, where the in-place epilogue was measured slower than slab + LayerNorm: keep the slabs then.)
bool gemm_resid_inplace_ok(int M, int N, int K, int rows_per_gate, bool lab) {
    const int forced = forced_shape(lab);
    return knobs(lab).resid_inplace && lp_takes(M, N, K, lab) && (rows_per_gate == 0 || rows_per_gate >= 32) && (forced == 0 || forced == 31);
}
int gemm_choose_splitk(int M, int N, int K, bool lab) {
    if (lp_takes(M, N, K, lab)) return 1;
    if (knobs(lab).debug & 256) return 1;   // A/B with GTAV_RESID_INPLACE_MIN_M=1: full-K residual GEMMs on 64 x 48 tiles + in-place epilogue (measured slower, profiles/round2/forward_ab_B1_inplace_fullK.txt)
    const int tiles = gemm_tiles(3, M, N);
    int s = 1;
    // Every slab is one more 16-byte load per thread in the LayerNorm behind the GEMM (~0.4 us per slab and launch at M = 720) and 3 MB more through the L2s that
    // hold the next GEMM's prefetched weight: from 48 tiles on (the batch-1 window step) a K slice is at least 512 deep — out-proj in two slices instead of four:
    // GEMM unchanged (6.7-7.0 us), LayerNorm 5.45 -> 4.7 us, forward -1.3 ... -3 % (profiles/round3/forward_ab_B1_splitk_slices.txt); fc2 keeps four slices of 1024
    // (two: +1.6 us).  Below 48 tiles (the 144-token cached step) the CUs matter more: 256 as before.
    const int min_slice = (tiles >= 48 && !knobs(lab).splitk_old) ? 512 : 256;
    while (tiles * s < 192 && s < 8 && (K / GEMM_TK) % (s * 2) == 0 && K / (s * 2) >= min_slice) s *= 2;
    // long-K GEMMs whose 128 x 192 grid would fill the 512 block slots unevenly (160-320 tiles): two K slices make it
    // 320-640 blocks of half the length — fc2 at M = 5760: 69.5 -> 57.6 us, for one more slab (+5 us) in the next LayerNorm
    if (s == 1 && K >= 4096 && (K / GEMM_TK) % 2 == 0) {
        const int t192 = gemm_tiles(12, M, N);
        if (t192 >= 160 && t192 < 320) s = 2;
    }
    return s;
}

// Width (in n-panels) of the tile groups of the block -> tile map (tile_map): the linear tile order is (K slice, group of gn
// n-panels, m-tile, panel in group) and every XCD takes a contiguous eighth of it.  One pass over a group streams the K slice of X
// once (its co-resident blocks share X row-tiles and W panels in the XCD's L2), so with G = tiles_n / gn groups and C = 8 / splitk
// XCDs per K slice the fabric sees  G x X  +  max(1, C / G) x W  bytes per slice: narrow groups re-stream X, wide groups make
// several XCDs fetch the same W panels.  Pick the minimum, with the W panels of a group capped at 2 MiB (they must survive in the
// 4 MiB L2 while the group's m-tiles sweep past).  Round 1's fixed gn = tiles_n / 8 is the G = 8 corner: right at M = 720 (X is
// small), 3.5x too much traffic for the N = 1024 GEMMs at M = 5760.
int gemm_choose_gn(int M, int N, int K, int tmb, int tnb, int splitk, bool lab) {
    const LabKnobs& k = knobs(lab);
    const int tiles_n = cdiv(N, tnb);
    if ((k.debug & 1024) || k.gn < 0) return tiles_n >= 8 ? tiles_n >> 3 : 1;   // debug bit 10: round-1 rule, for A/B runs in one process
    if (k.gn > 0) return k.gn < tiles_n ? k.gn : tiles_n;
    const double ks = (double)K / (splitk > 0 ? splitk : 1);
    const double xs = 2.0 * M * ks, ws = 2.0 * N * ks, wpanel = 2.0 * tnb * ks;
    const double c = splitk >= 8 ? 1.0 : 8.0 / (splitk > 0 ? splitk : 1);
    auto cost_of = [&](int gn) {
        const int g = cdiv(tiles_n, gn);
        return g * xs + ws * (c > g ? c / g : 1.0);
    };
    int best = 1;
    double best_cost = 1e300;
    // the 2 MiB cap protects W panels that must SURVIVE in L2 while further m-tiles of the group sweep past; a grid that is resident all at
    // once (<= 512 block slots) has no sweep — its blocks walk K in step and share the current K window only — so the cap does not apply
    // (weight gradients of the training step, K = 11 520 tokens: a 2.9 MB W panel forced gn = 1 = every XCD streaming ALL of the 94 MB X
    // operand, 778 MB per launch at 7 TB/s; uncapped gn = 4: 282 MB)
    const bool one_round = (long long)cdiv(M, tmb) * tiles_n * (splitk > 0 ? splitk : 1) <= 512;
    for (int gn = 1; gn <= tiles_n; ++gn) {
        if (!one_round && gn > 1 && gn * wpanel > 2.0 * 1024 * 1024) break;
        const double cost = cost_of(gn);
        if (cost < best_cost * 0.999) best_cost = cost, best = gn;   // ties keep the narrower group (more XCD-local W)
    }
    // The model ignores how the groups line up with the XCDs' runs of tiles: where it predicts less than a 20 % saving keep round 1's
    // eighth-of-the-panels groups, which do line up (fc1 at M = 720: gn = 5 instead of 4 was predicted 1 % better and measured
    // 34.1 MB per launch against 27.4 MB)
    const int gn1 = tiles_n >= 8 ? tiles_n >> 3 : 1;
    if (best_cost > 0.8 * cost_of(gn1)) best = gn1;
    return best;
}

// The rules, in the order they were measured in; each may replace what the ones before it picked.
static int heuristic_shape(const GemmProblem& g, int splitk, bool lab) {
    const LabKnobs& k = knobs(lab);
    const int M = g.M, N = g.N, K = g.K, epi_x = g.epi, epi = epi_base(epi_x);
    const bool fold_p = epi_x == EPI_RESID_FOLD, foldish = fold_p || epi_is_fold_consumer(epi_x);
    const bool spatial_qkv = epi == EPI_QKV && g.qkv_mode == QKV_SPATIAL;
    auto tiles = [&](int shape) { return gemm_tiles(shape, M, N) * splitk; };
    // Block shape (measured, profiles/round1/v6_gemm_shapes_microbench.txt):
    //   grid < 256 blocks of 128 x 128 (one block per CU at most): 8 waves per block (two staggered waves per SIMD),
    //     4-stage ring — 17-25 % faster than 4 waves at M = 720;
    //   larger grids: 4 waves, 2-stage ring, two co-resident blocks per CU; the 128 x 256 / 8-wave tile (shape 4) ties it.
    const int blocks128 = tiles(3);
    int wm = blocks128 <= 256 ? 3 : 2;
    if (blocks128 <= 256) {
        // small M: every block is bound by its own L2->LDS fill (~65 GB/s per CU), i.e. by (TN + TM) x K bytes, and the grid
        // by how many of the 256 CUs it covers.  Candidates: 128 x 128 (shape 3), 128 x 96 (shape 9), 96 x 96 (shape 8).
        auto cost = [&](int shape) { return cdiv(tiles(shape), 256) * (gemm_shape(shape)->features() + gemm_shape(shape)->tokens()); };
        int best = cost(3);
        if (cost(9) < best) best = cost(9), wm = 9;
        const bool ok96 = N % 96 == 0 && epi != EPI_GELU_TANH && epi != EPI_GELU_ERF && epi != EPI_F16_TILED && !spatial_qkv;
        if (ok96 && cost(8) < best) best = cost(8), wm = 8;
        // skinny M (M = 144: the context-cached sampler step): 64 x 48 tiles put 144-192 blocks of 224 KB where the
        // 128 x 96 grid has 48-64 blocks of 448 KB
        if (cost(14) < best) best = cost(14), wm = 14;   // M = 288-320 (g256 window step, batch-2 cached step)
        if (cost(11) < best) best = cost(11), wm = 11;
    }
    // Round 2: the 128 x 96 tile runs on the loader-wave kernel (shape 20: 4 loader + 8 compute waves, fills and MFMAs overlap by
    // construction): QKV 14.1 -> 10.7 us, fc1 13.3 -> 10.9, fc2 12.0 -> 10.2, out-proj 6.6 -> 6.1 at M = 720 (profiles/round2).
    if (!(k.debug & 64) && (wm == 9 || (wm == 8 && k.l_for_8))) wm = lab_shape_for_20(k, foldish, K / GEMM_TK / splitk);   // debug bit 6 (experiments build): round-1 shapes, for A/B runs in one process
    // Round 3: the skinny tiles on the loader-wave kernel too (6 compute + 2 loader waves): M = 144 QKV 8.45 -> 7.34 us, fc1 7.75 -> 6.83, out-proj 5.00 -> 4.68;
    // M = 288 QKV 10.3 -> 8.4, fc1 9.7 -> 8.4 (profiles/round3/skinny_loader_wave_shapes_M144_M288.txt); their compute waves carry the next-weight L2 prefetch.
    // The 8-slice fc2 at M = 288 stays on the all-waves-fill kernel (7.4 against 8.3 us).
    if (!(k.debug & 64)) {
        if (wm == 11) wm = 24;
        else if (wm == 14 && !(epi_x == EPI_PARTIAL && splitk >= 8)) wm = 26;
    }
    // Round 4: a little over a thousand tokens (M = 1152: the context-cached step at batch 8) sits between the small-M tiles (128 x 96: 12 row tiles, 1.1-1.5
    // rounds of one-block-per-CU tiles) and the large-M ones (128 x 128, two blocks per CU: 216-288 blocks on 512 slots).  128 x 144 tiles on the loader-wave
    // kernel (shape 29) are one round there: to_qkv 192, fc1 256, four-slice fc2 256 tiles (profiles/round4/step_B8_cached_*.json: to_qkv 14.9, fc1 18.5, fc2 19.7 us before).
    bool frame_tile = false;
    if (!foldish && !(k.debug & 64)) {
        const int t29 = tiles(29), t20 = tiles(20);
        if (t29 > 128 && t29 <= 256 && t20 > 256 && blocks128 <= 320) wm = 29, frame_tile = true;
    }
    if (wm == 2 && tiles(12) >= 320) {
        // large M: 128 x 192 tiles (4 waves of 64 x 96, still two blocks per CU) move 17 % fewer fill bytes per FLOP than
        // 128 x 128: QKV 62.6 -> 55.5 us, fc1 63.8 -> 61.1 us at M = 5760 (profiles/round1/v17_gemm_128x192_microbench.txt);
        // below ~320 tiles the 512 block slots are too unevenly filled (fc2 at M = 5760: 240 tiles, 65.7 -> 73.1 us).
        wm = 12;   // 8 waves of 64 x 48 (four per SIMD with the co-resident block): QKV 60.3 -> 54.8, fc1 62.1 -> 59.4 vs the 4-wave form (shape 10)
    }
    // Narrow outputs (the N = 1024 residual GEMMs) at a few thousand tokens: both two-blocks-per-CU tiles, 128 x 192 (shape 12) and 128 x 96
    // (shape 13), run a grid that FILLS the 512 block slots once faster than 128 x 128 runs 360-720 blocks: out-proj at M = 5760 20.6 -> 16.8 us
    // (shape 13: 480 tiles), at M = 11 520 33.4 -> 30.8 us and fc2 97.6 -> 90.2 us (shape 12: 480 tiles; the 256 x 256 tile lost to it),
    // M = 2880 out-proj 13.7 -> 11.4 us, fc2 34.6 -> 27.9 us (shape 13, two K slices) — profiles/round3/gemm_shapes_*.txt.  The LayerNorm-fold
    // producer takes the larger tile whenever its grid is more than half full (27.2 us against 33.5 us at M = 5760).
    bool narrow_pick = false;
    if (!frame_tile && blocks128 > 256 && N <= 2048 && epi != EPI_QKV) {
        const int t12 = tiles(12), t13 = tiles(13);
        if (t12 > 256 && t12 <= 512) wm = 12, narrow_pick = true;
        else if (t13 > 256 && t13 <= 512 && !fold_p) wm = 13, narrow_pick = true;
        else if (fold_p && t12 > 128) wm = 12, narrow_pick = true;
    }
    if (splitk == 1 && ((epi_x == EPI_PARTIAL && lp_takes(M, N, K, lab)) || (epi_x == EPI_RESID && gemm_resid_inplace_ok(M, N, K, g.rows_per_gate, lab)))) wm = 31, narrow_pick = true;
    // Tens of thousands of tokens (the VAE encode of a training batch: M = 46 080): the in-place residual GEMMs on whole rounds of 256 x 256 tiles
    // (>= 2 rounds, >= 90 % full) beat the persistent 128 x 192 kernel — fc2 453 -> 399 us, attention projection 182 -> 164 us back to back
    // (profiles/round5/gemm_vae_shapes_M23040_M46080.txt); at M = 23 040 (1.4 rounds) they lose (240 against 223 us) and shape 31 stays
    if (wm == 31 && epi_x == EPI_RESID && N % 256 == 0 && N <= 1024 && K >= 1024) {
        const int t256 = tiles(7), rounds = cdiv(t256, 256);
        if (rounds >= 2 && t256 * 10 >= rounds * 256 * 9) wm = 7;
    }
    wm = lab_shape_for_fc1(k, wm, epi_x, M, N);
    // large M: the persistent ping-pong kernel (epilogue and next tile's prologue under the other wave group's MFMAs)
    if (splitk == 1 && gemm_pp_ok(M, N, K, epi, lab) && !(spatial_qkv && g.S % 8 != 0)) wm = 16;
    // 256 x 256 tiles (shape 7) halve the fill bytes per FLOP but run one block per CU, so a tile's epilogue (a 32 MB
    // store burst per round of 256 tiles) is not hidden by a co-resident block: they win only where the K loop is long
    // relative to the output and the grid is one well-filled round — the N = 1024 residual GEMMs at M >= 11 520
    // (profiles/round1/v12_gemm_256tile_microbench.txt: fc2 129 -> 98 us, out-proj 40 -> 35 us).
    if (splitk == 1 && epi != EPI_QKV && !foldish && !narrow_pick && N % 256 == 0 && N <= 1024 && K >= 1024) {
        const int t256 = tiles(7), rounds = cdiv(t256, 256);
        if (t256 * 10 >= rounds * 256 * 7) wm = 7;
    }
    return wm;
}

int gemm_plan(const GemmProblem& g, GemmPlan* plan, bool lab) {
    const int splitk = g.epi == EPI_PARTIAL ? g.splitk : 1;
    GTAV_REQUIRE(g.M > 0 && g.N > 0 && g.K > 0 && splitk >= 1, "gemm: bad M=%d N=%d K=%d splitk=%d", g.M, g.N, g.K, splitk);
    const int forced = forced_shape(lab);
    const int wm = forced ? forced : heuristic_shape(g, splitk, lab);
    const GemmShape* s = gemm_shape(wm);
    GTAV_REQUIRE(s, "gemm: unknown block shape %d", wm);
    GTAV_REQUIRE(s->product || (lab && GEMM_LAB_BUILD), "gemm: block shape %d exists only in the experiments build (csrc/build.sh exp)", wm);
    GTAV_REQUIRE(!(wm == 8 && epi_base(g.epi) == EPI_QKV && g.qkv_mode == QKV_SPATIAL), "gemm: 96-feature tiles straddle the K / V boundary (spatial QKV)");
    int gn = gemm_choose_gn(g.M, g.N, g.K, s->tokens(), s->features(), splitk, lab);
    // A narrow output with far more activations than weights (the VAE's fc2 at M = 46 080: X 377 MB, W 8 MB): keep ALL n-tiles of an m-tile on one XCD,
    // beyond choose_gn's 2 MiB cap — X then crosses the fabric once and W, which stays in the Infinity Cache, is what gets re-read: 1.94 GB -> less per
    // launch by the PMC counters (profiles/traffic.json vae_fc2), 426 -> 408 us (profiles/round5/gemm_tile_group_width_large_M.txt)
    if (s->family == GF_T256 && !knobs(lab).gn && splitk == 1 && g.N <= 1024 && (size_t)g.M >= 8 * (size_t)g.N) gn = cdiv(g.N, s->features());
    const int ns = t_force_stages ? t_force_stages : ((wm == 12 || wm == 13) ? 2 : wm >= 8 ? 4 : wm == 3 ? 4 : 2);   // (shapes 20+ carry their ring depth in the template)
    *plan = GemmPlan{wm, ns, splitk, gn, s->tokens(), s->features(), gemm_tiles(wm, g.M, g.N) * splitk, s->threads()};
    return 0;
}

}  // namespace gtav_shared
