// Laboratory half of gemm.hip: compiled ONLY into libgtav_amd_exp.so (csrc/build.sh exp, -DGTAV_EXPERIMENTS), included by gemm.hip right in front of
// launch_epi.  Everything here measured slower than what launch_gemm's heuristic picks and is kept for A/B runs of the tools under tools/ (forced block
// shapes, GTAV_* environment overrides):
//   * kernels of their own: the persistent 256-token tiles with a K split of the remainder (gemm_p256_kernel, shapes 40 / 41, round 4), the persistent ping-pong
//     kernel (gemm_pp_kernel, shape 16, round 2), the 256 x 256 persistent tile on sixteen waves in two groups (gemm_s16_kernel, shape 42), the antiphase
//     256 x 256 main loop (mainloop256_pp / gemm256_pp_kernel, shape 17, round 6) and the loader-wave kernel with the weight operand straight into registers
//     (mainloop_lw / gemm_lw_kernel / launch_lw, shapes 22 / 18, round 6);
//   * further instantiations of the product's kernels: 8 / 9 (96-wide tiles of round 1), 21 / 23 / 25 / 27 / 28 (loader-wave variants), 30 / 32 / 33 (persistent
//     loader-wave variants).
// launch_experiment_shape, at the end, is the one hook launch_epi calls.  The product library (libgtav_amd.so) contains none of it and refuses these seventeen
// shape numbers in one place (launch_epi).
#pragma once
namespace {
// ---------------------------------------------------------------------------------------------------------------------
// Persistent 256-token tiles for large M (shape 40 / 41, round 4; docs/LABNOTES.md 4.11).
//
// mainloop256's K-tile (four quadrant phases of FI x 2 MFMAs, half-tile fills interleaved, two barriers) is the most efficient K-step of this file —
// 1.39 us for 8.4 MFLOP per CU = 0.62 of the MFMA peak in steady state, against 0.47 for the 128 x 192 loader-wave tile — but as a one-shot kernel it
// paid a prologue per tile and a whole round for any remainder of tiles (360 tiles on 256 CUs at M = 5760: 2 rounds for 1.41 rounds of work).  Here:
//   * ONE block of 8 waves per CU walks a sequence of work units; the two-parity LDS ring never drains — the W half-tiles of the next unit's first K-tile and
//     the X half-tiles of its first two are issued during the last K-tiles of the current unit, so only the first unit of a block pays a prologue;
//   * the epilogue runs straight from the accumulators (pairs of lanes exchange halves: every store is 16 bytes; bias through a 1 KiB LDS slice), the ring
//     is not touched, and the stores drain under the next unit's K loop;
//   * tiles are dealt in whole rounds (tile t on block t % grid); a remainder of r <= grid / 2 tiles is split in two K halves over 2 r blocks.  Block
//     2 i + 1 runs the K TAIL of tile dp + i FIRST in its sequence and hands its partial sums over (fp32, register layout, sk_ws); block 2 i runs the K HEAD
//     LAST, adds the partial tile and owns the epilogue — by then the partial has been waiting for a whole round, nobody spins in practice.  Hand-off:
//     plain stores -> every wave vmcnt(0) -> barrier -> one agent-scope release -> flag; relaxed poll -> one agent-scope acquire -> barrier -> plain loads
//     (MI355X_MICROARCH.md, inter-workgroup visibility); the flag is reset by its consumer, so it is zero between launches (graph replays included).
// FI = feature groups of 16 per wave: 8 -> 256-feature tiles, 6 -> 192 (3072 = 16 x 192: 368 instead of 276 tile slots at M = 5760).
// Fill addresses are wave-uniform (SGPR) bases + one per-lane offset (glds16_s): the kernel sits at the 256-register limit like gemm256_kernel.
// ---------------------------------------------------------------------------------------------------------------------
template <int FI>
struct P256 {
    static constexpr int TNB = 32 * FI, NWP = TNB / 8, NWQ = NWP / 8, NWQ0 = (NWQ + 1) / 2;   // W pieces (1 KiB = 8 rows) per K-tile, per wave, in phase 1
    static constexpr int WREG = NWP * 1024, PAR = WREG + 32 * 1024;                            // LDS bytes of the W region / of one parity (W + 256 X rows)
    static constexpr int BIAS_OFF = 2 * PAR, LDS = 2 * PAR + TNB * 4 + 16 * 8 * 4;   // ring, bias slice, unit list
};
struct P256Unit { int n0, m0, kt0, nkt, kind, slot; };   // kind 0: whole tile; 1: K tail of a split tile (partial sums out); 2: K head (partial sums in, owns the epilogue)

template <int FI>
__device__ __forceinline__ P256Unit p256_unit(const GemmParams& p, int u, int tiles_m, int tiles_n, int nktot) {
    const int G = gridDim.x, b = blockIdx.x;
    const bool split = b < 2 * p.sk_r, helper = split && (b & 1);
    const int n_dp = b < p.sk_dp ? (p.sk_dp - b + G - 1) / G : 0;
    const int d = u - (helper ? 1 : 0);
    P256Unit r;
    r.kt0 = 0; r.nkt = nktot; r.kind = 0; r.slot = 0;
    int v;
    const int kh = (nktot >> 1) & ~1;   // split point: both halves hold an even number of K-tiles (the K loop advances by pairs)
    if (helper && u == 0) { v = p.sk_dp + (b >> 1); r.kind = 1; r.slot = b >> 1; r.kt0 = kh; r.nkt = nktot - kh; }
    else if (d < n_dp) v = b + d * G;
    else { v = p.sk_dp + (b >> 1); r.kind = 2; r.slot = b >> 1; r.nkt = kh; }
    lp_tile_of(p, v, tiles_m, tiles_n, 32 * FI, 256, r.n0, r.m0);
    return r;
}

constexpr int P256_MAXU = 16;   // work units per block (whole rounds + one split piece): host-checked
template <int EPI, int FI>
__global__ __launch_bounds__(512, 1) void gemm_p256_kernel(GemmParams p) {
    using C = P256<FI>;
    constexpr int FIH = FI / 2, NWQ = C::NWQ, NWQ0 = C::NWQ0, TNB = C::TNB;
    static_assert(FI == 8 || FI == 6, "256- or 192-feature tiles");
    static_assert(EPI == EPI_F32 || EPI == EPI_PARTIAL || EPI == EPI_GELU_TANH || EPI == EPI_F16_TILED, "epilogues of the persistent 256-token-tile kernel");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = w & 1, wm = w >> 1;
    const int nktot = p.K / TK;
    const int G = gridDim.x, b = blockIdx.x;
    const bool split = b < 2 * p.sk_r;
    const int n_dp = b < p.sk_dp ? (p.sk_dp - b + G - 1) / G : 0;
    const int nunits = n_dp + (split ? 1 : 0);
    if (nunits == 0) return;
#ifdef GTAV_EXPERIMENTS   // per-block timeline of the FIRST unit (tools/gemm_stamps.py): entry, first K-tile landed, main loop done, epilogue done; slot 7 = block end
#define P256_STAMP(i) do { if (p.stamps && tid == 0) p.stamps[(size_t)blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
    if (p.stamps && tid == 0) { p.stamps[(size_t)blockIdx.x * 8 + 4] = __builtin_amdgcn_s_memtime(); }
#else
#define P256_STAMP(i) do { } while (0)
#endif
    P256_STAMP(0);
    const int S = n_dp * nktot + (split ? ((b & 1) ? nktot - ((nktot >> 1) & ~1) : ((nktot >> 1) & ~1)) : 0);   // K-tiles of this block (even)
    const int last_wt = ((p.N + 127) >> 7) - 1, last_rt = (p.M - 1) >> 7;
    const unsigned voff = (unsigned)lane * 16u, smem0 = lds_offset(smem);
    // ---- the block's unit list, decoded ONCE (one unit per thread: the tile map's integer divisions stay out of the K loop) into LDS ----
    int* const ut = (int*)(smem + C::BIAS_OFF + TNB * 4);
    if (tid < nunits) {
        const P256Unit un = p256_unit<FI>(p, tid, (p.M + 255) >> 8, (p.N + TNB - 1) / TNB, nktot);
        int* q = ut + 8 * tid;
        q[0] = un.n0; q[1] = un.m0; q[2] = un.kt0; q[3] = un.nkt; q[4] = un.kind; q[5] = un.slot;
    }
    __syncthreads();
    auto unit_field = [&](int u, int f) { return __builtin_amdgcn_readfirstlane(ut[8 * u + f]); };

    // ---- fill cursors: the next W K-tile / X K-tile to issue (they run one / two K-tiles ahead of the MFMAs, across unit boundaries) ----
    int wu = 0, wk = 0, wi = 0, wnk, xu = 0, xk = 0, xi = 0, xnk;
    // piece sources as 32-bit byte offsets from the operand's base (host-checked: both operands are smaller than 4 GiB): one SGPR per piece, and the
    // fill address is SGPR base + (per-lane offset + wave-uniform offset) — eight 64-bit bases did not fit the scalar file beside the rest of the kernel
    unsigned wso[NWQ], xso[4];
    auto setW = [&](int u) {
        const int n0 = unit_field(u, 0), kt0 = unit_field(u, 2);
        wnk = unit_field(u, 3);
#pragma unroll
        for (int i = 0; i < NWQ; ++i) {
            const int row = n0 + 8 * (w + 8 * i);
            int rt = row >> 7;
            rt = rt < last_wt ? rt : last_wt;                 // ragged edges re-read a valid tile (results are masked)
            wso[i] = (unsigned)(rt * nktot + kt0) * (unsigned)TILE_BYTES + (unsigned)(((row & 127) >> 3) * 1024);
        }
    };
    auto setX = [&](int u) {
        const int m0 = unit_field(u, 1), kt0 = unit_field(u, 2);
        xnk = unit_field(u, 3);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + 8 * (w + 8 * i);
            int rt = row >> 7;
            rt = rt < last_rt ? rt : last_rt;
            xso[i] = (unsigned)(rt * nktot + kt0) * (unsigned)TILE_BYTES + (unsigned)(((row & 127) >> 3) * 1024);
        }
    };
    auto issueW = [&](auto first) {      // pieces [0, NWQ0) (phase 1) or [NWQ0, NWQ) (phase 2) of W K-tile wi
        constexpr bool F = decltype(first)::value;
        const unsigned d = smem0 + (unsigned)(wi & 1) * C::PAR + (unsigned)w * 1024u;
        const unsigned go = (unsigned)wk * (unsigned)TILE_BYTES;
#pragma unroll
        for (int i = F ? 0 : NWQ0; i < (F ? NWQ0 : NWQ); ++i) glds16_s(p.W, voff + (wso[i] + go), d + i * 8192);
    };
    auto advW = [&]() {
        ++wi;
        if (++wk == wnk) {
            wk = 0;
            if (++wu < nunits) setW(wu);
        }
    };
    auto issueX = [&](auto first) {      // pieces 0, 1 (phase 3) or 2, 3 (phase 4) of X K-tile xi
        constexpr bool F = decltype(first)::value;
        const unsigned d = smem0 + (unsigned)(xi & 1) * C::PAR + C::WREG + (unsigned)w * 1024u;
        const unsigned go = (unsigned)xk * (unsigned)TILE_BYTES;
#pragma unroll
        for (int i = F ? 0 : 2; i < (F ? 2 : 4); ++i) glds16_s(p.X, voff + (xso[i] + go), d + i * 8192);
    };
    auto advX = [&]() {
        ++xi;
        if (++xk == xnk) {
            xk = 0;
            if (++xu < nunits) setX(xu);
        }
    };
    constexpr std::true_type FIRST{};
    constexpr std::false_type SECOND{};
    setW(0);
    setX(0);
    // K-tiles 0 and 1 are issued completely (X before W: the K loop's counted waits rely on that order), K-tile 0 is awaited with K-tile 1 in flight
    issueX(FIRST); issueX(SECOND); advX();
    issueW(FIRST); issueW(SECOND); advW();
    if (S > 1) {
        issueX(FIRST); issueX(SECOND); advX();
        issueW(FIRST); issueW(SECOND); advW();
        if constexpr (NWQ == 3) asm volatile("s_waitcnt vmcnt(7)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }

    P256_STAMP(1);
    const int li = lane & 15, g4 = lane >> 4;
    f32x4 acc[FI][4];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto mma = [&](const f16x8& wv, const f16x8& xv, f32x4& c) { c = mfma16(wv, xv, c, 0, 0, 0); };

    // the unit being computed; its bias slice (TNB floats, one 16-byte chunk per thread) is requested at its head and goes through LDS in the epilogue
    int cu = 0, ck = 0, cnk = unit_field(0, 3);
    auto bias_chunk = [&](int u) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        const int n = unit_field(u, 0) + 4 * tid;
        if (EPI != EPI_PARTIAL && p.bias && unit_field(u, 4) != 1 && tid < TNB / 4 && n < p.N) v = *(const f32x4*)(p.bias + n);
        return v;
    };
    f32x4 bias4 = bias_chunk(0);
    float amax = 0.f;

    // Fragment offsets from an opaque copy of the lane number (see the loop): used by the prologue read here
    auto frag_offsets = [&](int lo, int (&woff)[2], int (&xoff)[2]) {
#pragma unroll
        for (int sh = 0; sh < 2; ++sh) {
            const int l15 = lo & 15, ch = ((4 * sh + (lo >> 4)) ^ (l15 & 7)) << 4;
            woff[sh] = (16 * FI * wn + l15) * 128 + ch;
            xoff[sh] = C::WREG + (64 * wm + l15) * 128 + ch;
        }
    };
    // K-tile schedule (round 4, second form).  Every MFMA phase finds its fragments in registers, read ONE PHASE EARLIER — the first form read them at the head
    // of the phase that used them and its K-tile was the SUM of the LDS round trips (0.82 us of reads + barriers) and the MFMAs (0.64 us), tools/gemm_stamps.py:
    //   phase 1: MFMA W[0:h] x X[0:2]   | read X[2:4] and the first half of W[h:2h] of this K-tile
    //   phase 2: MFMA W[0:h] x X[2:4]   | read the rest of W[h:2h]
    //   -- lgkmcnt(0), barrier (b): every wave has read this parity -> it is free --
    //   phase 3: MFMA W[h:2h] x X[2:4]  | issue X(g + 2) into this parity
    //   -- vmcnt(4): everything older than X(g + 2) has landed = K-tile g + 1 complete; barrier (a) --
    //   phase 4: MFMA W[h:2h] x X[0:2]  | read W[0:h], X[0:2] of K-tile g + 1 (other parity) for the next phase 1; issue W(g + 2) into this parity
    // Fill order per K-tile is X then W, so the four youngest operations at (a) are exactly X(g + 2); K-tile g + 1 was issued during phases 3 / 4 of K-tile
    // g - 1: one whole K-tile of latency budget for every piece (the first form gave W half of that).
    // Two named fragment sets (A, B) alternate between consecutive K-tiles — no register copies, no conditional reads (the last K-tile of a block reads
    // its "next" fragments from whatever the other parity holds and nobody uses them) — so the K loop advances by PAIRS of K-tiles: every unit has an even
    // number of K-tiles (host-checked: K / 64 even, the split point is even).
    f16x8 wA[2][FIH], xA[2][2], wB[2][FIH], xB[2][2];
    {
        int lo = lane;
        asm volatile("" : "+v"(lo));
        int woff[2], xoff[2];
        frag_offsets(lo, woff, xoff);
#pragma unroll
        for (int sh = 0; sh < 2; ++sh) {
#pragma unroll
            for (int i = 0; i < FIH; ++i) wA[sh][i] = *(const f16x8*)(smem + woff[sh] + i * 16 * 128);
#pragma unroll
            for (int j = 0; j < 2; ++j) xA[sh][j] = *(const f16x8*)(smem + xoff[sh] + j * 16 * 128);
        }
    }
    const bool late = w >= 4;
    auto ktile = [&](int g, const f16x8 (&wa)[2][FIH], const f16x8 (&xa)[2][2], f16x8 (&wnx)[2][FIH], f16x8 (&xnx)[2][2]) {
        const char* bb = smem + (g & 1) * C::PAR;
        const char* bn = smem + ((g + 1) & 1) * C::PAR;
        const bool n2 = g + 2 < S && !GTAV_DBG(p, 1);   // (experiments build, debug bit 0: no refills — timing only)
        f16x8 wb[2][FIH], xb[2][2];
        // The per-lane fragment offsets are RECOMPUTED every K-tile from the lane number (a dozen VALU operations beside 48-64 MFMAs): kept in registers across
        // the loop they were spilled around the epilogue and reloaded in front of the loop's back edge — and hipcc's wait-count pass, which does not see the
        // inline-asm fills, then put an `s_waitcnt vmcnt(0)` at the head of EVERY K-tile (the fills in flight drained each step).  The empty asm makes the lane
        // number opaque so that the computation is not hoisted out of the loop again.
        int lo = lane;
        asm volatile("" : "+v"(lo));
        int woff[2], xoff[2];
        frag_offsets(lo, woff, xoff);
        // Third form: NOTHING is issued in a clump.  The second form put a phase's fragment reads (up to 10 per wave) and its fills (3-4 per wave) in front of
        // its MFMAs: eight waves then queue at the LDS (4 cycles per read) and at the address pipe (16 cycles per 1 KiB piece) at the same moment and none of
        // them feeds the matrix pipe meanwhile.  Here every MFMA of a phase carries at most one read in its issue shadow, and a wave's pieces are spread
        // over the phase, one per three or four MFMAs (waves 0-3 in front of the group, their SIMD partners 4-7 behind it).
        auto mm1 = [&](const f16x8 (&wf)[2][FIH], const f16x8 (&xf)[2][2], int m, int io, int jo) {   // the m-th of a phase's 4 FIH MFMAs
            const int sh = m / (2 * FIH), i = (m >> 1) % FIH, j = m & 1;
            mma(wf[sh][i], xf[sh][j], acc[io + i][jo + j]);
        };
        constexpr int NM = 4 * FIH;
        // ---- phase 1 ----
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            mm1(wa, xa, m, 0, 0);
            if (m < 4) xb[m >> 1][m & 1] = *(const f16x8*)(bb + xoff[m >> 1] + (2 + (m & 1)) * 16 * 128);
            else if (m < 4 + FIH) wb[0][m - 4] = *(const f16x8*)(bb + woff[0] + (FIH + m - 4) * 16 * 128);
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- phase 2 ----
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            mm1(wa, xb, m, 0, 2);
            if (m < FIH) wb[1][m] = *(const f16x8*)(bb + woff[1] + (FIH + m) * 16 * 128);
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // (b): every wave has read this parity's fragments
        // ---- phase 3: the four X pieces of K-tile g + 2 go into this parity ----
        {
            const unsigned d = smem0 + (unsigned)(xi & 1) * C::PAR + C::WREG + (unsigned)w * 1024u;
            const unsigned go = (unsigned)xk * (unsigned)TILE_BYTES;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                constexpr int PER = NM / 4;
                if (m % PER == 0 && n2 && !late) glds16_s(p.X, voff + (xso[m / PER] + go), d + (m / PER) * 8192);
                mm1(wb, xb, m, FIH, 2);
                if (m % PER == PER - 1 && n2 && late) glds16_s(p.X, voff + (xso[m / PER] + go), d + (m / PER) * 8192);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (n2) advX();
        }
        if (n2) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");   // (a): everything but X(g + 2) has landed = K-tile g + 1 complete
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        // ---- phase 4: next K-tile's first fragments from the other parity; the W pieces of K-tile g + 2 into this one ----
        {
            const unsigned d = smem0 + (unsigned)(wi & 1) * C::PAR + (unsigned)w * 1024u;
            const unsigned go = (unsigned)wk * (unsigned)TILE_BYTES;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                constexpr int PER = NM / NWQ;
                if (m % PER == 0 && m / PER < NWQ && n2 && !late) glds16_s(p.W, voff + (wso[m / PER] + go), d + (m / PER) * 8192);
                mm1(wb, xa, m, FIH, 0);
                if (m < 2 * (FIH + 2)) {   // in the order phase 1 consumes them: the first K half's X and W fragments, then the second half's
                    const int sh = m / (FIH + 2), q = m % (FIH + 2);
                    if (q < 2) xnx[sh][q] = *(const f16x8*)(bn + xoff[sh] + q * 16 * 128);
                    else wnx[sh][q - 2] = *(const f16x8*)(bn + woff[sh] + (q - 2) * 16 * 128);
                }
                if (m % PER == PER - 1 && m / PER < NWQ && n2 && late) glds16_s(p.W, voff + (wso[m / PER] + go), d + (m / PER) * 8192);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (n2) advW();
        }
    };
    for (int g = 0; g < S; g += 2) {
        ktile(g, wA, xA, wB, xB);
        ktile(g + 1, wB, xB, wA, xA);
        ck += 2;
        if (ck < cnk) continue;

        if (cu == 0) P256_STAMP(2);
        // ================= the unit is complete: epilogue straight from the accumulators =================
        const int kind = unit_field(cu, 4), slot = unit_field(cu, 5);
        const size_t slot_off = (size_t)slot * (TNB * 256);
        if (kind == 1) {
            // K tail of a split tile: partial sums out in register layout (1 KiB per wave-instruction), then publish
            float* dst = p.sk_ws + slot_off + (size_t)(w * FI * 4) * 256 + lane * 4;
#pragma unroll
            for (int i = 0; i < FI; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) *(f32x4*)(dst + (i * 4 + j) * 256) = acc[i][j];
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(p.sk_flags + slot, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            if (kind == 2) {
                if (tid == 0) {
                    int spins = 0;
                    while (__hip_atomic_load(p.sk_flags + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 1 && ++spins < (1 << 22)) __builtin_amdgcn_s_sleep(8);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (spins >= (1 << 22) && p.err_flag) atomicOr(p.err_flag, ERR_NONFINITE);   // (never seen: every block is resident and the helper runs its piece first)
                }
                __builtin_amdgcn_s_barrier();
                const float* src = p.sk_ws + slot_off + (size_t)(w * FI * 4) * 256 + lane * 4;
#pragma unroll
                for (int i = 0; i < FI; ++i) {
                    f32x4 t[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) t[j] = *(const f32x4*)(src + (i * 4 + j) * 256);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] + t[j];
                    __builtin_amdgcn_sched_barrier(0);
                }
                __builtin_amdgcn_s_barrier();       // every wave has its partial sums in registers: the slot may be reused by the next launch
                if (tid == 0) __hip_atomic_store(p.sk_flags + slot, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            float* bl = (float*)(smem + C::BIAS_OFF);
            if constexpr (EPI != EPI_PARTIAL) {
                if (tid < TNB / 4) *(f32x4*)(bl + 4 * tid) = bias4;
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
            const int n0 = unit_field(cu, 0), m0 = unit_field(cu, 1);
#pragma unroll
            for (int i = 0; i < FI; ++i) {
                const int nl = 16 * FI * wn + 16 * i + 4 * g4, n = n0 + nl;
                f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (EPI != EPI_PARTIAL) bv = *(const f32x4*)(bl + nl);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int m = m0 + 64 * wm + 16 * j + li;
                    const bool ok = n < p.N && m < p.M;
                    const f32x4 v = acc[i][j] + bv;
                    if constexpr (EPI == EPI_PARTIAL || EPI == EPI_F32) {
                        if (ok) *(f32x4*)((float*)p.out + (size_t)m * p.ldo + n) = v;
                    } else {
                        const float xin[4] = {v[0], v[1], v[2], v[3]};
                        float yo[4];
                        if constexpr (EPI == EPI_GELU_TANH) gelu_tanh_f4(xin, yo);
                        else { yo[0] = xin[0]; yo[1] = xin[1]; yo[2] = xin[2]; yo[3] = xin[3]; }
                        const uint2 mine = pack4(amax, yo[0], yo[1], yo[2], yo[3]);
                        // lanes (li, g) and (li, g ^ 1) hold adjacent 4-feature groups of one token: one 16-byte store per pair
                        const unsigned o0 = __shfl_xor(mine.x, 16, 64), o1 = __shfl_xor(mine.y, 16, 64);
                        if (ok && !(lane & 16)) *(uint4*)((f16*)p.out + tiled_off(m, n, p.ldo)) = uint4{mine.x, mine.y, o0, o1};
                    }
                }
                __builtin_amdgcn_sched_barrier(0);   // one feature group (four token groups) per scheduling region: every accumulator is live here
            }
        }
#pragma unroll
        for (int i = 0; i < FI; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        ck = 0;
#ifdef GTAV_EXPERIMENTS
        if (cu == 0 && p.stamps && tid == 0) {
            p.stamps[(size_t)blockIdx.x * 8 + 3] = __builtin_amdgcn_s_memrealtime();
            p.stamps[(size_t)blockIdx.x * 8 + 5] = __builtin_amdgcn_s_memtime();
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            p.stamps[(size_t)blockIdx.x * 8 + 6] = xcc & 0xF;
        }
#endif
        if (++cu < nunits) {
            cnk = unit_field(cu, 3);
            bias4 = bias_chunk(cu);
            // the next unit's first fragments are read (again) HERE, not carried through the epilogue from phase 4 of the K-tile before it: 40 registers
            // that the epilogue needs (all accumulators are live there) for one exposed LDS round trip per unit
            int lo = lane;
            asm volatile("" : "+v"(lo));
            int woff[2], xoff[2];
            frag_offsets(lo, woff, xoff);
            const char* bn = smem + (g & 1) * C::PAR;        // K-tile g + 2: landed and visible since barrier (a) of K-tile g + 1
#pragma unroll
            for (int sh = 0; sh < 2; ++sh) {
#pragma unroll
                for (int i = 0; i < FIH; ++i) wA[sh][i] = *(const f16x8*)(bn + woff[sh] + i * 16 * 128);
#pragma unroll
                for (int j = 0; j < 2; ++j) xA[sh][j] = *(const f16x8*)(bn + xoff[sh] + j * 16 * 128);
            }
        }
    }
    P256_STAMP(7);
#undef P256_STAMP
    if constexpr (EPI == EPI_GELU_TANH || EPI == EPI_F16_TILED) sat_report(amax, p.err_flag);
}

}  // namespace



namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Persistent ping-pong GEMM for large M (shape 16): one 1024-thread block per CU, two groups of 8 waves.
//
// What the stamps of round 2 showed for the two-blocks-per-CU shape at M = 5760 (profiles/round2/stamps_*.txt): the 512
// resident blocks run in LOCKSTEP — every block is in its prologue (2 us), main loop (21.6 us at half the CU's fill rate
// each) and epilogue (6.1 us: GELU / RoPE VALU + staging + stores) at the same time, so the co-resident block never hides
// anything: 8 of every 30 us the MFMA pipe and the L2->LDS path of the whole chip idle.  Here the overlap is built in:
//   * the block is persistent and walks its tiles (blockIdx + i * gridDim of an XCD-aware order) — 128 features x 192 tokens
//     each, the per-wave 64 x 48 sub-tile and fragment reads of shape 12;
//   * group (i & 1) runs the MAIN loop of tile i (all the LDS-DMA fills, fragment reads and MFMAs) while the other group runs
//     the EPILOGUE of tile i - 1 out of its accumulators: one 16 x 16 accumulator tile per K-step slot, straight from registers
//     to memory (pairs of lanes exchange halves for 16-byte stores; no LDS staging, so no LDS or barrier of its own), and in
//     its last NS - 1 slots issues the first fills of tile i + 1, which it will compute next: the LDS ring never drains
//     between tiles, a tile's prologue latency and its epilogue are both under the other group's MFMAs;
//   * one s_barrier per K-step, shared by all 16 waves: MAIN waves arrive after their counted vmcnt / lgkmcnt(0) (tile data
//     landed, previous stage no longer read), EPILOGUE waves arrive bare.  Ring slot of K-step k of tile i = (i P + k) % NS.
// 16 waves per CU = 4 per SIMD = 128 VGPRs per lane: 48 accumulator + 56 fragment registers fit (shape 12's budget).
// Because the epilogue is free, the residual GEMMs use the in-place gated residual epilogue here (EPI_RESID: x += gate (acc +
// bias), a read-modify-write whose loads are issued one slot ahead) instead of split-K slabs: the LayerNorm that follows
// reads and writes 35 MB instead of 83-106 MB at M = 5760.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PP_FI = 4, PP_FJ = 3, PP_WM = 4, PP_G = 5, PP_NT = PP_FI * PP_FJ;
constexpr int PP_WPC = 16, PP_NP = 40, PP_STAGE = PP_NP * 1024, PP_TN = 128, PP_TM = 192;

__device__ __forceinline__ void pp_tile_of(const GemmParams& p, int v, int tiles_m, int tiles_n, int& n0, int& m0) {
    const int T = tiles_m * tiles_n;
    const int xcd = v & 7, qq = T >> 3, rr = T & 7;
    const int tile_id = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (v >> 3);
    int gn = p.tm.gn;                                      // host: gemm_choose_gn() (every launcher fills it)
    const int group = tiles_m * gn;
    const int ng = tile_id / group, rem = tile_id - ng * group;
    const int n_first = ng * gn;
    if (n_first + gn > tiles_n) gn = tiles_n - n_first;
    const int tile_m = rem / gn, tile_n = n_first + (rem - tile_m * gn);
    n0 = tile_n * PP_TN;
    m0 = tile_m * PP_TM;
}

// 16-byte store of the fp16x4 of lanes (l, l ^ 16): the MFMA tile's lane groups g and g ^ 1 hold adjacent 4-element runs
__device__ __forceinline__ void pp_store_pair(f16* dst, uint2 mine, int lane, bool sc1, bool ok) {
    const unsigned o0 = __shfl_xor(mine.x, 16, 64), o1 = __shfl_xor(mine.y, 16, 64);
    if (ok && !(lane & 16)) {
        if (sc1) store16_sc1(dst, u32x4{mine.x, mine.y, o0, o1});
        else *(uint4*)dst = uint4{mine.x, mine.y, o0, o1};
    }
}

template <int EPI, int NS>
__global__ __launch_bounds__(1024, 1) void gemm_pp_kernel(GemmParams p) {
    constexpr int FI = PP_FI, FJ = PP_FJ, G = PP_G, NT = PP_NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = w >> 3, wg = w & 7, wn = wg & 1, wm = wg >> 1;
    const int li = lane & 15, g = lane >> 4;
    const int P = p.K / TK;
    const int tiles_m = (p.M + PP_TM - 1) / PP_TM, tiles_n = (p.N + PP_TN - 1) / PP_TN;
    const int T = tiles_m * tiles_n;
    const int nt = (T - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;   // tiles of this block (grid <= T)
    const int last_wt = ((p.N + 127) >> 7) - 1, last_rt = (p.M - 1) >> 7;
    const bool late = wg >= 4;

    // ---- fills: 40 one-KiB pieces per K-step (16 of W, 24 of X), 5 per MAIN wave; sources located per piece (mainloop_g).
    // Address of a piece = operand base + k * 16 KiB (SGPRs) + a 32-bit per-lane offset set once per tile (glds16_s) ----
    unsigned soff[G];
    const unsigned smem0 = lds_offset(smem);
    auto setup = [&](int n0, int m0) {
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int q = wg * G + i;
            const bool isw = q < PP_WPC;
            const int row = isw ? n0 + 8 * q : m0 + 8 * (q - PP_WPC);
            int rt = row >> 7;
            const int lim = isw ? last_wt : last_rt;
            rt = rt < lim ? rt : lim;                    // ragged edges re-read a valid tile (results are masked)
            soff[i] = (unsigned)rt * (unsigned)(P * TILE_BYTES) + (unsigned)(((row & 127) >> 3) * 1024 + lane * 16);
        }
    };
    auto stage = [&](int slot, int k) {
        const unsigned base = smem0 + slot * PP_STAGE + wg * (G * 1024);
        const char* wk = (const char*)p.W + (size_t)k * TILE_BYTES;
        const char* xk = (const char*)p.X + (size_t)k * TILE_BYTES;
#pragma unroll
        for (int i = 0; i < G; ++i) glds16_s(wg * G + i < PP_WPC ? wk : xk, soff[i], base + i * 1024);
    };
    int woff[2], xoff[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int ch = ((4 * s + g) ^ (li & 7)) << 4;
        woff[s] = (16 * FI * wn + li) * 128 + ch;
        xoff[s] = PP_WPC * 1024 + (16 * FJ * wm + li) * 128 + ch;
    }

    f32x4 acc[FI][FJ];
    float amax = 0.f;
    int en0 = 0, em0 = 0;          // tile whose accumulators this group holds
    bool etr = false;

#ifdef GTAV_EXPERIMENTS
    if (p.stamps && tid == 0) p.stamps[(size_t)blockIdx.x * 8 + 0] = __builtin_amdgcn_s_memrealtime();
#endif
    if (grp == 0) {                // prologue of the first tile
        int n0, m0;
        pp_tile_of(p, blockIdx.x, tiles_m, tiles_n, n0, m0);
        setup(n0, m0);
        const int npro = P < NS - 1 ? P : NS - 1;
        for (int k = 0; k < npro; ++k) stage(k % NS, k);
    }

    for (int i = 0; i <= nt; ++i) {
        const bool has_main = i < nt;
        const int base_slot = (int)(((long long)i * P) % NS);
        if ((i & 1) == grp) {
            if (!has_main) continue;
            // =========================================== MAIN loop of tile i ===========================================
            int n0, m0;
            pp_tile_of(p, blockIdx.x + i * gridDim.x, tiles_m, tiles_n, n0, m0);
            bool tr = false;
            if constexpr (EPI == EPI_QKV) tr = (p.qkv_mode == QKV_SPATIAL) && (n0 >= 2 * p.D);
            en0 = n0; em0 = m0; etr = tr;
#pragma unroll
            for (int a = 0; a < FI; ++a)
#pragma unroll
                for (int b = 0; b < FJ; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
            // two copies of the K loop (operands swapped for the transposed V tiles) instead of a per-MFMA select
            auto main_loop = [&](auto trc) {
                constexpr bool TR = decltype(trc)::value;
                int slot = base_slot;
                for (int k = 0; k < P; ++k) {
                    const int rem = P - 1 - k;
                    // this wave's share of K-step k has landed (younger fills of this wave: min(NS - 2, rem) K-steps of G)
                    kstep_sync_ring<(NS < 4 ? NS : 4), G>(rem);
                    const bool refill = k + NS - 1 < P;      // the last NS - 1 slots belong to the next tile (filled by the other group)
                    int fslot = slot + NS - 1;
                    fslot = fslot >= NS ? fslot - NS : fslot;
                    if (refill && !late) stage(fslot, k + NS - 1);
                    const char* b = smem + slot * PP_STAGE;
                    // all 14 fragment reads of the K-step go out before its first MFMA (one LDS round trip per K-step instead of the
                    // eight read / wait / 3-MFMA groups hipcc forms at this register budget)
                    f16x8 wf[2][FI], xf[2][FJ];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
#pragma unroll
                        for (int a = 0; a < FI; ++a) wf[s][a] = *(const f16x8*)(b + woff[s] + a * 16 * 128);
#pragma unroll
                        for (int c = 0; c < FJ; ++c) xf[s][c] = *(const f16x8*)(b + xoff[s] + c * 16 * 128);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int a = 0; a < FI; ++a)
#pragma unroll
                            for (int c = 0; c < FJ; ++c) {
                                if (TR) acc[a][c] = mfma16(xf[s][c], wf[s][a], acc[a][c], 0, 0, 0);
                                else acc[a][c] = mfma16(wf[s][a], xf[s][c], acc[a][c], 0, 0, 0);
                            }
                    if (refill && late) {
                        asm volatile("" ::: "memory");
                        stage(fslot, k + NS - 1);
                    }
                    slot = slot + 1 == NS ? 0 : slot + 1;
                }
            };
            if (tr) main_loop(std::true_type{});
            else main_loop(std::false_type{});
#ifdef GTAV_EXPERIMENTS
            if (p.stamps && wg == 0 && lane == 0 && i < 5) p.stamps[(size_t)blockIdx.x * 8 + 2 + i] = __builtin_amdgcn_s_memrealtime();   // end of MAIN(i)
#endif
        } else {
            // ================= EPILOGUE of tile i - 1 (this group's accumulators) + first fills of tile i + 1 =================
            const bool do_epi = i >= 1, do_pref = i + 1 < nt;
            // (the fill pointers of tile i + 1 are set up at its first prefetch slot, not here: ten VGPRs less through the epilogue)
            auto prefetch = [&](int e, int pbase_, int pfirst_) {
                if (e == pfirst_) {
                    int pn0, pm0;
                    pp_tile_of(p, blockIdx.x + (i + 1) * gridDim.x, tiles_m, tiles_n, pn0, pm0);
                    setup(pn0, pm0);
                }
                int ps = pbase_ + (e - pfirst_);
                ps = ps >= NS ? ps - NS : ps;
                stage(ps, e - pfirst_);
            };
            const int pbase = (int)(((long long)(i + 1) * P) % NS);      // ring slot of K-step 0 of tile i + 1
            const int pfirst = P - (NS - 1);                              // slot index in this phase at which tile i + 1's step 0 may be issued
            const int n0 = en0, m0 = em0;
            // ---- per-token destination coordinates of this wave's FJ token columns (integer divisions: once per tile) ----
            int tok_a[FJ], tok_b[FJ];          // tok_b: token inside its frame (spatial, = RoPE position) / window frame (temporal RoPE position)
            bool tok_ok[FJ];
#pragma unroll
            for (int c = 0; c < FJ; ++c) {
                const int m = m0 + 16 * FJ * wm + 16 * c + (etr ? 4 * g : li);
                tok_ok[c] = m < p.M;
                const int mm = tok_ok[c] ? m : p.M - 1;
                tok_a[c] = 0; tok_b[c] = 0;
                if constexpr (EPI == EPI_QKV) {
                    const int fr = mm / p.S;
                    if (p.qkv_mode == QKV_SPATIAL) {
                        tok_a[c] = fr; tok_b[c] = mm - fr * p.S;
                    } else {
                        const int bb = fr / p.Tq, tfr = p.t0 + (fr - bb * p.Tq);
                        tok_a[c] = (bb * p.Tmax + tfr) * p.S + (mm - fr * p.S); tok_b[c] = tfr;
                    }
                } else if constexpr (EPI == EPI_RESID) {
                    int row = p.gate ? mm / p.rows_per_gate : 0;
                    if (p.gate && p.gate_rows) row = p.gate_rows[row];
                    tok_a[c] = row;
                }
            }
            // one accumulator tile per slot; the loads a tile needs (residual row, gate, bias, RoPE) are issued one slot ahead
            f32x4 ld0 = f32x4{0.f, 0.f, 0.f, 0.f}, ld1 = ld0, ld2 = ld0;      // for the tile processed in THIS slot
            f32x4 nx0 = ld0, nx1 = ld0, nx2 = ld0;                            // for the next one
            auto issue_loads = [&](int e, f32x4& r0, f32x4& r1, f32x4& r2) {
                const int a = e / FJ, c = e - a * FJ;
                const int m = m0 + 16 * FJ * wm + 16 * c + li;
                const int n = n0 + 16 * FI * wn + 16 * a + 4 * g;
                r0 = f32x4{0.f, 0.f, 0.f, 0.f}; r1 = r0; r2 = r0;
                if (etr) {
                    if (p.bias) { const int nf = n0 + 16 * FI * wn + 16 * a + li; r0[0] = nf < p.N ? p.bias[nf] : 0.f; }
                    return;
                }
                if (n >= p.N || !tok_ok[c]) return;
                if (p.bias) r0 = *(const f32x4*)(p.bias + n);
                if constexpr (EPI == EPI_RESID) {
                    r1 = *(const f32x4*)((const float*)p.out + (size_t)m * p.ldo + n);
                    if (p.gate) r2 = *(const f32x4*)(p.gate + (size_t)tok_a[c] * p.gate_stride + n);
                } else if constexpr (EPI == EPI_QKV) {
                    if (n < 2 * p.D) r1 = *(const f32x4*)(p.rope_cs + tok_b[c] * 64 + (n & 63));
                }
            };
            auto epi_tile = [&](int e, const f32x4& r0, const f32x4& r1, const f32x4& r2) {
                const int a = e / FJ, c = e - a * FJ;
                const f32x4 av = acc[a][c];
                // every lane runs the pair exchange of pp_store_pair (cross-lane reads need both lanes active); only the store is
                // predicated.  A pair (g, g ^ 1) shares its token(s) / feature group, so `ok` is the same in both lanes.
                if (etr) {
                    // D[row = token][col = feature] (spatial V): the lane owns tokens m .. m + 3 of feature n -> V^T [feature][token]
                    const int n = n0 + 16 * FI * wn + 16 * a + li;
                    const int heads = p.D >> 6, nn = n - 2 * p.D;
                    const uint2 pk = pack4(amax, av[0] + r0[0], av[1] + r0[0], av[2] + r0[0], av[3] + r0[0]);
                    const bool ok = tok_ok[c] && n < p.N;
                    f16* dst = p.v + ((size_t)(tok_a[c] * heads + (nn >> 6)) * 64 + (nn & 63)) * p.S + tok_b[c];
                    pp_store_pair(dst, pk, lane, p.out_sc1, ok);
                    return;
                }
                const int m = m0 + 16 * FJ * wm + 16 * c + li;
                const int n = n0 + 16 * FI * wn + 16 * a + 4 * g;
                const bool ok = n < p.N && tok_ok[c];         // a pair covers 8 consecutive features: N % 8 == 0
                f32x4 v = av + r0;
                if constexpr (EPI == EPI_RESID) {
                    if (ok) {
                        float* dst = (float*)p.out + (size_t)m * p.ldo + n;
                        const f32x4 x = p.gate ? r1 + r2 * v : r1 + v;
                        if (p.out_sc1) store16_sc1(dst, x);
                        else *(f32x4*)dst = x;
                    }
                } else if constexpr (EPI == EPI_GELU_TANH || EPI == EPI_GELU_ERF) {
                    uint2 pk;
                    if constexpr (EPI == EPI_GELU_TANH) pk = pack4(amax, gelu_tanh_f(v[0]), gelu_tanh_f(v[1]), gelu_tanh_f(v[2]), gelu_tanh_f(v[3]));
                    else pk = pack4(amax, gelu_erf_f(v[0]), gelu_erf_f(v[1]), gelu_erf_f(v[2]), gelu_erf_f(v[3]));
                    pp_store_pair((f16*)p.out + (ok ? tiled_off(m, n, p.ldo) : 0), pk, lane, p.out_sc1, ok);
                } else if constexpr (EPI == EPI_QKV) {
                    const int which = n >= 2 * p.D ? 2 : (n >= p.D ? 1 : 0);
                    const int nn = n - which * p.D;
                    if (which < 2) {
                        v = rope4(v, r1);
                    }
                    const uint2 pk = pack4(amax, v[0], v[1], v[2], v[3]);
                    f16* dst;
                    if (p.qkv_mode == QKV_SPATIAL) {
                        const int heads = p.D >> 6;
                        dst = (which == 0 ? p.q : p.k) + ((size_t)(tok_a[c] * heads + (nn >> 6)) * p.S + tok_b[c]) * 64 + (nn & 63);
                    } else if (which == 0) {
                        dst = p.q + (size_t)(tok_ok[c] ? m : 0) * p.D + nn;
                    } else {
                        dst = p.k + (size_t)tok_a[c] * 2 * p.D + (which == 2 ? p.D : 0) + nn;
                    }
                    pp_store_pair(dst, pk, lane, p.out_sc1, ok);
                }
            };
            // the residual epilogue's read-modify-write loads are issued one slot ahead; the others (bias / RoPE rows: L2 hits) are
            // loaded in their own slot — the epilogue has slack (12 tiles in >= 14 slots) and the QKV variant has no registers to spare
            constexpr bool AHEAD = EPI == EPI_RESID;
            if (do_epi && AHEAD) issue_loads(0, ld0, ld1, ld2);
#pragma unroll
            for (int e = 0; e < NT; ++e) {
                if (has_main) asm volatile("s_barrier" ::: "memory");
                if (do_epi) {
                    if constexpr (AHEAD) {
                        if (e + 1 < NT) issue_loads(e + 1, nx0, nx1, nx2);
                        epi_tile(e, ld0, ld1, ld2);
                        ld0 = nx0; ld1 = nx1; ld2 = nx2;
                    } else {
                        issue_loads(e, ld0, ld1, ld2);
                        epi_tile(e, ld0, ld1, ld2);
                    }
                }
                if (has_main && do_pref && e >= pfirst) prefetch(e, pbase, pfirst);
            }
            if (has_main) {
                for (int e = NT; e < P; ++e) {
                    asm volatile("s_barrier" ::: "memory");
                    if (do_pref && e >= pfirst) prefetch(e, pbase, pfirst);
                }
            }
        }
    }
    if constexpr (EPI != EPI_RESID) sat_report(amax, p.err_flag);
#ifdef GTAV_EXPERIMENTS
    // timeline (tools/gemm_stamps.py --pp): [0] entry, [2 + i] end of the MAIN loop of this block's i-th tile (i < 5), [7] end of the
    // last epilogue (written by the group that ran it), [1] = number of tiles
    if (p.stamps && wg == 0 && lane == 0 && grp == ((nt - 1) & 1)) {
        p.stamps[(size_t)blockIdx.x * 8 + 7] = __builtin_amdgcn_s_memrealtime();
        p.stamps[(size_t)blockIdx.x * 8 + 1] = nt;
    }
#endif
}



} // namespace
// ---- launcher of the ping-pong kernel ----
// (what it measured, and gemm_pp_ok: gemm_plan.hip)
template <int EPI>
static int launch_pp(const GemmParams& p, hipStream_t stream) {
    constexpr int NS = 3;
    int cus = 0;
    if (int rc_ = lds_opt_in<gemm_pp_kernel<EPI, NS>>(NS * PP_STAGE, &cus)) return rc_;
    const int T = cdiv(p.M, PP_TM) * cdiv(p.N, PP_TN);
    const dim3 grid(T < cus ? T : cus);
    GemmParams q = p;
    const int tiles_n = cdiv(p.N, PP_TN);
    q.tm.gn = tiles_n >= 8 ? tiles_n >> 3 : 1;   // pp_tile_of: an eighth of the n-panels per group (the persistent walk strides over XCD runs)
    GTAV_LAUNCH((gemm_pp_kernel<EPI, NS>), grid, dim3(1024), NS * PP_STAGE, stream, q);
    GTAV_CHECK_HIP(hipGetLastError());
    return 0;
}
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Persistent 256 x 256 tiles on SIXTEEN waves in two staggered groups (shape 42, round 4; docs/LABNOTES.md 4.11).
//
// What shapes 40 / 41 showed: with two waves per SIMD that all run the same phase, every fragment-read clump and every fill burst of a K-tile is time the
// matrix pipe idles — no placement of the reads and fills inside the phases changed the 1.43 us K-tile (second and third form) — while the two INDEPENDENT
// 8-wave blocks of shape 12 (four waves per SIMD, 128 registers) keep the pipe 84 % busy inside their K loop because one block's fill / read phase falls
// into the other one's MFMAs by chance.  Here that overlap is by construction, inside one block that shares one 256 x 256 stage (0.6 of shape 12's fill
// bytes per FLOP):
//   * 16 waves of 64 x 64 outputs each (64 accumulator + 32 fragment registers: the 128-register budget of four waves per SIMD); group A = waves 0-7,
//     group B = waves 8-15 (two of each on every SIMD);
//   * a K-tile is four intervals, each closed by ONE s_barrier of all 16 waves: R0 (read the first K half's fragments) | M0 (16 MFMAs) | R1 | M1.  Group B
//     runs one interval behind group A: while one group issues MFMAs the other one reads fragments and issues its fills, and the next interval they swap;
//   * two-parity ring of 64 KiB stages: a wave issues its four pieces of K-tile g + 1 at the head of its R0 of K-tile g (the parity of K-tile g - 1 is
//     free: the lagging group drained its last reads of it before the barrier that closed the interval before A's R0) and waits for them — vmcnt(0) — in
//     front of the barrier that closes the interval before group A's R0 of K-tile g + 1 (A: end of its M1, B: end of its R1);
//   * persistence, unit list, K split of the remainder tiles, epilogue from the accumulators: as the 8-wave kernel above.  The groups re-align at every
//     unit boundary (A gives one interval back) so that the epilogue's own barriers mean the same thing to every wave.
// Measured (profiles/round4/persistent_256_token_tile_kernel_shape41_fc1.txt, fc1 at M = 5760): correct and bit-reproducible, but 73-79 us against 54-64 us
// for shape 12.  Strict form (a barrier after every interval): 1.74 us per K-tile, 1.46 us with the fills off — the sixteen-wave barrier costs ~170 cycles
// per interval; the form below (ONE barrier per K-tile, the groups alternate on their own): 1.51 us, 1.40 us with the fills off, 0.90 us for the fills
// alone (67 GB/s per CU), against 1.05 us of MFMAs.  And the tile's GELU epilogue — 12 VALU slots per output, 65 536 outputs on 64 lanes per clock — is
// 11 us that nothing hides with one block per CU; the two-blocks-per-CU tile pays 4.6 us per 49 152 outputs.  Experiments build only.
// ---------------------------------------------------------------------------------------------------------------------
struct S16 {
    static constexpr int PAR = 4 * TILE_BYTES, XOFF = 2 * TILE_BYTES, BIAS_OFF = 2 * PAR, TOUCH_OFF = BIAS_OFF + 256 * 4 + 16 * 8 * 4, LDS = TOUCH_OFF + 256;   // ring, bias slice, unit list, touch sink
};
template <int EPI>
__global__ __launch_bounds__(1024, 1) void gemm_s16_kernel(GemmParams p) {
    using C = S16;
    constexpr int FI = 4, TNB = 256;
    static_assert(EPI == EPI_F32 || EPI == EPI_PARTIAL || EPI == EPI_GELU_TANH || EPI == EPI_F16_TILED, "epilogues of the persistent 256-token-tile kernels");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = w & 3, wm = w >> 2;
    const bool lagB = w >= 8;
    const int nktot = p.K / TK;
    const int G = gridDim.x, b = blockIdx.x;
    const bool split = b < 2 * p.sk_r;
    const int n_dp = b < p.sk_dp ? (p.sk_dp - b + G - 1) / G : 0;
    const int nunits = n_dp + (split ? 1 : 0);
    if (nunits == 0) return;
#ifdef GTAV_EXPERIMENTS
#define S16_STAMP(i) do { if (p.stamps && tid == 0) p.stamps[(size_t)blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
    if (p.stamps && tid == 0) { p.stamps[(size_t)blockIdx.x * 8 + 4] = __builtin_amdgcn_s_memtime(); }
#else
#define S16_STAMP(i) do { } while (0)
#endif
    S16_STAMP(0);
    const int S = n_dp * nktot + (split ? ((b & 1) ? nktot - ((nktot >> 1) & ~1) : ((nktot >> 1) & ~1)) : 0);   // K-tiles of this block
    const int last_wt = ((p.N + 127) >> 7) - 1, last_rt = (p.M - 1) >> 7;
    const unsigned voff = (unsigned)lane * 16u, smem0 = lds_offset(smem);
    int* const ut = (int*)(smem + C::BIAS_OFF + TNB * 4);
    if (tid < nunits) {
        const P256Unit un = p256_unit<8>(p, tid, (p.M + 255) >> 8, (p.N + TNB - 1) / TNB, nktot);
        int* q = ut + 8 * tid;
        q[0] = un.n0; q[1] = un.m0; q[2] = un.kt0; q[3] = un.nkt; q[4] = un.kind; q[5] = un.slot;
    }
    if (tid < TNB) ((float*)(smem + C::BIAS_OFF))[tid] = 0.f;   // (a launch without bias adds zeros)
    __syncthreads();
    auto unit_field = [&](int u, int f) { return __builtin_amdgcn_readfirstlane(ut[8 * u + f]); };

    // ---- fill cursor: the next K-tile to issue (one K-tile ahead of the reads, across unit boundaries).  Wave w owns pieces w and w + 16 of each operand
    // (piece q = rows 8 q .. 8 q + 7 of the 256-row block = 1 KiB of tile q / 16); sources as 32-bit offsets from the operand base (host-checked) ----
    int fu = 0, fk = 0, fi = 0, fnk;
    unsigned wso[2], xso[2];
    auto setF = [&](int u) {
        const int n0 = unit_field(u, 0), m0 = unit_field(u, 1), kt0 = unit_field(u, 2);
        fnk = unit_field(u, 3);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rw = n0 + 8 * (w + 16 * i), rx = m0 + 8 * (w + 16 * i);
            int tw = rw >> 7, tx = rx >> 7;
            tw = tw < last_wt ? tw : last_wt;                 // ragged edges re-read a valid tile (results are masked)
            tx = tx < last_rt ? tx : last_rt;
            wso[i] = (unsigned)(tw * nktot + kt0) * (unsigned)TILE_BYTES + (unsigned)(((rw & 127) >> 3) * 1024);
            xso[i] = (unsigned)(tx * nktot + kt0) * (unsigned)TILE_BYTES + (unsigned)(((rx & 127) >> 3) * 1024);
        }
    };
    auto issueF = [&]() {
        const unsigned d = smem0 + (unsigned)(fi & 1) * C::PAR + (unsigned)w * 1024u;
        const unsigned go = (unsigned)fk * (unsigned)TILE_BYTES;
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16_s(p.W, voff + (wso[i] + go), d + i * TILE_BYTES);
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16_s(p.X, voff + (xso[i] + go), d + C::XOFF + i * TILE_BYTES);
        ++fi;
        if (++fk == fnk) {
            fk = 0;
            if (++fu < nunits) setF(fu);
        }
    };
    setF(0);
    issueF();
    if (S > 1) {
        issueF();
        asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    S16_STAMP(1);

    const int li = lane & 15, g4 = lane >> 4;
    int woff[2], xoff[2];
#pragma unroll
    for (int sh = 0; sh < 2; ++sh) {
        const int ch = ((4 * sh + g4) ^ (li & 7)) << 4;
        woff[sh] = (64 * wn + li) * 128 + ch;
        xoff[sh] = C::XOFF + (64 * wm + li) * 128 + ch;
    }
    f32x4 acc[FI][4];
    float amax = 0.f;
    const bool fills = !GTAV_DBG(p, 1), compute = !GTAV_DBG(p, 16);   // (experiments build, debug bits 0 / 4: no refills / fills and barriers only — timing only)
    int g = 0;                            // K-tile counter of the block: parity g & 1
    for (int cu = 0; cu < nunits; ++cu) {
        const int cnk = unit_field(cu, 3);
        // the unit's bias slice (256 floats) goes straight into LDS (waves 0-3, one dword per lane: no register lives through the K loop); the K loop's
        // vmcnt(0) waits and barriers order it for the epilogue, the barrier that closed the previous unit's epilogue protects its last readers
        if constexpr (EPI != EPI_PARTIAL) {
            if (w < 4 && p.bias && unit_field(cu, 4) != 1) {
                int n = unit_field(cu, 0) + 64 * w + lane;
                n = n < p.N ? n : p.N - 1;
                glds4_s(p.bias, (unsigned)n * 4u, smem0 + C::BIAS_OFF + (unsigned)w * 256u);
            }
        }
#pragma unroll
        for (int i = 0; i < FI; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        // ONE barrier per K-tile (X_g, at its head).  Behind it a group-A wave runs R0 M0 R1 M1 of K-tile g, a group-B wave first the M1 it still owes K-tile
        // g - 1 (its fragments are in registers), then R0 M0 R1 of K-tile g: the two groups of a SIMD alternate between fragment reads and MFMAs without being
        // forced to (the strict form — a barrier after every interval — measured 170 cycles of barrier per interval: 1.46 us per K-tile without any fill).
        //   WAR: every wave drained its reads of K-tile g - 1 (lgkmcnt(0)) in front of X_g, so the fills of K-tile g + 1 may go into that parity behind X_g;
        //   RAW: every wave waited for its own pieces of K-tile g (vmcnt(0)) in front of X_g.
        f16x8 wf[FI], xf[4];
        auto rd = [&](const char* bb, int sh) {
#pragma unroll
            for (int i = 0; i < FI; ++i) wf[i] = *(const f16x8*)(bb + woff[sh] + i * 16 * 128);
#pragma unroll
            for (int j = 0; j < 4; ++j) xf[j] = *(const f16x8*)(bb + xoff[sh] + j * 16 * 128);
        };
        auto mm = [&]() {
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(wf[i], xf[j], acc[i][j], 0, 0, 0);
        };
        for (int k = 0; k < cnk; ++k, ++g) {
            const char* bb = smem + (g & 1) * C::PAR;
            if (g > 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // X_g (K-tile 0: the prologue's barrier)
            __builtin_amdgcn_sched_barrier(0);
            if (lagB && k > 0 && compute) mm();                 // M1 of K-tile g - 1
            __builtin_amdgcn_sched_barrier(0);
            if (g >= 1 && fi < S && fills) issueF();          // K-tile g + 1 into the parity K-tile g - 1 has left
#ifdef GTAV_EXPERIMENTS
            // (debug bit 11) L2 touch of K-tile k + 3 of this unit: waves 0 / 8 request this block's SHARE of the W / X lines the blocks of its XCD that
            // work on the same feature / token panel will all fill from (one dword per 128-byte line, into an LDS sink)
            if (GTAV_DBG(p, 2048) && k + 3 < cnk && (w == 0 || w == 8)) {
                const int gn = p.tm.gn > 0 ? p.tm.gn : 1, cw = 32 / gn > 0 ? 32 / gn : 1;
                const bool isw = w == 0;
                const int cnt = isw ? cw : gn, rank = isw ? (unit_field(cu, 1) >> 8) % cw : (unit_field(cu, 0) >> 8) % gn;
                const int r0 = isw ? unit_field(cu, 0) : unit_field(cu, 1), lim = isw ? last_wt : last_rt;
                const int kt = unit_field(cu, 2) + k + 3;
                for (int q = 0; rank + cnt * 64 * q < 256; ++q) {
                    const int l = rank + cnt * (lane + 64 * q);
                    const int row = r0 + (l < 256 ? l : rank);
                    int rt = row >> 7;
                    rt = rt < lim ? rt : lim;
                    const unsigned off = (unsigned)(rt * nktot + kt) * (unsigned)TILE_BYTES + (unsigned)(row & 127) * 128u;
                    glds4_s(isw ? (const void*)p.W : (const void*)p.X, off, smem0 + C::TOUCH_OFF);
                }
            }
#endif
            if (compute) {
                rd(bb, 0);
                __builtin_amdgcn_sched_barrier(0);
                mm();                                          // M0
                __builtin_amdgcn_sched_barrier(0);
                rd(bb, 1);
                __builtin_amdgcn_sched_barrier(0);
                if (!lagB) mm();                               // M1 (group B: behind the next barrier)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (lagB && compute) mm();                              // group B's last M1 of the unit
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (cu == 0) S16_STAMP(2);
        // ================= the unit is complete: epilogue straight from the accumulators (as the 8-wave kernel) =================
        const int kind = unit_field(cu, 4), slot = unit_field(cu, 5);
        const size_t slot_off = (size_t)slot * (TNB * 256);
        if (kind == 1) {
            float* dst = p.sk_ws + slot_off + (size_t)(w * FI * 4) * 256 + lane * 4;
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) *(f32x4*)(dst + (i * 4 + j) * 256) = acc[i][j];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(p.sk_flags + slot, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            if (kind == 2) {
                if (tid == 0) {
                    int spins = 0;
                    while (__hip_atomic_load(p.sk_flags + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 1 && ++spins < (1 << 22)) __builtin_amdgcn_s_sleep(8);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (spins >= (1 << 22) && p.err_flag) atomicOr(p.err_flag, ERR_NONFINITE);
                }
                __builtin_amdgcn_s_barrier();
            }
            // (the K tail's partial sums are added inside the store loop below, four accumulator tiles at a time: adding them in a loop of their own made the
            // accumulators a phi of two paths, which hipcc resolved with sixteen register-pair copies and four spilled tiles at the 128-register cap)
            const float* const psrc = p.sk_ws + slot_off + (size_t)(w * FI * 4) * 256 + lane * 4;
            const float* bl = (const float*)(smem + C::BIAS_OFF);
            if constexpr (EPI != EPI_PARTIAL) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");   // the bias slice (issued at the unit's head by waves 0-3) is in LDS
            // (the lane number goes through an empty asm here: offsets derived from it cannot be hoisted out of the unit loop, where they would live — spilled —
            // through every K loop of the block)
            int lo = lane;
            asm volatile("" : "+v"(lo));
            const int li = lo & 15, g4 = lo >> 4;
            // Stores: wave-uniform base (SGPRs) + ONE 32-bit per-lane offset + small per-(i, j) terms, one (i, j) per scheduling region — with 64-bit per-lane
            // addresses hoisted for all sixteen stores hipcc spilled a third of the accumulators around this loop, and every scratch reload then waited
            // (vmcnt retires in order) for the global stores in front of it: 20-30 us per unit (tools/gemm_stamps.py).  Host-checked: the output is < 4 GiB.
            const int n0 = unit_field(cu, 0), m0 = unit_field(cu, 1);
            const bool tiled = EPI == EPI_GELU_TANH || EPI == EPI_F16_TILED;
            // tile-major fp16: row tile (m0 >> 7) + (wm >> 1), column tile (n0 >> 6) + wn are wave-uniform; in the tile: row 64 (wm & 1) + 16 j + li, chunk (2 i + (g4 >> 1)) ^ (li & 7)
            const char* const obase = tiled ? (const char*)p.out + ((size_t)((m0 >> 7) + (wm >> 1)) * (size_t)(p.ldo >> 6) + (size_t)((n0 >> 6) + wn)) * TILE_BYTES
                                            : (const char*)p.out + ((size_t)(m0 + 64 * wm) * p.ldo + (size_t)(n0 + 64 * wn)) * 4;
            const unsigned lane_off = tiled ? (unsigned)((64 * (wm & 1) + li) * 128) : (unsigned)li * (unsigned)p.ldo * 4u + (unsigned)g4 * 16u;
#pragma unroll
            for (int i = 0; i < FI; ++i) {
                const int nl = 64 * wn + 16 * i + 4 * g4, n = n0 + nl;
                f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (EPI != EPI_PARTIAL) bv = *(const f32x4*)(bl + nl);
                f32x4 t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (kind == 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) t[j] = *(const f32x4*)(psrc + (i * 4 + j) * 256);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int m = m0 + 64 * wm + 16 * j + li;
                    const bool ok = n < p.N && m < p.M;
                    const f32x4 v = (acc[i][j] + t[j]) + bv;
                    if constexpr (EPI == EPI_PARTIAL || EPI == EPI_F32) {
                        union { f32x4 f; u32x4 u; } cv;
                        cv.f = v;
                        if (ok) store16_soff(obase, lane_off + (unsigned)(16 * j) * (unsigned)p.ldo * 4u + (unsigned)(64 * i), cv.u);
                    } else {
                        const float xin[4] = {v[0], v[1], v[2], v[3]};
                        float yo[4];
                        if constexpr (EPI == EPI_GELU_TANH) gelu_tanh_f4(xin, yo);
                        else { yo[0] = xin[0]; yo[1] = xin[1]; yo[2] = xin[2]; yo[3] = xin[3]; }
                        const uint2 mine = pack4(amax, yo[0], yo[1], yo[2], yo[3]);
                        asm volatile("" : "+v"(amax));   // the running maximum is updated HERE: hipcc otherwise keeps all 64 values alive (spilled) and folds them at the end
                        const unsigned o0 = __shfl_xor(mine.x, 16, 64), o1 = __shfl_xor(mine.y, 16, 64);
                        if (ok && !(lane & 16)) store16_soff(obase, lane_off + (unsigned)(j * 2048) + (unsigned)(((2 * i + (g4 >> 1)) ^ (li & 7)) << 4), u32x4{mine.x, mine.y, o0, o1});
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            wg_barrier();   // every wave has read the bias slice (the next unit's head rewrites it) and, kind 2, its partial sums (the slot may be reused by the next launch)
            if (kind == 2 && tid == 0) __hip_atomic_store(p.sk_flags + slot, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#ifdef GTAV_EXPERIMENTS
        if (cu == 0 && p.stamps && tid == 0) {
            p.stamps[(size_t)blockIdx.x * 8 + 3] = __builtin_amdgcn_s_memrealtime();
            p.stamps[(size_t)blockIdx.x * 8 + 5] = __builtin_amdgcn_s_memtime();
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            p.stamps[(size_t)blockIdx.x * 8 + 6] = xcc & 0xF;
        }
#endif
    }
    S16_STAMP(7);
#undef S16_STAMP
    if constexpr (EPI == EPI_GELU_TANH || EPI == EPI_F16_TILED) sat_report(amax, p.err_flag);
}

// The persistent 256-token-tile kernels (shapes 40 / 41 / 42): whole rounds of the T tiles + a two-way K split of a remainder of <= grid / 2 tiles (q.sk_dp / q.sk_r)
static int p256_units(GemmParams& q, int T, int cus, int* grid) {
    GTAV_REQUIRE((size_t)round_up(q.M, 128) * q.K * 2 < (1ull << 32) && (size_t)round_up(q.N, 128) * q.K * 2 < (1ull << 32),
                 "gemm: the persistent 256-token-tile kernels address their operands with 32-bit offsets (M=%d N=%d K=%d)", q.M, q.N, q.K);
    GTAV_REQUIRE(cdiv(T, cus) + 1 <= P256_MAXU, "gemm: %d tiles are more than %d rounds of the persistent 256-token-tile kernel", T, P256_MAXU - 1);
    const int full = T / cus, rem = T - full * cus;
    *grid = T < cus ? T : cus;
    q.sk_dp = T;
    q.sk_r = 0;
    if (rem > 0 && 2 * rem <= cus && rem <= GEMM_SK_MAX_SPLIT && q.sk_ws && q.sk_flags && q.K / TK >= 4) {
        q.sk_dp = T - rem;
        q.sk_r = rem;
        if (full == 0) *grid = 2 * rem;
    }
    return 0;
}

template <int EPI>
static int launch_s16(const GemmParams& p, hipStream_t stream) {
    using C = S16;
    int cus = 0;
    if (int rc_ = lds_opt_in<gemm_s16_kernel<EPI>>(C::LDS, &cus)) return rc_;
    GemmParams q = p;
    GTAV_REQUIRE((size_t)round_up(p.M, 128) * (size_t)p.ldo * 4 < (1ull << 32), "gemm: the sixteen-wave persistent kernel addresses its output with 32-bit offsets (M=%d ldo=%d)", p.M, p.ldo);
    int grid = 0;
    if (int rc_ = p256_units(q, cdiv(p.M, 256) * cdiv(p.N, 256), cus, &grid)) return rc_;
    GTAV_LAUNCH((gemm_s16_kernel<EPI>), dim3(grid), dim3(1024), C::LDS, stream, q);
    GTAV_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- antiphase 256 x 256 main loop (shape 17) ----
// The same 256 x 256 tile, LDS image, fill schedule and accumulator layout as mainloop256, run as TWO WAVE GROUPS IN ANTIPHASE (round 6; cdna_hip_programming.md
// "The 256^2 8-phase template"): waves 0-3 and waves 4-7 — one wave of each group per SIMD — execute the same phase sequence one barrier interval apart, so that on
// every SIMD one wave issues its 16 MFMAs of a phase (s_setprio 1) while its partner issues the fragment reads and the LDS-DMA fills of its next phase and waits for
// the reads to land.  In the lockstep loop both waves of a SIMD reach their reads at the same time and the matrix pipe waits out the LDS round trip with them
// (docs/LABNOTES.md 4.11: reads + MFMAs without fills 1.18 us per K-tile against 0.77 us of MFMA issue); here that latency and the address-pipe time of a fill
// (a wave that issues an LDS-DMA instruction is held until the pipe accepts it) lie under the partner's MFMAs.  Price: two barriers per phase.
//   phase p of a wave:   [L]  fill one half-tile | fragment reads of the phase | (phase 4: counted vmcnt) | lgkmcnt(0) | barrier
//                        [M]  16 MFMAs                                                                                | barrier
//   K-tile t (parity b):  L1 W0(t+1) | wa (W rows 0-63: 8 reads), xa (tokens 0-31: 4)     M1 wa x xa
//                         L2 W1(t+1) | xb (tokens 32-63: 4)                               M2 wa x xb
//                         L3 X0(t+2) | wb (W rows 64-127: 8)                              M3 wb x xb
//                         L4 X1(t+2) | vmcnt(4): all but X0 / X1(t+2) landed              M4 wb x xa
// Group 1 starts one barrier late and group 0 ends one barrier late: barrier instance k closes group 0's section k and group 1's section k - 1.
// WAR: a slot is refilled at least one barrier after every wave's last read of it HAS RETURNED — the lgkmcnt(0) stands in FRONT of the barrier that ends a read section
// (X slots of parity b: last read L2(t), refilled L3(t) by group 0 while group 1 is in M2(t), its L2 reads retired before the barrier between; W slots: last read
// L3(t), refilled L1(t+1)).  RAW: a wave reads K-tile t+1 (from L1(t+1) on) only behind BOTH groups' vmcnt(4) of L4(t): group 0's own stands two barriers back, group
// 1's one barrier back (its L4(t) ends at the barrier that ends group 0's M4(t)); group 1 reads after group 0's by construction.  LDS-DMA data is ordered for a
// ds_read by exactly that: the issuing wave's counted vmcnt, then a barrier the reader has passed (MI355X_MICROARCH.md).
template <bool TR, typename AfterPrologue>
__device__ __forceinline__ void mainloop256_pp(const GemmParams& p, char* smem, int n0, int m0, int kt0, int nkt,
                                               f32x4 (&acc)[8][4], BlockStamps& bs, AfterPrologue after_prologue) {
    constexpr int PAR = 4 * TILE_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = w & 1, wm = w >> 1;
    const bool late = w >= 4;                        // group 1: one barrier interval behind group 0
    const int nktot = p.K / TK;
    const int last_wt = ((p.N + 127) >> 7) - 1, last_rt = (p.M - 1) >> 7;
    const int wt0 = n0 >> 7, wt1 = wt0 + 1 < last_wt ? wt0 + 1 : last_wt;     // ragged edges re-read a valid tile (masked)
    const int rt0 = (m0 >> 7) < last_rt ? (m0 >> 7) : last_rt, rt1 = (m0 >> 7) + 1 < last_rt ? (m0 >> 7) + 1 : last_rt;
    const size_t po = (size_t)(2 * w) * 1024 + lane * 16;
    const char* const sw0 = (const char*)p.W + ((size_t)wt0 * nktot + kt0) * TILE_BYTES + po;
    const char* const sw1 = (const char*)p.W + ((size_t)wt1 * nktot + kt0) * TILE_BYTES + po;
    const char* const sx0 = (const char*)p.X + ((size_t)rt0 * nktot + kt0) * TILE_BYTES + po;
    const char* const sx1 = (const char*)p.X + ((size_t)rt1 * nktot + kt0) * TILE_BYTES + po;
    char* const dst0 = smem + (2 * w) * 1024;
    auto stage = [&](const char* src, int h, int t) {
        const char* s = src + (size_t)t * TILE_BYTES;
        char* d = dst0 + (t & 1) * PAR + h * TILE_BYTES;
        glds16(s, d);
        glds16(s + 1024, d + 1024);
    };
    const int li = lane & 15, g = lane >> 4;
    int woff[2], xoff[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int ch = ((4 * s + g) ^ (li & 7)) << 4;
        woff[s] = wn * TILE_BYTES + li * 128 + ch;
        xoff[s] = (2 + (wm >> 1)) * TILE_BYTES + (64 * (wm & 1) + li) * 128 + ch;
    }
    auto mma = [&](const f16x8& wv, const f16x8& xv, f32x4& c) {
        if (TR) c = mfma16(xv, wv, c, 0, 0, 0);
        else c = mfma16(wv, xv, c, 0, 0, 0);
    };
    // end of a read / fill section: this wave's LDS reads have returned (the WAR rule above), then the barrier; nothing may be scheduled across
    auto end_l = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    auto end_m = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    stage(sx0, 2, 0); stage(sx1, 3, 0); stage(sw0, 0, 0); stage(sw1, 1, 0);
    if (nkt > 1) {
        stage(sx0, 2, 1); stage(sx1, 3, 1);
        asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    after_prologue();
    const bool fills = !GTAV_DBG(p, 1);
    GTAV_STAMP(bs.t[1]);
    if (late) end_m();                               // group 1 enters the loop one interval behind
    for (int t = 0; t < nkt; ++t) {
        const char* b = smem + (t & 1) * PAR;
        const bool n1 = t + 1 < nkt && fills, n2 = t + 2 < nkt && fills;
        f16x8 wa[2][4], wb[2][4], xa[2][2], xb[2][2];
        // ---- L1 / M1 ----
        if (n1) stage(sw0, 0, t + 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int j = 0; j < 2; ++j) xa[s][j] = *(const f16x8*)(b + xoff[s] + j * 16 * 128);
#pragma unroll
            for (int i = 0; i < 4; ++i) wa[s][i] = *(const f16x8*)(b + woff[s] + i * 16 * 128);
        }
        end_l();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma(wa[s][i], xa[s][j], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
        end_m();
        // ---- L2 / M2 ----
        if (n1) stage(sw1, 1, t + 1);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 2; ++j) xb[s][j] = *(const f16x8*)(b + xoff[s] + (2 + j) * 16 * 128);
        end_l();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma(wa[s][i], xb[s][j], acc[i][2 + j]);
        __builtin_amdgcn_s_setprio(0);
        end_m();
        // ---- L3 / M3 ----
        if (n2) stage(sx0, 2, t + 2);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) wb[s][i] = *(const f16x8*)(b + woff[s] + (4 + i) * 16 * 128);
        end_l();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma(wb[s][i], xb[s][j], acc[4 + i][2 + j]);
        __builtin_amdgcn_s_setprio(0);
        end_m();
        // ---- L4 / M4 ----
        if (n2) stage(sx1, 3, t + 2);
        __builtin_amdgcn_sched_barrier(0);
        if (n2) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");   // K-tile t + 1 complete (this wave's share): everything but X0 / X1(t+2)
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma(wb[s][i], xa[s][j], acc[4 + i][j]);
        __builtin_amdgcn_s_setprio(0);
        end_m();
    }
    if (!late) end_m();                              // group 0 leaves one interval late: every wave has executed the same number of barriers
}

// gemm256_kernel around the antiphase main loop (block shape 17): the same launch bounds, LDS array, bias prefetch and epilogue
template <int EPI>
__global__ __launch_bounds__(512, 1) void gemm256_pp_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(16))) char smem[8 * TILE_BYTES + (EPI == EPI_QKV ? 2048 : 0)];   // + qkv_staged's token table
    BlockStamps bs;
    bs.begin(p);
    int n0, m0, ks, kt0, nkt;
    tile_map<EPI == EPI_PARTIAL, 256, 256>(p, n0, m0, ks, kt0, nkt);
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool tr = false;
    f32x4 pbias[8];
    auto pf = [&]() { prefetch_bias<EPI, 8, 4>(p, n0, pbias); };
    auto nopf = []() {};
    if constexpr (EPI == EPI_QKV) {
        tr = (p.qkv_mode == QKV_SPATIAL) && (n0 >= 2 * p.D);
        if (tr) mainloop256_pp<true>(p, smem, n0, m0, kt0, nkt, acc, bs, nopf);
        else mainloop256_pp<false>(p, smem, n0, m0, kt0, nkt, acc, bs, nopf);
        pf();   // the QKV variant is at the 256-register limit: fetch after the main loop
    } else {
        mainloop256_pp<false>(p, smem, n0, m0, kt0, nkt, acc, bs, pf);
    }
    GTAV_STAMP(bs.t[2]);
    epilogue<EPI, 8, 4, 4>(p, acc, pbias, smem, n0, m0, ks, tr);
    bs.end(p);
}

// ---------------------------------------------------------------------------------------------------------------------
// Loader-wave GEMM with the WEIGHT operand straight into registers (shape 22, round 6).
//
// What bounds the loader-wave kernel at a few hundred tokens (the batch-1 window step: one 128 x 96 tile per CU, 16 K-steps) is how many fill bytes a CU keeps in
// flight against the latency of a weight that comes from HBM or the Infinity Cache: the ring holds NS - 1 = 3 stages of 28 KiB, of which 16 KiB are W — 48 KiB of W
// in flight per CU — and the K-step costs 0.45-0.5 us where ingest (64 B/clk) and the matrix pipes need 0.2-0.25 (profiles/round6/*per_class*: out-proj with 8
// K-steps 6.1 us, fc2's slices with 16 K-steps 9.9 us).  LDS capacity caps the ring; the register file does not: 8 compute waves x D = 4 K-steps x 4 KiB of W
// fragments = 128 KiB in flight per CU.  So here
//   * the compute waves load their OWN W fragments (16 features x 32 k per 16-byte lane load: the tile-major image makes a fragment half of eight 128-byte lines)
//     D K-steps ahead into a register ring (plain global loads: hipcc counts their vmcnt itself; the waves issue no other vector-memory operation in the loop);
//   * the loader waves move only X (the activations: L2-hot, 12 KiB per K-step) through the LDS ring, as before;
//   * W never touches LDS: the ring is 12 KiB per stage and the LDS array serves X fragment reads only.
// Price: the WM = 2 waves that share a W row tile each load it (W crosses the CU's texture path twice: 32 + 12 = 44 KiB of ingest per K-step against 28).
// ---------------------------------------------------------------------------------------------------------------------
template <bool TR, int NS, int FI, int FJ, int WN, int WM, int NL, int D, typename AfterPrologue>
__device__ __forceinline__ void mainloop_lw(const GemmParams& p, char* smem, int n0, int m0, int kt0, int nkt,
                                            f32x4 (&acc)[FI][FJ], BlockStamps& bs, AfterPrologue after_prologue) {
    static_assert(NS >= 3 && NL >= 1 && D >= 2 && D % 2 == 0 && (FI == 1 || FI == 2), "X ring of at least 3 stages; an even W register ring; 1 or 2 feature tiles per wave");
    constexpr int XPC = 2 * FJ * WM;                         // 1-KiB X pieces per stage
    constexpr int G = (XPC + NL - 1) / NL;
    constexpr int STAGE_BYTES = XPC * 1024;
    constexpr bool XDB = FI * FJ * 2 + 2 * FJ * 8 <= 96;     // X fragments of two K-steps in registers (one-step software pipeline) only while they fit
    const int tid = threadIdx.x, lane = tid & 63;
    const int wraw = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nktot = p.K / TK;
    if (wraw < NL) {
        // ------------------------------------------------ loader wave: X only ------------------------------------------------
        const int lw = wraw;
        const int last_rt = (p.M - 1) >> 7;
        const unsigned voff = (unsigned)lane * 16u;
        const unsigned smem0 = lds_offset(smem);
        const char* sb[G];
        unsigned ldso[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            int q = lw * G + i;
            q = q < XPC ? q : XPC - 1;                       // the last wave repeats the final piece (same bytes, same place)
            const int row = m0 + 8 * q;
            int rt = row >> 7;
            rt = rt < last_rt ? rt : last_rt;                // ragged edge: re-read a valid tile (results are masked)
            sb[i] = (const char*)p.X + ((size_t)rt * nktot + kt0) * TILE_BYTES + ((row & 127) >> 3) * 1024;
            ldso[i] = smem0 + q * 1024;
        }
        auto stage = [&](int t) {
            const unsigned so = (unsigned)(t % NS) * STAGE_BYTES;
            const size_t go = (size_t)t * TILE_BYTES;
#pragma unroll
            for (int i = 0; i < G; ++i) glds16_s(sb[i] + go, voff, ldso[i] + so);
        };
        const int npro = nkt < NS - 1 ? nkt : NS - 1;
        for (int t = 0; t < npro; ++t) stage(t);
        for (int t = 0; t < nkt; ++t) {
            wait_vm_ring<NS, G>(nkt - 1 - t);                // this wave's share of tile t has landed
            wg_barrier();
            if (t == 0) GTAV_STAMP(bs.t[1]);
            if (t + NS - 1 < nkt && !GTAV_DBG(p, 1)) stage(t + NS - 1);
        }
        return;
    }
    // ------------------------------------------------ compute wave ------------------------------------------------
    const int w = wraw - NL;
    const int wn = w % WN, wm = w / WN;
    const int li = lane & 15, g = lane >> 4;
    int xoff[2];
    // this lane's W fragment source: row n0 + 16 FI wn + 16 i + li of the tile-major weight, 16-byte chunk 4 s + g of its 128-byte row (common.h tiled_off)
    const int last_wt = ((p.N + 127) >> 7) - 1;
    const int wrow = n0 + 16 * FI * wn + li;                 // (+ 16 i: 16 FI WN <= 128 and n0 % 128 == 0 keep every i inside one row tile)
    int wrt = wrow >> 7;
    wrt = wrt < last_wt ? wrt : last_wt;
    int soff[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int ch = ((4 * s + g) ^ (li & 7)) << 4;
        xoff[s] = (16 * FJ * wm + li) * 128 + ch;
        soff[s] = ch;                                        // (row & 7) == (li & 7): n0 + 16 FI wn + 16 i is a multiple of 8
    }
    after_prologue();   // register loads the epilogue wants early (bias): OLDER than every W load, so the first W wait covers them
    // The W loads and their waits are inline asm with hand-counted vmcnt: behind plain loads hipcc's wait-count pass loses the ring at the loop's back edge and
    // drains to vmcnt(3) ... vmcnt(0) inside every K-step (seen in the first build of this loop: no load stayed in flight across a step).  A wait statement names
    // the registers it retires as in-out operands, so no use of them can be scheduled above it (the pattern of mainloop256_tn).  vmcnt retires in issue order
    // and these waves issue nothing else in the loop: when K-step u is consumed, the loads issued after its own are those of steps u + 1 .. min(u + D - 1, nkt - 1).
    f16x8 wr[D][2][FI];
    const unsigned wvoff0 = (unsigned)((wrow & 127) * 128 + soff[0]), wvoff1 = (unsigned)((wrow & 127) * 128 + soff[1]);
    const char* const wbase = (const char*)p.W + ((size_t)wrt * nktot + kt0) * TILE_BYTES;    // wave-uniform
    auto ldw = [&](int t, f16x8 (&dst)[2][FI]) {
        const char* sb = wbase + (size_t)t * TILE_BYTES;
#pragma unroll
        for (int i = 0; i < FI; ++i) {
            asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst[0][i]) : "v"(wvoff0), "s"(sb), "n"(i * 2048) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst[1][i]) : "v"(wvoff1), "s"(sb), "n"(i * 2048) : "memory");
        }
    };
    // slot `a` is consumed while the loads of YOUNGER later K-steps (2 FI each) may still be in flight.  ONE asm statement per call site and a compile-time count:
    // a run-time choice between wait statements makes the in-out registers phis of several definitions, and hipcc then copies them — in one of the paths AHEAD of
    // the wait, i.e. before the data has landed (seen in the second build of this loop).  Hence the loop below has no branch around a wait: a steady part in which
    // every step has D - 1 younger steps in flight, and a tail of exactly D steps with D - 1, ..., 0 (host-checked: K-steps per slice a multiple of D).
    auto wait_w = [&](f16x8 (&a)[2][FI], auto younger) {
        constexpr int CNT = decltype(younger)::value * 2 * FI;
        if constexpr (FI == 2) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]) : "n"(CNT));
        else asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a[0][0]), "+v"(a[1][0]) : "n"(CNT));
    };
#pragma unroll
    for (int d = 0; d < D; ++d) ldw(d, wr[d]);
    auto mmh = [&](const f16x8 (&wf)[FI], const f16x8 (&xv)[FJ]) {      // one 32-deep half of a K-step
#pragma unroll
        for (int i = 0; i < FI; ++i)
#pragma unroll
            for (int j = 0; j < FJ; ++j) {
                if (TR) acc[i][j] = mfma16(xv[j], wf[i], acc[i][j], 0, 0, 0);
                else acc[i][j] = mfma16(wf[i], xv[j], acc[i][j], 0, 0, 0);
            }
    };
    const bool domm = !GTAV_DBG(p, 2);
    auto rdx = [&](int t, f16x8 (&dst)[2][FJ]) {
        const char* b = smem + (t % NS) * STAGE_BYTES;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < FJ; ++j) dst[s][j] = *(const f16x8*)(b + xoff[s] + j * 16 * 128);
    };
    if constexpr (XDB) {
        // one-step software pipeline on the X side (as mainloop_l): barrier u + 1 | read X(u + 1) | MFMAs of K-step u (W from register slot u % D) | refill the slot with step u + D
        f16x8 xf[2][2][FJ];
        auto next_x = [&](int t, f16x8 (&dst)[2][FJ]) {    // barrier t (X stage t complete and visible), then its fragment reads
            wait_lgkm0();
            wg_barrier();
            rdx(t, dst);
        };
        auto mm = [&](const f16x8 (&wf)[2][FI], const f16x8 (&xv)[2][FJ]) { mmh(wf[0], xv[0]); mmh(wf[1], xv[1]); };
        next_x(0, xf[0]);
        GTAV_STAMP(bs.t[1]);
        auto steady = [&](int u0, auto dc) {
            constexpr int d = decltype(dc)::value;
            next_x(u0 + d + 1, xf[(d + 1) & 1]);
            wait_w(wr[d], std::integral_constant<int, D - 1>{});
            if (domm) mm(wr[d], xf[d & 1]);
            __builtin_amdgcn_sched_barrier(0);
            ldw(u0 + d + D, wr[d]);
            __builtin_amdgcn_sched_barrier(0);
        };
        auto tail = [&](int u0, auto dc) {
            constexpr int d = decltype(dc)::value;
            if constexpr (d + 1 < D) next_x(u0 + d + 1, xf[(d + 1) & 1]);
            wait_w(wr[d], std::integral_constant<int, D - 1 - d>{});
            if (domm) mm(wr[d], xf[d & 1]);
            __builtin_amdgcn_sched_barrier(0);
        };
        auto run = [&](auto&& f, int u0) {
            if constexpr (D == 4) { f(u0, std::integral_constant<int, 0>{}); f(u0, std::integral_constant<int, 1>{}); f(u0, std::integral_constant<int, 2>{}); f(u0, std::integral_constant<int, 3>{}); }
            else { static_assert(D == 8, "rings of 4 or 8 K-steps");
                   f(u0, std::integral_constant<int, 0>{}); f(u0, std::integral_constant<int, 1>{}); f(u0, std::integral_constant<int, 2>{}); f(u0, std::integral_constant<int, 3>{});
                   f(u0, std::integral_constant<int, 4>{}); f(u0, std::integral_constant<int, 5>{}); f(u0, std::integral_constant<int, 6>{}); f(u0, std::integral_constant<int, 7>{}); }
        };
        for (int u0 = 0; u0 < nkt - D; u0 += D) run(steady, u0);     // (nkt % D == 0: slot and X set of step u0 + d are d and d & 1)
        run(tail, nkt - D);
    } else {
        // wide token tiles (FJ = 6: 48 fragment registers per K-step): no second X set — barrier u | read both halves of X(u) | MFMAs half 0 behind lgkmcnt(FJ),
        // half 1 behind lgkmcnt(0) | refill.  The co-resident compute wave of the SIMD covers the LDS round trip.
        f16x8 xf[2][FJ];
        auto step = [&](int u, auto dc, auto yc, bool refill) {
            constexpr int d = decltype(dc)::value;
            wait_lgkm0();
            wg_barrier();
            if (u == 0) GTAV_STAMP(bs.t[1]);
            rdx(u, xf);
            wait_w(wr[d], yc);
            if (domm) { mmh(wr[d][0], xf[0]); mmh(wr[d][1], xf[1]); }
            __builtin_amdgcn_sched_barrier(0);
            if (refill) ldw(u + D, wr[d]);
            __builtin_amdgcn_sched_barrier(0);
        };
        static_assert(D == 8 || D == 4, "rings of 4 or 8 K-steps");
#define GTAV_LW_STEADY(dd) step(u0 + dd, std::integral_constant<int, dd>{}, std::integral_constant<int, D - 1>{}, true)
#define GTAV_LW_TAIL(dd) step(nkt - D + dd, std::integral_constant<int, dd>{}, std::integral_constant<int, D - 1 - dd>{}, false)
        for (int u0 = 0; u0 < nkt - D; u0 += D) {
            GTAV_LW_STEADY(0); GTAV_LW_STEADY(1); GTAV_LW_STEADY(2); GTAV_LW_STEADY(3);
            if constexpr (D == 8) { GTAV_LW_STEADY(4); GTAV_LW_STEADY(5); GTAV_LW_STEADY(6); GTAV_LW_STEADY(7); }
        }
        GTAV_LW_TAIL(0); GTAV_LW_TAIL(1); GTAV_LW_TAIL(2); GTAV_LW_TAIL(3);
        if constexpr (D == 8) { GTAV_LW_TAIL(4); GTAV_LW_TAIL(5); GTAV_LW_TAIL(6); GTAV_LW_TAIL(7); }
#undef GTAV_LW_STEADY
#undef GTAV_LW_TAIL
    }
}

template <int EPIX, int NS, int FI, int FJ, int WN, int WM, int NL, int D>
__global__ __launch_bounds__(64 * (WN * WM + NL), 1) void gemm_lw_kernel(GemmParams p) {
    constexpr int EPI = epi_base(EPIX);
    static_assert(!epi_is_fold_consumer(EPIX) && EPI != EPI_RESID_FOLD, "no LayerNorm-fold epilogues on this kernel");
    constexpr int TNB = 16 * FI * WN, TM = 16 * FJ * WM;
    static_assert(TNB <= 128 && 128 % TNB == 0, "a block's features stay inside one 128-row weight tile");
    extern __shared__ __attribute__((aligned(16))) char smem_l[];
    char* smem = smem_l;
#define GTAV_PIN_S(x) asm volatile("" ::"s"(x))
    GTAV_PIN_S(p.X); GTAV_PIN_S(p.W); GTAV_PIN_S(p.M); GTAV_PIN_S(p.N); GTAV_PIN_S(p.K); GTAV_PIN_S(p.splitk);
    GTAV_PIN_S(p.tm.tiles_m); GTAV_PIN_S(p.tm.tiles_n); GTAV_PIN_S(p.tm.gn); GTAV_PIN_S(p.tm.group); GTAV_PIN_S(p.tm.tiles);
    GTAV_PIN_S(p.tm.rcp_tiles); GTAV_PIN_S(p.tm.rcp_group); GTAV_PIN_S(p.tm.rcp_gn); GTAV_PIN_S(p.tm.rcp_gnlast);
    GTAV_PIN_S(p.bias); GTAV_PIN_S(p.out); GTAV_PIN_S(p.ldo); GTAV_PIN_S(p.qkv_mode); GTAV_PIN_S(p.D);
#undef GTAV_PIN_S
    BlockStamps bs;
    bs.begin(p);
    int n0, m0, ks, kt0, nkt;
    tile_map_fast<EPI == EPI_PARTIAL, TNB, TM>(p, n0, m0, ks, kt0, nkt);
    f32x4 acc[FI][FJ];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool tr = false;
    f32x4 pbias[FI];
    FoldTok<FJ> ft;
    auto pf = [&]() { prefetch_bias<EPI, FI, WM, WN, NL>(p, n0, pbias); };
    if constexpr (EPI == EPI_QKV) {
        tr = (p.qkv_mode == QKV_SPATIAL) && (n0 >= 2 * p.D);
        if (tr) mainloop_lw<true, NS, FI, FJ, WN, WM, NL, D>(p, smem, n0, m0, kt0, nkt, acc, bs, pf);
        else mainloop_lw<false, NS, FI, FJ, WN, WM, NL, D>(p, smem, n0, m0, kt0, nkt, acc, bs, pf);
    } else {
        mainloop_lw<false, NS, FI, FJ, WN, WM, NL, D>(p, smem, n0, m0, kt0, nkt, acc, bs, pf);
    }
    GTAV_STAMP(bs.t[2]);
    epilogue<EPIX, FI, FJ, WM, WN, NL, false>(p, acc, pbias, smem, n0, m0, ks, tr, acc, ft);
    bs.end(p);
}

// loader-wave kernel with the weight operand straight into registers (shape 22): dynamic LDS = the X ring, or the epilogue's image if that is larger
template <int EPI, int SHAPE, int D>
static int launch_lw(const GemmParams& p, int splitk, hipStream_t stream) {
    constexpr GemmShape R = *gemm_shape(SHAPE);
    static_assert(R.family == GF_LW, "gemm_lw_kernel");
    constexpr int NS = R.ns, FI = R.fi, FJ = R.fj, WN = R.wn, WM = R.wm, NL = R.nl, TNB = R.features(), TM = R.tokens();
    constexpr int RING = NS * 2 * FJ * WM * 1024;
    constexpr int PNB = (TNB / 8 + 7) / 8 * 8 * 16, PTB = (TM / 8 + 7) / 8 * 8 * 16;
    constexpr int EPIB = (TM * PNB > TNB * PTB ? TM * PNB : TNB * PTB) + TM * 8;      // qkv_staged's pitched image + token table (gemm_l_kernel)
    constexpr int GELUB = (TNB / 64 > 0 ? TNB / 64 : 1) * TM * 128;                     // the tile-major GELU image
    constexpr int LDS = RING > EPIB ? (RING > GELUB ? RING : GELUB) : (EPIB > GELUB ? EPIB : GELUB);
    if (int rc_ = lds_opt_in<gemm_lw_kernel<EPI, NS, FI, FJ, WN, WM, NL, D>>(LDS)) return rc_;
    GemmParams q = p;
    if (int rc_ = fill_tile_map(q.tm, p.M, p.N, TM, TNB, splitk, p.tm.gn)) return rc_;
    const dim3 grid(q.tm.tiles * splitk);
    GTAV_LAUNCH((gemm_lw_kernel<EPI, NS, FI, FJ, WN, WM, NL, D>), grid, dim3(R.threads()), LDS, stream, q);
    GTAV_CHECK_HIP(hipGetLastError());
    return 0;
}

// persistent 256-token-tile kernel (shapes 40 / 41): one block per CU; whole rounds of tiles + a two-way K split of a remainder of <= grid / 2 tiles
template <int EPI, int FI>
static int launch_p256(const GemmParams& p, hipStream_t stream) {
    using C = P256<FI>;
    int cus = 0;
    if (int rc_ = lds_opt_in<gemm_p256_kernel<EPI, FI>>(C::LDS, &cus)) return rc_;
    GemmParams q = p;
    GTAV_REQUIRE(p.K / TK % 2 == 0, "gemm: the persistent 256-token-tile kernel walks K in pairs of K-tiles (K = %d is not a multiple of 128)", p.K);
    int grid = 0;
    if (int rc_ = p256_units(q, cdiv(p.M, 256) * cdiv(p.N, C::TNB), cus, &grid)) return rc_;
    GTAV_LAUNCH((gemm_p256_kernel<EPI, FI>), dim3(grid), dim3(512), C::LDS, stream, q);
    GTAV_CHECK_HIP(hipGetLastError());
    return 0;
}

// Block shapes of the experiments build (tiles, thread counts and grids: the plan / the table, gemm_plan.h): what launch_epi ends with there.
template <int EPI>
static int launch_experiment_shape(const GemmParams& p, const GemmPlan& plan, hipStream_t stream) {
    constexpr bool FOLDISH = EPI == EPI_RESID_FOLD || epi_is_fold_consumer(EPI);
    const int shape = plan.shape, splitk = plan.splitk;
    if (shape == 27) return launch_l<EPI, 27>(p, plan, stream);
    if (shape == 28) return launch_l<EPI, 28>(p, plan, stream);
    if (shape == 42 || shape == 41 || shape == 40) {
        // 42: persistent 256 x 256 tiles on sixteen waves in two staggered groups (round 4); 41: persistent 256-token tiles (round 4), 192 x 256 (N x M);
        // 40: persistent 256 x 256 tiles, 128 accumulator registers — hipcc spills inside the K loop at the 256-register cap (117 us for fc1 at M = 5760)
        if constexpr (EPI == EPI_F32 || EPI == EPI_GELU_TANH || EPI == EPI_PARTIAL || EPI == EPI_F16_TILED) {
            GTAV_REQUIRE(splitk == 1 && p.N % 8 == 0, "gemm: the persistent 256-token-tile kernels split K themselves (one slab, N %% 8 == 0)");
            if (shape == 42) return launch_s16<EPI>(p, stream);
            if (shape == 41) return launch_p256<EPI, gemm_shape(41)->fi>(p, stream);
            return launch_p256<EPI, gemm_shape(40)->fi>(p, stream);
        } else {
            GTAV_REQUIRE(false, "gemm: the persistent 256-token-tile kernel (shape %d) has no epilogue %d", shape, (int)EPI);
        }
    }
    if (shape == 30 || shape == 32 || shape == 33) {
        // persistent loader-wave kernel variants, measured against shape 31 / the two-blocks-per-CU shapes (docs/LABNOTES.md 4.9): 30 (4-stage ring) ties 31; 32 / 33
        // (256 x 128 / 128 x 256) win back to back on cold operands (fc1 at M = 5760 67 -> 57 us) and LOSE inside the forward (54 -> 59-60 us)
        if (shape == 30) return launch_lp<EPI, 30>(p, plan, stream);
        if (shape == 32) return launch_lp<EPI, 32>(p, plan, stream);
        return launch_lp<EPI, 33>(p, plan, stream);
    }
    if constexpr (!FOLDISH) {
        // Round 6, measured SLOWER (profiles/round6/weight_operand_straight_into_registers_shapes_22_18.txt): the captured batch-1 step 2.05 -> 2.26 ms
        // (shape 22) / 2.12 -> 2.23 ms (shape 18), bit-identical results.  More weight bytes in flight per CU (128 KiB in registers against 48 KiB of the LDS ring) buy
        // nothing at M = 720: the K-step of the loader-wave kernel is not waiting for the weight.
        // shape 20's tile, the weight operand straight into registers 4 K-steps ahead (its K loop is written for K-steps per slice that are a multiple of 4: else shape 20)
        if (shape == 22) return (p.K / TK / splitk) % 4 == 0 ? launch_lw<EPI, 22, 4>(p, splitk, stream) : launch_l<EPI, 20>(p, plan, stream);
        // ... and with the eight compute waves side by side along the features (16 features x all 96 tokens each): every W fragment is loaded by exactly one wave,
        // 8 K-steps ahead
        if (shape == 18) return (p.K / TK / splitk) % 8 == 0 ? launch_lw<EPI, 18, 8>(p, splitk, stream) : launch_l<EPI, 20>(p, plan, stream);
        // Shape 7 (its grid, group width and narrow-output rule: the planner) with the two wave groups of a block in antiphase (gemm256_pp_kernel).  Round 6: correct,
        // race-screened (profiles/round6/race_screen_shape17.txt) and within +-1 % of shape 7 on the shapes that select it (fc2 / projection at M >= 11 520, fc1 -7 % at
        // M = 11 520 where shape 12 is still ahead of both at the model level): the K-tile is bound by how many fill bytes a CU keeps in flight, not by how its two
        // waves per SIMD interleave reads and MFMAs (profiles/round6/antiphase_256x256_main_loop_shape17_vs_shape7_vs_heuristic.txt: main loop 26.9 vs 27.2 us)
        if (shape == 17) {
            GEMM_LAUNCH((gemm256_pp_kernel<EPI>), dim3(plan.blocks), dim3(plan.threads));
            GTAV_CHECK_HIP(hipGetLastError());
            return 0;
        }
        // measured slower than the shapes the heuristic picks (docs/LABNOTES.md 4.1.1)
        if (shape == 21) return launch_l<EPI, 21>(p, plan, stream);
        if (shape == 23) return launch_l<EPI, 23>(p, plan, stream);
        if (shape == 25) return launch_l<EPI, 25>(p, plan, stream);
        if (shape == 16) {
            if constexpr (EPI == EPI_GELU_TANH || EPI == EPI_GELU_ERF || EPI == EPI_QKV || EPI == EPI_RESID) {
                GTAV_REQUIRE(gemm_pp_ok(p.M, p.N, p.K, EPI) || (p.K / TK >= 12 && p.M % 8 == 0 && p.N % 8 == 0),
                             "gemm: the ping-pong kernel needs K >= 768, M %% 8 == 0, N %% 8 == 0 (M=%d N=%d K=%d)", p.M, p.N, p.K);
                return launch_pp<EPI>(p, stream);
            } else {
                GTAV_REQUIRE(false, "gemm: the ping-pong kernel (shape 16) has no epilogue %d", (int)EPI);
            }
        }
        if (shape == 9) return launch_plain<EPI, 9>(p, plan, stream);
        if (shape == 8) {
            if constexpr (EPI == EPI_GELU_TANH || EPI == EPI_GELU_ERF || EPI == EPI_F16_TILED) {
                GTAV_REQUIRE(false, "gemm: the 96-feature tile has no tile-major (GELU) epilogue");
            } else {
                return launch_plain<EPI, 8>(p, plan, stream);
            }
        }
    }
    GTAV_REQUIRE(false, "gemm: block shape %d has no kernel for epilogue %d", shape, (int)EPI);
    return 0;
}

}  // namespace
