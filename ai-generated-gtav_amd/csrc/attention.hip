// Attention kernels for gfx950.
//
// attn_spatial: non-causal attention over S tokens per (frame, head), head_dim 64, on v_mfma_f32_16x16x32_f16:
//     S^T = K . Q^T          (keys on accumulator ROWS, queries on lanes)
//     softmax                (row max / sum = in-lane + two cross-lane steps)
//     O^T += Vt . P^T        (P^T is taken straight from the S^T accumulators: the k-slot -> key map is applied to the Vt read instead,
//                             so P never moves between lanes or through LDS)
//   attn_spatial_1p_kernel   S <= 160 (the DiT's 144 frame tokens): K / Vt of the head resident in LDS, one pass per query tile
//   attn_flash_kernel        longer sequences (the VAE's 576 tokens): K / Vt streamed through an LDS ring, flash form (round 5)
//
// attn_temporal: causal attention over the <= 8 frames of the sliding window per (b, position, head);
// 25 dot products of length 64 per head: VALU + 16-lane xor-shuffle reductions, everything in registers.
#include "ops.h"
#include "attn_tile.h"

#include <cstdlib>

namespace gtav {
using namespace gtav_shared;   // the instantiation lists and the planner (launch_plan.h)

namespace {

constexpr float kScaleLog2e = kAttnQScale;  // 1/sqrt(64) * log2(e)

// SHORT sequences (S_pad = 16 NK <= 160 keys: the DiT's 144 patch tokens per frame; round 4): one block per (frame, head[, q-split]); K [S][64] (rows XOR-swizzled
// for conflict-free ds_read_b128) and Vt [64][S] (rows padded) of the head are staged once in LDS, every wave then walks 16-query tiles in ONE pass: the scores
// of all NK key tiles live in registers (4 NK floats per lane), one row maximum, one exponential per score, then the PV products — no online-softmax rescale and
// no dependency between key blocks (the online-softmax kernel of round 1 walked a query tile as three serial QK^T -> max -> exp -> rescale -> PV rounds: 17.7 us
// per launch at batch 8 against a 9.4 us traffic floor).  softmax(QK^T / 8) V is computed with one fp32 rounding order for every batch size and both sampling
// algorithms (the kernel is chosen by S alone).
template <int NW, int NK>
__global__ __launch_bounds__(64 * NW) void attn_spatial_1p_kernel(const f16* __restrict__ Q, const f16* __restrict__ K,
                                                              const f16* __restrict__ Vt, f16* __restrict__ O, int heads, int S,
                                                              int qsplit, int sc1) {
    constexpr int S_pad = 16 * NK;
    static_assert(NK % 2 == 0 && NK <= 10, "an even number of 16-key tiles, at most 160 keys");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                              // [S_pad][128 B], 16-B chunk c of row r stored at c ^ (r & 7)
    constexpr int vstride = (S_pad + 8) * 2;      // bytes per Vt row
    char* Vs = smem + (size_t)S_pad * 128;        // [64][S_pad + 8] halves
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int bh = blockIdx.x;                    // nb * heads + head
    const int nb = bh / heads, head = bh - nb * heads;
    const f16* Kg = K + (size_t)bh * S * 64;
    const f16* Vg = Vt + (size_t)bh * 64 * S;
    const f16* Qg = Q + (size_t)bh * S * 64;
    const int nqt = (S + 15) >> 4;
    constexpr int NT = 64 * NW;
    const int qt_first = blockIdx.y * NW + w;
    f16x8 qpre[2] = {};
    if (qt_first < nqt) {
        int qr = qt_first * 16 + li;
        qr = qr < S ? qr : S - 1;
        qpre[0] = *(const f16x8*)(Qg + (size_t)qr * 64 + 8 * g);
        qpre[1] = *(const f16x8*)(Qg + (size_t)qr * 64 + 32 + 8 * g);
    }
    {   // stage K (swizzled) and Vt (padded), zero the padding: every load of a batch before the first LDS write (one memory round trip)
        constexpr int nk = S_pad * 8, vchunks = (S_pad + 8) / 8, nv = 64 * vchunks, nmax = nk > nv ? nk : nv;
        for (int base = tid; base < nmax; base += NT * 6) {
            uint4 kv[6], vv[6];
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                const int idx = base + u * NT;
                kv[u] = make_uint4(0, 0, 0, 0);
                if (idx < nk && (idx >> 3) < S) kv[u] = *(const uint4*)(Kg + (size_t)(idx >> 3) * 64 + (idx & 7) * 8);
            }
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                const int idx = base + u * NT;
                vv[u] = make_uint4(0, 0, 0, 0);
                if (idx < nv) {
                    const int d = idx / vchunks, c = idx - d * vchunks;
                    if (c * 8 < S) vv[u] = *(const uint4*)(Vg + (size_t)d * S + c * 8);  // S % 8 == 0
                }
            }
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                const int idx = base + u * NT;
                if (idx < nk) {
                    const int r = idx >> 3, c = idx & 7;
                    *(uint4*)(Ks + r * 128 + ((c ^ (r & 7)) << 4)) = kv[u];
                }
            }
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                const int idx = base + u * NT;
                if (idx < nv) {
                    const int d = idx / vchunks, c = idx - d * vchunks;
                    *(uint4*)(Vs + d * vstride + c * 16) = vv[u];
                }
            }
        }
    }
    __syncthreads();
    const int Dm = heads * 64;
    for (int qt = qt_first; qt < nqt; qt += NW * qsplit) {
        const int q0 = qt * 16;
        f16x8 qf[2];
        if (qt == qt_first) {
            qf[0] = qpre[0];
            qf[1] = qpre[1];
        } else {
            int qr = q0 + li;
            qr = qr < S ? qr : S - 1;
            qf[0] = *(const f16x8*)(Qg + (size_t)qr * 64 + 8 * g);
            qf[1] = *(const f16x8*)(Qg + (size_t)qr * 64 + 32 + 8 * g);
        }
        attn_1p_tile<NK>(Ks, Vs, qf, S, q0, O, nb * S + q0, head * 64, Dm, lane, sc1);   // attn_tile.h: shared with the fused to_qkv + attention GEMM
    }
}

// ---- long sequences (S_pad > 160: the VAE's 576 tokens per frame; round 5) ---------------------------------------------------------------
// The kernel of rounds 1-4 kept ALL of K / Vt of a (frame, head) in LDS (148 KB at S = 576: one 4-wave block per CU, whose 144 KB prologue load nothing hid)
// and walked 16-query tiles one at a time with an online softmax, so every K / Vt fragment read from LDS fed ONE MFMA (64 B/clk/SIMD = the whole LDS bandwidth
// at the MFMA issue rate) and every 64-key block paid the rescale: 0.106-0.117 of the MFMA peak at 40-80 frames x 16 heads
// (profiles/round4/train_step_kernel_stats.csv, profiles/round5/attn_flash_S576_ab_first_version.txt; removed in round 5).  This kernel is the flash form of the same arithmetic:
//   * a block = 4 waves x NQT 16-query tiles (NQT = 3: 192 queries; S = 576 is three blocks per (frame, head), whose ids are 8 apart = one XCD's L2
//     under round-robin placement, speed only); several blocks per CU (48 KiB of LDS, <= 168 registers)
//   * K / Vt arrive in 64-key blocks by LDS-DMA (global_load_lds_dwordx4, 4 pieces per wave and block) into a 3-slot ring: counted vmcnt, ONE barrier
//     per key block, block kb + 2 in flight while block kb is consumed; the bank swizzles are applied to the per-lane SOURCE address (the LDS image
//     of an LDS-DMA is lane-linear): K rows chunk ^ kswz(key), Vt rows chunk ^ ((d >> 1) & 7): every fragment is one conflict-free ds_read_b128
//   * every K / Vt fragment feeds NQT MFMAs; S^T = K Q^T and O^T += Vt P^T with the operand maps of the kernels above (P^T straight from the score registers)
//   * scores live in the exponent's own unit: Q carries 1/8 log2 e (applied in fp32 by the to_qkv epilogue — GemmParams::rope_cs_q — or, for callers with
//     plain q, by this kernel on the fp16 fragments), and the reference maximum is the C INPUT of the score MFMAs (S' = K Q^T - mref comes out of the
//     matrix pipe), so a probability is ONE v_exp_f32; the reference maximum moves only when a score exceeds it by more than 8 (P <= 2^8: exact in fp16
//     to the same 11 bits; the sums are fp32): detection is lane-local (8 v_max3 + 1 compare per query tile), the cross-lane maximum (v_permlane16_swap /
//     v_permlane32_swap) and the rescale of O are a rare wave-uniform branch; the row sums are a fifth output tile of the PV product (a ones A operand:
//     6 more MFMAs per key block instead of 48 additions per lane, and no cross-lane sum at the end)
//   profiles/round5/attn_flash_*: 373 -> 159 us (first version) -> see there, per 80-frame x 16-head launch
constexpr float kLazyThr = 8.0f;   // in exponent units (log2)
// Plain q on bf16 operands: q * (1/8 log2 e) rounded to bf16 again is an error of up to 2^-9 per element ahead of a dot product with k — against a key of
// large norm that is percents of a probability (tests/test_gpu_ops_typed.py: the running-max-jump case missed its per-row bound by it).  The twin therefore
// scales q by 1/8 only (a power of two: exact) and keeps its scores in the natural logarithm's unit: the factor log2 e goes onto the fp32 score in front of
// v_exp_f32, and the threshold is the same factor 2^8 in that unit.  The fp16 objects (11-bit q, the rounding is 8 times smaller) are unchanged.
#ifdef GTAV_BF16_OPERANDS
constexpr bool kPlainQNaturalUnit = true;
#else
constexpr bool kPlainQNaturalUnit = false;
#endif

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
constexpr int attn_waitcnt_imm(int vm, int lgkm) { return (vm & 15) | (7 << 4) | ((lgkm & 15) << 8) | ((vm >> 4) << 14); }

// 16-byte direct-to-LDS load, scalar-base form: address = sbase (SGPR pair) + voff (32-bit per-lane byte offset); LDS destination = lds_addr (-> M0) + lane * 16
__device__ __forceinline__ void glds16_s_attn(const void* sbase, unsigned voff, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_addr) : "memory");
}
// bank swizzle of the K rows of the flash kernel (16-byte chunk c of key row r sits at c ^ kswz(r)): its lanes read the rows 8 (li >> 2) + (li & 3) (+ 4),
// and with (r & 7) the lanes li and li + 12 / li + 4 and li + 8 of a ds_read_b128 lane group would share banks; bits 1, 3, 4 of the row separate all sixteen
__device__ __forceinline__ int kswz(int r) { return ((r >> 1) & 1) | (((r >> 3) & 3) << 1); }
// max over the four lanes li, li + 16, li + 32, li + 48 (every lane ends with the result)
__device__ __forceinline__ float max_over_g(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);   // rows 1 <-> 0, 3 <-> 2
    v = fmaxf(__builtin_bit_cast(float, (unsigned)a[0]), __builtin_bit_cast(float, (unsigned)a[1]));
    const unsigned w = __builtin_bit_cast(unsigned, v);
    auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);   // lanes 32-63 <-> 0-31
    return fmaxf(__builtin_bit_cast(float, (unsigned)b[0]), __builtin_bit_cast(float, (unsigned)b[1]));
}
template <int NQT, int OCC, bool RAGGED, bool PRESCALED>   // OCC = blocks per CU the register budget must admit; RAGGED: S % 64 != 0; PRESCALED: Q holds q / 8 log2 e
__global__ __launch_bounds__(256, OCC) void attn_flash_kernel(const f16* __restrict__ Q, const f16* __restrict__ K, const f16* __restrict__ Vt,
                                                            f16* __restrict__ O, int heads, int S, int nfh, int nqb, int sc1) {
    constexpr bool NAT = !PRESCALED && kPlainQNaturalUnit;   // scores in units of ln, not log2 (see kPlainQNaturalUnit)
    constexpr float kLog2e = 1.4426950408889634f, kThr = NAT ? kLazyThr * 0.6931471805599453f : kLazyThr;
    const bool dbg_force = (sc1 & 2) != 0;
    constexpr int SLOT = 16384, NSLOT = 3;          // per slot: K block [64 keys][128 B] | Vt block [64 d][128 B]
    __shared__ __attribute__((aligned(1024))) char smem[NSLOT * SLOT];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: the LDS-DMA base goes to M0 (no waterfall loop)
    const int li = lane & 15, g = lane >> 4;
    // block -> ((frame, head), query block).  The nqb query blocks of one (frame, head) re-read the same K / Vt: give them ids that are 8 apart
    int fh, qb;
    {
        const int bid = blockIdx.x;
        if ((nfh & 7) == 0) {
            const int x = bid & 7, j = bid >> 3, fl = j / nqb;
            qb = j - fl * nqb;
            fh = fl * 8 + x;
        } else {
            fh = bid / nqb;
            qb = bid - fh * nqb;
        }
    }
    const int nb = fh / heads, head = fh - nb * heads;
    const f16* Kg = K + (size_t)fh * S * 64;
    const f16* Vg = Vt + (size_t)fh * 64 * S;
    const f16* Qg = Q + (size_t)fh * S * 64;
    const int qt0 = (qb * 4 + w) * NQT;            // first 16-query tile of this wave

    // LDS-DMA of key block kb into ring slot `slot`: 8 K pieces + 8 Vt pieces of 1 KiB (8 rows of 128 B each); wave w owns pieces 2 w, 2 w + 1 of both.
    // Rows / columns beyond S are clamped to valid memory (finite values): their scores are masked and their probabilities are exactly 0.
    // The fills are inline asm in the scalar-base form (wave-uniform base + 32-bit lane offset): behind the builtin, hipcc's wait-count pass assumes
    // every later ds_read may alias a fill in flight and drains vmcnt(0) in front of the first fragment read of EVERY key block (the ring's prefetch gone).
    const int prow = lane >> 3, pcp = lane & 7;
    const unsigned smem_base = (unsigned)(size_t)(lptr_t)smem;
    unsigned kvo[2], vvo[2];          // per-lane source offsets (bytes) of this wave's two K / two Vt pieces inside key block 0
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = 8 * (2 * w + i) + prow;     // key row / feature row of the piece's lane
        kvo[i] = (unsigned)(r * 128 + ((pcp ^ kswz(r)) << 4));
        vvo[i] = (unsigned)(r * S * 2 + ((pcp ^ ((r >> 1) & 7)) << 4));
    }
    auto issue = [&](int kb, int slot) {
        const unsigned base = smem_base + slot * SLOT + 2 * w * 1024;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            unsigned off = kvo[i] + (unsigned)(kb * 8192);
            if constexpr (RAGGED) {               // clamp the ROW to the last valid key, keep the chunk
                const int rowoff = (int)(off & ~127u), klast = (S - 1) * 128;
                off = (unsigned)(rowoff < klast ? rowoff : klast) + (off & 127u);
            }
            glds16_s_attn(Kg, off, base + i * 1024);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            unsigned off = vvo[i] + (unsigned)(kb * 128);
            if constexpr (RAGGED) {               // clamp the 8-key chunk to the last valid one (S % 8 == 0)
                const int r = 8 * (2 * w + i) + prow, col = kb * 64 + ((pcp ^ ((r >> 1) & 7)) << 3);
                off = (unsigned)(r * S * 2) + (unsigned)((col < S ? col : S - 8) * 2);
            }
            glds16_s_attn(Vg, off, base + 8192 + i * 1024);
        }
    };

    const int nkb = (S + 63) >> 6;
    issue(0, 0);
    if (nkb > 1) issue(1, 1);

    f16x8 qf[NQT][2];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        int qr = (qt0 + qt) * 16 + li;
        qr = qr < S ? qr : S - 1;
        qf[qt][0] = *(const f16x8*)(Qg + (size_t)qr * 64 + 8 * g);
        qf[qt][1] = *(const f16x8*)(Qg + (size_t)qr * 64 + 32 + 8 * g);
    }
    // The compiler's own wait for the Q loads must sit HERE, ahead of the loop (the empty asm "uses" the registers): left to the first MFMA it lands INSIDE
    // the loop, and since the wait-count pass cannot see the inline-asm fills it is a vmcnt(0) that drains the ring's prefetch in every key block
    // (vmcnt retires in order: the first two key blocks, issued before Q, have landed here too)
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) asm volatile("" : "+v"(qf[qt][0]), "+v"(qf[qt][1]));
    if constexpr (!PRESCALED) {   // plain q: the exponent's unit goes onto the fp16 fragments here (one more fp16 rounding of q than the prescaled form)
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[qt][h][e] = (f16)((float)qf[qt][h][e] * (NAT ? 0.125f : kScaleLog2e));
    }

    // per-lane LDS offsets of the fragment reads inside a slot.  Key tile kt holds the keys 32 (kt >> 1) + 8 (i >> 2) + 4 (kt & 1) + (i & 3) on its rows i
    // (a lane simply reads that K row): the score registers of tiles 2 s and 2 s + 1 are then the P^T operand of the keys 32 s + 8 g .. + 7 in natural
    // order, and the Vt fragment of a lane is ONE 16-byte read (chunk 4 s + g of feature row d) instead of two 8-byte reads 32 bytes apart
    int koff[2][2];   // [kt & 1][k-step]  (+ (kt >> 1) * 4096)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int r = 8 * (li >> 2) + 4 * e + (li & 3);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) koff[e][ks] = r * 128 + (((4 * ks + g) ^ kswz(r)) << 4);
    }
    int voff[2];      // [s2]  (+ dt * 2048)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) voff[s2] = 8192 + li * 128 + (((4 * s2 + g) ^ ((li >> 1) & 7)) << 4);

    f32x4 o[NQT][5];      // [4] = the row sums: O^T tile of an all-ones feature tile (every row of it holds sum_k P[k][q])
    float nmref[NQT];     // minus the reference maximum of the lane's query: splat, it is the C operand of the score MFMAs
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        nmref[qt] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) o[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (f16)1.0f;

    int slot = 0;
    for (int kb = 0; kb < nkb; ++kb) {
        // this wave's pieces of block kb have landed (block kb + 1 may still be in flight); the barrier then (a) makes every wave's pieces visible and
        // (b) proves every wave has finished reading block kb - 1, whose slot block kb + 2 overwrites
        if (kb + 1 < nkb) __builtin_amdgcn_s_waitcnt(attn_waitcnt_imm(4, 15));
        else __builtin_amdgcn_s_waitcnt(attn_waitcnt_imm(0, 15));
        asm volatile("s_barrier" ::: "memory");
        if (kb + 2 < nkb) issue(kb + 2, slot >= 1 ? slot - 1 : NSLOT - 1);
        const char* sb = smem + slot * SLOT;
        slot = slot + 1 < NSLOT ? slot + 1 : 0;

        // ---- S' = K Q^T - mref: 4 key tiles x NQT query tiles, every K fragment feeds NQT MFMAs ----
        f32x4 sc[NQT][4], cin[NQT];
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) cin[qt] = f32x4{nmref[qt], nmref[qt], nmref[qt], nmref[qt]};
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const f16x8 k0 = *(const f16x8*)(sb + (kt >> 1) * 4096 + koff[kt & 1][0]);
            const f16x8 k1 = *(const f16x8*)(sb + (kt >> 1) * 4096 + koff[kt & 1][1]);
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                sc[qt][kt] = mfma16(k0, qf[qt][0], cin[qt], 0, 0, 0);
                sc[qt][kt] = mfma16(k1, qf[qt][1], sc[qt][kt], 0, 0, 0);
            }
        }
        if constexpr (RAGGED) {
            if (kb * 64 + 64 > S) {   // padded keys exist only in the last block (wave-uniform)
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kb * 64 + 32 * (kt >> 1) + 8 * g + 4 * (kt & 1) + r >= S) {
#pragma unroll
                            for (int qt = 0; qt < NQT; ++qt) sc[qt][kt][r] = -INFINITY;
                        }
            }
        }
        // ---- does any score exceed its reference maximum by more than the threshold?  Lane-local: every key sits in some lane ----
        // Signed-INTEGER maxima of the score bits: a positive float is its bit pattern in integer order and every negative one is a negative integer, which is
        // all that "some score > 8" needs (v_max3_i32; behind fmaxf hipcc canonicalises every MFMA result with a v_max_f32 x, x, x of its own, and inline
        // asm must not read MFMA results: the compiler pads that hazard only for instructions it emits itself)
        bool need = kb == 0 || dbg_force;   // the first block SETS the reference maximum (with cin = 0 a row of very negative scores would underflow to a zero sum)
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            int im = (int)0x80000000;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                // (every element through a scalar float first: __builtin_bit_cast applied to the vector subscript itself read element 0 four times — hipcc, ROCm 7.2)
                const float s0 = sc[qt][kt][0], s1 = sc[qt][kt][1], s2_ = sc[qt][kt][2], s3 = sc[qt][kt][3];
                im = max(max(__float_as_int(s0), __float_as_int(s1)), im);
                im = max(max(__float_as_int(s2_), __float_as_int(s3)), im);
            }
            need = need || (im > __float_as_int(kThr));
        }
        if (__any(need)) {   // rare after the first block: a jump of the maximum.  Everything at the old reference is rescaled exactly once, the pending scores re-based
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                float m = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    m = __builtin_fmaxf(__builtin_fmaxf(sc[qt][kt][0], sc[qt][kt][1]), m);
                    m = __builtin_fmaxf(__builtin_fmaxf(sc[qt][kt][2], sc[qt][kt][3]), m);
                }
                const float bm = max_over_g(m);
                const float delta = kb == 0 ? bm : __builtin_fmaxf(bm, 0.f);   // the reference only ever rises after the first block
                if (kb != 0) {
                    const float alpha = __builtin_amdgcn_exp2f(NAT ? -delta * kLog2e : -delta);
#pragma unroll
                    for (int dt = 0; dt < 5; ++dt) o[qt][dt] = o[qt][dt] * alpha;
                }
                nmref[qt] -= delta;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[qt][kt][r] -= delta;
            }
        }
        // ---- P = 2^S' (one v_exp_f32 per score), then O^T += Vt P^T: two 32-key steps x (4 feature tiles + the ones tile); every Vt fragment feeds NQT MFMAs ----
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            f16x8 pf[NQT];
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (NAT) {
                        pf[qt][r] = (f16)__builtin_amdgcn_exp2f(sc[qt][2 * s2][r] * kLog2e);
                        pf[qt][4 + r] = (f16)__builtin_amdgcn_exp2f(sc[qt][2 * s2 + 1][r] * kLog2e);
                    } else {
                        pf[qt][r] = (f16)__builtin_amdgcn_exp2f(sc[qt][2 * s2][r]);
                        pf[qt][4 + r] = (f16)__builtin_amdgcn_exp2f(sc[qt][2 * s2 + 1][r]);
                    }
                }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const f16x8 vf = *(const f16x8*)(sb + dt * 2048 + voff[s2]);
#pragma unroll
                for (int qt = 0; qt < NQT; ++qt) o[qt][dt] = mfma16(vf, pf[qt], o[qt][dt], 0, 0, 0);
            }
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) o[qt][4] = mfma16(ones, pf[qt], o[qt][4], 0, 0, 0);
        }
    }

    const int Dm = heads * 64;
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        const float inv = 1.0f / o[qt][4][0];
        const int qrow = (qt0 + qt) * 16 + li;
        if (qrow < S) {
            const int mrow = nb * S + qrow;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                f16x4 h;
#pragma unroll
                for (int r = 0; r < 4; ++r) h[r] = (f16)(o[qt][dt][r] * inv);
                store_f16x4_paired<16>(O + tiled_off(mrow, head * 64 + dt * 16 + 4 * g, Dm), h, lane, sc1 & 1);
            }
        }
    }
}

// One thread per 8 consecutive features (16-byte loads / stores; 8 lanes per head), D/8 threads per (b, p) column and as many
// columns per block as fit in 256 threads; grid = (column groups, query-frame group): with `split` every query frame of a column
// gets its own block, which loads only the K / V frames its causal mask admits — five times as many independent blocks for the
// 144-column batch-1 step (one block per column left 112 of 256 CUs idle and chained five softmaxes per thread).
// q.k uses v_dot2_f32_f16 (exact fp16 products, fp32 accumulation), the head reduction is DPP, exp is the raw v_exp_f32.
// TM = compile-time bound on the number of frames (5 for the DiT's window, 8 otherwise): the frame loops are fully unrolled.
template <int TM>
__global__ __launch_bounds__(256) void attn_temporal_kernel(const f16* __restrict__ q, const f16* __restrict__ kv,
                                                            f16* __restrict__ O, int ncol, int P, int D, int Tq, int t0, int Tmax,
                                                            int split) {
    const int tpc = D >> 3;                                     // threads per column
    const int ci = threadIdx.x / tpc, lc = threadIdx.x - ci * tpc;
    const int bp = blockIdx.x * ((int)blockDim.x / tpc) + ci;
    if (bp >= ncol) return;                                     // whole 8-lane head groups leave together (tpc % 8 == 0)
    const int b = bp / P, p = bp - b * P;
    const int c = lc * 8;
    const int tl_lo = split ? blockIdx.y : 0, tl_hi = split ? blockIdx.y + 1 : Tq;
    const int Tk = t0 + tl_hi;                    // frames 0 .. t0 + tl_hi - 1 are visible to the last query of this block
    union H8 { f16x8 v; f16x2 h[4]; };
    H8 k8[TM], v8[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        if (t < Tk) {
            const f16* base = kv + (((size_t)b * Tmax + t) * P + p) * 2 * D;
            k8[t].v = *(const f16x8*)(base + c);
            v8[t].v = *(const f16x8*)(base + D + c);
        }
    }
    // every query row of this block is fetched up front, together with K / V (one memory round trip for the block)
    H8 qall[TM];
#pragma unroll
    for (int tl = 0; tl < TM; ++tl)
        if (tl >= tl_lo && tl < tl_hi) qall[tl].v = *(const f16x8*)(q + (((size_t)b * Tq + tl) * P + p) * D + c);
#pragma unroll
    for (int tl = 0; tl < TM; ++tl) {
        if (tl >= tl_hi) break;
        if (tl < tl_lo) continue;
        const int tq = t0 + tl;
        const size_t row = ((size_t)b * Tq + tl) * P + p;
        float s[TM];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < TM; ++t) {
            s[t] = -INFINITY;
            if (t <= tq) {  // causal (model/attention.py:62-64), wave-uniform
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) d = dot2acc(qall[tl].h[e], k8[t].h[e], d, false);
                s[t] = group8_sum(d) * 0.125f;
                mx = fmaxf(mx, s[t]);
            }
        }
        float den = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TM; ++t) {
            if (t <= tq) {
                const float pr = __builtin_amdgcn_exp2f((s[t] - mx) * 1.4426950408889634f);   // argument <= 0
                den += pr;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(pr, (float)v8[t].v[e], acc[e]);   // explicit fma: the fused QKV + attention GEMM (gemm.hip) must round identically
            }
        }
        const float inv = 1.0f / den;
        f16x8 o8;
#pragma unroll
        for (int e = 0; e < 8; ++e) o8[e] = (f16)(acc[e] * inv);
        *(f16x8*)(O + tiled_off((int)row, c, D)) = o8;
    }
}

// Windows of 9 .. 32 visible frames (t0 + Tq > 8).  The register-resident kernel above cannot be instantiated there (3 x 32 x 4 VGPRs of
// K / V / Q per lane), so this one keeps the QUERIES in registers and streams the cache past them: same thread map (8 features per lane,
// 8 lanes per head, D/8 lanes per column, 16-byte loads, whole 2 D-half cache rows per column), grid.y = groups of QG query frames.
// A block reads frames 0 .. t0 + (its last query) once, FB frames per round trip with the next FB already in flight, and folds every
// frame into the running softmax (m, den, acc[8]) of each query that may see it; whole frames beyond a query's causal limit are skipped
// by wave-uniform branches, frames >= t0 + Tq are never loaded.
// The arithmetic of one query is a fixed sequence over keys 0 .. t0 + tl that depends on nothing else (not on QG, FB, the group it
// falls in or the other queries of the block): the window launch (Tq = T) and the context-cached launch (Tq = 1, QG = 1) give the same
// bits.  Rescaling on a new maximum is a per-lane condition (a lane whose maximum stands multiplies by nothing), so the skipped
// branch changes no value either.
template <int QG, int FB>
__global__ __launch_bounds__(256) void attn_temporal_stream_kernel(const f16* __restrict__ q, const f16* __restrict__ kv,
                                                                   f16* __restrict__ O, int ncol, int P, int D, int Tq, int t0, int Tmax) {
#pragma clang fp contract(off)   // both instantiations must round alike: only the explicit fma below is fused
    const int tpc = D >> 3;                                     // threads per column
    const int ci = threadIdx.x / tpc, lc = threadIdx.x - ci * tpc;
    const int bp = blockIdx.x * ((int)blockDim.x / tpc) + ci;
    if (bp >= ncol) return;                                     // whole 8-lane head groups leave together (tpc % 8 == 0); no barrier below
    const int b = bp / P, p = bp - b * P;
    const int c = lc * 8;
    const int tl0 = blockIdx.y * QG;
    const int nq = Tq - tl0 < QG ? Tq - tl0 : QG;               // queries of this block: frames t0 + tl0 .. t0 + tl0 + nq - 1
    const int Tk = t0 + tl0 + nq;                               // frames 0 .. Tk - 1 are visible to its last query
    union H8 { f16x8 v; f16x2 h[4]; };
    H8 qv[QG];
    float m[QG], den[QG], acc[QG][8];
#pragma unroll
    for (int j = 0; j < QG; ++j) {
        qv[j].v = f16x8{};
        if (j < nq) qv[j].v = *(const f16x8*)(q + (((size_t)b * Tq + tl0 + j) * P + p) * D + c);
        m[j] = -INFINITY; den[j] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
    }
    const size_t fstride = (size_t)P * 2 * D;                   // halves between two frames of one column
    const f16* const base = kv + ((size_t)b * Tmax * P + p) * 2 * D + c;
    H8 kc[FB], vc[FB];
#pragma unroll
    for (int i = 0; i < FB; ++i) {
        kc[i].v = f16x8{}; vc[i].v = f16x8{};
        if (i < Tk) {
            kc[i].v = *(const f16x8*)(base + i * fstride);
            vc[i].v = *(const f16x8*)(base + i * fstride + D);
        }
    }
    for (int tb = 0; tb < Tk; tb += FB) {
        H8 kn[FB], vn[FB];
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            kn[i].v = f16x8{}; vn[i].v = f16x8{};
            if (tb + FB + i < Tk) {
                kn[i].v = *(const f16x8*)(base + (size_t)(tb + FB + i) * fstride);
                vn[i].v = *(const f16x8*)(base + (size_t)(tb + FB + i) * fstride + D);
            }
        }
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            const int t = tb + i;
            if (t < Tk) {
                float vf[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) vf[e] = (float)vc[i].v[e];
#pragma unroll
                for (int j = 0; j < QG; ++j) {
                    if (j < nq && t <= t0 + tl0 + j) {  // causal (model/attention.py:62-64), wave-uniform
                        float d = 0.f;
#pragma unroll
                        for (int e = 0; e < 4; ++e) d = dot2acc(qv[j].h[e], kc[i].h[e], d, false);
                        const float s = group8_sum(d) * 0.125f;
                        if (s > m[j]) {                 // new maximum (always at t = 0: m = -inf gives a factor 2^-inf = 0 on den = acc = 0)
                            const float r = __builtin_amdgcn_exp2f((m[j] - s) * 1.4426950408889634f);
                            den[j] *= r;
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[j][e] *= r;
                            m[j] = s;
                        }
                        const float pr = __builtin_amdgcn_exp2f((s - m[j]) * 1.4426950408889634f);   // argument <= 0
                        den[j] += pr;
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[j][e] = __builtin_fmaf(pr, vf[e], acc[j][e]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < FB; ++i) { kc[i] = kn[i]; vc[i] = vn[i]; }
    }
#pragma unroll
    for (int j = 0; j < QG; ++j) {
        if (j < nq) {
            const size_t row = ((size_t)b * Tq + tl0 + j) * P + p;
            const float inv = 1.0f / den[j];
            f16x8 o8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float r = acc[j][e] * inv;
                asm volatile("" : "+v"(r));   // the product is rounded to fp32 first in every instantiation (no v_fma_mix fold of multiply + conversion: one rounding less)
                o8[e] = (f16)r;
            }
            *(f16x8*)(O + tiled_off((int)row, c, D)) = o8;
        }
    }
}

}  // namespace

// output as paired 16-byte write-through stores (common.h store_f16x4_paired); experiments build: GTAV_ATTN_SC1=1 enables it
static int g_attn_sc1 = GTAV_ENV_INT("GTAV_ATTN_SC1", 0) | (GTAV_ENV_INT("GTAV_ATTN_DBG_FORCE", 0) ? 2 : 0);   // measured neutral at B = 1 (attention re-reads nothing, writes little)

bool attn_spatial_wants_prescaled_q(int S) { return S > 0 && S % 8 == 0 && round_up(S, 32) > 160; }

// what a launch of this problem runs: the launcher's own refusals, then the planner (launch_plan.hip: the one-pass / flash rules, query split and NQT tie rule)
static int attn_spatial_check_plan(int NB, int heads, int S, bool q_prescaled, AttnSpatialPlan* plan) {
    GTAV_REQUIRE(S > 0 && S % 8 == 0, "attn_spatial: S=%d must be a positive multiple of 8", S);
    GTAV_REQUIRE(!q_prescaled || attn_spatial_wants_prescaled_q(S), "attn_spatial: S=%d runs a kernel that takes plain q", S);
    if (int rc_ = attn_spatial_plan(AttnSpatialProblem{NB, heads, S, q_prescaled}, plan)) return rc_;
    GTAV_REQUIRE(ATTN_SPATIAL_KERNELS[plan->kernel].family != LF_ATTN_FLASH || ((long long)NB * heads * plan->nqb < (1ll << 31) && (long long)S * 64 * 2 < (1ll << 31)),
                 "attn_spatial: grid / sequence too large");
    return 0;
}
int launch_attn_spatial(const f16* Q, const f16* K, const f16* Vt, f16* O, int NB, int heads, int S, hipStream_t stream, bool q_prescaled) {
    AttnSpatialPlan plan;
    if (int rc_ = attn_spatial_check_plan(NB, heads, S, q_prescaled, &plan)) return rc_;
    const dim3 grid(plan.gx, plan.gy), block(plan.block);
    return dispatch_kernel<kernel_count(ATTN_SPATIAL_KERNELS)>(plan.kernel, [&](auto I) {
        constexpr KernelInst R = ATTN_SPATIAL_KERNELS[decltype(I)::value];
        if constexpr (!R.product && !GTAV_LAB_BUILD) {
            GTAV_REQUIRE(false, "attn_spatial: this kernel exists only in the experiments build (csrc/build.sh exp)");
        } else if constexpr (R.family == LF_ATTN_1P) {
            if (int rc_ = lds_opt_in<attn_spatial_1p_kernel<R.a, R.b>>(LAUNCH_LDS_MAX)) return rc_;
            GTAV_LAUNCH((attn_spatial_1p_kernel<R.a, R.b>), grid, block, plan.lds, stream, Q, K, Vt, O, heads, S, plan.qsplit, g_attn_sc1 & 1);
        } else {
            GTAV_LAUNCH((attn_flash_kernel<R.a, R.b, R.c != 0, R.d != 0>), grid, block, 0, stream, Q, K, Vt, O, heads, S, NB * heads, plan.nqb, g_attn_sc1);
        }
        GTAV_CHECK_HIP(hipGetLastError());
        return 0;
    });
}

static int attn_temporal_check_plan(int B, int P, int D, int Tq, int t0, int Tmax, AttnTemporalPlan* plan) {
    GTAV_REQUIRE(D % 256 == 0 && D <= 2048, "attn_temporal: D=%d must be a multiple of 256 and <= 2048", D);
    GTAV_REQUIRE(Tq > 0 && t0 >= 0 && t0 + Tq <= Tmax && Tmax <= 32, "attn_temporal: window t0=%d Tq=%d Tmax=%d (max 32)", t0, Tq, Tmax);
    GTAV_REQUIRE(P > 0 && B > 0 && (long long)B * Tq * P < (1ll << 31), "attn_temporal: B=%d P=%d Tq=%d", B, P, Tq);
    return attn_temporal_plan(AttnTemporalProblem{B * P, D, Tq, t0}, plan);
}
int launch_attn_temporal(const f16* q, const f16* kv, f16* O, int B, int P, int D, int Tq, int t0, int Tmax,
                         hipStream_t stream) {
    AttnTemporalPlan plan;
    if (int rc_ = attn_temporal_check_plan(B, P, D, Tq, t0, Tmax, &plan)) return rc_;
    const dim3 grid(plan.gx, plan.gy), block(plan.block);
    return dispatch_kernel<kernel_count(ATTN_TEMPORAL_KERNELS)>(plan.kernel, [&](auto I) {
        constexpr KernelInst R = ATTN_TEMPORAL_KERNELS[decltype(I)::value];
        if constexpr (R.family == LF_ATTN_T) GTAV_LAUNCH(attn_temporal_kernel<R.a>, grid, block, 0, stream, q, kv, O, B * P, P, D, Tq, t0, Tmax, plan.split);
        else GTAV_LAUNCH((attn_temporal_stream_kernel<R.a, R.b>), grid, block, 0, stream, q, kv, O, B * P, P, D, Tq, t0, Tmax);
        GTAV_CHECK_HIP(hipGetLastError());
        return 0;
    });
}

// gtav_op_launch_plan, kinds 1 (a = NB, heads, S, q_prescaled) and 2 (a = B, P, D, Tq, t0, Tmax)
int attn_launch_plan(int kind, const int* a, int* out12) {
    if (kind == 1) {
        AttnSpatialPlan plan;
        if (int rc_ = attn_spatial_check_plan(a[0], a[1], a[2], a[3] != 0, &plan)) return rc_;
        launch_plan_report(ATTN_SPATIAL_KERNELS[plan.kernel], plan, plan.qsplit, plan.nqb, 0, out12);
    } else {
        AttnTemporalPlan plan;
        if (int rc_ = attn_temporal_check_plan(a[0], a[1], a[2], a[3], a[4], a[5], &plan)) return rc_;
        launch_plan_report(ATTN_TEMPORAL_KERNELS[plan.kernel], plan, plan.split, 0, 0, out12);
    }
    return 0;
}

}  // namespace gtav
