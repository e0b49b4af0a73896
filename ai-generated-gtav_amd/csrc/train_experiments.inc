// Laboratory half of train.hip: compiled ONLY into libgtav_amd_exp.so (csrc/build.sh exp, -DGTAV_EXPERIMENTS), included by train.hip in front of the
// matrix-core kernel that replaced it.  The product library contains none of it.
//
// Spatial attention backward on the VALU (math, layouts and output: the comment in front of the include).  Kept for A/B runs against
// attn_spatial_bwd_mfma_kernel: GTAV_ATTN_BWD_VALU=1 makes launch_attn_spatial_bwd launch it.
// Query rows are processed 16 at a time: their P and dS rows live in LDS, dK / dV accumulate in registers (thread = (d, key group)).
#pragma once
__device__ __forceinline__ float dot8(const f16x8& a, const f16x8& b, float acc) {
    // v_dot2_f32_f16 (bf16 twin: v_dot2c_f32_bf16): two 2-byte products accumulated in fp32 per instruction
    acc = dot2acc(f16x2{a[0], a[1]}, f16x2{b[0], b[1]}, acc, false);
    acc = dot2acc(f16x2{a[2], a[3]}, f16x2{b[2], b[3]}, acc, false);
    acc = dot2acc(f16x2{a[4], a[5]}, f16x2{b[4], b[5]}, acc, false);
    acc = dot2acc(f16x2{a[6], a[7]}, f16x2{b[6], b[7]}, acc, false);
    return acc;
}
template <int NT>   // threads per block: NT / 16 query rows per row block, NT / 64 key groups
__global__ __launch_bounds__(NT) void attn_spatial_bwd_kernel(const f16* __restrict__ Q, const f16* __restrict__ K, const f16* __restrict__ Vt,
                                                              const f16* __restrict__ dO, int heads, int S, int D,
                                                              const float* __restrict__ rope_cs, f16* __restrict__ dqkv, int* err_flag) {
    constexpr int RB = NT / 16, JG = NT / 64;
    extern __shared__ __attribute__((aligned(16))) char smraw[];
    // rows of 64 halves padded to 72 (144 bytes): a 16-byte read of consecutive rows by consecutive lanes is bank-conflict free
    constexpr int LP = 72;
    f16* sQ = (f16*)smraw;                 // [S][LP]
    f16* sK = sQ + S * LP;
    f16* sV = sK + S * LP;                 // [S][LP] (transposed back from Vt)
    f16* sdO = sV + S * LP;
    float* sP = (float*)(sdO + S * LP);    // [RB][SP]
    const int SP = S + 4;                  // fp32 row pitch of the P / dS row blocks
    float* sdS = sP + RB * SP;
    const int item = blockIdx.x, nb = item / heads, head = item % heads;
    const int tid = threadIdx.x;
    const f16* q = Q + (size_t)item * S * 64;
    const f16* k = K + (size_t)item * S * 64;
    const f16* vt = Vt + (size_t)item * 64 * S;
    for (int i = tid; i < S * 8; i += NT) {        // 16-byte chunks
        const int s = i >> 3, ch = i & 7;
        *(uint4*)(sQ + s * LP + 8 * ch) = ((const uint4*)q)[i];
        *(uint4*)(sK + s * LP + 8 * ch) = ((const uint4*)k)[i];
        *(uint4*)(sdO + s * LP + 8 * ch) = *(const uint4*)(dO + ((size_t)nb * S + s) * D + head * 64 + 8 * ch);
    }
    for (int i = tid; i < S * 64; i += NT) {
        const int d = i / S, s = i % S;
        sV[s * LP + d] = vt[i];
    }
    __syncthreads();
    // dK / dV ownership: feature d_own, keys j = 4 JG c + 4 jg + e (e < 4): the P / dS rows are read as float4
    const int d_own = tid & 63, jg = tid >> 6;
    constexpr int CMAX = (AB_MAXS + 4 * JG - 1) / (4 * JG);
    f32x4 accK[CMAX], accV[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) accK[c] = accV[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ri = tid >> 4, cj = tid & 15;        // score ownership: query row ri of the RB-row block, keys cj, cj + 16, ...
    float amax = 0.f;
    for (int r0 = 0; r0 < S; r0 += RB) {
        const int i = r0 + ri;
        const bool iv = i < S;
        constexpr int NJ = AB_MAXS / 16;
        float sc[NJ], dp[NJ];
        float mx = -INFINITY;
        {
            // this thread's query row and its output-gradient row stay in registers for the whole block of keys
            f16x8 qr[8], gr[8];
            const int ic = iv ? i : S - 1;
#pragma unroll
            for (int ch = 0; ch < 8; ++ch) {
                qr[ch] = *(const f16x8*)(sQ + ic * LP + 8 * ch);
                gr[ch] = *(const f16x8*)(sdO + ic * LP + 8 * ch);
            }
#pragma unroll
            for (int c = 0; c < NJ; ++c) {
                const int j = cj + 16 * c;
                sc[c] = -INFINITY;
                dp[c] = 0.f;
                if (j < S) {
                    float a = 0.f, b = 0.f;
#pragma unroll
                    for (int ch = 0; ch < 8; ++ch) {
                        a = dot8(qr[ch], *(const f16x8*)(sK + j * LP + 8 * ch), a);
                        b = dot8(gr[ch], *(const f16x8*)(sV + j * LP + 8 * ch), b);
                    }
                    if (iv) {
                        sc[c] = a * 0.125f;
                        dp[c] = b;
                        mx = fmaxf(mx, sc[c]);
                    }
                }
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < NJ; ++c) {
            sc[c] = (cj + 16 * c < S && iv) ? __expf(sc[c] - mx) : 0.f;
            sum += sc[c];
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        const float inv = sum > 0.f ? 1.0f / sum : 0.f;
        float dsum = 0.f;
#pragma unroll
        for (int c = 0; c < NJ; ++c) {
            sc[c] *= inv;
            dsum += sc[c] * dp[c];
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) dsum += __shfl_xor(dsum, o, 64);
#pragma unroll
        for (int c = 0; c < NJ; ++c) {
            const int j = cj + 16 * c;
            if (j < S) {       // rows beyond S hold zeros (sc = 0): the dK / dV loops below may read all 16 rows
                sP[ri * SP + j] = sc[c];
                sdS[ri * SP + j] = sc[c] * (dp[c] - dsum) * 0.125f;
            }
        }
        __syncthreads();
        // dQ rows of this block: 16 x 64 outputs, 4 per thread (row ri, features 4 cj .. 4 cj + 3); RoPE^T; store
        if (iv) {
            float dq[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < S; j += 4) {
                const f32x4 w4 = *(const f32x4*)(sdS + ri * SP + j);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const f16x4 kx = *(const f16x4*)(sK + (j + jj) * LP + 4 * cj);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dq[e] += w4[jj] * (float)kx[e];
                }
            }
            const f32x4 cs = *(const f32x4*)(rope_cs + (size_t)i * 64 + 4 * cj);
            const float o0 = dq[0] * cs[0] + dq[1] * cs[1], o1 = dq[1] * cs[0] - dq[0] * cs[1];
            const float o2 = dq[2] * cs[2] + dq[3] * cs[3], o3 = dq[3] * cs[2] - dq[2] * cs[3];
            *(f16x4*)(dqkv + tiled_off(nb * S + i, head * 64 + 4 * cj, 3 * D)) = sat4(o0, o1, o2, o3, amax);
        }
        // dV[j][d] += sum_r P[r][j] dO[r][d];  dK[j][d] += sum_r dS[r][j] Q[r][d]   (rows past S contribute zeros)
        const int rows = min(RB, S - r0);
        for (int r = 0; r < rows; ++r) {
            const float go = (float)sdO[(r0 + r) * LP + d_own], qq = (float)sQ[(r0 + r) * LP + d_own];
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                const int j = 4 * JG * c + 4 * jg;
                if (j < S) {
                    accV[c] += *(const f32x4*)(sP + r * SP + j) * go;
                    accK[c] += *(const f32x4*)(sdS + r * SP + j) * qq;
                }
            }
        }
        __syncthreads();
    }
    // dK (RoPE^T needs the pair partner: lanes d and d ^ 1 are neighbours in the wave) and dV
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * JG * c + 4 * jg + e;
            if (j < S) {      // uniform per wave: j depends on jg (= the wave index), c and e only
                const float mine = accK[c][e], other = __shfl_xor(mine, 1, 64);
                const float co = rope_cs[(size_t)j * 64 + (d_own & ~1)], si = rope_cs[(size_t)j * 64 + (d_own | 1)];
                const float dk = (d_own & 1) ? mine * co - other * si : mine * co + other * si;
                const size_t m = (size_t)nb * S + j;
                amax = fmaxf(amax, fmaxf(fabsf(dk), fabsf(accV[c][e])));
                dqkv[tiled_off((int)m, D + head * 64 + d_own, 3 * D)] = (f16)__builtin_amdgcn_fmed3f(dk, -F16_MAX, F16_MAX);
                dqkv[tiled_off((int)m, 2 * D + head * 64 + d_own, 3 * D)] = (f16)__builtin_amdgcn_fmed3f(accV[c][e], -F16_MAX, F16_MAX);
            }
        }
    }
    sat_report(amax, err_flag);
}

// What launch_attn_spatial_bwd needs of it: the knob, the kernel's dynamic LDS, and the launch (with its per-device opt-in to more than 64 KiB)
static int g_attn_bwd_valu = GTAV_ENV_INT("GTAV_ATTN_BWD_VALU", 0);   // 1 = this kernel instead of attn_spatial_bwd_mfma_kernel (A/B runs)
constexpr int AB_VALU_NT = 512;
static size_t attn_bwd_valu_lds(int S) { return (size_t)4 * S * 72 * 2 + (size_t)2 * (AB_VALU_NT / 16) * (S + 4) * 4; }
static int launch_attn_bwd_valu(const f16* Q, const f16* K, const f16* Vt, const f16* dO, int NB, int heads, int S, int D, const float* rope_cs, f16* dqkv,
                                int* err_flag, hipStream_t stream) {
    if (int rc_ = lds_opt_in<attn_spatial_bwd_kernel<AB_VALU_NT>>(LAUNCH_LDS_MAX)) return rc_;
    hipLaunchKernelGGL(attn_spatial_bwd_kernel<AB_VALU_NT>, dim3(NB * heads), dim3(AB_VALU_NT), attn_bwd_valu_lds(S), stream, Q, K, Vt, dO, heads, S, D, rope_cs, dqkv, err_flag);
    GTAV_CHECK_HIP(hipGetLastError());
    return 0;
}
