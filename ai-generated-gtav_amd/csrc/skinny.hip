// Exact-fp32 "skinny" GEMM for the conditioning path (timestep MLP, action Linear, the adaLN
// mega-projection):  Y[m][n] = act( sum_k X[m][k] * W[n][k] + bias[n] ),  M = B*T rows (tens), N up to
// 198 656, K ~ 1 K.  The fp16 experiment in DESIGN.md shows this path alone costs 9.5e-4 rel-L2 if
// its operands are rounded to fp16, so it runs on v_mfma_f32_16x16x4_f32 (bit-for-bit an fp32 fma
// chain) with fp32 weights.  It is weight-streaming (HBM) bound: each wave streams 16 rows of W
// straight into registers (never reused), X (16 rows) sits in LDS.
#include "ops.h"

namespace gtav {
using namespace gtav_shared;   // the instantiation lists and the planner (launch_plan.h)

namespace {

// One block = 4 waves x FT feature tiles of 16 = 64 FT output features x one slab of 16 RT rows of X.  A wave reads each X fragment from LDS once per 32 k and uses it
// for its FT feature tiles; each W fragment comes straight from memory once and is used for the RT row tiles.  At tens of rows (FT = RT = 1) the launch is a weight
// stream; at hundreds — the adaLN table of a batch-8 frame, 808 rows x 198 656 features — FT = RT = 1 was bound by the LDS read per four MFMAs (11.3 ms = 30 TFLOP/s),
// FT = 4 by re-streaming W_ada once per 16 rows (7.2 ms = 5.9 TB/s out of L2 / Infinity Cache), hence 32-row slabs on top (tools/skinny_bench.py).  Per output the
// same fp32 fma chain in the same order for every FT / RT.
// KC = 0: the whole K of the slab is staged once (RT <= 2 at K = 1024).  KC > 0 (round 4): the slab is staged KC columns at a time, which lets a block keep 80-112 rows
// (RT = 5 .. 7): W_ada is then streamed ONCE for the 80 rows of a training batch / the 101 rows of a batch-1 frame instead of three or four times, and 9 instead of 26
// times for the 808 rows of a batch-8 frame.
template <int ACT, int FT, int RT, int KC = 0>
__global__ __launch_bounds__(256) void skinny_f32_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ Y, int ldy,
                                                        int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [16 RT][(KC ? KC : K) + 8]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.y * 16 * RT;
    const int n0 = (blockIdx.x * 4 + w) * 16 * FT;
    const int kspan = KC ? KC : K;          // columns staged at a time (K % KC == 0, host-checked)
    const int ldk = kspan + 8;
    const bool live = n0 < N;               // (with KC every wave takes part in the staging barriers)

    auto stage = [&](int k0) {              // rows beyond M are zero
        const int kq = kspan >> 2;
        for (int idx = tid; idx < 16 * RT * kq; idx += 256) {
            const int r = idx / kq, c = idx - r * kq;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (m0 + r < M) v = *(const f32x4*)(X + (size_t)(m0 + r) * ldx + k0 + 4 * c);
            *(f32x4*)(xs + r * ldk + 4 * c) = v;
        }
    };
    if constexpr (KC == 0) {
        stage(0);
        __syncthreads();
        if (!live) return;
    }

    const float* wp[FT];
#pragma unroll
    for (int f = 0; f < FT; ++f) {
        int nrow = n0 + 16 * f + li;
        nrow = nrow < N ? nrow : N - 1;
        wp[f] = W + (size_t)nrow * K + 4 * g;
    }
    const float* xp = xs + li * ldk + 4 * g;
    f32x4 acc[FT][RT];
#pragma unroll
    for (int f = 0; f < FT; ++f)
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[f][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // K % 32 == 0; each step covers 32 k: lane group g holds k = kb + 16 i + 4 g + e
    for (int k0 = 0; k0 < K; k0 += kspan) {
    if constexpr (KC != 0) {
        if (k0) __syncthreads();            // every wave has read the chunk before
        stage(k0);
        __syncthreads();
    }
    if (live)
#pragma unroll 2
    for (int kb = 0; kb < kspan; kb += 32) {
        f32x4 x0[RT], x1[RT], w0[FT], w1[FT];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            x0[t] = *(const f32x4*)(xp + (size_t)t * 16 * ldk + kb);
            x1[t] = *(const f32x4*)(xp + (size_t)t * 16 * ldk + kb + 16);
        }
#pragma unroll
        for (int f = 0; f < FT; ++f) {
            w0[f] = *(const f32x4*)(wp[f] + k0 + kb);
            w1[f] = *(const f32x4*)(wp[f] + k0 + kb + 16);
        }
#pragma unroll
        for (int f = 0; f < FT; ++f)
#pragma unroll
            for (int t = 0; t < RT; ++t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[f][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[f][e], x0[t][e], acc[f][t], 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[f][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[f][e], x1[t][e], acc[f][t], 0, 0, 0);
            }
    }
    }
    if (!live) return;
    // D[row = feature 4g + r][col = X row li]
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int m = m0 + 16 * t + li;
#pragma unroll
        for (int f = 0; f < FT; ++f) {
            const int n = n0 + 16 * f + 4 * g;
            if (m < M && n < N) {
                f32x4 v = acc[f][t];
                if (bias) v = v + *(const f32x4*)(bias + n);
                if (ACT == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.0f + expf(-v[e]));
                }
                *(f32x4*)(Y + (size_t)m * ldy + n) = v;
            }
        }
    }
}

}  // namespace

// what a launch of this problem runs: the launcher's own refusals, then the planner (launch_plan.hip skinny_plan: the measured (FT, RT) / K-chunk rules)
static int skinny_check_plan(int ldx, int ldy, int M, int N, int K, int act_silu, LaunchGeom* plan) {
    GTAV_REQUIRE(M > 0 && N > 0 && N % 4 == 0, "skinny: bad M=%d N=%d", M, N);
    // the bound on K is the LDS of ONE 16-row slab of X (what lds_opt_in raises the kernels to), not a round number: the second projection of the conditioning MLP reads
    // hidden + the padded action columns, 2080 at hidden 2048 — K <= 2048 refused every forward of that width with actions
    // (tests/test_gpu_models.py::test_hidden_2048_dit_forward_and_fused_spatial_switch)
    constexpr int SKINNY_MAX_K = (LAUNCH_LDS_MAX / (16 * (int)sizeof(float)) - 8) / 32 * 32;   // 2528
    GTAV_REQUIRE(K > 0 && K % 32 == 0 && K <= SKINNY_MAX_K, "skinny: K=%d must be a multiple of 32 and <= %d", K, SKINNY_MAX_K);
    GTAV_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && ldx >= K && ldy >= N, "skinny: bad leading dims");
    return skinny_plan(SkinnyProblem{M, N, K, act_silu != 0}, plan);
}
int skinny_launch_plan(const int* a, int* out12) {
    LaunchGeom plan;
    if (int rc_ = skinny_check_plan(a[2], a[1], a[0], a[1], a[2], a[3], &plan)) return rc_;
    launch_plan_report(SKINNY_KERNELS[plan.kernel], plan, 0, 0, 0, out12);
    return 0;
}

int launch_skinny_f32(const float* X, int ldx, const float* W, const float* bias, float* Y, int ldy, int M, int N,
                      int K, int act_silu, hipStream_t stream) {
    LaunchGeom plan;
    if (int rc_ = skinny_check_plan(ldx, ldy, M, N, K, act_silu, &plan)) return rc_;
    return dispatch_kernel<kernel_count(SKINNY_KERNELS)>(plan.kernel, [&](auto I) {
        constexpr KernelInst R = SKINNY_KERNELS[decltype(I)::value];
        if (int rc_ = lds_opt_in<skinny_f32_kernel<R.a, R.b, R.c, R.d>>(LAUNCH_LDS_MAX)) return rc_;
        hipLaunchKernelGGL((skinny_f32_kernel<R.a, R.b, R.c, R.d>), dim3(plan.gx, plan.gy), dim3(plan.block), plan.lds, stream, X, ldx, W, bias, Y, ldy, M, N, K);
        GTAV_CHECK_HIP(hipGetLastError());
        return 0;
    });
}

}  // namespace gtav
