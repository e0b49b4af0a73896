/* gtav_amd — test hooks of libgtav_amd.so.  NOT part of the product interface (include/gtav_amd.h): nothing in a binding of the
 * reference's API needs them.  tests/ use them to run every GEMM block shape the launch heuristic can pick through every epilogue.
 *
 * All settings are PER THREAD (thread_local in csrc/gemm_plan.hip, one set for both operand types), like the handles: forcing a shape on one thread never
 * changes what another thread's handle launches.  Every choice computes the same result.  0 restores the heuristic.
 *   gtav_op_gemm_set_stages   LDS ring depth of the 128 x 128 tiles: 2 or 4
 *   gtav_op_gemm_set_wm       block shape, an id of the shape table GEMM_SHAPES in csrc/gemm_plan.h — the ONE place where a shape's tile, waves and ring are
 *                             defined; gtav_op_gemm_plan (gtav_amd.h) reports them, and tests/test_host_gemm_plan.py holds this list against the table:
 *                                id   features x tokens   compute [+ loader] waves
 *     2     128 x 128     4 waves
 *     3     128 x 128     8 waves
 *     7     256 x 256     8 waves
 *     11    64 x 48       6 waves
 *     12    128 x 192     8 waves
 *     13    128 x 96      4 waves
 *     14    64 x 96       6 waves
 *     20    128 x 96      8 + 4 waves   (loader-wave kernel, as 24 / 26 / 29)
 *     24    64 x 48       6 + 2 waves
 *     26    64 x 96       6 + 2 waves
 *     29    128 x 144     12 + 4 waves
 *     31    128 x 192     8 + 4 waves   (persistent loader-wave kernel, 3-stage ring; its 4-stage / 256 x 128 / 128 x 256 forms 30 / 32 / 33 and the
 *                             other laboratory shapes exist in the experiments build only: a product library refuses them by name)
 *                             Plus GTAV_GEMM_WM_NT_WEIGHT_FILLS (0x100; with a shape or with 0 = heuristic): every loader-wave
 *                             launch of the thread (shapes 20 / 24 / 26 / 29 and the two fused to_qkv + attention launches) fills its weight operand with the
 *                             non-temporal cache policy (GemmParams::wfill, the kernel side of gtav_dit_set_weight_fill_policy): the same bits again
 *                             (tests/test_gpu_launch_head.py)
 *
 * gtav_op_set_operand_dtype   operand type of the kernel-level entry points (gtav_op_*) that have no _bf16 sibling: GTAV_OPERAND_F16 (0, the default) or
 *                             GTAV_OPERAND_BF16 (1), PER THREAD like the two above.  With bf16 set, gtav_op_gemm_f16, gtav_op_gemm_qkv, gtav_op_ln_modulate,
 *                             gtav_op_ln_affine, gtav_op_attn_spatial[_prescaled], gtav_op_gemm_tn, gtav_op_gemm_dw_grouped, gtav_op_gemm_splitk_ln and
 *                             gtav_op_convert_f16 launch the bf16 twins (the objects a bf16 layer group of a handle runs) and every 2-byte buffer they read or
 *                             write holds bf16.  Entry points with a _bf16 sibling (attn_temporal, attn_spatial_bwd, attn_temporal_bwd) keep their fixed type, the
 *                             type-free ones (skinny_f32, rope_interleave, the elementwise math) are unaffected, and the fused fp16-only launches
 *                             (gtav_op_gemm_qkvt_attn, gtav_op_gemm_qkvs_attn, gtav_op_qkv_head_major[_spatial]) refuse by name.  At the default every entry point
 *                             launches what it launched before the hook existed.  gtav_op_gemm_set_stages / _set_wm set the forced shape of BOTH operand types.
 * gtav_op_attn_spatial_prescaled   gtav_op_attn_spatial on a q that already carries 1/8 log2 e (the form the VAE's flash attention runs, GemmParams::rope_cs_q);
 *                             refused at the sequence lengths whose kernel takes plain q.  Honours the operand type above.
 * tests/test_gpu_ops_typed.py runs every one of these in both operand types against fp64 math with per-element bounds.
 * (Timing experiments that change results, and the block shapes that measured slower than these, exist only in the separate
 * -DGTAV_EXPERIMENTS build: csrc/build.sh exp -> libgtav_amd_exp.so, loaded by tools/ only.) */
#ifndef GTAV_AMD_TESTING_H
#define GTAV_AMD_TESTING_H

#include <stdint.h>

#define GTAV_GEMM_WM_NT_WEIGHT_FILLS 0x100

#ifdef __cplusplus
extern "C" {
#endif

void gtav_op_gemm_set_stages(int32_t ns);
void gtav_op_gemm_set_wm(int32_t wm);
void gtav_op_set_operand_dtype(int32_t dtype);   /* GTAV_OPERAND_F16 (default) / GTAV_OPERAND_BF16, per thread */
int gtav_op_attn_spatial_prescaled(const void* q, const void* k, const void* vt, void* o, int32_t NB, int32_t heads, int32_t S, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GTAV_AMD_TESTING_H */
