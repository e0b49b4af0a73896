// Layout of the parameter structs that cross from the fp16 objects into their bf16 twins (ops_bf16.h): api.hip / api_train.hip hand a gtav::GemmParams,
// LnPending, GemmDwGroup, AdamParam or AdamItem to a gtav_bf16 launcher through a reference cast, so the twin namespace's struct must have the same size and the
// same field offsets.  The constants live here once; every translation unit asserts ITS OWN structs against them (ops.h includes this header at its end, inside
// the namespace that -Dgtav=gtav_bf16 renames): a field added, moved or resized in one of the two builds only is a compile error, never a silent
// misread.  A deliberate change of a struct updates its list here (sizes and offsets of an x86-64 / gfx950 build: pointers and size_t are 8 bytes).
#pragma once
#include <cstddef>

// F(field, byte offset) for every field, in declaration order
#define GTAV_LAYOUT_GemmParams_SIZE 352
#define GTAV_LAYOUT_GemmParams(F) \
    F(X, 0) F(ldx, 8) F(W, 16) F(M, 24) F(N, 28) F(K, 32) F(debug, 36) F(stamps, 40) F(err_flag, 48) F(out_sc1, 56) F(splitk, 60) F(bias, 64) \
    F(out2, 72) F(out, 80) F(ldo, 88) F(gate, 96) F(gate_stride, 104) F(gate_rows, 112) F(rows_per_gate, 120) F(qkv_mode, 124) F(q, 128) F(k, 136) \
    F(v, 144) F(D, 152) F(S, 156) F(Tq, 160) F(t0, 164) F(Tmax, 168) F(rope_cs, 176) F(rope_cs_q, 184) F(tm, 192) F(f_P, 228) F(f_rows, 232) \
    F(f_stats, 240) F(f_nslot, 248) F(f_c1, 256) F(f_c2, 264) F(f_ldc, 272) F(f_stats_out, 280) F(f_scale, 288) F(f_a, 296) F(pf, 304) F(sk_ws, 328) \
    F(sk_flags, 336) F(sk_dp, 344) F(sk_r, 348)
#define GTAV_LAYOUT_LnPending_SIZE 104
#define GTAV_LAYOUT_LnPending(F) \
    F(parts, 0) F(nsplit, 8) F(slab_stride, 16) F(ld, 24) F(bias, 32) F(gate, 40) F(gate_stride, 48) F(gate_rows, 56) F(rows_per_gate, 64) \
    F(flags, 68) F(err_flag, 72) F(x_out, 80) F(y_save, 88) F(tperm_T, 96) F(tperm_P, 100)
#define GTAV_LAYOUT_GemmDwGroup_SIZE 40
#define GTAV_LAYOUT_GemmDwGroup(F) \
    F(X, 0) F(W, 8) F(out, 16) F(M, 24) F(N, 28) F(ldo, 32)
#define GTAV_LAYOUT_AdamParam_SIZE 80
#define GTAV_LAYOUT_AdamParam(F) \
    F(p, 0) F(ldp, 8) F(R, 12) F(C, 16) F(g, 24) F(m, 32) F(v, 40) F(w16, 48) F(Cp16, 56) F(wT, 64) F(RpT, 72)
#define GTAV_LAYOUT_AdamItem_SIZE 8
#define GTAV_LAYOUT_AdamItem(F) \
    F(param, 0) F(start, 4)

#define GTAV_LAYOUT_ASSERT_FIELD_(S, f, off) static_assert(offsetof(S, f) == (off), #S "::" #f " is not at the offset its twin expects (struct_layout.h)");
#define GTAV_LAYOUT_FIELD_GemmParams(f, off) GTAV_LAYOUT_ASSERT_FIELD_(GemmParams, f, off)
#define GTAV_LAYOUT_FIELD_LnPending(f, off) GTAV_LAYOUT_ASSERT_FIELD_(LnPending, f, off)
#define GTAV_LAYOUT_FIELD_GemmDwGroup(f, off) GTAV_LAYOUT_ASSERT_FIELD_(GemmDwGroup, f, off)
#define GTAV_LAYOUT_FIELD_AdamParam(f, off) GTAV_LAYOUT_ASSERT_FIELD_(AdamParam, f, off)
#define GTAV_LAYOUT_FIELD_AdamItem(f, off) GTAV_LAYOUT_ASSERT_FIELD_(AdamItem, f, off)
// in the namespace that declares S (ops.h): sizeof(S) and every field offset of THIS translation unit's S against the constants above
#define GTAV_LAYOUT_ASSERT(S)                                                                                                      \
    static_assert(sizeof(S) == GTAV_LAYOUT_##S##_SIZE, "sizeof(" #S ") differs from the size its twin expects (struct_layout.h)"); \
    GTAV_LAYOUT_##S(GTAV_LAYOUT_FIELD_##S)
