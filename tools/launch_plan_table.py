#!/usr/bin/env python3
"""What the launch planner (csrc/launch_plan.hip) selects for the non-GEMM launchers: the table tests/test_host_launch_plan.py pins.

    python tools/launch_plan_table.py                    # print the table of the library in the tree
    python tools/launch_plan_table.py --write            # rewrite tests/launch_plan_parent.json (a pull request that changes a rule ON PURPOSE does this and shows the diff)
    python tools/launch_plan_table.py --lib other.so     # any library that exports gtav_op_launch_plan

Needs no GPU: gtav_op_launch_plan touches no device.  Per launcher family: `rows` = [inputs..., plan] at the models' own sizes, `sweep` = the change points
[inputs..., plan] of a dense sweep whose last input runs fastest; a change is a change of the family's `key` fields of the plan (kernel, block, splits: what a
rule decides; the grid and LDS at a change point are recorded with it).  plan = the twelve integers of gtav_op_launch_plan (include/gtav_amd.h), or
[return code, message] where the launcher refuses the problem."""
import argparse
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "launch_plan_parent.json")

LN, ATTN_S, ATTN_T, ATTN_S_BWD, ATTN_T_BWD, SKINNY, GEMM_TN, GEMM_NN, ADA_BWD, LN_BWD_FUSED = range(10)   # the kinds of gtav_op_launch_plan
SEL = (0, 1, 2, 3, 4, 7, 9, 10, 11)       # plan fields that are a selection: family, template arguments, block, the family's own numbers
ALL = tuple(range(12))
WIDTHS = (128, 192, 256, 512, 1024, 2048)
LN_FORMS = ((0, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (0, 0, 0, 1), (0, 1, 0, 0), (1, 1, 0, 0))   # slabs, permutation, k_save, k_load
LN_M = (1, 4, 5, 144, 720, 1152, 5760, 46080)
NBH = (1, 16, 80, 128, 511, 512, 1280, 4096)
SKINNY_N = (256, 1024, 6144, 65536, 198656)
SKINNY_K = (256, 1024, 1056, 2080, 2528)


def families():
    """name -> (kind, key fields, rows, sweep groups); a group is a list of input tuples, swept in order."""
    f = {}
    f["layernorm"] = (LN, SEL,
                      [(mode, M) + form + (D,) for mode in (0, 1) for M in LN_M for form in LN_FORMS for D in (256, 512, 1024, 2048)],
                      [[(mode, M) + form + (D,) for D in range(64, 2048 + 1, 64)] for mode in (0, 1) for M in LN_M for form in LN_FORMS])
    S_sweep = list(range(8, 640 + 1, 8)) + [1024, 4096]
    f["attn_spatial"] = (ATTN_S, SEL,
                         [(pre, nbh, S) for pre in (0, 1) for nbh in NBH for S in (64, 144, 160, 168, 576, 1024, 4096)],
                         [[(pre, nbh, S) for S in S_sweep] for pre in (0, 1) for nbh in NBH])
    windows = [(Tq, t0) for Tq in range(1, 33) for t0 in range(0, 33 - Tq)]
    f["attn_temporal"] = (ATTN_T, SEL,
                          [(D, bp, Tq, t0) for D in (256, 1024, 2048) for bp in (32, 144, 1023, 1024, 5760)
                           for Tq, t0 in ((1, 0), (5, 0), (1, 4), (1, 5), (8, 0), (1, 7), (9, 0), (1, 8), (16, 0), (32, 0), (1, 31))],
                          [[(D, bp, Tq, t0) for Tq, t0 in windows] for D in (256, 1024, 2048) for bp in (32, 144, 1023, 1024, 5760)])
    f["attn_spatial_bwd"] = (ATTN_S_BWD, ALL, [(1280, S) for S in (64, 144, 160, 168, 576, 15360)],
                             [[(80, S) for S in list(range(8, 640 + 1, 8)) + list(range(15344, 15400, 8))]])
    f["attn_temporal_bwd"] = (ATTN_T_BWD, ALL, [(16, 144, 256, 5), (2, 144, 1024, 8), (2, 144, 1024, 9)],
                              [[(B, 144, D, T) for T in range(1, 34)] for B, D in ((2, 1024), (16, 256))])
    skinny_m = list(range(1, 129)) + [808, 1616]   # (101 is in the range)
    f["skinny"] = (SKINNY, SEL,
                   [(act, N, K, M) for act in (0, 1) for N in SKINNY_N for K in SKINNY_K for M in (1, 5, 16, 32, 33, 80, 101, 128, 808, 1616)],
                   [[(act, N, K, M) for M in skinny_m] for act in (0, 1) for N in SKINNY_N for K in SKINNY_K + (2560,)])
    odd = WIDTHS + (32, 100)
    f["gemm_tn_f32"] = (GEMM_TN, ALL, [], [[(80, N, K) for N in odd for K in odd]])
    f["gemm_nn_f32"] = (GEMM_NN, ALL, [], [[(R, N, K) for N in WIDTHS + (100, 1040, 2064, 4096, 4112) for R in (1, 4, 5, 8, 9, 16, 17, 80) for K in (64, 256, 1056)]])
    f["ada_bwd_dx"] = (ADA_BWD, ALL, [], [[(MODW, D, R) for D in WIDTHS + (1000,) for R in (1, 5, 80, 81, 128) for MODW in (1024, 1025, 2048, 2049, 6144, 198656)]])
    f["ln_mod_bwd_fused"] = (LN_BWD_FUSED, ALL, [], [[(fr, P, D) for D in WIDTHS for fr in (1, 5, 80) for P in (1, 16, 17, 144, 160)]])
    return f


def call_args(kind, x):
    """the a0 .. a6 of gtav_op_launch_plan for an input tuple of a family"""
    if kind == LN:
        mode, M, slabs, perm, k_save, k_load, D = x
        return (mode, M, D, slabs, perm, k_save, k_load)
    if kind == ATTN_S:
        pre, nbh, S = x
        return (nbh, 1, S, pre)
    if kind == ATTN_T:
        D, bp, Tq, t0 = x
        return (1, bp, D, Tq, t0, 32)
    if kind == ATTN_S_BWD:
        return (x[0], 1, x[1])
    if kind == SKINNY:
        act, N, K, M = x
        return (M, N, K, act)
    return x


def load(path):
    lib = ctypes.CDLL(path)
    i = ctypes.c_int32
    lib.gtav_op_launch_plan.argtypes = [i] * 8 + [ctypes.POINTER(i)]
    lib.gtav_op_launch_plan.restype = ctypes.c_int
    lib.gtav_last_error.restype = ctypes.c_char_p
    return lib


def plan(lib, kind, x):
    a = tuple(call_args(kind, x))
    out = (ctypes.c_int32 * 12)()
    rc = lib.gtav_op_launch_plan(kind, *(a + (0,) * (7 - len(a))), out)
    return [rc, lib.gtav_last_error().decode()] if rc else list(out)


def build_table(lib):
    table = {}
    for name, (kind, key, rows, groups) in families().items():
        sweep = []
        for group in groups:
            last = None
            for x in group:
                p = plan(lib, kind, x)
                k = [re.sub(r"\d+", "#", str(v)) for v in p] if len(p) == 2 else [p[i] for i in key]   # a refusal: its code and the message without its numbers
                if k != last:
                    last = k
                    sweep.append(list(x) + [p])
        table[name] = {"rows": [list(x) + [plan(lib, kind, x)] for x in rows], "sweep": sweep}
    return table


def dumps(table):
    lines = ["{"]
    for fi, (name, t) in enumerate(table.items()):
        lines.append(f' "{name}": {{')
        for part in ("rows", "sweep"):
            lines.append(f'  "{part}": [')
            lines.extend("   " + json.dumps(r, separators=(",", ":")) + ("," if i + 1 < len(t[part]) else "") for i, r in enumerate(t[part]))
            lines.append("  ]" + ("," if part == "rows" else ""))
        lines.append(" }" + ("," if fi + 1 < len(table) else ""))
    lines.append("}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "ai-generated-gtav_amd", "libgtav_amd.so"))
    ap.add_argument("--write", action="store_true", help=f"write {os.path.relpath(TABLE, ROOT)} instead of printing")
    ap.add_argument("--out", default=TABLE)
    a = ap.parse_args()
    text = dumps(build_table(load(a.lib)))
    if a.write:
        open(a.out, "w").write(text)
        print(f"wrote {a.out}", file=sys.stderr)
    else:
        sys.stdout.write(text)
