#!/usr/bin/env python3
"""What the GEMM planner (csrc/gemm_plan.hip) selects for every GEMM class the product issues: the table tests/test_host_gemm_plan.py pins.

    python tools/gemm_plan_table.py                    # print the table of the library in the tree
    python tools/gemm_plan_table.py --write            # rewrite tests/gemm_plan_parent.json (a pull request that changes a rule ON PURPOSE does this and shows the diff)
    python tools/gemm_plan_table.py --lib other.so     # any library that exports gtav_op_gemm_plan / gtav_op_gemm_choose_splitk

Needs no GPU: gtav_op_gemm_plan touches no device.  Per class: `rows` = [M, shape, ring depth, splitk, gn, blocks] at the token counts the models run,
`sweep` = the change points [first M, shape, ring depth, splitk, gn] of a dense sweep of M.  For the weight-gradient classes M counts the tokens they
contract over (their K, rounded up to whole 128-token tiles as the training step does)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "gemm_plan_parent.json")

F32, F16, GELU_TANH, GELU_ERF, RESID, QKV, PARTIAL, F16_TILED = range(8)   # csrc/gemm.h GemmEpi
ROWS_M = (144, 288, 320, 720, 1152, 1440, 2880, 4320, 5760, 8640, 11520, 23040, 46080)
SWEEP_M = range(16, 12288 + 1, 16)
P = 144   # DiT tokens per frame (bench.py P_TOK)


def classes(D, vae):
    """name -> (N, K, epilogue, qkv_mode, S, splitk (None: gtav_op_gemm_choose_splitk), rows_per_gate, tokens_are_K).  N or K None = the swept token count."""
    H = 4 * D
    c = {
        # forward / sampler (api_dit.hip dit_blocks, api_internal.h ResidGemm::gemm)
        "to_qkv_spatial": (3 * D, D, QKV, 0, P, 1, 0, False),
        "to_qkv_temporal": (3 * D, D, QKV, 1, P, 1, 0, False),
        "out_proj_partial": (D, D, PARTIAL, 0, 0, None, 0, False),
        "fc2_partial": (D, H, PARTIAL, 0, 0, None, 0, False),
        "out_proj_resid_gate": (D, D, RESID, 0, 0, 1, P, False),
        "fc2_resid_gate": (D, H, RESID, 0, 0, 1, P, False),
        "out_proj_resid": (D, D, RESID, 0, 0, 1, 0, False),
        "fc2_resid": (D, H, RESID, 0, 0, 1, 0, False),
        "fc1_gelu_tanh": (H, D, GELU_TANH, 0, 0, 1, 0, False),
        "fc1_gelu_erf": (H, D, GELU_ERF, 0, 0, 1, 0, False),
        "fc1_f16_tiled": (H, D, F16_TILED, 0, 0, 1, 0, False),
        "patch_embed": (D, 64, F32, 0, 0, 1, 0, False),
        "final_proj": (64, D, F32, 0, 0, 1, 0, False),
        # training step, activation gradients (api_train.hip gemm_dx)
        "dx_final": (D, 64, F32, 0, 0, 1, 0, False),
        "dx_fc2": (H, D, F16_TILED, 0, 0, 1, 0, False),
        "dx_fc1": (D, H, F32, 0, 0, 1, 0, False),
        "dx_out_proj": (D, D, F16, 0, 0, 1, 0, False),
        "dx_to_qkv": (D, 3 * D, F32, 0, 0, 1, 0, False),
        # ... and its ungrouped weight gradients: M = the layer's outputs, N = its inputs, K = the tokens (accumulating EPI_RESID, no gate)
        "dw_to_qkv": (3 * D, D, RESID, 0, 0, 1, 0, True),
        "dw_out_proj": (D, D, RESID, 0, 0, 1, 0, True),
        "dw_fc1": (H, D, RESID, 0, 0, 1, 0, True),
        "dw_fc2": (D, H, RESID, 0, 0, 1, 0, True),
        "dw_final": (64, D, RESID, 0, 0, 1, 0, True),
    }
    if vae:   # api_vae.hip: the four GEMMs around the blocks (the blocks' own are the classes above without a gate) and to_qkv over 576-token images
        c.update({
            "vae_patch": (D, 1216, F32, 0, 0, 1, 0, False),
            "vae_quant": (32, D, F32, 0, 0, 1, 0, False),
            "vae_post_quant": (D, 64, F32, 0, 0, 1, 0, False),
            "vae_pred": (1200, D, F32, 0, 0, 1, 0, False),
            "vae_to_qkv": (3 * D, D, QKV, 0, 576, 1, 0, False),
        })
    return c


def load(path):
    lib = ctypes.CDLL(path)
    i = ctypes.c_int32
    lib.gtav_op_gemm_plan.argtypes = [i] * 8 + [ctypes.POINTER(i)]
    lib.gtav_op_gemm_plan.restype = ctypes.c_int
    lib.gtav_op_gemm_choose_splitk.argtypes = [i, i, i]
    lib.gtav_last_error.restype = ctypes.c_char_p
    return lib


def plan(lib, cls, tokens):
    """[shape, ring depth, splitk, gn, blocks] for `tokens` rows of class `cls`, or None where the class has no such launch (to_qkv on part of a frame)."""
    N, K, epi, mode, S, splitk, rpg, tokens_are_k = cls
    if tokens_are_k:
        M, K = N, (tokens + 127) // 128 * 128
        N = cls[1]
    else:
        M = tokens
    if epi == QKV and M % S:
        return None
    if splitk is None:
        splitk = lib.gtav_op_gemm_choose_splitk(M, N, K)
    out = (ctypes.c_int32 * 8)()
    if lib.gtav_op_gemm_plan(M, N, K, epi, mode, S, splitk, rpg, out):
        raise RuntimeError(f"gtav_op_gemm_plan({M}, {N}, {K}, epilogue {epi}): {lib.gtav_last_error().decode()}")
    return [out[0], out[1], out[2], out[3], out[6]]


def build_table(lib):
    table = {}
    for D in (1024, 256, 512):   # the widths bench.py runs (DiT-S/2, ViT-L/20), then the smoke and test models
        per = {}
        for name, cls in classes(D, vae=D == 1024).items():
            rows = [[m] + r for m in ROWS_M for r in [plan(lib, cls, m)] if r] if D == 1024 else []
            sweep, last = [], None
            for m in SWEEP_M:
                r = plan(lib, cls, m)
                if r and r[:4] != last:
                    last = r[:4]
                    sweep.append([m] + last)
            per[name] = {"rows": rows, "sweep": sweep}
        table[f"hidden_{D}"] = per
    return table


def dumps(table):
    lines = ["{"]
    for hi, (hk, per) in enumerate(table.items()):
        lines.append(f' "{hk}": {{')
        for ci, (name, t) in enumerate(per.items()):
            lines.append(f'  "{name}": {{')
            lines.append('   "rows": [' + ", ".join(json.dumps(r, separators=(",", ":")) for r in t["rows"]) + "],")
            lines.append('   "sweep": [' + ", ".join(json.dumps(r, separators=(",", ":")) for r in t["sweep"]) + "]")
            lines.append("  }" + ("," if ci + 1 < len(per) else ""))
        lines.append(" }" + ("," if hi + 1 < len(table) else ""))
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
