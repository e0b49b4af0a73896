"""CPU (no GPU): the launch planner of the non-GEMM kernels (csrc/launch_plan.hip, gtav_op_launch_plan).  Every instantiation a launcher can pick computes the
same result, so no parity test can see which one a launch runs: (a) pins kernel, grid, block and LDS to what the commit before the planner existed launched,
recorded from that commit's own launchers; (b) checks every plan against the instantiation lists of csrc/launch_plan.h, the lists the launchers dispatch over;
both through the function the launchers themselves call.  That every product instantiation is also RUN by an op-level parity test is the business of
tests/test_host_op_coverage.py, which reuses _instantiation_lists() below."""
import importlib.util
import json
import os
import re

from gtav_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-generated-gtav_amd", "csrc")
FAMILY_LIST = {"layernorm": "LN_KERNELS", "attn_spatial": "ATTN_SPATIAL_KERNELS", "attn_temporal": "ATTN_TEMPORAL_KERNELS", "attn_spatial_bwd": "ATTN_SPATIAL_BWD_KERNELS",
               "attn_temporal_bwd": "ATTN_TEMPORAL_BWD_KERNELS", "skinny": "SKINNY_KERNELS", "gemm_tn_f32": "GEMM_TN_F32_KERNELS", "gemm_nn_f32": "GEMM_NN_F32_KERNELS",
               "ada_bwd_dx": "ADA_BWD_DX_KERNELS", "ln_mod_bwd_fused": "LN_BWD_FUSED_KERNELS"}


def _tool():
    spec = importlib.util.spec_from_file_location("launch_plan_table", os.path.join(ROOT, "tools", "launch_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _instantiation_lists():
    """csrc/launch_plan.h: list name -> {(family number, a, b, c, d)} of the instantiations the product library holds."""
    hdr = open(os.path.join(CSRC, "launch_plan.h")).read()
    enum = re.search(r"enum LaunchFamily : int \{(.*?)\};", hdr, flags=re.S).group(1)
    number = {n: i for i, n in enumerate(re.findall(r"^\s*(LF_\w+),", enum, flags=re.M))}
    lists = {}
    for name, body in re.findall(r"constexpr KernelInst (\w+)\[\] = \{(.*?)\n?\};", hdr, flags=re.S):
        rows = re.findall(r"\{(LF_\w+), (\d+), (\d+), (\d+), (\d+), (true|false)\}", body)
        assert rows and len(rows) == body.count("{LF_"), name
        lists[name] = {(number[f], int(a), int(b), int(c), int(d)) for f, a, b, c, d, product in rows if product == "true"}
    return lists


def test_selection_equals_the_recorded_parent_table():
    """tests/launch_plan_parent.json: kernel instantiation, grid, block, LDS bytes and the family's own numbers (query split, K chunks, the second launch of a
    pair) of every launcher that picks between instantiations (tools/launch_plan_table.py lists the sweeps), refusals included.  A difference is a moved rule:
    fix the planner, or — for a rule changed on purpose — regenerate the table with the tool and show its diff."""
    tool = _tool()
    want = json.load(open(tool.TABLE))
    got = tool.build_table(tool.load(L.LIB_PATH))
    assert list(got) == list(want) == list(FAMILY_LIST)
    n_rows = 0
    for name, t in want.items():
        g = got[name]
        for w, r in zip(t["rows"], g["rows"]):
            assert r == w, f"{name}: [inputs ..., plan] = {r}, the parent commit ran {w}"
        for w, r in zip(t["sweep"], g["sweep"]):
            assert r == w, f"{name}: a boundary moved: [inputs ..., plan] = {r}, the parent commit had {w}"
        assert len(g["rows"]) == len(t["rows"]) and len(g["sweep"]) == len(t["sweep"]), name
        n_rows += len(t["rows"]) + len(t["sweep"])
    # the table is the whole one, not a stub: every family, its refusals, and the sweeps at their recorded density
    assert n_rows > 3200 and len(want["layernorm"]["sweep"]) > 700 and len(want["attn_spatial"]["sweep"]) > 300 and len(want["attn_temporal"]["sweep"]) > 300
    assert len(want["skinny"]["rows"]) == 500 and len(want["attn_spatial_bwd"]["sweep"]) > 50 and len(want["attn_temporal_bwd"]["sweep"]) >= 18
    refused = {name: [r[-1][1] for r in t["rows"] + t["sweep"] if len(r[-1]) == 2] for name, t in want.items()}
    assert any("S=15368 needs" in m for m in refused["attn_spatial_bwd"]) and any("K=2560" in m for m in refused["skinny"])
    assert any("takes plain q" in m for m in refused["attn_spatial"]) and any("bad output row permutation" in m for m in refused["layernorm"])


def test_every_plan_names_a_member_of_its_instantiation_list():
    """The kernel a plan names — over the whole sweep, not only its change points — is one the product library instantiates: a member of the family's list in
    csrc/launch_plan.h.  And each launcher dispatches over exactly that list, so a plan is never launched as nothing."""
    tool = _tool()
    lib = tool.load(L.LIB_PATH)
    lists = _instantiation_lists()
    assert set(lists) == set(FAMILY_LIST.values())
    used = {name: set() for name in FAMILY_LIST}
    for name, (kind, key, rows, groups) in tool.families().items():
        for x in rows + [x for group in groups for x in group]:
            p = tool.plan(lib, kind, x)
            if len(p) == 2:
                assert p[0] == 2 and "no kernel instantiation" not in p[1], (name, x, p)   # a refusal is the launcher's own, never the planner finding no kernel
                continue
            assert tuple(p[:5]) in lists[FAMILY_LIST[name]], f"{name} {x}: the plan names {p[:5]}, which is not in {FAMILY_LIST[name]}"
            assert p[5] >= 1 and p[6] >= 1 and p[7] >= 64 and p[7] % 64 == 0 and 0 <= p[8] <= 160 * 1024, (name, x, p)
            used[name].add(tuple(p[:5]))
    for name, seen in used.items():   # the sweep reaches every product instantiation but the flash kernel's unselected occupancy variant
        missing = lists[FAMILY_LIST[name]] - seen
        assert all(m[0] == 3 and m[1:3] == (3, 2) for m in missing), (name, sorted(missing))
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("attention.hip", "elementwise.hip", "skinny.hip", "train.hip"))
    for lst in lists:
        assert len(re.findall(rf"dispatch_kernel<kernel_count\({lst}\)>", text)) == 1, f"{lst}: one launcher dispatches over it"
    assert not re.search(r"hipFuncSetAttribute|hipFuncAttributeMaxDynamicSharedMemorySize", text), "one LDS opt-in: common.h lds_opt_in"


def test_launch_plan_refuses_bad_arguments():
    lib = L.load()
    assert lib.gtav_op_launch_plan(0, 0, 720, 1024, 0, 0, 0, 0, None) != 0
    assert lib.gtav_op_launch_plan(10, 0, 0, 0, 0, 0, 0, 0, None) != 0 and b"op_launch_plan" in lib.gtav_last_error()
