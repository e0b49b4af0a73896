"""CPU (no GPU): the GEMM planner (csrc/gemm_plan.hip, gtav_op_gemm_plan).  Every block shape computes the same result, so no parity test can see which
one a launch picks: (a) pins the selection to what the commit before the planner existed selected, recorded from that commit's own launch_gemm;
(b) checks the shape table against the documented hooks; both through the function launch_gemm itself calls."""
import ctypes
import importlib.util
import json
import os
import re
import threading

import pytest

from gtav_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_SHAPES = {2, 3, 7, 11, 12, 13, 14, 20, 24, 26, 29, 31}


def _tool():
    spec = importlib.util.spec_from_file_location("gemm_plan_table", os.path.join(ROOT, "tools", "gemm_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _plan(lib, M, N, K, epi=0, mode=0, S=0, splitk=1, rpg=0):
    out = (ctypes.c_int32 * 8)()
    rc = lib.gtav_op_gemm_plan(M, N, K, epi, mode, S, splitk, rpg, out)
    return rc, list(out)


@pytest.fixture
def lib():
    lib = L.load()
    lib.gtav_op_gemm_set_wm(0)
    lib.gtav_op_gemm_set_stages(0)
    yield lib
    lib.gtav_op_gemm_set_wm(0)
    lib.gtav_op_gemm_set_stages(0)


def test_selection_equals_the_recorded_parent_table(lib):
    """tests/gemm_plan_parent.json: shape, ring depth, splitk, gn and blocks of every GEMM class the product issues (tools/gemm_plan_table.py lists them), at the
    token counts the models run and as the change points of a dense sweep of M, for hidden sizes 1024, 256 and 512.  A difference is a moved rule: fix the
    planner, or — for a rule changed on purpose — regenerate the table with the tool and show its diff."""
    tool = _tool()
    want = json.load(open(tool.TABLE))
    got = tool.build_table(tool.load(L.LIB_PATH))
    assert list(got) == list(want) == ["hidden_1024", "hidden_256", "hidden_512"]
    n_rows = 0
    for hidden, per in want.items():
        assert list(got[hidden]) == list(per), hidden
        for name, t in per.items():
            g = got[hidden][name]
            for w, r in zip(t["rows"], g["rows"]):
                assert r == w, f"{hidden} {name} at M = {w[0]}: [M, shape, ring depth, splitk, gn, blocks] = {r}, the parent commit ran {w}"
            for w, r in zip(t["sweep"], g["sweep"]):
                assert r == w, f"{hidden} {name}: a boundary moved: [first M, shape, ring depth, splitk, gn] = {r}, the parent commit had {w}"
            assert len(g["rows"]) == len(t["rows"]) and len(g["sweep"]) == len(t["sweep"]), (hidden, name)
            n_rows += len(t["rows"]) + len(t["sweep"])
    assert len(want["hidden_1024"]) >= 28 and n_rows > 700   # the table is the whole one, not a stub


def _documented_shapes():
    """The block-shape list of include/gtav_amd_testing.h: ` *   <id>   <features> x <tokens>   <compute>[ + <loader>] waves`."""
    hdr = open(os.path.join(ROOT, "include", "gtav_amd_testing.h")).read()
    rows = re.findall(r"^ \*\s+(\d+)\s+(\d+) x (\d+)\s+(\d+)(?: \+ (\d+))? waves", hdr, flags=re.M)
    return {int(i): (int(t), int(f), 64 * (int(c) + int(l or 0))) for i, f, t, c, l in rows}


def test_shape_table_matches_the_documented_hooks(lib):
    doc = _documented_shapes()
    assert set(doc) == PRODUCT_SHAPES
    accepted = set()
    for shape in range(1, 64):
        lib.gtav_op_gemm_set_wm(shape)
        rc, p = _plan(lib, 720, 1024, 1024)
        if rc == 0:
            accepted.add(shape)
            assert p[0] == shape and (p[4], p[5], p[7]) == doc[shape], (shape, p)
            assert p[6] == -(-720 // p[4]) * -(-1024 // p[5])
            for epi in range(8):   # a forced shape comes back unchanged for every epilogue (whether that pair has a kernel is the launch's business)
                rc, q = _plan(lib, 5760, 3072, 1024, epi=epi, mode=0, S=144, splitk=2, rpg=144)
                assert rc == 0 and q[0] == shape, (shape, epi, q)
        else:
            assert str(shape).encode() in lib.gtav_last_error() and b"block shape" in lib.gtav_last_error(), (shape, lib.gtav_last_error())
    assert accepted == PRODUCT_SHAPES
    lib.gtav_op_gemm_set_wm(12)
    lib.gtav_op_gemm_set_stages(4)
    assert _plan(lib, 720, 1024, 1024)[1][:2] == [12, 4]
    lib.gtav_op_gemm_set_stages(0)
    lib.gtav_op_gemm_set_wm(0)
    assert _plan(lib, 720, 1024, 1024, epi=6, splitk=2)[1][:4] == [26, 4, 2, 8]   # the heuristic again (the table's out_proj_partial row at M = 720)
    assert lib.gtav_op_gemm_plan(720, 1024, 1024, 0, 0, 0, 1, 0, None) != 0


def test_forced_shape_is_per_thread(lib):
    heuristic = _plan(lib, 720, 1024, 1024)[1][:2]
    assert heuristic[0] not in (2, 7)
    lib.gtav_op_gemm_set_wm(7)
    lib.gtav_op_gemm_set_stages(2)
    seen = {}

    def other():
        seen["before"] = _plan(lib, 720, 1024, 1024)[1][:2]
        lib.gtav_op_gemm_set_wm(2)
        seen["after"] = _plan(lib, 720, 1024, 1024)[1][:2]

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == {"before": heuristic, "after": [2, 2]}        # the other thread saw the heuristic, then its own override
    assert _plan(lib, 720, 1024, 1024)[1][:2] == [7, 2]        # ... which this thread never saw
