"""CPU (no GPU): every product kernel instantiation of the non-GEMM launchers is run by an op-level parity test.  tests/test_host_launch_plan.py pins WHICH
instantiation a problem selects; because every instantiation computes the same result, no parity test can see which one it ran — so this file proves, through
the function the launchers themselves call (gtav_op_launch_plan), that the problems of the parity tests (tests/parity_bounds.py op_rows: the case tables, each
row with its declared plan) select what they are declared to, and that the declared plans together are the whole product list of csrc/launch_plan.h but for the
exceptions written out below.  The GPU tests assert the same declared plan before they launch (helpers.assert_declared_plan)."""
import parity_bounds as PB
from gtav_amd import lib as L
from test_host_launch_plan import FAMILY_LIST, _instantiation_lists, _tool

LF_ATTN_FLASH = 3
# product instantiations no op-level parity test runs, each with its reason.  Anything else that is uncovered gets a case, not a line here.
EXCEPTIONS = {
    "attn_spatial": {(LF_ATTN_FLASH, 3, 2, r, p): "attn_flash_kernel<3, 2, *, *>: three query tiles per wave at two blocks per CU is chosen by the laboratory knob attn_flash_occ3 "
                                                 "alone (csrc/launch_plan.hip); the product planner cannot select it" for r in (0, 1) for p in (0, 1)},
}


def test_every_row_selects_its_declared_plan():
    lib = _tool().load(L.LIB_PATH)
    rows = PB.op_rows()
    assert {(f, a) for f, a, _, _ in rows} == set(PB.DECLARED_PLANS), "a declared plan without a problem in the case tables: " + \
        str(sorted(set(PB.DECLARED_PLANS) - {(f, a) for f, a, _, _ in rows}))
    assert {f for f, _, _, _ in rows} == set(FAMILY_LIST) == set(PB.OP_KIND)
    for family, args, declared, table in rows:
        got = PB.query_plan(lib, family, args)
        assert got == declared, f"{family} {args} ({table}): the library plans {got}, the table declares {declared}"


def test_declared_plans_are_the_product_lists():
    """per family: declared instantiations == product list - exceptions; an exception is a product instantiation that no row declares"""
    lists = _instantiation_lists()
    declared = {f: set() for f in FAMILY_LIST}
    for family, args, (inst, form), table in PB.op_rows():
        declared[family].add(inst)
    for family, lst in FAMILY_LIST.items():
        exc = set(EXCEPTIONS.get(family, {}))
        assert exc <= lists[lst], f"{family}: an exception that is no product instantiation: {sorted(exc - lists[lst])}"
        assert not (exc & declared[family]), f"{family}: an exception that a case covers: {sorted(exc & declared[family])}"
        assert declared[family] <= lists[lst], f"{family}: declared but not in {lst}: {sorted(declared[family] - lists[lst])}"
        missing = lists[lst] - declared[family] - exc
        assert not missing, f"{family}: no op-level parity case runs the instantiation(s) {sorted(missing)} of {lst}"
    assert set(EXCEPTIONS) <= set(FAMILY_LIST) and all(reason for e in EXCEPTIONS.values() for reason in e.values())


def test_every_launch_form_occurs_on_every_instantiation_that_can_take_it():
    """(instantiation, form) over the dense planner sweep of tools/launch_plan_table.py — every pair a launch can be — against the declared ones: the one-pass
    spatial kernel with and without a query split, the register-resident temporal kernel on one query frame, split over query frames and looping over them"""
    tool = _tool()
    lib = tool.load(L.LIB_PATH)
    for family in ("attn_spatial", "attn_temporal"):
        kind, _, rows, groups = tool.families()[family]
        possible = set()
        for x in rows + [x for group in groups for x in group]:
            args = tuple(tool.call_args(kind, x))
            p = tool.plan(lib, kind, x)
            if len(p) != 2 and PB.plan_form(family, args, p) is not None:
                possible.add((tuple(p[:5]), PB.plan_form(family, args, p)))
        declared = {d for f, a, d, t in PB.op_rows() if f == family and d[1] is not None}
        assert len(possible) >= 6
        assert possible - declared == set(), f"{family}: no op-level parity case runs (instantiation, launch form) {sorted(possible - declared)}"
        assert declared - possible == set(), f"{family}: declared but never planned over the sweep: {sorted(declared - possible)}"
