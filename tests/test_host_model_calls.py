"""CPU (no GPU): the C-ABI calls DiT and AutoencoderKL make.  The classes' transfer loops, handle settings and handle creation were folded into one path
each (DESIGN.md "The Python classes"); no result can show whether such a refactor dropped or reordered a call, so tests/model_calls_parent.json pins the
calls to what the commit before it made, recorded by tools/model_call_trace.py against a recording stand-in for the library."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ = "gtav_dit_get_operand_dtype"


def _tool():
    spec = importlib.util.spec_from_file_location("model_call_trace", os.path.join(ROOT, "tools", "model_call_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def traces():
    tool = _tool()
    return tool, json.load(open(tool.TABLE)), json.loads(json.dumps(tool.build_table()))


def test_every_case_makes_the_calls_the_parent_commit_made(traces):
    """Symbol by symbol, argument by argument (pointers as a placeholder), in order.  A difference is a dropped, added or moved call: fix the class, or — for a
    call changed on purpose — record the table again with the tool on the commit before and list the case here as ITEM5 is."""
    tool, want, got = traces
    assert list(got) == list(want)
    for case in want:
        if case == tool.ITEM5:
            continue                     # (the test below)
        w, g = want[case], got[case]
        first = next((i for i, (a, b) in enumerate(zip(w, g)) if a != b), min(len(w), len(g)))
        assert g == w, (f"{case}: call {first} of {len(g)} is {g[first] if first < len(g) else 'missing'}, the parent commit made "
                        f"{w[first] if first < len(w) else f'only {len(w)} calls'}")


def test_a_failed_autorange_check_reads_the_group_types_back(traces):
    """The one case that differs on purpose: check() under range_policy="auto" reads the group types from the handle after every gtav_dit_autorange, also
    after one that moved a group and then failed with another error — the parent commit read none then, kept its stale view of the groups and sent the next
    forward to a handle that was no longer finalized.  Apart from the reads, the calls are the parent's with the weight upload repeated before that forward."""
    tool, want, got = traces
    w, g = want[tool.ITEM5], got[tool.ITEM5]
    assert not any(c[0] == READ for c in w)
    at = [i for i, c in enumerate(g) if c[0] == "gtav_dit_autorange"]
    assert len(at) == 2
    for i in at:                                                 # (4 operand groups at depth 1)
        assert [c[:3:2] for c in g[i + 1:i + 5]] == [[READ, grp] for grp in range(4)], g[i + 1:i + 5]
    rest = [c for c in g if c[0] != READ]
    assert len(rest) == len(g) - 8
    lo = next(i for i, c in enumerate(w) if c[0] == "gtav_dit_set_weight")
    hi = next(i for i, c in enumerate(w) if c[0] == "torch.cuda.synchronize")
    upload = w[lo:hi + 1]
    assert upload[-2][0] == "gtav_dit_finalize" and w[-1][0] == "gtav_dit_forward"
    assert rest == w[:-1] + upload + w[-1:]


def test_the_stand_in_leaves_the_process_as_it_found_it():
    import torch

    from gtav_amd import lib as L
    before = (L.load, L.current_stream, torch.cuda.device, torch.cuda.synchronize)
    tool = _tool()
    with tool.stand_in() as sim:
        assert L.load() is sim
    assert (L.load, L.current_stream, torch.cuda.device, torch.cuda.synchronize) == before
