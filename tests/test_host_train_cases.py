"""CPU: tests/train_cases.py builds the tensors the training tests have always seen.  tests/train_case_digests.json holds the SHA-256 of the raw bytes of every
tensor the per-file builders returned before they were merged into that module (recorded from those builders, after checking that the copies agreed with one
another); a builder that draws in another order, or from another seed, changes every margin `pytest -s` prints and fails here first."""
import hashlib
import json
import os

import train_cases as TC

LONG_FRAME = dict(TC.TOY_KW, input_h=20, input_w=40)
GEO = {"p2c4": dict(TC.TOY_KW, in_channels=4), "p4c16": dict(TC.TOY_KW, input_h=16, input_w=32, patch_size=4)}       # tests/test_gpu_geometry_train.py GEO
INPUTS, CLIP = ("x", "t", "a", "vt"), ("lat", "a", "tgt", "ctx", "cn", "nz")

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_case_digests.json")) as _f:
    DIGESTS = json.load(_f)


def _digests(names, tensors):
    assert len(names) == len(tensors)
    return {n: None if t is None else hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest() for n, t in zip(names, tensors)}


def _cases():
    for B, T in ((2, 3), (1, 5), (2, 9)):
        for actions in (True, False):
            yield f"inputs toy B={B} T={T} actions={actions}", _digests(INPUTS, TC.inputs(TC.TOY_KW, B, T, actions))
    yield "inputs 20x40 B=2 T=3 actions=True", _digests(INPUTS, TC.inputs(LONG_FRAME))
    for geo, kw in GEO.items():
        yield f"inputs {geo} B=2 T=3 actions=True", _digests(INPUTS, TC.inputs(kw))
    yield "clip toy B=2 F=5", _digests(CLIP, TC.clip(TC.TOY_KW))
    yield "clip 24x48 B=2 F=5", _digests(CLIP, TC.clip(dict(TC.TOY_KW, input_h=24, input_w=48)))
    yield "clip p4c16 B=2 F=3", _digests(CLIP, TC.clip(GEO["p4c16"], F=3))
    yield "clip toy B=2 F=12", _digests(CLIP, TC.clip(TC.TOY_KW, F=12))
    yield "clip toy B=2 F=6 (lat, a)", _digests(CLIP[:2], TC.clip(TC.TOY_KW, F=6)[:2])
    sd = TC.state_dict(TC.TOY_KW, 1)
    yield "state_dict toy seed=1", _digests(*zip(*((k, sd[k]) for k in DIGESTS["state_dict toy seed=1"])))


def test_builders_reproduce_the_recorded_digests():
    got = dict(_cases())
    assert got.keys() == DIGESTS.keys()
    for name in DIGESTS:
        assert got[name] == DIGESTS[name], name


def test_state_dict_and_oracle_are_computed_once():
    assert TC.state_dict(TC.TOY_KW, 1) is TC.state_dict(dict(TC.TOY_KW), 1)
    assert TC.state_dict(TC.TOY_KW, 3) is not TC.state_dict(TC.TOY_KW, 1)
    first, again = TC.oracle(TC.TOY_KW, 1, 1, True), TC.oracle(dict(TC.TOY_KW), 1, 1, True)
    assert all(a is b for a, b in zip(first, again))
    sd, inp, loss_ref, v_ref, grads = first
    assert sd is TC.state_dict(TC.TOY_KW, 1) and v_ref.shape == inp[0].shape and float(loss_ref) > 0
    assert set(grads) == {k for k in sd if not k.endswith("freqs")}
    assert TC.oracle(TC.TOY_KW, 1, 1, False) is not first
