"""CPU (no GPU): the host side of mixed fp16 / bf16 operand groups in training — the data-parallel merge of the per-group saturation words over gloo, the
step.json fields that carry the groups through a checkpoint, and the constructor's refusals."""
import json
import socket

import pytest
import torch

F16, BF16 = torch.float16, torch.bfloat16
SAT, NONFINITE = 2, 4                       # csrc/common.h ERR_F16_SAT, ERR_NONFINITE
STUB_WORDS = ([0, SAT, 0, 0, SAT | NONFINITE, 0], [0, 0, 0, SAT, SAT, 0])     # what two ranks read from their handles


def _merge_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gtav_amd.train import autorange_step, merge_range_words

    class FakeDit:          # autorange_step touches train_range_words() (this rank's sticky words) and train_autorange(merged words) -> switched groups
        applied = None

        def train_range_words(self):
            return list(STUB_WORDS[rank])

        def train_autorange(self, merged):
            self.applied = list(merged)
            return [g for g, w in enumerate(merged) if w & SAT]
    merged, groups = merge_range_words(STUB_WORDS[rank], world)           # default collective: torch.distributed MAX
    d = FakeDit()
    switched = autorange_step(d, world)
    q.put((rank, merged, groups, switched, d.applied))
    dist.destroy_process_group()


def test_rank_merge_gives_every_rank_the_union_gloo():
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_merge_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    outs = {o[0]: o[1:] for o in (q.get(timeout=120) for _ in range(2))}
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    union = [1, 3, 4]
    for rank in (0, 1):
        merged, groups, switched, applied = outs[rank]
        assert groups == union and switched == union, (rank, groups, switched)
        assert applied == merged
        assert [bool(w & SAT) for w in merged] == [g in union for g in range(6)]
    # bits that are not a range decision stay with the rank that raised them: reported there, not spread
    assert outs[0][0][4] == SAT | NONFINITE and outs[1][0][4] == SAT


def test_merge_is_the_identity_on_one_rank_and_takes_an_injected_collective():
    from gtav_amd.train import merge_range_words
    merged, groups = merge_range_words(STUB_WORDS[0])
    assert merged == STUB_WORDS[0] and groups == [1, 4]
    seen = []

    def fake_all_reduce(t):                 # "the other rank saturated group 3"
        assert t.dtype == torch.int32 and t.tolist() == [0, 1, 0, 0, 1, 0]
        seen.append(1)
        t[3] = 1
    merged, groups = merge_range_words(STUB_WORDS[0], 2, fake_all_reduce)
    assert seen and groups == [1, 3, 4] and merged == [0, SAT, 0, SAT, SAT | NONFINITE, 0]


class _FakeModel:
    """What save_state / load_state touch besides the tensors."""
    n_operand_groups = 6
    loss_scale = 1.0
    train_dtype = F16

    def __init__(self, policy, bf16=()):
        self.train_range_policy, self.bf16, self.restored = policy, set(bf16), None

    def operand_dtypes(self):
        return [BF16 if g in self.bf16 else F16 for g in range(self.n_operand_groups)]

    def restore_operand_groups(self, groups):
        if self.train_range_policy != "auto":
            raise RuntimeError("train_range_policy='auto'")
        self.restored = list(groups)


def test_step_json_carries_the_bf16_groups():
    from gtav_amd.train import _restore_groups, _step_state
    state = json.loads(json.dumps(_step_state(_FakeModel("auto", {0, 3}), 7, 1)))
    assert state == {"step": 7, "epoch": 1, "loss_scale": 1.0, "operand_dtype": "fp16", "bf16_groups": [0, 3]}
    m = _FakeModel("auto")
    _restore_groups(m, state)
    assert m.restored == [0, 3]
    with pytest.raises(RuntimeError, match="train_range_policy='auto'"):      # a mixed checkpoint needs the opt-in
        _restore_groups(_FakeModel("report"), state)
    # one type for every group (what every earlier checkpoint is, with or without the field): a model without the opt-in loads it as before
    for groups in ([], list(range(6))):
        m = _FakeModel("report")
        _restore_groups(m, dict(state, bf16_groups=groups))
        assert m.restored is None
    m = _FakeModel("report")
    _restore_groups(m, {"step": 1})
    assert m.restored is None
    m = _FakeModel("auto", {1})               # an opted-in model takes the checkpoint's groups whatever they are
    _restore_groups(m, dict(state, bf16_groups=[]))
    assert m.restored == []


def test_constructor_and_host_side_refusals():
    from gtav_amd.lib import GtavError
    from gtav_amd.model.dit import DiT
    kw = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25, init_weights=False)
    with pytest.raises(ValueError, match="trainable=True"):
        DiT(**kw, train_range_policy="auto")
    with pytest.raises(ValueError, match="train_range_policy"):
        DiT(**kw, trainable=True, train_range_policy="always")
    m = DiT(**kw, trainable=True)
    assert m.train_range_policy == "report" and all(d == F16 for d in m.operand_dtypes())
    with pytest.raises(GtavError, match="train_range_policy='auto'"):
        m.train_autorange()
    with pytest.raises(GtavError, match="train_range_policy='auto'"):
        m.restore_operand_groups([0])
    m.restore_operand_groups([])              # the groups it has anyway
    a = DiT(**kw, trainable=True, train_range_policy="auto", train_dtype=BF16)
    assert all(d == BF16 for d in a.operand_dtypes()) and a.loss_scale == 1.0
    a.restore_operand_groups([0, 5])          # no handle yet: kept for the handle the first step builds
    assert [g for g, d in enumerate(a.operand_dtypes()) if d == BF16] == [0, 5]
    with pytest.raises(ValueError, match="outside"):
        a.restore_operand_groups([6])


def test_mixed_type_entry_points_refuse_a_null_handle():
    import ctypes as C
    from gtav_amd import lib as L
    lib = L.load()
    n = C.c_int32(0)
    for rc in (lib.gtav_dit_train_allow_mixed(None, 1), lib.gtav_dit_train_set_group_dtype(None, 0, 1, None), lib.gtav_dit_train_range_words(None, None, None),
               lib.gtav_dit_train_autorange(None, None, C.byref(n), None)):
        assert rc != 0 and b"null handle" in lib.gtav_last_error()
