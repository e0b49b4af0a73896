#!/usr/bin/env python3
"""The C-ABI calls the Python classes (gtav_amd.model.dit.DiT, gtav_amd.model.vae.AutoencoderKL) make, case by case: the table tests/test_host_model_calls.py pins.

    python tools/model_call_trace.py                   # print the traces of the classes in the tree
    python tools/model_call_trace.py --write           # rewrite tests/model_calls_parent.json (run on the commit a refactor starts from)
    python tools/model_call_trace.py --time            # five timings of 1e5 _ensure(1, 2) calls on a built, clean model (the path of every forward)

Needs neither a GPU nor the built library: gtav_amd.lib.load returns a stand-in whose every symbol records [symbol, arguments...] and returns 0.  Pointers are
recorded as "<ptr>" (which arguments are pointers: gtav_amd.lib.SIGNATURES), names, element counts, integers and floats exactly, the config of a *_create
as a dict; torch.cuda.synchronize is recorded as a call of that name.  The stand-in fills the out-parameters the classes read: the handle, the trainable
parameter count, the operand type of a group (tracked from the set calls it saw), the optimizer step counts and the count of an autorange, whose outcome a
case scripts.  The cases use public methods only, so the tool runs unchanged on an older commit."""
import argparse
import contextlib
import ctypes
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "model_calls_parent.json")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gtav_amd  # noqa: E402,F401
from gtav_amd import lib as L  # noqa: E402

SIGNATURES = dict(L.SIGNATURES, **L.EXP_SIGNATURES)
INTS = (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64)


class StandIn:
    """What gtav_amd.lib.load() returns while a case runs."""

    _gtav_experiments = True      # (DiT.set_fold asks)

    def __init__(self):
        self.calls = []
        self.bf16 = set()         # operand groups on bf16, from the set calls
        self.autorange = []       # scripted outcomes of the next gtav_dit_autorange / gtav_dit_train_autorange calls: (groups that move to bf16, return code)

    def __getattr__(self, name):
        if name == "gtav_last_error":
            return lambda: b"stand-in: scripted error"
        if name not in SIGNATURES:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        sig = SIGNATURES[name]
        assert len(args) == len(sig), (name, len(args), len(sig))
        self.calls.append([name] + [self._render(name, a, t) for a, t in zip(args, sig)])
        out = lambda i: args[i]._obj          # the object behind a ctypes.byref
        rc = 0
        if name.endswith("_create"):
            out(1).value = 0x1000
            self.bf16 = set()
        elif name == "gtav_dit_train_param_count":
            out(1).value = 1000
        elif name == "gtav_dit_train_saved_bytes":
            out(1).value = 4096
        elif name in ("gtav_dit_set_operand_dtype", "gtav_dit_train_set_group_dtype"):
            (self.bf16.add if args[2] else self.bf16.discard)(args[1])
        elif name == "gtav_dit_train_enable_typed" and args[3] == 1:
            self.bf16 = set(range(64))
        elif name == "gtav_dit_get_operand_dtype":
            out(2).value = int(args[1] in self.bf16)
        elif name == "gtav_dit_get_opt_step":
            out(1).value, out(2).value = 3, 1
        elif name in ("gtav_dit_autorange", "gtav_dit_train_autorange"):
            groups, rc = self.autorange.pop(0) if self.autorange else ((), 0)
            self.bf16 |= set(groups)
            out(1 if name == "gtav_dit_autorange" else 2).value = len(groups)
        return rc

    @staticmethod
    def _render(name, a, t):
        if t is ctypes.c_char_p:
            return a.decode()
        if t in INTS:
            return int(a)
        if t is ctypes.c_float:
            return float(a)
        if name.endswith("_create") and hasattr(a, "_obj") and isinstance(a._obj, ctypes.Structure):
            return {f: getattr(a._obj, f) for f, _ in a._obj._fields_}
        return "<ptr>"


@contextlib.contextmanager
def stand_in():
    """Patches the library loader, the stream lookup and torch.cuda's device context and synchronisation for the block, and yields the StandIn."""
    sim = StandIn()
    saved = (L.load, L.current_stream, torch.cuda.device, torch.cuda.synchronize)
    L.load, L.current_stream = (lambda: sim), (lambda: 0)
    torch.cuda.device = lambda device: contextlib.nullcontext()
    torch.cuda.synchronize = lambda *a: sim.calls.append(["torch.cuda.synchronize"])
    try:
        yield sim
    finally:
        gc.collect()              # the models of the block destroy their handles while the stand-in is still the library
        L.load, L.current_stream, torch.cuda.device, torch.cuda.synchronize = saved


# ------------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------------
CPU = torch.device("cpu")
ITEM5 = "inference_autorange_check"      # the one case a refactor of check() is allowed to change (tests/test_host_model_calls.py)
ALIVE = []                               # the models of the running case: none destroys its handle before the case's calls are taken


def dit(**kw):
    from gtav_amd.model.dit import DiT
    torch.manual_seed(0)
    m = DiT(input_h=4, input_w=4, patch_size=2, hidden_size=128, depth=1, num_heads=2, external_cond_dim=3, **kw)
    m.device = CPU
    ALIVE.append(m)
    return m


def vae(**kw):
    from gtav_amd.model.vae import AutoencoderKL
    torch.manual_seed(0)
    m = AutoencoderKL(4, input_height=8, input_width=8, patch_size=4, enc_dim=64, enc_depth=1, enc_heads=2, dec_dim=64, dec_depth=1, dec_heads=2, **kw)
    m.device = CPU
    ALIVE.append(m)
    return m


def batch(B, T):
    return torch.zeros(B, T, 16, 4, 4), torch.zeros(B, T, dtype=torch.int64), torch.zeros(B, T, 3)


def schedule():
    return torch.linspace(0.999, 0.001, 1000)


def every_setter(m):
    m.set_fused_temporal(True)
    m.set_fused_spatial(False)
    m.set_fold(1, 10, 20)
    m.set_weight_prefetch(0x10003)
    m.set_weight_fill_policy(0x0101)
    m.set_guidance(2.5)
    m.loss_scale = 1024.0
    m.grad_divisor = 2.0
    m.set_schedule(schedule())


def train_step(m, B=1, T=2):
    x, t, c = batch(B, T)
    m.zero_grad()
    v = m.forward_train(x, t, c)
    m.backward_(v, torch.zeros_like(v[:, -1]))
    m.adamw_step(1e-4, weight_decay=0.01, max_grad_norm=1.0)
    m.train_stats()


def case_inference_defaults(sim):
    m = dit()
    m(*batch(1, 2))
    m(*batch(1, 2))
    m.check()


def case_setters_before_first_use(sim):
    m = dit(max_batch=2)
    every_setter(m)
    m(*batch(1, 2))
    m.prepare_frame_(1, 3, 0, 2, 0, [999, 500, 0])
    off = dit()
    off.set_fused_temporal(False)          # the library's default: recorded, nothing to replay
    off.set_guidance(None)
    off(*batch(1, 2))


def case_setters_after_the_handle_exists(sim):
    m = dit(max_batch=2)
    m(*batch(1, 2))
    every_setter(m)
    m.set_fused_temporal(False)
    m.set_fused_spatial(True)
    m.set_weight_prefetch(False)
    m.set_weight_fill_policy(0)
    m.set_guidance(None)
    m(*batch(1, 2))


def case_growth_through_reserve(sim):
    m = dit(max_batch=2)
    every_setter(m)
    m(*batch(1, 2))
    m.reserve(4, 5, noise_steps=10)        # destroy, create, replay, upload, schedule
    m(*batch(4, 5))
    m.max_frames = 8                       # (the window setter drops the handle)
    m(*batch(1, 8))


def case_operand_dtype_on_a_subset_of_groups(sim):
    m = dit()
    m.set_operand_dtype(torch.bfloat16, [1, 3])
    m(*batch(1, 2))
    m.set_operand_dtype(torch.float16, [1])
    m(*batch(1, 2))
    m.reserve(2)
    m(*batch(2, 2))
    assert m.operand_dtypes() == [torch.float16] * 3 + [torch.bfloat16]


def case_trainable_fp16(sim):
    m = dit(trainable=True)
    train_step(m)
    m.param_range("blocks.")
    m.loss_scale = 4096.0
    m.grad_divisor = 8.0
    train_step(m)
    m(*batch(1, 2))


def case_trainable_bf16(sim):
    m = dit(trainable=True, train_dtype=torch.bfloat16)
    m.grad_divisor = 4.0
    train_step(m)
    m.set_operand_dtype(torch.bfloat16)    # a no-op on a bf16-trainable model


def case_train_max_frames_12(sim):
    m = dit(trainable=True, max_frames=12, train_max_frames=12)
    train_step(m, 1, 10)


def case_train_recompute(sim):
    m = dit(trainable=True, train_recompute=True)
    m.train_saved_bytes()
    train_step(m)


def case_train_range_policy_auto(sim):
    m = dit(trainable=True, train_range_policy="auto")
    m.restore_operand_groups([1])          # before the handle exists: applied to the handle when it is built
    train_step(m)
    m.restore_operand_groups([0, 2])       # after: in place
    m.train_range_words()
    sim.autorange.append(([3], 0))
    assert m.train_autorange() == [3]
    m.train_set_group_dtype(torch.float16, [3])
    train_step(m)
    b = dit(trainable=True, train_dtype=torch.bfloat16, train_range_policy="auto")
    b.restore_operand_groups([0, 1, 2])
    train_step(b)


def case_lora_rank_16_with_ema(sim):
    m = dit(trainable=True, train_lora_rank=16, train_ema_decay=0.999, train_ema_warmup=True)
    train_step(m)
    m.load_state_dict(m.state_dict())      # pull adapters, pull average, upload, push average
    m(*batch(1, 2))
    with m.ema_weights():
        m(*batch(1, 2))
    m.load_opt_state_dict(m.opt_state_dict())
    m.pull_weights()
    m.grad("blocks.0.s_attn.to_qkv.lora_A.weight")
    m.merged_state_dict()
    m.load_ema_state_dict(m.ema_state_dict())
    train_step(m)
    m.load_lora_state_dict(m.lora_state_dict())
    m.init_lora(seed=1)


def case_full_training_with_ema(sim):
    m = dit(trainable=True, train_ema_decay=0.99)
    train_step(m)
    m.load_opt_state_dict(m.opt_state_dict())
    m.pull_weights()
    m.grad("final_layer.linear.weight")
    m.load_ema_state_dict(m.ema_state_dict())
    with m.ema_weights():
        m(*batch(1, 2))
    m.load_state_dict(m.state_dict())
    m(*batch(1, 2))
    fresh = dit(trainable=True)            # a checkpoint onto a model whose handle does not exist yet
    fresh.load_opt_state_dict(m.opt_state_dict())


def case_inference_autorange_switch(sim):
    m = dit(range_policy="auto")
    m(*batch(1, 2))
    sim.autorange.append(([2], 0))
    try:
        m.check()
        raise AssertionError("check() did not raise")
    except L.GtavRangeSwitch as e:
        assert e.groups == [2]
    m(*batch(1, 2))


def case_inference_autorange_check(sim):
    """A clean check(), then one whose gtav_dit_autorange moves group 0 and fails with another error."""
    m = dit(range_policy="auto")
    m(*batch(1, 2))
    m.check()
    sim.autorange.append(([0], 1))
    try:
        m.check()
        raise AssertionError("check() did not raise")
    except L.GtavRangeSwitch:
        raise
    except L.GtavError:
        pass
    m(*batch(1, 2))


def case_vae_default(sim):
    m = vae(max_frames_per_call=2)
    z = m.encode(torch.zeros(2, 3, 8, 8)).mean
    m.decode(z)
    m.encode_moments(torch.zeros(5, 3, 8, 8))      # chunks of 2
    m.check()


def case_vae_bf16(sim):
    m = vae(max_frames_per_call=2)
    m.set_operand_dtype(torch.bfloat16)
    m.set_operand_dtype(torch.bfloat16)
    m.encode_moments(torch.zeros(1, 3, 8, 8))
    m.set_operand_dtype(torch.float16)
    m.encode_moments(torch.zeros(1, 3, 8, 8))


def case_vae_growth(sim):
    m = vae(max_frames_per_call=2, grow_frames_per_call=True)
    m.set_operand_dtype(torch.bfloat16)
    m.encode_moments(torch.zeros(2, 3, 8, 8))
    m.encode_moments(torch.zeros(3, 3, 8, 8))      # destroy, create, replay, upload


CASES = {k[len("case_"):]: v for k, v in list(globals().items()) if k.startswith("case_")}


def build_table():
    table = {}
    for name, case in CASES.items():
        with stand_in() as sim:
            case(sim)
            table[name] = list(sim.calls)
            del ALIVE[:]
    return table


def dumps(table):
    lines = ["{"]
    for i, (name, calls) in enumerate(table.items()):
        lines.append(f' "{name}": [')
        lines += ["  " + json.dumps(c, separators=(",", ":")) + ("," if j + 1 < len(calls) else "") for j, c in enumerate(calls)]
        lines.append(" ]" + ("," if i + 1 < len(table) else ""))
    lines.append("}")
    return "\n".join(lines) + "\n"


def time_ensure(rounds=5, calls=100000):
    """Seconds per `calls` calls of _ensure(1, 2) on a built, clean model, `rounds` times."""
    out = []
    with stand_in():
        m = dit()
        m(*batch(1, 2))
        for _ in range(rounds):
            t0 = time.perf_counter()
            for _ in range(calls):
                m._ensure(1, 2)
            out.append(time.perf_counter() - t0)
        del m, ALIVE[:]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", action="store_true", help=f"write {os.path.relpath(TABLE, ROOT)} instead of printing")
    ap.add_argument("--out", default=TABLE)
    ap.add_argument("--time", action="store_true", help="time the fast path of _ensure instead")
    ap.add_argument("--rounds", type=int, default=5, help="timing rounds (1: for alternating with another commit's tool)")
    a = ap.parse_args()
    if a.time:
        r = time_ensure(a.rounds)
        print(json.dumps({"ensure_1e5_calls_s": [round(x, 5) for x in r], "median_s": round(statistics.median(r), 5)}))
    elif a.write:
        open(a.out, "w").write(dumps(build_table()))
        print(f"wrote {a.out}", file=sys.stderr)
    else:
        sys.stdout.write(dumps(build_table()))
