"""CPU (no GPU): the host side of low-rank adapter training — the adapters' names and shapes, the constructor's refusals, the CPU control of the kernel-level
bounds of tests/lora_bounds.py (a correct fp32 emulation stays inside every one, the truncating store does not pass the global threshold), and the C-ABI."""
import ctypes
import math
import os
import re

import pytest
import torch

import lora_bounds as LB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = torch.float16, torch.bfloat16
NEW_SYMBOLS = ("gtav_dit_train_set_lora", "gtav_dit_lora_get_merged")
KERNEL_LEVEL = ("gtav_op_lora_grads", "gtav_op_lora_merge")     # declared with the other gtav_op_* kernel-level entry points of gtav_amd.h
TOY = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)


def test_lora_param_shapes_dit_s2_rank16():
    import gtav_amd.weights as W
    kw = dict(input_h=18, input_w=32, patch_size=2, hidden_size=1024, depth=16, num_heads=16)
    s = W.lora_param_shapes(16, **kw)
    assert list(s) == sorted(s), "the gradient arena is laid out in lexicographic name order"
    assert len(s) == 2 * 2 * 16 * 4                               # A and B, two half-blocks, 16 blocks, four Linears
    assert s["blocks.0.s_attn.to_qkv.lora_A.weight"] == (16, 1024) and s["blocks.0.s_attn.to_qkv.lora_B.weight"] == (3072, 16)
    assert s["blocks.15.t_attn.to_out.lora_A.weight"] == (16, 1024) and s["blocks.15.t_attn.to_out.lora_B.weight"] == (1024, 16)
    assert s["blocks.7.t_mlp.fc1.lora_A.weight"] == (16, 1024) and s["blocks.7.t_mlp.fc1.lora_B.weight"] == (4096, 16)
    assert s["blocks.7.s_mlp.fc2.lora_A.weight"] == (16, 4096) and s["blocks.7.s_mlp.fc2.lora_B.weight"] == (1024, 16)
    base = W.dit_param_shapes(**kw)
    for k, shp in s.items():                                      # every adapter belongs to a GEMM weight of a block, with matching outer dimensions
        w = base[re.sub(r"\.lora_[AB]\.weight$", ".weight", k)]
        assert shp == ((16, w[1]) if ".lora_A." in k else (w[0], 16)), k
    nk = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)]
    assert sum(a * b for a, b in s.values()) == 2 * 16 * 16 * sum(n + k for n, k in nk) == 8388608
    assert not any(k in s for k in base) and not any("adaLN" in k or "embedder" in k or "final_layer" in k for k in s)
    with pytest.raises(ValueError, match="rank"):
        W.lora_param_shapes(8, **kw)


def test_constructor_validation():
    from gtav_amd.model.dit import DiT
    with pytest.raises(ValueError, match="trainable=True"):
        DiT(**TOY, init_weights=False, train_lora_rank=16)
    for bad in (8, 48, 128, 0, 16.5):
        with pytest.raises(ValueError, match="train_lora_rank"):
            DiT(**TOY, init_weights=False, trainable=True, train_lora_rank=bad)
    with pytest.raises(ValueError, match="train_range_policy"):
        DiT(**TOY, init_weights=False, trainable=True, train_lora_rank=16, train_range_policy="auto")
    with pytest.raises(ValueError, match="train_lora_alpha"):
        DiT(**TOY, init_weights=False, trainable=True, train_lora_rank=16, train_lora_alpha=0.0)
    with pytest.raises(ValueError, match="train_lora_rank"):
        DiT(**TOY, init_weights=False, trainable=True, train_lora_alpha=4.0)
    m = DiT(**TOY, init_weights=False, trainable=True, train_lora_rank=32)
    assert m.lora_rank == 32 and m.lora_alpha == 32.0 and not m._handle                 # alpha defaults to the rank; nothing touches the device
    sd = m.lora_state_dict()
    import gtav_amd.weights as W
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(W.lora_param_shapes(32, **TOY))
    for k, v in sd.items():
        if ".lora_B." in k:
            assert v.abs().max() == 0
        else:
            bound = 1 / math.sqrt(v.shape[1])
            assert 0.9 * bound < v.abs().max() <= bound and abs(v.mean()) < 0.1 * bound
    m2 = DiT(**TOY, init_weights=False, trainable=True, train_lora_rank=32)
    assert all(torch.equal(v, m2.lora_state_dict()[k]) for k, v in sd.items())         # seeded
    m2.init_lora(seed=1)
    assert not torch.equal(sd["blocks.0.s_attn.to_qkv.lora_A.weight"], m2.lora_state_dict()["blocks.0.s_attn.to_qkv.lora_A.weight"])
    bad = dict(sd)
    bad["blocks.0.s_attn.to_qkv.lora_A.weight"] = torch.zeros(16, 256)
    with pytest.raises(RuntimeError, match=r"blocks\.0\.s_attn\.to_qkv\.lora_A\.weight has shape \(16, 256\)"):
        m.load_lora_state_dict(bad)
    missing = dict(sd)
    del missing["blocks.1.t_mlp.fc2.lora_B.weight"]
    missing["blocks.1.t_mlp.fc2.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match=r"missing keys \['blocks\.1\.t_mlp\.fc2\.lora_B\.weight'\], unexpected keys \['blocks\.1\.t_mlp\.fc2\.weight'\]"):
        m.load_lora_state_dict(missing)
    plain = DiT(**TOY, init_weights=False, trainable=True)
    from gtav_amd.lib import GtavError
    with pytest.raises(GtavError, match="no adapters"):
        plain.lora_state_dict()


DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])


@DTYPES
def test_emulation_controls(dtype):
    """The fp32 emulation with t and u stored round-to-nearest passes every per-element bound and the global threshold on every shape and rank; with the
    truncating store it fails the global threshold on every one.  Prints the figures GLOBAL_TOL's comment quotes."""
    rne, trunc = [], []
    for (M, N, K) in LB.SHAPES:
        for r in LB.RANKS:
            c = LB.lora_case(M, N, K, r, dtype)
            good, bad = LB.grad_errors(c, *c.emulate(LB.store_rne)), LB.grad_errors(c, *c.emulate(LB.store_trunc))
            for name in ("dA", "dB"):
                assert good[name][1] <= 1.0, (M, N, K, r, name, good[name])
                assert good[name][0] < LB.GLOBAL_TOL[dtype] < bad[name][0], (M, N, K, r, name, good[name], bad[name], LB.GLOBAL_TOL[dtype])
                rne.append(good[name][0])
                trunc.append(bad[name][0])
            w = c.emulate_merge()
            assert LB.outside((w.double() - c.w).abs(), c.w_acc)[1] <= 1.0                       # the fp32 export's bound
            for store, ok in ((LB.store_rne, True), (LB.store_trunc, False)):
                worst = LB.outside((store(w, dtype).double() - c.w).abs(), c.w_tol)[1]
                assert (worst <= 1.0) == ok, (M, N, K, r, store.__name__, worst)                  # ... and the image's catches the wrong store
    print(f"[lora emulation {LB.NAME[dtype]}] store_rne {min(rne):.3e} .. {max(rne):.3e}, store_trunc {min(trunc):.3e} .. {max(trunc):.3e}, "
          f"threshold {LB.GLOBAL_TOL[dtype]:.3e}")
    assert abs(math.sqrt(max(rne) * min(trunc)) / LB.GLOBAL_TOL[dtype] - 1) < 0.02, "GLOBAL_TOL is the geometric mean of the two measured figures"


def test_cabi_declares_and_exports_the_new_symbols():
    from gtav_amd import lib as L

    def decls(name):
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        return set(re.findall(r"\b(gtav_[a-z0-9_]+)\s*\(", hdr))
    product, hooks = decls("gtav_amd.h"), decls("gtav_amd_testing.h")
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS + KERNEL_LEVEL:
        assert name in product and name not in hooks and name in L.SIGNATURES and hasattr(dll, name), name
    lib = L.load()
    assert lib.gtav_abi_version() == 4           # new entry points, no changed signature
    # argument validation that touches no device
    assert lib.gtav_dit_train_set_lora(None, 16, 16.0) != 0 and b"null handle" in lib.gtav_last_error()
    assert lib.gtav_dit_lora_get_merged(None, b"x", None, 0, None) != 0 and b"null argument" in lib.gtav_last_error()
    assert lib.gtav_op_lora_grads(None, None, None, None, 96, 256, 256, 16, 1.0, None, None, None, 0, None, None) != 0 and b"null argument" in lib.gtav_last_error()
    assert lib.gtav_op_lora_merge(None, None, None, 256, 256, 16, 1.0, None, None, None, None) != 0 and b"null image" in lib.gtav_last_error()
