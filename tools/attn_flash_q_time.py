"""Flash spatial attention with plain and with prescaled q, fp16 and bf16 operands (gtav_op_attn_spatial / _prescaled under gtav_op_set_operand_dtype): us per
launch, 3 rounds of 50 back-to-back launches after 10 warm-up launches.  profiles/op_parity_typed/attn_flash_plain_q_time.txt is its printout."""
import sys, os, torch
sys.path.insert(0, os.getcwd())
from gtav_amd import lib as L
lib = L.load()
s = torch.cuda.current_stream().cuda_stream
for dt, code in ((torch.float16, 0), (torch.bfloat16, 1)):
    lib.gtav_op_set_operand_dtype(code)
    for NB, heads, S in ((40, 16, 576), (8, 16, 576), (16, 16, 256)):
        q, k, v = (torch.randn(NB, heads, S, 64, device="cuda").to(dt) for _ in range(3))
        vt = v.transpose(-1, -2).contiguous()
        o = torch.zeros((NB * S + 127) // 128 * 128, heads * 64, device="cuda", dtype=dt)
        res = {}
        for rnd in range(3):
            for name, fn in (("plain", lib.gtav_op_attn_spatial), ("prescaled", lib.gtav_op_attn_spatial_prescaled)):
                for _ in range(10):
                    L.check(fn(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), NB, heads, S, s))
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(50):
                    L.check(fn(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), NB, heads, S, s))
                b.record(); torch.cuda.synchronize()
                res.setdefault(name, []).append(a.elapsed_time(b) * 1e3 / 50)
        print(f"[attn_time {dt} NB={NB} heads={heads} S={S}] us per launch, 3 rounds of 50: " + "; ".join(f"{n} {min(r):.1f} .. {max(r):.1f}" for n, r in res.items()), flush=True)
lib.gtav_op_set_operand_dtype(0)
