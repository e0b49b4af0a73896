#!/usr/bin/env python3
"""Per-kernel register / scratch / LDS / kernel-argument-preload report of one HIP source: compiles its device code for gfx950 to assembly with
-Rpass-analysis=kernel-resource-usage and prints one line per kernel instantiation (demangled).  `preload` is the kernel descriptor's
.amdhsa_user_sgpr_kernarg_preload_length: how many leading kernel-argument dwords arrive in SGPRs with the wave (csrc/build.sh passes
-mllvm -amdgpu-kernarg-preload-count for the sources of the batch-1 step; pass the same flag here to see what the build sees).
usage: tools/kernel_resources.py csrc/gemm.hip [filter-regex] [extra hipcc flags]"""
import re
import subprocess
import sys

src = sys.argv[1]
flt = sys.argv[2] if len(sys.argv) > 2 else ""
extra = sys.argv[3:]
r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-pass-failed",
                    "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", src, "-o", "-"] + extra, capture_output=True, text=True)
blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
if not blocks:      # the compile failed (or has no kernels): show why instead of handing c++filt an empty list, which makes it wait on stdin
    sys.exit(r.stderr[-4000:] or "no kernels found")
preload = {m.group(1): int(m.group(2)) for m in
           re.finditer(r"\.amdhsa_kernel (\S+)\n.*?\.amdhsa_user_sgpr_kernarg_preload_length (\d+)\n.*?\.end_amdhsa_kernel", r.stdout, re.S)}
names = [b.split()[0] for b in blocks]
dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.strip().split("\n")
# (a c++filt that predates the _Float16 / __bf16 manglings leaves kernels with such pointer arguments mangled: the name and its template arguments still read)
dem = [re.sub(r"^_ZN\d+gtav(?:_bf16)?\d+_GLOBAL__N_1\d+", "", d) for d in dem]
for b, d, raw in zip(blocks, dem, names):
    g = lambda k: int(re.search(re.escape(k) + r": (\d+)", b).group(1))
    m = re.search(r"(\w+<.*>)\(", d)
    nm = (m.group(1) if m else d).replace("gtav::(anonymous namespace)::", "").replace("gtav_bf16::(anonymous namespace)::", "")
    if flt and not re.search(flt, nm):
        continue
    print(f"{nm:70s} VGPR {g('VGPRs'):4d} AGPR {g('AGPRs'):4d} SGPR {g('TotalSGPRs'):4d} scratch {g('ScratchSize [bytes/lane]'):5d} "
          f"spill s/v {g('SGPRs Spill')}/{g('VGPRs Spill')} occ {g('Occupancy [waves/SIMD]')} LDS {g('LDS Size [bytes/block]')} preload {preload.get(raw, 0):2d}")
