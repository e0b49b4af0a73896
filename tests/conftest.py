import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# torch's CPU sin / cos run through MKL's vector math, whose last bits depend on the code branch MKL picks for the host CPU: its AVX-512 branch on an
# Intel CPU, its generic branch on an AMD one whatever the CPU offers.  Several oracle tests compare with tests/golden bit for bit (the timestep
# embedding, the product's host tables), so the session pins the branch every x86-64 CPU can run alike (MKL conditional numerical reproducibility,
# COMPATIBLE); g0_constants and g1_ops_dit were recorded under the same setting (tools/make_golden.py).  MKL reads it at its first call: it is set
# here, before any test computes anything, and passes to the subprocesses tests start.
os.environ.setdefault("MKL_CBWR", "COMPATIBLE")


# tests/exp/ holds the checks of code that exists only in the EXPERIMENTS build (csrc/build.sh exp -> libgtav_amd_exp.so: the LayerNorm fold, the persistent
# 256-token-tile kernel — measured slower, kept for tools/).  One process never mixes the two libraries, so they run in a session of their own:
#   GTAV_TEST_EXP=1 python -m pytest tests/exp -q        (GPU box)
# Every other session ignores the directory and loads the product library.
EXP_SESSION = os.environ.get("GTAV_TEST_EXP") == "1"
collect_ignore = [] if EXP_SESSION else ["exp"]


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: full-size CPU oracle cases (tens of seconds)")
    config.addinivalue_line("markers", "exp: experiments-build checks (GTAV_TEST_EXP=1 python -m pytest tests/exp)")


@pytest.fixture(scope="session", autouse=True)
def _built_library():
    """The HIP library is built in-tree (hipcc cross-compiles gfx950 without a GPU); tests never run on a fallback."""
    from gtav_amd import lib as L
    if EXP_SESSION:
        L.load_experiments()
        return
    L.build()          # mtime-aware (lib.build): a stale in-tree .so — they are git-ignored but travel to the GPU box — is rebuilt, a current one is kept
    L.load()


@pytest.fixture(scope="session")
def lib():
    from gtav_amd import lib as L
    L.load()
    return L
