"""The noise-stream contract (DESIGN.md "Noise streams") on the host: gtav_amd.rng restates it in numpy, and these tests pin that restatement — the known
answers of Philox4x32-10, the moments of the normal transform, the integer draws, the NoiseSource state — plus everything of the rng= interface that can be
checked without a GPU (argument exclusivity, C-ABI validation).  tests/test_gpu_rng.py holds the kernels to the same restatement."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

from gtav_amd import lib as L
from gtav_amd import rng as R

N = 1 << 20
SEED = 0x1234

# Random123's known-answer vectors for philox4x32_10: counter, key -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    assert tuple(int(v) for v in R.philox4x32_10(counter, key)) == want


def test_philox_is_vectorised_over_leading_axes():
    ctr = np.array([k[0] for k in KAT], dtype=np.uint64)
    key = np.array([k[1] for k in KAT], dtype=np.uint64)
    out = R.philox4x32_10(ctr, key)
    assert out.dtype == np.uint32 and out.tolist() == [list(k[2]) for k in KAT]


def test_host_bits_follow_the_counter_layout():
    """Element e of row r is word e & 3 of the generator at counter (e >> 2, slot, sample, draw), key = the two halves of the seed; the fields wrap in
    their own 32 bits."""
    seed, draw, sample0, slot0, sps = 0xDEADBEEF12345678, 7, 0xFFFFFFFE, 30, 3
    bits = R.host_bits(7, 12, seed, draw, sample0, slot0, sps)
    assert bits.shape == (7, 12) and bits.dtype == np.uint32
    for r, e in [(0, 0), (2, 5), (3, 11), (6, 8)]:
        ctr = (e >> 2, slot0 + r % sps, (sample0 + r // sps) & 0xFFFFFFFF, draw)
        assert int(bits[r, e]) == int(R.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[e & 3])
    # any split of the rows gives the same words
    assert np.array_equal(bits[3:6], R.host_bits(3, 12, seed, draw, sample0 + 1, slot0, sps))
    assert np.array_equal(bits[4:5], R.host_bits(1, 12, seed, draw, sample0 + 1, slot0 + 1, 1))
    with pytest.raises(ValueError):
        R.host_bits(1, 6, seed, draw)


def test_uniform_is_exact_in_fp32_and_strictly_inside_the_unit_interval():
    x = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF], dtype=np.uint32)
    u = R.uniform(x)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert abs(R.NORMAL_ABS_MAX - 5.7682) < 1e-4


def moment_checks(z):
    """The five-sigma bounds of the issue for N standard normals: (name, measured, bound) per statistic.  Under the null the mean has variance 1/N, the
    variance 2/N, the third moment 15/N, the fourth 96/N, the lag-1 correlation 1/N."""
    n = z.size
    z = z.astype(np.float64)
    lag1 = float(np.mean(z[:-1] * z[1:]) / np.mean(z * z))
    return [("mean", float(z.mean()), 5 / math.sqrt(n)), ("var - 1", float(z.var() - 1), 5 * math.sqrt(2 / n)),
            ("third moment", float((z ** 3).mean()), 5 * math.sqrt(15 / n)), ("fourth moment - 3", float((z ** 4).mean() - 3), 5 * math.sqrt(96 / n)),
            ("lag-1 correlation", lag1, 5 / math.sqrt(n))]


def test_host_normal_moments():
    z = R.host_normal(1, N, SEED, 0)[0]
    for name, got, bound in moment_checks(z):
        print(f"[host normal] {name}: {got:.3e} (bound {bound:.3e})")
        assert abs(got) < bound, name
    print(f"[host normal] max |z|: {np.abs(z).max():.4f}")
    assert np.abs(z).max() <= 5.7682


def test_host_normal_pairs_are_box_muller_of_the_words():
    bits = R.host_bits(1, 8, SEED, 3, 5, 2)[0]
    u = R.uniform(bits)
    z = R.host_normal(1, 8, SEED, 3, 5, 2)[0]
    for p in range(4):
        r = math.sqrt(-2 * math.log(u[2 * p]))
        assert z[2 * p] == pytest.approx(r * math.cos(2 * math.pi * u[2 * p + 1]), abs=1e-14)
        assert z[2 * p + 1] == pytest.approx(r * math.sin(2 * math.pi * u[2 * p + 1]), abs=1e-14)


# ---- integer draws ------------------------------------------------------------------------------------------------------------------------
def test_randint_range_determinism_and_counter():
    src = R.NoiseSource(SEED, sample0=3)
    a = src.randint(1, 51, 4096, R.SLOT_TARGET_IDX, 9)
    assert a.dtype == torch.long and a.shape == (4096,) and int(a.min()) >= 1 and int(a.max()) <= 50
    assert set(a.tolist()) == set(range(1, 51))
    assert torch.equal(a, R.NoiseSource(SEED, sample0=3).randint(1, 51, 4096, R.SLOT_TARGET_IDX, 9))
    assert not torch.equal(a, src.randint(1, 51, 4096, R.SLOT_TARGET_IDX, 10))
    assert not torch.equal(a, R.NoiseSource(SEED + 1, sample0=3).randint(1, 51, 4096, R.SLOT_TARGET_IDX, 9))
    # value = low + ((x0 (high - low)) >> 32), x0 = word 0 at counter (0, slot, sample, draw)
    x0 = int(R.philox4x32_10((0, R.SLOT_TARGET_IDX, 3 + 17, 9), (SEED, 0))[0])
    assert int(a[17]) == 1 + ((x0 * 50) >> 32)
    assert src.draw == 0                                  # explicit draw numbers do not advance the source
    with pytest.raises(ValueError):
        src.randint(5, 5, 4, 0, 0)


def test_randint_slots_are_independent():
    src = R.NoiseSource(SEED)
    n = 100_000
    t = src.randint(0, 1 << 20, n, R.SLOT_TARGET_IDX, 0).double()
    c = src.randint(0, 1 << 20, n, R.SLOT_CTX_IDX, 0).double()
    corr = float(((t - t.mean()) * (c - c.mean())).mean() / (t.std() * c.std()))
    assert abs(corr) < 5 / math.sqrt(n), corr
    assert float((t == c).double().mean()) < 1e-3


def test_randint_is_uniform_chi_square():
    """10^5 draws over 50 bins: the statistic is chi-square with 49 degrees of freedom under the null, 99.9 % quantile 85.351."""
    n = 100_000
    v = R.NoiseSource(SEED).randint(0, 50, n, R.SLOT_TARGET_IDX, 0)
    counts = torch.bincount(v, minlength=50).double()
    chi2 = float(((counts - n / 50) ** 2 / (n / 50)).sum())
    print(f"[randint] chi-square {chi2:.2f} (49 dof, 99.9 % quantile 85.351)")
    assert chi2 < 85.351


def test_randint_does_not_depend_on_the_batch_split():
    whole = R.NoiseSource(SEED, sample0=0).randint(1, 41, 8, R.SLOT_CTX_IDX, 2)
    parts = [R.NoiseSource(SEED, sample0=s).randint(1, 41, b, R.SLOT_CTX_IDX, 2) for s, b in ((0, 3), (3, 1), (4, 4))]
    assert torch.equal(whole, torch.cat(parts))


# ---- NoiseSource ----------------------------------------------------------------------------------------------------------------------------
def test_noise_source_state_round_trip_through_json():
    src = R.NoiseSource(0xFEDCBA9876543210, sample0=16)
    assert [src.next_draw() for _ in range(3)] == [0, 1, 2]
    state = json.loads(json.dumps({"step": 3, "rng": src.state_dict()}))["rng"]
    assert state == {"seed": 0xFEDCBA9876543210, "draw": 3}
    fresh = R.NoiseSource(1, sample0=16)
    fresh.load_state_dict(state)
    assert (fresh.seed, fresh.draw, fresh.sample0) == (src.seed, src.draw, 16)
    d = fresh.next_draw()
    assert d == src.next_draw() == 3
    assert torch.equal(fresh.randint(1, 51, 5, R.SLOT_TARGET_IDX, d), src.randint(1, 51, 5, R.SLOT_TARGET_IDX, d))
    c = src.clone()
    assert c.state_dict() == src.state_dict() and c.sample0 == src.sample0
    c.next_draw()
    assert c.draw == src.draw + 1                        # a clone advances on its own


def test_rng_and_explicit_draws_exclude_each_other():
    """Checked before anything touches the model or the device."""
    from gtav_amd.generate import generate_latents
    from gtav_amd.train import forward_loss, predict, predict_noise, training_step
    src = R.NoiseSource(SEED)
    lat = torch.zeros(2, 5, 16, 8, 16)
    idx, cn, nz = torch.tensor([3, 4]), torch.zeros(2, 4, 16, 8, 16), torch.zeros(2, 1, 16, 8, 16)
    for given in ({"target_noise_idx": idx}, {"ctx_noise_idx": idx}, {"ctx_noise": cn}, {"noise": nz},
                  {"target_noise_idx": idx, "ctx_noise_idx": idx, "ctx_noise": cn, "noise": nz}):
        with pytest.raises(ValueError, match="must be None"):
            training_step(None, lat, None, lr=1e-3, rng=src, ctx_max_noise_idx=40, **given)
        with pytest.raises(ValueError, match="must be None"):
            forward_loss(None, lat, None, rng=src, ctx_max_noise_idx=40, **given)
    with pytest.raises(ValueError, match="ctx_max_noise_idx"):
        training_step(None, lat, None, lr=1e-3, rng=src)
    with pytest.raises(ValueError, match="ctx_max_noise_idx"):
        forward_loss(None, lat, None, rng=src)
    with pytest.raises(ValueError, match="exactly one"):
        generate_latents(None, lat[:, :1], 4, 3, nz, rng=src)
    with pytest.raises(ValueError, match="exactly one"):
        generate_latents(None, lat[:, :1], 4, 3)
    with pytest.raises(ValueError, match="must be None"):
        predict(None, None, lat, None, nz, rng=src)
    with pytest.raises(ValueError, match="must be None"):
        predict_noise(None, None, lat, None, cn, None, rng=src)
    assert src.draw == 0                                  # a refused call consumes nothing


def test_cabi_rng_argument_validation_without_gpu():
    """The noise entry points reject bad arguments before touching the device: an error code and a message (the buffer is host memory that is never used)."""
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    inf = float("inf")

    def refused(rc, text):
        assert rc != 0 and text in lib.gtav_last_error(), lib.gtav_last_error()

    refused(lib.gtav_rng_normal(None, 8, 1, 8, 1, 0, 0, 0, 1, inf, None), b"null pointer")
    refused(lib.gtav_rng_normal(addr, 6, 1, 6, 1, 0, 0, 0, 1, inf, None), b"multiple of 4")
    refused(lib.gtav_rng_normal(addr, 8, 0, 8, 1, 0, 0, 0, 1, inf, None), b"rows")
    refused(lib.gtav_rng_normal(addr, 8, 1, 8, 1, 0, 0, 0, 0, inf, None), b"slots_per_sample")
    refused(lib.gtav_rng_normal(addr + 4, 8, 1, 8, 1, 0, 0, 0, 1, inf, None), b"16-byte")
    refused(lib.gtav_rng_normal(addr, 8, 4, 8, 1, 0, 0, 0, 2, inf, None), b"sample_stride")
    refused(lib.gtav_noise_window_rng(addr, None, addr, addr, 1, 1, 8, 1, 0, 0, 20.0, None), b"null pointer")
    refused(lib.gtav_noise_window_rng(addr, addr, addr, addr, 1, 1, 6, 1, 0, 0, 20.0, None), b"multiple of 4")
    refused(lib.gtav_noise_window_rng(addr, addr, addr, addr, 0, 5, 8, 1, 0, 0, 20.0, None), b"B=0")
    refused(lib.gtav_vae_posterior_sample(None, addr, 1, 2, 4, 1, 0, 0, 0, 1, None), b"null pointer")
    refused(lib.gtav_vae_posterior_sample(addr, addr, 1, 2, 6, 1, 0, 0, 0, 1, None), b"multiple of 4")
    refused(lib.gtav_vae_posterior_sample(addr, addr, 1, 2, 4, 1, 0, 0, 0, 0, None), b"slots_per_sample")
    refused(lib.gtav_op_rng_bits(None, 1, 8, 1, 0, 0, 0, 1, None), b"null")
    refused(lib.gtav_op_rng_bits(addr, 1, 6, 1, 0, 0, 0, 1, None), b"multiple of 4")
    assert not any(buf)
