"""Counter-based noise (DESIGN.md "Noise streams"): the random draws of the training step (train_dit.py:574-587 `torch.randint`, :625-643
`torch.randn_like` + `clamp_`), of the sampling loop (generate.py:201, train_dit.py:417-422) and of the VAE posterior (model/vae.py:36) as pure functions of
(seed, draw number, global sample id, frame slot, element) — Philox4x32-10.  The normals are made on the device inside the launches that consume them
(gtav_rng_normal, gtav_noise_window_rng, gtav_vae_posterior_sample); the noise indices, which the host consumes, are made on the host.  This module also
restates the contract in numpy (`philox4x32_10`, `host_bits`, `host_normal`): the specification the tests hold the kernels to.

The result is distribution-identical to the reference's draws, not stream-identical to torch's generator."""
from __future__ import annotations

import math

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
SLOT_TARGET_IDX, SLOT_CTX_IDX = 0xFFFFFFFE, 0xFFFFFFFF         # the frame slots of the two integer draws (no frame of a window or clip gets there)
NORMAL_ABS_MAX = math.sqrt(-2.0 * math.log(2.0 ** -24))         # 5.7682: the largest |z| the transform can make (u >= 2^-24)
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., Random123): counter (..., 4) and key (..., 2) or (2,) of 32-bit words -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., j] for j in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _MASK, (k1 + np.uint64(PHILOX_W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _key(seed: int):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def _check_row(n: int):
    if n < 4 or n % 4:
        raise ValueError(f"a row of {n} elements: the stream is defined for rows of a multiple of 4 (one generator call makes four elements)")


def host_bits(rows: int, n: int, seed: int, draw: int, sample0: int = 0, slot0: int = 0, slots_per_sample: int = 1) -> np.ndarray:
    """The raw words of `rows` rows of n elements, (rows, n) uint32: element e of row r is word e & 3 of the generator at counter
    (e >> 2, slot0 + r % slots_per_sample, sample0 + r // slots_per_sample, draw); every counter field wraps in its own 32 bits."""
    _check_row(n)
    if slots_per_sample < 1:
        raise ValueError("slots_per_sample must be at least 1")
    r = np.arange(rows, dtype=np.uint64)
    ctr = np.empty((rows, n // 4, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(n // 4, dtype=np.uint64)[None, :]
    ctr[..., 1] = ((np.uint64(slot0) + r % np.uint64(slots_per_sample)) & _MASK)[:, None]
    ctr[..., 2] = ((np.uint64(sample0) + r // np.uint64(slots_per_sample)) & _MASK)[:, None]
    ctr[..., 3] = np.uint64(int(draw) & 0xFFFFFFFF)
    return philox4x32_10(ctr, _key(seed)).reshape(rows, n)


def uniform(bits) -> np.ndarray:
    """u(x) = ((x >> 9) + 0.5) 2^-23 in fp64: 24 significant bits, so the same number in fp32, strictly inside (0, 1)."""
    return ((np.asarray(bits, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def host_normal(rows: int, n: int, seed: int, draw: int, sample0: int = 0, slot0: int = 0, slots_per_sample: int = 1) -> np.ndarray:
    """The standard normals of the same rows in fp64 from the exact u, (rows, n): Box-Muller per word pair,
    (z0, z1) = sqrt(-2 ln u(x0)) (cos, sin)(2 pi u(x1)) and (z2, z3) likewise from (x2, x3).  |z| <= NORMAL_ABS_MAX."""
    u = uniform(host_bits(rows, n, seed, draw, sample0, slot0, slots_per_sample)).reshape(rows, n // 2, 2)
    r, phi = np.sqrt(-2.0 * np.log(u[..., 0])), 2.0 * np.pi * u[..., 1]
    return np.stack([r * np.cos(phi), r * np.sin(phi)], axis=-1).reshape(rows, n)


def host_randint(low: int, high: int, B: int, seed: int, draw: int, slot: int, sample0: int = 0) -> np.ndarray:
    """Integers in [low, high) for samples sample0 .. sample0 + B - 1, (B,) int64: low + ((x0 (high - low)) >> 32) with x0 the first word of the generator at
    counter (0, slot, sample, draw)."""
    if high <= low:
        raise ValueError(f"randint: empty range [{low}, {high})")
    ctr = np.zeros((B, 4), dtype=np.uint64)
    ctr[:, 1] = int(slot) & 0xFFFFFFFF
    ctr[:, 2] = (np.uint64(sample0) + np.arange(B, dtype=np.uint64)) & _MASK
    ctr[:, 3] = int(draw) & 0xFFFFFFFF
    x0 = philox4x32_10(ctr, _key(seed))[:, 0].astype(np.uint64)
    return (int(low) + ((x0 * np.uint64(high - low)) >> np.uint64(32)).astype(np.int64)).astype(np.int64)


def check_exclusive(rng, what: str, **draws):
    """With a NoiseSource the explicit draws of a call must be None; without one they are all required, as they were before rng= existed."""
    if rng is None:
        missing = [k for k, v in draws.items() if v is None]
        if missing:
            raise TypeError(f"{what}: {', '.join(missing)} missing (or pass rng=, a gtav_amd.rng.NoiseSource)")
        return
    given = [k for k, v in draws.items() if v is not None]
    if given:
        raise ValueError(f"{what}: rng= makes the draws itself; {', '.join(given)} must be None")


class NoiseSource:
    """One noise stream: a 64-bit seed, a draw counter and the global id of the first sample of this process' batch (data-parallel runs set
    sample0 = rank * B: every rank then draws what the unsharded batch would have drawn for its samples).  Consumers take one draw number per target
    frame of a training step and one per generated clip (`next_draw`); the state a checkpoint needs is {"seed", "draw"}."""

    def __init__(self, seed: int, sample0: int = 0):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.sample0 = int(sample0)
        self.draw = 0

    def next_draw(self) -> int:
        d = self.draw
        self.draw = (self.draw + 1) & 0xFFFFFFFF
        return d

    def randint(self, low: int, high: int, B: int, slot: int, draw: int):
        """(B,) torch.long in [low, high), made on the host (the noise indices are consumed there, train.py `_frame_step`)."""
        import torch
        return torch.from_numpy(host_randint(low, high, B, self.seed, draw, slot, self.sample0))

    def normal(self, B: int, slots: int, frame_shape, draw: int, slot0: int = 0, device=None, clamp_abs: float = math.inf):
        """(B, slots, *frame_shape) float32 on `device`: clamp(N(0,1), +-clamp_abs) of samples sample0 .. sample0 + B - 1, frame slots slot0 .. slot0 +
        slots - 1, through gtav_rng_normal."""
        import torch

        from . import lib as _lib
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        out = torch.empty((B, slots, *frame_shape), device=device, dtype=torch.float32)
        if B * slots == 0:
            return out
        n = out[0, 0].numel()
        with torch.cuda.device(device):
            _lib.check(_lib.load().gtav_rng_normal(out.data_ptr(), slots * n, B * slots, n, self.seed, draw, self.sample0 & 0xFFFFFFFF, slot0, slots,
                                                   float(clamp_abs), _lib.current_stream()))
        return out

    def clone(self) -> "NoiseSource":
        c = NoiseSource(self.seed, self.sample0)
        c.draw = self.draw
        return c

    def state_dict(self) -> dict:
        return {"seed": self.seed, "draw": self.draw}

    def load_state_dict(self, state: dict):
        self.seed = int(state["seed"]) & 0xFFFFFFFFFFFFFFFF
        self.draw = int(state["draw"]) & 0xFFFFFFFF
