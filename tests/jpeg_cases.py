"""Shared case builders of the JPEG tests (test_jpeg_oracle.py, test_gpu_jpeg.py): the smallest images at which each part of the
format can go wrong, each with the oracle's encoding computed once."""
import functools
from collections import namedtuple

import numpy as np

import jpeg_oracle as O

Case = namedtuple("Case", "name image quality restart subsampling")
ALL_Q = (1, 50, 85, 100)


def gray(plane):
    return np.repeat(np.asarray(plane, np.uint8)[:, :, None], 3, axis=2)


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def block_checkerboard():
    """16 x 32 of 8 x 8 black and white blocks: the DC difference swings over the whole range (category 11 at q100)."""
    y, x = np.mgrid[0:16, 0:32]
    return gray(((y // 8 + x // 8) % 2) * 255)


def pixel_checkerboard():
    """16 x 32, every pixel the opposite of its neighbours: the largest AC coefficient (category 10 at q100)."""
    y, x = np.mgrid[0:16, 0:32]
    return gray(((y + x) % 2) * 255)


def one_high_frequency():
    """Blocks whose only AC energy is coefficient (7, 7): long zero runs, ZRL three times per block."""
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    return gray(np.tile(np.clip(np.rint(128 + 100 * np.outer(c, c)), 0, 255), (2, 2)))


def primaries():
    """Left half blue, right half red, green added on the lower 8 rows: the chroma extremes."""
    img = np.zeros((16, 16, 3), np.uint8)
    img[:, :8, 0], img[:, 8:, 2], img[8:, :, 1] = 255, 255, 255
    return img


def flat():
    return np.full((16, 16, 3), 128, np.uint8)


def scene(h, w, seed=0):
    """A smooth synthetic-style scene with a few rectangles and mild noise: what a camera frame compresses like."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(h + w - 2, 1)], axis=-1).astype(np.int32)
    for _ in range(4):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[y0:y0 + h // 3 + 1, x0:x0 + w // 4 + 1] = rng.integers(0, 256, 3)
    return np.clip(img + rng.integers(-6, 7, img.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def images():
    return {"noise": noise(16, 16, 1), "block_checkerboard": block_checkerboard(), "pixel_checkerboard": pixel_checkerboard(),
            "one_high_frequency": one_high_frequency(), "primaries": primaries(), "flat": flat(), "tiny_1x1": scene(1, 1, 2),
            "tiny_8x8": scene(8, 8, 3), "odd_17x33": scene(17, 33, 4), "odd_33x17": scene(33, 17, 5), "tall": scene(160, 16, 6),
            "chunk_walk": noise(24, 2048, 7)}


@functools.lru_cache(maxsize=None)
def cases():
    im, out = images(), []

    def add(name, qualities, restarts=(0,), subs=(420, 444)):
        out.extend(Case(f"{name}-q{q}-r{r}-{s}", im[name], q, r, s) for q in qualities for r in restarts for s in subs)
    add("noise", (100, 1))
    add("block_checkerboard", (100,))
    add("pixel_checkerboard", (100,))
    add("one_high_frequency", (100, 50))
    add("primaries", (100,))
    add("flat", ALL_Q)
    for name in ("tiny_1x1", "tiny_8x8", "odd_17x33", "odd_33x17"):
        add(name, ALL_Q)
    add("tall", ALL_Q, restarts=(0, 1, 3, 65535))
    add("chunk_walk", (100,), restarts=(65535,))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's bytes of a case, computed once."""
    c = next(c for c in cases() if c.name == name)
    return O.encode(c.image, c.quality, c.restart, c.subsampling)


def bank(n, h=17, w=33):
    """n images of different content and one size, for one call."""
    return np.stack([scene(h, w, 100 + i) if i % 2 else noise(h, w, 100 + i) for i in range(n)])
