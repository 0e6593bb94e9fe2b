"""The column-tile mapping of the 3x3 patch kernels on ReID's narrow maps (ai-camera_amd/csrc/pad_skip_map.hpp) on the CPU: the header is
HIP-free, built with the system g++ beside a test-only probe (tests/pad_skip_map_probe.cpp), no hipcc, no GPU.

A block of the 256-pixel x 256-channel tile holds NI whole images in two wave rows of eight 16-pixel MFMA tiles each.  A tile is one column
of one (16 x 8 maps) or two (8 x 4 maps) images, so that the tiles of the map's first and last column read nothing but the zero halo at
the taps kw = 0 / kw = 2 and the kernels leave those MFMAs out.  Checked here, for (TH, TW, NI) = (16, 8, 2) and (8, 4, 8):

  bijection   (wave row, tile, lane) -> (image, y, x) covers every pixel of the block exactly once
  columns     the sixteen pixels of a tile share x
  skip        skip(tile, tap) is true exactly where all sixteen pixels read outside the map at that tap (brute force)
  balance     every wave row skips the same number of tiles at every tap (a K-step ends at a block barrier: it only gets shorter if
              every SIMD has less to do)
  patch       the patch offset of (lane, tap) is the patch pixel (image, y + kh, x + kw) of the kernels' LDS-DMA table (slot p is image
              p / IPIXP, row rem / PW, column rem % PW; the halo and the unused columns come from the zero page)
  banks       the sixteen lanes of a ds_read_b128 lane group hit sixteen distinct 16-byte bank slots (64 banks x 4 bytes) for every tile
              and tap; the four planes of a patch buffer are a whole number of 256-byte bank rows apart
  fits        the patch passes, the kernel's LDS and the ds_read immediates
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WM, MT = 2, 8
CONFIGS = {0: (16, 8, 2), 1: (8, 4, 8)}          # probe cfg -> (TH, TW, NI)
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the mapping test builds pad_skip_map.hpp with the system compiler")
    so = str(tmp_path_factory.mktemp("pad_skip") / "libpadskip.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-fPIC", "-shared", os.path.join(ROOT, "tests", "pad_skip_map_probe.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def ints(n):
    a = np.zeros(n, np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def geom(probe, cfg):
    a, p = ints(9)
    probe.probe_geom(cfg, p)
    return dict(zip(("PW", "PH", "IPIX", "IPIXP", "NPIX", "NPASS", "CG", "IW", "max_off"), (int(v) for v in a)))


def lanes(probe, cfg):
    """[wm, tile, lane] -> (image, y, x, patch offset of tap (0, 0))"""
    out = np.zeros((WM, MT, 16, 4), np.int32)
    a, p = ints(4)
    for wm in range(WM):
        for i in range(MT):
            for r in range(16):
                probe.probe_lane(cfg, wm, i, r, p)
                out[wm, i, r] = a
    return out


@pytest.mark.parametrize("cfg", sorted(CONFIGS), ids=["16x8", "8x4"])
def test_tiles_are_columns_and_cover_the_block(probe, cfg):
    TH, TW, NI = CONFIGS[cfg]
    L = lanes(probe, cfg)
    pix = {tuple(int(v) for v in L[wm, i, r, :3]) for wm in range(WM) for i in range(MT) for r in range(16)}
    assert len(pix) == WM * MT * 16 == NI * TH * TW
    assert pix == {(il, y, x) for il in range(NI) for y in range(TH) for x in range(TW)}
    assert (L[..., 2] == L[..., :1, 2]).all()                                   # one x per tile
    for wm in range(WM):                                                        # a wave row keeps whole images: wm * IW .. wm * IW + IW - 1
        assert set(L[wm, :, :, 0].ravel().tolist()) == set(range(wm * NI // WM, (wm + 1) * NI // WM))


@pytest.mark.parametrize("cfg", sorted(CONFIGS), ids=["16x8", "8x4"])
def test_skip_is_exactly_the_halo_only_pairs_and_the_same_in_every_wave(probe, cfg):
    TH, TW, NI = CONFIGS[cfg]
    L = lanes(probe, cfg)
    counts = np.zeros((WM, 9), int)
    for wm in range(WM):
        for i in range(MT):
            for tap in range(9):
                kh, kw = divmod(tap, 3)
                iy, ix = L[wm, i, :, 1] + kh - 1, L[wm, i, :, 2] + kw - 1
                outside = (iy < 0) | (iy >= TH) | (ix < 0) | (ix >= TW)
                assert bool(probe.probe_skip(cfg, i, tap)) == bool(outside.all()), (wm, i, tap)
                counts[wm, tap] += int(outside.all())
    assert (counts == counts[0]).all()
    assert counts[0].tolist() == [MT // TW, 0, MT // TW] * 3                   # the tiles of column 0 at kw = 0, of column TW - 1 at kw = 2
    assert counts[0].sum() * 3 * TW == 9 * MT * 2                              # 2 / TW of the tiles x 1 / 3 of the taps: 1 / 12 and 1 / 6


@pytest.mark.parametrize("cfg", sorted(CONFIGS), ids=["16x8", "8x4"])
def test_patch_offsets_bank_slots_and_sizes(probe, cfg):
    TH, TW, NI = CONFIGS[cfg]
    g = geom(probe, cfg)
    L = lanes(probe, cfg)
    PW, IPIXP = g["PW"], g["IPIXP"]
    assert PW >= TW + 2 and PW % 2 == 1 and g["PH"] == TH + 2 and g["IPIX"] == PW * g["PH"] and IPIXP >= g["IPIX"]
    assert g["NPIX"] == NI * IPIXP and g["NPASS"] == -(-g["NPIX"] // 128)
    assert (cfg, PW, IPIXP, g["NPASS"]) in ((0, 11, 198, 4), (1, 7, 72, 5))
    worst = 0
    for wm in range(WM):
        for i in range(MT):
            for tap in range(9):
                kh, kw = divmod(tap, 3)
                off = L[wm, i, :, 3] + probe.probe_tap_off(cfg, tap)
                # the kernels' LDS-DMA table: slot p holds patch pixel (p / IPIXP, rem / PW, rem % PW), i.e. map pixel (row - 1, column - 1)
                il, rem = off // IPIXP, off % IPIXP
                assert (off < g["NPIX"]).all() and (rem < g["IPIX"]).all()
                assert (il == L[wm, i, :, 0]).all() and (rem // PW == L[wm, i, :, 1] + kh).all() and (rem % PW == L[wm, i, :, 2] + kw).all()
                assert len(set((off % 16).tolist())) == 16, (wm, i, tap, (off % 16).tolist())     # sixteen lanes, sixteen bank slots
                worst = max(worst, int(off.max()))
    assert worst == g["max_off"]
    plane = g["NPASS"] * 128 * 16                          # bytes of one plane (8 channels of every patch pixel) of a patch buffer
    assert plane % 256 == 0                                 # the lane groups of the other planes see the same slots
    pbuf = 4 * plane
    ring = 4 * 256 * 64                                     # four weight stages of 256 channels x one K-step
    assert g["NPASS"] <= 7                                  # v6: the passes of a chunk ride on the bodies of taps 0 .. 6
    assert 2 * pbuf + 8192 + ring <= LDS_LIMIT              # v6 (kernels_conv_sp.hip launch_sp_patch)
    assert (cfg, (2 * pbuf + 8192 + ring) // 1024) in ((0, 136), (1, 152))
    assert pbuf + g["max_off"] * 16 + 15 < 65536            # ds_read_b128 offset field: buffer + tap + tile are one immediate
