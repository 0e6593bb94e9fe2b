// pad_skip_map.hpp -- column-major 16-pixel MFMA tiles for the 3x3 / pad 1 patch kernels on maps narrower than a tile (ReID layer3: 16 x 8,
// layer4: 8 x 4), and the (tile, tap) pairs whose sixteen pixels ALL read the zero halo.  HIP-free: the kernel (kernels_conv_sp.hip)
// and the host probe of tests/test_pad_skip_map.py read the same constants.
//
// A block holds NI whole images, wave row wm the images wm * IW .. wm * IW + IW - 1 (IW = NI / WM).  A tile is ONE COLUMN x of CG = 16 / TH
// consecutive images: lane r of the MFMA's pixel operand is (image r / TH of the group, y = r % TH, x).  Tile i of a wave is column i % TW of
// its image group i / TW.  Every pixel of a tile shares x, so at the taps kw = 0 the tiles x = 0 read only the left halo and at kw = 2 the
// tiles x = TW - 1 only the right one: 2 / TW of the tiles x 1 / 3 of the taps issue no MFMA (1 / 6 on 8 x 4, 1 / 12 on 16 x 8) -- the
// same tiles in every wave, so every SIMD's K-step gets shorter by the same amount.
//
// LDS: the sixteen lanes of a ds_read_b128 lane group must hit sixteen distinct 16-byte bank slots (64 banks x 4 B = 16 slots).  Walking a
// column the stride is the patch row pitch PW, which therefore is ODD (TW + 3: one unused column per row); with two images per tile the
// image pitch IPIXP is 8 (mod 16), so that the second image's eight rows take the other eight slots.
#pragma once

namespace aic {

template <int TH, int TW, int NI, int WM = 2, int MT = 8>
struct ColTiles {
    static constexpr int CG = 16 / TH;                      // images per tile
    static constexpr int IW = NI / WM;                      // images per wave row
    static constexpr int PW = TW + 3, PH = TH + 2;          // patch row pitch (odd) and rows
    static constexpr int IPIX = PW * PH;                    // patch pixels of one image
    static constexpr int IPIXP = CG == 1 ? IPIX : IPIX + (8 - IPIX % 16 + 16) % 16;      // image pitch
    static constexpr int NPIX = NI * IPIXP, NPASS = (NPIX + 127) / 128;                  // LDS-DMA passes (128 pixels x 4 planes) per chunk
    static_assert(16 % TH == 0 && TH >= 8 && TW % 2 == 0 && NI % WM == 0 && IW % CG == 0, "a tile is one column of one or two whole images");
    static_assert(MT * CG == TW * IW, "a wave's MT tiles are the TW columns of its IW / CG image groups");
    static_assert(PW % 2 == 1 && (CG == 1 || IPIXP % 16 == 8), "bank slots");

    // patch pixel (units of 16 bytes within a plane) of tap (0, 0) of: wave row wm's first image, tile i relative to it, lane r relative to the tile
    static constexpr int wave_off(int wm) { return wm * IW * IPIXP; }
    static constexpr int tile_off(int i) { return (i / TW) * CG * IPIXP + i % TW; }
    static constexpr int lane_off(int r) { return (r / TH) * IPIXP + (r % TH) * PW; }
    static constexpr int tap_off(int tap) { return (tap / 3) * PW + tap % 3; }
    // the pixel itself: image within the block, row, column
    static constexpr int img(int wm, int i, int r) { return wm * IW + (i / TW) * CG + r / TH; }
    static constexpr int y(int r) { return r % TH; }
    static constexpr int x(int i) { return i % TW; }
    // every pixel of tile i reads padding at this tap: its MFMAs would add +-0 to every accumulator
    static constexpr bool skip(int i, int tap) { return (tap % 3 == 0 && x(i) == 0) || (tap % 3 == 2 && x(i) == TW - 1); }
    static constexpr int max_off() { return wave_off(WM - 1) + tile_off(MT - 1) + lane_off(15) + tap_off(8); }
};

}  // namespace aic
