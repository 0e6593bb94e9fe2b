// pad_skip_map_probe.cpp -- test-only entry points into the column-tile mapping of the patch kernels (ai-camera_amd/csrc/pad_skip_map.hpp),
// built with the system g++ by tests/test_pad_skip_map.py.  Not part of libaicam.so.
#include "../ai-camera_amd/csrc/pad_skip_map.hpp"

using namespace aic;

namespace {
typedef ColTiles<16, 8, 2> L3;      // ReID layer3: 16 x 8 maps, 2 images per 256-pixel block
typedef ColTiles<8, 4, 8> L4;       // ReID layer4: 8 x 4 maps, 8 images per block

template <class C> void geom(int* o) {
    o[0] = C::PW, o[1] = C::PH, o[2] = C::IPIX, o[3] = C::IPIXP, o[4] = C::NPIX, o[5] = C::NPASS, o[6] = C::CG, o[7] = C::IW, o[8] = C::max_off();
}
template <class C> void lane(int wm, int i, int r, int* o) {
    o[0] = C::img(wm, i, r), o[1] = C::y(r), o[2] = C::x(i), o[3] = C::wave_off(wm) + C::tile_off(i) + C::lane_off(r);
}
}  // namespace

// cfg 0: (TH, TW, NI) = (16, 8, 2); cfg 1: (8, 4, 8)
// out: PW, PH, IPIX, IPIXP, NPIX, NPASS, images per tile, images per wave row, largest patch offset any lane reads at any tap
extern "C" void probe_geom(int cfg, int* out) { cfg ? geom<L4>(out) : geom<L3>(out); }
// lane r of tile i of wave row wm -> image within the block, y, x, patch offset (16-byte units within a plane) of its tap (0, 0)
extern "C" void probe_lane(int cfg, int wm, int i, int r, int* out) { cfg ? lane<L4>(wm, i, r, out) : lane<L3>(wm, i, r, out); }
extern "C" int probe_tap_off(int cfg, int tap) { return cfg ? L4::tap_off(tap) : L3::tap_off(tap); }
extern "C" int probe_skip(int cfg, int i, int tap) { return cfg ? L4::skip(i, tap) : L3::skip(i, tap); }
