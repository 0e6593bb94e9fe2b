// conv_plan.hpp -- which kernel runs a conv layer, decided apart from launching it.  Plain C++ (no HIP header): the CPU test
// (tests/test_conv_plan.py) builds conv_plan.cpp with the system compiler and checks the decision tree against a table of the
// project's layers.  The launchers (kernels_conv*.hip) map a ConvPlan to its template instantiation and launch it.
#pragma once
#include "assoc_host.hpp"
#include "row_band.hpp"

namespace aic {

// ------------------------------------------------------------------ conv layer arguments (the kernels' argument block)
struct ConvArgs {
    const void* x;      // NHWC input, element type T
    const void* w;      // packed weights [CoutPad][Kp], element type T, K = (kh, kw, cin)
    const float* bias;  // [CoutPad]
    void* y;            // NHWC output (T, or float when out_f32)
    const void* res;    // residual, same layout family as y (type T)
    int x_cs, x_coff, H, W, Cin;       // pixel stride (elements), channel offset, spatial dims, cin (multiple of 16B/sizeof(T))
    int y_cs, y_coff, Ho, Wo, Cout;
    int r_cs, r_coff, res_mode, act;
    int KH, KW, stride, pad;
    int Kp;             // K padded to a multiple of the K-step
    int M;              // N * Ho * Wo
    int out_f32;
    int cout_pad;       // rows in w / bias (multiple of 128)
    unsigned tap_rows;  // bit kh*KW set for kh < KH (replication pattern of the tap-validity mask)
    const void* zero;   // 64 bytes of zeros in HBM: LDS-DMA source for padded / out-of-range chunks
    int xcd_map;        // 1: blocks take tiles through xcd_tile() (set by launch_conv_igemm)
    const float* bias_init;   // non-NULL (k_order 2 only): the accumulators START from this bias and `bias` points at zeros -- the
                              // weights-resident kernels add their products onto the bias, (bias + sum) and (sum + bias) round differently
    const int* n_dev;   // optional DEVICE-side item count (images / crops of this launch): M then is only an upper bound the grid was sized
                        // for, and tiles past n_dev[0] * Ho * Wo leave at once (ReID behind the on-device detection filter, where the
                        // host does not know the count when it launches).  NULL: M is exact
    int k_order;        // order in which the K-steps (tap row kh, tap column kw, channel chunk cc) are accumulated:
                        //   0 = (kh, kw, cc)  tap-major, the memory order of the packed weights (default);
                        //   1 = (cc, kh, kw)  the order of the ping-pong patch kernel (conv3x3_pp_patch_kernel);
                        //   2 = (kw, cc, kh)  the order of the weights-resident 64-channel kernels (conv3x3_c64_resident / _block).
                        // Set by launch_conv_igemm from the layer SHAPE (conv_k_order): a layer one of those kernels can take is accumulated in that
                        // kernel's order by EVERY kernel its batch size may select, so embeddings do not depend on the batch
    // ---- optional SECOND SOURCE: a 1x1 conv of another tensor accumulated into the same outputs (ResNet's downsample branch folded into
    // the block's last conv: relu(conv3x3(t) + b + conv1x1/s(x) + b') is ONE GEMM over K = [window of t | channels of x]).  The packed
    // weight rows hold the window's K columns, then Cin2 more; `bias` is the sum of both.  Only layers walked chunk-major (k_order 1)
    // by the LDS-DMA implicit-GEMM kernels take it; x2's K-steps come after the window's.  x2 == NULL: none.
    const void* x2;       // NHWC, element type T; output pixel (oh, ow) reads x2 pixel (oh * s2, ow * s2)
    int x2_cs, x2_coff, H2, W2, s2, Cin2;
    // ---- optional SPLIT SOURCE of a 1x1 / stride 1 conv: its first Cs input channels are not in x but in another tensor of half the
    // resolution, read at (ih >> 1, iw >> 1) -- a 2x nearest-neighbour upsample that was only ever the first slice of this conv's
    // concatenated input (YOLOv8's neck: up(P5) | P4 -> C2f.cv1).  The upsample launch, its write and three quarters of this conv's read
    // of those channels go away; same values, same K order: bit-identical.  x / x_coff address channel 0 of the concat buffer as
    // before (channels Cs .. Cin-1 are read from it).  xs == NULL: none.
    const void* xs;
    int xs_cs, xs_coff, Hs, Ws, Cs;
    // ---- optional 1x1 "tail" conv run in this conv's epilogue (fp16 only; conv_tail_supported()).  This conv's own output
    // (SiLU(acc + bias) rounded to fp16, exactly what it would have stored) never leaves the registers: it is the B operand of
    // the tail's MFMAs.  y / y_cs / y_coff of THIS conv are then unused.  w_tail == NULL: no tail.
    const void* w_tail;   // packed weights of the 1x1 [t_cout_pad][t_kp], K = this conv's Cout
    const float* b_tail;  // [t_cout_pad]
    void* y_tail;         // NHWC output of the tail (fp16, or float when t_out_f32)
    int t_cout, t_kp, t_y_cs, t_y_coff, t_out_f32, t_act;
    // ---- optional CLASS REDUCTION of the tail (the detect head's class branch, whose logits only ever feed an arg-max): instead of
    // storing t_cout fp32 logits per pixel (320 bytes per anchor written here, read back by decode_kernel) the tail stores their
    // maximum and the FIRST channel that reaches it (np.argmax's rule, as decode_kernel) -- the very fp32 values it would have stored,
    // compared in registers.  Pixel m of the tail's map goes to t_max / t_arg[(m / t_hw) * t_na + t_a0 + m % t_hw]
    // (image-major anchor order of DetArgs).  t_max == NULL: none (y_tail is then written as usual).
    float* t_max; int* t_arg;
    int t_hw, t_a0, t_na;
    // ---- optional BOX DECODE of the tail (the detect head's box branch: 4 sides x 16 DFL bins per pixel): instead of 64 fp32 logits
    // per pixel (256 bytes per anchor written, read back by decode_kernel) the tail stores the decoded xyxy box -- decode_kernel's own
    // arithmetic on the same fp32 values in the same order (max, then exp / running sums bin 0 .. 15, one division per side), so the
    // boxes are the bits decode_kernel would have produced.  Same anchor indexing as t_max; t_w / t_stride: the level's map width and
    // stride.  t_box == NULL: none.
    float* t_box; int t_w, t_stride;
    // ---- optional ROW WINDOW (row_band.hpp): the launch computes output rows [win_y0, win_y0 + win_rows) only -- in whole tiles from a
    // clamped origin (tile_window) or exactly, by kernel -- and leaves every other row of y as it is.  Bounds checks and zero padding
    // stay those of the full map: the window's edge rows read their real neighbours.  Only the direct kernels of YOLOv8n's first stages
    // take it (conv3x3_c16, conv3x3_c32s2_tail, conv3x3_patch, conv1x1_stream, and c2f16_fused through its cv2's arguments); plan_conv
    // does not look at it.  win_rows == 0: the full map.
    int win_y0, win_rows;
    // ---- optional PIXEL LIST (conv_igemm_dma_kernel only, fp16; plan_conv sends a listed launch nowhere else): GEMM row m stands for
    // output pixel pix_list[m] -- a linear index img * Ho * Wo + oy * Wo + ox of the FULL map -- instead of pixel m.  The row is gathered,
    // stored, and (with a tail) decoded at that pixel's own position, every row independently of its tile neighbours, in the layer's K
    // order: the listed pixels get the bits the dense launch gives them and every other pixel of y is left as it is.  The live rows are
    // min(pix_count[0], M) with M = N * Ho * Wo still the map's size (the grid is sized for it: a list never holds more); an entry outside
    // [0, M) is a dead row -- it reads the zero page and stores nothing.  Both are DEVICE pointers.  pix_list == NULL: none.
    const int* pix_list; const int* pix_count;
};

// CUs the persistent (one-block-per-CU) conv kernels size their grids for: all of them, minus the one the association epoch
// kernel occupies for ~1 ms at a time while the tracker runs on the device (a 256th persistent block would otherwise sit in
// the queue until that CU or another block's whole share of the images is done).
int conv_cu_budget();
void set_conv_cu_budget(int cus);

// The kernel forms, by translation unit.
enum class ConvForm {
    Dma,          // kernels_conv.hip: LDS-DMA implicit GEMM, tile mt x nt MFMA tiles per wave on wm x wn waves, nstage-deep ring (fp16 / fp32)
    Wide,         // kernels_conv_wide.hip: the same tiles with one wait + barrier per group of g K-steps, for launches of a few tiles (fp16)
    Pp,           // kernels_conv_pp.hip: v4 ping-pong im2col, one block per CU (long K, Cout 128 / 256k)
    PpPatch,      // kernels_conv_pp.hip: v5 ping-pong patch (3x3 / 1, Cout 128 / 256k), `run` tiles per block
    SpPatch,      // kernels_conv_sp.hip: v6 software-pipelined patch (the shapes of v5 without a second source), `run` tiles per block
    S2Patch,      // kernels_conv_sp.hip: the stride-2 3x3 layers on the space-to-depth view (k_order 3), `run` tiles per block
    Patch,        // kernels_conv_direct.hip: 4-wave 3x3 patch kernel (Cout 32 / 64 / 80), th x tw tiles, K order kord
    PmPatch,      // kernels_conv_direct.hip: pixel-major 3x3 patch, cpp chunks per pixel at an LDS pitch of `pitch`, th x tw tiles
    C16,          // kernels_conv_direct.hip: 3x3 with 16 input channels
    C32s2Tail,    // kernels_conv_direct.hip: 3x3 / 2, 32 -> 64 channels with a.w_tail's 1x1 in its epilogue
    Stream1x1,    // kernels_conv_direct.hip: 1x1, 64 .. 128 -> 64 channels, no LDS (large batch)
    C64Resident,  // kernels_conv_direct.hip: persistent weights-resident 3x3, Cin = Cout = 64, `blocks` blocks
};

// What launch_conv_igemm launches for one layer: the form, its template parameters (0 where it has none) and the launch's shape.
struct ConvPlan {
    ConvForm form = ConvForm::Dma;
    int mt = 0, nt = 0, wm = 0, wn = 0;   // MFMA tiles per wave (pixels, channels), waves per block (pixels, channels)
    int nstage = 0;                       // Dma, Pp, PpPatch: ring depth; Wide: groups of K-steps in the ring
    int th = 0, tw = 0;                   // the patch forms' output tile (rows x columns)
    int cpp = 0, pitch = 0;               // Patch: 16-byte chunks per input pixel; PmPatch: the same and its LDS pitch in chunks
    int kord = 0;                         // Patch: K order it walks (ConvArgs::k_order 0 or 2)
    int g = 0;                            // Wide: K-steps per group
    bool tail = false;                    // the kernel runs a.w_tail's 1x1 in its epilogue
    bool x2 = false;                      // the kernel walks a second source (ConvArgs::x2)
    bool list = false;                    // Dma: the pixel-list form (ConvArgs::pix_list)
    int run = 1;                          // PpPatch, SpPatch, S2Patch: tiles per block
    long blocks = 0;                      // PpPatch, SpPatch, S2Patch, C64Resident: grid size
};

// Row windows (ConvArgs::win_rows): the tile rows a form's launch walks its window in, and whether it stores exactly the window's rows
// (`exact`) or whole tiles.  0: the form has no window and always computes the full map.  The launchers assert these against their
// kernels' tiles; the window planner (Model::row_plan) asks here and nowhere else.
constexpr int kWinTileC16 = 8, kWinTileC32s2Tail = 8, kWinTileC2f16 = 8;
inline int conv_window_tile(const ConvPlan& p, bool& exact) {
    exact = p.form == ConvForm::Patch || p.form == ConvForm::Stream1x1;
    switch (p.form) {
        case ConvForm::C16: return kWinTileC16;
        case ConvForm::C32s2Tail: return kWinTileC32s2Tail;
        case ConvForm::Patch: return p.th;          // conv3x3_patch_kernel drops the rows of its tiles outside the window
        case ConvForm::Stream1x1: return 1;         // conv1x1_stream_kernel walks the window's pixels of every image
        default: return 0;
    }
}

// The K order of a layer (ConvArgs::k_order): a property of its SHAPE, never of the batch, so that every kernel any batch size may
// select accumulates in the same order and embeddings do not depend on the batch.
int conv_k_order(int dtype, const ConvArgs& a);
// The plan for `a` as launch_conv_igemm passes it (k_order set): the first rule of the tree that takes the layer.
ConvPlan plan_conv(int dtype, const ConvArgs& a, int cu_budget);

// What launch_conv_igemm does before it launches: sets a.k_order from the shape, then plans with it.
ConvPlan plan_conv_launch(int dtype, ConvArgs& a, int cu_budget);

// true when launch_conv_igemm can run `lead` with `tail` (a 1x1 / stride 1 / pad 0 conv reading exactly lead's output) in its epilogue:
// fp16, lead = SiLU without residual with Cout 64 or 80 (a wave then owns every channel of its pixels), tail.Cout <= lead.Cout
bool conv_tail_supported(int dtype, const ConvArgs& lead, const ConvArgs& tail);
// true when launch_conv_igemm takes this 1x1 conv with the first cs channels of its input read from a half-resolution tensor (ConvArgs::xs)
bool conv_xs_supported(int dtype, const ConvArgs& a, int cs);
// true when launch_conv_igemm takes a conv of this shape (x2 fields ignored) with a second source (ConvArgs::x2) of cin2 channels
bool conv_x2_supported(int dtype, const ConvArgs& a, int cin2);

// A whole 64-channel BasicBlock (c1: conv3x3 + ReLU, c2: conv3x3 + block input, ReLU) in one fp16 kernel with the intermediate in LDS:
// the images per block when the pair is one it takes (launch_c64_block), 0 otherwise.
int plan_c64_block(const ConvArgs& c1, const ConvArgs& c2, int cu_budget);
// A whole C2f block with 16-channel halves (cv1 1x1 32->32, m.cv1 / m.cv2 3x3 16->16 with shortcut, cv2 1x1 48->32) in one fp16 kernel,
// concat buffer and intermediate in LDS: true when the four convs are wired as engine_file.py's c2f() wires them (launch_c2f16).
bool plan_c2f16(const ConvArgs& cv1, const ConvArgs& m_cv1, const ConvArgs& m_cv2, const ConvArgs& cv2);

}  // namespace aic
