// engine.cpp -- loads an .aicw engine file and runs it: the replacement for TRTEngine
// (src/trt_utils/trt_engine.py:15-216), plus the fused detector / ReID entry points that replace
// YOLODetector.detect (src/detector/yolo_detector.py:68-149) and the crop->embed half of
// DeepSORT.update (src/tracker/deepsort_tracker.py:104-113, src/tracker/reid_model.py:67-126).
//
// Data layout in HBM: every activation is NHWC ([items][h][w][c], c contiguous) in the activation
// dtype (fp16 or fp32); concatenations are channel slices of one buffer; head outputs and
// embeddings are fp32.  Weights are repacked once at load to [cout][kh][kw][cin] with K padded to
// the MFMA K-step and zero rows up to cout_pad, so the conv kernel needs no bounds checks on them.
#include "engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <fstream>

namespace aic {

namespace {

struct Reader {
    const char* p;
    size_t n, off = 0;
    template <class T> const T* take(size_t count) {
        AIC_REQUIRE(off + count * sizeof(T) <= n, AIC_ERR_FORMAT, "engine file truncated");
        const T* r = reinterpret_cast<const T*>(p + off);
        off += count * sizeof(T);
        return r;
    }
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// IEEE fp32 -> fp16 bits, round-to-nearest-even (host side; no dependence on compiler-rt helpers)
inline uint16_t f32_to_f16_bits(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7FFFFFFFu;
    if (x >= 0x7F800000u) return (uint16_t)(sign | (x > 0x7F800000u ? 0x7E00u : 0x7C00u));
    if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);            // rounds to inf
    if (x < 0x33000001u) return (uint16_t)sign;                          // rounds to zero
    int e = (int)(x >> 23) - 127;
    uint32_t m = (x & 0x7FFFFFu) | 0x800000u;
    int shift;
    uint32_t base;
    if (e < -14) { shift = 13 + (-14 - e); base = 0; }                   // subnormal half
    else { shift = 13; base = (uint32_t)(e + 15) << 10; m &= 0x7FFFFFu; }
    uint32_t q = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (q & 1u))) ++q;
    return (uint16_t)(sign | (base + q));
}

}  // namespace

Model::Model(Device& d, const void* blob, size_t nbytes, int dtype_, int max_items_)
    : dev(&d), dtype(dtype_), max_items(max_items_) {
    AIC_REQUIRE(dtype == AIC_F16 || dtype == AIC_F32, AIC_ERR_INVALID, "dtype must be AIC_F16 or AIC_F32");
    AIC_REQUIRE(max_items > 0, AIC_ERR_INVALID, "max_items must be positive");
    d.use();
    blob_copy = std::make_shared<const std::vector<char>>(reinterpret_cast<const char*>(blob), reinterpret_cast<const char*>(blob) + nbytes);
    Reader rd{reinterpret_cast<const char*>(blob), nbytes};
    const uint32_t* head = rd.take<uint32_t>(2);
    AIC_REQUIRE(head[0] == 0x57434941u && head[1] == 1u, AIC_ERR_FORMAT, "not an AICW v1 engine file");
    const int32_t* h = rd.take<int32_t>(15);
    kind = h[0], in_h = h[1], in_w = h[2];
    const int nb = h[3], no = h[4], nw = h[5], nout = h[6];
    for (int i = 0; i < 8; ++i) meta[i] = h[7 + i];
    AIC_REQUIRE((kind == KIND_YOLO || kind == KIND_REID) && nb > 0 && no > 0 && nw >= 0 && nout > 0, AIC_ERR_FORMAT,
                "bad engine header");
    const int32_t* btab = rd.take<int32_t>((size_t)nb * 4);
    const int32_t* otab = rd.take<int32_t>((size_t)no * 20);
    const int64_t* wtab = rd.take<int64_t>((size_t)nw * 6);
    const int32_t* outtab = rd.take<int32_t>((size_t)nout * 8);
    const size_t payload_off = rd.off;
    const float* payload = reinterpret_cast<const float*>(rd.p + payload_off);
    const size_t payload_n = (nbytes - payload_off) / 4;

    const int esz = dtype == AIC_F16 ? 2 : 4;
    const int vec = 16 / esz;
    // ---- activation arena
    bufs.resize(nb);
    storage.resize(nb);
    for (int i = 0; i < nb; ++i) {
        BufDesc& b = bufs[i];
        b.h = btab[i * 4], b.w = btab[i * 4 + 1], b.c = btab[i * 4 + 2], b.f32 = btab[i * 4 + 3];
        AIC_REQUIRE(b.h > 0 && b.w > 0 && b.c > 0, AIC_ERR_FORMAT, "bad buffer shape");
        b.esize = b.f32 ? 4 : esz;
        // whole 16-byte vectors per pixel: every conv reads its input, and the fast epilogues store, in such vectors.  The one exception is
        // a YOLO level's fp32 class tensor: nothing reads it but decode_kernel (scalar arg-max when nc % 4 != 0) and the copies of
        // aic_yolo_head, and a conv whose Cout is no multiple of 4 stores it through the scalar epilogue (epilogue_generic)
        bool cls_out = false;
        for (int o = 0; o < nout && kind == KIND_YOLO; ++o) cls_out = cls_out || outtab[(size_t)o * 8 + 1] == i;
        AIC_REQUIRE(b.c % (16 / b.esize) == 0 || (cls_out && b.f32 && b.c == meta[0]), AIC_ERR_FORMAT,
                    "buffer channel count must be a multiple of 16 bytes");
        b.per_item = (size_t)b.h * b.w * b.c * b.esize;
        storage[i].alloc(b.per_item * max_items + 256);
        HIP_CHECK(hipMemsetAsync(storage[i].p, 0, storage[i].n, d.s_main));
        b.p = storage[i].p;
    }
    AIC_REQUIRE(bufs[0].h == in_h && bufs[0].w == in_w && bufs[0].c == 8, AIC_ERR_FORMAT, "input buffer must be HxWx8");
    d_zero.alloc(256);
    HIP_CHECK(hipMemsetAsync(d_zero.p, 0, 256, d.s_main));
    // ---- ops
    ops.resize(no);
    for (int i = 0; i < no; ++i) std::memcpy(ops[i].v, otab + (size_t)i * 20, 80);
    outs.resize(nout);
    for (int i = 0; i < nout; ++i) std::memcpy(outs[i].v, outtab + (size_t)i * 8, 32);
    // ---- weights: OIHW fp32 -> [cout_pad][Kp] (kh, kw, cin) in the activation dtype
    weights.resize(nw);
    const int bke = 4 * vec;
    // one device weight = the output channels of one or more engine-file weights stacked (a merged conv, below)
    struct WSrc { const float* w; const float* b; int cout; };
    // `second` (one part only): a 1x1 conv of cin2 channels with the same output channels, folded in as K columns behind the window's
    // (ConvArgs::x2); the bias becomes the sum of the two
    auto pack_weights = [&](ConvWeights& w, const std::vector<WSrc>& parts, int cin, int kh, int kw, const WSrc* second = nullptr, int cin2 = 0) {
        w.cout = 0;
        for (const WSrc& p : parts) w.cout += p.cout;
        w.cin = cin, w.kh = kh, w.kw = kw;
        w.cin_eff = w.cin == 3 ? 8 : w.cin;
        AIC_REQUIRE(w.cin_eff % vec == 0, AIC_ERR_FORMAT, "conv input channels must be a multiple of 16 bytes");
        w.cin2 = second ? cin2 : 0;
        w.K = w.kh * w.kw * w.cin_eff + w.cin2;
        w.Kp = round_up(w.K, bke);
        w.cout_pad = round_up(w.cout, 128) + 128;
        // + 8 K-steps of zero slack: the conv kernel's drain iterations step the weight pointer past the last row
        std::vector<char> packed(((size_t)w.cout_pad * w.Kp + 8 * bke) * esz, 0);
        std::vector<float> bias(w.cout_pad, 0.f);
        int co0 = 0;
        for (const WSrc& p : parts) {
            for (int co = 0; co < p.cout; ++co)
                for (int ci = 0; ci < w.cin; ++ci)
                    for (int ky = 0; ky < w.kh; ++ky)
                        for (int kx = 0; kx < w.kw; ++kx) {
                            const float v = p.w[(((size_t)co * w.cin + ci) * w.kh + ky) * w.kw + kx];
                            const size_t k = (size_t)(co0 + co) * w.Kp + (size_t)(ky * w.kw + kx) * w.cin_eff + ci;
                            if (dtype == AIC_F16) reinterpret_cast<uint16_t*>(packed.data())[k] = f32_to_f16_bits(v);
                            else reinterpret_cast<float*>(packed.data())[k] = v;
                        }
            std::copy(p.b, p.b + p.cout, bias.begin() + co0);
            co0 += p.cout;
        }
        if (second) {
            const size_t k0 = (size_t)w.kh * w.kw * w.cin_eff;
            for (int co = 0; co < second->cout; ++co) {
                for (int ci = 0; ci < cin2; ++ci) {
                    const float v = second->w[(size_t)co * cin2 + ci];
                    const size_t k = (size_t)co * w.Kp + k0 + ci;
                    if (dtype == AIC_F16) reinterpret_cast<uint16_t*>(packed.data())[k] = f32_to_f16_bits(v);
                    else reinterpret_cast<float*>(packed.data())[k] = v;
                }
                bias[co] += second->b[co];
            }
        }
        w.w.alloc(packed.size());
        HIP_CHECK(hipMemcpy(w.w.p, packed.data(), packed.size(), hipMemcpyHostToDevice));
        w.bias.alloc(w.cout_pad);
        HIP_CHECK(hipMemcpy(w.bias.p, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    };
    auto wsrc_of = [&](int i) {
        const int cout = (int)wtab[i * 6], cin = (int)wtab[i * 6 + 1], kh = (int)wtab[i * 6 + 2], kw = (int)wtab[i * 6 + 3];
        const size_t woff = (size_t)wtab[i * 6 + 4], boff = (size_t)wtab[i * 6 + 5];
        AIC_REQUIRE(woff + (size_t)cout * cin * kh * kw <= payload_n && boff + cout <= payload_n, AIC_ERR_FORMAT, "weight offsets out of range");
        return WSrc{payload + woff, payload + boff, cout};
    };
    for (int i = 0; i < nw; ++i)
        pack_weights(weights[i], {wsrc_of(i)}, (int)wtab[i * 6 + 1], (int)wtab[i * 6 + 2], (int)wtab[i * 6 + 3]);
    // ---- validate ops against buffers, count FLOPs
    for (const OpDesc& o : ops) {
        const int* v = o.v;
        AIC_REQUIRE(v[1] >= 0 && v[1] < nb && v[4] >= 0 && v[4] < nb, AIC_ERR_FORMAT, "op references a missing buffer");
        const BufDesc& sb = bufs[v[1]];
        const BufDesc& db = bufs[v[4]];
        const int cin_chk = (v[0] == OP_CONV && v[3] == 3) ? 8 : v[3];
        AIC_REQUIRE(v[2] >= 0 && v[2] + cin_chk <= sb.c && v[2] % vec == 0, AIC_ERR_FORMAT, "op source slice out of range");
        if (v[0] == OP_CONV) {
            AIC_REQUIRE(v[15] >= 0 && v[15] < nw, AIC_ERR_FORMAT, "conv references a missing weight");
            const ConvWeights& w = weights[v[15]];
            AIC_REQUIRE(w.cout == v[6] && w.cin == v[3] && w.kh == v[7] && w.kw == v[8], AIC_ERR_FORMAT, "conv/weight shape mismatch");
            AIC_REQUIRE(v[5] >= 0 && v[5] + v[6] <= db.c && v[5] % 4 == 0, AIC_ERR_FORMAT, "conv destination slice out of range");
            AIC_REQUIRE((sb.h + 2 * v[10] - v[7]) / v[9] + 1 == db.h && (sb.w + 2 * v[10] - v[8]) / v[9] + 1 == db.w,
                        AIC_ERR_FORMAT, "conv geometry mismatch");
            AIC_REQUIRE(!sb.f32 || dtype == AIC_F32, AIC_ERR_FORMAT, "conv input must be an activation buffer");
            if (v[14]) {
                AIC_REQUIRE(v[12] >= 0 && v[12] < nb, AIC_ERR_FORMAT, "residual references a missing buffer");
                const BufDesc& rb = bufs[v[12]];
                AIC_REQUIRE(rb.h == db.h && rb.w == db.w && v[13] + v[6] <= rb.c && !rb.f32, AIC_ERR_FORMAT, "residual shape mismatch");
            }
            flops_per_item += 2.0 * db.h * db.w * (double)v[6] * v[3] * v[7] * v[8];
            ++n_convs;
        }
    }
    // ---- fold: a ResNet downsample branch (1x1 / stride s, linear, read only as the residual of the block's last conv) into that conv:
    // relu(conv3x3(t) + b + ds(x) + b') is ONE GEMM over K = [window of t | channels of x] (ConvArgs::x2).  The 1x1's launch goes away and
    // with it its output tensor -- written once, read once, 2 GB per 15 360 crops on ReID layer2 (1.58 ms of downsample launches per
    // 512-frame group, and the 9 us residual epilogue of the three convs that added them).  The sum no longer passes through an fp16
    // rounding of the branch: not bit-identical to the unfolded graph, 8e-5 from it and as far from the fp32 oracle as it is
    // (tests/test_gpu_nets.py::test_downsample_branch_folded_into_last_conv).
    // AICAM_NO_DS_FOLD=1: off.
    if (dtype == AIC_F16 && !getenv("AICAM_NO_DS_FOLD")) {
        for (size_t j = 0; j < ops.size(); ++j) {
            int* c = ops[j].v;
            if (c[0] != OP_CONV || c[14] != 1 || ops[j].fuse || c[15] >= nw || c[13] != 0 || c[16] != 0) continue;
            const int rbuf = c[12];
            size_t i = ops.size();
            for (size_t k = 0; k < j; ++k)
                if (ops[k].v[0] == OP_CONV && ops[k].v[4] == rbuf && !ops[k].fuse) i = k;
            if (i == ops.size()) continue;
            const int* p = ops[i].v;
            if (p[7] != 1 || p[8] != 1 || p[10] != 0 || p[11] != 0 || p[14] != 0 || p[5] != 0 || p[6] != c[6] || p[15] >= nw) continue;
            if (bufs[rbuf].c != c[6] || bufs[rbuf].f32) continue;
            bool clash = false;                         // nobody else reads or writes the branch's tensor; its source is still intact at the last conv
            for (size_t k = 0; k < ops.size(); ++k) {
                const int* u = ops[k].v;
                if (k != i && u[4] == rbuf) clash = true;
                if (u[1] == rbuf || (k != j && u[0] == OP_CONV && u[14] && u[12] == rbuf)) clash = true;
                if (k > i && k <= j && u[4] == p[1]) clash = true;
            }
            for (auto& o : outs)
                if (o.v[0] == rbuf) clash = true;
            if (clash) continue;
            const BufDesc& xb = bufs[c[1]];
            const BufDesc& yb = bufs[c[4]];
            ConvArgs q{};
            q.H = xb.h, q.W = xb.w, q.Cin = c[3], q.Ho = yb.h, q.Wo = yb.w, q.Cout = c[6], q.KH = c[7], q.KW = c[8], q.stride = c[9], q.pad = c[10];
            q.out_f32 = yb.f32;
            if (!conv_x2_supported(dtype, q, p[3])) continue;
            const WSrc second = wsrc_of(p[15]);
            weights.emplace_back();
            pack_weights(weights.back(), {wsrc_of(c[15])}, c[3], c[7], c[8], &second, p[3]);
            c[15] = (int)weights.size() - 1;
            c[14] = 0, c[12] = 0, c[13] = 0;            // no residual any more
            c[16] = p[1] + 1, c[17] = p[2], c[18] = p[3], c[19] = p[9];
            ops[i].fuse = 2;                            // absorbed: run_range skips it
            storage[rbuf].release();
            bufs[rbuf].p = nullptr;
        }
    }
    // ---- fold: a 2x nearest-neighbour upsample whose output slice is read by exactly one 1x1 conv, as the FIRST channels of its input
    // (YOLOv8's neck: up(P5) | P4 -> 12.c2f.cv1, up(12) | P3 -> 15.c2f.cv1), into that conv: it reads those channels from the
    // half-resolution tensor at (y >> 1, x >> 1) (ConvArgs::xs).  Same values in the same K order: bit-identical
    // (tests/test_gpu_nets.py::test_upsample_folded_into_its_reader).  AICAM_NO_UP_FOLD=1: off.
    if (!getenv("AICAM_NO_UP_FOLD")) {
        auto overlap = [](int a0, int an, int b0, int bn) { return a0 < b0 + bn && b0 < a0 + an; };
        for (size_t i = 0; i < ops.size(); ++i) {
            const int* u = ops[i].v;
            if (u[0] != OP_UPSAMPLE2X || ops[i].fuse) continue;
            const int S = u[1], sc = u[2], c = u[3], D = u[4], dc = u[5];
            size_t j = ops.size();
            bool clash = false;
            for (size_t k = 0; k < ops.size(); ++k) {
                if (k == i || ops[k].fuse == 2) continue;
                const int* w = ops[k].v;
                const bool reads = w[1] == D && overlap(w[2], w[0] == OP_CONV && w[3] == 3 ? 8 : w[3], dc, c);
                if (reads) {
                    if (j != ops.size() || k < i) clash = true;
                    j = k;
                }
                if (w[0] == OP_CONV && w[14] && w[12] == D && overlap(w[13], w[6], dc, c)) clash = true;
                if (w[4] == D && overlap(w[5], w[6], dc, c)) clash = true;                      // another writer of the slice
            }
            for (auto& o : outs)
                if (o.v[0] == D || (kind == KIND_YOLO && o.v[1] == D)) clash = true;
            if (clash || j == ops.size()) continue;
            int* v = ops[j].v;
            if (v[0] != OP_CONV || ops[j].fuse || v[2] != dc || v[3] <= c || v[16] != 0 || v[15] >= (int)weights.size()) continue;
            for (size_t k = i + 1; k <= j; ++k)                                                  // the low-resolution source is still intact at the reader
                if (ops[k].fuse != 2 && ops[k].v[4] == S && overlap(ops[k].v[5], ops[k].v[6], sc, c)) clash = true;
            if (clash) continue;
            const BufDesc& xb = bufs[v[1]];
            const BufDesc& yb = bufs[v[4]];
            const ConvWeights& w = weights[v[15]];
            ConvArgs q{};
            q.H = xb.h, q.W = xb.w, q.Cin = w.cin_eff, q.Ho = yb.h, q.Wo = yb.w, q.Cout = v[6], q.KH = v[7], q.KW = v[8], q.stride = v[9], q.pad = v[10];
            q.Kp = w.Kp, q.out_f32 = yb.f32;
            if (2 * bufs[S].h != xb.h || 2 * bufs[S].w != xb.w || !conv_xs_supported(dtype, q, c)) continue;
            // (a conv that takes the next 1x1 into its epilogue -- fuse 3, marked below -- is launched with a tail; the marking skips
            // every conv with a split source, and conv_tail_supported() refuses one as well)
            ops[j].xs_buf = S, ops[j].xs_coff = sc, ops[j].xs_c = c;
            ops[i].fuse = 2;                            // absorbed: run_range skips it
        }
    }
    // ---- merge: two convs that read the SAME tensor slice with the same window, stride, padding and activation and no residual
    // (YOLOv8's detect branches: 22.box{l}.0 and 22.cls{l}.0 both start from the level's feature map) become ONE conv whose output
    // channels are the two sets side by side in one new buffer; their readers take channel slices of it.  The map is read once
    // instead of twice and the GEMM is 144 wide instead of 64 and 80 (levels with maps up to 40 x 40, see below).  Per output channel nothing changes (same K order, same
    // epilogue): the head is bit-identical (tests/test_gpu_nets.py::test_merged_detect_branch_heads).  AICAM_NO_MERGE=1: off.
    if (dtype == AIC_F16 && !getenv("AICAM_NO_MERGE")) {
        for (size_t i = 0; i < ops.size(); ++i) {
            int* c = ops[i].v;
            if (c[0] != OP_CONV || c[14] != 0 || ops[i].fuse || c[15] >= nw) continue;
            for (size_t j = i + 1; j < ops.size() && j <= i + 8; ++j) {
                int* p = ops[j].v;
                if (p[0] != OP_CONV || p[14] != 0 || ops[j].fuse || p[15] >= nw) continue;
                bool same = p[1] == c[1] && p[2] == c[2] && p[3] == c[3];
                for (int k = 7; k <= 11; ++k) same = same && p[k] == c[k];
                const int di = c[4], dj = p[4];
                if (!same || di == dj || c[5] != 0 || p[5] != 0 || c[7] != 3) continue;
                const BufDesc bi = bufs[di], bj = bufs[dj];
                if (bi.f32 || bj.f32 || bi.c != c[6] || bj.c != p[6] || bi.h != bj.h || bi.w != bj.w || (c[6] % vec) || (p[6] % vec)) continue;
                // maps up to 40 x 40 only (measured, profiles/r03: on the 80 x 80 level the 64-channel conv has the 3x3 patch kernel at
                // 645 TFLOP/s and the 144-wide 4-wave tile reaches 470: 1 157 us merged against 633 + 374; on the 40 x 40 and 20 x 20
                // levels the merged conv wins, 490 against 513 us and 233 against 286)
                static const int merge_px = [] { const char* e = getenv("AICAM_MERGE_MAXPX"); return e ? atoi(e) : 1600; }();
                if (bi.h * bi.w > merge_px) continue;
                bool clash = false;                     // the second conv now runs at the first one's place: nobody may touch its output in between,
                for (size_t k = 0; k < ops.size(); ++k) {   // and nobody else may write either buffer
                    const int* u = ops[k].v;
                    if (k != i && k != j && (u[4] == di || u[4] == dj)) clash = true;
                    if (k > i && k < j && (u[1] == dj || (u[0] == OP_CONV && u[14] && u[12] == dj))) clash = true;
                }
                for (auto& o : outs)
                    if (o.v[0] == di || o.v[0] == dj || (kind == KIND_YOLO && (o.v[1] == di || o.v[1] == dj))) clash = true;
                if (clash) continue;
                // new buffer and weight
                BufDesc nb = bi;
                nb.c = c[6] + p[6];
                nb.per_item = (size_t)nb.h * nb.w * nb.c * nb.esize;
                storage.emplace_back();
                storage.back().alloc(nb.per_item * max_items + 256);
                HIP_CHECK(hipMemsetAsync(storage.back().p, 0, storage.back().n, d.s_main));
                nb.p = storage.back().p;
                bufs.push_back(nb);
                const int m = (int)bufs.size() - 1;
                weights.emplace_back();
                pack_weights(weights.back(), {wsrc_of(c[15]), wsrc_of(p[15])}, c[3], c[7], c[8]);
                const int ci_out = c[6];
                for (auto& o : ops) {                   // readers of either output: slices of the merged buffer
                    int* u = o.v;
                    if (u[1] == di) u[1] = m;
                    else if (u[1] == dj) { u[1] = m; u[2] += ci_out; }
                    if (u[0] == OP_CONV && u[14]) {
                        if (u[12] == di) u[12] = m;
                        else if (u[12] == dj) { u[12] = m; u[13] += ci_out; }
                    }
                }
                c[4] = m, c[5] = 0, c[6] = nb.c, c[15] = (int)weights.size() - 1;
                ops[j].fuse = 2;                        // absorbed: run_range skips it
                storage[di].release(), storage[dj].release();      // (nobody reads the two old buffers any more)
                bufs[di].p = bufs[dj].p = nullptr;
                break;
            }
        }
    }
    // ---- fusion: conv3x3/1 (3->64)+ReLU followed by max-pool 3x3/2 of exactly that tensor (ReID stem)
    if (dtype == AIC_F16) {
        for (size_t i = 0; i + 1 < ops.size(); ++i) {
            const int* c = ops[i].v;
            const int* p = ops[i + 1].v;
            if (c[0] != OP_CONV || p[0] != OP_MAXPOOL3S2) continue;
            const BufDesc& cb = bufs[c[4]];
            const bool conv_ok = c[3] == 3 && c[6] == 64 && c[7] == 3 && c[8] == 3 && c[9] == 1 && c[10] == 1 && c[11] == 2 &&
                                 c[14] == 0 && c[5] == 0 && cb.c == 64 && !cb.f32 && cb.w == 64 && cb.h % 8 == 0 && c[2] == 0;
            const bool pool_ok = p[1] == c[4] && p[2] == 0 && p[3] == 64 && !bufs[p[4]].f32;
            bool other_reader = false;
            for (size_t j = 0; j < ops.size(); ++j)
                if (j != i + 1 && (ops[j].v[1] == c[4] || (ops[j].v[0] == OP_CONV && ops[j].v[14] && ops[j].v[12] == c[4]))) other_reader = true;
            if (conv_ok && pool_ok && !other_reader) { ops[i].fuse = 1; ops[i + 1].fuse = 2; }
        }
    }
    // ---- fusion: a SiLU conv with 64 or 80 output channels whose output feeds exactly one 1x1/1/0 conv and nothing else (YOLOv8's
    // detect branches: 22.box*.1 -> .2, 22.cls*.1 -> .2).  The 1x1 runs in the first conv's epilogue on the tile in registers;
    // the intermediate tensor is never written.  Marked here (graph properties); run_range() asks conv_tail_supported() for the rest.
    if (dtype == AIC_F16) {
        for (size_t i = 0; i + 1 < ops.size(); ++i) {
            const int* c = ops[i].v;
            const int* p = ops[i + 1].v;
            if (c[0] != OP_CONV || p[0] != OP_CONV || ops[i].fuse || ops[i + 1].fuse) continue;
            // a lead with a split source (folded upsample) or a second source (folded downsample) has no tail form: the tail kernels would
            // ignore that source and read channels nobody wrote
            if (ops[i].xs_buf >= 0 || c[16] != 0) continue;
            const bool lead_ok = (c[6] == 64 || c[6] == 80) && c[11] == 1 && c[14] == 0 && !bufs[c[4]].f32;
            const bool tail_ok = p[7] == 1 && p[8] == 1 && p[9] == 1 && p[10] == 0 && p[14] == 0 && p[1] == c[4] && p[2] == c[5] &&
                                 p[3] == c[6] && p[6] <= c[6];
            if (!lead_ok || !tail_ok) continue;
            bool other_reader = false;
            for (size_t j = 0; j < ops.size(); ++j)
                if (j != i + 1 && (ops[j].v[1] == c[4] || (ops[j].v[0] == OP_CONV && ops[j].v[14] && ops[j].v[12] == c[4]))) other_reader = true;
            for (auto& o : outs)
                if (o.v[0] == c[4] || (kind == KIND_YOLO && o.v[1] == c[4])) other_reader = true;
            if (!other_reader) ops[i].fuse = 3;          // the follower keeps fuse = 0: it runs on its own whenever the lead cannot take it
        }
    }
    if (kind == KIND_YOLO) {
        AIC_REQUIRE(nout <= 4, AIC_ERR_FORMAT, "at most 4 detection levels");
        n_anchors = 0;
        for (auto& o : outs) n_anchors += o.v[3] * o.v[4];
        out_dim = meta[0];
        max_det_cap = 1024;
        const size_t ba = (size_t)max_items * n_anchors;
        d_boxes.alloc(ba * 4), d_maxlogit.alloc(ba), d_labels.alloc(ba);
        d_ncand.alloc(max_items), d_numdets.alloc(max_items);
        d_out_boxes.alloc((size_t)max_items * max_det_cap * 4), d_out_boxes_orig.alloc((size_t)max_items * max_det_cap * 4);
        d_out_scores.alloc((size_t)max_items * max_det_cap), d_out_labels.alloc((size_t)max_items * max_det_cap);
        plan_sparse_box();
        if (sbx.ok) {                           // every list holds a whole map: no count can overflow one
            for (int l = 0; l < 4; ++l) d_sp_list[l].alloc((size_t)max_items * outs[l % 3].v[3] * outs[l % 3].v[4]);
            d_sp_count.alloc(4), h_sp_count.alloc(4);
            HIP_CHECK(hipMemsetAsync(d_sp_count.p, 0, 16, d.s_main));
            HIP_CHECK(hipEventCreateWithFlags(&sp_ev, hipEventDisableTiming));
            sp_force = getenv("AICAM_SPARSE_BOX_FORCE") != nullptr;
        }
    } else {
        out_dim = outs[0].v[1];
        AIC_REQUIRE(bufs[outs[0].v[0]].f32, AIC_ERR_FORMAT, "embedding buffer must be fp32");
    }
    plan_side_heads();
    HIP_CHECK(hipStreamSynchronize(d.s_main));
}

Model::~Model() {
    if (sp_ev) (void)hipEventDestroy(sp_ev);
    for (int i = 0; i < 2; ++i) {
        if (side_fork[i]) (void)hipEventDestroy(side_fork[i]);
        if (side_join[i]) (void)hipEventDestroy(side_join[i]);
    }
}

// The launches a run may list (engine.hpp, SparseBox): graph properties only, asked once at load time.
void Model::plan_sparse_box() {
    sbx = SparseBox{};
    if (kind != KIND_YOLO || dtype != AIC_F16 || outs.size() != 3 || meta[1] != 16) return;
    for (int l = 0; l < 3; ++l) {
        for (size_t i = 0; i + 1 < ops.size(); ++i) {
            if (ops[i].fuse != 3 || ops[i + 1].v[0] != OP_CONV) continue;
            if (ops[i + 1].v[4] == outs[l].v[0]) sbx.box_tail[l] = (int)i;
            if (ops[i + 1].v[4] == outs[l].v[1]) sbx.cls_tail[l] = (int)i;
        }
        if (sbx.box_tail[l] < 0 || sbx.cls_tail[l] < 0) return;
    }
    // level 0's lead: the conv that writes exactly the slice 22.box0.1 reads -- 3x3 / 1 / 1 SiLU, 64 channels, nothing folded into it --
    // into a buffer nobody else reads or writes (levels whose first convs were merged into one 144-channel launch have no such op)
    const int* t = ops[sbx.box_tail[0]].v;
    const int buf = t[1];
    int lead = -1;
    for (int k = 0; k < sbx.box_tail[0]; ++k) {
        const int* u = ops[k].v;
        if (u[0] == OP_CONV && ops[k].fuse == 0 && u[4] == buf && u[5] == t[2] && u[6] == t[3] && u[6] == 64 && u[7] == 3 && u[8] == 3 && u[9] == 1 &&
            u[10] == 1 && u[11] == 1 && u[14] == 0 && u[16] == 0 && ops[k].xs_buf < 0 && u[3] % 32 == 0 && !bufs[buf].f32 && bufs[buf].c == 64)
            lead = k;
    }
    for (size_t j = 0; j < ops.size() && lead >= 0; ++j) {
        const int* u = ops[j].v;
        if (ops[j].fuse == 2) continue;
        if ((int)j != lead && u[4] == buf) lead = -1;
        else if ((int)j != sbx.box_tail[0] && (u[1] == buf || (u[0] == OP_CONV && u[14] && u[12] == buf) || ops[j].xs_buf == buf || (u[0] == OP_CONV && u[16] - 1 == buf))) lead = -1;
    }
    for (auto& o : outs)
        if (o.v[0] == buf || o.v[1] == buf) lead = -1;
    sbx.lead0 = lead;
    sbx.ok = true;
}

// Whether this run can list its box branches (engine.hpp): the switch, the arming, and what conv_step plans for the six branches at n.
bool Model::sp_eligible(size_t op0, int n) {
    static const bool off = getenv("AICAM_NO_SPARSE_BOX") != nullptr;      // the dense head, always: A/B runs, the reference of the equality tests
    if (off || !sbx.ok || !reduce_cls || dtype != AIC_F16) return false;
    int first = sbx.lead0 >= 0 ? sbx.lead0 : (int)ops.size();
    for (int l = 0; l < 3; ++l) first = std::min(first, std::min(sbx.box_tail[l], sbx.cls_tail[l]));
    if ((int)op0 > first) return false;
    for (int l = 0; l < 3; ++l) {
        sp_steps[l] = conv_step((size_t)sbx.box_tail[l], ops.size(), n);
        if (sp_steps[l].kind != ConvStep::Tail || sp_steps[l].box_bits != (1u << l) || sp_steps[l].cls_bits) return false;   // the box tail decodes in place (t_box)
        const ConvStep c = conv_step((size_t)sbx.cls_tail[l], ops.size(), n);
        if (c.kind != ConvStep::Tail || c.cls_bits != (1u << l)) return false;                                               // the max logits come from the class tails
        if (rb_now && (rb_now->win[sbx.box_tail[l]].rows > 0 || rb_now->win[sbx.cls_tail[l]].rows > 0)) return false;
    }
    if (sbx.lead0 >= 0) {
        sp_steps[3] = conv_step((size_t)sbx.lead0, (size_t)sbx.lead0 + 1, n);
        if (sp_steps[3].kind != ConvStep::Single || (rb_now && rb_now->win[sbx.lead0].rows > 0)) return false;
    }
    return true;
}

// The candidate pass at `thr` over n frames and, with `lists`, the launches run_ops left out, on its lists (engine.hpp).
void Model::sparse_box_pass(int n, float thr, bool lists, const int* n_dev, hipStream_t s) {
    BoxListArgs b{};
    b.max_logit = d_maxlogit.p, b.logit_thr = thr, b.batch = n, b.n_anchors = n_anchors, b.n_dev = n_dev, b.count = d_sp_count.p;
    int a0 = 0;
    for (int l = 0; l < 3; ++l) {
        b.h[l] = outs[l].v[3], b.w[l] = outs[l].v[4], b.a0[l] = a0;
        a0 += b.h[l] * b.w[l];
    }
    for (int l = 0; l < 4; ++l) b.list[l] = d_sp_list[l].p;
    {
        Prof pr(*dev, PROF_DET, s, 0, (double)n * n_anchors * 4);
        launch_box_candidates(b, s);
    }
    sp_pass = true, sp_thr = thr, sp_n = n;
    if (!lists) return;
    const bool prof_conv = (dev->prof_mask >> PROF_CONV) & 1u;
    if (prof_conv) dev->prof_begin(PROF_CONV, s, 0, 0);
    try {
        for (int k = sbx.lead0 >= 0 ? 3 : 0; ; k = k == 3 ? 0 : k + 1) {      // level 0's lead on the neighbour list, then the three tail pairs
            ConvArgs a = sp_steps[k].a[0];
            a.pix_list = d_sp_list[k].p, a.pix_count = d_sp_count.p + k, a.n_dev = n_dev;
            // accounted with the last counts read back (what ran, never the dense layer's FLOPs); nothing known yet: nothing
            const double share = sp_known_n > 0 ? std::min(1.0, (double)sp_known[k] / ((double)sp_known_n * a.Ho * a.Wo)) : 0.0;
            if (prof_conv) dev->prof_account(PROF_CONV, sp_steps[k].fl * share, sp_steps[k].by * share);
            launch_conv_igemm(dtype, a, s);
            if (k == 2) break;
        }
    } catch (...) {
        if (prof_conv) dev->prof_end(PROF_CONV, s);
        throw;
    }
    if (prof_conv) dev->prof_end(PROF_CONV, s);
    box_decoded |= 7u;
    sp_listed = true;
}

// Which ops may leave the main stream (engine.hpp, side_heads).  An op's slices: what it reads (source, residual, second source, split
// source) and the one it writes, as (buffer, first channel, channels); elementwise ops count with their whole buffers.  Level l's set =
// the live ops from which output l and no other output is reachable through those slices; it has to be ONE run of consecutive live ops,
// its fork point `cut` = one past the last op outside the set that writes something the set reads, and nothing that can run beside it
// (any op at or behind `cut` outside the set) may write what the set reads or writes, or read what it writes.  Anything else: no plan.
void Model::plan_side_heads() {
    side_heads.clear();
    static const int opt = [] { const char* e = getenv("AICAM_SIDE_HEADS"); return e ? atoi(e) : 2; }();
    side_max_items = opt;
    if (kind != KIND_YOLO || opt <= 0 || outs.size() < 2) return;
    struct Slice { int buf, c0, cn; };
    const size_t no = ops.size();
    std::vector<std::vector<Slice>> rd(no);
    std::vector<Slice> wr(no);
    auto whole = [&](int b) { return Slice{b, 0, 1 << 30}; };
    for (size_t i = 0; i < no; ++i) {
        const OpDesc& o = ops[i];
        const int* v = o.v;
        if (o.fuse == 2) continue;
        if (o.fuse == 1) return;                          // (a fused stem + pool: not a detector)
        if (v[0] == OP_CONV) {
            rd[i].push_back(Slice{v[1], v[2], v[3] == 3 ? 8 : v[3]});
            if (v[14]) rd[i].push_back(Slice{v[12], v[13], v[6]});
            if (v[16]) rd[i].push_back(Slice{v[16] - 1, v[17], v[18]});
            if (o.xs_buf >= 0) rd[i].push_back(Slice{o.xs_buf, o.xs_coff, o.xs_c});
            wr[i] = Slice{v[4], v[5], v[6]};
        } else {
            rd[i].push_back(whole(v[1]));
            wr[i] = whole(v[4]);
        }
    }
    auto hit = [](const Slice& a, const Slice& b) { return a.buf == b.buf && a.c0 < b.c0 + b.cn && b.c0 < a.c0 + a.cn; };
    auto live = [&](size_t i) { return ops[i].fuse != 2; };
    // levels reachable from each op (backwards over the list: a later reader of what an op writes)
    std::vector<unsigned> reach(no, 0u);
    for (size_t ii = no; ii-- > 0;) {
        if (!live(ii)) continue;
        for (size_t l = 0; l < outs.size(); ++l)
            if (wr[ii].buf == outs[l].v[0] || wr[ii].buf == outs[l].v[1]) reach[ii] |= 1u << l;
        for (size_t j = ii + 1; j < no; ++j) {
            if (!live(j)) continue;
            for (const Slice& r : rd[j])
                if (hit(r, wr[ii])) reach[ii] |= reach[j];
        }
    }
    for (size_t l = 0; l + 1 < outs.size() && side_heads.size() < 2; ++l) {
        size_t a = no, b = 0;
        for (size_t i = 0; i < no; ++i)
            if (live(i) && reach[i] == (1u << l)) { a = std::min(a, i); b = std::max(b, i + 1); }
        if (a >= b) continue;
        bool ok = true;
        for (size_t i = a; i < b; ++i)
            if (live(i) && reach[i] != (1u << l)) ok = false;             // one run of consecutive live ops
        size_t cut = 0;
        for (size_t i = a; i < b && ok; ++i) {
            if (!live(i)) continue;
            for (size_t k = 0; k < a; ++k) {
                if (!live(k)) continue;
                for (const Slice& r : rd[i])
                    if (hit(r, wr[k])) cut = std::max(cut, k + 1);
            }
        }
        if (!ok || cut == 0 || cut > a) continue;
        if (ops[cut - 1].fuse == 3) continue;                             // (never between a lead and the 1x1 it may take as its tail)
        for (size_t k = cut; k < no && ok; ++k) {                         // whoever may run beside the set
            if (!live(k) || (k >= a && k < b)) continue;
            for (size_t i = a; i < b && ok; ++i) {
                if (!live(i)) continue;
                if (hit(wr[k], wr[i])) ok = false;
                for (const Slice& r : rd[i])
                    if (hit(r, wr[k])) ok = false;
                for (const Slice& r : rd[k])
                    if (hit(r, wr[i])) ok = false;
            }
        }
        if (!ok) continue;
        if (!side_heads.empty() && (cut < side_heads.back().cut || a < side_heads.back().b || cut > side_heads[0].a)) continue;   // forks and sets in list order, every fork in front of every set
        side_heads.push_back(SideHead{a, b, cut});
    }
    if (getenv("AICAM_SIDE_DBG"))
        for (const SideHead& h : side_heads) fprintf(stderr, "[aicam] side head: ops [%zu, %zu) of %zu fork behind op %zu\n", h.a, h.b, no, h.cut);
    for (size_t i = 0; i < side_heads.size(); ++i) {
        side_stream[i] = i == 0 ? dev->s_det : dev->s_reid;
        HIP_CHECK(hipEventCreateWithFlags(&side_fork[i], hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&side_join[i], hipEventDisableTiming));
    }
}

void Model::run_ops(size_t op0, int n, hipStream_t s) {
    const bool prof_conv = (dev->prof_mask >> PROF_CONV) & 1u;            // the HIP-event brackets describe one stream: measured runs stay on it
    const bool one_stream = !side_ok || side_heads.empty() || n > side_max_items || prof_conv || n_items_dev || op0 > side_heads[0].cut || s != dev->s_main;
    // ---- sparse box branches (engine.hpp).  The arming holds for this run only; what the last run listed is void from here on
    const bool armed = sp_armed;
    const float thr = sp_arm_thr;
    sp_armed = sp_pass = sp_listed = false;
    last_n = n;
    if (armed && sp_eligible(op0, n)) {
        if (sp_ev_pending) {                                              // the counts of the last decoded run, if they have arrived
            // (the very first ones are waited for, once per engine: the second launch of a stream of frames already knows its path)
            if ((sp_known_n > 0 ? hipEventQuery(sp_ev) : hipEventSynchronize(sp_ev)) == hipSuccess) {
                std::copy(h_sp_count.p, h_sp_count.p + 4, sp_known);
                sp_known_n = sp_ev_n, sp_ev_pending = false;
            } else {
                (void)hipGetLastError();                                  // (not ready is no error)
            }
        }
        // Which path: time only, both give the same bits.  Large launches whose last known counts leave every list at most a quarter of
        // its map: the lead runs on the neighbour list, so level 0 breaks even where that list is the 6 400-pixel map, and a quarter leaves
        // room for the gathered rows costing more per pixel than the direct forms' tiles.  For isolated candidates, 9 listed pixels each,
        // that is ~170 candidates per frame; a trained detector's candidates cluster (the bench: 278 per frame in 762 pixels).  No counts
        // yet: dense.  Seeded heads list thousands of candidates per frame and stay dense
        const bool big = n >= 32 && one_stream;
        bool few = sp_known_n > 0;
        for (int k = 0; k < 4 && few; ++k) few = 4l * sp_known[k] <= (long)sp_known_n * outs[k % 3].v[3] * outs[k % 3].v[4];
        static const bool dbg = getenv("AICAM_SPARSE_DBG") != nullptr;
        if (dbg)
            fprintf(stderr, "[aicam] sparse box: n %d, last counts %d %d %d + %d neighbours over %d frames -> %s\n", n, sp_known[0], sp_known[1], sp_known[2],
                    sp_known[3], sp_known_n, sp_force || (big && few) ? "lists" : "dense");
        if (sp_force || (big && few)) {
            sp_skip.assign(ops.size(), 0);
            for (int l = 0; l < 3; ++l) sp_skip[sbx.box_tail[l]] = sp_skip[sbx.box_tail[l] + 1] = 1;
            if (sbx.lead0 >= 0) sp_skip[sbx.lead0] = 1;
            try {
                run_range(op0, ops.size(), n, s);
            } catch (...) {
                sp_skip.clear();
                throw;
            }
            sp_skip.clear();
            sparse_box_pass(n, thr, true, n_items_dev, s);
            return;
        }
        // dense, and counted for the next launch -- every launch until counts are known, then every 16th: a head that lists thousands of
        // candidates per frame (seeded weights) pays for the pass and gets nothing back
        if (big && (sp_known_n == 0 || ++sp_dense_runs % 16 == 0)) {
            run_range(op0, ops.size(), n, s);
            sparse_box_pass(n, thr, false, n_items_dev, s);
            return;
        }
    }
    if (one_stream) {
        run_range(op0, ops.size(), n, s);
        return;
    }
    size_t at = op0;
    try {
    for (size_t i = 0; i < side_heads.size(); ++i) {                      // main stream up to each fork, the level's ops behind it on their stream
        const SideHead& h = side_heads[i];
        run_range(at, h.cut, n, s);
        at = h.cut;
        HIP_CHECK(hipEventRecord(side_fork[i], s));
        HIP_CHECK(hipStreamWaitEvent(side_stream[i], side_fork[i], 0));
        run_range(h.a, h.b, n, side_stream[i]);
        HIP_CHECK(hipEventRecord(side_join[i], side_stream[i]));
    }
    for (size_t i = 0; i <= side_heads.size(); ++i) {                     // the rest of the list, around the sets
        const size_t e = i < side_heads.size() ? side_heads[i].a : ops.size();
        if (at < e) run_range(at, e, n, s);
        if (i < side_heads.size()) at = std::max(at, side_heads[i].b);
    }
    for (size_t i = 0; i < side_heads.size(); ++i) HIP_CHECK(hipStreamWaitEvent(s, side_join[i], 0));
    } catch (...) {                                                       // a launch failed between a fork and its join: nothing of this call may still run when the next one starts
        for (size_t i = 0; i < side_heads.size(); ++i) (void)hipStreamSynchronize(side_stream[i]);
        (void)hipStreamSynchronize(s);
        throw;
    }
}

bool Model::input_pix4_ok() const {
    return kind == KIND_REID && dtype == AIC_F16 && !ops.empty() && ops[0].fuse == 1 && reid_stem2_usable(in_h, in_w);
}

void Model::run(int n, hipStream_t s) {
    AIC_REQUIRE(n >= 0 && n <= max_items, AIC_ERR_CAPACITY, "batch exceeds the engine's max_items");
    if (n == 0) return;
    cls_reduced = box_decoded = 0;
    rb_slots = 0;                                   // whoever filled input() wrote anything: no row of any map is known any more
    std::fill(rb_ran.begin(), rb_ran.end(), 0);
    run_ops(0, n, s);
}

// ---- row bands (engine.hpp, row_band.hpp)
std::vector<RowBand> Model::plan_bands(const LetterboxGeom& g) const {
    std::vector<RbOp> ro(ops.size());
    std::vector<int> bh(bufs.size());
    for (size_t i = 0; i < bufs.size(); ++i) bh[i] = bufs[i].h;
    for (size_t i = 0; i < ops.size(); ++i) {
        const OpDesc& o = ops[i];
        const int* v = o.v;
        RbOp& r = ro[i];
        r.src = v[1], r.src_c0 = v[2], r.src_cn = v[0] == OP_CONV && v[3] == 3 ? 8 : v[3];
        r.dst = v[4], r.dst_c0 = v[5], r.dst_cn = v[0] == OP_SPPF_POOL ? 3 * v[6] : v[6];      // (the SPPF pool writes its three copies side by side)
        r.conv = dtype == AIC_F16 && v[0] == OP_CONV && (o.fuse == 0 || o.fuse == 3) && o.xs_buf < 0 && v[16] == 0 && v[7] == v[8] &&
                 !bufs[v[1]].f32 && !bufs[v[4]].f32;
        r.k = v[7], r.stride = v[9], r.pad = v[10];
        if (v[0] == OP_CONV && v[14]) r.res = v[12], r.res_c0 = v[13];
    }
    const bool side_pad = g.left != 0 || g.unpad_w != g.out_w || g.out_h != in_h;
    return plan_row_bands(ro, bh, g.top, g.unpad_h, side_pad);
}

const Model::RowPlan& Model::row_plan(const LetterboxGeom& g, int n) {
    for (const RowPlan& p : row_plans)
        if (p.top == g.top && p.unpad_h == g.unpad_h && p.n == n && p.cu == conv_cu_budget() && p.n_dev == (n_items_dev != nullptr)) return p;
    RowPlan p;
    p.top = g.top, p.unpad_h = g.unpad_h, p.n = n, p.cu = conv_cu_budget(), p.n_dev = n_items_dev != nullptr;
    const size_t no = ops.size();
    p.bands = plan_bands(g);
    p.win.assign(no, RowWindow{}), p.n_ops.assign(no, 0), p.frac.assign(no, 1.f), p.covered.assign(no, 0), p.th.assign(no, 0), p.exact.assign(no, 0);
    // the launches of run_range(1, end) behind the fused stem, as the window planner sees them
    std::vector<RbStep> steps;
    std::vector<size_t> first;
    std::vector<std::vector<int>> step_sig;                           // per step: what it launches (kind, ops, the conv plan)
    constexpr int all_ch = 1 << 30;
    auto read_all = [&](int buf) { RbRead r; r.buf = buf, r.c0 = 0, r.cn = all_ch, r.all = true; return r; };
    {
        RbStep st;                                                    // the stem: reads the frames
        st.op = 0, st.dst = ops[0].v[4], st.dst_c0 = ops[0].v[5], st.dst_cn = ops[0].v[6], st.Ho = bufs[ops[0].v[4]].h, st.th = 8;
        steps.push_back(st), first.push_back(0), step_sig.push_back({0, 1});
        p.n_ops[0] = 1;
    }
    for (size_t oi = 1; oi < no; ++oi) {
        const OpDesc& o = ops[oi];
        if (o.fuse == 2) continue;
        RbStep st;
        int n_ops = 1;
        std::vector<int> sg{(int)oi, -1};
        if (o.v[0] != OP_CONV || o.fuse == 1) {
            st.op = (int)oi, st.dst = o.v[4], st.dst_c0 = o.v[5], st.dst_cn = o.v[0] == OP_SPPF_POOL ? 3 * o.v[6] : o.v[6], st.Ho = bufs[o.v[4]].h;
            st.reads.push_back(read_all(o.v[1]));
        } else {
            const ConvStep cs = conv_step(oi, no, n);
            n_ops = cs.n_ops;
            sg = {(int)oi, cs.kind, cs.n_ops, cs.ipb};
            const OpDesc& last = ops[oi + n_ops - 1];
            st.op = (int)(oi + n_ops - 1), st.dst = last.v[4], st.dst_c0 = last.v[5], st.dst_cn = last.v[6], st.Ho = bufs[last.v[4]].h;
            const ConvArgs& a = cs.a[0];
            RbRead r;
            r.buf = o.v[1], r.c0 = o.v[2], r.cn = a.Cin, r.stride = a.stride, r.halo_lo = a.pad, r.halo_hi = a.KH - 1 - a.pad;
            if (cs.kind == ConvStep::C2f16) {
                st.th = kWinTileC2f16, r.halo_lo = r.halo_hi = 2;     // cv1's input under the two 3x3 convs of the bottleneck
            } else if (cs.kind == ConvStep::Single || cs.kind == ConvStep::Tail) {
                ConvArgs b = a;
                const ConvPlan cp = plan_conv_launch(dtype, b, conv_cu_budget());
                st.th = conv_window_tile(cp, st.exact);
                if (a.xs || a.x2 || a.n_dev || a.out_f32) st.th = 0;
                for (int f : {(int)cp.form, cp.mt, cp.nt, cp.wm, cp.wn, cp.nstage, cp.th, cp.tw, cp.cpp, cp.pitch, cp.kord, cp.g, (int)cp.tail, (int)cp.x2, b.k_order}) sg.push_back(f);
            }
            if (st.th == 0) r.all = true;
            st.reads.push_back(r);
            for (int k = 0; k < n_ops; ++k) {                         // residuals and further sources from outside the launch
                const OpDesc& q = ops[oi + k];
                if (q.v[14] && cs.kind != ConvStep::C2f16) { RbRead rr; rr.buf = q.v[12], rr.c0 = q.v[13], rr.cn = q.v[6], rr.all = st.th == 0; st.reads.push_back(rr); }
                if (q.v[16]) st.reads.push_back(read_all(q.v[16] - 1));
                if (q.xs_buf >= 0) st.reads.push_back(read_all(q.xs_buf));
            }
        }
        steps.push_back(st), first.push_back(oi), step_sig.push_back(sg);
        p.n_ops[oi] = n_ops;
        oi += n_ops - 1;
    }
    const std::vector<RowWindow> w = plan_row_windows(steps, p.bands);
    size_t last_win = 0;
    for (size_t k = 0; k < steps.size(); ++k)
        if (w[k].rows) last_win = k;
    // the rows a windowed run leaves alone were computed by the kernels of the run that put them there, from rows the kernels in front of
    // them computed: the signature names every launch up to the last windowed one (kernels of one layer may round differently)
    for (size_t k = 0; k <= last_win && k < steps.size(); ++k) {
        p.sig.insert(p.sig.end(), step_sig[k].begin(), step_sig[k].end());
        p.sig.push_back(w[k].y0), p.sig.push_back(w[k].rows);
    }
    for (size_t k = 0; k < steps.size(); ++k) {
        if (w[k].rows == 0) continue;
        const RbStep& st = steps[k];
        const TileWindow t = tile_window(w[k].y0, w[k].rows, st.th, st.Ho);
        p.win[first[k]] = w[k];
        p.th[first[k]] = st.th, p.exact[first[k]] = st.exact;
        p.frac[first[k]] = (float)(st.exact ? w[k].rows : t.tiles * st.th) / (float)st.Ho;
        for (int j = 0; j < p.n_ops[first[k]]; ++j) p.covered[first[k] + j] = 1;
        p.any = true;
    }
    if (row_plans.size() >= 8) row_plans.erase(row_plans.begin());
    row_plans.push_back(std::move(p));
    return row_plans.back();
}

void Model::run_frames(const uint8_t* frames, int n, const LetterboxGeom& g, hipStream_t s) {
    AIC_REQUIRE(n >= 0 && n <= max_items, AIC_ERR_CAPACITY, "batch exceeds the engine's max_items");
    if (n == 0) return;
    const int* v = ops[0].v;
    const bool stem = kind == KIND_YOLO && dtype == AIC_F16 && ops[0].fuse == 0 && v[0] == OP_CONV && v[1] == 0 && v[2] == 0 &&
                      v[3] == 3 && v[6] == 16 && v[7] == 3 && v[8] == 3 && v[9] == 2 && v[10] == 1 && v[11] == 1 && v[14] == 0;
    rb_ran.assign(ops.size(), 0), rb_ran_win.assign(ops.size(), RowWindow{});
    if (stem) {
        const ConvWeights& w = weights[v[15]];
        const BufDesc& db = bufs[v[4]];
        // AICAM_NO_ROW_BAND=1: every launch computes its full map, as before the row bands (A/B runs, the reference of the bit-equality tests)
        static const bool rb_on = getenv("AICAM_NO_ROW_BAND") == nullptr;
        // (launches of a few frames may run their heads on side streams in pieces of the op list: no windows there)
        const bool plain = !(side_ok && !side_heads.empty() && n <= side_max_items);
        const RowPlan* rp = rb_on && plain && db.h % 8 == 0 ? &row_plan(g, n) : nullptr;
        if (rp && !rp->any) rp = nullptr;
        const bool windowed = rp && rb_slots >= n && rb_top == rp->top && rb_unpad == rp->unpad_h && rb_sig == rp->sig;
        const int slots = rb_slots;
        rb_slots = 0;                               // until this call is through: a failed launch leaves nothing known
        const RowWindow w0 = windowed ? rp->win[0] : RowWindow{};
        const double share = windowed ? rp->frac[0] : 1.0;
        bool ok;
        {
            Prof pr(*dev, PROF_LETTERBOX, s, 2.0 * n * db.h * db.w * 16.0 * 27.0 * share,
                    (double)n * ((double)g.src_h * g.src_w * 3 + (double)db.h * db.w * 32.0 * share));
            ok = launch_yolo_stem_fused(frames, n, g, w.w.p, w.bias.p, w.Kp, db.p, db.c, v[5], db.h, db.w, s, w0.y0, w0.rows);
        }
        if (ok) {
            cls_reduced = box_decoded = 0;
            rb_now = windowed ? rp : nullptr;
            try {
                run_ops(1, n, s);
            } catch (...) {
                rb_now = nullptr;
                throw;
            }
            rb_now = nullptr;
            if (windowed) {
                rb_slots = slots;
                rb_ran = rp->covered, rb_ran_win = rp->win;
                for (size_t i = 0; i < ops.size(); ++i)           // (the query answers per op: a covered op has its launch's window)
                    if (rp->covered[i] && rp->n_ops[i] == 0 && i > 0) rb_ran_win[i] = rb_ran_win[i - 1];
            } else if (rp) {
                rb_top = rp->top, rb_unpad = rp->unpad_h, rb_slots = n, rb_sig = rp->sig;
            }
            return;
        }
    }
    {
        Prof pr(*dev, PROF_LETTERBOX, s, 0, (double)n * ((double)g.src_h * g.src_w * 3 + 16.0 * in_h * in_w));
        launch_letterbox(frames, n, g, 1, dtype, input(), s);
    }
    run(n, s);
}

// What run_range launches at conv op `oi` (engine.hpp, ConvStep).  No launch, no change to the model: aic_model_conv_plan asks the same
// question for a test.
Model::ConvStep Model::conv_step(size_t oi, size_t op1, int n) const {
    ConvStep st;
    const OpDesc& o = ops[oi];
    double fl = 0, by = 0;
    auto conv_args = [&](size_t k) {
        const int* u = ops[k].v;
        const BufDesc& xb = bufs[u[1]];
        const BufDesc& yb = bufs[u[4]];
        const ConvWeights& w = weights[u[15]];
        ConvArgs a{};
        a.x = xb.p, a.w = w.w.p, a.bias = w.bias.p, a.y = yb.p;
        a.x_cs = xb.c, a.x_coff = u[2], a.H = xb.h, a.W = xb.w, a.Cin = w.cin_eff;
        a.y_cs = yb.c, a.y_coff = u[5], a.Ho = yb.h, a.Wo = yb.w, a.Cout = w.cout;
        a.res = nullptr, a.r_cs = 0, a.r_coff = 0, a.res_mode = u[14], a.act = u[11];
        if (u[14]) { a.res = bufs[u[12]].p, a.r_cs = bufs[u[12]].c, a.r_coff = u[13]; }
        a.KH = w.kh, a.KW = w.kw, a.stride = u[9], a.pad = u[10];
        if (ops[k].xs_buf >= 0) {               // folded 2x upsample: the first channels come from the half-resolution tensor
            const BufDesc& bs = bufs[ops[k].xs_buf];
            a.xs = bs.p, a.xs_cs = bs.c, a.xs_coff = ops[k].xs_coff, a.Hs = bs.h, a.Ws = bs.w, a.Cs = ops[k].xs_c;
        }
        if (u[16]) {                            // folded 1x1 second source
            const BufDesc& b2 = bufs[u[16] - 1];
            a.x2 = b2.p, a.x2_cs = b2.c, a.x2_coff = u[17], a.H2 = b2.h, a.W2 = b2.w, a.s2 = u[19], a.Cin2 = u[18];
            fl += 2.0 * n * yb.h * yb.w * (double)w.cout * u[18];
            by += ((double)n * yb.h * yb.w * u[18] + (double)w.cout * u[18]) * (dtype == AIC_F16 ? 2 : 4);
        }
        a.Kp = w.Kp, a.M = n * yb.h * yb.w, a.out_f32 = yb.f32, a.cout_pad = w.cout_pad, a.zero = d_zero.p;
        a.tap_rows = 0;
        a.n_dev = n_items_dev;
        for (int kh = 0; kh < w.kh; ++kh) a.tap_rows |= 1u << (kh * w.kw);
        AIC_REQUIRE(w.kh * w.kw <= 25, AIC_ERR_FORMAT, "kernel window larger than 5x5");
        fl += 2.0 * a.M * (double)w.cout * w.cin * w.kh * w.kw;
        by += ((double)n * xb.h * xb.w * w.cin + (double)a.M * w.cout) * (dtype == AIC_F16 ? 2 : 4) +
              (double)w.cout * w.cin * w.kh * w.kw * (dtype == AIC_F16 ? 2 : 4);
        return a;
    };
    auto done = [&](int kind, int n_ops) { st.kind = kind, st.n_ops = n_ops, st.fl = fl, st.by = by; return st; };
    const ConvArgs a = st.a[0] = conv_args(oi);
    // a 64-channel BasicBlock (this conv and the next, which adds this one's input) runs as ONE kernel where it applies;
    // FLOPs and algorithmic bytes are accounted as for the two convs
    bool pair = false;
    ConvArgs a2{};
    if (dtype == AIC_F16 && oi + 1 < op1 && ops[oi + 1].v[0] == OP_CONV && ops[oi + 1].fuse == 0 && a.Cin == 64 && a.Cout == 64 &&
        a.res_mode == 0 && ops[oi + 1].v[14] == 1) {
        const double fl0 = fl, by0 = by;
        a2 = conv_args(oi + 1);
        pair = a2.res == a.x && a2.x == a.y;
        if (!pair) fl = fl0, by = by0;
    }
    // a C2f block with 16-channel halves (YOLOv8n's 160 x 160 stage: cv1, m.cv1, m.cv2 + shortcut, cv2) runs as ONE kernel where
    // it applies; FLOPs and algorithmic bytes are accounted as for the four convs
    if (!pair && dtype == AIC_F16 && oi + 3 < op1 && a.KH == 1 && a.Cin == 32 && a.Cout == 32 && ops[oi + 1].v[0] == OP_CONV &&
        ops[oi + 2].v[0] == OP_CONV && ops[oi + 3].v[0] == OP_CONV && !ops[oi + 1].fuse && !ops[oi + 2].fuse && !ops[oi + 3].fuse) {
        const double fl0 = fl, by0 = by;
        const ConvArgs b1 = conv_args(oi + 1), b2 = conv_args(oi + 2), b3 = conv_args(oi + 3);
        if (plan_c2f16(a, b1, b2, b3)) {
            st.a[1] = b1, st.a[2] = b2, st.a[3] = b3;
            return done(ConvStep::C2f16, 4);
        }
        fl = fl0, by = by0;
    }
    if (const int ipb = pair ? plan_c64_block(a, a2, conv_cu_budget()) : 0) {
        st.a[1] = a2, st.ipb = ipb;
        return done(ConvStep::C64Block, 2);
    }
    if (pair) { fl = 0, by = 0; (void)conv_args(oi); }          // not fused after all: account this conv alone
    // a conv whose only consumer is the 1x1 conv after it (marked at load time) takes that conv into its epilogue where the
    // kernels can; FLOPs and algorithmic bytes are accounted as for the two convs
    if (o.fuse == 3 && oi + 1 < op1) {
        const double fl0 = fl, by0 = by;
        const ConvArgs t = conv_args(oi + 1);
        if (conv_tail_supported(dtype, a, t)) {
            ConvArgs at = a;
            at.w_tail = t.w, at.b_tail = t.bias, at.y_tail = t.y, at.t_cout = t.Cout, at.t_kp = t.Kp;
            at.t_y_cs = t.y_cs, at.t_y_coff = t.y_coff, at.t_out_f32 = t.out_f32, at.t_act = t.act;
            static const bool cls_reduce_on = getenv("AICAM_NO_CLS_REDUCE") == nullptr;
            static const bool box_decode_on = getenv("AICAM_NO_BOX_DECODE") == nullptr;
            if (reduce_cls && kind == KIND_YOLO && t.out_f32 && t.act == 0 && t.y_coff == 0 && t.y_cs == t.Cout) {
                // a detect level's class / box branch: its logits only feed decode's arg-max / DFL expectation.  Which of the two it is, is
                // what it writes -- the level's class or box tensor -- not its width: with nc = 64 both 1x1s have 64 outputs
                int a0 = 0;
                for (size_t l = 0; l < outs.size(); ++l) {
                    const int* ov = outs[l].v;
                    const int hw = ov[3] * ov[4];
                    const bool is_cls = cls_reduce_on && bufs[ov[1]].p == t.y && t.Cout == meta[0];
                    const bool is_box = box_decode_on && bufs[ov[0]].p == t.y && meta[1] == 16 && t.Cout == 64 && a.Cout == 64;   // tail_1x1 decodes in place only in its NT == 4 form (lead Cout 64; YOLOv8x leads with 80)
                    if ((is_cls || is_box) && hw == t.Ho * t.Wo) {
                        at.t_hw = hw, at.t_a0 = a0, at.t_na = n_anchors;
                        if (is_cls) {
                            at.t_max = d_maxlogit.p, at.t_arg = d_labels.p;
                            st.cls_bits |= 1u << l;
                        } else {
                            at.t_box = d_boxes.p, at.t_w = ov[4], at.t_stride = ov[2];
                            st.box_bits |= 1u << l;
                        }
                        break;
                    }
                    a0 += hw;
                }
            }
            st.a[0] = at;
            return done(ConvStep::Tail, 2);
        }
        fl = fl0, by = by0;
    }
    return done(ConvStep::Single, 1);
}

void Model::run_range(size_t op0, size_t op1, int n, hipStream_t s) {
    // HIP-event timing of the conv kernel brackets RUNS of consecutive conv launches (one event pair per
    // run, not per launch: two event records per launch cost 13 % of end-to-end throughput); the summed
    // time therefore includes the ~1-2 us dependent-launch gaps inside a run (a conservative `achieved`).
    const bool prof_conv = (dev->prof_mask >> PROF_CONV) & 1u;
    bool span_open = false;
    auto span_close = [&] { if (span_open) { dev->prof_end(PROF_CONV, s); span_open = false; } };
    for (size_t oi = op0; oi < op1; ++oi) {
        const OpDesc& o = ops[oi];
        const int* v = o.v;
        const BufDesc& sb = bufs[v[1]];
        const BufDesc& db = bufs[v[4]];
        if (o.fuse == 2 || (!sp_skip.empty() && sp_skip[oi])) continue;     // absorbed at load time, or listed behind the head by run_ops
        if (o.fuse == 1 || v[0] != OP_CONV) span_close();
        if (o.fuse == 1) {
            const ConvWeights& w = weights[v[15]];
            const int* pv = ops[oi + 1].v;
            const BufDesc& pb = bufs[pv[4]];
            const double fl = 2.0 * n * sb.h * sb.w * 64.0 * 27.0;
            Prof pr(*dev, PROF_CONV_DIRECT, s, fl, (double)n * (sb.h * sb.w * 16.0 + pb.h * pb.w * 128.0));
            launch_reid_stem_pool(sb.p, w.w.p, w.bias.p, pb.p, n, sb.h, sb.w, w.Kp, pb.c, pv[5], in_pix4 ? 4 : 8, s,
                                  (crop_src.frames && in_pix4) ? &crop_src : nullptr, n_items_dev);
            continue;
        }
        if (v[0] == OP_CONV) {
            if (prof_conv && !span_open) { dev->prof_begin(PROF_CONV, s, 0, 0); span_open = true; }
            ConvStep st = conv_step(oi, op1, n);
            double share = 1.0;
            if (rb_now && rb_now->win[oi].rows > 0) {                   // a row window (engine.hpp): planned for exactly this launch
                AIC_REQUIRE(rb_now->n_ops[oi] == st.n_ops && rb_now->n == n, AIC_ERR_INVALID, "row window planned for another launch");
                if (st.kind == ConvStep::Single || st.kind == ConvStep::Tail) {   // ... and for the kernel form launch_conv_igemm is about to select
                    ConvArgs b = st.a[0];
                    bool exact = false;
                    const int th = conv_window_tile(plan_conv_launch(dtype, b, conv_cu_budget()), exact);
                    AIC_REQUIRE(th > 0 && th == rb_now->th[oi] && exact == (rb_now->exact[oi] != 0), AIC_ERR_INVALID, "row window planned for another kernel form");
                }
                ConvArgs& wa = st.a[st.kind == ConvStep::C2f16 ? 3 : 0];
                wa.win_y0 = rb_now->win[oi].y0, wa.win_rows = rb_now->win[oi].rows;
                share = rb_now->frac[oi];
            }
            if (prof_conv) dev->prof_account(PROF_CONV, st.fl * share, st.by * share);   // what the launch executes, not the layer's
            switch (st.kind) {
                case ConvStep::C2f16: launch_c2f16(st.a[0], st.a[1], st.a[2], st.a[3], s); break;
                case ConvStep::C64Block: launch_c64_block(st.a[0], st.a[1], st.ipb, s); break;
                case ConvStep::Tail: cls_reduced |= st.cls_bits, box_decoded |= st.box_bits; [[fallthrough]];
                default: launch_conv_igemm(dtype, st.a[0], s);
            }
            oi += st.n_ops - 1;
        } else {
            EltArgs a{};
            a.src = sb.p, a.dst = db.p, a.n = n, a.h = sb.h, a.w = sb.w, a.c = v[3];
            if (emb_host_out && oi + 1 == ops.size() && v[0] == OP_L2NORM && v[4] == outs[0].v[0]) a.dst = emb_host_out;
            a.s_cs = sb.c, a.s_coff = v[2], a.d_cs = db.c, a.d_coff = v[5];
            a.n_dev = n_items_dev;
            Prof pr(*dev, PROF_MISC, s, 0, 0);
            switch (v[0]) {
                case OP_SPPF_POOL: launch_sppf_pool(dtype, a, s); break;
                case OP_UPSAMPLE2X: launch_upsample2x(dtype, a, s); break;
                case OP_MAXPOOL3S2: launch_maxpool3s2(dtype, a, s); break;
                case OP_AVGPOOL: launch_avgpool(dtype, a, s); break;
                case OP_L2NORM: launch_l2norm(dtype, a, s); break;
                default: throw Error(AIC_ERR_FORMAT, "unknown op in engine file");
            }
        }
    }
    span_close();
}

DetArgs Model::det_args(int batch, float conf, float iou, int max_det, const LetterboxGeom* g) {
    AIC_REQUIRE(kind == KIND_YOLO, AIC_ERR_INVALID, "not a YOLO engine");
    AIC_REQUIRE(max_det > 0 && max_det <= max_det_cap, AIC_ERR_CAPACITY, "max_det out of range (1..1024)");
    AIC_REQUIRE(conf > 0.f && conf < 1.f, AIC_ERR_INVALID, "conf_thresh must be in (0,1)");
    DetArgs a{};
    int a0 = 0;
    for (size_t l = 0; l < outs.size(); ++l) {
        const int* v = outs[l].v;
        a.lvl[l].box = reinterpret_cast<const float*>(bufs[v[0]].p);
        a.lvl[l].cls = reinterpret_cast<const float*>(bufs[v[1]].p);
        a.lvl[l].stride = v[2], a.lvl[l].h = v[3], a.lvl[l].w = v[4], a.lvl[l].a0 = a0;
        a.lvl[l].cls_reduced = (cls_reduced >> l) & 1u, a.lvl[l].box_decoded = (box_decoded >> l) & 1u;
        a0 += v[3] * v[4];
    }
    a.n_levels = (int)outs.size(), a.n_anchors = n_anchors, a.nc = meta[0], a.reg_max = meta[1], a.batch = batch;
    a.fast_exp = dtype == AIC_F16;
    a.logit_thr = logit_of(conf);
    a.iou_thr = iou, a.max_det = max_det;
    a.pad_w = g ? g->pad_w : 0.f, a.pad_h = g ? g->pad_h : 0.f, a.ratio = g ? g->ratio : 1.f;
    a.orig_w = g ? g->src_w : in_w, a.orig_h = g ? g->src_h : in_h;
    a.boxes = d_boxes.p, a.max_logit = d_maxlogit.p, a.labels = d_labels.p, a.keys = nullptr;
    a.n_cand = d_ncand.p, a.num_dets = d_numdets.p;
    a.out_boxes = d_out_boxes.p, a.out_boxes_orig = g ? d_out_boxes_orig.p : nullptr;
    a.out_scores = d_out_scores.p, a.out_labels = d_out_labels.p;
    return a;
}

void Model::decode_nms(int batch, float conf, float iou, int max_det, const LetterboxGeom* g, hipStream_t s, char* host_out) {
    DetArgs a = det_args(batch, conf, iou, max_det, g);
    if (host_out) {
        AIC_REQUIRE(g != nullptr, AIC_ERR_INVALID, "decode_nms: host output wants the letterbox geometry");
        a.num_dets = reinterpret_cast<int*>(host_out);
        a.out_boxes_orig = reinterpret_cast<float*>(host_out + (size_t)batch * 4);
        a.out_scores = reinterpret_cast<float*>(host_out + (size_t)batch * 4 + (size_t)batch * max_det * 16);
        a.out_labels = reinterpret_cast<int*>(host_out + (size_t)batch * 4 + (size_t)batch * max_det * 20);
    }
    // a run that listed its box branches left boxes at the candidates of ITS threshold: a call at or above it reads a subset of them, a
    // call below it lists and computes again at its own threshold first (the neck's outputs are still in place, every buffer has its own storage)
    if (sp_listed && a.logit_thr < sp_thr) sparse_box_pass(sp_n, a.logit_thr, true, nullptr, s);
    {
        Prof pr(*dev, PROF_DET, s, 0, (double)batch * n_anchors * (4 * meta[1] + meta[0]) * 4);
        launch_decode(a, s);
        launch_select_sort_nms(a, s);
    }
    if (sp_pass) {                              // the four counts come back with the detections: 16 bytes behind the NMS on its stream
        HIP_CHECK(hipMemcpyAsync(h_sp_count.p, d_sp_count.p, 16, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipEventRecord(sp_ev, s));
        sp_ev_pending = true, sp_ev_n = sp_n;
    }
}

}  // namespace aic

// =================================================================================================
using namespace aic;

namespace {

// conf passed through Python is a double rounded to float; the logit threshold is computed from the
// fp64 value of that float so both sides of the parity test agree on the same number.
void copy_out(void* dst, const void* src, size_t bytes, int mem, hipStream_t s) {
    if (!bytes || !dst) return;
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, mem == AIC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
}

// The detections of a call into the caller's host arrays (each may be NULL), from the staged block decode_nms's host_out names:
// counts[batch] | boxes[batch, max_det, 4] | scores[batch, max_det] | labels[batch, max_det].  One contract at every batch size
// (include/aicam.h, aic_detect): the first min(count, max_det) rows of a frame are written, rows past a frame's count are left as
// the caller passed them -- the NMS kernel stores only the rows it keeps, what lies behind them in the block is nobody's.
void scatter_dets(const char* h, int batch, int max_det, int32_t* num_dets, float* boxes, float* scores, int32_t* labels) {
    const int32_t* hn = reinterpret_cast<const int32_t*>(h);
    const char* hb = h + (size_t)batch * 4;
    const char* hs = hb + (size_t)batch * max_det * 16;
    const char* hl = hb + (size_t)batch * max_det * 20;
    for (int b = 0; b < batch; ++b) {
        const int n = std::min(std::max(hn[b], 0), max_det);
        if (num_dets) num_dets[b] = hn[b];
        if (boxes) std::memcpy(boxes + (size_t)b * max_det * 4, hb + (size_t)b * max_det * 16, (size_t)n * 16);
        if (scores) std::memcpy(scores + (size_t)b * max_det, hs + (size_t)b * max_det * 4, (size_t)n * 4);
        if (labels) std::memcpy(labels + (size_t)b * max_det, hl + (size_t)b * max_det * 4, (size_t)n * 4);
    }
}

// ... of a decode_nms that stored on the device: staged through the engine's page-locked block, then as above.  Waits for the stream.
void copy_out_dets(Model& m, int batch, int max_det, const float* d_boxes, int32_t* num_dets, float* boxes, float* scores,
                   int32_t* labels, hipStream_t s) {
    const size_t rows = (size_t)batch * max_det;
    m.h_det.ensure((size_t)batch * 4 + rows * 24 + 16);
    char* h = m.h_det.p;
    copy_out(h, m.d_numdets.p, (size_t)batch * 4, AIC_HOST, s);
    copy_out(h + (size_t)batch * 4, d_boxes, rows * 16, AIC_HOST, s);
    copy_out(h + (size_t)batch * 4 + rows * 16, m.d_out_scores.p, rows * 4, AIC_HOST, s);
    copy_out(h + (size_t)batch * 4 + rows * 20, m.d_out_labels.p, rows * 4, AIC_HOST, s);
    HIP_CHECK(hipStreamSynchronize(s));
    scatter_dets(h, batch, max_det, num_dets, boxes, scores, labels);
}

void load_input_nchw(Model& m, const float* images, int n, int mem, hipStream_t s) {
    const size_t cnt = (size_t)n * 3 * m.in_h * m.in_w;
    const float* src = images;
    if (mem == AIC_HOST) {
        m.d_in_f32.ensure(cnt);
        HIP_CHECK(hipMemcpyAsync(m.d_in_f32.p, images, cnt * 4, hipMemcpyHostToDevice, s));
        src = m.d_in_f32.p;
    }
    Prof pr(*m.dev, PROF_MISC, s);
    m.in_pix4 = false;
    launch_nchw_to_nhwc8(m.dtype, src, m.input(), n, m.in_h, m.in_w, s);
}

// Every call uploads the frames it is handed into its own engine's staging buffer: nothing is shared with another engine's call.
const uint8_t* stage_frames(Model& m, const uint8_t* frames, size_t bytes, int mem, hipStream_t s) {
    if (mem == AIC_DEVICE) return frames;
    m.d_frames.ensure(bytes + 16);           // (slack: the fused crop reads aligned 12-byte groups that may end past the last pixel)
    HIP_CHECK(hipMemcpyAsync(m.d_frames.p, frames, bytes, hipMemcpyHostToDevice, s));
    return m.d_frames.p;
}

}  // namespace

extern "C" {

int aic_model_load_mem(const void* blob, size_t nbytes, int device_id, int dtype, int max_items, aic_model** out) {
    return guarded([&] {
        AIC_REQUIRE(blob && out, AIC_ERR_INVALID, "NULL argument");
        *out = new aic_model(device(device_id), blob, nbytes, dtype, max_items);
    });
}

int aic_model_load(const char* path, int device_id, int dtype, int max_items, aic_model** out) {
    return guarded([&] {
        AIC_REQUIRE(path && out, AIC_ERR_INVALID, "NULL argument");
        std::ifstream f(path, std::ios::binary | std::ios::ate);
        AIC_REQUIRE(f.good(), AIC_ERR_NOT_FOUND, std::string("engine file not found: ") + path);
        const size_t n = (size_t)f.tellg();
        std::vector<char> blob(n);
        f.seekg(0);
        f.read(blob.data(), (std::streamsize)n);
        AIC_REQUIRE(f.good(), AIC_ERR_FORMAT, std::string("cannot read engine file: ") + path);
        *out = new aic_model(device(device_id), blob.data(), n, dtype, max_items);
    });
}

int aic_debug_alloc_probe(int device_id, float* f32_out, int32_t* i32_out, uint8_t* u8_out, uint8_t* pinned_u8_out) {
    return guarded([&] {
        AIC_REQUIRE(f32_out && i32_out && u8_out && pinned_u8_out, AIC_ERR_INVALID, "NULL argument");
        device(device_id).use();
        DevBuf<float> df(64);                   // fresh, and nothing below writes them: an uninitialised read by construction
        DevBuf<int> di(64);
        DevBuf<uint8_t> du(64);
        PinBuf<uint8_t> hu;
        hu.alloc(64);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(f32_out, df.p, 16, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(i32_out, di.p, 16, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(u8_out, du.p, 4, hipMemcpyDeviceToHost));
        std::memcpy(pinned_u8_out, hu.p, 4);
    });
}

int aic_model_read_buffer(aic_model* m, int buf, void* out, size_t bytes) {
    return guarded([&] {
        AIC_REQUIRE(m && out && buf >= 0 && buf < (int)m->m.bufs.size() && m->m.bufs[buf].p, AIC_ERR_INVALID, "bad buffer index");
        AIC_REQUIRE(bytes <= m->m.bufs[buf].per_item * (size_t)m->m.max_items, AIC_ERR_CAPACITY, "more bytes than the buffer holds");
        m->m.dev->use();
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, m->m.bufs[buf].p, bytes, hipMemcpyDeviceToHost));
    });
}

// aic_model_conv_plan / aic_model_conv_plan_live: the walk of run_range up to op `op`, every step asked of Model::conv_step
static void conv_plan_query(const Model& m, int op, int n, int32_t* out) {
    {
        std::fill(out, out + 24, 0);
        for (size_t oi = 0; oi < m.ops.size(); ++oi) {          // the walk of run_range
            const OpDesc& o = m.ops[oi];
            const bool launches = o.v[0] == OP_CONV && o.fuse != 2 && o.fuse != 1;
            if (!launches) {
                if ((int)oi == op) { out[0] = -1; return; }
                continue;
            }
            const Model::ConvStep st = m.conv_step(oi, m.ops.size(), n);
            if (op >= (int)(oi + st.n_ops)) { oi += st.n_ops - 1; continue; }
            out[1] = (int)oi, out[2] = st.n_ops, out[3] = st.ipb;
            if ((int)oi != op) { out[0] = -2; return; }
            out[0] = st.kind;
            if (st.kind == Model::ConvStep::Single || st.kind == Model::ConvStep::Tail) {
                ConvArgs a = st.a[0];
                const ConvPlan p = plan_conv_launch(m.dtype, a, conv_cu_budget());
                const long v[] = {(long)p.form, p.mt, p.nt, p.wm, p.wn, p.nstage, p.th, p.tw, p.cpp, p.pitch, p.kord, p.g, p.tail, p.x2, p.run, p.blocks};
                out[4] = a.k_order;
                for (int i = 0; i < 16; ++i) out[5 + i] = (int32_t)v[i];
                out[21] = a.xs != nullptr, out[22] = a.y_coff, out[23] = a.x_coff;
            }
            return;
        }
    }
}

int aic_model_conv_plan(aic_model* mm, int op, int n, int32_t* out) {
    return guarded([&] {
        AIC_REQUIRE(mm && out && op >= 0 && op < (int)mm->m.ops.size() && n > 0 && n <= mm->m.max_items, AIC_ERR_INVALID, "bad argument");
        conv_plan_query(mm->m, op, n, out);
    });
}

int aic_model_conv_plan_live(aic_model* mm, int op, int n, int32_t* out) {
    return guarded([&] {
        AIC_REQUIRE(mm && out && op >= 0 && op < (int)mm->m.ops.size() && n > 0 && n <= mm->m.max_items, AIC_ERR_INVALID, "bad argument");
        Model& m = mm->m;
        const int* before = m.n_items_dev;
        m.n_items_dev = reinterpret_cast<const int*>(m.d_zero.p);      // any device address: nothing is launched, nobody reads it
        try {
            conv_plan_query(m, op, n, out);
        } catch (...) {
            m.n_items_dev = before;
            throw;
        }
        m.n_items_dev = before;
    });
}

int aic_model_row_band(aic_model* mm, int op, int src_h, int src_w, int32_t* out) {
    return guarded([&] {
        AIC_REQUIRE(mm && out && op >= 0 && op < (int)mm->m.ops.size() && src_h > 0 && src_w > 0, AIC_ERR_INVALID, "bad argument");
        const Model& m = mm->m;
        const LetterboxGeom g = letterbox_geometry(src_h, src_w, m.in_h, m.in_w);
        const RowBand b = m.plan_bands(g)[op];
        const int h = m.bufs[m.ops[op].v[4]].h;
        out[0] = b.full ? 1 : 0, out[1] = b.full ? 0 : b.lo, out[2] = b.full ? h - 1 : b.hi, out[3] = h;
        const bool ran = op < (int)m.rb_ran.size() && m.rb_ran[op];
        out[4] = ran ? 1 : 0;
        out[5] = ran ? m.rb_ran_win[op].y0 : 0, out[6] = ran ? m.rb_ran_win[op].rows : 0;
        out[7] = m.rb_slots;
    });
}

int aic_model_destroy(aic_model* m) {
    return guarded([&] {
        if (m) {
            m->m.dev->use();
            (void)hipDeviceSynchronize();
        }
        delete m;
    });
}

int aic_model_info(const aic_model* m, int* kind, int* in_h, int* in_w, int* out_dim, int* n_anchors,
                   double* flops_per_item, int* n_convs) {
    return guarded([&] {
        AIC_REQUIRE(m, AIC_ERR_INVALID, "NULL model");
        if (kind) *kind = m->m.kind;
        if (in_h) *in_h = m->m.in_h;
        if (in_w) *in_w = m->m.in_w;
        if (out_dim) *out_dim = m->m.out_dim;
        if (n_anchors) *n_anchors = m->m.n_anchors;
        if (flops_per_item) *flops_per_item = m->m.flops_per_item;
        if (n_convs) *n_convs = m->m.n_convs;
    });
}

int aic_yolo_infer(aic_model* mm, const float* images, int batch, int mem, float conf, float iou, int max_det,
                   int32_t* num_dets, float* bboxes, float* scores, int32_t* labels) {
    return guarded([&] {
        AIC_REQUIRE(mm && images && batch > 0, AIC_ERR_INVALID, "bad argument");
        Model& m = mm->m;
        AIC_REQUIRE(m.kind == KIND_YOLO, AIC_ERR_INVALID, "not a YOLO engine");
        m.dev->use();
        hipStream_t s = m.dev->s_main;
        load_input_nchw(m, images, batch, mem, s);
        m.reduce_cls = true;                    // (only the decoded outputs leave this call)
        m.side_ok = true;
        m.run(batch, s);
        m.side_ok = false;
        m.decode_nms(batch, conf, iou, max_det, nullptr, s);
        if (mem == AIC_HOST) {                  // rows past a frame's count stay the caller's, as in aic_detect
            copy_out_dets(m, batch, max_det, m.d_out_boxes.p, num_dets, bboxes, scores, labels, s);
            return;
        }
        copy_out(num_dets, m.d_numdets.p, (size_t)batch * 4, mem, s);
        copy_out(bboxes, m.d_out_boxes.p, (size_t)batch * max_det * 16, mem, s);
        copy_out(scores, m.d_out_scores.p, (size_t)batch * max_det * 4, mem, s);
        copy_out(labels, m.d_out_labels.p, (size_t)batch * max_det * 4, mem, s);
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aic_yolo_head(aic_model* mm, const float* images, int batch, int mem, float* dfl, float* cls) {
    return guarded([&] {
        AIC_REQUIRE(mm && images && batch > 0, AIC_ERR_INVALID, "bad argument");
        Model& m = mm->m;
        AIC_REQUIRE(m.kind == KIND_YOLO, AIC_ERR_INVALID, "not a YOLO engine");
        m.dev->use();
        hipStream_t s = m.dev->s_main;
        load_input_nchw(m, images, batch, mem, s);
        m.reduce_cls = false;                   // the raw class logits are what this call returns
        m.side_ok = true;
        m.run(batch, s);
        m.side_ok = false;
        const int nc = m.meta[0], nb = 4 * m.meta[1];
        int a0 = 0;
        for (auto& o : m.outs) {
            const int hw = o.v[3] * o.v[4];
            const float* bsrc = reinterpret_cast<const float*>(m.bufs[o.v[0]].p);
            const float* csrc = reinterpret_cast<const float*>(m.bufs[o.v[1]].p);
            for (int b = 0; b < batch; ++b) {
                if (dfl) HIP_CHECK(hipMemcpyAsync(dfl + ((size_t)b * m.n_anchors + a0) * nb, bsrc + (size_t)b * hw * nb,
                                                  (size_t)hw * nb * 4, hipMemcpyDeviceToHost, s));
                if (cls) HIP_CHECK(hipMemcpyAsync(cls + ((size_t)b * m.n_anchors + a0) * nc, csrc + (size_t)b * hw * nc,
                                                  (size_t)hw * nc * 4, hipMemcpyDeviceToHost, s));
            }
            a0 += hw;
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aic_yolo_decode(aic_model* mm, const float* images, int batch, int mem, float* boxes, float* max_logit, int32_t* labels) {
    return guarded([&] {
        AIC_REQUIRE(mm && images && batch > 0, AIC_ERR_INVALID, "bad argument");
        Model& m = mm->m;
        AIC_REQUIRE(m.kind == KIND_YOLO, AIC_ERR_INVALID, "not a YOLO engine");
        m.dev->use();
        hipStream_t s = m.dev->s_main;
        load_input_nchw(m, images, batch, mem, s);
        m.reduce_cls = true;
        m.side_ok = true;
        m.run(batch, s);
        m.side_ok = false;
        const DetArgs a = m.det_args(batch, 0.5f, 0.5f, 1, nullptr);
        launch_decode(a, s);
        const size_t ba = (size_t)batch * m.n_anchors;
        copy_out(boxes, m.d_boxes.p, ba * 16, AIC_HOST, s);
        copy_out(max_logit, m.d_maxlogit.p, ba * 4, AIC_HOST, s);
        copy_out(labels, m.d_labels.p, ba * 4, AIC_HOST, s);
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aic_yolo_postprocess(aic_model* mm, const float* dfl, const float* cls, int batch, float conf, float iou, int max_det, int use_geom,
                         float pad_w, float pad_h, float ratio, int orig_w, int orig_h, float* boxes, float* max_logit, int32_t* labels,
                         int32_t* n_cand, int32_t* num_dets, float* out_boxes, float* out_boxes_orig, float* out_scores, int32_t* out_labels) {
    return guarded([&] {
        AIC_REQUIRE(mm && dfl && cls && boxes && max_logit && labels && n_cand && num_dets && out_boxes && out_scores && out_labels,
                    AIC_ERR_INVALID, "NULL argument");
        Model& m = mm->m;
        AIC_REQUIRE(m.kind == KIND_YOLO, AIC_ERR_INVALID, "not a YOLO engine");
        AIC_REQUIRE(batch > 0, AIC_ERR_INVALID, "batch must be positive");
        AIC_REQUIRE(batch <= m.max_items, AIC_ERR_CAPACITY, "batch exceeds the engine's max_items");
        AIC_REQUIRE(iou >= 0.f && iou <= 1.f, AIC_ERR_INVALID, "iou_thresh must be in [0,1]");
        AIC_REQUIRE(!use_geom || (out_boxes_orig && ratio > 0.f && orig_w > 0 && orig_h > 0), AIC_ERR_INVALID, "bad letterbox geometry");
        m.dev->use();
        hipStream_t s = m.dev->s_main;
        LetterboxGeom g{};
        g.pad_w = pad_w, g.pad_h = pad_h, g.ratio = ratio, g.src_w = orig_w, g.src_h = orig_h;
        // decode_kernel does everything itself for this call: no detect-branch tail has run on these logits
        const unsigned keep_cls = m.cls_reduced, keep_box = m.box_decoded;
        m.cls_reduced = m.box_decoded = 0;
        DetArgs a;
        try {
            a = m.det_args(batch, conf, iou, max_det, use_geom ? &g : nullptr);       // (refuses max_det / conf out of range)
        } catch (...) {
            m.cls_reduced = keep_cls, m.box_decoded = keep_box;
            throw;
        }
        m.cls_reduced = keep_cls, m.box_decoded = keep_box;
        // the inverse of aic_yolo_head's copies: level-major host logits -> the model's own per-level head buffers
        const int nc = m.meta[0], nb = 4 * m.meta[1];
        int a0 = 0;
        for (auto& o : m.outs) {
            const int hw = o.v[3] * o.v[4];
            const BufDesc& bb = m.bufs[o.v[0]];
            const BufDesc& cb = m.bufs[o.v[1]];
            AIC_REQUIRE(bb.p && cb.p && bb.esize == 4 && cb.esize == 4, AIC_ERR_FORMAT, "head buffers are not fp32");
            for (int b = 0; b < batch; ++b) {
                HIP_CHECK(hipMemcpyAsync(reinterpret_cast<float*>(bb.p) + (size_t)b * hw * nb, dfl + ((size_t)b * m.n_anchors + a0) * nb,
                                         (size_t)hw * nb * 4, hipMemcpyHostToDevice, s));
                HIP_CHECK(hipMemcpyAsync(reinterpret_cast<float*>(cb.p) + (size_t)b * hw * nc, cls + ((size_t)b * m.n_anchors + a0) * nc,
                                         (size_t)hw * nc * 4, hipMemcpyHostToDevice, s));
            }
            a0 += hw;
        }
        // in/out: what the caller put into the output arrays is on the device before the kernels run
        const size_t ba = (size_t)batch * m.n_anchors, bm = (size_t)batch * max_det;
        const struct { void* host; void* dev; size_t bytes; } io[] = {
            {boxes, a.boxes, ba * 16}, {max_logit, a.max_logit, ba * 4}, {labels, a.labels, ba * 4}, {n_cand, a.n_cand, (size_t)batch * 4},
            {num_dets, a.num_dets, (size_t)batch * 4}, {out_boxes, a.out_boxes, bm * 16}, {out_boxes_orig, a.out_boxes_orig, bm * 16},
            {out_scores, a.out_scores, bm * 4}, {out_labels, a.out_labels, bm * 4}};
        for (const auto& e : io)
            if (e.host && e.dev) HIP_CHECK(hipMemcpyAsync(e.dev, e.host, e.bytes, hipMemcpyHostToDevice, s));
        launch_decode(a, s);
        launch_select_sort_nms(a, s);
        for (const auto& e : io)
            if (e.host && e.dev) HIP_CHECK(hipMemcpyAsync(e.host, e.dev, e.bytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aic_det_filter(int device_id, const int32_t* num_dets, const float* boxes, const float* scores, const int32_t* labels, int batch,
                   int max_det, float min_conf, const uint64_t* mask, int cap, int32_t* rank, int32_t* frame_n, int32_t* frame_d0,
                   int32_t* total, float* xyxy, float* tlwh, float* conf, int32_t* cls, int32_t* frame_of) {
    return guarded([&] {
        AIC_REQUIRE(num_dets && boxes && scores && labels && mask && rank && frame_n && frame_d0 && total && xyxy && tlwh && conf && cls &&
                    frame_of, AIC_ERR_INVALID, "NULL argument");
        AIC_REQUIRE(batch > 0 && max_det > 0 && cap > 0, AIC_ERR_INVALID, "batch, max_det and cap must be positive");
        AIC_REQUIRE((size_t)batch * max_det <= ((size_t)1 << 28), AIC_ERR_CAPACITY, "batch * max_det too large");
        Device& d = device(device_id);
        hipStream_t s = d.s_main;
        const size_t bm = (size_t)batch * max_det;
        DevBuf<int> d_nd(batch), d_lab(bm), d_rank(bm), d_fn(batch), d_fd0(batch), d_total(2), d_cls(cap), d_fof(cap);
        DevBuf<float> d_box(bm * 4), d_sc(bm), d_xyxy((size_t)cap * 4), d_tlwh((size_t)cap * 4), d_conf(cap);
        const struct { void* host; void* dev; size_t bytes; bool out; } io[] = {
            {const_cast<int32_t*>(num_dets), d_nd.p, (size_t)batch * 4, false}, {const_cast<float*>(boxes), d_box.p, bm * 16, false},
            {const_cast<float*>(scores), d_sc.p, bm * 4, false}, {const_cast<int32_t*>(labels), d_lab.p, bm * 4, false},
            {rank, d_rank.p, bm * 4, true}, {frame_n, d_fn.p, (size_t)batch * 4, true}, {frame_d0, d_fd0.p, (size_t)batch * 4, true},
            {total, d_total.p, 8, true}, {xyxy, d_xyxy.p, (size_t)cap * 16, true}, {tlwh, d_tlwh.p, (size_t)cap * 16, true},
            {conf, d_conf.p, (size_t)cap * 4, true}, {cls, d_cls.p, (size_t)cap * 4, true}, {frame_of, d_fof.p, (size_t)cap * 4, true}};
        for (const auto& e : io) HIP_CHECK(hipMemcpyAsync(e.dev, e.host, e.bytes, hipMemcpyHostToDevice, s));
        DetFilterArgs fa{};
        fa.num_dets = d_nd.p, fa.boxes = d_box.p, fa.scores = d_sc.p, fa.labels = d_lab.p;
        fa.batch = batch, fa.max_det = max_det, fa.min_conf = min_conf;
        fa.mask[0] = mask[0], fa.mask[1] = mask[1];
        fa.cap = cap, fa.rank = d_rank.p, fa.frame_n = d_fn.p, fa.frame_d0 = d_fd0.p, fa.total = d_total.p;
        fa.xyxy = d_xyxy.p, fa.tlwh = d_tlwh.p, fa.conf = d_conf.p, fa.cls = d_cls.p, fa.frame_of = d_fof.p;
        launch_det_filter(fa, s);
        for (const auto& e : io)
            if (e.out) HIP_CHECK(hipMemcpyAsync(e.host, e.dev, e.bytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aic_reid_infer(aic_model* mm, const float* crops, int n, int mem, float* emb, int out_mem) {
    return guarded([&] {
        AIC_REQUIRE(mm && n >= 0, AIC_ERR_INVALID, "bad argument");
        if (n == 0) return;
        AIC_REQUIRE(crops && emb, AIC_ERR_INVALID, "NULL argument");
        Model& m = mm->m;
        AIC_REQUIRE(m.kind == KIND_REID, AIC_ERR_INVALID, "not a ReID engine");
        m.dev->use();
        hipStream_t s = m.dev->s_main;
        // more crops than the activation arena holds: launch groups of max_items (reid_model.py:80-101 passes every valid
        // crop; a crowded frame must not fail or drop detections)
        const size_t per_in = (size_t)3 * m.in_h * m.in_w;
        for (int c0 = 0; c0 < n; c0 += m.max_items) {
            const int k = std::min(m.max_items, n - c0);
            load_input_nchw(m, crops + (size_t)c0 * per_in, k, mem, s);
            m.run(k, s);
            copy_out(emb + (size_t)c0 * m.out_dim, m.embeddings(), (size_t)k * m.out_dim * 4, out_mem, s);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aic_reid_infer_live(aic_model* mm, const float* crops, int n, int n_live, int mem, float* emb, int out_mem) {
    return guarded([&] {
        AIC_REQUIRE(mm && n >= 0 && n_live >= 0, AIC_ERR_INVALID, "bad argument");
        if (n == 0) return;
        AIC_REQUIRE(crops && emb, AIC_ERR_INVALID, "NULL argument");
        Model& m = mm->m;
        AIC_REQUIRE(m.kind == KIND_REID, AIC_ERR_INVALID, "not a ReID engine");
        AIC_REQUIRE(n <= m.max_items, AIC_ERR_INVALID, "more crops than the engine's max_items");
        m.dev->use();
        hipStream_t s = m.dev->s_main;
        DevBuf<int> d_live(1);
        const int live_host = n_live;                                     // the upload's source: lives until the stream is through
        HIP_CHECK(hipMemcpyAsync(d_live.p, &live_host, 4, hipMemcpyHostToDevice, s));
        m.n_items_dev = d_live.p;                                         // as the pipeline's device-filtered round sets it (pipeline.cpp)
        try {
            load_input_nchw(m, crops, n, mem, s);
            m.run(n, s);
        } catch (...) {
            m.n_items_dev = nullptr;
            (void)hipStreamSynchronize(s);
            throw;
        }
        m.n_items_dev = nullptr;
        copy_out(emb, m.embeddings(), (size_t)std::min(n, n_live) * m.out_dim * 4, out_mem, s);
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aic_letterbox(int device_id, const uint8_t* frame, int h, int w, int out_h, int out_w, float* out, float* ratio,
                  float* pad_w, float* pad_h) {
    return guarded([&] {
        AIC_REQUIRE(frame && out && h > 0 && w > 0 && out_h > 0 && out_w > 0, AIC_ERR_INVALID, "bad argument");
        Device& d = device(device_id);
        hipStream_t s = d.s_main;
        const LetterboxGeom g = letterbox_geometry(h, w, out_h, out_w);
        DevBuf<uint8_t> df((size_t)h * w * 3);
        DevBuf<float> dout((size_t)3 * out_h * out_w);
        HIP_CHECK(hipMemcpyAsync(df.p, frame, df.n, hipMemcpyHostToDevice, s));
        {
            Prof pr(d, PROF_LETTERBOX, s, 0, (double)h * w * 3 + 12.0 * out_h * out_w);
            launch_letterbox(df.p, 1, g, 0, AIC_F32, dout.p, s);
        }
        HIP_CHECK(hipMemcpyAsync(out, dout.p, dout.n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (ratio) *ratio = g.ratio;
        if (pad_w) *pad_w = g.pad_w;
        if (pad_h) *pad_h = g.pad_h;
    });
}

int aic_letterbox_image(int device_id, const uint8_t* frame, int h, int w, int unpad_h, int unpad_w, int top, int bottom, int left, int right,
                        int color_b, int color_g, int color_r, uint8_t* out) {
    return guarded([&] {
        AIC_REQUIRE(frame && out && h > 0 && w > 0 && unpad_h > 0 && unpad_w > 0, AIC_ERR_INVALID, "bad argument");
        AIC_REQUIRE(top >= 0 && bottom >= 0 && left >= 0 && right >= 0, AIC_ERR_INVALID, "negative border");   // cv2.copyMakeBorder refuses them too
        Device& d = device(device_id);
        hipStream_t s = d.s_main;
        LetterboxGeom g{};
        g.src_h = h, g.src_w = w, g.unpad_h = unpad_h, g.unpad_w = unpad_w, g.top = top, g.left = left;
        g.out_h = unpad_h + top + bottom, g.out_w = unpad_w + left + right;
        auto u8 = [](int v) { return v < 0 ? 0 : v > 255 ? 255 : v; };
        const int color[3] = {u8(color_b), u8(color_g), u8(color_r)};
        DevBuf<uint8_t> df((size_t)h * w * 3), dout((size_t)g.out_h * g.out_w * 3);
        HIP_CHECK(hipMemcpyAsync(df.p, frame, df.n, hipMemcpyHostToDevice, s));
        launch_letterbox_u8(df.p, g, color, dout.p, s);
        HIP_CHECK(hipMemcpyAsync(out, dout.p, dout.n, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aic_crop_resize(int device_id, const uint8_t* frame, int h, int w, const float* boxes, int n, int out_h, int out_w,
                    float* out, int32_t* valid) {
    return guarded([&] {
        AIC_REQUIRE(n >= 0 && h > 0 && w > 0 && out_h > 0 && out_w > 0, AIC_ERR_INVALID, "bad argument");
        if (n == 0) return;
        AIC_REQUIRE(frame && boxes && out, AIC_ERR_INVALID, "NULL argument");
        Device& d = device(device_id);
        hipStream_t s = d.s_main;
        DevBuf<uint8_t> df((size_t)h * w * 3);
        DevBuf<float> db((size_t)n * 4), dout((size_t)n * 3 * out_h * out_w);
        DevBuf<int> dv(n);
        HIP_CHECK(hipMemcpyAsync(df.p, frame, df.n, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(db.p, boxes, (size_t)n * 16, hipMemcpyHostToDevice, s));
        {
            Prof pr(d, PROF_CROP, s, 0, (double)n * out_h * out_w * 15);
            launch_crop_resize(df.p, h, w, db.p, nullptr, n, nullptr, out_h, out_w, 0, AIC_F32, dout.p, dv.p, s);
        }
        HIP_CHECK(hipMemcpyAsync(out, dout.p, dout.n * 4, hipMemcpyDeviceToHost, s));
        if (valid) HIP_CHECK(hipMemcpyAsync(valid, dv.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

// aic_detect; n_live >= 0 (aic_detect_live): with a device-side frame count holding n_live in force
static void detect_frames(aic_model* mm, const uint8_t* frames, int batch, int h, int w, int mem, float conf, float iou, int max_det,
                          int32_t* num_dets, float* boxes, float* scores, int32_t* labels, int n_live) {
    {
        AIC_REQUIRE(mm && frames && batch > 0 && h > 0 && w > 0, AIC_ERR_INVALID, "bad argument");
        Model& m = mm->m;
        AIC_REQUIRE(m.kind == KIND_YOLO, AIC_ERR_INVALID, "not a YOLO engine");
        AIC_REQUIRE(batch <= m.max_items, AIC_ERR_CAPACITY, "batch exceeds the engine's max_items");
        m.dev->use();
        hipStream_t s = m.dev->s_main;
        const uint8_t* df = stage_frames(m, frames, (size_t)batch * h * w * 3, mem, s);
        const LetterboxGeom g = letterbox_geometry(h, w, m.in_h, m.in_w);
        DevBuf<int> d_live;
        const int live_host = n_live;                                     // the upload's source: lives until the stream is through
        if (n_live >= 0) {
            d_live.alloc(1);
            HIP_CHECK(hipMemcpyAsync(d_live.p, &live_host, 4, hipMemcpyHostToDevice, s));
            m.n_items_dev = d_live.p;
        }
        m.reduce_cls = true;
        m.arm_sparse_box(conf);                 // the box branches may run at the anchors this call's NMS will read, and nowhere else
        m.side_ok = true;
        try {
            m.run_frames(df, batch, g, s);
        } catch (...) {
            m.side_ok = false, m.n_items_dev = nullptr;
            (void)hipStreamSynchronize(s);
            throw;
        }
        m.side_ok = false, m.n_items_dev = nullptr;
        if (n_live >= 0) batch = std::min(batch, n_live);                 // frames at and past the live count were not computed
        if (batch == 0) {
            HIP_CHECK(hipStreamSynchronize(s));
            return;
        }
        if (batch <= 4 && num_dets && boxes && scores && labels) {
            // the per-frame plugin loop: the NMS kernel stores what it keeps into page-locked host memory itself
            const size_t per = (size_t)max_det * 24;
            m.h_det.ensure((size_t)batch * (4 + per) + 16);
            m.decode_nms(batch, conf, iou, max_det, &g, s, m.h_det.p);
            HIP_CHECK(hipStreamSynchronize(s));
            scatter_dets(m.h_det.p, batch, max_det, num_dets, boxes, scores, labels);
            return;
        }
        m.decode_nms(batch, conf, iou, max_det, &g, s);
        copy_out_dets(m, batch, max_det, m.d_out_boxes_orig.p, num_dets, boxes, scores, labels, s);
    }
}

int aic_detect(aic_model* mm, const uint8_t* frames, int batch, int h, int w, int mem, float conf, float iou, int max_det,
               int32_t* num_dets, float* boxes, float* scores, int32_t* labels) {
    return guarded([&] { detect_frames(mm, frames, batch, h, w, mem, conf, iou, max_det, num_dets, boxes, scores, labels, -1); });
}

int aic_detect_live(aic_model* mm, const uint8_t* frames, int batch, int n_live, int h, int w, int mem, float conf, float iou, int max_det,
                    int32_t* num_dets, float* boxes, float* scores, int32_t* labels) {
    return guarded([&] {
        AIC_REQUIRE(n_live >= 0, AIC_ERR_INVALID, "bad argument");
        detect_frames(mm, frames, batch, h, w, mem, conf, iou, max_det, num_dets, boxes, scores, labels, n_live);
    });
}

int aic_detect_decode(aic_model* mm, int batch, int h, int w, float conf, float iou, int max_det, int32_t* num_dets, float* boxes,
                      float* scores, int32_t* labels) {
    return guarded([&] {
        AIC_REQUIRE(mm && batch > 0 && h > 0 && w > 0, AIC_ERR_INVALID, "bad argument");
        Model& m = mm->m;
        AIC_REQUIRE(m.kind == KIND_YOLO, AIC_ERR_INVALID, "not a YOLO engine");
        AIC_REQUIRE(m.reduce_cls && batch <= m.last_n, AIC_ERR_INVALID, "no detect run on that many frames to decode again");
        m.dev->use();
        hipStream_t s = m.dev->s_main;
        const LetterboxGeom g = letterbox_geometry(h, w, m.in_h, m.in_w);
        m.decode_nms(batch, conf, iou, max_det, &g, s);
        copy_out_dets(m, batch, max_det, m.d_out_boxes_orig.p, num_dets, boxes, scores, labels, s);
    });
}

int aic_model_sparse_box(aic_model* mm, int force, int32_t* out) {
    return guarded([&] {
        AIC_REQUIRE(mm && mm->m.kind == KIND_YOLO, AIC_ERR_INVALID, "not a YOLO engine");
        Model& m = mm->m;
        if (force >= 0) m.sp_force = force != 0;
        if (!out) return;
        std::fill(out, out + 8, 0);
        out[0] = m.sp_listed, out[5] = m.sp_pass, out[6] = m.sbx.ok, out[7] = m.sbx.ok && m.sbx.lead0 >= 0;
        if (m.sp_pass) {                        // the counts themselves, from the device (what the path choice knows may be a run older)
            m.dev->use();
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(out + 1, m.d_sp_count.p, 16, hipMemcpyDeviceToHost));
        }
    });
}

int aic_model_read_det(aic_model* mm, int n, float* boxes, float* max_logit, int32_t* labels) {
    return guarded([&] {
        AIC_REQUIRE(mm && mm->m.kind == KIND_YOLO && n > 0 && n <= mm->m.max_items, AIC_ERR_INVALID, "bad argument");
        Model& m = mm->m;
        m.dev->use();
        HIP_CHECK(hipDeviceSynchronize());
        const size_t ba = (size_t)n * m.n_anchors;
        if (boxes) HIP_CHECK(hipMemcpy(boxes, m.d_boxes.p, ba * 16, hipMemcpyDeviceToHost));
        if (max_logit) HIP_CHECK(hipMemcpy(max_logit, m.d_maxlogit.p, ba * 4, hipMemcpyDeviceToHost));
        if (labels) HIP_CHECK(hipMemcpy(labels, m.d_labels.p, ba * 4, hipMemcpyDeviceToHost));
    });
}

int aic_reid_embed(aic_model* mm, const uint8_t* frame, int h, int w, int mem, const float* boxes, int n, float* emb,
                   int32_t* valid) {
    return guarded([&] {
        AIC_REQUIRE(mm && n >= 0 && h > 0 && w > 0, AIC_ERR_INVALID, "bad argument");
        if (n == 0) return;
        AIC_REQUIRE(frame && boxes && emb, AIC_ERR_INVALID, "NULL argument");
        Model& m = mm->m;
        AIC_REQUIRE(m.kind == KIND_REID, AIC_ERR_INVALID, "not a ReID engine");
        m.dev->use();
        hipStream_t s = m.dev->s_main;
        const uint8_t* df = stage_frames(m, frame, (size_t)h * w * 3, mem, s);
        m.d_crop_boxes.ensure((size_t)n * 4);
        m.d_valid.ensure(n);
        HIP_CHECK(hipMemcpyAsync(m.d_crop_boxes.p, boxes, (size_t)n * 16, hipMemcpyHostToDevice, s));
        m.in_pix4 = m.input_pix4_ok();
        const BufDesc& eb = m.bufs[m.outs[0].v[0]];
        if (n <= m.max_items && n <= 512 && m.in_pix4 && m.in_h <= 192 && mem != AIC_DEVICE && eb.f32 &&
            eb.c == m.out_dim && m.outs[0].v[2] == 0 && m.ops.back().v[0] == OP_L2NORM && m.ops.back().v[5] == 0) {
            // the per-frame plugin loop: embeddings and crop validity are stored into page-locked host memory by the kernels that produce them
            const size_t eb_bytes = (size_t)n * m.out_dim * 4;
            m.h_emb.ensure(eb_bytes + (size_t)n * 4 + 16);
            int* hv = reinterpret_cast<int*>(m.h_emb.p + eb_bytes);
            m.crop_src = CropSrc{df, h, w, m.d_crop_boxes.p, nullptr, hv};
            m.emb_host_out = reinterpret_cast<float*>(m.h_emb.p);
            try {
                m.run(n, s);
            } catch (...) {
                m.crop_src.frames = nullptr, m.emb_host_out = nullptr;
                throw;
            }
            m.crop_src.frames = nullptr, m.emb_host_out = nullptr;
            HIP_CHECK(hipStreamSynchronize(s));
            std::memcpy(emb, m.h_emb.p, eb_bytes);
            if (valid) std::memcpy(valid, hv, (size_t)n * 4);
            return;
        }
        for (int c0 = 0; c0 < n; c0 += m.max_items) {   // launch groups of max_items: every detection is embedded (deepsort_tracker.py:104-113)
            const int k = std::min(m.max_items, n - c0);
            if (m.in_pix4 && m.in_h <= 192 && mem != AIC_DEVICE) {
                // crop + resize + normalise inside the stem kernel, as the pipeline does it (same arithmetic, pixel for pixel): one launch fewer
                // per call of the per-frame plugin loop, and no crop tensor.  (A caller's own device buffer keeps the separate crop kernel:
                // the fused form's aligned 12-byte reads want 16 bytes of slack behind the frame, which only our staging buffer promises.)
                m.crop_src = CropSrc{df, h, w, m.d_crop_boxes.p + (size_t)c0 * 4, nullptr, m.d_valid.p + c0};
            } else {
                Prof pr(*m.dev, PROF_CROP, s, 0, (double)k * m.in_h * m.in_w * 19);
                launch_crop_resize(df, h, w, m.d_crop_boxes.p + (size_t)c0 * 4, nullptr, k, nullptr, m.in_h, m.in_w, m.in_pix4 ? 2 : 1, m.dtype,
                                   m.input(), m.d_valid.p + c0, s);
            }
            m.run(k, s);
            m.crop_src.frames = nullptr;
            copy_out(emb + (size_t)c0 * m.out_dim, m.embeddings(), (size_t)k * m.out_dim * 4, AIC_HOST, s);
        }
        if (valid) HIP_CHECK(hipMemcpyAsync(valid, m.d_valid.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

}  // extern "C"

namespace {

// The staging of the two parity-test entries below: a bank of n_frames frames that starts byte_offset (0..3) bytes into a device buffer
// filled with a non-zero byte, so that a tap taken from outside the bank shows as a wrong VALUE; with `slack` 16 of those bytes follow
// the bank (what the aligned 12-byte loads of the wide crop path and of the fused stem are promised), without it the buffer ends with
// the bank.  frame_of (may be NULL) is checked against the bank on the host: no kernel ever sees an index outside it.
struct TestBank {
    DevBuf<uint8_t> buf;
    DevBuf<int> frame_of, n_live;
    int n_live_host = 0;                 // the upload's source: lives as long as the bank
    const uint8_t* frames = nullptr;
};

void stage_test_bank(TestBank& tb, const uint8_t* frames, int n_frames, int h, int w, int byte_offset, bool slack, const int32_t* frame_of,
                     int n, int n_live, hipStream_t s) {
    AIC_REQUIRE(frames && n_frames > 0 && h > 0 && w > 0 && byte_offset >= 0 && byte_offset <= 3, AIC_ERR_INVALID, "bad bank");
    const size_t bytes = (size_t)n_frames * h * w * 3;
    AIC_REQUIRE(bytes < ((size_t)1 << 31), AIC_ERR_INVALID, "bank too large");
    if (frame_of)
        for (int i = 0; i < n; ++i) AIC_REQUIRE(frame_of[i] >= 0 && frame_of[i] < n_frames, AIC_ERR_INVALID, "frame_of outside the bank");
    tb.buf.alloc((size_t)byte_offset + bytes + (slack ? 16 : 0));
    HIP_CHECK(hipMemsetAsync(tb.buf.p, 0xA5, tb.buf.n, s));
    tb.frames = tb.buf.p + byte_offset;
    HIP_CHECK(hipMemcpyAsync(tb.buf.p + byte_offset, frames, bytes, hipMemcpyHostToDevice, s));
    if (frame_of) {
        tb.frame_of.alloc(n);
        HIP_CHECK(hipMemcpyAsync(tb.frame_of.p, frame_of, (size_t)n * 4, hipMemcpyHostToDevice, s));
    }
    if (n_live >= 0) {
        tb.n_live.alloc(1);
        tb.n_live_host = n_live;
        HIP_CHECK(hipMemcpyAsync(tb.n_live.p, &tb.n_live_host, 4, hipMemcpyHostToDevice, s));
    }
}

}  // namespace

extern "C" {

int aic_crop_resize_ex(int device_id, const uint8_t* frames, int n_frames, int h, int w, int byte_offset, const float* boxes,
                       const int32_t* frame_of, int n, int n_live, int out_h, int out_w, int mode, int dtype, int slack, void* out,
                       int32_t* valid) {
    return guarded([&] {
        AIC_REQUIRE(n >= 0 && out_h > 0 && out_w > 0 && mode >= 0 && mode <= 2 && (dtype == AIC_F32 || dtype == AIC_F16), AIC_ERR_INVALID, "bad argument");
        AIC_REQUIRE(mode != 0 || dtype == AIC_F32, AIC_ERR_INVALID, "the NCHW layout is fp32");
        if (n == 0) return;
        AIC_REQUIRE(boxes && out && valid, AIC_ERR_INVALID, "NULL argument");
        Device& d = device(device_id);
        hipStream_t s = d.s_main;
        TestBank tb;
        stage_test_bank(tb, frames, n_frames, h, w, byte_offset, slack != 0, frame_of, n, n_live, s);
        const size_t px = (size_t)n * out_h * out_w;
        const size_t out_bytes = mode == 0 ? px * 3 * 4 : mode == 1 ? px * 8 * (dtype == AIC_F16 ? 2 : 4) : px * 4 * 2;
        DevBuf<float> db((size_t)n * 4);
        DevBuf<char> dout(out_bytes);
        DevBuf<int> dv(n);
        HIP_CHECK(hipMemcpyAsync(db.p, boxes, (size_t)n * 16, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(dout.p, 0xFF, out_bytes, s));           // an element no thread stores keeps this pattern
        HIP_CHECK(hipMemsetAsync(dv.p, 0xFF, (size_t)n * 4, s));         // = -1
        try {
            launch_crop_resize(tb.frames, h, w, db.p, tb.frame_of.p, n, tb.n_live.p, out_h, out_w, mode, dtype, dout.p, dv.p, s, slack != 0);
        } catch (...) {
            (void)hipStreamSynchronize(s);                                // the staging copies read the caller's arrays
            throw;
        }
        HIP_CHECK(hipMemcpyAsync(out, dout.p, out_bytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(valid, dv.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aic_reid_embed_bank(aic_model* mm, const uint8_t* frames, int n_frames, int h, int w, int byte_offset, const float* boxes,
                        const int32_t* frame_of, int n, int n_live, float* emb, int32_t* valid) {
    return guarded([&] {
        AIC_REQUIRE(mm && n >= 0, AIC_ERR_INVALID, "bad argument");
        if (n == 0) return;
        AIC_REQUIRE(boxes && emb && valid, AIC_ERR_INVALID, "NULL argument");
        Model& m = mm->m;
        AIC_REQUIRE(m.kind == KIND_REID && m.dtype == AIC_F16 && m.input_pix4_ok() && reid_stem2_usable(m.in_h, m.in_w) && m.in_h <= 192,
                    AIC_ERR_INVALID, "this engine does not take the fused crop");
        AIC_REQUIRE(n <= m.max_items, AIC_ERR_INVALID, "more crops than the engine's max_items");
        m.dev->use();
        hipStream_t s = m.dev->s_main;
        TestBank tb;
        stage_test_bank(tb, frames, n_frames, h, w, byte_offset, true, frame_of, n, n_live, s);
        m.d_crop_boxes.ensure((size_t)n * 4);
        m.d_valid.ensure(n);
        HIP_CHECK(hipMemcpyAsync(m.d_crop_boxes.p, boxes, (size_t)n * 16, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(m.d_valid.p, 0xFF, (size_t)n * 4, s));
        // as the pipeline's device-filtered round sets it (pipeline.cpp, stage_a_device_filter)
        m.in_pix4 = true;
        m.crop_src = CropSrc{tb.frames, h, w, m.d_crop_boxes.p, tb.frame_of.p, m.d_valid.p};
        m.n_items_dev = tb.n_live.p;
        try {
            m.run(n, s);
        } catch (...) {
            m.crop_src.frames = nullptr, m.n_items_dev = nullptr;
            (void)hipStreamSynchronize(s);
            throw;
        }
        m.crop_src.frames = nullptr, m.n_items_dev = nullptr;
        copy_out(emb, m.embeddings(), (size_t)n * m.out_dim * 4, AIC_HOST, s);
        HIP_CHECK(hipMemcpyAsync(valid, m.d_valid.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

}  // extern "C"
