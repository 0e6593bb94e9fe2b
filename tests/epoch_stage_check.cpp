// epoch_stage_check.cpp -- stand-alone check of ai-camera_amd/csrc/epoch_stage.hpp on the CPU (tests/test_epoch_stage_host.py builds it with
// the system g++ under the address and undefined-behaviour sanitizers and reads what it prints).
//   layout lines   "<site> <parameters> | <field>=<offset>:<bytes> ... bytes=<size>" for the layout of every call site, built with the
//                  structs the call sites build theirs with, over the cross product of the test's cases;
//   fill lines     DetBlock::fill / fill_valid on three frames of 2, 0 and 3 detections, in exact-size buffers;
//   deliver lines  deliver() on two streams of 2 and 3 frames.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ai-camera_amd/csrc/epoch_stage.hpp"

using namespace aic;

static void field(const char* name, size_t off, size_t bytes) { printf(" %s=%zu:%zu", name, off, bytes); }

static void det_fields(const DetBlock& d) {
    field("frame_n", d.o_n, d.F * 4), field("frame_d0", d.o_d0, d.F * 4), field("tlwh", d.o_tlwh, d.n * 16);
    field("conf", d.o_conf, d.n * 4), field("cls", d.o_cls, d.n * 4);
    if (d.has_valid) field("valid", d.o_valid, d.n * 4);
}

static void out_fields(const OutBlock& o, size_t F) {
    field("n_tracks", o.o_out, F * 4), field("rows", o.o_rows, F * o.cap * 24), field("oconf", o.o_conf, F * o.cap * 4);
}

static void layouts() {
    const int Ss[] = {1, 2, 3, 256}, caps[] = {0, 1, 7}, dims[] = {0, 4, 512};
    const size_t Fs[] = {0, 1, 3, 5, 17}, ns[] = {0, 1, 3, 4, 5, 513}, Es[] = {0, 1, 3};
    for (size_t F : Fs)
        for (size_t n : ns)
            for (int cap : caps) {
                for (int dbg : {0, 2 * TRK_DEV_TMAX + 8}) {       // update_device is k = 1, cap = TRK_DEV_TMAX, dbg = 0: its own lines below
                    const CallStage L = tracker_stage(F, n, cap, dbg);
                    printf("tracker F=%zu n=%zu cap=%d dbg=%d |", F, n, cap, dbg);
                    det_fields(L.det), out_fields(L.out, F);
                    if (dbg) field("dbg", L.o_tail, F * dbg * 4);
                    printf(" bytes=%zu\n", L.bytes);
                }
                {
                    StageCursor c;
                    const OutBlock ob(c, F, cap);                 // stage_b_device
                    printf("pipeline F=%zu cap=%d |", F, cap);
                    out_fields(ob, F);
                    printf(" bytes=%zu\n", ob.end);
                }
                for (int S : Ss)
                    for (int dim : dims) {
                        for (int x = 0; x < 8; ++x) {
                            const bool valid = x & 1, warps = x & 2, feat = x & 4;
                            const CallStage L = bank_stage(S, F, n, cap, valid, warps, feat, dim);
                            printf("bank S=%d F=%zu n=%zu cap=%d dim=%d valid=%d warps=%d feat=%d |", S, F, n, cap, dim, valid, warps, feat);
                            field("plan", 0, (size_t)S * 8), det_fields(L.det);
                            if (warps) field("warps", L.o_warp, F * 24);
                            if (L.has_feat) field("feat", L.o_feat, L.feat_bytes);
                            out_fields(L.out, F), field("feat_n", L.o_featn, L.feat_bytes);
                            printf(" bytes=%zu\n", L.bytes);
                        }
                        for (size_t E : Es)
                            for (int feats = 0; feats < 2; ++feats) {
                                StageCursor c;
                                const DeepSortPlanBlock pb(c, E, S, F, n);
                                const CallStage L = deepsort_stage(c, S, F, n, cap, feats, dim);
                                printf("deepsort S=%d F=%zu n=%zu cap=%d dim=%d E=%zu feats=%d |", S, F, n, cap, dim, E, feats);
                                field("plans", 0, E * S * sizeof(EpochStreamPlan)), field("row_map", pb.o_map, n * 4);
                                field("frame_e0", pb.o_e0, F * 4), field("stream_f0", pb.o_f0, (size_t)S * 4);
                                field("stream_k", pb.o_k, (size_t)S * 4), det_fields(L.det), field("feat", L.o_feat, L.feat_bytes);
                                out_fields(L.out, F), field("hdr", L.o_tail, S * sizeof(DevTrkHdr)), field("feat_n", L.o_featn, L.feat_bytes);
                                printf(" bytes=%zu\n", L.bytes);
                            }
                    }
            }
    for (size_t n : ns) {
        const CallStage L = tracker_stage(1, n, TRK_DEV_TMAX, 0);
        printf("update_device n=%zu |", n);
        det_fields(L.det), out_fields(L.out, 1);
        printf(" bytes=%zu\n", L.bytes);
    }
}

template <class T>
static void print_row(const char* name, const T* p, size_t count, const char* fmt) {
    printf("%s", name);
    for (size_t i = 0; i < count; ++i) printf(fmt, p[i]);
    printf("\n");
}

static void print_bits(const char* name, const float* p, size_t count) {
    printf("%s", name);
    for (size_t i = 0; i < count; ++i) {
        uint32_t u;
        std::memcpy(&u, p + i, 4);
        printf(" %08x", u);
    }
    printf("\n");
}

static void fills() {
    const int32_t counts[3] = {2, 0, 3}, cls[5] = {0, 1, 2, 3, 4};
    const float boxes[20] = {0.1f, 0.2f, 0.7f, 1.3f, 1e7f, -3.3f, 1e7f + 3.f, 0.1f, 5.5f, 6.25f, 5.6f, 1e-3f, 100.3f, 7.f, 33.33f, 7.1f, 0.f, 0.f, 1e-8f, 3e8f};
    const float conf[5] = {0.9f, 0.8f, 0.7f, 0.6f, 0.5f};
    print_bits("fill boxes", boxes, 20);
    for (int xyxy = 0; xyxy < 2; ++xyxy) {
        const CallStage L = tracker_stage(3, 5, 2, 0);
        std::vector<char> h(L.out.o_out);                          // the input half, to the byte
        L.det.fill(h.data(), counts, boxes, xyxy != 0, conf, cls);
        print_row(xyxy ? "fill xyxy frame_n" : "fill tlwh frame_n", L.det.host_n(h.data()), 3, " %d");
        print_row(xyxy ? "fill xyxy frame_d0" : "fill tlwh frame_d0", L.det.host_d0(h.data()), 3, " %d");
        print_bits(xyxy ? "fill xyxy tlwh" : "fill tlwh tlwh", reinterpret_cast<const float*>(h.data() + L.det.o_tlwh), 20);
        print_bits(xyxy ? "fill xyxy conf" : "fill tlwh conf", reinterpret_cast<const float*>(h.data() + L.det.o_conf), 5);
        print_row(xyxy ? "fill xyxy cls" : "fill tlwh cls", reinterpret_cast<const int32_t*>(h.data() + L.det.o_cls), 5, " %d");
        const uint8_t has[5] = {1, 0, 1, 1, 0};
        const int32_t* hv = reinterpret_cast<const int32_t*>(h.data() + L.det.o_valid);
        L.det.fill_valid(h.data(), true, (const uint8_t*)nullptr);
        print_row("valid has=NULL", hv, 5, " %d");
        L.det.fill_valid(h.data(), true, has);
        print_row("valid has=mixed", hv, 5, " %d");
        L.det.fill_valid(h.data(), false, has);
        print_row("valid no_features", hv, 5, " %d");
    }
}

static void delivery() {
    const int S = 2, cap = 2, F = 5;
    const int32_t fps[S] = {2, 3}, counts[F] = {1, 3, 0, 2, 5}, good[S] = {2, 1};
    StageCursor c;
    const OutBlock ob(c, F, cap);
    std::vector<char> h(ob.end);
    int32_t* hn = reinterpret_cast<int32_t*>(h.data() + ob.o_out);
    int32_t* hr = reinterpret_cast<int32_t*>(h.data() + ob.o_rows);
    float* hc = reinterpret_cast<float*>(h.data() + ob.o_conf);
    for (int f = 0; f < F; ++f) {
        hn[f] = counts[f];
        for (int j = 0; j < cap * 6; ++j) hr[f * cap * 6 + j] = 1000 * (f + 1) + j;
        for (int r = 0; r < cap; ++r) hc[f * cap + r] = 10.f * (f + 1) + r + 0.5f;
    }
    std::vector<int32_t> n_out(F, -77), out6((size_t)F * cap * 6, -77);
    std::vector<float> out_conf((size_t)F * cap, -77.f);
    deliver(ob.host(h.data()), cap, S, fps, [&](int q, int i) { return i < good[q]; }, n_out.data(), out6.data(), out_conf.data());
    print_row("deliver n_out", n_out.data(), n_out.size(), " %d");
    print_row("deliver out6", out6.data(), out6.size(), " %d");
    print_row("deliver out_conf", out_conf.data(), out_conf.size(), " %g");
    deliver(ob.host(h.data()), cap, S, fps, [](int, int) { return true; }, nullptr, nullptr, nullptr);   // every destination is optional
}

static void checks() {
    const int32_t fps[2] = {2, 3}, ok[5] = {1, 3, 0, 2, 512}, neg[5] = {1, -1, 0, 2, 5}, big[5] = {1, 513, 0, 2, 5}, bad_fps[2] = {2, -3};
    auto show = [](const char* what, const CallShape& c) {
        printf("check %s | F=%ld kmax_s=%d total=%ld nmax=%d capacity=%d err=%s\n", what, c.F, c.kmax_s, c.total, c.nmax, (int)c.capacity, c.err.c_str());
    };
    show("ok", check_call("X", 2, fps, ok, true));
    show("negative_frames", check_call("X", 2, bad_fps, ok, true));
    show("negative_count", check_call("X", 2, fps, neg, true));
    show("too_many", check_call("X", 2, fps, big, true));
    show("no_arrays", check_call("X", 2, fps, ok, false));
    show("max_total", check_call("X", 2, fps, ok, false, 518));
}

int main() {
    layouts();
    fills();
    delivery();
    checks();
    return 0;
}
