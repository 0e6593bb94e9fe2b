// trk_math_probe.cpp -- the scalar pieces of ai-camera_amd/csrc/trk_math.hpp on the CPU: a stand-alone program that
// tests/test_trk_math_host.py builds with the system compiler (-ffp-contract=off) under the address and undefined-behaviour sanitizers
// and runs as a child process.  usage: trk_math_probe <jobs> <results>.  Both files are raw little-endian int32 / float32.
// A job is a header (op, n, m, flag as int32; dt as float32) and its payload; the results follow each other in job order:
//   0 initiate   z [n, 4]                                       -> mean [n, 8], cov [n, 64]
//   1 predict    mean [n, 8], cov [n, 64]; dt                   -> mean, cov
//   2 project    mean, cov                                      -> mean [n, 4], S [n, 16]
//   3 update     mean, cov, z [n, 4]                            -> mean, cov of the wave form; mean, cov of the row form
//   4 gating     mean, cov, zs [m, 4] (flag & 1) or [n, m, 4]   -> d2 [n, m]; flag & 2: the position block alone
//   5 boxes      mean [n, 8], tlwh [m, 4]                       -> mean_box [n, 4], iou_dist [n, m]
// The wave form is kf_*_wave emulated: the per-lane compute part for lanes 0 .. 63 on the state as it was, then the stores.  The row form
// is the thread-per-row update of trk_epoch_kernel: gain row, S K and the mean element once per row, then kf_cov_elem per element.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ai-camera_amd/csrc/trk_math.hpp"

using namespace aic;

static std::vector<float> take(FILE* f, size_t count) {
    std::vector<float> v(count);
    if (count && std::fread(v.data(), 4, count, f) != count) { std::fprintf(stderr, "short job file\n"); std::exit(2); }
    return v;
}
static void put(FILE* f, const float* p, size_t count) {
    if (count && std::fwrite(p, 4, count, f) != count) { std::fprintf(stderr, "short write\n"); std::exit(2); }
}

// the stores of a wave wrapper, after every lane has its values
static void store_wave(float* P, float* m, const float pij[64], const float mi[64]) {
    for (int lane = 0; lane < 64; ++lane) {
        P[lane] = pij[lane];
        if ((lane & 7) == 0) m[lane >> 3] = mi[lane];
    }
}

static void update_rows(float* P, float* m, const float* zz) {
    float ks[8][9];                                 // K[i][0..3], (S K[i])[0..3], new mean[i]
    for (int i = 0; i < 8; ++i) {
        float S[4][4], L[4][4], Ki[4], u[4];
        innovation_cov(P, m[3], S);
        cholesky<4>(S, L);
        kf_gain_row(L, P, i, Ki);
        kf_s_gain(S, Ki, u);
        for (int q = 0; q < 4; ++q) ks[i][q] = Ki[q], ks[i][4 + q] = u[q];
        ks[i][8] = kf_mean_elem(m, zz, Ki, i);
    }
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) P[i * 8 + j] = kf_cov_elem(P[i * 8 + j], ks[i], ks[j] + 4);
    for (int i = 0; i < 8; ++i) m[i] = ks[i][8];
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: trk_math_probe <jobs> <results>\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t hd[4];
    float pij[64], mi[64];
    while (std::fread(hd, 4, 4, in) == 4) {
        const int op = hd[0], n = hd[1], m = hd[2], flag = hd[3];
        const float dt = take(in, 1)[0];
        if (n < 0 || m < 0 || n > (1 << 16) || m > (1 << 16)) { std::fprintf(stderr, "bad job\n"); return 2; }
        if (op == 0) {
            const std::vector<float> z = take(in, (size_t)n * 4);
            std::vector<float> mean((size_t)n * 8), cov((size_t)n * 64);
            for (int k = 0; k < n; ++k) {
                for (int lane = 0; lane < 64; ++lane) kf_initiate_lane(&z[(size_t)k * 4], lane >> 3, lane & 7, pij[lane], mi[lane]);
                store_wave(&cov[(size_t)k * 64], &mean[(size_t)k * 8], pij, mi);
            }
            put(out, mean.data(), mean.size()), put(out, cov.data(), cov.size());
        } else if (op == 5) {
            const std::vector<float> mean = take(in, (size_t)n * 8), det = take(in, (size_t)m * 4);
            std::vector<float> box((size_t)n * 4), cost((size_t)n * m);
            for (int k = 0; k < n; ++k) {
                mean_box(&mean[(size_t)k * 8], &box[(size_t)k * 4]);
                for (int j = 0; j < m; ++j) cost[(size_t)k * m + j] = iou_dist(&box[(size_t)k * 4], &det[(size_t)j * 4]);
            }
            put(out, box.data(), box.size()), put(out, cost.data(), cost.size());
        } else if (op >= 1 && op <= 4) {
            std::vector<float> mean = take(in, (size_t)n * 8), cov = take(in, (size_t)n * 64);
            if (op == 1) {
                for (int k = 0; k < n; ++k) {
                    float* P = &cov[(size_t)k * 64];
                    float* mu = &mean[(size_t)k * 8];
                    for (int lane = 0; lane < 64; ++lane) kf_predict_lane(P, mu, lane >> 3, lane & 7, dt, pij[lane], mi[lane]);
                    store_wave(P, mu, pij, mi);
                }
                put(out, mean.data(), mean.size()), put(out, cov.data(), cov.size());
            } else if (op == 2) {
                std::vector<float> pm((size_t)n * 4), ps((size_t)n * 16);
                for (int k = 0; k < n; ++k) {
                    float S[4][4];
                    innovation_cov(&cov[(size_t)k * 64], mean[(size_t)k * 8 + 3], S);
                    for (int a = 0; a < 4; ++a) {
                        pm[(size_t)k * 4 + a] = mean[(size_t)k * 8 + a];
                        for (int b = 0; b < 4; ++b) ps[(size_t)k * 16 + a * 4 + b] = S[a][b];
                    }
                }
                put(out, pm.data(), pm.size()), put(out, ps.data(), ps.size());
            } else if (op == 3) {
                const std::vector<float> z = take(in, (size_t)n * 4);
                std::vector<float> mean2 = mean, cov2 = cov;
                for (int k = 0; k < n; ++k) {
                    float* P = &cov[(size_t)k * 64];
                    float* mu = &mean[(size_t)k * 8];
                    for (int lane = 0; lane < 64; ++lane) kf_update_lane(P, mu, &z[(size_t)k * 4], lane >> 3, lane & 7, pij[lane], mi[lane]);
                    store_wave(P, mu, pij, mi);
                    update_rows(&cov2[(size_t)k * 64], &mean2[(size_t)k * 8], &z[(size_t)k * 4]);
                }
                put(out, mean.data(), mean.size()), put(out, cov.data(), cov.size());
                put(out, mean2.data(), mean2.size()), put(out, cov2.data(), cov2.size());
            } else {
                const bool shared = flag & 1, pos = flag & 2;
                const std::vector<float> zs = take(in, (size_t)(shared ? 1 : n) * m * 4);
                std::vector<float> d2((size_t)n * m);
                for (int k = 0; k < n; ++k) {
                    const float* mu = &mean[(size_t)k * 8];
                    float S[4][4], L[4][4];
                    innovation_cov(&cov[(size_t)k * 64], mu[3], S);
                    const bool ok = pos ? cholesky<2>(S, L) : cholesky<4>(S, L);
                    for (int j = 0; j < m; ++j) {
                        const float* z = &zs[((size_t)(shared ? 0 : k) * m + j) * 4];
                        float acc;
                        if (pos) {                  // kf_gating_kernel's own branch, restated
                            float d[4], y[4];
                            for (int a = 0; a < 4; ++a) d[a] = z[a] - mu[a];
                            fwd_solve<2>(L, d, y);
                            acc = y[0] * y[0] + y[1] * y[1];
                            if (!ok) acc = __builtin_inff();
                        } else {
                            acc = maha4(L, ok, mu, z);
                        }
                        d2[(size_t)k * m + j] = acc;
                    }
                }
                put(out, d2.data(), d2.size());
            }
        } else {
            std::fprintf(stderr, "unknown op %d\n", op);
            return 2;
        }
    }
    if (std::fclose(out) != 0) return 2;
    std::fclose(in);
    return 0;
}
