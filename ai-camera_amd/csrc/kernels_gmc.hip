// kernels_gmc.hip -- camera-motion estimation (gfx950): gray pyramid level, integer block matching, robust similarity fit.
// The specification is tests/gmc_oracle.py (steps 1-8 there); every result is np.array_equal to it: the sums are integers, the fp64
// sequence of the fit runs in the stated order (-ffp-contract=off) and the residuals are one fixed expression per block.
#include "gmc.hpp"

namespace aic {

struct __attribute__((packed)) GmcU128 { uint32_t v[4]; };   // a 16-byte load from any byte address (rows of 3 W bytes are not aligned)
struct __attribute__((packed)) GmcU32 { uint32_t v; };       // ... and a dword at any byte address (gray rows of W / s bytes)

// ---------------------------------------------------------------------------------------------------------------- step 1
// One thread per 16 frame pixels of one gray row: S rows of 48 bytes (three 16-byte loads each) -> 16 / S gray pixels.
template <int S>
__global__ __launch_bounds__(256) void gmc_gray_kernel(const uint8_t* __restrict__ frames, int h, int w, int gh, int gw, size_t level,
                                                       uint8_t* __restrict__ gray) {
    constexpr int NG = 16 / S;
    constexpr int SH = S == 4 ? 12 : 10;
    const int spans = (gw + NG - 1) / NG;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= gh * spans) return;
    const int gy = t / spans, sp = t - gy * spans;
    const size_t row = (size_t)w * 3;
    const uint8_t* src = frames + ((size_t)blockIdx.y * h + (size_t)gy * S) * row + (size_t)sp * 48;
    uint8_t* dst = gray + (size_t)blockIdx.y * level + (size_t)gy * gw + sp * NG;
    const int ng = min(NG, gw - sp * NG);
    int acc[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) acc[j] = 0;
    if (ng == NG) {
#pragma unroll
        for (int r = 0; r < S; ++r) {
            uint32_t d[12];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const GmcU128 u = *reinterpret_cast<const GmcU128*>(src + r * row + q * 16);
                d[q * 4 + 0] = u.v[0], d[q * 4 + 1] = u.v[1], d[q * 4 + 2] = u.v[2], d[q * 4 + 3] = u.v[3];
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b0 = 3 * i, b1 = 3 * i + 1, b2 = 3 * i + 2;
                const int B = (d[b0 >> 2] >> (8 * (b0 & 3))) & 255, G = (d[b1 >> 2] >> (8 * (b1 & 3))) & 255, R = (d[b2 >> 2] >> (8 * (b2 & 3))) & 255;
                acc[i / S] += 29 * B + 150 * G + 77 * R;
            }
        }
    } else {   // the row's last, partial span: bytes of the pixels it covers only
#pragma unroll
        for (int r = 0; r < S; ++r)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i < ng * S) {
                    const uint8_t* p = src + r * row + 3 * i;
                    acc[i / S] += 29 * p[0] + 150 * p[1] + 77 * p[2];
                }
    }
    if (ng == NG) {                              // a full span: its 4 or 8 gray pixels as one or two dword stores
#pragma unroll
        for (int q = 0; q < NG / 4; ++q) {
            GmcU32 o;
            o.v = (uint32_t)(acc[4 * q] >> SH) | (uint32_t)(acc[4 * q + 1] >> SH) << 8 | (uint32_t)(acc[4 * q + 2] >> SH) << 16 |
                  (uint32_t)(acc[4 * q + 3] >> SH) << 24;
            *reinterpret_cast<GmcU32*>(dst + 4 * q) = o;
        }
    } else {
#pragma unroll
        for (int j = 0; j < NG; ++j)
            if (j < ng) dst[j] = (uint8_t)(acc[j] >> SH);
    }
}

void launch_gmc_gray(const uint8_t* frames, int k, const GmcGeom& g, uint8_t* gray, hipStream_t s) {
    if (k <= 0 || g.gh <= 0 || g.gw <= 0) return;
    const int ng = 16 / g.s, spans = (g.gw + ng - 1) / ng;
    dim3 grid(ceil_div((long)g.gh * spans, 256), k);
    if (g.s == 4) hipLaunchKernelGGL(gmc_gray_kernel<4>, grid, dim3(256), 0, s, frames, g.h, g.w, g.gh, g.gw, g.level, gray);
    else hipLaunchKernelGGL(gmc_gray_kernel<2>, grid, dim3(256), 0, s, frames, g.h, g.w, g.gh, g.gw, g.level, gray);
    KCHECK();
}

// ---------------------------------------------------------------------------------------------------------------- steps 2-5
__device__ __forceinline__ int gmc_step(int m, int z, int p) {
    const int den = max(m, p) - z;
    if (den <= 0 || z == 0) return 0;
    const int d = m - p, q = (8 * abs(d)) / den;
    return d > 0 ? q : -q;
}

// One wavefront per (block, frame).  The frames are tick-major over `streams` streams: the predecessor of row f is row f - streams, and
// for the first tick level f of the carried bank `prev_bank`, where have[f] says that stream f has one.  LDS: the previous level's 17 x 17 pixels at the block (16 x 16 + the texture's right / lower
// neighbours; rows of 20 bytes), the current level's 32 x 32 window (rows of 32 bytes) and the 289 SADs.  A lane takes the candidates
// lane, lane + 64, ...: 16 rows of four packed byte SADs, the window dwords byte-aligned to dx.
__global__ __launch_bounds__(64) void gmc_match_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ prev_bank,
                                                       const uint8_t* __restrict__ have, int streams, int gw, int nbx, int nb, int s, size_t level, const int32_t* __restrict__ frame_n,
                                                       const int32_t* __restrict__ frame_d0, const float* __restrict__ boxes, int tlwh,
                                                       int32_t* __restrict__ disp) {
    constexpr int NC = (2 * GMC_R + 1) * (2 * GMC_R + 1);
    __shared__ uint32_t s_prev[17 * 5];
    __shared__ uint32_t s_win[32 * 8 + 8];      // + 8: the fifth dword of the last row's byte alignment is read (and not used)
    __shared__ int s_sad[NC];
    const int lane = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
    int32_t* out = disp + ((size_t)f * nb + b) * 2;
    const uint8_t* cur = gray + (size_t)f * level;
    const uint8_t* prev = f >= streams ? cur - (size_t)streams * level : have[f] ? prev_bank + (size_t)f * level : nullptr;
    const int bj = b / nbx, bi = b - bj * nbx;
    const int x0 = GMC_R + GMC_B * bi, y0 = GMC_R + GMC_B * bj;
    bool skip = prev == nullptr;
    if (!skip && frame_n) {                    // step 3: a detection box of the current frame over the block
        const float bx0 = (float)(s * x0), by0 = (float)(s * y0), bx1 = (float)(s * (x0 + GMC_B)), by1 = (float)(s * (y0 + GMC_B));
        const int n = frame_n[f];
        const float* bb = boxes + (size_t)frame_d0[f] * 4;
        bool hit = false;
        for (int i = lane; i < n; i += 64) {
            const float x1 = bb[i * 4], y1 = bb[i * 4 + 1];
            const float x2 = tlwh ? x1 + bb[i * 4 + 2] : bb[i * 4 + 2], y2 = tlwh ? y1 + bb[i * 4 + 3] : bb[i * 4 + 3];
            hit |= x1 < bx1 && x2 > bx0 && y1 < by1 && y2 > by0;
        }
        skip = __any(hit);
    }
    if (skip) {
        if (lane == 0) out[0] = GMC_SKIPPED, out[1] = 0;
        return;
    }
    uint8_t* pb = reinterpret_cast<uint8_t*>(s_prev);
    for (int i = lane; i < 17 * 17; i += 64) {
        const int y = i / 17, x = i - y * 17;
        pb[y * 20 + x] = prev[(size_t)(y0 + y) * gw + x0 + x];
    }
    for (int i = lane; i < 32 * 8; i += 64) {    // the window as dwords: 32 rows of 8
        const int y = i >> 3, x = (i & 7) * 4;
        s_win[i] = reinterpret_cast<const GmcU32*>(cur + (size_t)(y0 - GMC_R + y) * gw + x0 - GMC_R + x)->v;
    }
    if (lane < 8) s_win[32 * 8 + lane] = 0;
    __syncthreads();
    int tex = 0;                               // step 3: texture of the previous block
    for (int i = lane; i < 256; i += 64) {
        const int y = i >> 4, x = i & 15;
        const int v = pb[y * 20 + x];
        tex += abs((int)pb[y * 20 + x + 1] - v) + abs((int)pb[(y + 1) * 20 + x] - v);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) tex += __shfl_xor(tex, o, 64);
    if (tex < GMC_TEX_MIN) {
        if (lane == 0) out[0] = GMC_SKIPPED, out[1] = 0;
        return;
    }
    uint32_t best = 0xffffffffu;               // step 4: ordered (SAD, index) minimum -> the first candidate wins a tie
    for (int c = lane; c < NC; c += 64) {
        const int wy = c / 17, wx = c - wy * 17;
        const int sh = wx & 3;
        const uint32_t* wrow = s_win + wy * 8 + (wx >> 2);
        uint32_t sad = 0;
#pragma unroll 4
        for (int y = 0; y < 16; ++y) {
            const uint32_t* w = wrow + y * 8;
            const uint32_t* p = s_prev + y * 5;
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, sh), p[0], sad);
            sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w2, w1, sh), p[1], sad);
            sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w3, w2, sh), p[2], sad);
            sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w4, w3, sh), p[3], sad);
        }
        s_sad[c] = (int)sad;
        best = min(best, (sad << 9) | (uint32_t)c);   // SAD <= 65 280 < 2^16, c < 289 < 2^9
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o, 64));
    __syncthreads();
    if (lane == 0) {
        const int c = best & 511, z = (int)(best >> 9);
        const int ky = c / 17, kx = c - ky * 17;
        if (ky == 0 || ky == 2 * GMC_R || kx == 0 || kx == 2 * GMC_R) {
            out[0] = GMC_SKIPPED, out[1] = 0;
        } else {                                 // step 5
            out[0] = 16 * (kx - GMC_R) + gmc_step(s_sad[c - 1], z, s_sad[c + 1]);
            out[1] = 16 * (ky - GMC_R) + gmc_step(s_sad[c - 17], z, s_sad[c + 17]);
        }
    }
}

void launch_gmc_match(const uint8_t* gray, const uint8_t* prev_bank, const uint8_t* have, int streams, int k, const GmcGeom& g,
                      const int32_t* frame_n, const int32_t* frame_d0, const float* boxes, bool tlwh, int32_t* disp, hipStream_t s) {
    if (k <= 0 || g.nb <= 0) return;
    hipLaunchKernelGGL(gmc_match_kernel, dim3(g.nb, k), dim3(64), 0, s, gray, prev_bank, have, streams, g.gw, g.nbx, g.nb, g.s, g.level, frame_n,
                       frame_d0, boxes, tlwh ? 1 : 0, disp);
    KCHECK();
}

// ---------------------------------------------------------------------------------------------------------------- steps 6-8
// One workgroup per frame.  The kept blocks' displacements sit in LDS; medians by rank counting, the int64 sums by LDS atomics
// (integers: any order), the fp64 sequence on thread 0, the residuals of every kept block by the thread that owns it.
__global__ __launch_bounds__(256) void gmc_fit_kernel(const int32_t* __restrict__ disp, int nbx, int nb, int s, int min_inliers,
                                                      float* __restrict__ warps, int32_t* __restrict__ stats) {
    __shared__ int s_dx[GMC_MAX_BLOCKS], s_dy[GMC_MAX_BLOCKS];
    __shared__ uint8_t s_in[GMC_MAX_BLOCKS];
    __shared__ long long s_sum[8];             // n, Spx, Spy, Sqx, Sqy, Spp, Sd, Sc
    __shared__ int s_kept, s_med[2], s_fail;
    __shared__ double s_fit[4];                // a, b, tx, ty
    const int tid = threadIdx.x, f = blockIdx.x;
    const int32_t* d = disp + (size_t)f * nb * 2;
    if (tid == 0) s_kept = 0, s_fail = 0;
    __syncthreads();
    int kept = 0;
    for (int i = tid; i < nb; i += 256) {
        s_dx[i] = d[i * 2], s_dy[i] = d[i * 2 + 1];
        kept += s_dx[i] != GMC_SKIPPED;
    }
    if (kept) atomicAdd(&s_kept, kept);
    __syncthreads();
    kept = s_kept;
    int n_in = 0;
    bool ok = kept >= min_inliers;
    if (ok) {
        const int km = (kept - 1) / 2;         // lower median per axis: the value whose rank interval holds km
        for (int i = tid; i < nb; i += 256) {
            if (s_dx[i] == GMC_SKIPPED) continue;
            const int vx = s_dx[i], vy = s_dy[i];
            int lx = 0, ex = 0, ly = 0, ey = 0;
            for (int j = 0; j < nb; ++j) {
                if (s_dx[j] == GMC_SKIPPED) continue;
                lx += s_dx[j] < vx, ex += s_dx[j] == vx, ly += s_dy[j] < vy, ey += s_dy[j] == vy;
            }
            if (lx <= km && km < lx + ex) s_med[0] = vx;
            if (ly <= km && km < ly + ey) s_med[1] = vy;
        }
        __syncthreads();
        const int mx = s_med[0], my = s_med[1];
        for (int i = tid; i < nb; i += 256)
            s_in[i] = s_dx[i] != GMC_SKIPPED && abs(s_dx[i] - mx) <= GMC_START_GATE && abs(s_dy[i] - my) <= GMC_START_GATE;
        for (int rnd = 0; rnd < 3; ++rnd) {
            if (tid < 8) s_sum[tid] = 0;
            __syncthreads();
            long long a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = tid; i < nb; i += 256) {
                if (!s_in[i]) continue;
                const int bj = i / nbx, bi = i - bj * nbx;
                const long long px = 16 * (GMC_R + GMC_B * bi) + 120, py = 16 * (GMC_R + GMC_B * bj) + 120;
                const long long qx = px + s_dx[i], qy = py + s_dy[i];
                a[0] += 1, a[1] += px, a[2] += py, a[3] += qx, a[4] += qy;
                a[5] += px * px + py * py, a[6] += px * qx + py * qy, a[7] += px * qy - py * qx;
            }
            if (a[0]) {
#pragma unroll
                for (int q = 0; q < 8; ++q) atomicAdd(reinterpret_cast<unsigned long long*>(&s_sum[q]), (unsigned long long)a[q]);
            }
            __syncthreads();
            if (tid == 0) {
                const long long n = s_sum[0], P = s_sum[1], Q = s_sum[2], U = s_sum[3], W = s_sum[4];
                const long long V = n * s_sum[5] - P * P - Q * Q;
                const long long D = n * s_sum[6] - P * U - Q * W;
                const long long C = n * s_sum[7] - (P * W - Q * U);
                if (n < min_inliers || V <= 0) s_fail = 1;
                else {
                    const double nd = (double)n;
                    const double fa = (double)D / (double)V, fb = (double)C / (double)V;
                    const double mpx = (double)P / nd, mpy = (double)Q / nd, mqx = (double)U / nd, mqy = (double)W / nd;
                    const double e1 = fa * mpx, e2 = fb * mpy, e3 = fb * mpx, e4 = fa * mpy;
                    s_fit[0] = fa, s_fit[1] = fb;
                    s_fit[2] = mqx - (e1 - e2);
                    s_fit[3] = mqy - (e3 + e4);
                }
            }
            __syncthreads();
            n_in = (int)s_sum[0];
            if (s_fail) break;
            if (rnd < 2) {
                const double fa = s_fit[0], fb = s_fit[1], tx = s_fit[2], ty = s_fit[3];
                for (int i = tid; i < nb; i += 256) {
                    if (s_dx[i] == GMC_SKIPPED) continue;
                    const int bj = i / nbx, bi = i - bj * nbx;
                    const int ipx = 16 * (GMC_R + GMC_B * bi) + 120, ipy = 16 * (GMC_R + GMC_B * bj) + 120;
                    const double px = (double)ipx, py = (double)ipy, qx = (double)(ipx + s_dx[i]), qy = (double)(ipy + s_dy[i]);
                    const double e1 = fa * px, e2 = fb * py, e3 = fb * px, e4 = fa * py;
                    const double rx = ((e1 - e2) + tx) - qx, ry = ((e3 + e4) + ty) - qy;
                    s_in[i] = fmax(fabs(rx), fabs(ry)) <= 16.0;
                }
            }
            __syncthreads();
        }
        ok = !s_fail;
    }
    if (tid == 0) {
        float* w = warps + (size_t)f * 6;
        if (ok) {                                // step 7
            const double fa = s_fit[0], fb = s_fit[1], tx = s_fit[2], ty = s_fit[3];
            const double k = (double)s / 16.0, c = (double)(s - 1) / 2.0;
            const double ac = fa * c, bc = fb * c;
            const double t0 = (((tx * k) + c) - ac) + bc;
            const double t1 = (((ty * k) + c) - bc) - ac;
            w[0] = (float)fa, w[1] = (float)-fb, w[2] = (float)t0, w[3] = (float)fb, w[4] = (float)fa, w[5] = (float)t1;
        } else {
            w[0] = 1.f, w[1] = 0.f, w[2] = 0.f, w[3] = 0.f, w[4] = 1.f, w[5] = 0.f;
        }
        int32_t* st = stats + (size_t)f * 4;
        st[0] = ok ? 1 : 0, st[1] = nb, st[2] = kept, st[3] = n_in;
    }
}

void launch_gmc_fit(const int32_t* disp, int k, const GmcGeom& g, int min_inliers, float* warps, int32_t* stats, hipStream_t s) {
    if (k <= 0) return;
    hipLaunchKernelGGL(gmc_fit_kernel, dim3(k), dim3(256), 0, s, disp, g.nbx, g.nb, g.s, min_inliers, warps, stats);
    KCHECK();
}

}  // namespace aic
