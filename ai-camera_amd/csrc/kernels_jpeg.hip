// kernels_jpeg.hip -- the kernels of the JPEG stage (jpeg.hpp).  Integer arithmetic only; tests/jpeg_oracle.py is
// the specification.  No floating point, no scratch.
//
// jpeg_transform_kernel  the one that reads the frames, every byte once.  A block takes 4 (4:2:0) or 8 (4:4:4) consecutive MCUs = 24
//                        blocks of 8 x 8.  A lane loads 4 pixels of a pixel row -- 12 bytes as three or four aligned dwords and an
//                        alignbyte, correct for any base and width; pixels past the right edge go byte by byte with clamped
//                        coordinates -- and leaves Y, Cb, Cr as bytes in LDS; 16 neighbouring lanes cover one pixel row of the group.
//                        Then 8 lanes per block: a lane does one row of the row pass, then one column of the column pass, quantises
//                        with a multiply-high (rcp = ceil(2^32 / 8Q): exact below 2^15) and writes zigzag positions into LDS; the
//                        group's 3072 bytes leave as 16-byte vectors.
// jpeg_entropy_kernel    one block per (restart interval, image), a lane per 8 x 8 block of a round of up to 256 blocks: the lane
//                        holds its 64 coefficients in 32 registers, computes its bit length (the DC predictor is the neighbouring
//                        block's quantised DC, read directly), a block scan gives the bit offsets, and the round takes as many
//                        blocks as fit the 16 KB LDS bit tile (one always fits: a block is at most 1658 bits).  The lanes then
//                        emit at their offsets with LDS OR-atomics, order-free and so deterministic.  The tile's complete bytes are
//                        counted with their 0xFF bytes, scanned, and written stuffed; the 0..7 bits left over are carried into the
//                        next round, so an interval of any length is walked in rounds.  Without an output pointer nothing is
//                        written but the interval's stuffed size (pass 1); with one, the bytes go to their final address (pass 2).
// jpeg_scan_kernel       one block per image: the exclusive scan of its interval sizes and their sum.
#include "jpeg.hpp"

namespace aic {

namespace {

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax0(int a) { return a < 0 ? 0 : a; }

constexpr int JT = 256;

// exclusive scan of v over the 256 lanes of the block; total = the sum.  Two barriers.
template <class V>
__device__ __forceinline__ V block_scan_excl(V v, V* s_wave, V& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    V inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const V o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    V base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < JT / 64; ++w) {
        const V t = s_wave[w];
        if (w < wv) base += t;
        sum += t;
    }
    __syncthreads();
    total = sum;
    return base + inc - v;
}

template <int SUB>
__global__ __launch_bounds__(JT) void jpeg_transform_kernel(const uint8_t* __restrict__ frames, JpegGeom g, const uint32_t* __restrict__ tab,
                                                            int16_t* __restrict__ coef) {
    constexpr int MW = SUB == 420 ? 16 : 8, MPB = SUB == 420 ? 4 : 8, BPM = SUB == 420 ? 6 : 3, SEGS = MW / 4, UNITS = 16 * MW;
    static constexpr int T[8][8] = {{1448, 1448, 1448, 1448, 1448, 1448, 1448, 1448},   {2009, 1703, 1138, 400, -400, -1138, -1703, -2009},
                                    {1892, 784, -784, -1892, -1892, -784, 784, 1892},   {1703, -400, -2009, -1138, 1138, 2009, 400, -1703},
                                    {1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448}, {1138, -2009, 400, 1703, -1703, -400, 2009, -1138},
                                    {784, -1892, 1892, -784, -784, 1892, -1892, 784},   {400, -1138, 1703, -2009, 2009, -1703, 1138, -400}};
    __shared__ uint8_t s_px[3][MPB][MW][MW];
    __shared__ int s_a[24][8][9];
    __shared__ __align__(16) int16_t s_out[24][64];
    __shared__ unsigned s_q[256];                                            // rcp[2][64] | add[2][64], natural order
    __shared__ uint8_t s_zz[64];                                             // zigzag position of a natural index
    const int tid = threadIdx.x, img = blockIdx.y, m_first = blockIdx.x * MPB;
    s_q[tid] = tab[JPEG_TAB_RCP + tid];
    if (tid < 64) s_zz[tid] = reinterpret_cast<const uint8_t*>(tab + JPEG_TAB_ZZ)[tid];
    const uint8_t* f = frames + (size_t)img * g.h * g.w * 3;
    if (tid < UNITS) {
        const int row = tid >> 4, ml = (tid & 15) / SEGS, xs = (tid % SEGS) * 4, m = m_first + ml;
        if (m < g.n_mcu) {
            const int my = m / g.mcus_x, mx = m - my * g.mcus_x;
            const int y = imin(my * MW + row, g.h - 1), x0 = mx * MW + xs;
            unsigned px[4];                                                  // B | G << 8 | R << 16
            if (x0 + 3 < g.w) {
                const uintptr_t a = reinterpret_cast<uintptr_t>(f + ((size_t)y * g.w + x0) * 3);
                const unsigned sh = (unsigned)(a & 3);
                const unsigned* q = reinterpret_cast<const unsigned*>(a - sh);   // every aligned word read holds a byte of the 12
                const unsigned d0 = q[0], d1 = q[1], d2 = q[2], d3 = sh ? q[3] : 0u;
                const unsigned v0 = __builtin_amdgcn_alignbyte(d1, d0, sh), v1 = __builtin_amdgcn_alignbyte(d2, d1, sh),
                               v2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
                px[0] = v0 & 0xffffffu, px[1] = (v0 >> 24) | (v1 & 0xffffu) << 8, px[2] = (v1 >> 16) | (v2 & 0xffu) << 16, px[3] = v2 >> 8;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint8_t* p = f + ((size_t)y * g.w + imin(x0 + j, g.w - 1)) * 3;
                    px[j] = p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int B = px[j] & 255, G = (px[j] >> 8) & 255, R = px[j] >> 16;
                s_px[0][ml][row][xs + j] = (uint8_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
                s_px[1][ml][row][xs + j] = (uint8_t)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16);
                s_px[2][ml][row][xs + j] = (uint8_t)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16);
            }
        }
    }
    __syncthreads();
    const int tb = tid >> 3, r = tid & 7, ml = tb / BPM, bi = tb - ml * BPM;
    if (tid < 192) {
        int s[8];
        if constexpr (SUB == 444) {
#pragma unroll
            for (int x = 0; x < 8; ++x) s[x] = (int)s_px[bi][ml][r][x] - 128;
        } else {
            if (bi < 4) {
#pragma unroll
                for (int x = 0; x < 8; ++x) s[x] = (int)s_px[0][ml][(bi >> 1) * 8 + r][(bi & 1) * 8 + x] - 128;
            } else {
#pragma unroll
                for (int x = 0; x < 8; ++x)
                    s[x] = (((int)s_px[bi - 3][ml][2 * r][2 * x] + s_px[bi - 3][ml][2 * r][2 * x + 1] + s_px[bi - 3][ml][2 * r + 1][2 * x] +
                             s_px[bi - 3][ml][2 * r + 1][2 * x + 1] + 2) >> 2) - 128;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int acc = 0;
#pragma unroll
            for (int x = 0; x < 8; ++x) acc += __mul24(T[u][x], s[x]);       // |T| < 2^11, |s| <= 128: 24-bit operands, full rate
            s_a[tb][r][u] = (acc + 256) >> 9;
        }
    }
    __syncthreads();
    if (tid < 192) {
        int a[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) a[y] = s_a[tb][y][r];
        const int comp = bi >= BPM - 2;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            int acc = 0;
#pragma unroll
            for (int y = 0; y < 8; ++y) acc += __mul24(T[v][y], a[y]);       // |A| <= 2896
            const int F = (acc + 2048) >> 12, nat = v * 8 + r;
            const unsigned mag = (unsigned)(F < 0 ? -F : F) + s_q[128 + comp * 64 + nat];
            const int q = (int)__umulhi(mag, s_q[comp * 64 + nat]);
            s_out[tb][s_zz[nat]] = (int16_t)(F < 0 ? -q : q);
        }
    }
    __syncthreads();
    const int valid = imin(MPB, g.n_mcu - m_first) * BPM * 8;               // 16-byte vectors of the group's MCUs inside the image
    if (tid < valid) {
        uint4* dst = reinterpret_cast<uint4*>(coef + ((size_t)img * g.n_mcu + m_first) * BPM * 64);
        dst[tid] = reinterpret_cast<const uint4*>(&s_out[0][0])[tid];
    }
}

constexpr int TILE_WORDS = 4096;                                             // the bit tile: 16 KB
constexpr int TILE_BITS = TILE_WORDS * 32 - 32;                              // what a round may emit behind the carried bits

// The bits of one block, appended MSB first at bit `pos` of the tile.  EMIT = false: only their number.
template <bool EMIT>
struct BitSink {
    unsigned* tile;
    unsigned long long acc = 0;
    int word, fill, bits = 0;
    __device__ BitSink(unsigned* t, unsigned pos) : tile(t), word((int)(pos >> 5)), fill((int)(pos & 31)) {}
    __device__ __forceinline__ void put(unsigned code, int len) {           // len <= 26, code < 2^len
        bits += len;
        if constexpr (EMIT) {
            acc |= (unsigned long long)code << (64 - fill - len);
            fill += len;
            if (fill >= 32) {
                atomicOr(&tile[word], (unsigned)(acc >> 32));
                ++word, acc <<= 32, fill -= 32;
            }
        }
    }
    __device__ __forceinline__ void flush() {
        if constexpr (EMIT)
            if (fill) atomicOr(&tile[word], (unsigned)(acc >> 32));
    }
};

__device__ __forceinline__ unsigned value_bits(int v, int cat) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u); }

template <bool EMIT>
__device__ __forceinline__ int encode_block(const unsigned (&w)[32], int pred, const unsigned* __restrict__ dc, const unsigned* __restrict__ ac,
                                            unsigned* tile, unsigned pos) {
    BitSink<EMIT> sink(tile, pos);
    const int diff = (int)(short)(w[0] & 0xffffu) - pred;
    int cat = 32 - __clz(diff < 0 ? -diff : diff);
    unsigned e = dc[cat];
    sink.put((e >> 5) << cat | value_bits(diff, cat), (int)(e & 31u) + cat);
    int run = 0;
    auto one = [&](int v) {
        if (v == 0) { ++run; return; }
        while (run > 15) {
            e = ac[0xF0];
            sink.put(e >> 5, (int)(e & 31u));
            run -= 16;
        }
        cat = 32 - __clz(v < 0 ? -v : v);
        e = ac[run << 4 | cat];
        sink.put((e >> 5) << cat | value_bits(v, cat), (int)(e & 31u) + cat);
        run = 0;
    };
    one((int)(short)(w[0] >> 16));
#pragma unroll
    for (int j = 1; j < 32; ++j) {
        if (w[j] == 0u) { run += 2; continue; }
        one((int)(short)(w[j] & 0xffffu));
        one((int)(short)(w[j] >> 16));
    }
    if (run) {
        e = ac[0x00];
        sink.put(e >> 5, (int)(e & 31u));
    }
    sink.flush();
    return sink.bits;
}

template <bool WRITE>
__global__ __launch_bounds__(JT) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, JpegGeom g, const uint32_t* __restrict__ tab,
                                                          int* __restrict__ sizes, const int64_t* __restrict__ ivl_off,
                                                          const int64_t* __restrict__ img_off, const int* __restrict__ status,
                                                          uint8_t* __restrict__ out) {
    __shared__ unsigned s_tile[TILE_WORDS + 1];
    __shared__ unsigned s_dc[32], s_ac[512];
    __shared__ int s_wave[JT / 64];
    __shared__ int s_first[2];                                               // the first block that does not fit the tile, the bits before it
    const int tid = threadIdx.x, ivl = blockIdx.x, img = blockIdx.y;
    if constexpr (WRITE)
        if (status[img]) return;
    if (tid < 32) s_dc[tid] = tab[JPEG_TAB_DC + tid];
    s_ac[tid] = tab[JPEG_TAB_AC + tid], s_ac[tid + 256] = tab[JPEG_TAB_AC + 256 + tid];
    __syncthreads();
    const int b0 = ivl * g.ri * g.bpm, b1 = imin((ivl + 1) * g.ri, g.n_mcu) * g.bpm;   // the interval's blocks inside the image
    const int16_t* ic = coef + (size_t)img * g.n_mcu * g.bpm * 64;
    uint8_t* dst = nullptr;
    if constexpr (WRITE) {
        uint8_t* file = out + img_off[img];
        if (ivl == 0) {
            const uint8_t* hdr = reinterpret_cast<const uint8_t*>(tab);
            for (int i = tid; i < JPEG_HEADER_BYTES; i += JT) file[i] = hdr[i];
        }
        dst = file + JPEG_HEADER_BYTES + ivl_off[(size_t)img * g.intervals + ivl] + 2 * (int64_t)ivl;
    }
    int written = 0;
    unsigned carry_bits = 0, carry_byte = 0;                                 // uniform over the block
    for (int start = b0; start < b1;) {
        const int b = start + tid;
        const bool have = b < b1;
        unsigned w[32];
        int pred = 0, comp = 0, len = 0;
        if (tid == 0) s_first[0] = -1;
        if (have) {
            const uint4* src = reinterpret_cast<const uint4*>(ic + (size_t)b * 64);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint4 v = src[i];
                w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
            }
            const int bi = b % g.bpm;
            comp = bi >= g.bpm - 2;
            const int prev = g.bpm == 3 ? b - 3 : bi == 0 ? b - 3 : bi < 4 ? b - 1 : b - 6;   // the component's block before this one
            if (prev >= b0) pred = ic[(size_t)prev * 64];
            len = encode_block<false>(w, pred, s_dc + comp * 16, s_ac + comp * 256, nullptr, 0u);
        }
        int total;
        const int excl = block_scan_excl(len, s_wave, total);                // its first barrier also publishes s_first
        if (have && excl + len > TILE_BITS && excl <= TILE_BITS) s_first[0] = tid, s_first[1] = excl;
        __syncthreads();
        const int count = s_first[0] < 0 ? imin(JT, b1 - start) : s_first[0];
        const int bits = s_first[0] < 0 ? total : s_first[1];
        const int tile_bits = (int)carry_bits + bits;
        for (int i = tid; i <= (tile_bits >> 5); i += JT) s_tile[i] = i == 0 ? carry_byte << 24 : 0u;
        __syncthreads();
        if (tid < count) encode_block<true>(w, pred, s_dc + comp * 16, s_ac + comp * 256, s_tile, carry_bits + (unsigned)excl);
        __syncthreads();
        const bool last = start + count == b1;
        int nb = tile_bits >> 3, rem = tile_bits & 7, pad_at = -1;
        if (last && rem) pad_at = nb, ++nb;                                  // the interval ends: ones up to the byte boundary
        for (int k0 = 0; k0 < nb; k0 += 4 * JT) {
            const int wi = (k0 >> 2) + tid, kb = wi * 4;
            const int nvalid = imin(imax0(nb - kb), 4);
            unsigned word = nvalid ? s_tile[wi] : 0u;
            if (pad_at >= 0 && (pad_at >> 2) == wi) word |= (0xffu >> rem) << (24 - 8 * (pad_at & 3));
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nvalid) cnt += 1 + (((word >> (24 - 8 * j)) & 255u) == 255u);
            int sum;
            const int at = block_scan_excl(cnt, s_wave, sum);
            if constexpr (WRITE) {
                uint8_t* p = dst + written + at;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nvalid) {
                        const unsigned byte = (word >> (24 - 8 * j)) & 255u;
                        *p++ = (uint8_t)byte;
                        if (byte == 255u) *p++ = 0;
                    }
            }
            written += sum;
        }
        carry_bits = last ? 0u : (unsigned)rem;
        carry_byte = carry_bits ? (s_tile[nb >> 2] >> (24 - 8 * (nb & 3))) & 255u : 0u;
        start += count;
    }
    if (tid == 0) {
        if constexpr (WRITE) {
            dst[written] = 0xff;
            dst[written + 1] = (uint8_t)(ivl < g.intervals - 1 ? 0xd0 + (ivl & 7) : 0xd9);
        } else {
            sizes[(size_t)img * g.intervals + ivl] = written;
        }
    }
}

__global__ __launch_bounds__(JT) void jpeg_scan_kernel(const int* __restrict__ sizes, int intervals, int64_t* __restrict__ ivl_off,
                                                       int64_t* __restrict__ totals) {
    __shared__ long long s_wave[JT / 64];
    const size_t base = (size_t)blockIdx.x * intervals;
    long long run = 0;
    for (int i0 = 0; i0 < intervals; i0 += JT) {
        const int i = i0 + (int)threadIdx.x;
        const long long v = i < intervals ? sizes[base + i] : 0;
        long long sum;
        const long long at = block_scan_excl(v, s_wave, sum);
        if (i < intervals) ivl_off[base + i] = run + at;
        run += sum;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = run;
}

}  // namespace

void launch_jpeg_transform(const uint8_t* frames, int n_images, const JpegGeom& g, const uint32_t* tab, int16_t* coef, hipStream_t s) {
    if (g.sub == 420)
        hipLaunchKernelGGL(jpeg_transform_kernel<420>, dim3(ceil_div(g.n_mcu, 4), n_images), dim3(JT), 0, s, frames, g, tab, coef);
    else
        hipLaunchKernelGGL(jpeg_transform_kernel<444>, dim3(ceil_div(g.n_mcu, 8), n_images), dim3(JT), 0, s, frames, g, tab, coef);
    KCHECK();
}

void launch_jpeg_entropy(const int16_t* coef, int n_images, const JpegGeom& g, const uint32_t* tab, int* sizes, const int64_t* ivl_off,
                         const int64_t* img_off, const int* status, uint8_t* out, hipStream_t s) {
    if (out)
        hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3(g.intervals, n_images), dim3(JT), 0, s, coef, g, tab, sizes, ivl_off, img_off, status, out);
    else
        hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3(g.intervals, n_images), dim3(JT), 0, s, coef, g, tab, sizes, ivl_off, img_off, status, out);
    KCHECK();
}

void launch_jpeg_scan(const int* sizes, int n_images, const JpegGeom& g, int64_t* ivl_off, int64_t* totals, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(n_images), dim3(JT), 0, s, sizes, g.intervals, ivl_off, totals);
    KCHECK();
}

}  // namespace aic
