// xvector.hip -- the x-vector forward pass on the device: speaker embeddings from a feature batch.
//
//   xv_convert_kernel   fp32 rows -> bf16 rows (round to nearest even) of the padded width: the features into the first layer, the
//                       pooled statistics into the first segment layer
//   xv_layer_kernel     every tdnn and affine layer: an implicit GEMM  Y[row][col] = sum_j sum_c  X[row + o_j - o_1][c] W[col][j][c]
//                       on the bf16 matrix cores with fp32 accumulators.  A workgroup of four waves takes one tile of the host-built
//                       tile list (128 output rows of ONE segment) x 128 output channels; the K loop runs "for each offset, for
//                       each 32 channels", two such granules (K = 64) per LDS stage, double-buffered: the global loads of stage
//                       s + 1 are in flight under the MFMAs of stage s, one barrier per stage.  For an offset the tile's A rows
//                       are a contiguous run of input rows, shifted by o_j - o_1.  Rows past the tile's count are zero-filled, never
//                       loaded: no load leaves the segment.  The weight image is padded to whole tiles and whole stages with zeros
//                       when the network is created, so its loads need no mask.
//                       An output element's sum depends on its own row of A alone and runs in the layer's fixed order, so a
//                       segment's values do not depend on its place in a batch, on its neighbours or on the chunking.
//                       Epilogue in fp32: z = acc + b, a = act(z), y = fma(scale, a, shift); stored as bf16 (round to nearest even)
//                       into the next layer's padded input, or as fp32 into the call's result (the last layer, a tapped layer).
//   xv_pool_kernel      a workgroup per (segment, 64 channels): four row lanes sum x and x^2 of every fourth row in float64, in
//                       row order; the four partial sums are added as (0 + 1) + (2 + 3).  The order depends on the frame count
//                       alone.  Writes [mean | std] as fp32.
//
// LDS image: a staged row is 128 bytes (K = 64 bf16), eight 16-byte pieces; piece p of row r is kept at piece p ^ ((r >> 1) & 7).
// A fragment read is 16 bytes per lane at one row per lane and the same logical piece: of 16 consecutive rows the even ones fall
// into banks 0 .. 31 and the odd ones into banks 32 .. 63 (a row is 32 banks), and the XOR spreads the eight rows of one parity
// over the eight pieces -- the 16 reads tile the 64 banks once.  The staging stores (eight lanes a row, pieces 0 .. 7) do the same.
// Two buffers of (128 + 128) rows are exactly 64 KiB: no padding fits, hence the swizzle.
#include "xvector.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>

namespace sr {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));      // 16 bytes in flight (a plain vector: a select, not a copy through memory)

struct XvShifts {
    int s[XV_MAX_OFFSETS];      // o_j - o_1
};

struct XvCopyTile {
    int64_t src, dst;           // first rows
    int32_t rows, pad;
};

__device__ __forceinline__ unsigned bf16_rne_bits(float v) {
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;      // NaN: quiet, sign and payload top kept
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__global__ __launch_bounds__(256)
void xv_convert_kernel(const float *__restrict__ src, int ld_src, int C, const XvCopyTile *__restrict__ tiles, uint16_t *__restrict__ dst, int cp) {
    const XvCopyTile t = tiles[blockIdx.x];
    const int per_row = cp >> 3;
    const int n = t.rows * per_row;
    const bool vec = ((C | ld_src) & 3) == 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int r = i / per_row, c0 = (i - r * per_row) << 3;
        const float *p = src + (size_t)(t.src + r) * (size_t)ld_src + c0;
        float v[8];
        if (vec) {       // C a multiple of 4: a float4 lies wholly inside the row or wholly in the padding
            const float4 a = c0 < C ? *reinterpret_cast<const float4 *>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 b = c0 + 4 < C ? *reinterpret_cast<const float4 *>(p + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
            v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = c0 + e < C ? p[e] : 0.f;
        }
        uint4 o;
        o.x = bf16_rne_bits(v[0]) | (bf16_rne_bits(v[1]) << 16);
        o.y = bf16_rne_bits(v[2]) | (bf16_rne_bits(v[3]) << 16);
        o.z = bf16_rne_bits(v[4]) | (bf16_rne_bits(v[5]) << 16);
        o.w = bf16_rne_bits(v[6]) | (bf16_rne_bits(v[7]) << 16);
        *reinterpret_cast<uint4 *>(dst + (size_t)(t.dst + r) * (size_t)cp + c0) = o;
    }
}

// SHAPE 0: v_mfma_f32_32x32x16_bf16 (a wave's 64 x 64 as 2 x 2 tiles); 1: v_mfma_f32_16x16x32_bf16 (4 x 4 tiles)
template <bool F32OUT, int SHAPE>
__global__ __launch_bounds__(XV_WG)
void xv_layer_kernel(const uint16_t *__restrict__ A, int lda, const int64_t *__restrict__ in_base, const int64_t *__restrict__ out_base,
                     const XvTile *__restrict__ tiles, const uint16_t *__restrict__ W, int kp, int n_off, XvShifts shifts, int gran_per_off,
                     const float *__restrict__ bias, const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                     void *__restrict__ out, int ldo, int c_out) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[XV_LDS_BYTES];
    constexpr int BUF = (XV_TM + XV_TN) * XV_LDS_ROW;
    const XvTile t = tiles[blockIdx.x];
    const int col0 = blockIdx.y * XV_TN;
    const int64_t in_row0 = in_base[t.seg] + t.first, out_row0 = out_base[t.seg] + t.first;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n_sub = n_off * gran_per_off, n_stage = (n_sub + 1) >> 1;

    // staging: a thread moves 16 bytes of four A rows and four B rows per stage; its half (granule of the stage) and piece are fixed
    const int l_row = tid >> 3, l_half = (tid >> 2) & 1, l_piece = tid & 3;
    u32x4 ra[4], rb[4];
    auto load_stage = [&](int s) {
        const int q = 2 * s + l_half;
        const bool live = q < n_sub;
        const int j = live ? q / gran_per_off : 0;
        const int c = live ? q - j * gran_per_off : 0;
        const uint16_t *pa = A + (size_t)(in_row0 + shifts.s[j]) * (size_t)lda + c * XV_GRAN + l_piece * 8;
        const uint16_t *pb = W + (size_t)col0 * (size_t)kp + (size_t)s * XV_KC + l_half * XV_GRAN + l_piece * 8;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = l_row + 32 * i;
            const u32x4 zero = {0u, 0u, 0u, 0u};
            ra[i] = zero;
            if (live && r < t.rows) ra[i] = *reinterpret_cast<const u32x4 *>(pa + (size_t)r * (size_t)lda);
            rb[i] = *reinterpret_cast<const u32x4 *>(pb + (size_t)r * (size_t)kp);
        }
    };
    auto store_stage = [&](int buf) {
        // (rows r and r + 32 i share (r >> 1) & 7, and so do a row of A and the same row of B)
        unsigned char *base = smem + buf * BUF + (((l_half * 4 + l_piece) ^ ((l_row >> 1) & 7)) << 4);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = l_row + 32 * i;
            *reinterpret_cast<u32x4 *>(base + r * XV_LDS_ROW) = ra[i];
            *reinterpret_cast<u32x4 *>(base + (XV_TM + r) * XV_LDS_ROW) = rb[i];
        }
    };

    constexpr int NT = SHAPE == 0 ? 2 : 4;            // tiles per side of the wave's 64 x 64
    constexpr int TS = SHAPE == 0 ? 32 : 16;          // side of an MFMA tile
    constexpr int KS = SHAPE == 0 ? 16 : 32;          // K of an MFMA
    typedef typename std::conditional<SHAPE == 0, f32x16, f32x4>::type acc_t;
    acc_t acc[NT][NT];
#pragma unroll
    for (int mi = 0; mi < NT; mi++)
#pragma unroll
        for (int ni = 0; ni < NT; ni++)
#pragma unroll
            for (int r = 0; r < (SHAPE == 0 ? 16 : 4); r++) acc[mi][ni][r] = 0.f;
    const int f_row = lane & (TS - 1), f_p = lane / TS;      // a lane's row of the operand tile and its 16-byte piece of the K step
    const int f_x = (f_row >> 1) & 7;                        // (the same for rows f_row + 16 i: the fragments' rows)

    load_stage(0);
    store_stage(0);
    __syncthreads();
    for (int s = 0; s < n_stage; s++) {
        const bool more = s + 1 < n_stage;
        if (more) load_stage(s + 1);
        const unsigned char *pa = smem + (s & 1) * BUF + (wm * 64 + f_row) * XV_LDS_ROW;
        const unsigned char *pb = smem + (s & 1) * BUF + (XV_TM + wn * 64 + f_row) * XV_LDS_ROW;
#pragma unroll
        for (int ks = 0; ks < XV_KC / KS; ks++) {
            bf16x8 fa[NT], fb[NT];
#pragma unroll
            for (int i = 0; i < NT; i++) {
                const int piece = ((ks * (KS / 8) + f_p) ^ f_x) << 4;
                fa[i] = *reinterpret_cast<const bf16x8 *>(pa + i * TS * XV_LDS_ROW + piece);
                fb[i] = *reinterpret_cast<const bf16x8 *>(pb + i * TS * XV_LDS_ROW + piece);
            }
#pragma unroll
            for (int mi = 0; mi < NT; mi++)
#pragma unroll
                for (int ni = 0; ni < NT; ni++) {
                    if constexpr (SHAPE == 0)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
                    else
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
                }
        }
        if (more) store_stage((s + 1) & 1);
        __syncthreads();
    }

    // epilogue: the accumulator's column is on the lane, its rows in the registers
#pragma unroll
    for (int ni = 0; ni < NT; ni++) {
        const int col = col0 + wn * 64 + ni * TS + f_row;       // < n_pad: bias, scale and shift are padded to it
        const float bc = bias[col], sc = scale[col], sh = shift[col];
#pragma unroll
        for (int mi = 0; mi < NT; mi++)
#pragma unroll
            for (int r = 0; r < (SHAPE == 0 ? 16 : 4); r++) {
                const int row = wm * 64 + mi * TS + (SHAPE == 0 ? (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) : (lane >> 4) * 4 + r);
                if (row >= t.rows) continue;
                const float z = acc[mi][ni][r] + bc;
                const float a = relu ? fmaxf(z, 0.f) : z;
                const float y = __builtin_fmaf(sc, a, sh);
                if constexpr (F32OUT) {
                    if (col < c_out) static_cast<float *>(out)[(size_t)(out_row0 + row) * (size_t)ldo + col] = y;
                } else {
                    if (col < ldo) static_cast<uint16_t *>(out)[(size_t)(out_row0 + row) * (size_t)ldo + col] = (uint16_t)bf16_rne_bits(y);
                }
            }
    }
}

__global__ __launch_bounds__(XV_POOL_COLS * XV_POOL_LANES)
void xv_pool_kernel(const uint16_t *__restrict__ X, int ld, int C, const int64_t *__restrict__ base, double var_floor, float *__restrict__ out) {
    __shared__ double s_sum[XV_POOL_LANES][XV_POOL_COLS], s_sq[XV_POOL_LANES][XV_POOL_COLS];
    const int seg = blockIdx.x;
    const int cl = threadIdx.x & (XV_POOL_COLS - 1), rl = threadIdx.x / XV_POOL_COLS;
    const int c = blockIdx.y * XV_POOL_COLS + cl;
    const int64_t r0 = base[seg], n = base[seg + 1] - r0;
    double S = 0.0, Q = 0.0;
    if (c < C)
        for (int64_t r = rl; r < n; r += XV_POOL_LANES) {
            const double x = (double)__uint_as_float((unsigned)X[(size_t)(r0 + r) * (size_t)ld + c] << 16);
            S += x;
            Q += x * x;
        }
    s_sum[rl][cl] = S;
    s_sq[rl][cl] = Q;
    __syncthreads();
    if (rl == 0 && c < C) {
        S = (s_sum[0][cl] + s_sum[1][cl]) + (s_sum[2][cl] + s_sum[3][cl]);
        Q = (s_sq[0][cl] + s_sq[1][cl]) + (s_sq[2][cl] + s_sq[3][cl]);
        const double mean = S / (double)n;
        const double var = fmax(Q / (double)n - mean * mean, var_floor);
        out[(size_t)seg * (size_t)(2 * C) + c] = (float)mean;
        out[(size_t)seg * (size_t)(2 * C) + C + c] = (float)sqrt(var);
    }
}

std::atomic<long> g_scratch_mib{(long)(XV_DEFAULT_SCRATCH >> 20)};
std::atomic<int> g_mfma_shape{0};

struct XvWorkspace {
    DevBuf<uint16_t> buf[2], seg_buf[2];
    DevBuf<float> pooled, result;
    DevBuf<XvTile> tiles;
    DevBuf<XvCopyTile> copy_tiles;
    DevBuf<int64_t> bases;
    PinnedBuf<float> h_result;
    PinnedBuf<uint16_t> h_bf16;
    std::vector<hipEvent_t> events;
};

void upload_model(SRXvector &net) {
    if (net.device >= 0) {
        if (net.device != current_device())
            fail("the network is resident on device %d, the calling thread is on device %d; create one network per device", net.device,
                 current_device());
        return;
    }
    const size_t L = net.layers.size();
    net.d_w.resize(L);
    net.d_b.resize(L);
    net.d_scale.resize(L);
    net.d_shift.resize(L);
    for (size_t l = 0; l < L; l++) {
        if (net.layers[l].kind == XV_POOL) continue;
        net.d_w[l].upload(net.h_w[l].data(), net.h_w[l].size());
        net.d_b[l].upload(net.h_b[l].data(), net.h_b[l].size());
        net.d_scale[l].upload(net.h_scale[l].data(), net.h_scale[l].size());
        net.d_shift[l].upload(net.h_shift[l].data(), net.h_shift[l].size());
    }
    sync_stream();
    net.device = current_device();
}

template <bool F32OUT>
void launch_layer(int shape, dim3 grid, hipStream_t st, const uint16_t *A, int lda, const int64_t *in_base, const int64_t *out_base,
                  const XvTile *tiles, const uint16_t *W, int kp, int n_off, const XvShifts &sh, int gpo, const float *b, const float *scale,
                  const float *shift, int relu, void *out, int ldo, int c_out) {
    if (shape == 0)
        hipLaunchKernelGGL((xv_layer_kernel<F32OUT, 0>), grid, dim3(XV_WG), 0, st, A, lda, in_base, out_base, tiles, W, kp, n_off, sh, gpo,
                           b, scale, shift, relu, out, ldo, c_out);
    else
        hipLaunchKernelGGL((xv_layer_kernel<F32OUT, 1>), grid, dim3(XV_WG), 0, st, A, lda, in_base, out_base, tiles, W, kp, n_off, sh, gpo,
                           b, scale, shift, relu, out, ldo, c_out);
    SR_HIP(hipGetLastError());
}

}  // namespace

long xvector_scratch_mib() { return g_scratch_mib.load(); }
void set_xvector_scratch_mib(long mib) { g_scratch_mib.store(mib); }
int xvector_mfma_shape() { return g_mfma_shape.load(); }
void set_xvector_mfma_shape(int shape) { g_mfma_shape.store(shape); }

uint16_t xv_bf16_rne(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

SRXvector *xvector_create(const XvLayer *layers, int n_layers, const float *const *W, const float *const *b, const float *const *scale,
                          const float *const *shift) {
    auto net = std::make_unique<SRXvector>();
    std::string why;
    if (!xv_check_model(layers, n_layers, net->info, why)) fail("sr_xvector_create: %s", why.c_str());
    const XvModelInfo &m = net->info;
    net->layers.assign(layers, layers + n_layers);
    const size_t L = (size_t)n_layers;
    net->h_w.resize(L);
    net->h_b.resize(L);
    net->h_scale.resize(L);
    net->h_shift.resize(L);
    for (size_t l = 0; l < L; l++) {
        const XvLayer &Ly = layers[l];
        if (Ly.kind == XV_POOL) continue;
        if (!W || !b || !W[l] || !b[l]) fail("sr_xvector_create: layer %d has no weights or no bias", (int)l);
        const bool aff = scale && shift && scale[l] && shift[l];
        if (Ly.has_affine != aff) fail("sr_xvector_create: layer %d: scale and shift are given together, as its descriptor says, or not at all", (int)l);
        const int ci = Ly.c_in, cip = m.width_pad[l], co = Ly.c_out, kp = m.k_pad[l], np = m.n_pad[l];
        for (size_t i = 0; i < (size_t)co * Ly.n_off * ci; i++)
            if (!std::isfinite(W[l][i])) fail("sr_xvector_create: layer %d holds a non-finite weight at entry %lld; clean the checkpoint", (int)l, (long long)i);
        for (int c = 0; c < co; c++)
            if (!std::isfinite(b[l][c]) || (aff && (!std::isfinite(scale[l][c]) || !std::isfinite(shift[l][c]))))
                fail("sr_xvector_create: layer %d holds a non-finite bias, scale or shift at channel %d; clean the checkpoint", (int)l, c);
        net->h_w[l].assign((size_t)np * kp, 0);
        net->h_b[l].assign((size_t)np, 0.f);
        net->h_scale[l].assign((size_t)np, 0.f);
        net->h_shift[l].assign((size_t)np, 0.f);
        for (int c = 0; c < co; c++) {
            for (int j = 0; j < Ly.n_off; j++)
                for (int k = 0; k < ci; k++)
                    net->h_w[l][(size_t)c * kp + (size_t)j * cip + k] = xv_bf16_rne(W[l][((size_t)c * Ly.n_off + j) * ci + k]);
            net->h_b[l][(size_t)c] = b[l][c];
            net->h_scale[l][(size_t)c] = aff ? scale[l][c] : 1.f;
            net->h_shift[l][(size_t)c] = aff ? shift[l][c] : 0.f;
        }
    }
    return net.release();
}

void xvector_forward(SRXvector &net, SRBatch &feat, const int32_t *segs, const XvPlan &plan, bool tap_bf16, float *out, double *times_ms) {
    const XvModelInfo &m = net.info;
    const int L = m.n_layers, P = m.pool;
    const int64_t n_seg = plan.n_seg;
    std::vector<int64_t> lengths((size_t)n_seg);
    for (int64_t i = 0; i < n_seg; i++) lengths[(size_t)i] = segs[3 * i + 2];
    if (times_ms) std::fill(times_ms, times_ms + L + 1, 0.0);
    if (n_seg == 0) return;
    ensure_device();
    if (feat.device >= 0 && feat.device != current_device())
        fail("the feature batch lives on device %d, the calling thread is on device %d", feat.device, current_device());
    upload_model(net);
    XvWorkspace &ws = per_device<XvWorkspace>();
    hipStream_t st = ctx().stream;
    const int last = plan.last, shape = xvector_mfma_shape();
    ws.buf[0].ensure((size_t)(plan.buf_bytes[0] / 2));
    ws.buf[1].ensure((size_t)(plan.buf_bytes[1] / 2));

    std::vector<XvTile> tiles_all, tiles_l;
    std::vector<size_t> tile_off((size_t)L + 1);
    std::vector<XvCopyTile> copies;
    std::vector<int64_t> bases;
    std::vector<int> interval;        // what the time between two consecutive events belongs to: 0 the converts, 1 + l layer l
    int64_t out_row = 0;
    for (const XvChunk &ch : plan.chunks) {
        const int64_t n = ch.seg_end - ch.seg_begin;
        const int64_t *len = lengths.data() + ch.seg_begin;
        // row bases of every frame-level stage, then one zero (the pooled matrix is a single run of rows)
        const size_t stride = (size_t)n + 1;
        bases.assign(stride * (size_t)(P + 1) + 1, 0);
        for (int s = 0; s <= P; s++)
            for (int64_t i = 0; i < n; i++) bases[stride * s + i + 1] = bases[stride * s + i] + xv_stage_rows(m, len[i], s);
        const size_t zero_base = stride * (size_t)(P + 1);
        // convert tiles: the segments' feature rows, then the pooled rows
        copies.clear();
        for (int64_t i = 0; i < n; i++) {
            const int32_t *sg = segs + 3 * (ch.seg_begin + i);
            const int64_t src0 = feat.offsets[(size_t)sg[0]] + sg[1];
            for (int64_t f = 0; f < len[i]; f += XV_CONVERT_ROWS)
                copies.push_back({src0 + f, bases[i] + f, (int32_t)std::min<int64_t>(XV_CONVERT_ROWS, len[i] - f), 0});
        }
        const size_t n_copy_feat = copies.size();
        for (int64_t f = 0; f < n; f += XV_CONVERT_ROWS) copies.push_back({f, f, (int32_t)std::min<int64_t>(XV_CONVERT_ROWS, n - f), 0});
        tiles_all.clear();
        for (int l = 0; l <= last; l++) {
            tile_off[(size_t)l] = tiles_all.size();
            if (l == P) continue;
            xv_layer_tiles(m, lengths.data(), ch.seg_begin, ch.seg_end, l, tiles_l);
            tiles_all.insert(tiles_all.end(), tiles_l.begin(), tiles_l.end());
        }
        tile_off[(size_t)last + 1] = tiles_all.size();
        ws.bases.upload(bases.data(), bases.size());
        ws.copy_tiles.upload(copies.data(), copies.size());
        if (!tiles_all.empty()) ws.tiles.upload(tiles_all.data(), tiles_all.size());
        const int64_t res_rows = ch.stage_rows[(size_t)last + 1];
        const int res_cols = plan.out_cols;
        if (!tap_bf16) ws.result.ensure((size_t)res_rows * res_cols);
        if (last >= P) {
            ws.pooled.ensure((size_t)n * m.width[(size_t)P + 1]);
            int wmax = 0;
            for (int s = P + 1; s <= L; s++) wmax = std::max(wmax, m.width_pad[(size_t)s]);
            ws.seg_buf[0].ensure((size_t)n * wmax);
            ws.seg_buf[1].ensure((size_t)n * wmax);
        }

        size_t ev = 0;
        interval.clear();
        auto mark = [&](int what) {      // closes the interval `what` (the first call opens the sequence)
            if (!times_ms) return;
            if (ev == ws.events.size()) {
                hipEvent_t e;
                SR_HIP(hipEventCreate(&e));
                ws.events.push_back(e);
            }
            SR_HIP(hipEventRecord(ws.events[ev++], st));
            if (what >= 0) interval.push_back(what);
        };
        mark(-1);
        hipLaunchKernelGGL(xv_convert_kernel, dim3((unsigned)n_copy_feat), dim3(256), 0, st, feat.data.p, feat.dim, m.width[0], ws.copy_tiles.p,
                           ws.buf[0].p, m.width_pad[0]);
        SR_HIP(hipGetLastError());
        mark(0);
        for (int l = 0; l <= last; l++) {
            const XvLayer &Ly = net.layers[(size_t)l];
            if (l == P) {
                float *dst = last == P ? ws.result.p : ws.pooled.p;
                hipLaunchKernelGGL(xv_pool_kernel, dim3((unsigned)n, (unsigned)((Ly.c_in + XV_POOL_COLS - 1) / XV_POOL_COLS)),
                                   dim3(XV_POOL_COLS * XV_POOL_LANES), 0, st, ws.buf[P & 1].p, m.width_pad[(size_t)P], Ly.c_in, ws.bases.p + stride * P,
                                   Ly.var_floor, dst);
                SR_HIP(hipGetLastError());
                mark(1 + l);
                if (last > P) {
                    hipLaunchKernelGGL(xv_convert_kernel, dim3((unsigned)(copies.size() - n_copy_feat)), dim3(256), 0, st, ws.pooled.p,
                                       m.width[(size_t)P + 1], m.width[(size_t)P + 1], ws.copy_tiles.p + n_copy_feat, ws.seg_buf[(P + 1) & 1].p,
                                       m.width_pad[(size_t)P + 1]);
                    SR_HIP(hipGetLastError());
                    mark(0);
                }
                continue;
            }
            const size_t nt = tile_off[(size_t)l + 1] - tile_off[(size_t)l];
            XvShifts sh = {};
            for (int j = 0; j < Ly.n_off; j++) sh.s[j] = Ly.off[j] - Ly.off[0];
            const bool frame = l < P;
            const uint16_t *A = frame ? ws.buf[l & 1].p : ws.seg_buf[l & 1].p;
            const int64_t *in_base = frame ? ws.bases.p + stride * l : ws.bases.p + zero_base;
            const int64_t *out_base = frame ? ws.bases.p + stride * (l + 1) : ws.bases.p + zero_base;
            const bool f32 = l == last && !tap_bf16;
            void *dst = f32 ? (void *)ws.result.p : frame ? (void *)ws.buf[(l + 1) & 1].p : (void *)ws.seg_buf[(l + 1) & 1].p;
            const int ldo = f32 ? Ly.c_out : m.width_pad[(size_t)l + 1];
            const dim3 grid((unsigned)nt, (unsigned)(m.n_pad[(size_t)l] / XV_TN));
            if (f32)
                launch_layer<true>(shape, grid, st, A, m.width_pad[(size_t)l], in_base, out_base, ws.tiles.p + tile_off[(size_t)l], net.d_w[(size_t)l].p,
                                   m.k_pad[(size_t)l], Ly.n_off, sh, m.width_pad[(size_t)l] / XV_GRAN, net.d_b[(size_t)l].p, net.d_scale[(size_t)l].p,
                                   net.d_shift[(size_t)l].p, Ly.act == XV_ACT_RELU, dst, ldo, Ly.c_out);
            else
                launch_layer<false>(shape, grid, st, A, m.width_pad[(size_t)l], in_base, out_base, ws.tiles.p + tile_off[(size_t)l], net.d_w[(size_t)l].p,
                                    m.k_pad[(size_t)l], Ly.n_off, sh, m.width_pad[(size_t)l] / XV_GRAN, net.d_b[(size_t)l].p, net.d_scale[(size_t)l].p,
                                    net.d_shift[(size_t)l].p, Ly.act == XV_ACT_RELU, dst, ldo, Ly.c_out);
            mark(1 + l);
        }
        // the chunk's rows of the result
        if (tap_bf16) {
            const int cp = m.width_pad[(size_t)last + 1];
            const uint16_t *src = last < P ? ws.buf[(last + 1) & 1].p : ws.seg_buf[(last + 1) & 1].p;
            ws.h_bf16.ensure((size_t)res_rows * cp);
            SR_HIP(hipMemcpyAsync(ws.h_bf16.p, src, (size_t)res_rows * cp * 2, hipMemcpyDeviceToHost, st));
            sync_stream();
            for (int64_t r = 0; r < res_rows; r++)
                for (int c = 0; c < res_cols; c++) {
                    const uint32_t u = (uint32_t)ws.h_bf16.p[(size_t)r * cp + c] << 16;
                    std::memcpy(out + (size_t)(out_row + r) * res_cols + c, &u, 4);
                }
        } else {
            ws.h_result.ensure((size_t)res_rows * res_cols);
            SR_HIP(hipMemcpyAsync(ws.h_result.p, ws.result.p, (size_t)res_rows * res_cols * 4, hipMemcpyDeviceToHost, st));
            sync_stream();
            std::memcpy(out + (size_t)out_row * res_cols, ws.h_result.p, (size_t)res_rows * res_cols * 4);
        }
        if (times_ms)
            for (size_t k = 0; k < interval.size(); k++) {
                float ms = 0.f;
                SR_HIP(hipEventElapsedTime(&ms, ws.events[k], ws.events[k + 1]));
                times_ms[interval[k]] += (double)ms;
            }
        out_row += res_rows;
    }
}

}  // namespace sr
