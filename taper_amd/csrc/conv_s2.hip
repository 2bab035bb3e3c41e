// conv_s2.hip -- the exact 3x3 convolution with stride (2, 2) and padding (1, 1), forward and both gradients, on the fp32 matrix cores
// (th_conv3x3_s2_fwd / _bwd_input / _bwd_weight; full_backward extension of the host: the reference's strided path is quirk Q9 and has
// no gradient at all).  v_mfma_f32_16x16x4_f32 is exact fp32 (a k-ordered fmaf chain), so the parity bar is the stride-1 layers'.
//
// All three are DIRECT convolutions in the design of conv3x3_mfma_kernel (conv_mfma.hip, whose header comment holds the operand
// layouts): no im2col matrix, no zero-dilated gy and no full-resolution map exist anywhere, and only the products the strided layer has
// are formed.  h_out = (h - 1) / 2 + 1; output pixel (oh, ow) has its window's top-left corner at (2 oh - 1, 2 ow - 1).
//
//   forward          D[co][px] = sum_k Wc[k][co] X[px, k], k = (ci, kh, kw).  A workgroup owns images x output rows x output columns
//                    (<= 128 pixels) and 16 CT output channels; per pass 8 input channels of the zero-haloed band
//                    [8][img_t][2 rows_t + 1][2 cols_t + 1] and the weight slab [72][16 CT] are staged.  The stride lives in a lane's
//                    pixel offset alone (il img_stride + 2 r wp + 2 c); the tap offsets are the stride-1 kernel's.
//   input gradient   gx[ih][iw] = sum_co sum_(kh, kw) gy[(ih + 1 - kh) / 2][(iw + 1 - kw) / 2] W[co][ci][kh][kw] over the taps whose
//                    quotients are whole and in range.  Input pixel (2 a + ph, 2 b + pw) belongs to parity class (ph, pw) and to QUAD
//                    (a, b); the quads are the output grid.  Even parity takes tap 1 at offset 0, odd parity tap 2 at offset 0 and tap 0
//                    at offset 1 (gy[a + 1], dropped past the last row): the classes have 1, 2, 2, 4 taps = 9 tap-products per quad, and
//                    each is a dense contraction over K = c_out x taps on the SAME staged gy patch [8][img_t][rows_t + 1][cols_t + 1].
//                    A workgroup owns <= 128 quads (512 input pixels) x 16 CT input channels and all four classes: 18 k-steps per pass.
//   weight gradient  gw[k][co] = sum_px X[px, k] gy[px][co], px = (image, oh, ow): conv3x3_wgrad_mfma_kernel with the forward's stride-2
//                    patch addressing; pixel blocks into partial slabs, wgrad_reduce (conv_mfma.hip) adds them in order.
//
// No float atomics: every result is the same bits from run to run.  What lies outside (halo, ragged band / column block / image group,
// channels past c_in or c_out) is SELECTED to zero or not stored -- never read and multiplied by zero.
#include <algorithm>

#include "common.h"
#include "conv_plan.h"
#include "conv_s2_plan.h"

namespace th {

int wgrad_reduce(th_ctx *ctx, const float *part, float *gw, int G, int kt, int c_out, int co_ld, int layout, int accumulate);   // conv_mfma.hip

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int S2_CI = 8;                  // channels of the contraction staged per pass: 72 k = 18 k-steps
constexpr int S2_KS = 18;
constexpr int S2_OOB = 0x7ffffff0;        // a byte offset beyond every buffer descriptor's range: the load returns 0
constexpr int S2_PX_MAX = 128;            // pixels (quads) per workgroup: 8 tiles of 16, two per wave
constexpr int S2_FWD_CHUNK = 1024;        // forward: floats of one channel's staged band (four per thread)
constexpr int S2_FWD_PQ = S2_FWD_CHUNK / 256;
constexpr int S2_BWI_PQ = 2;              // input gradient: a channel's gy patch is <= 4 x 128 floats (two per thread)
constexpr int S2_WG_CHUNK = 512;          // weight gradient: floats of one channel's staged band (two per thread)
constexpr int S2_WG_PQ = S2_WG_CHUNK / 256;
constexpr int S2_WG_CI = 16;              // weight gradient: input channels per slab
constexpr int S2_WG_KT = 9;               // ... = 9 k-tiles (one per tap)
constexpr int S2_WG_GP = S2_PX_MAX + 2;   // pitch of the gy tile, 2 (mod 32)
__host__ __device__ constexpr int s2_cpitch(int chunk) { return chunk + ((2 - chunk % 32) + 32) % 32; }

struct ConvS2Args {
    const float *x, *w, *bias, *gy;
    float *y;              // forward: y; input gradient: gx
    int n, c_in, h, w_in, c_out, h_out, w_out;
    int img_t, rows_t, cols_t, bands, cblks;
    int layout, relu, accumulate;
};

// element (k, co) of the weight matrix [9 c_in][c_out], k = (ci, kh, kw): layout 0 is the buffer as it lies, 1 is [co][ci][kh][kw]
__device__ __forceinline__ long s2_widx(int k, int co, int kt, int c_out, int layout) {
    return layout == 0 ? (long)k * c_out + co : (long)co * kt + k;
}

// ------------------------------------------------------------------------------------------------ forward
template <int CT>
__global__ __launch_bounds__(256) void conv3x3_s2_fwd_kernel(ConvS2Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int CO_B = 16 * CT, WN = 4 * S2_KS * CO_B, WPT = (WN + 255) / 256, PQ = S2_FWD_PQ;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l16 = lane & 15, g4 = lane >> 4;
    const int wp = 2 * a.cols_t + 1, rp = 2 * a.rows_t + 1;
    const int img_stride = rp * wp, ci_stride = a.img_t * img_stride, patch_n = S2_CI * ci_stride;
    float *patch = lds;                                        // [8][img_t][rp][wp]
    float *wsl = lds + ((patch_n + 3) & ~3);                   // [72][CO_B]
    const int cblk = blockIdx.x % a.cblks, bb = blockIdx.x / a.cblks, band = bb % a.bands, grp = bb / a.bands;
    const int img0 = grp * a.img_t, oh0 = band * a.rows_t, ow0 = cblk * a.cols_t, co0 = blockIdx.y * CO_B;
    const int rows_here = min(a.rows_t, a.h_out - oh0), cols_here = min(a.cols_t, a.w_out - ow0);
    const int px_per_img = a.rows_t * a.cols_t, m_wg = a.img_t * px_per_img;
    const int kt = 9 * a.c_in;

    // this lane's B column in its two pixel tiles: LDS offset of the window's top-left corner -- the stride is here and nowhere else
    int pix_off[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int p = (wave + 4 * q) * 16 + l16, pc = p < m_wg ? p : 0;
        const int il = pc / px_per_img, rem = pc % px_per_img;
        pix_off[q] = il * img_stride + 2 * (rem / a.cols_t) * wp + 2 * (rem % a.cols_t);
    }
    int koff[S2_KS];   // tap k = 4 s + g4 relative to the window corner: the stride-1 kernel's offsets
#pragma unroll
    for (int s = 0; s < S2_KS; ++s) {
        const int kk = 4 * s + g4, cl = kk / 9, tap = kk % 9;
        koff[s] = cl * ci_stride + (tap / 3) * wp + (tap % 3);
    }
    // staging plan, fixed for the kernel: element q = t + 256 u of a channel's chunk -> offset within a channel of image img0, or -1
    // (halo, rows / columns past the plane, images past the batch: zero)
    // Such an element gets a byte offset past the buffer descriptor's range and reads as 0 without touching memory: no select behind the
    // load, so the loads of a pass go out back to back.  The descriptor covers this workgroup's images alone (below 2 GiB: the plan).
    const int chan = a.h * a.w_in, imgs_here = min(a.img_t, a.n - img0);
    int p_goff[PQ];
#pragma unroll
    for (int u = 0; u < PQ; ++u) {
        const int q = t + 256 * u;
        p_goff[u] = S2_OOB;
        if (q < ci_stride) {
            const int il = q / img_stride, r2 = q % img_stride, rr = r2 / wp, cc = r2 % wp;
            const int ih = 2 * oh0 - 1 + rr, iw = 2 * ow0 - 1 + cc;
            if (il < imgs_here && ih >= 0 && ih < a.h && iw >= 0 && iw < a.w_in) p_goff[u] = ((il * a.c_in * chan) + ih * a.w_in + iw) * 4;
        }
    }
    const auto rx = __builtin_amdgcn_make_buffer_rsrc((void *)(a.x + (long)img0 * a.c_in * chan), 0, imgs_here * a.c_in * chan * 4, 0x00020000);

    floatx4 acc[2][CT];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[q][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    float pv[S2_CI][PQ], wv[WPT];
    // the global loads of a pass are issued back to back and parked in registers while the previous pass computes
    auto load = [&](int cb) {
#pragma unroll
        for (int cl = 0; cl < S2_CI; ++cl) {
            const bool ch_ok = cb + cl < a.c_in;                 // uniform: a channel pass past c_in reads zeros
            const int so = ch_ok ? (cb + cl) * chan * 4 : 0;
#pragma unroll
            for (int u = 0; u < PQ; ++u)
                if (256 * u < ci_stride)                         // uniform
                    pv[cl][u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, ch_ok ? p_goff[u] : S2_OOB, so, 0));
        }
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int u = t + 256 * j, kk = u / CO_B, k = cb * 9 + kk, co = co0 + u % CO_B;
            const bool ok = u < WN && k < kt && co < a.c_out;
            const float v = a.w[ok ? s2_widx(k, co, kt, a.c_out, a.layout) : 0];
            wv[j] = ok ? v : 0.f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int cl = 0; cl < S2_CI; ++cl)
#pragma unroll
            for (int u = 0; u < PQ; ++u)
                if (t + 256 * u < ci_stride) patch[cl * ci_stride + t + 256 * u] = pv[cl][u];
#pragma unroll
        for (int j = 0; j < WPT; ++j)
            if (t + 256 * j < WN) wsl[t + 256 * j] = wv[j];
    };
    load(0);
    store();
    __syncthreads();
    for (int cb = 0; cb < a.c_in; cb += S2_CI) {
        const bool more = cb + S2_CI < a.c_in;
        if (more) load(cb + S2_CI);
#pragma unroll
        for (int s = 0; s < S2_KS; ++s) {
            const float b0 = patch[pix_off[0] + koff[s]];
            const float b1 = patch[pix_off[1] + koff[s]];
            const float *wk = wsl + (4 * s + g4) * CO_B + l16;
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                const float av = wk[16 * j];
                acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc[1][j], 0, 0, 0);
            }
        }
        if (more) {
            __syncthreads();   // every wave is done reading this pass
            store();
            __syncthreads();
        }
    }
    // ---- epilogue: bias + ReLU, NCHW store straight from the D tiles (lane (l16, g4) holds pixel px0 + l16 of channels co0 + 4 g4 + i)
    const long ochan = (long)a.h_out * a.w_out;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int p = (wave + 4 * q) * 16 + l16;
        if (p >= m_wg) continue;
        const int il = p / px_per_img, rem = p % px_per_img, r = rem / a.cols_t, c = rem % a.cols_t;
        if (!(r < rows_here && c < cols_here && img0 + il < a.n)) continue;
        float *ypx = a.y + ((long)(img0 + il) * a.c_out) * ochan + (long)(oh0 + r) * a.w_out + ow0 + c;
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = co0 + 16 * j + 4 * g4 + i;
                if (co >= a.c_out) continue;
                float v = acc[q][j][i] + (a.bias ? a.bias[co] : 0.f);
                if (a.relu) v = v > 0.f ? v : 0.f;
                ypx[(long)co * ochan] = v;
            }
    }
}

// ------------------------------------------------------------------------------------------------ input gradient
// k-steps 0-1: class (0, 0), one tap; 2-5: class (0, 1); 6-9: class (1, 0); 10-17: class (1, 1), four taps
__host__ __device__ constexpr int s2_class_of_step(int s) { return s < 2 ? 0 : (s < 6 ? 1 : (s < 10 ? 2 : 3)); }
__host__ __device__ constexpr int s2_class_first(int cls) { return cls == 0 ? 0 : (cls == 1 ? 2 : (cls == 2 ? 6 : 10)); }

template <int CT>
__global__ __launch_bounds__(256, CT <= 2 ? 2 : 1) void conv3x3_s2_bwd_input_kernel(ConvS2Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int CI_B = 16 * CT, WN = 4 * S2_KS * CI_B, WPT = (WN + 255) / 256, PQ = S2_BWI_PQ;
    constexpr int WA = CI_B + 1;                                 // pitch of a weight row: odd, so that the staging's stores spread over the banks
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l16 = lane & 15, g4 = lane >> 4;
    const int wq = a.cols_t + 1, rq = a.rows_t + 1;              // quads (a, b) read gy rows a, a + 1 and columns b, b + 1
    const int img_stride = rq * wq, co_stride = a.img_t * img_stride, patch_n = S2_CI * co_stride;
    float *gp = lds;                                             // [8][img_t][rq][wq]
    float *wsl = lds + ((patch_n + 3) & ~3);                     // [72][WA], row (output channel of the pass) * 9 + tap
    const int cblk = blockIdx.x % a.cblks, bb = blockIdx.x / a.cblks, band = bb % a.bands, grp = bb / a.bands;
    const int img0 = grp * a.img_t, oh0 = band * a.rows_t, ow0 = cblk * a.cols_t, ci0 = blockIdx.y * CI_B;
    const int q_per_img = a.rows_t * a.cols_t, m_wg = a.img_t * q_per_img;
    const int kt = 9 * a.c_in;
    const long ochan = (long)a.h_out * a.w_out;

    int quad_off[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int p = (wave + 4 * q) * 16 + l16, pc = p < m_wg ? p : 0;
        const int il = pc / q_per_img, rem = pc % q_per_img;
        quad_off[q] = il * img_stride + (rem / a.cols_t) * wq + rem % a.cols_t;
    }
    // k-step s' of class (ph, pw) with T = (1 + ph)(1 + pw) taps covers k = 4 s' + g4 = (output channel of the pass) * T + tap: channel
    // g4 / T + (4 / T) s', tap g4 % T.  A tap of an even parity is kernel row 1 at offset 0, of an odd parity kernel row 2 at offset 0 or
    // kernel row 0 at offset 1.  The lane's part of both operand offsets is kept per class; the step's part is uniform.
    int bq[4][2], al[4];
#pragma unroll
    for (int cls = 0; cls < 4; ++cls) {
        const int ph = cls >> 1, pw = cls & 1, T = (1 + ph) * (1 + pw);
        const int cl = g4 / T, ti = g4 % T, tr = ti / (1 + pw), tc = ti % (1 + pw);
        const int kh = ph ? (tr ? 0 : 2) : 1, dr = ph ? tr : 0, kw = pw ? (tc ? 0 : 2) : 1, dc = pw ? tc : 0;
        bq[cls][0] = quad_off[0] + cl * co_stride + dr * wq + dc;
        bq[cls][1] = quad_off[1] + cl * co_stride + dr * wq + dc;
        al[cls] = (cl * 9 + kh * 3 + kw) * WA + l16;
    }
    // staging plan: element q = t + 256 u of an output channel's chunk -> byte offset within channel 0 of this workgroup's images, or one
    // past the descriptor's range, which reads as 0 without touching memory (gy rows / columns past the map -- the dropped taps of an even
    // side --, images past the batch)
    const int ochan_i = a.h_out * a.w_out, imgs_here = min(a.img_t, a.n - img0);
    int g_goff[PQ];
#pragma unroll
    for (int u = 0; u < PQ; ++u) {
        const int q = t + 256 * u;
        g_goff[u] = S2_OOB;
        if (q < co_stride) {
            const int il = q / img_stride, r2 = q % img_stride, oh = oh0 + r2 / wq, ow = ow0 + r2 % wq;
            if (il < imgs_here && oh < a.h_out && ow < a.w_out) g_goff[u] = (il * a.c_out * ochan_i + oh * a.w_out + ow) * 4;
        }
    }
    const auto rg = __builtin_amdgcn_make_buffer_rsrc((void *)(a.gy + (long)img0 * a.c_out * ochan), 0, imgs_here * a.c_out * ochan_i * 4, 0x00020000);

    floatx4 acc[4][2][CT];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < CT; ++j) acc[c][q][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    float pv[S2_CI][PQ], wv[WPT];
    auto load = [&](int cb) {
#pragma unroll
        for (int cl = 0; cl < S2_CI; ++cl) {
            const bool ch_ok = cb + cl < a.c_out;                // uniform: a channel pass past c_out reads zeros
            const int so = ch_ok ? (cb + cl) * ochan_i * 4 : 0;
#pragma unroll
            for (int u = 0; u < PQ; ++u)
                if (256 * u < co_stride)                         // uniform
                    pv[cl][u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, ch_ok ? g_goff[u] : S2_OOB, so, 0));
        }
        // weight element u = t + 256 j: output channel u % 8 of the pass (fastest: neighbours in memory under layout 0), tap, input channel
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int u = t + 256 * j, co = cb + u % S2_CI, tap = (u / S2_CI) % 9, ci = ci0 + u / (9 * S2_CI);
            const bool ok = u < WN && co < a.c_out && ci < a.c_in;
            const float v = a.w[ok ? s2_widx(ci * 9 + tap, co, kt, a.c_out, a.layout) : 0];
            wv[j] = ok ? v : 0.f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int cl = 0; cl < S2_CI; ++cl)
#pragma unroll
            for (int u = 0; u < PQ; ++u)
                if (t + 256 * u < co_stride) gp[cl * co_stride + t + 256 * u] = pv[cl][u];
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int u = t + 256 * j;
            if (u < WN) wsl[((u % S2_CI) * 9 + (u / S2_CI) % 9) * WA + u / (9 * S2_CI)] = wv[j];
        }
    };
    load(0);
    store();
    __syncthreads();
    for (int cb = 0; cb < a.c_out; cb += S2_CI) {
        const bool more = cb + S2_CI < a.c_out;
        if (more) load(cb + S2_CI);
#pragma unroll
        for (int s = 0; s < S2_KS; ++s) {
            const int cls = s2_class_of_step(s), sp = s - s2_class_first(cls), cstep = sp * (4 >> ((cls >> 1) + (cls & 1)));   // constants of the unrolled step
            const float b0 = gp[bq[cls][0] + cstep * co_stride];
            const float b1 = gp[bq[cls][1] + cstep * co_stride];
            const float *wk = wsl + al[cls] + cstep * 9 * WA;
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                const float av = wk[16 * j];
                acc[cls][0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc[cls][0][j], 0, 0, 0);
                acc[cls][1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc[cls][1][j], 0, 0, 0);
            }
        }
        if (more) {
            __syncthreads();
            store();
            __syncthreads();
        }
    }
    // ---- epilogue: quad (a, b) of class (ph, pw) is input pixel (2 a + ph, 2 b + pw): every pixel of the plane belongs to exactly one
    const long chan = (long)a.h * a.w_in;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int p = (wave + 4 * q) * 16 + l16;
        if (p >= m_wg) continue;
        const int il = p / q_per_img, rem = p % q_per_img, r = rem / a.cols_t, c = rem % a.cols_t;
        if (img0 + il >= a.n) continue;
        float *gimg = a.y + (long)(img0 + il) * a.c_in * chan;
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            const int ih = 2 * (oh0 + r) + (cls >> 1), iw = 2 * (ow0 + c) + (cls & 1);
            if (ih >= a.h || iw >= a.w_in) continue;
#pragma unroll
            for (int j = 0; j < CT; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ci = ci0 + 16 * j + 4 * g4 + i;
                    if (ci >= a.c_in) continue;
                    float *dst = gimg + (long)ci * chan + (long)ih * a.w_in + iw;
                    const float v = acc[cls][q][j][i];
                    *dst = a.accumulate ? *dst + v : v;
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// conv3x3_wgrad_mfma_kernel (conv_mfma.hip) on the stride-2 patch: a workgroup owns a slab of 16 input channels (9 k-tiles, one per
// tap: row l16 of a k-tile is a channel) x 16 CT output channels and walks every G-th pixel block, keeping its 9 CT accumulator tiles in
// registers; it writes ONE partial [144][16 CT] slab.
//   A operand (16 k x 4 px): lane l -> patch[pixoff[px0 + (l>>4)] + (l&15) cpitch + tap offset]
//   B operand (4 px x 16 co): lane l -> gyl[co0 + (l&15)][px0 + (l>>4)]
struct ConvS2WgradArgs {
    const float *x, *gy;
    float *part;           // [G][9 c_in][co_ld]
    int n, c_in, h, w_in, c_out, h_out, w_out;
    int img_t, rows_t, cols_t, bands, cblks, n_pb, G, co_ld;
    unsigned x_bytes, gy_bytes;   // extents of x / gy: the ranges of the kernel's buffer descriptors
};

template <int CT>
__global__ __launch_bounds__(256, 2) void conv3x3_s2_wgrad_kernel(ConvS2WgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int CO_B = 16 * CT, NPAIR = S2_WG_KT * CT, SLOTS = (NPAIR + 3) / 4, PQ = S2_WG_PQ;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l16 = lane & 15, g4 = lane >> 4;
    const int wp = 2 * a.cols_t + 1, rp = 2 * a.rows_t + 1;
    const int img_stride = rp * wp, ci_stride = a.img_t * img_stride;        // <= 512
    const int cpitch = s2_cpitch(ci_stride);
    float *patch = lds;                                                        // [16][cpitch]
    float *gyl = lds + S2_WG_CI * cpitch;                                      // [CO_B][S2_WG_GP]
    int *pixoff = reinterpret_cast<int *>(gyl + CO_B * S2_WG_GP);              // [128]
    const int cb = blockIdx.y * S2_WG_CI, co0 = blockIdx.z * CO_B;
    const int px_per_img = a.rows_t * a.cols_t, m_wg = a.img_t * px_per_img;
    const int chan = a.h * a.w_in, ochan = a.h_out * a.w_out;                  // (maps below 2 GiB: the plan refuses the rest)

    if (t < S2_PX_MAX) {   // pixel p of a block -> LDS offset of its window corner (stride 2), the same for every block
        const int il = t < m_wg ? t / px_per_img : 0, rem = t < m_wg ? t % px_per_img : 0;
        pixoff[t] = il * img_stride + 2 * (rem / a.cols_t) * wp + 2 * (rem % a.cols_t);
    }
    int pq_rel[PQ], pq_meta[PQ];          // meta = il | rr << 8 | cc << 17 | present << 26
#pragma unroll
    for (int u = 0; u < PQ; ++u) {
        const int q = t + 256 * u;
        pq_rel[u] = 0;
        pq_meta[u] = 0;
        if (q < ci_stride) {
            const int il = q / img_stride, r2 = q % img_stride, rr = r2 / wp, cc = r2 % wp;
            pq_rel[u] = il * a.c_in * chan + rr * a.w_in + cc;
            pq_meta[u] = il | (rr << 8) | (cc << 17) | (1 << 26);
        }
    }
    const int gp = t & 127, gpar = t >> 7;   // gy element: pixel t % 128, output-channel parity t / 128
    const int g_il = gp < m_wg ? gp / px_per_img : 0, g_rem = gp < m_wg ? gp % px_per_img : 0;
    const int g_r = g_rem / a.cols_t, g_c = g_rem % a.cols_t;
    int koffk[SLOTS];
    bool slot_ok[SLOTS], slot_hi[SLOTS];
    const int p_first = wave * SLOTS;
    const int ct_lo = min(p_first / S2_WG_KT, CT - 1), ct_hi = min((p_first + SLOTS - 1) / S2_WG_KT, CT - 1);
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const int p = p_first + j;
        slot_ok[j] = p < NPAIR;
        const int ct = slot_ok[j] ? p / S2_WG_KT : ct_lo, kt = slot_ok[j] ? p % S2_WG_KT : 0;
        slot_hi[j] = ct != ct_lo;
        koffk[j] = l16 * cpitch + (kt / 3) * wp + kt % 3;
    }
    floatx4 acc[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};

    // blocks are software-pipelined through registers: block pb + G is REQUESTED (buffer loads; an element outside the plane, the batch
    // or the channel range gets an offset past the buffer and reads as 0 without touching memory) before block pb's steps, stored after
    const auto rx = __builtin_amdgcn_make_buffer_rsrc((void *)a.x, 0, a.x_bytes, 0x00020000);
    const auto rg = __builtin_amdgcn_make_buffer_rsrc((void *)a.gy, 0, a.gy_bytes, 0x00020000);
    constexpr int OOB = 0x7ffffff0;
    float vp[16][PQ], vg[CO_B / 2];
    auto request = [&](int pb) {
        const int cblk = pb % a.cblks, bb = pb / a.cblks, band = bb % a.bands, grp = bb / a.bands;
        const int img0 = grp * a.img_t, oh0 = band * a.rows_t, ow0 = cblk * a.cols_t;
        const int rows_here = min(a.rows_t, a.h_out - oh0), cols_here = min(a.cols_t, a.w_out - ow0);
        const int xb = (img0 * a.c_in + cb) * chan + (2 * oh0 - 1) * a.w_in + (2 * ow0 - 1);
        int xo[PQ];
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
            const int meta = pq_meta[u];
            const int il = meta & 255, ih = 2 * oh0 - 1 + ((meta >> 8) & 511), iw = 2 * ow0 - 1 + ((meta >> 17) & 511);
            const bool ok = (meta >> 26 & 1) && ih >= 0 && ih < a.h && iw >= 0 && iw < a.w_in && img0 + il < a.n;
            xo[u] = ok ? (xb + pq_rel[u]) * 4 : OOB;
        }
#pragma unroll
        for (int cl = 0; cl < 16; ++cl)
#pragma unroll
            for (int u = 0; u < PQ; ++u)
                vp[cl][u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, (cb + cl < a.c_in) ? xo[u] : OOB, cl * chan * 4, 0));
        const bool pok = gp < m_wg && g_r < rows_here && g_c < cols_here && img0 + g_il < a.n;
        const int go = pok ? (((img0 + g_il) * a.c_out + co0 + gpar) * ochan + (oh0 + g_r) * a.w_out + ow0 + g_c) * 4 : OOB;
#pragma unroll
        for (int i = 0; i < CO_B / 2; ++i)
            vg[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, (co0 + 2 * i + gpar < a.c_out) ? go : OOB, 2 * i * ochan * 4, 0));
    };
    const int n_steps = (m_wg + 3) / 4;
    if ((int)blockIdx.x < a.n_pb) request(blockIdx.x);
    for (int pb = blockIdx.x; pb < a.n_pb; pb += a.G) {
        __syncthreads();   // the previous block's MFMAs are done with patch / gyl (and pixoff is written)
#pragma unroll
        for (int cl = 0; cl < 16; ++cl)
#pragma unroll
            for (int u = 0; u < PQ; ++u)
                if (pq_meta[u] >> 26 & 1) patch[cl * cpitch + t + 256 * u] = vp[cl][u];
#pragma unroll
        for (int i = 0; i < CO_B / 2; ++i) gyl[(2 * i + gpar) * S2_WG_GP + gp] = vg[i];
        __syncthreads();
        if (pb + a.G < a.n_pb) request(pb + a.G);
        // reduction steps of 4 pixels (pixels past m_wg, rows past the band, columns past the block are zero columns of gyl)
        for (int rs = 0; rs < n_steps; ++rs) {
            const int px = 4 * rs + g4;
            const int po = pixoff[px];
            const float b_lo = gyl[(ct_lo * 16 + l16) * S2_WG_GP + px];
            const float b_hi = gyl[(ct_hi * 16 + l16) * S2_WG_GP + px];
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const float av = patch[po + koffk[j]];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, slot_hi[j] ? b_hi : b_lo, acc[j], 0, 0, 0);
            }
        }
    }
    // one partial slab per workgroup: part[g][k][co]  (D tile: row = channel 4 g4 + i of the slab, column = co l16; tile = tap kt)
    float *pp = a.part + (long)blockIdx.x * 9 * a.c_in * a.co_ld;
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const int p = p_first + j;
        if (p >= NPAIR) continue;
        const int ct = p / S2_WG_KT, kt = p % S2_WG_KT;
        const int co = co0 + ct * 16 + l16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ch = cb + 4 * g4 + i;
            if (ch < a.c_in && co < a.co_ld) pp[(long)(ch * 9 + kt) * a.co_ld + co] = acc[j][i];
        }
    }
}

// ------------------------------------------------------------------------------------------------ plans (host data, no device call)
// images x rows x columns per workgroup tile: the fullest tiling of <= 128 pixels of the output grid whose staged chunk of one channel
// (per_px_rows(r) x per_px_cols(c) floats per image) stays within chunk_cap; rows wider than col_max are cut into equal column blocks
// (by_steps, the weight gradient: the tiling that takes the fewest 4-pixel reduction steps per image instead -- the kernel's steps stop at
// the block's pixels, as in conv_wgrad_plan)
// (img_max: the images one buffer descriptor may cover)
static void s2_tile_plan(ConvS2Plan *p, int n, int h_out, int w_out, int chunk_cap, int col_max, bool quads, bool by_steps = false, long img_max = 128) {
    p->h_out = h_out; p->w_out = w_out;
    p->cblks = ceil_div(w_out, col_max);
    p->cols_t = ceil_div(w_out, p->cblks);
    p->cblks = ceil_div(w_out, p->cols_t);
    const int c = p->cols_t, cw = quads ? c + 1 : 2 * c + 1;
    long best_fill = -(1L << 62);
    p->img_t = 1; p->rows_t = 1;
    for (int r = 1; r <= h_out; ++r) {
        if (r * c > S2_PX_MAX) break;
        const int rh = quads ? r + 1 : 2 * r + 1;
        int im = std::min(n, S2_PX_MAX / (r * c));
        im = (int)std::min<long>(std::min(im, chunk_cap / (rh * cw)), img_max);
        if (im < 1) continue;
        const int bands = ceil_div(h_out, r);
        // useful pixels per 128-pixel workgroup slot, counting the ragged last band; fewer, taller bands on ties (less halo re-read)
        const long fill = by_steps ? -((long)bands * ceil_div((long)im * r * c, 4) * 1000 / im)
                                   : (long)h_out * w_out * im * 1000 / ((long)bands * p->cblks * S2_PX_MAX);
        if (fill >= best_fill) { best_fill = fill; p->img_t = im; p->rows_t = r; }
    }
    p->bands = ceil_div(h_out, p->rows_t);
}

// 16-channel tiles per workgroup: up to 64 channels, halved when the launch has fewer than 1.5 workgroups per CU (conv3x3_mfma_plan's rule)
static int s2_ct(int channels, long tiles) {
    const int c_tiles = ceil_div(channels, 16);
    int ct = c_tiles >= 4 ? 4 : (c_tiles >= 2 ? 2 : 1);
    if (ct == 4 && tiles * ceil_div(channels, 64) < 384) ct = 2;
    return ct;
}

static void s2_grid(ConvS2Plan *p, int n, int channels) {
    const long tiles = (long)ceil_div(n, p->img_t) * p->bands * p->cblks;
    p->ct = s2_ct(channels, tiles);
    p->grid_y = ceil_div(channels, 16 * p->ct); p->grid_z = 1;
    if (tiles > 0x7fffffffL || p->grid_y > 65535) { p->refused = CONV_S2_REFUSED_GRID; p->grid_x = 1; return; }
    p->grid_x = (int)tiles;
}

void conv3x3_s2_fwd_plan(ConvS2Plan *p, int n, int c_in, int h, int w, int c_out) {
    *p = ConvS2Plan{};
    p->op = 0;
    // a workgroup's images lie behind one buffer descriptor with 32-bit byte offsets: below 2 GiB (one image of more is refused)
    const long img_floats = (long)c_in * h * w, img_max = ((1L << 29) - 1) / img_floats;
    s2_tile_plan(p, n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, S2_FWD_CHUNK, S2_PX_MAX, false, false, std::max(1L, img_max));
    s2_grid(p, n, c_out);
    if (img_max < 1) p->refused = CONV_S2_REFUSED_2GIB;
    const size_t patch_n = (size_t)S2_CI * p->img_t * (2 * p->rows_t + 1) * (2 * p->cols_t + 1);
    p->lds = (int)((((patch_n + 3) & ~(size_t)3) + (size_t)72 * 16 * p->ct) * sizeof(float));
    p->lds_limit = 64 << 10;
}

void conv3x3_s2_bwd_input_plan(ConvS2Plan *p, int n, int c_in, int h, int w, int c_out, bool accumulate) {
    *p = ConvS2Plan{};
    p->op = 1; p->acc = accumulate;
    const long img_floats = (long)c_out * ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1), img_max = ((1L << 29) - 1) / img_floats;
    s2_tile_plan(p, n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, 256 * S2_BWI_PQ, S2_PX_MAX, true, false, std::max(1L, img_max));
    s2_grid(p, n, c_in);
    if (img_max < 1) p->refused = CONV_S2_REFUSED_2GIB;
    const size_t patch_n = (size_t)S2_CI * p->img_t * (p->rows_t + 1) * (p->cols_t + 1);
    p->lds = (int)((((patch_n + 3) & ~(size_t)3) + (size_t)72 * (16 * p->ct + 1)) * sizeof(float));
    p->lds_limit = 64 << 10;
}

void conv3x3_s2_bwd_weight_plan(ConvS2Plan *p, int n, int c_in, int h, int w, int c_out, int layout, bool accumulate, bool gw_aligned) {
    *p = ConvS2Plan{};
    p->op = 2; p->acc = accumulate;
    s2_tile_plan(p, n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, S2_WG_CHUNK, 64, false, true);
    const long n_pb = (long)ceil_div(n, p->img_t) * p->bands * p->cblks;
    const int c_tiles = ceil_div(c_out, 16);
    p->ct = c_tiles >= 4 ? 4 : (c_tiles >= 2 ? 2 : 1);
    const int co_b = 16 * p->ct, slabs = ceil_div(c_in, S2_WG_CI), co_blocks = ceil_div(c_out, co_b);
    p->co_ld = co_blocks * co_b;
    const size_t xb = (size_t)n * c_in * h * w * 4, gb = (size_t)n * c_out * p->h_out * p->w_out * 4;
    if (xb >= (1u << 31) || gb >= (1u << 31) || n_pb > 0x7fffffffL || slabs > 65535 || co_blocks > 65535) {
        p->refused = n_pb > 0x7fffffffL || slabs > 65535 || co_blocks > 65535 ? CONV_S2_REFUSED_GRID : CONV_S2_REFUSED_2GIB;
        p->grid_x = p->grid_y = p->grid_z = 1;
        return;
    }
    p->n_pb = (int)n_pb;
    int G = ceil_div(2 * kNumCU, (long)slabs * co_blocks);      // two workgroups per CU in total
    G = std::max(1, std::min(G, std::min(p->n_pb, 512)));
    p->G = G; p->slabs = G;
    const int ci_stride = p->img_t * (2 * p->rows_t + 1) * (2 * p->cols_t + 1);
    p->lds = (int)((S2_WG_CI * (size_t)s2_cpitch(ci_stride) + (size_t)co_b * S2_WG_GP) * sizeof(float) + S2_PX_MAX * sizeof(int));
    p->lds_limit = 160 << 10;
    p->grid_x = G; p->grid_y = slabs; p->grid_z = co_blocks;
    p->reduce = wgrad_reduce_plan(G, 9 * c_in, c_out, p->co_ld, layout, accumulate, gw_aligned);
}

// what this thread's most recent stride-2 launch ran (th_debug_last_conv_s2_config)
thread_local int t_last_s2_cfg[8] = {-1, 0, 0, 0, 0, 0, 0, 0};
static void s2_note(const ConvS2Plan &p) {
    const int v[8] = {p.op, p.ct, p.acc, p.grid_x, p.grid_y, p.grid_z, p.lds, p.reduce};
    for (int i = 0; i < 8; ++i) t_last_s2_cfg[i] = v[i];
}

static void s2_args(ConvS2Args *a, const ConvS2Plan &p, int n, int c_in, int h, int w, int c_out, int layout) {
    a->n = n; a->c_in = c_in; a->h = h; a->w_in = w; a->c_out = c_out; a->h_out = p.h_out; a->w_out = p.w_out;
    a->img_t = p.img_t; a->rows_t = p.rows_t; a->cols_t = p.cols_t; a->bands = p.bands; a->cblks = p.cblks;
    a->layout = layout;
}

}  // namespace th

using namespace th;

#define TH_S2_CHECK(NAME, P0, P1, P2)                                                                                                    \
    TH_REQUIRE(ctx && (P0) && (P1) && (P2), NAME ": null argument");                                                                     \
    TH_REQUIRE(n >= 1 && c_in >= 1 && h >= 1 && w >= 1 && c_out >= 1, NAME ": bad geometry n=%d c_in=%d h=%d w=%d c_out=%d (all must be >= 1)", \
               n, c_in, h, w, c_out);                                                                                                    \
    TH_REQUIRE(weight_layout == 0 || weight_layout == 1, NAME ": weight_layout must be 0 (taper) or 1 (standard), got %d", weight_layout)

extern "C" {

int th_conv3x3_s2_fwd(th_ctx *ctx, const float *d_x, const float *d_w, const float *d_bias, float *d_y, int n, int c_in, int h, int w,
                      int c_out, int weight_layout, int relu) {
    TH_S2_CHECK("th_conv3x3_s2_fwd", d_x, d_w, d_y);
    TH_REQUIRE(relu == 0 || relu == 1, "th_conv3x3_s2_fwd: relu must be 0 or 1, got %d", relu);
    ConvS2Plan p;
    conv3x3_s2_fwd_plan(&p, n, c_in, h, w, c_out);
    TH_REQUIRE(!p.refused, "th_conv3x3_s2_fwd: one image of 2 GiB and more, or a launch grid over the device limit (not supported)");
    ConvS2Args a{};
    s2_args(&a, p, n, c_in, h, w, c_out, weight_layout);
    a.x = d_x; a.w = d_w; a.bias = d_bias; a.y = d_y; a.relu = relu;
    const dim3 grid(p.grid_x, p.grid_y);
    switch (p.ct) {
        case 4: hipLaunchKernelGGL(conv3x3_s2_fwd_kernel<4>, grid, dim3(256), (size_t)p.lds, ctx->stream, a); break;
        case 2: hipLaunchKernelGGL(conv3x3_s2_fwd_kernel<2>, grid, dim3(256), (size_t)p.lds, ctx->stream, a); break;
        default: hipLaunchKernelGGL(conv3x3_s2_fwd_kernel<1>, grid, dim3(256), (size_t)p.lds, ctx->stream, a); break;
    }
    TH_LAUNCH_CHECK();
    s2_note(p);
    return 0;
}

int th_conv3x3_s2_bwd_input(th_ctx *ctx, const float *d_gy, const float *d_w, float *d_gx, int n, int c_in, int h, int w, int c_out,
                            int weight_layout, int accumulate) {
    TH_S2_CHECK("th_conv3x3_s2_bwd_input", d_gy, d_w, d_gx);
    TH_REQUIRE(accumulate == 0 || accumulate == 1, "th_conv3x3_s2_bwd_input: accumulate must be 0 or 1, got %d", accumulate);
    ConvS2Plan p;
    conv3x3_s2_bwd_input_plan(&p, n, c_in, h, w, c_out, accumulate != 0);
    TH_REQUIRE(!p.refused, "th_conv3x3_s2_bwd_input: one image of 2 GiB and more, or a launch grid over the device limit (not supported)");
    ConvS2Args a{};
    s2_args(&a, p, n, c_in, h, w, c_out, weight_layout);
    a.gy = d_gy; a.w = d_w; a.y = d_gx; a.accumulate = accumulate;
    const dim3 grid(p.grid_x, p.grid_y);
    switch (p.ct) {
        case 4: hipLaunchKernelGGL(conv3x3_s2_bwd_input_kernel<4>, grid, dim3(256), (size_t)p.lds, ctx->stream, a); break;
        case 2: hipLaunchKernelGGL(conv3x3_s2_bwd_input_kernel<2>, grid, dim3(256), (size_t)p.lds, ctx->stream, a); break;
        default: hipLaunchKernelGGL(conv3x3_s2_bwd_input_kernel<1>, grid, dim3(256), (size_t)p.lds, ctx->stream, a); break;
    }
    TH_LAUNCH_CHECK();
    s2_note(p);
    return 0;
}

int th_conv3x3_s2_bwd_weight(th_ctx *ctx, const float *d_x, const float *d_gy, float *d_gw, int n, int c_in, int h, int w, int c_out,
                             int weight_layout, int accumulate) {
    TH_S2_CHECK("th_conv3x3_s2_bwd_weight", d_x, d_gy, d_gw);
    TH_REQUIRE(accumulate == 0 || accumulate == 1, "th_conv3x3_s2_bwd_weight: accumulate must be 0 or 1, got %d", accumulate);
    ConvS2Plan p;
    conv3x3_s2_bwd_weight_plan(&p, n, c_in, h, w, c_out, weight_layout, accumulate != 0, ((uintptr_t)d_gw & 15) == 0);
    // (checked before the slabs are taken from the pool: an error return holds nothing)
    TH_REQUIRE(!p.refused, "th_conv3x3_s2_bwd_weight: maps of 2 GiB and more, or a launch grid over the device limit (not supported)");
    const int kt = 9 * c_in;
    void *ws = nullptr;
    if (th_malloc(ctx, (size_t)p.slabs * kt * p.co_ld * sizeof(float), &ws)) return 1;
    ConvS2WgradArgs a{};
    a.x = d_x; a.gy = d_gy; a.part = (float *)ws;
    a.n = n; a.c_in = c_in; a.h = h; a.w_in = w; a.c_out = c_out; a.h_out = p.h_out; a.w_out = p.w_out;
    a.img_t = p.img_t; a.rows_t = p.rows_t; a.cols_t = p.cols_t; a.bands = p.bands; a.cblks = p.cblks;
    a.n_pb = p.n_pb; a.G = p.G; a.co_ld = p.co_ld;
    a.x_bytes = (unsigned)((size_t)n * c_in * h * w * 4);
    a.gy_bytes = (unsigned)((size_t)n * c_out * p.h_out * p.w_out * 4);
    const dim3 grid(p.grid_x, p.grid_y, p.grid_z);
    const size_t lds = (size_t)p.lds;
    hipError_t attr = hipSuccess;
#define TH_S2_WG(CT_)                                                                                                                    \
    do {                                                                                                                                \
        auto kern = conv3x3_s2_wgrad_kernel<CT_>;                                                                                       \
        if (lds > (64u << 10)) attr = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);    \
        if (attr == hipSuccess) hipLaunchKernelGGL(kern, grid, dim3(256), lds, ctx->stream, a);                                         \
    } while (0)
    switch (p.ct) {
        case 4: TH_S2_WG(4); break;
        case 2: TH_S2_WG(2); break;
        default: TH_S2_WG(1); break;
    }
#undef TH_S2_WG
    if (attr != hipSuccess || hipGetLastError() != hipSuccess) { th_free(ctx, ws); th::set_error("conv3x3_s2_wgrad_kernel: launch failed"); return 1; }
    if (int rc = wgrad_reduce(ctx, a.part, d_gw, p.G, kt, c_out, p.co_ld, weight_layout, accumulate)) { th_free(ctx, ws); return rc; }
    s2_note(p);
    return th_free(ctx, ws);
}

int th_debug_conv3x3_s2_plan(int op, int n, int c_in, int h, int w, int c_out, int weight_layout, int relu_bias, int accumulate,
                             int w_misalign_bytes, int *outN) {
    TH_REQUIRE(outN, "th_debug_conv3x3_s2_plan: null output");
    TH_REQUIRE(op >= 0 && op <= 2, "th_debug_conv3x3_s2_plan: op must be 0 (fwd), 1 (bwd_input) or 2 (bwd_weight), got %d", op);
    TH_REQUIRE(n >= 1 && c_in >= 1 && h >= 1 && w >= 1 && c_out >= 1, "th_debug_conv3x3_s2_plan: bad geometry n=%d c_in=%d h=%d w=%d c_out=%d", n, c_in,
               h, w, c_out);
    TH_REQUIRE(weight_layout == 0 || weight_layout == 1, "th_debug_conv3x3_s2_plan: weight_layout must be 0 (taper) or 1 (standard)");
    TH_REQUIRE(relu_bias >= 0 && relu_bias <= 3 && (op == 0 || relu_bias == 0),
               "th_debug_conv3x3_s2_plan: relu_bias is relu + 2 * bias present (0 .. 3; 0 for the two backward ops), got %d", relu_bias);
    TH_REQUIRE(accumulate == 0 || (accumulate == 1 && op >= 1), "th_debug_conv3x3_s2_plan: accumulate is 0, or 1 for the two backward ops");
    TH_REQUIRE(w_misalign_bytes >= 0 && w_misalign_bytes < 16 && w_misalign_bytes % 4 == 0,
               "th_debug_conv3x3_s2_plan: w_misalign_bytes must be 0, 4, 8 or 12");
    ConvS2Plan p;
    if (op == 0) conv3x3_s2_fwd_plan(&p, n, c_in, h, w, c_out);
    else if (op == 1) conv3x3_s2_bwd_input_plan(&p, n, c_in, h, w, c_out, accumulate != 0);
    else conv3x3_s2_bwd_weight_plan(&p, n, c_in, h, w, c_out, weight_layout, accumulate != 0, w_misalign_bytes == 0);
    const int *src = reinterpret_cast<const int *>(&p);
    for (int i = 0; i < kConvS2PlanInts; ++i) outN[i] = src[i];
    return 0;
}

int th_debug_last_conv_s2_config(th_ctx *ctx, int *out8) {
    TH_REQUIRE(ctx && out8, "th_debug_last_conv_s2_config: null argument");
    for (int i = 0; i < 8; ++i) out8[i] = th::t_last_s2_cfg[i];
    return 0;
}

}  // extern "C"
