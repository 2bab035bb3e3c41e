// qconv_i8.hip -- calibrated int8 convolution: an implicit GEMM on the integer matrix cores (v_mfma_i32_32x32x32_i8) over
// channel-last codes, on qi8_dev.h's piece, stage image, epilogue value and window -- the ones qgemm_i8.hip's product uses.
//
//   th_quantize_act_nhwc_int8  f32 [n, c, h, w] -> int8 codes [n, h, w, cpitch] (th_quantize_act_int8's codec) and the int32 sum of each
//                              pixel's codes; one launch, the NCHW -> NHWC turn through LDS
//   th_pack_conv_weight_int8   packed codes [c_out, c_in, k_h, k_w] -> [c_out][k_h k_w][cpitch] with zero padding (once per weight);
//                              th_pack_conv_weight_taper_int8: the same from a weight in the float conv kernels' weight_layout 0
//   th_conv2d_q8q8_fwd         y = sx * (sw * (float)(acc + 128 rs) + mw * (float)rs) [+ deq(bias)] [ReLU] into f32 NCHW; acc = the sum
//                              over the in-image taps of qx qw from the MFMA, rs = the sum of d_pixsum over the same taps
//   th_conv2d_q8q8_fwd_codes   the same product, its f32 value coded at once with the NEXT layer's scale: int8 [n, h_out, w_out, cpitch_y]
//                              and the pixel sums, what th_quantize_act_nhwc_int8 would make of th_conv2d_q8q8_fwd's output
//   th_conv2d_q8q8_fwd_pc, th_conv2d_q8q8_fwd_codes_pc: both with one {mw, sw} per output channel, a template flag of the kernel
//   th_conv2d_q8q8_fwd_affine, th_conv2d_q8q8_fwd_codes_affine: both with a frozen BatchNorm2d behind the bias, y = v a[co] + b[co], then the
//                              ReLU: one more template flag, the pairs {a, b} staged beside the weight pairs
//   th_conv2d_q8q8_fwd_residual, th_conv2d_q8q8_fwd_codes_residual: the affine twins with a skip connection's value added behind the affine and in
//                              front of the ReLU: an f32 NCHW map of the output's shape, or channel-last codes with their scale
//   th_maxpool2d_nhwc_int8     the max-pool on channel-last codes (the codec is monotone: the maximum of the codes is the code of the maximum)
//
// With both operands channel-last a 16-byte piece of K is 16 consecutive channels of one tap: M = n h_out w_out output pixels, N = c_out,
// K = k_h k_w cpitch.  The im2col matrix exists only as addresses; an out-of-image tap is a zero piece, and code 0 IS value 0, so padding
// adds nothing to acc or rs.  A pixel's result depends on its own window alone: nothing of the tiling reaches the arithmetic.
#include "common.h"
#include "qi8_dev.h"

namespace th {

constexpr int kQcPix = 128;        // output pixels per workgroup: four waves of 32
constexpr int kQcChan = 32;        // channels per MFMA tile; a workgroup takes NT of them (1, 2 or 4)
constexpr int kQcTurnPix = 64;     // th_quantize_act_nhwc_int8: pixels ...
constexpr int kQcTurnChan = 64;    // ... by channels of one LDS turn
constexpr int kQcTurnPitch = 20;   // words per pixel row of the turn: 16 of codes, 4 of padding (a row stays 16-byte aligned)

// ---- activations -> channel-last codes ----
// A workgroup turns 64 consecutive pixels of one image, 64 channels at a time.  In: lane = pixel, so a wave's load is 64 consecutive
// floats of one channel plane; a thread packs four consecutive channels into one LDS word.  Out: four lanes per pixel, one 16-byte piece
// each -- 64 consecutive bytes per pixel, the whole wave contiguous when cpitch == 64.  Channels c .. cpitch - 1 get the code 0.
__global__ __launch_bounds__(256) void quantize_act_nhwc_kernel(const float *__restrict__ x, int n, int c, int hw, const float *__restrict__ d_scale,
                                                                int8_t *__restrict__ q, int cpitch, int *__restrict__ pixsum, int tiles_per_img) {
    __shared__ uint4 turn[kQcTurnPix * kQcTurnPitch / 4];   // 5 KB
    uint32_t *turn_w = (uint32_t *)turn;
    const int t = threadIdx.x, pin = t & 63, cq = t >> 6, pout = t >> 2, piece = t & 3;
    const float scale = d_scale[0];
    const long tiles = (long)n * tiles_per_img;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int img = (int)(tile / tiles_per_img), p0 = (int)(tile - (long)img * tiles_per_img) * kQcTurnPix;
        const float *xi = x + (size_t)img * c * hw;
        int sum = 0;
        for (int cb = 0; cb < cpitch; cb += kQcTurnChan) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint32_t word = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ch = cb + 16 * i + 4 * cq + j;
                    if (ch < c && p0 + pin < hw) word |= code_at(act_code(xi[(size_t)ch * hw + p0 + pin], scale), j);
                }
                turn_w[pin * kQcTurnPitch + 4 * i + cq] = word;
            }
            __syncthreads();
            if (p0 + pout < hw && cb + 16 * piece < cpitch) {
                const uint4 v = turn[pout * (kQcTurnPitch / 4) + piece];
                sum += piece_sum(v);
                *(uint4 *)(q + ((size_t)img * hw + p0 + pout) * cpitch + cb + 16 * piece) = v;
            }
            __syncthreads();
        }
        sum += __shfl_xor(sum, 1, 64);   // the four lanes of a pixel (integers: any order gives the same bits)
        sum += __shfl_xor(sum, 2, 64);
        if (piece == 0 && p0 + pout < hw) pixsum[(size_t)img * hw + p0 + pout] = sum;
    }
}

// ---- the product ----
struct QcArgs {
    const int8_t *qx, *qw;
    const int *pixsum;
    const float *xscale, *wparams;
    const int8_t *qb;
    const float *bparams;
    float *y;   // the f32 form's output; the codes form's are the next four (null / 0 in the f32 form)
    const float *yscale;
    int8_t *qy;
    int *ypixsum;
    int cpitch_y;
    QWindow win;
    int cpitch, c_out, M, relu, tiles_n;
    const float *affine;   // AFFINE: {a, b} per output channel (null otherwise)
    const float *res;      // RES == 1: the f32 residual [n][c_out][h_out][w_out]
    const int8_t *res_q;   // RES == 2: the residual's codes [n][h_out][w_out][cpitch_r] with the scale *res_scale
    const float *res_scale;
    int cpitch_r;
};

// A workgroup owns 128 output pixels (any run of the n h_out w_out list: it may span map rows and images) by 32 NT channels; wave v
// owns pixels 32 v .. 32 v + 31 against every channel tile.  A stage is 64 bytes of K = four pieces; piece g of K is channels
// 16 (g % cp16) .. + 15 of tap g / cp16 for BOTH operands, so the fragments pair code with code (qi8_dev.h).  The weights are
// the A operand and the pixels the B operand: C column = lane & 31 is a pixel, C row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) a
// channel, and a wave's store of one register is 32 consecutive pixels of one channel plane.
// CODES (tiles_n == 1: the workgroup sees every channel of its pixels): the epilogue's f32 value goes through the activation codec with the
// next layer's scale instead of to memory.  An accumulator group (reg >> 2) is four consecutive channels = one word of the pixel's
// channel-last row, the lane's at byte 8 (reg >> 2) + 4 (lane >> 5) of a 32-channel tile; two half-wave swaps (v_permlane32_swap) with
// the lane that holds the other half of the same pixel leave 16 consecutive bytes in each, so a tile of a pixel is two 16-byte stores.
// PC: wparams holds one {mw, sw} per output channel.  A lane needs the pairs of its 16 NT channels: the workgroup's 32 NT
// pairs are staged once in the LDS the K loop has released (its last barrier is behind every read of a stage), one pair a thread, and
// the epilogue reads them from there -- 16 NT dependent loads from memory a lane cost 2.6 - 7.5 us a layer, measured; this costs 0.0 - 0.6.
// AFFINE: a frozen BatchNorm2d behind the layer: the value is q8_value without its ReLU, then __fadd_rn(__fmul_rn(v, a), b) with
// the channel's {a, b}, then the ReLU.  The workgroup's 32 NT pairs are staged like the weight pairs, behind them and the same barrier.
// RES (with AFFINE): a skip connection's value r is added behind the affine and in front of the ReLU (affine_residual_value).
// 1: r is read from an f32 map of the output's shape at the f32 store's address pattern, 32 consecutive pixels of one channel plane a wave
// access, a tile's 16 values requested before the first is used (each loaded next to its use cost 3 - 11 us a call, measured).
// 2: r = __fmul_rn((float)qr, *res_scale) with qr the code at byte co of the pixel's row of a channel-last map; an accumulator
// group's four channels are one word of that row, at byte 8 (reg >> 2) + 4 (lane >> 5) of the tile -- four dword loads a tile, the words
// the codes form's swaps would gather.  A pixel past M and a word whose first channel is past c_out are not read.
template <int NT, bool CODES, bool PC, bool AFFINE = false, int RES = 0>
__global__ __launch_bounds__(256) void qconv_i8_kernel(QcArgs a) {
    __shared__ uint4 lds_x[2][kQcPix * 4];          // 16 KB
    __shared__ uint4 lds_w[2][kQcChan * NT * 4];    // 4 / 8 / 16 KB
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, h = lane >> 5;
    const int tile_m = blockIdx.x / a.tiles_n, tile_n = blockIdx.x - tile_m * a.tiles_n;
    const int m0 = tile_m * kQcPix, col0 = CODES ? 0 : tile_n * kQcChan * NT;   // (CODES: tiles_n == 1)
    const int cp16 = a.cpitch >> 4, taps = a.win.k_h * a.win.k_w, pieces = taps * cp16, nk = (pieces + 3) >> 2, hw_out = a.win.h_out * a.win.w_out;

    // staging: thread t brings piece t & 3 of pixel rows t >> 2 and (t >> 2) + 64, and of weight rows (t >> 2) + 64 i below 32 NT
    const int srow = t >> 2, piece = t & 3;
    const int8_t *px[2];
    int ih0[2], iw0[2];   // the window's first tap in the image; a pixel past M gets a window that no tap of is inside any image
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + srow + 64 * i;
        const bool live = m < a.M;
        const QWindow::Pixel o = a.win.split(live ? m : 0);
        ih0[i] = live ? a.win.top(o.oh) : -a.win.k_h;
        iw0[i] = a.win.left(o.ow);
        px[i] = a.qx + (size_t)o.img * a.win.h * a.win.w * a.cpitch;
    }
    constexpr int WL = (NT + 1) / 2;   // weight pieces a thread stages
    const size_t wrow_bytes = (size_t)pieces * 16;
    uint4 gx[2], gw[WL];
    auto fetch = [&](int kt) {
        const int g = kt * 4 + piece;
        const bool in_k = g < pieces;
        const int tap = g / cp16, cpiece = g - tap * cp16, kh = tap / a.win.k_w, kw = tap - kh * a.win.k_w;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ih = ih0[i] + kh, iw = iw0[i] + kw;
            const bool inside = in_k && ih >= 0 && ih < a.win.h && iw >= 0 && iw < a.win.w;
            gx[i] = inside ? *(const uint4 *)(px[i] + ((size_t)ih * a.win.w + iw) * a.cpitch + cpiece * 16) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < WL; ++i) {
            const int row = srow + 64 * i;   // (rows past c_out re-read the last row: never stored)
            gw[i] = in_k && row < kQcChan * NT ? *(const uint4 *)(a.qw + (size_t)min(col0 + row, a.c_out - 1) * wrow_bytes + (size_t)g * 16)
                                               : make_uint4(0, 0, 0, 0);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) lds_x[buf][stage_slot(srow + 64 * i, piece)] = gx[i];
#pragma unroll
        for (int i = 0; i < WL; ++i)
            if (srow + 64 * i < kQcChan * NT) lds_w[buf][stage_slot(srow + 64 * i, piece)] = gw[i];
    };

    intx16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0;

    fetch(0);
    stage(0);
    lds_barrier();
    int buf = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) fetch(kt + 1);   // in flight under this stage's MFMAs
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const intx4 xf = stage_frag(lds_x[buf], wave * 32 + li, s, h);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(stage_frag(lds_w[buf], 32 * j + li, s, h), xf, acc[j], 0, 0, 0);
        }
        if (kt + 1 < nk) stage(buf ^ 1);   // (read last in step kt - 1: every wave passed that step's barrier)
        lds_barrier();
        buf ^= 1;
    }

    // epilogue: this lane's pixel, its window's sum of pixel sums (integer; border windows have fewer taps), then q8_value of the lane's 16 NT
    // channels.  A pixel past M: the f32 form is done; the codes form keeps both its lanes (they share m) in the swaps and stores nothing.
    float2 *pairs = (float2 *)lds_w;   // PC: {mw, sw} of channel col0 + i at pairs[i] (channels past c_out re-read the last: never used)
    if constexpr (PC) {
        if (t < kQcChan * NT) {
            const int co = min(col0 + t, a.c_out - 1);
            pairs[t] = make_float2(a.wparams[2 * co], a.wparams[2 * co + 1]);
        }
    }
    float2 *ab = pairs + kQcChan * NT;   // AFFINE: {a, b} of channel col0 + i at ab[i]
    if constexpr (AFFINE) {
        if (t < kQcChan * NT) {
            const int co = min(col0 + t, a.c_out - 1);
            ab[t] = make_float2(a.affine[2 * co], a.affine[2 * co + 1]);
        }
    }
    if constexpr (PC || AFFINE) lds_barrier();
    const int m = m0 + wave * 32 + li;
    const bool live = m < a.M;
    if (!CODES && !live) return;
    const QWindow::Pixel o = a.win.split(live ? m : 0);
    const int *ps = a.pixsum + (size_t)o.img * a.win.h * a.win.w;
    int rs = 0;
    if (live) a.win.for_taps(o.oh, o.ow, [&](int ih, int iw) { rs += ps[ih * a.win.w + iw]; });
    const float sx = a.xscale[0], mw = PC ? 0.f : a.wparams[0], sw = PC ? 0.f : a.wparams[1], rterm = q8_rterm(mw, rs), sy = CODES ? a.yscale[0] : 0.f;
    float *yp = CODES ? nullptr : a.y + ((size_t)o.img * a.c_out + col0 + 4 * h) * hw_out + o.p;   // the f32 form: this pixel in the lane's first channel plane
    const float *rp = nullptr;      // RES == 1: this pixel in the residual's plane of the lane's first channel
    const uint32_t *rrow = nullptr; // RES == 2: the word at byte col0 + 4 h of this pixel's row of residual codes
    float sr = 0.f;
    if constexpr (RES == 1) rp = a.res + ((size_t)o.img * a.c_out + col0 + 4 * h) * hw_out + o.p;
    if constexpr (RES == 2) {
        rrow = (const uint32_t *)(a.res_q + (size_t)(live ? m : 0) * a.cpitch_r + col0 + 4 * h);
        sr = a.res_scale[0];
    }
    int sum = 0;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        uint32_t rw[4] = {0, 0, 0, 0};   // RES == 2: the lane's four words of this tile
        if constexpr (RES == 2) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (live && col0 + 32 * j + 8 * g + 4 * h < a.c_out) rw[g] = rrow[8 * j + 2 * g];
        }
        float rv[16];   // RES == 1: the lane's 16 values of this tile, all requested before the first is used
        if constexpr (RES == 1) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int c = 32 * j + (e & 3) + 8 * (e >> 2);
                rv[e] = live && col0 + c + 4 * h < a.c_out ? rp[(size_t)c * hw_out] : 0.f;
            }
        }
        int q[16];   // CODES: the lane's channels of this tile through the activation codec with the next layer's scale; past c_out the code 0
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = col0 + 32 * j + (e & 3) + 8 * (e >> 2) + 4 * h;
            q[e] = 0;
            if (co >= a.c_out) continue;
            float v = q8_value(acc[j][e], rs, PC ? q8_rterm(pairs[co - col0].x, rs) : rterm, sx, PC ? pairs[co - col0].y : sw, a.qb != nullptr,
                               [&] { return dequant_int8(a.qb[co], a.bparams[1], a.bparams[0]); }, AFFINE ? 0 : a.relu);
            if constexpr (AFFINE && RES == 0) v = affine_value(v, ab[co - col0].x, ab[co - col0].y, a.relu);
            if constexpr (RES != 0) {
                float r;   // (a pixel past M read nothing: its value is stored nowhere)
                if constexpr (RES == 1) r = rv[e];
                else r = __fmul_rn((float)(int)(int8_t)((rw[e >> 2] >> (8 * (e & 3))) & 0xFF), sr);
                v = affine_residual_value(v, ab[co - col0].x, ab[co - col0].y, r, a.relu);
            }
            if constexpr (CODES) {
                q[e] = act_code(v, sy);
                sum += q[e];
            } else {
                yp[(size_t)(32 * j + (e & 3) + 8 * (e >> 2)) * hw_out] = v;
            }
        }
        if constexpr (CODES) {
            // q[4 g ..] is the word at byte 8 g + 4 h of the tile.  Swapped, the lower half holds {own 0, upper's 0, own 1, upper's 1}
            // = bytes 0 .. 15 and the upper half {lower's 2, own 2, lower's 3, own 3} = bytes 16 .. 31
            const uint4 w = piece_pack(q);
            const auto r02 = __builtin_amdgcn_permlane32_swap(w.x, w.z, false, false);
            const auto r13 = __builtin_amdgcn_permlane32_swap(w.y, w.w, false, false);
            if (live && 32 * j + 16 * h < a.cpitch_y) *(uint4 *)(a.qy + (size_t)m * a.cpitch_y + 16 * h + 32 * j) = make_uint4(r02[0], r02[1], r13[0], r13[1]);
        }
    }
    if constexpr (CODES) {
        for (int off = 32 * NT + 16 * h; off < a.cpitch_y; off += 32)   // a pitch beyond the channel tile: zeros
            if (live) *(uint4 *)(a.qy + (size_t)m * a.cpitch_y + off) = make_uint4(0, 0, 0, 0);
        sum += __shfl_xor(sum, 32, 64);   // the pixel's other half (integers: no order to keep)
        if (a.ypixsum && live && h == 0) a.ypixsum[m] = sum;
    }
}

// every host decision of the product (th_conv2d_q8q8_fwd launches from it, th_debug_qconv_plan reports it)
struct QcPlan {
    int nt, tiles_m, tiles_n, grid;
    QWindow win;
};
// nullptr, or why the shape is refused
static const char *qconv_plan(int n, int c_in, int h, int w, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, QcPlan *p) {
    const int bad = window_check(h, w, k_h, k_w, s_h, s_w, pad_h, pad_w, &p->win);
    if (n < 0 || c_in <= 0 || c_out <= 0 || bad == kWinBelowOne) return "a shape, kernel or stride below 1, or a negative padding";
    if (bad == kWinEmpty) return "an empty output map";
    if (bad == kWinSide) return "a padded map side above 2^31";
    if ((long)c_in * k_h * k_w > kQ8MaxK) return "c_in * k_h * k_w above " TH_Q8_STR(TH_Q8_MAX_K) ", where the int32 sum can overflow";
    const long M = (long)n * p->win.h_out * p->win.w_out;
    if (M > 0x7fffffffL - kQcPix || (long)n * h * w > 0x7fffffffL) return "more than 2^31 pixels";
    p->nt = c_out <= kQcChan ? 1 : c_out <= 2 * kQcChan ? 2 : 4;   // a 128-wide channel tile on a 4- or 32-channel layer is mostly waste
    p->tiles_m = ceil_div(M, kQcPix);
    p->tiles_n = ceil_div(c_out, kQcChan * p->nt);
    if ((long)p->tiles_m * p->tiles_n > 0x7fffffffL) return "more than 2^31 workgroups";
    p->grid = p->tiles_m * p->tiles_n;
    return nullptr;
}

// the kernel of a plan's NT and a call's form: one lookup over (nt, codes, pc, affine), or over (nt, codes, pc, res) for a residual
using QcKernel = void (*)(QcArgs);
template <bool CODES, bool PC, bool AFFINE, int RES = 0>
static QcKernel qconv_kernel_of(int nt) {
    return nt == 1 ? qconv_i8_kernel<1, CODES, PC, AFFINE, RES> : nt == 2 ? qconv_i8_kernel<2, CODES, PC, AFFINE, RES> : qconv_i8_kernel<4, CODES, PC, AFFINE, RES>;
}
static QcKernel qconv_kernel(int nt, bool codes, bool pc, bool affine, int res) {
    if (res) {
        static constexpr QcKernel (*of_res[2][2][2])(int) = {
            {{qconv_kernel_of<false, false, true, 1>, qconv_kernel_of<false, false, true, 2>}, {qconv_kernel_of<false, true, true, 1>, qconv_kernel_of<false, true, true, 2>}},
            {{qconv_kernel_of<true, false, true, 1>, qconv_kernel_of<true, false, true, 2>}, {qconv_kernel_of<true, true, true, 1>, qconv_kernel_of<true, true, true, 2>}}};
        return of_res[codes][pc][res - 1](nt);
    }
    static constexpr QcKernel (*of[2][2][2])(int) = {
        {{qconv_kernel_of<false, false, false>, qconv_kernel_of<false, false, true>}, {qconv_kernel_of<false, true, false>, qconv_kernel_of<false, true, true>}},
        {{qconv_kernel_of<true, false, false>, qconv_kernel_of<true, false, true>}, {qconv_kernel_of<true, true, false>, qconv_kernel_of<true, true, true>}}};
    return of[codes][pc][affine](nt);
}

// ---- the max-pool on codes ----
// G lanes (a power of two, at most 64) share an output pixel and take its 16-byte pieces in turn; a piece's 16 maxima start from -128,
// the code of the float pool's -inf start (maxpool_fwd_kernel), and run over the in-image taps.  Channels c .. cpitch - 1 come out 0.
__global__ __launch_bounds__(256) void maxpool_nhwc_i8_kernel(const int8_t *__restrict__ q, int c, int cpitch, QWindow win, long pixels, int8_t *__restrict__ qy,
                                                              int *__restrict__ ypixsum, int G) {
    const int t = threadIdx.x, gl = t & (G - 1), per_block = 256 / G, cp16 = cpitch >> 4;
    for (long base = (long)blockIdx.x * per_block; base < pixels; base += (long)gridDim.x * per_block) {
        const long o = base + t / G;
        const bool live = o < pixels;
        int sum = 0;
        if (live) {
            const QWindow::Pixel px = win.split((int)o);   // (the host refuses 2^31 pixels)
            const int8_t *xi = q + (size_t)px.img * win.h * win.w * cpitch;
            for (int piece = gl; piece < cp16; piece += G) {
                int best[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) best[i] = -128;
                win.for_taps(px.oh, px.ow, [&](int ih, int iw) {
                    const uint4 v = *(const uint4 *)(xi + ((size_t)ih * win.w + iw) * cpitch + piece * 16);
#pragma unroll
                    for (int i = 0; i < 16; ++i) best[i] = max(best[i], piece_code(v, i));
                });
                const uint4 out = piece_pack(best, c - piece * 16);
                sum += piece_sum(out);
                *(uint4 *)(qy + (size_t)o * cpitch + piece * 16) = out;
            }
        }
        for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);   // the pixel's lanes (integers: no order to keep)
        if (live && gl == 0) ypixsum[o] = sum;
    }
}

}  // namespace th

using namespace th;

extern "C" {

int th_qconv_i8_cpitch(int c_in) { return c_in > 0 ? (c_in + 15) / 16 * 16 : 0; }

int th_quantize_act_nhwc_int8(th_ctx *ctx, const float *d_x, int n, int c, int h, int w, const float *d_scale, int8_t *d_q, int cpitch, int *d_pixsum) {
    TH_REQUIRE(ctx && d_x && d_scale && d_q && d_pixsum, "th_quantize_act_nhwc_int8: null argument");
    TH_REQUIRE(n >= 0 && c > 0 && h > 0 && w > 0 && cpitch >= c && cpitch % 16 == 0 && (long)h * w <= 0x7fffffffL && (long)n * h * w <= 0x7fffffffL,
               "th_quantize_act_nhwc_int8: bad shape n=%d c=%d h=%d w=%d cpitch=%d (cpitch >= c, a multiple of 16)", n, c, h, w, cpitch);
    TH_REQUIRE(((uintptr_t)d_q & 15) == 0, "th_quantize_act_nhwc_int8: the code pointer must be 16-byte aligned");
    if (n == 0) return 0;
    const int hw = h * w, tiles_per_img = ceil_div(hw, kQcTurnPix);
    const long tiles = (long)n * tiles_per_img;
    hipLaunchKernelGGL(quantize_act_nhwc_kernel, dim3((unsigned)std::min(tiles, (long)kNumCU * 32)), dim3(256), 0, ctx->stream, d_x, n, c, hw, d_scale, d_q,
                       cpitch, d_pixsum, tiles_per_img);
    TH_LAUNCH_CHECK();
    return 0;
}

static int pack_conv_weight(const char *fn, bool taper, th_ctx *ctx, const int8_t *d_src, int c_out, int c_in, int k_h, int k_w, int8_t *d_dst, int cpitch) {
    TH_REQUIRE(ctx && d_src && d_dst, "%s: null argument", fn);
    TH_REQUIRE(c_out >= 0 && c_in > 0 && k_h > 0 && k_w > 0 && cpitch >= c_in && cpitch % 16 == 0 && (long)k_h * k_w <= 0x7fffffffL && ((uintptr_t)d_dst & 15) == 0,
               "%s: bad shape c_out=%d c_in=%d k=%dx%d cpitch=%d (cpitch >= c_in, a multiple of 16) or a destination off a 16-byte boundary", fn, c_out, c_in,
               k_h, k_w, cpitch);
    if (c_out == 0) return 0;
    const dim3 grid(ew_grid((size_t)c_out * k_h * k_w * (cpitch / 16), 256));
    hipLaunchKernelGGL(taper ? pack_conv_weight_kernel<true> : pack_conv_weight_kernel<false>, grid, dim3(256), 0, ctx->stream, d_src, (long)c_out, c_in, k_h * k_w,
                       d_dst, cpitch);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_pack_conv_weight_int8(th_ctx *ctx, const int8_t *d_src, int c_out, int c_in, int k_h, int k_w, int8_t *d_dst, int cpitch) {
    return pack_conv_weight("th_pack_conv_weight_int8", false, ctx, d_src, c_out, c_in, k_h, k_w, d_dst, cpitch);
}

int th_pack_conv_weight_taper_int8(th_ctx *ctx, const int8_t *d_src, int c_out, int c_in, int k_h, int k_w, int8_t *d_dst, int cpitch) {
    return pack_conv_weight("th_pack_conv_weight_taper_int8", true, ctx, d_src, c_out, c_in, k_h, k_w, d_dst, cpitch);
}

// One call of a product, as its entry point fills it: fn = the entry point's name for the messages; codes, pc, affine = its form (pc:
// d_wparams holds a pair per output channel; affine: d_affine holds {a, b} per output channel); then the arguments in the prototypes'
// order -- the 21 that every entry point takes (QC_SHARED), the f32 form's output, the codes form's four, d_affine, and with
// `residual` the skip connection's four (exactly one of d_res, d_res_q).  What a form does not take stays null / 0 and is not read.
struct QcCall {
    const char *fn;
    bool codes, pc, affine;
    th_ctx *ctx;
    const int8_t *d_qx;
    int cpitch;
    const int *d_pixsum;
    const float *d_xscale;
    int n, c_in, h, w;
    const int8_t *d_qw;
    int c_out, k_h, k_w, s_h, s_w, pad_h, pad_w;
    const float *d_wparams;
    const int8_t *d_qb;
    const float *d_bparams;
    int relu;
    float *d_y = nullptr;
    const float *d_yscale = nullptr;
    int8_t *d_qy = nullptr;
    int cpitch_y = 0;
    int *d_ypixsum = nullptr;
    const float *d_affine = nullptr;
    bool residual = false;
    const float *d_res = nullptr;
    const int8_t *d_res_q = nullptr;
    int cpitch_r = 0;
    const float *d_res_scale = nullptr;
};
#define QC_SHARED ctx, d_qx, cpitch, d_pixsum, d_xscale, n, c_in, h, w, d_qw, c_out, k_h, k_w, s_h, s_w, pad_h, pad_w, d_wparams, d_qb, d_bparams, relu

// both products: their checks, then the launch
static int qconv_run(const QcCall &c) {
    TH_REQUIRE(c.ctx && c.d_qx && c.d_pixsum && c.d_xscale && c.d_qw && c.d_wparams && (c.codes ? c.d_yscale && c.d_qy : c.d_y != nullptr) &&
                   (!c.d_qb || c.d_bparams) && (!c.affine || c.d_affine),
               "%s: null argument", c.fn);
    QcPlan p{};
    const char *why = qconv_plan(c.n, c.c_in, c.h, c.w, c.c_out, c.k_h, c.k_w, c.s_h, c.s_w, c.pad_h, c.pad_w, &p);
    TH_REQUIRE(!why, "%s: %s (n=%d c_in=%d %dx%d, c_out=%d k=%dx%d stride %dx%d pad %dx%d)", c.fn, why, c.n, c.c_in, c.h, c.w, c.c_out, c.k_h, c.k_w, c.s_h, c.s_w,
               c.pad_h, c.pad_w);
    TH_REQUIRE((((uintptr_t)c.d_qx | (uintptr_t)c.d_qw) & 15) == 0, "%s: the code pointers must be 16-byte aligned", c.fn);
    TH_REQUIRE(c.cpitch % 16 == 0 && c.cpitch >= c.c_in, "%s: cpitch %d must be a multiple of 16 and at least c_in %d", c.fn, c.cpitch, c.c_in);
    if (c.codes) {
        TH_REQUIRE(p.tiles_n == 1, "%s: c_out %d is above %d, the channels one workgroup covers (a wider layer writes f32: th_conv2d_q8q8_fwd%s)", c.fn, c.c_out,
                   th_qconv_i8_chain_max_cout(), c.affine ? "_affine" : c.pc ? "_pc" : "");
        TH_REQUIRE(((uintptr_t)c.d_qy & 15) == 0, "%s: the output code pointer must be 16-byte aligned", c.fn);
        TH_REQUIRE(c.cpitch_y % 16 == 0 && c.cpitch_y >= c.c_out, "%s: cpitch_y %d must be a multiple of 16 and at least c_out %d", c.fn, c.cpitch_y, c.c_out);
    }
    if (c.residual) {
        TH_REQUIRE((c.d_res != nullptr) != (c.d_res_q != nullptr), "%s: exactly one of d_res (an f32 residual) and d_res_q (a residual in codes) must be set", c.fn);
        if (c.d_res_q) {
            TH_REQUIRE(c.d_res_scale, "%s: null d_res_scale with a residual in codes", c.fn);
            TH_REQUIRE(c.cpitch_r % 16 == 0 && c.cpitch_r >= c.c_out, "%s: cpitch_r %d must be a multiple of 16 and at least c_out %d", c.fn, c.cpitch_r, c.c_out);
            TH_REQUIRE(((uintptr_t)c.d_res_q & 15) == 0, "%s: the residual code pointer must be 16-byte aligned", c.fn);
        }
    }
    const int res = !c.residual ? 0 : c.d_res ? 1 : 2;
    if (c.n == 0) return 0;
    const QcArgs a{c.d_qx, c.d_qw, c.d_pixsum, c.d_xscale, c.d_wparams, c.d_qb, c.d_bparams, c.d_y, c.d_yscale, c.d_qy, c.d_ypixsum, c.cpitch_y, p.win, c.cpitch, c.c_out,
                   c.n * p.win.h_out * p.win.w_out, c.relu, p.tiles_n, c.affine ? c.d_affine : nullptr, res == 1 ? c.d_res : nullptr, res == 2 ? c.d_res_q : nullptr, res == 2 ? c.d_res_scale : nullptr,
                   res == 2 ? c.cpitch_r : 0};
    hipLaunchKernelGGL(qconv_kernel(p.nt, c.codes, c.pc, c.affine, res), dim3(p.grid), dim3(256), 0, c.ctx->stream, a);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_conv2d_q8q8_fwd(th_ctx *ctx, const int8_t *d_qx, int cpitch, const int *d_pixsum, const float *d_xscale, int n, int c_in, int h, int w,
                       const int8_t *d_qw, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, const float *d_wparams, const int8_t *d_qb,
                       const float *d_bparams, int relu, float *d_y) {
    return qconv_run({"th_conv2d_q8q8_fwd", false, false, false, QC_SHARED, d_y});
}

int th_qconv_i8_chain_max_cout(void) { return kQcChan * 4; }

int th_conv2d_q8q8_fwd_codes(th_ctx *ctx, const int8_t *d_qx, int cpitch, const int *d_pixsum, const float *d_xscale, int n, int c_in, int h, int w,
                             const int8_t *d_qw, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, const float *d_wparams,
                             const int8_t *d_qb, const float *d_bparams, int relu, const float *d_yscale, int8_t *d_qy, int cpitch_y, int *d_ypixsum) {
    return qconv_run({"th_conv2d_q8q8_fwd_codes", true, false, false, QC_SHARED, nullptr, d_yscale, d_qy, cpitch_y, d_ypixsum});
}

int th_conv2d_q8q8_fwd_pc(th_ctx *ctx, const int8_t *d_qx, int cpitch, const int *d_pixsum, const float *d_xscale, int n, int c_in, int h, int w,
                          const int8_t *d_qw, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, const float *d_wparams, const int8_t *d_qb,
                          const float *d_bparams, int relu, float *d_y) {
    return qconv_run({"th_conv2d_q8q8_fwd_pc", false, true, false, QC_SHARED, d_y});
}

int th_conv2d_q8q8_fwd_codes_pc(th_ctx *ctx, const int8_t *d_qx, int cpitch, const int *d_pixsum, const float *d_xscale, int n, int c_in, int h, int w,
                                const int8_t *d_qw, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, const float *d_wparams,
                                const int8_t *d_qb, const float *d_bparams, int relu, const float *d_yscale, int8_t *d_qy, int cpitch_y, int *d_ypixsum) {
    return qconv_run({"th_conv2d_q8q8_fwd_codes_pc", true, true, false, QC_SHARED, nullptr, d_yscale, d_qy, cpitch_y, d_ypixsum});
}

int th_conv2d_q8q8_fwd_affine(th_ctx *ctx, const int8_t *d_qx, int cpitch, const int *d_pixsum, const float *d_xscale, int n, int c_in, int h, int w,
                              const int8_t *d_qw, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, const float *d_wparams, const int8_t *d_qb,
                              const float *d_bparams, int relu, float *d_y, int per_channel, const float *d_affine) {
    return qconv_run({"th_conv2d_q8q8_fwd_affine", false, per_channel != 0, true, QC_SHARED, d_y, nullptr, nullptr, 0, nullptr, d_affine});
}

int th_conv2d_q8q8_fwd_codes_affine(th_ctx *ctx, const int8_t *d_qx, int cpitch, const int *d_pixsum, const float *d_xscale, int n, int c_in, int h, int w,
                                    const int8_t *d_qw, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, const float *d_wparams,
                                    const int8_t *d_qb, const float *d_bparams, int relu, const float *d_yscale, int8_t *d_qy, int cpitch_y, int *d_ypixsum,
                                    int per_channel, const float *d_affine) {
    return qconv_run({"th_conv2d_q8q8_fwd_codes_affine", true, per_channel != 0, true, QC_SHARED, nullptr, d_yscale, d_qy, cpitch_y, d_ypixsum, d_affine});
}

int th_conv2d_q8q8_fwd_residual(th_ctx *ctx, const int8_t *d_qx, int cpitch, const int *d_pixsum, const float *d_xscale, int n, int c_in, int h, int w,
                                const int8_t *d_qw, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, const float *d_wparams, const int8_t *d_qb,
                                const float *d_bparams, int relu, float *d_y, int per_channel, const float *d_affine, const float *d_res, const int8_t *d_res_q,
                                int cpitch_r, const float *d_res_scale) {
    return qconv_run({"th_conv2d_q8q8_fwd_residual", false, per_channel != 0, true, QC_SHARED, d_y, nullptr, nullptr, 0, nullptr, d_affine, true, d_res, d_res_q,
                      cpitch_r, d_res_scale});
}

int th_conv2d_q8q8_fwd_codes_residual(th_ctx *ctx, const int8_t *d_qx, int cpitch, const int *d_pixsum, const float *d_xscale, int n, int c_in, int h, int w,
                                      const int8_t *d_qw, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, const float *d_wparams,
                                      const int8_t *d_qb, const float *d_bparams, int relu, const float *d_yscale, int8_t *d_qy, int cpitch_y, int *d_ypixsum,
                                      int per_channel, const float *d_affine, const float *d_res, const int8_t *d_res_q, int cpitch_r, const float *d_res_scale) {
    return qconv_run({"th_conv2d_q8q8_fwd_codes_residual", true, per_channel != 0, true, QC_SHARED, nullptr, d_yscale, d_qy, cpitch_y, d_ypixsum, d_affine, true,
                      d_res, d_res_q, cpitch_r, d_res_scale});
}
#undef QC_SHARED

int th_maxpool2d_nhwc_int8(th_ctx *ctx, const int8_t *d_q, int n, int c, int h, int w, int cpitch, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w,
                           int8_t *d_qy, int *d_ypixsum) {
    TH_REQUIRE(ctx && d_q && d_qy && d_ypixsum, "th_maxpool2d_nhwc_int8: null argument");
    TH_REQUIRE((((uintptr_t)d_q | (uintptr_t)d_qy) & 15) == 0, "th_maxpool2d_nhwc_int8: the code pointers must be 16-byte aligned");
    QWindow win{};
    const int bad = window_check(h, w, k_h, k_w, s_h, s_w, pad_h, pad_w, &win);
    TH_REQUIRE(n >= 0 && c > 0 && bad != kWinBelowOne,
               "th_maxpool2d_nhwc_int8: a shape, window or stride below 1, or a negative padding (n=%d c=%d %dx%d, k=%dx%d stride %dx%d pad %dx%d)", n, c, h, w,
               k_h, k_w, s_h, s_w, pad_h, pad_w);
    TH_REQUIRE(cpitch % 16 == 0 && cpitch >= c, "th_maxpool2d_nhwc_int8: cpitch %d must be a multiple of 16 and at least c %d", cpitch, c);
    TH_REQUIRE(bad == kWinOk, "th_maxpool2d_nhwc_int8: an empty output map (%dx%d, k=%dx%d pad %dx%d)", h, w, k_h, k_w, pad_h, pad_w);
    const long pixels = (long)n * win.h_out * win.w_out;
    TH_REQUIRE(pixels <= 0x7fffffffL && (long)n * h * w <= 0x7fffffffL, "th_maxpool2d_nhwc_int8: more than 2^31 pixels");
    if (n == 0) return 0;
    int G = 1;   // lanes per pixel: the pieces of a pixel row rounded up to a power of two, a wave at the most
    while (G < cpitch / 16 && G < kWave) G *= 2;
    const long blocks = (pixels + 256 / G - 1) / (256 / G);
    hipLaunchKernelGGL(maxpool_nhwc_i8_kernel, dim3((unsigned)std::min(blocks, (long)kNumCU * 32)), dim3(256), 0, ctx->stream, d_q, c, cpitch, win, pixels, d_qy,
                       d_ypixsum, G);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_debug_qconv_plan(int n, int c_in, int h, int w, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, int *out8) {
    TH_REQUIRE(out8 && n >= 1, "th_debug_qconv_plan: null argument or n=%d below 1", n);
    QcPlan p{};
    const char *why = qconv_plan(n, c_in, h, w, c_out, k_h, k_w, s_h, s_w, pad_h, pad_w, &p);
    TH_REQUIRE(!why, "th_debug_qconv_plan: %s (n=%d c_in=%d %dx%d, c_out=%d k=%dx%d stride %dx%d pad %dx%d)", why, n, c_in, h, w, c_out, k_h, k_w, s_h, s_w,
               pad_h, pad_w);
    const int out[8] = {p.nt, kQcPix, kQcChan * p.nt, p.tiles_m, p.tiles_n, p.grid, p.win.h_out, p.win.w_out};
    std::copy(out, out + 8, out8);
    return 0;
}

}  // extern "C"
