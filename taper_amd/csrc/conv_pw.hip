// conv_pw.hip -- the exact pointwise (1x1) convolution with stride (1, 1) or (2, 2), padding 0, forward and both gradients, on the fp32
// matrix cores (th_conv1x1_exact_fwd / _bwd_input / _bwd_weight; full_backward extension of the host: the reference's 1x1 path is quirk Q4,
// th_conv1x1_fwd, which is no convolution for c_in > 1 and has no stride and no gradient).  v_mfma_f32_16x16x4_f32 is exact fp32 (a
// k-ordered fmaf chain), so the parity bar is the 3x3 layers'.
//
// A pointwise convolution is one matrix product per image, and all three kernels are DIRECT in the design of conv_s2.hip (operand layouts:
// conv_mfma.hip's header comment): no repacked copy of x or gy exists anywhere.  h_out = (h - 1) / s + 1; output pixel (oh, ow) reads input
// pixel (s oh, s ow).  The output pixels of the whole batch form ONE flat axis g = (image, oh, ow) of n h_out w_out pixels.
//
//   forward          D[co][g] = sum_ci W[co][ci] x[image(g)][ci][s oh, s ow].  A workgroup owns 128 consecutive pixels of the flat axis (a
//                    tile runs over image boundaries: no ragged tile but the last) and 16 CT output channels; it contracts over c_in in
//                    passes of 16 channels.  The B operand needs no staging: lane (l16, g4) of a k-step loads x[ci = 4 s + g4][pixel l16] of
//                    its wave's two adjacent pixel tiles straight into the operand register -- at stride 1 sixteen lanes read 64 contiguous
//                    bytes, at stride 2 the stride lives in the lane's pixel offset alone and the skipped rows and columns are never loaded.
//                    The weights of a pass [16][16 CT] go through LDS.  A pass's loads are issued before the previous pass's MFMAs.
//   input gradient   gx[image][ci][s oh, s ow] = sum_co W[co][ci] gy[image][co][oh, ow]: the SAME kernel with the roles swapped (gy is the
//                    unit-stride source, c_out the contraction, the weight matrix read transposed, the stride in the store).  At stride 2
//                    the lane of output pixel (oh, ow) owns the input quad (2 oh .. 2 oh + 1, 2 ow .. 2 ow + 1): without accumulate it
//                    writes +0.0 to the quad's three pixels no output reads, with accumulate it leaves them alone.
//   weight gradient  gw[co][ci] = sum_g gy[g][co] x[g][ci]: a workgroup owns a slab of 32 input channels x 16 CT output channels and walks
//                    every G-th 128-pixel block of the flat axis; both operands are staged [channel][pixel] in LDS (pitch 2 mod 32) and read
//                    transposed.  It writes ONE partial [c_in][co_ld] slab; wgrad_reduce (conv_mfma.hip) adds the slabs in order.
//
// No float atomics: every result is the same bits from run to run.  What lies outside (pixels past the batch, channel passes past the
// contraction, channel tiles past the output) is read as 0 through a buffer descriptor's range, SELECTED to zero or not stored -- never
// read and multiplied by zero.
#include <algorithm>

#include "common.h"
#include "conv_plan.h"
#include "conv_pw_plan.h"

namespace th {

int wgrad_reduce(th_ctx *ctx, const float *part, float *gw, int G, int kt, int c_out, int co_ld, int layout, int accumulate);   // conv_mfma.hip

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int PW_PX = 128;                // pixels per workgroup tile / pixel block: 8 tiles of 16, two adjacent ones per wave
constexpr int PW_CI = 16;                 // channels of the contraction per pass: 4 k-steps
constexpr int PW_KS = PW_CI / 4;
constexpr int PW_OOB = 0x7ffffff0;        // a byte offset beyond every buffer descriptor's range: the load returns 0
constexpr int PW_WG_CI = 32;              // weight gradient: input channels per slab (two row tiles)
constexpr int PW_WG_RT = PW_WG_CI / 16;
constexpr int PW_WG_PITCH = PW_PX + 2;    // pitch of a staged channel, 2 (mod 32): 16 channels x 4 pixels read 32 distinct banks twice

// forward and input gradient: D[m][g] = sum_k Wm[m][k] src[image][k][pixel], m the output channel of the launch, k its contraction channel
struct ConvPwArgs {
    const float *src, *w, *bias;
    float *dst;
    int n, k_ch, m_ch;            // forward: c_in, c_out; input gradient: c_out, c_in
    int src_chan, src_w, s_src;   // floats of a source plane, its row width, the pixel stride in it (forward: s; input gradient: 1)
    int dst_h, dst_w, s_dst;      // the destination plane and the pixel stride in it (forward: 1; input gradient: s)
    int w_out, P, total;          // output grid: row width, pixels per image, pixels of the batch
    int w_sm, w_sk;               // element (m, k) of the weight matrix lies at m w_sm + k w_sk of the buffer
    int span;                     // images a tile can touch
    int relu, accumulate;
};

template <int CT, bool BWD>
__global__ __launch_bounds__(256, CT <= 2 ? 2 : 1) void conv_pw_kernel(ConvPwArgs a) {
    constexpr int M_B = 16 * CT, WP = M_B + 8, WN = PW_CI * M_B, WPT = WN / 256;   // (WP: the four k rows of a step fall 8 banks apart)
    __shared__ float wsl[PW_CI * WP];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l16 = lane & 15, g4 = lane >> 4;
    const int g0 = blockIdx.x * PW_PX, m0 = blockIdx.y * M_B;
    const int img0 = g0 / a.P, imgs_here = min(a.span, a.n - img0);

    // this lane's B column in its wave's two pixel tiles: byte offset of channel g4 of the pixel within this tile's images, or one past the
    // descriptor's range (a pixel past the batch), which reads as 0 without touching memory
    int src_off[2], px_img[2], px_op[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int g = g0 + (2 * wave + q) * 16 + l16;
        const bool ok = g < a.total;
        const int gc = ok ? g : g0, img = gc / a.P, op = gc % a.P, oh = op / a.w_out, ow = op % a.w_out;
        px_img[q] = ok ? img : -1;
        px_op[q] = BWD ? a.s_dst * (oh * a.dst_w + ow) : op;
        src_off[q] = ok ? (((img - img0) * a.k_ch + g4) * a.src_chan + a.s_src * (oh * a.src_w + ow)) * 4 : PW_OOB;
    }
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)(a.src + (long)img0 * a.k_ch * a.src_chan), 0, imgs_here * a.k_ch * a.src_chan * 4, 0x00020000);

    floatx4 acc[2][CT];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[q][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    float xn[PW_KS][2], xc[PW_KS][2], wv[WPT];
    // the global loads of a pass are issued back to back and parked in registers while the previous pass computes
    auto load = [&](int cb) {
#pragma unroll
        for (int s = 0; s < PW_KS; ++s) {
            const bool ch_ok = cb + 4 * s + g4 < a.k_ch;         // a channel past the contraction reads zeros
            const int so = (cb + 4 * s) * a.src_chan * 4;
#pragma unroll
            for (int q = 0; q < 2; ++q)
                xn[s][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, ch_ok ? src_off[q] : PW_OOB, ch_ok ? so : 0, 0));
        }
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int u = t + 256 * j, m = m0 + u % M_B, k = cb + u / M_B;
            const bool ok = k < a.k_ch && m < a.m_ch;
            const float v = a.w[ok ? (long)m * a.w_sm + (long)k * a.w_sk : 0];
            wv[j] = ok ? v : 0.f;
        }
    };
    load(0);
    for (int cb = 0; cb < a.k_ch; cb += PW_CI) {
#pragma unroll
        for (int s = 0; s < PW_KS; ++s) { xc[s][0] = xn[s][0]; xc[s][1] = xn[s][1]; }
        __syncthreads();   // every wave is done reading the previous pass's weights
#pragma unroll
        for (int j = 0; j < WPT; ++j) wsl[((t + 256 * j) / M_B) * WP + (t + 256 * j) % M_B] = wv[j];
        __syncthreads();
        if (cb + PW_CI < a.k_ch) load(cb + PW_CI);
#pragma unroll
        for (int s = 0; s < PW_KS; ++s) {
            const float *wk = wsl + (4 * s + g4) * WP + l16;
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                const float av = wk[16 * j];
                acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc[s][0], acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc[s][1], acc[1][j], 0, 0, 0);
            }
        }
    }
    // ---- epilogue: NCHW store straight from the D tiles (lane (l16, g4) holds pixel l16 of its tile, channels m0 + 16 j + 4 g4 + i)
    const long dchan = (long)a.dst_h * a.dst_w;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (px_img[q] < 0) continue;
        float *dpx = a.dst + (long)px_img[q] * a.m_ch * dchan + px_op[q];
        // input gradient at stride 2: the three pixels of this lane's quad no output reads (those inside the plane)
        bool right = false, below = false;
        if (BWD && a.s_dst == 2 && !a.accumulate) {
            const int ih = px_op[q] / a.dst_w, iw = px_op[q] % a.dst_w;
            right = iw + 1 < a.dst_w;
            below = ih + 1 < a.dst_h;
        }
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + 16 * j + 4 * g4 + i;
                if (m >= a.m_ch) continue;
                float *d = dpx + (long)m * dchan;
                float v = acc[q][j][i];
                if (BWD) {
                    *d = a.accumulate ? *d + v : v;
                    if (right) d[1] = 0.f;
                    if (below) d[a.dst_w] = 0.f;
                    if (right && below) d[a.dst_w + 1] = 0.f;
                } else {
                    v += a.bias ? a.bias[m] : 0.f;
                    if (a.relu) v = v > 0.f ? v : 0.f;
                    *d = v;
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
//   A operand (16 ci x 4 px): lane l -> xs[rt 16 + (l&15)][4 step + (l>>4)]
//   B operand (4 px x 16 co): lane l -> gs[ct 16 + (l&15)][4 step + (l>>4)]
struct ConvPwWgradArgs {
    const float *x, *gy;
    float *part;           // [G][c_in][co_ld]
    int n, c_in, c_out, chan, w_in, stride, w_out, P, total;
    int n_pb, G, co_ld;
    unsigned x_bytes, gy_bytes;   // extents of x / gy: the ranges of the kernel's buffer descriptors
};

template <int CT>
__global__ __launch_bounds__(256, 2) void conv_pw_wgrad_kernel(ConvPwWgradArgs a) {
    constexpr int CO_B = 16 * CT, NPAIR = PW_WG_RT * CT, SLOTS = (NPAIR + 3) / 4, PITCH = PW_WG_PITCH;
    __shared__ float xs[PW_WG_CI * PITCH];
    __shared__ float gs[CO_B * PITCH];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l16 = lane & 15, g4 = lane >> 4;
    const int cb = blockIdx.y * PW_WG_CI, co0 = blockIdx.z * CO_B;
    const int gp = t & (PW_PX - 1), gpar = t >> 7;   // staging: pixel t % 128 of the block, channel parity t / 128

    // the (row tile, channel tile) pairs of this wave: pair p = ct PW_WG_RT + rt
    int a_off[SLOTS], b_off[SLOTS];
    bool slot_ok[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const int p = wave * SLOTS + j;
        slot_ok[j] = p < NPAIR;
        const int pc = slot_ok[j] ? p : 0;
        a_off[j] = ((pc % PW_WG_RT) * 16 + l16) * PITCH + g4;
        b_off[j] = ((pc / PW_WG_RT) * 16 + l16) * PITCH + g4;
    }
    floatx4 acc[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};

    // blocks are software-pipelined through registers: block pb + G is REQUESTED (buffer loads; a pixel past the batch or a channel past
    // the range gets an offset past the buffer and reads as 0 without touching memory) before block pb's steps, stored after
    const auto rx = __builtin_amdgcn_make_buffer_rsrc((void *)a.x, 0, a.x_bytes, 0x00020000);
    const auto rg = __builtin_amdgcn_make_buffer_rsrc((void *)a.gy, 0, a.gy_bytes, 0x00020000);
    float vx[PW_WG_CI / 2], vg[CO_B / 2];
    auto request = [&](int pb) {
        const int g = pb * PW_PX + gp;
        const bool ok = g < a.total;
        const int gc = ok ? g : 0, img = gc / a.P, op = gc % a.P, oh = op / a.w_out, ow = op % a.w_out;
        const int xo = ok ? ((img * a.c_in + cb + gpar) * a.chan + a.stride * (oh * a.w_in + ow)) * 4 : PW_OOB;
        const int go = ok ? ((img * a.c_out + co0 + gpar) * a.P + op) * 4 : PW_OOB;
#pragma unroll
        for (int i = 0; i < PW_WG_CI / 2; ++i)
            vx[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, (cb + 2 * i + gpar < a.c_in) ? xo : PW_OOB, 2 * i * a.chan * 4, 0));
#pragma unroll
        for (int i = 0; i < CO_B / 2; ++i)
            vg[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, (co0 + 2 * i + gpar < a.c_out) ? go : PW_OOB, 2 * i * a.P * 4, 0));
    };
    if ((int)blockIdx.x < a.n_pb) request(blockIdx.x);
    for (int pb = blockIdx.x; pb < a.n_pb; pb += a.G) {
        __syncthreads();   // the previous block's MFMAs are done with xs / gs
#pragma unroll
        for (int i = 0; i < PW_WG_CI / 2; ++i) xs[(2 * i + gpar) * PITCH + gp] = vx[i];
#pragma unroll
        for (int i = 0; i < CO_B / 2; ++i) gs[(2 * i + gpar) * PITCH + gp] = vg[i];
        __syncthreads();
        if (pb + a.G < a.n_pb) request(pb + a.G);
        // reduction steps of 4 pixels, up to the block's last pixel (the pixels of a ragged last step were read as zeros on both sides)
        const int n_steps = (min(PW_PX, a.total - pb * PW_PX) + 3) / 4;
        for (int rs = 0; rs < n_steps; ++rs) {
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const float av = xs[a_off[j] + 4 * rs], bv = gs[b_off[j] + 4 * rs];
                if (slot_ok[j]) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
            }
        }
    }
    // one partial slab per workgroup: part[g][ci][co]  (D tile: row = channel 4 g4 + i of the row tile, column = co l16)
    float *pp = a.part + (long)blockIdx.x * a.c_in * a.co_ld;
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const int p = wave * SLOTS + j;
        if (p >= NPAIR) continue;
        const int co = co0 + (p / PW_WG_RT) * 16 + l16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ch = cb + (p % PW_WG_RT) * 16 + 4 * g4 + i;
            if (ch < a.c_in && co < a.co_ld) pp[(long)ch * a.co_ld + co] = acc[j][i];
        }
    }
}

// ------------------------------------------------------------------------------------------------ plans (host data, no device call)
// 16-channel tiles per workgroup: up to 64 channels, halved when the launch has fewer than 1.5 workgroups per CU (conv3x3_mfma_plan's rule)
static int pw_ct(int channels, long tiles) {
    const int c_tiles = ceil_div(channels, 16);
    int ct = c_tiles >= 4 ? 4 : (c_tiles >= 2 ? 2 : 1);
    if (ct == 4 && tiles * ceil_div(channels, 64) < 384) ct = 2;
    return ct;
}

// forward / input gradient: the flat pixel axis in tiles of 128; `src_img_floats`: one image of the operand behind the buffer descriptor,
// `channels`: the output channels of the launch
static void pw_tile_plan(ConvPwPlan *p, int n, int h, int w, int stride, long src_img_floats, int channels) {
    p->stride = stride;
    p->h_out = (h - 1) / stride + 1; p->w_out = (w - 1) / stride + 1;
    p->px_t = PW_PX;
    const long P = (long)p->h_out * p->w_out, total = (long)n * P, tiles = (total + PW_PX - 1) / PW_PX;
    // 128 consecutive pixels that begin anywhere in an image end at most floor((P + 126) / P) images further on
    p->span = (int)std::min<long>(n, (P + PW_PX - 2) / P + 1);
    p->ct = pw_ct(channels, tiles);
    p->grid_x = p->grid_y = p->grid_z = 1;
    p->lds = PW_CI * (16 * p->ct + 8) * (int)sizeof(float);
    p->lds_limit = 64 << 10;
    if (total > 0x7fffff00L || ceil_div(channels, 16 * p->ct) > 65535) { p->refused = CONV_PW_REFUSED_GRID; p->tiles = 1; return; }
    p->tiles = (int)tiles;
    p->grid_x = p->tiles; p->grid_y = ceil_div(channels, 16 * p->ct);
    if ((long)p->span * src_img_floats >= (1L << 29)) p->refused = CONV_PW_REFUSED_2GIB;
}

void conv_pw_fwd_plan(ConvPwPlan *p, int n, int c_in, int h, int w, int c_out, int stride) {
    *p = ConvPwPlan{};
    p->op = 0;
    pw_tile_plan(p, n, h, w, stride, (long)c_in * h * w, c_out);
}

void conv_pw_bwd_input_plan(ConvPwPlan *p, int n, int c_in, int h, int w, int c_out, int stride, bool accumulate) {
    *p = ConvPwPlan{};
    p->op = 1; p->acc = accumulate;
    pw_tile_plan(p, n, h, w, stride, (long)c_out * ((h - 1) / stride + 1) * ((w - 1) / stride + 1), c_in);
}

void conv_pw_bwd_weight_plan(ConvPwPlan *p, int n, int c_in, int h, int w, int c_out, int stride, int layout, bool accumulate, bool gw_aligned) {
    *p = ConvPwPlan{};
    p->op = 2; p->acc = accumulate; p->stride = stride;
    p->h_out = (h - 1) / stride + 1; p->w_out = (w - 1) / stride + 1;
    p->px_t = PW_PX; p->ci_slab = PW_WG_CI;
    const long total = (long)n * p->h_out * p->w_out, n_pb = (total + PW_PX - 1) / PW_PX;
    const int c_tiles = ceil_div(c_out, 16);
    p->ct = c_tiles >= 4 ? 4 : (c_tiles >= 2 ? 2 : 1);
    const int co_b = 16 * p->ct, slabs = ceil_div(c_in, PW_WG_CI), co_blocks = ceil_div(c_out, co_b);
    p->co_ld = co_blocks * co_b;
    p->lds = (PW_WG_CI + co_b) * PW_WG_PITCH * (int)sizeof(float);
    p->lds_limit = 64 << 10;
    p->grid_x = p->grid_y = p->grid_z = 1;
    const size_t xb = (size_t)n * c_in * h * w * 4, gb = (size_t)total * c_out * 4;
    const bool grid_bad = total > 0x7fffff00L || slabs > 65535 || co_blocks > 65535;
    if (grid_bad || xb >= (1u << 31) || gb >= (1u << 31)) {
        p->refused = grid_bad ? CONV_PW_REFUSED_GRID : CONV_PW_REFUSED_2GIB;
        p->tiles = 1;
        return;
    }
    p->tiles = (int)n_pb;
    int G = ceil_div(2 * kNumCU, (long)slabs * co_blocks);      // two workgroups per CU in total
    G = std::max(1, std::min(G, std::min(p->tiles, 512)));
    p->G = G; p->slabs = G;
    p->grid_x = G; p->grid_y = slabs; p->grid_z = co_blocks;
    p->reduce = wgrad_reduce_plan(G, c_in, c_out, p->co_ld, layout, accumulate, gw_aligned);
}

// what this thread's most recent pointwise launch ran (th_debug_last_conv_pw_config)
thread_local int t_last_pw_cfg[9] = {-1, 0, 0, 0, 0, 0, 0, 0, 0};
static void pw_note(const ConvPwPlan &p) {
    const int v[9] = {p.op, p.ct, p.acc, p.stride, p.grid_x, p.grid_y, p.grid_z, p.lds, p.reduce};
    for (int i = 0; i < 9; ++i) t_last_pw_cfg[i] = v[i];
}

template <bool BWD>
static void pw_launch(th_ctx *ctx, const ConvPwPlan &p, const ConvPwArgs &a) {
    const dim3 grid(p.grid_x, p.grid_y);
    switch (p.ct) {
        case 4: hipLaunchKernelGGL((conv_pw_kernel<4, BWD>), grid, dim3(256), 0, ctx->stream, a); break;
        case 2: hipLaunchKernelGGL((conv_pw_kernel<2, BWD>), grid, dim3(256), 0, ctx->stream, a); break;
        default: hipLaunchKernelGGL((conv_pw_kernel<1, BWD>), grid, dim3(256), 0, ctx->stream, a); break;
    }
}

}  // namespace th

using namespace th;

#define TH_PW_CHECK(NAME, P0, P1, P2)                                                                                                    \
    TH_REQUIRE(ctx && (P0) && (P1) && (P2), NAME ": null argument");                                                                     \
    TH_REQUIRE(n >= 1 && c_in >= 1 && h >= 1 && w >= 1 && c_out >= 1, NAME ": bad geometry n=%d c_in=%d h=%d w=%d c_out=%d (all must be >= 1)", \
               n, c_in, h, w, c_out);                                                                                                    \
    TH_REQUIRE(stride == 1 || stride == 2, NAME ": stride must be 1 or 2, got %d", stride);                                              \
    TH_REQUIRE(weight_layout == 0 || weight_layout == 1, NAME ": weight_layout must be 0 (taper) or 1 (standard), got %d", weight_layout)

extern "C" {

int th_conv1x1_exact_fwd(th_ctx *ctx, const float *d_x, const float *d_w, const float *d_bias, float *d_y, int n, int c_in, int h, int w,
                         int c_out, int stride, int weight_layout, int relu) {
    TH_PW_CHECK("th_conv1x1_exact_fwd", d_x, d_w, d_y);
    TH_REQUIRE(relu == 0 || relu == 1, "th_conv1x1_exact_fwd: relu must be 0 or 1, got %d", relu);
    ConvPwPlan p;
    conv_pw_fwd_plan(&p, n, c_in, h, w, c_out, stride);
    TH_REQUIRE(!p.refused, "th_conv1x1_exact_fwd: the images of one pixel tile hold 2 GiB and more, 2^31 output pixels and more, or a launch grid "
                           "over the device limit (not supported)");
    ConvPwArgs a{};
    a.src = d_x; a.w = d_w; a.bias = d_bias; a.dst = d_y; a.relu = relu;
    a.n = n; a.k_ch = c_in; a.m_ch = c_out;
    a.src_chan = h * w; a.src_w = w; a.s_src = stride;
    a.dst_h = p.h_out; a.dst_w = p.w_out; a.s_dst = 1;
    a.w_out = p.w_out; a.P = p.h_out * p.w_out; a.total = n * a.P; a.span = p.span;
    a.w_sm = weight_layout == 0 ? 1 : c_in; a.w_sk = weight_layout == 0 ? c_out : 1;      // (m, k) = (co, ci)
    pw_launch<false>(ctx, p, a);
    TH_LAUNCH_CHECK();
    pw_note(p);
    return 0;
}

int th_conv1x1_exact_bwd_input(th_ctx *ctx, const float *d_gy, const float *d_w, float *d_gx, int n, int c_in, int h, int w, int c_out,
                               int stride, int weight_layout, int accumulate) {
    TH_PW_CHECK("th_conv1x1_exact_bwd_input", d_gy, d_w, d_gx);
    TH_REQUIRE(accumulate == 0 || accumulate == 1, "th_conv1x1_exact_bwd_input: accumulate must be 0 or 1, got %d", accumulate);
    ConvPwPlan p;
    conv_pw_bwd_input_plan(&p, n, c_in, h, w, c_out, stride, accumulate != 0);
    TH_REQUIRE(!p.refused, "th_conv1x1_exact_bwd_input: the images of one pixel tile hold 2 GiB and more, 2^31 output pixels and more, or a launch "
                           "grid over the device limit (not supported)");
    ConvPwArgs a{};
    a.src = d_gy; a.w = d_w; a.dst = d_gx; a.accumulate = accumulate;
    a.n = n; a.k_ch = c_out; a.m_ch = c_in;
    a.src_chan = p.h_out * p.w_out; a.src_w = p.w_out; a.s_src = 1;
    a.dst_h = h; a.dst_w = w; a.s_dst = stride;
    a.w_out = p.w_out; a.P = p.h_out * p.w_out; a.total = n * a.P; a.span = p.span;
    a.w_sm = weight_layout == 0 ? c_out : 1; a.w_sk = weight_layout == 0 ? 1 : c_in;      // (m, k) = (ci, co)
    pw_launch<true>(ctx, p, a);
    TH_LAUNCH_CHECK();
    pw_note(p);
    return 0;
}

int th_conv1x1_exact_bwd_weight(th_ctx *ctx, const float *d_x, const float *d_gy, float *d_gw, int n, int c_in, int h, int w, int c_out,
                                int stride, int weight_layout, int accumulate) {
    TH_PW_CHECK("th_conv1x1_exact_bwd_weight", d_x, d_gy, d_gw);
    TH_REQUIRE(accumulate == 0 || accumulate == 1, "th_conv1x1_exact_bwd_weight: accumulate must be 0 or 1, got %d", accumulate);
    ConvPwPlan p;
    conv_pw_bwd_weight_plan(&p, n, c_in, h, w, c_out, stride, weight_layout, accumulate != 0, ((uintptr_t)d_gw & 15) == 0);
    // (checked before the slabs are taken from the pool: an error return holds nothing)
    TH_REQUIRE(!p.refused, "th_conv1x1_exact_bwd_weight: maps of 2 GiB and more, 2^31 output pixels and more, or a launch grid over the device "
                           "limit (not supported)");
    void *ws = nullptr;
    if (th_malloc(ctx, (size_t)p.slabs * c_in * p.co_ld * sizeof(float), &ws)) return 1;
    ConvPwWgradArgs a{};
    a.x = d_x; a.gy = d_gy; a.part = (float *)ws;
    a.n = n; a.c_in = c_in; a.c_out = c_out; a.chan = h * w; a.w_in = w; a.stride = stride;
    a.w_out = p.w_out; a.P = p.h_out * p.w_out; a.total = n * a.P;
    a.n_pb = p.tiles; a.G = p.G; a.co_ld = p.co_ld;
    a.x_bytes = (unsigned)((size_t)n * c_in * h * w * 4);
    a.gy_bytes = (unsigned)((size_t)a.total * c_out * 4);
    const dim3 grid(p.grid_x, p.grid_y, p.grid_z);
    switch (p.ct) {
        case 4: hipLaunchKernelGGL(conv_pw_wgrad_kernel<4>, grid, dim3(256), 0, ctx->stream, a); break;
        case 2: hipLaunchKernelGGL(conv_pw_wgrad_kernel<2>, grid, dim3(256), 0, ctx->stream, a); break;
        default: hipLaunchKernelGGL(conv_pw_wgrad_kernel<1>, grid, dim3(256), 0, ctx->stream, a); break;
    }
    if (hipGetLastError() != hipSuccess) { th_free(ctx, ws); th::set_error("conv_pw_wgrad_kernel: launch failed"); return 1; }
    if (int rc = wgrad_reduce(ctx, a.part, d_gw, p.G, c_in, c_out, p.co_ld, weight_layout, accumulate)) { th_free(ctx, ws); return rc; }
    pw_note(p);
    return th_free(ctx, ws);
}

int th_debug_conv1x1_exact_plan(int op, int n, int c_in, int h, int w, int c_out, int stride, int weight_layout, int relu_bias, int accumulate,
                                int w_misalign_bytes, int *outN) {
    TH_REQUIRE(outN, "th_debug_conv1x1_exact_plan: null output");
    TH_REQUIRE(op >= 0 && op <= 2, "th_debug_conv1x1_exact_plan: op must be 0 (fwd), 1 (bwd_input) or 2 (bwd_weight), got %d", op);
    TH_REQUIRE(n >= 1 && c_in >= 1 && h >= 1 && w >= 1 && c_out >= 1, "th_debug_conv1x1_exact_plan: bad geometry n=%d c_in=%d h=%d w=%d c_out=%d", n,
               c_in, h, w, c_out);
    TH_REQUIRE(stride == 1 || stride == 2, "th_debug_conv1x1_exact_plan: stride must be 1 or 2, got %d", stride);
    TH_REQUIRE(weight_layout == 0 || weight_layout == 1, "th_debug_conv1x1_exact_plan: weight_layout must be 0 (taper) or 1 (standard)");
    TH_REQUIRE(relu_bias >= 0 && relu_bias <= 3 && (op == 0 || relu_bias == 0),
               "th_debug_conv1x1_exact_plan: relu_bias is relu + 2 * bias present (0 .. 3; 0 for the two backward ops), got %d", relu_bias);
    TH_REQUIRE(accumulate == 0 || (accumulate == 1 && op >= 1), "th_debug_conv1x1_exact_plan: accumulate is 0, or 1 for the two backward ops");
    TH_REQUIRE(w_misalign_bytes >= 0 && w_misalign_bytes < 16 && w_misalign_bytes % 4 == 0,
               "th_debug_conv1x1_exact_plan: w_misalign_bytes must be 0, 4, 8 or 12");
    ConvPwPlan p;
    if (op == 0) conv_pw_fwd_plan(&p, n, c_in, h, w, c_out, stride);
    else if (op == 1) conv_pw_bwd_input_plan(&p, n, c_in, h, w, c_out, stride, accumulate != 0);
    else conv_pw_bwd_weight_plan(&p, n, c_in, h, w, c_out, stride, weight_layout, accumulate != 0, w_misalign_bytes == 0);
    const int *src = reinterpret_cast<const int *>(&p);
    for (int i = 0; i < kConvPwPlanInts; ++i) outN[i] = src[i];
    return 0;
}

int th_debug_last_conv_pw_config(th_ctx *ctx, int *out9) {
    TH_REQUIRE(ctx && out9, "th_debug_last_conv_pw_config: null argument");
    for (int i = 0; i < 9; ++i) out9[i] = th::t_last_pw_cfg[i];
    return 0;
}

}  // extern "C"
