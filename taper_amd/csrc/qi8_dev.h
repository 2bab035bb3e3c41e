// qi8_dev.h -- what the int8 matrix-core kernels (qgemm_i8.hip, qconv_i8.hip) agree on, each decision written once: the 16-byte piece
// of codes, the LDS image of an operand stage with its fragment pairing, the epilogue's four f32 operations, and the window of a
// convolution or pool over channel-last codes.  Their results are bit-identical to a numpy restatement because of these and nothing else.
#pragma once
#include "quant_dev.h"

namespace th {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx16 __attribute__((ext_vector_type(16)));

// The longest K (in_features, or c_in k_h k_w) the products take: |acc + 128 rs| <= 128 * 255 * K stays below 2^31.
#define TH_Q8_MAX_K 65536
#define TH_Q8_STR_(x) #x
#define TH_Q8_STR(x) TH_Q8_STR_(x)
constexpr int kQ8MaxK = TH_Q8_MAX_K;

// ---- the piece ----
// 16 consecutive codes in a uint4: byte i in word i >> 2 at shift 8 (i & 3).  Padding is the code 0, which IS the value 0.
__device__ __forceinline__ uint32_t code_at(int q, int i) { return (uint32_t)(uint8_t)(int8_t)q << (8 * (i & 3)); }   // code q as byte i of its word

__device__ __forceinline__ uint4 piece_pack(const int (&q)[16], int live = 16) {   // codes live .. 15 come out 0
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i < live) w[i >> 2] |= code_at(q[i], i);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ int piece_code(const uint4 &p, int i) {
    const uint32_t w[4] = {p.x, p.y, p.z, p.w};
    return (int)(int8_t)((w[i >> 2] >> (8 * (i & 3))) & 0xFF);
}

__device__ __forceinline__ int piece_sum(const uint4 &p) {
    int sum = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum += piece_code(p, i);
    return sum;
}

// ---- the stage image ----
// LDS image of an operand stage: rows of 64 bytes, the 16-byte piece c of row r at the slot stage_slot gives -- the 16 lanes a
// ds_read_b128 serves together (rows {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} of one piece) then land on 16 different slots.
// Fragments: lane l (r = l & 31, h = l >> 5) holds 16 consecutive codes of row r of its operand, piece 2 s + h of the stage in MFMA
// step s -- for BOTH operands, so that whatever order the instruction gives the 16 codes of a lane, a code of x meets the code of W at
// the same k.  C/D: column = lane & 31 (a row of the B operand), row = (reg & 3) + 8 (reg >> 2) + 4 h (a row of the A operand).
__device__ __forceinline__ int stage_slot(int row, int piece) { return row * 4 + (piece ^ ((row >> 2) & 3)); }

__device__ __forceinline__ intx4 as_frag(const uint4 &v) { return intx4{(int)v.x, (int)v.y, (int)v.z, (int)v.w}; }

__device__ __forceinline__ intx4 stage_frag(const uint4 *stage, int row, int s, int h) { return as_frag(stage[stage_slot(row, 2 * s + h)]); }

// ---- the epilogue value ----
// The weight codec is affine with zero_point -128: w = (qw + 128) sw + mw, so x . w = sx (sw (acc + 128 rs) + mw rs) with rs the sum of
// the activation codes that met a weight -- every integer term is exact, and the four f32 operations round once each, in this order.
__device__ __forceinline__ float q8_rterm(float mw, int rs) { return __fmul_rn(mw, (float)rs); }   // (a caller with one rs hoists it)

// y = sx * (sw * (float)(acc + 128 rs) + rterm) [+ bias()] [ReLU]; bias() is called only when biased, after the product (the conv's is a load)
template <class Bias>
__device__ __forceinline__ float q8_value(int acc, int rs, float rterm, float sx, float sw, bool biased, Bias bias, int relu) {
    float v = __fmul_rn(sx, __fadd_rn(__fmul_rn(sw, (float)(acc + 128 * rs)), rterm));
    if (biased) v = __fadd_rn(v, bias());
    return relu ? (v > 0.f ? v : 0.f) : v;
}

// ---- the window ----
// A k_h x k_w window at stride s over an h x w map padded by pad; output pixels are numbered image by image, row by row.
struct QWindow {
    int h, w, k_h, k_w, s_h, s_w, pad_h, pad_w, h_out, w_out;

    struct Pixel {
        int img, p, oh, ow;   // p: the pixel's place in its image's output map
    };
    __device__ __forceinline__ Pixel split(int o) const {
        const int hw_out = h_out * w_out, img = o / hw_out, p = o - img * hw_out, oh = p / w_out;
        return Pixel{img, p, oh, p - oh * w_out};
    }
    __device__ __forceinline__ int top(int oh) const { return oh * s_h - pad_h; }    // the window's first tap, maybe outside the image
    __device__ __forceinline__ int left(int ow) const { return ow * s_w - pad_w; }
    // f(ih, iw) for every tap of output pixel (oh, ow) that lies inside the image
    template <class F>
    __device__ __forceinline__ void for_taps(int oh, int ow, F f) const {
        for (int kh = 0; kh < k_h; ++kh) {
            const int ih = top(oh) + kh;
            if (ih < 0 || ih >= h) continue;
            for (int kw = 0; kw < k_w; ++kw) {
                const int iw = left(ow) + kw;
                if (iw >= 0 && iw < w) f(ih, iw);
            }
        }
    }
};

// Host: the refusals every window shares, in their order of precedence -- the caller words the first that applies -- then the output map.
enum { kWinOk = 0, kWinBelowOne, kWinEmpty, kWinSide };
static inline int window_check(int h, int w, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, QWindow *win) {
    if (h <= 0 || w <= 0 || k_h <= 0 || k_w <= 0 || s_h <= 0 || s_w <= 0 || pad_h < 0 || pad_w < 0) return kWinBelowOne;
    if ((long)h + 2L * pad_h < k_h || (long)w + 2L * pad_w < k_w) return kWinEmpty;
    if ((long)h + 2L * pad_h > 0x7fffffffL || (long)w + 2L * pad_w > 0x7fffffffL) return kWinSide;
    *win = QWindow{h, w, k_h, k_w, s_h, s_w, pad_h, pad_w, (h + 2 * pad_h - k_h) / s_h + 1, (w + 2 * pad_w - k_w) / s_w + 1};
    return kWinOk;
}

// ---- packed codes -> padded pieces ----
// A thread per 16-byte piece of the destination [rows][taps][cpitch] (packed sources are not aligned in general: byte loads, once per
// weight).  The source is [rows][c_in][taps]; with taps == 1 the rows are copied and padded with zeros.  TAPER: the source is a weight
// the float conv kernels read in the reference's reinterpretation (weight_layout 0, tensor.rs:1262): the code of w_eff[co][ci][tap]
// lies at src[(ci taps + tap) c_out + co]
template <bool TAPER>
__global__ __launch_bounds__(256) void pack_conv_weight_kernel(const int8_t *__restrict__ src, long rows, int c_in, int taps, int8_t *__restrict__ dst,
                                                               int cpitch) {
    const int cp16 = cpitch / 16;
    const long total = rows * taps * cp16;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long rt = i / cp16;   // row * taps + tap
        const int c0 = (int)(i - rt * cp16) * 16;
        const long row = rt / taps;
        const int tap = (int)(rt - row * taps);
        const int8_t *s = TAPER ? src + (size_t)tap * rows + row : src + (size_t)row * c_in * taps + tap;
        const size_t step = TAPER ? (size_t)taps * rows : (size_t)taps;   // from one input channel to the next
        int q[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) q[j] = c0 + j < c_in ? s[(size_t)(c0 + j) * step] : 0;
        *(uint4 *)(dst + (size_t)i * 16) = piece_pack(q);
    }
}

}  // namespace th
