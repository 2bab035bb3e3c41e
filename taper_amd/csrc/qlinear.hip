// qlinear.hip -- forward of the reference's quantized Linear (src/nn.rs:88-120: x . deq(W)^T + deq(b)) straight from packed int8 / f16
// weights, and the multi-tensor dequantize behind the quantized conv stages (nn.rs:336-429 dequantize on every call).
//
// Small batches are bound by weight bytes: B <= kStreamMaxBatch (8) rows take a weight-streaming kernel (the usual GEMV form for
// M <= 16: no LDS round trip for the weights) that reads 16 bytes of codes per lane per row straight into VGPRs (16 int8 or 8 f16), dequantizes them in
// registers with exactly the codec's arithmetic and accumulates in f32; a wave owns R rows of W and strides K, so every x element it
// loads serves R rows.  When N / (4 R) workgroups cannot fill the device, K is split over workgroups too and the slices' partial sums
// are combined in slice order by a second launch (no float atomics: the result is bit-identical from run to run).  Larger batches
// dequantize into a pooled workspace and run th_linear_fwd's f32 product; the workspace goes back to the pool before the call returns.
#include "common.h"
#include "quant_dev.h"

namespace th {

constexpr int kStreamMaxBatch = 8;   // measured (profiles/quant_linear.md): at 16 rows the streaming kernel (105 us, int8 4096^2) loses to dequantize + th_linear_fwd
constexpr int kRowsPerWave = 4;
constexpr int kDqMax = 32;   // tensors per th_dequantize_multi launch (kernel argument of 32 * 40 bytes)

template <int QT> struct QCodes;           // QT: TH_QTYPE_INT8 / TH_QTYPE_F16
template <> struct QCodes<TH_QTYPE_INT8> { using T = int8_t; static constexpr int kPerLoad = 16; };
template <> struct QCodes<TH_QTYPE_F16> { using T = uint16_t; static constexpr int kPerLoad = 8; };

template <int QT>
__device__ __forceinline__ float decode(uint32_t word, int j, float scale, float min_val) {
    if constexpr (QT == TH_QTYPE_INT8) return dequant_int8((int)(int8_t)((word >> (8 * j)) & 0xFF), scale, min_val);
    else return f16_bits_to_f32((uint16_t)((word >> (16 * j)) & 0xFFFF));
}

// One wave: rows [n0, n0 + R) of W, K range [kb, ke) of this workgroup's slice, every lane E = 16 bytes of codes per row per step.
// VEC: K % E == 0 and 16-byte aligned x / W (one dwordx4 load per row, float4 loads of x); else element loads under bounds.
template <int QT, int BT, bool VEC>
__global__ __launch_bounds__(256) void qgemv_kernel(const float *__restrict__ x, int B, int K, const void *__restrict__ w, int N,
                                                    const float *__restrict__ wparams, const void *__restrict__ bcodes,
                                                    const float *__restrict__ bparams, int relu, float *__restrict__ y,
                                                    float *__restrict__ part, int kslice) {
    using T = typename QCodes<QT>::T;
    constexpr int E = QCodes<QT>::kPerLoad, R = kRowsPerWave, PW = 4 / (int)sizeof(T);   // PW: codes per 32-bit word
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (n0 >= N) return;   // (no barrier below)
    const int kb = blockIdx.y * kslice, ke = min(K, kb + kslice);
    float scale = 0.f, mn = 0.f;
    if constexpr (QT == TH_QTYPE_INT8) {
        mn = wparams[0];
        scale = wparams[1];
    }
    const T *wt = (const T *)w;
    const T *rows[R];
#pragma unroll
    for (int r = 0; r < R; ++r) rows[r] = wt + (size_t)min(n0 + r, N - 1) * K;   // rows past N re-read row N - 1, never stored
    float acc[R][BT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int b = 0; b < BT; ++b) acc[r][b] = 0.f;

    for (int k = kb + lane * E; k < ke; k += 64 * E) {
        uint32_t raw[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (VEC) {
                const uint4 v = *(const uint4 *)(rows[r] + k);
                raw[r][0] = v.x; raw[r][1] = v.y; raw[r][2] = v.z; raw[r][3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    uint32_t word = 0;
#pragma unroll
                    for (int p = 0; p < PW; ++p) {
                        const int kk = k + i * PW + p;
                        const uint32_t c = kk < ke ? (uint32_t)(sizeof(T) == 1 ? (uint8_t)rows[r][kk] : (uint16_t)rows[r][kk]) : 0u;
                        word |= c << (8 * sizeof(T) * p);
                    }
                    raw[r][i] = word;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {          // 4 words of codes: PW k positions each
#pragma unroll
            for (int p0 = 0; p0 < PW; p0 += (PW >= 4 ? 4 : PW)) {
                constexpr int G = PW >= 4 ? 4 : PW;   // k positions per x load (float4 for int8, float2 for f16)
                const int kk = k + i * PW + p0;
                float xv[BT][G];
#pragma unroll
                for (int b = 0; b < BT; ++b) {
                    if (b < B) {
                        const float *xp = x + (size_t)b * K + kk;
                        if constexpr (VEC && G == 4) {
                            const float4 v = *(const float4 *)xp;
                            xv[b][0] = v.x; xv[b][1] = v.y; xv[b][2] = v.z; xv[b][3] = v.w;
                        } else if constexpr (VEC && G == 2) {
                            const float2 v = *(const float2 *)xp;
                            xv[b][0] = v.x; xv[b][1] = v.y;
                        } else {
#pragma unroll
                            for (int g = 0; g < G; ++g) xv[b][g] = kk + g < ke ? xp[g] : 0.f;
                        }
                    } else {
#pragma unroll
                        for (int g = 0; g < G; ++g) xv[b][g] = 0.f;
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        // a code past the slice end decodes to some value; its x is 0 (and finite codes give finite weights)
                        const float wv = decode<QT>(raw[r][i], p0 + g, scale, mn);
#pragma unroll
                        for (int b = 0; b < BT; ++b) acc[r][b] = fmaf(xv[b][g], wv, acc[r][b]);
                    }
            }
        }
    }
    // wave sums in a fixed butterfly order
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int b = 0; b < BT; ++b)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc[r][b] += __shfl_xor(acc[r][b], off, 64);
    if (lane != 0) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int n = n0 + r;
        if (n >= N) continue;
        float bias = 0.f;
        if (!part && bcodes) {
            if constexpr (QT == TH_QTYPE_INT8) bias = dequant_int8(((const int8_t *)bcodes)[n], bparams[1], bparams[0]);
            else bias = f16_bits_to_f32(((const uint16_t *)bcodes)[n]);
        }
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            if (b >= B) continue;
            if (part) {
                part[((size_t)blockIdx.y * B + b) * N + n] = acc[r][b];
            } else {
                float v = acc[r][b] + bias;
                y[(size_t)b * N + n] = relu ? (v > 0.f ? v : 0.f) : v;
            }
        }
    }
}

// y[b][n] = sum over the K slices in slice order + deq(b[n]), ReLU
template <int QT>
__global__ __launch_bounds__(256) void qgemv_combine_kernel(const float *__restrict__ part, int S, int B, int N, const void *__restrict__ bcodes,
                                                            const float *__restrict__ bparams, int relu, float *__restrict__ y) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * N) return;
    const int n = i % N;
    float s = part[i];
    for (int j = 1; j < S; ++j) s += part[(size_t)j * B * N + i];
    if (bcodes) {
        if constexpr (QT == TH_QTYPE_INT8) s += dequant_int8(((const int8_t *)bcodes)[n], bparams[1], bparams[0]);
        else s += f16_bits_to_f32(((const uint16_t *)bcodes)[n]);
    }
    y[i] = relu ? (s > 0.f ? s : 0.f) : s;
}

struct DqList {
    th_qtensor it[kDqMax];
};

__global__ __launch_bounds__(256) void dequant_multi_kernel(DqList L) {
    const th_qtensor t = L.it[blockIdx.y];
    if (t.qtype == TH_QTYPE_INT8) {
        const int8_t *q = (const int8_t *)t.d_codes;
        const float mn = t.d_params[0], scale = t.d_params[1];
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < t.n; i += (int64_t)gridDim.x * 256) t.d_out[i] = dequant_int8(q[i], scale, mn);
    } else {
        const uint16_t *h = (const uint16_t *)t.d_codes;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < t.n; i += (int64_t)gridDim.x * 256) t.d_out[i] = f16_bits_to_f32(h[i]);
    }
}

static int dequant_multi(th_ctx *ctx, const th_qtensor *items, int n_items) {
    for (int i0 = 0; i0 < n_items; i0 += kDqMax) {
        DqList L{};
        const int m = std::min(kDqMax, n_items - i0);
        int64_t most = 0;
        for (int j = 0; j < m; ++j) {
            const th_qtensor &t = items[i0 + j];
            TH_REQUIRE(t.n >= 0 && (t.qtype == TH_QTYPE_INT8 || t.qtype == TH_QTYPE_F16), "th_dequantize_multi: item %d: bad qtype or length", i0 + j);
            TH_REQUIRE(t.n == 0 || (t.d_codes && t.d_out && (t.qtype != TH_QTYPE_INT8 || t.d_params)), "th_dequantize_multi: item %d: null pointer", i0 + j);
            L.it[j] = t;
            most = std::max(most, t.n);
        }
        if (most == 0) continue;
        hipLaunchKernelGGL(dequant_multi_kernel, dim3(std::min(ew_grid((size_t)most, 256), std::max(1, 2048 / m)), m), dim3(256), 0, ctx->stream, L);
        TH_LAUNCH_CHECK();
    }
    return 0;
}

template <int QT, int BT>
static void launch_stream(th_ctx *ctx, bool vec, dim3 grid, const float *x, int B, int K, const void *w, int N, const float *wp, const void *bc,
                          const float *bp, int relu, float *y, float *part, int kslice) {
    if (vec) hipLaunchKernelGGL((qgemv_kernel<QT, BT, true>), grid, dim3(256), 0, ctx->stream, x, B, K, w, N, wp, bc, bp, relu, y, part, kslice);
    else hipLaunchKernelGGL((qgemv_kernel<QT, BT, false>), grid, dim3(256), 0, ctx->stream, x, B, K, w, N, wp, bc, bp, relu, y, part, kslice);
}

// Every host decision of a quantized Linear forward (qlinear_fwd launches from it; th_debug_qlinear_plan reports it): the workspace
// path above kStreamMaxBatch rows, else the streaming kernel's instance (vec, bt) and its grid blocks_n x S with kslice k positions a slice.
// E: codes per 16-byte load; x_bits / w_bits: the pointers (only their low 4 bits matter).
struct QPlan {
    int stream, vec, bt, kslice, S, blocks_n, want, steps;
};

static QPlan qlinear_plan(int E, int B, int K, int N, uintptr_t x_bits, uintptr_t w_bits) {
    QPlan p{};
    if (B > kStreamMaxBatch) return p;
    p.stream = 1;
    p.vec = K % E == 0 && (x_bits & 15) == 0 && (w_bits & 15) == 0;
    p.blocks_n = ceil_div(N, 4 * kRowsPerWave);
    p.steps = ceil_div(K, 64 * E);                                              // k steps of a wave over the whole row
    p.want = std::max(1, std::min(p.steps, ceil_div(4 * kNumCU, p.blocks_n)));   // ~4 workgroups per CU in all
    p.kslice = ceil_div(p.steps, p.want) * 64 * E;
    p.S = ceil_div(K, p.kslice);
    p.bt = B <= 1 ? 1 : B <= 2 ? 2 : B <= 4 ? 4 : 8;
    return p;
}

template <int QT>
static int qlinear_fwd(th_ctx *ctx, const char *name, const float *x, int B, int K, const void *w, int N, const float *wp, const void *bc,
                       const float *bp, int relu, float *y) {
    TH_REQUIRE(ctx && x && w && y && (QT != TH_QTYPE_INT8 || wp) && (!bc || QT != TH_QTYPE_INT8 || bp), "%s: null argument", name);
    TH_REQUIRE(B >= 0 && K > 0 && N > 0, "%s: bad shape B=%d K=%d N=%d", name, B, K, N);
    if (B == 0) return 0;
    const QPlan p = qlinear_plan(QCodes<QT>::kPerLoad, B, K, N, (uintptr_t)x, (uintptr_t)w);
    if (!p.stream) {
        // dequantize W (and b) into one pooled workspace, the f32 product, the workspace back to the pool
        const size_t wn = (size_t)K * N, boff = (wn + 63) / 64 * 64;
        void *ws = nullptr;
        if (th_malloc(ctx, (boff + (bc ? (size_t)N : 0)) * sizeof(float), &ws)) return 1;
        float *dw = (float *)ws, *db = bc ? dw + boff : nullptr;
        th_qtensor items[2] = {{w, wp, dw, (int64_t)wn, QT}, {bc, bp, db, (int64_t)N, QT}};
        int rc = dequant_multi(ctx, items, bc ? 2 : 1);
        if (!rc) rc = th_linear_fwd(ctx, x, dw, db, y, B, K, N, relu);
        const int rf = th_free(ctx, ws);
        return rc ? rc : rf;
    }
    const bool vec = p.vec != 0;
    const int kslice = p.kslice, S = p.S;
    float *part = nullptr;
    if (S > 1 && th_malloc(ctx, (size_t)S * B * N * sizeof(float), (void **)&part)) return 1;
    const dim3 grid(p.blocks_n, S);
    switch (p.bt) {
        case 1: launch_stream<QT, 1>(ctx, vec, grid, x, B, K, w, N, wp, bc, bp, relu, y, part, kslice); break;
        case 2: launch_stream<QT, 2>(ctx, vec, grid, x, B, K, w, N, wp, bc, bp, relu, y, part, kslice); break;
        case 4: launch_stream<QT, 4>(ctx, vec, grid, x, B, K, w, N, wp, bc, bp, relu, y, part, kslice); break;
        default: launch_stream<QT, 8>(ctx, vec, grid, x, B, K, w, N, wp, bc, bp, relu, y, part, kslice); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && part) {
        hipLaunchKernelGGL(qgemv_combine_kernel<QT>, dim3(ceil_div((long)B * N, 256)), dim3(256), 0, ctx->stream, part, S, B, N, bc, bp, relu, y);
        e = hipGetLastError();
    }
    const int rf = part ? th_free(ctx, part) : 0;
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", name, hipGetErrorString(e));
        return 1;
    }
    return rf;
}

}  // namespace th

using namespace th;

extern "C" {

int th_linear_q8_fwd(th_ctx *ctx, const float *d_x, int batch, int in_features, const int8_t *d_qw, int out_features, const float *d_wparams,
                     const int8_t *d_qb, const float *d_bparams, int relu, float *d_y) {
    return qlinear_fwd<TH_QTYPE_INT8>(ctx, "th_linear_q8_fwd", d_x, batch, in_features, d_qw, out_features, d_wparams, d_qb, d_bparams, relu, d_y);
}

int th_linear_h16_fwd(th_ctx *ctx, const float *d_x, int batch, int in_features, const uint16_t *d_hw, int out_features, const uint16_t *d_hb,
                      int relu, float *d_y) {
    return qlinear_fwd<TH_QTYPE_F16>(ctx, "th_linear_h16_fwd", d_x, batch, in_features, d_hw, out_features, nullptr, d_hb, nullptr, relu, d_y);
}

int th_qlinear_stream_max_batch(void) { return kStreamMaxBatch; }

int th_debug_qlinear_plan(int qtype, int batch, int in_features, int out_features, int x_misalign_bytes, int w_misalign_bytes, int *out8) {
    TH_REQUIRE(out8 && (qtype == TH_QTYPE_INT8 || qtype == TH_QTYPE_F16), "th_debug_qlinear_plan: null argument or bad qtype %d", qtype);
    TH_REQUIRE(batch >= 1 && in_features > 0 && out_features > 0 && x_misalign_bytes >= 0 && w_misalign_bytes >= 0,
               "th_debug_qlinear_plan: bad shape B=%d K=%d N=%d", batch, in_features, out_features);
    const QPlan p = qlinear_plan(qtype == TH_QTYPE_INT8 ? QCodes<TH_QTYPE_INT8>::kPerLoad : QCodes<TH_QTYPE_F16>::kPerLoad, batch, in_features,
                                 out_features, (uintptr_t)x_misalign_bytes, (uintptr_t)w_misalign_bytes);
    const int out[8] = {p.stream, p.vec, p.bt, p.kslice, p.S, p.blocks_n, p.want, p.steps};
    std::copy(out, out + 8, out8);
    return 0;
}

int th_dequantize_multi(th_ctx *ctx, const th_qtensor *h_items, int n_items) {
    TH_REQUIRE(ctx && n_items >= 0 && (n_items == 0 || h_items), "th_dequantize_multi: null argument");
    return dequant_multi(ctx, h_items, n_items);
}

}  // extern "C"
