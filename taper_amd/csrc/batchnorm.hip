// batchnorm.hip -- BatchNorm2d over an NCHW map, batch statistics on the device (torch.nn.BatchNorm2d's semantics: upstream announces the
// layer in nn.rs:829-857 and never writes it):
//
//   th_batchnorm2d_fwd   training: per-channel mean / biased variance over the M = n * hw elements of a channel, the running update
//                        (unbiased variance) and y = (x - mean) * (invstd * gamma) + beta [+ ReLU]; eval: the same map on the running pair
//   th_batchnorm2d_bwd   gbeta = sum gy, ggamma = sum gy * xh, gx = gamma * invstd * (gy - gbeta / M - xh * ggamma / M)
//
// Layout.  Channel ch owns the planes (b * c + ch) * hw, b < n.  Its elements are walked in UNITS: float4s when hw % 4 == 0 and every
// pointer is 16-byte aligned (then every plane base is), single floats otherwise.  Unit u of a channel is unit u % upp of plane u / upp
// (upp = units per plane); a lane keeps {plane, offset} and advances both by the workgroup's stride without a division, so a workgroup's
// 256 lanes stay busy whatever hw is (a 14 x 14 plane is 49 float4s; hw = 1 is one float per plane).
//
// Work items.  A channel's units are cut into S contiguous shares (bn_split: at least kBnSplitMin elements each, at most kBnGrid items
// in all, S <= 256); item w = ch * S + s, a workgroup takes the items w = blockIdx.x, + gridDim.x, ... -- c = 2 spreads over up to 512
// workgroups, c = 300 gets one workgroup per channel, c above the grid loops.
//
// Passes.  S > 1: two launches each way -- per-item partial sums {s1, s2} into a pooled block, then every item folds its channel's S
// partials itself (the same fixed tree in every workgroup: no hand-off between workgroups, no atomics) and maps its share; item s = 0
// also writes the per-channel outputs (saved statistics and the running update; ggamma / gbeta).  S == 1 (a channel is one share): ONE
// launch, the workgroup sums its channel and reads it a second time for the map, out of L2.  Eval: one launch.
//
// Numerics.  The sums of the forward are taken of x - K, K = the channel's first element, the same in every workgroup:
// mean = K + s1 / M, var = (s2 - s1 * s1 / M) / M -- the cancellation is that of a channel centred within its own spread, whatever
// |mean| / std is, and a constant channel gives mean = K exactly and var = 0 exactly.  Every sum is lane-local
// adds, a 64-lane butterfly and ((w0 + w1) + (w2 + w3)) over the waves: one order, bit-identical from run to run.
#include "common.h"
#include "stream_dev.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>

namespace th {

constexpr int kBnThreads = kStreamThreads;
constexpr int kBnMaxSplit = 256;           // shares of a channel at most: one lane of the fold each
constexpr int64_t kBnSplitMin = 4096;      // elements of a share at least (16 KiB: 4 float4s per lane)
constexpr int kBnGrid = 2048;              // work items at most when channels are split (8 per CU)

template <class V> struct BnUnit;
template <> struct BnUnit<float> { static constexpr int lanes = 1; };
template <> struct BnUnit<float4> { static constexpr int lanes = 4; };

__device__ __forceinline__ float hsum(float a) { return a; }
__device__ __forceinline__ float hsum(const float4 &a) { return (a.x + a.y) + (a.z + a.w); }

// every lane of the workgroup leaves with the workgroup's two sums (s: 8 floats of LDS; the trailing barrier frees it for the next call)
__device__ __forceinline__ void block_sum2(float *a, float *b, float *s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        *a = *a + __shfl_xor(*a, off, 64);
        *b = *b + __shfl_xor(*b, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s[threadIdx.x >> 6] = *a;
        s[4 + (threadIdx.x >> 6)] = *b;
    }
    lds_barrier();   // (global loads issued ahead of the sum stay in flight across it)
    *a = (s[0] + s[1]) + (s[2] + s[3]);
    *b = (s[4] + s[5]) + (s[6] + s[7]);
    lds_barrier();
}

// This lane's units of [u0, u1) of channel ch, as indices into the tensor seen as an array of V (a channel has fewer than 2^31 elements:
// 32-bit unit counts, one 32-bit division per lane)
struct BnCursor {
    unsigned u, u1, plane;
    int off, upp, c, ch, dp, doff;
    __device__ __forceinline__ BnCursor(unsigned u0, unsigned u1_, int upp_, int c_, int ch_) : u(u0 + threadIdx.x), u1(u1_), upp(upp_), c(c_), ch(ch_) {
        plane = u / (unsigned)upp;
        off = (int)(u - plane * (unsigned)upp);
        dp = kBnThreads / upp;
        doff = kBnThreads % upp;
    }
    __device__ __forceinline__ bool more(int ahead = 0) const { return u + ahead * kBnThreads < u1; }
    __device__ __forceinline__ int64_t next() {
        const int64_t i = ((int64_t)plane * c + ch) * upp + off;
        off += doff;
        plane += dp;
        if (off >= upp) {
            off -= upp;
            ++plane;
        }
        u += kBnThreads;
        return i;
    }
};
// use(i) for the rest of a cursor; four units per trip so that their loads are in flight together
template <class Use>
__device__ __forceinline__ void bn_walk(BnCursor cur, Use use) {
    while (cur.more(3)) {
        const int64_t i0 = cur.next(), i1 = cur.next(), i2 = cur.next(), i3 = cur.next();
        use(i0);
        use(i1);
        use(i2);
        use(i3);
    }
    while (cur.more()) use(cur.next());
}
template <class Use>
__device__ __forceinline__ void bn_walk(unsigned u0, unsigned u1, int upp, int c, int ch, Use use) {
    bn_walk(BnCursor(u0, u1, upp, c, ch), use);
}

// the shift of a channel's sums: the channel's first element (one uniform load; every workgroup of the channel takes the same)
__device__ __forceinline__ float bn_shift(const float *__restrict__ x, int hw, int ch) { return x[(int64_t)ch * hw]; }

struct BnItem {
    int ch, s;
    unsigned u0, u1;
};
// share s of S of a channel's units: the first units % S shares hold one unit more
__device__ __forceinline__ BnItem bn_item(int w, int S, unsigned units) {
    BnItem it;
    it.ch = w / S;
    it.s = w - it.ch * S;
    const unsigned q = units / (unsigned)S, r = units - q * (unsigned)S, s = (unsigned)it.s;
    it.u0 = s * q + (s < r ? s : r);
    it.u1 = it.u0 + q + (s < r ? 1u : 0u);
    return it;
}

// ---- forward ----
template <class V>
__device__ __forceinline__ void bn_fwd_sums(const float *__restrict__ x, unsigned u0, unsigned u1, int upp, int c, int ch, float k, float *s1, float *s2) {
    float a = 0.0f, b = 0.0f;
    bn_walk(u0, u1, upp, c, ch, [&](int64_t i) {
        const V d = vmap([k](float v) { return v - k; }, at<V>(x, i));
        a += hsum(d);
        b += hsum(vmap([](float v) { return v * v; }, d));
    });
    *s1 = a;
    *s2 = b;
}

template <class V>
__device__ __forceinline__ void bn_fwd_map(const float *__restrict__ x, float *__restrict__ y, unsigned u0, unsigned u1, int upp, int c, int ch, float mean,
                                           float a, float b, int relu) {
    const float floor_ = relu ? 0.0f : -INFINITY;
    bn_walk(u0, u1, upp, c, ch, [&](int64_t i) {
        put(y, i, vmap([=](float v) { return fmaxf((v - mean) * a + b, floor_); }, at<V>(x, i)));
    });
}

// first launch of a split forward: part[2 w] = sum (x - K), part[2 w + 1] = sum (x - K)^2 of item w
template <class V>
__global__ __launch_bounds__(kBnThreads) void bn_fwd_parts_kernel(const float *__restrict__ x, float *__restrict__ part, int n, int c, int hw, int S) {
    __shared__ float lds[8];
    const int upp = hw / BnUnit<V>::lanes;
    const unsigned units = (unsigned)n * (unsigned)upp;
    for (int w = blockIdx.x; w < c * S; w += gridDim.x) {
        const BnItem it = bn_item(w, S, units);
        const float k = bn_shift(x, hw, it.ch);
        float s1, s2;
        bn_fwd_sums<V>(x, it.u0, it.u1, upp, c, it.ch, k, &s1, &s2);
        block_sum2(&s1, &s2, lds);
        if (threadIdx.x == 0) {
            part[2 * (int64_t)w] = s1;
            part[2 * (int64_t)w + 1] = s2;
        }
    }
}

// the training forward's statistics, running update and map.  kSingle: S == 1, the sums are taken here (part unused)
template <class V, bool kSingle>
__global__ __launch_bounds__(kBnThreads) void bn_fwd_train_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                  float *__restrict__ y, float *__restrict__ running_mean, float *__restrict__ running_var,
                                                                  float *__restrict__ save_mean, float *__restrict__ save_invstd,
                                                                  const float *__restrict__ part, int n, int c, int hw, int S, float eps, float momentum, int relu) {
    __shared__ float lds[8];
    const int upp = hw / BnUnit<V>::lanes;
    const unsigned units = (unsigned)n * (unsigned)upp;
    const int64_t m = (int64_t)n * hw;
    for (int w = blockIdx.x; w < c * S; w += gridDim.x) {
        const BnItem it = bn_item(w, S, units);
        const float k = bn_shift(x, hw, it.ch);
        // the split form asks for its partials, then for its first trip, and folds while the trip's loads fly (the partials come back
        // first: the wait in front of the fold leaves the four younger loads out)
        float s1 = 0.0f, s2 = 0.0f;
        if constexpr (!kSingle) {   // (every lane loads, lanes past S a partial they drop: no branch, so the wait below can count)
            const int t = (int)threadIdx.x < S ? (int)threadIdx.x : S - 1;
            const float2 p = *reinterpret_cast<const float2 *>(part + 2 * ((int64_t)it.ch * S + t));
            s1 = (int)threadIdx.x < S ? p.x : 0.0f;
            s2 = (int)threadIdx.x < S ? p.y : 0.0f;
        }
        BnCursor cur(it.u0, it.u1, upp, c, it.ch);
        const bool pre = !kSingle && cur.more(3);
        int64_t i0, i1, i2, i3;
        i0 = i1 = i2 = i3 = (int64_t)it.ch * upp;   // (lanes without a whole trip load the channel's first unit and drop it)
        if (pre) i0 = cur.next(), i1 = cur.next(), i2 = cur.next(), i3 = cur.next();
        V v0 = V(), v1 = V(), v2 = V(), v3 = V();
        if constexpr (!kSingle) v0 = at<V>(x, i0), v1 = at<V>(x, i1), v2 = at<V>(x, i2), v3 = at<V>(x, i3);
        if (kSingle) bn_fwd_sums<V>(x, it.u0, it.u1, upp, c, it.ch, k, &s1, &s2);
        block_sum2(&s1, &s2, lds);
        const float fm = (float)m, d = s1 / fm;
        const float mean = k + d;
        const float var = fmaxf((s2 - s1 * d) / fm, 0.0f);
        const float invstd = __fdiv_rn(1.0f, __fsqrt_rn(var + eps));
        if (it.s == 0 && threadIdx.x == 0) {
            save_mean[it.ch] = mean;
            save_invstd[it.ch] = invstd;
            running_mean[it.ch] = (1.0f - momentum) * running_mean[it.ch] + momentum * mean;
            running_var[it.ch] = (1.0f - momentum) * running_var[it.ch] + momentum * (var * (fm / (fm - 1.0f)));
        }
        const float a = invstd * gamma[it.ch], b = beta[it.ch], floor_ = relu ? 0.0f : -INFINITY;
        auto f = [=](float v) { return fmaxf((v - mean) * a + b, floor_); };
        if (pre) {
            put(y, i0, vmap(f, v0));
            put(y, i1, vmap(f, v1));
            put(y, i2, vmap(f, v2));
            put(y, i3, vmap(f, v3));
        }
        bn_walk(cur, [&](int64_t i) { put(y, i, vmap(f, at<V>(x, i))); });
    }
}

template <class V>
__global__ __launch_bounds__(kBnThreads) void bn_fwd_eval_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                 float *__restrict__ y, const float *__restrict__ running_mean,
                                                                 const float *__restrict__ running_var, float *__restrict__ save_mean,
                                                                 float *__restrict__ save_invstd, int n, int c, int hw, int S, float eps, int relu) {
    const int upp = hw / BnUnit<V>::lanes;
    const unsigned units = (unsigned)n * (unsigned)upp;
    for (int w = blockIdx.x; w < c * S; w += gridDim.x) {
        const BnItem it = bn_item(w, S, units);
        const float mean = running_mean[it.ch];
        const float invstd = __fdiv_rn(1.0f, __fsqrt_rn(running_var[it.ch] + eps));
        if (it.s == 0 && threadIdx.x == 0) {
            save_mean[it.ch] = mean;
            save_invstd[it.ch] = invstd;
        }
        bn_fwd_map<V>(x, y, it.u0, it.u1, upp, c, it.ch, mean, invstd * gamma[it.ch], beta[it.ch], relu);
    }
}

// ---- backward ----
// gy with the fused ReLU's mask (ops.rs:358-369: a gradient is kept where the output is > 0)
__device__ __forceinline__ float bn_masked(float g, float y) { return y > 0.0f ? g : 0.0f; }

template <class V, bool kMask>
__device__ __forceinline__ V bn_gy(const float *__restrict__ gy, const float *__restrict__ y, int64_t i) {
    const V g = at<V>(gy, i);
    if constexpr (kMask) return vmap([](float gv, float yv) { return bn_masked(gv, yv); }, g, at<V>(y, i));
    else return g;
}

template <class V, bool kMask>
__device__ __forceinline__ void bn_bwd_sums(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ y, unsigned u0, unsigned u1,
                                            int upp, int c, int ch, float mean, float invstd, float *s1, float *s2) {
    float a = 0.0f, b = 0.0f;
    bn_walk(u0, u1, upp, c, ch, [&](int64_t i) {
        const V g = bn_gy<V, kMask>(gy, y, i);
        a += hsum(g);
        b += hsum(vmap([=](float gv, float xv) { return gv * ((xv - mean) * invstd); }, g, at<V>(x, i)));
    });
    *s1 = a;
    *s2 = b;
}

template <class V, bool kMask>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_parts_kernel(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ y,
                                                                  const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
                                                                  float *__restrict__ part, int n, int c, int hw, int S) {
    __shared__ float lds[8];
    const int upp = hw / BnUnit<V>::lanes;
    const unsigned units = (unsigned)n * (unsigned)upp;
    for (int w = blockIdx.x; w < c * S; w += gridDim.x) {
        const BnItem it = bn_item(w, S, units);
        float s1, s2;
        bn_bwd_sums<V, kMask>(gy, x, y, it.u0, it.u1, upp, c, it.ch, save_mean[it.ch], save_invstd[it.ch], &s1, &s2);
        block_sum2(&s1, &s2, lds);
        if (threadIdx.x == 0) {
            part[2 * (int64_t)w] = s1;
            part[2 * (int64_t)w + 1] = s2;
        }
    }
}

// the channel sums (kSingle: taken here), ggamma / gbeta by item s = 0, and the map unless gx is null.  acc: bit 0 gx, 1 ggamma, 2 gbeta
template <class V, bool kSingle, bool kMask>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_final_kernel(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ y,
                                                                  const float *__restrict__ gamma, const float *__restrict__ save_mean,
                                                                  const float *__restrict__ save_invstd, float *__restrict__ gx, float *__restrict__ ggamma,
                                                                  float *__restrict__ gbeta, const float *__restrict__ part, int n, int c, int hw, int S,
                                                                  int batch_stats, int acc) {
    __shared__ float lds[8];
    const int upp = hw / BnUnit<V>::lanes;
    const unsigned units = (unsigned)n * (unsigned)upp;
    const float fm = (float)((int64_t)n * hw);
    for (int w = blockIdx.x; w < c * S; w += gridDim.x) {
        const BnItem it = bn_item(w, S, units);
        const float mean = save_mean[it.ch], invstd = save_invstd[it.ch];
        // (as in the forward: the split form asks for its partials, then for its first trip, and folds while that trip's loads fly)
        float s1 = 0.0f, s2 = 0.0f;
        if constexpr (!kSingle) {   // (every lane loads, lanes past S a partial they drop: no branch, so the wait below can count)
            const int t = (int)threadIdx.x < S ? (int)threadIdx.x : S - 1;
            const float2 p = *reinterpret_cast<const float2 *>(part + 2 * ((int64_t)it.ch * S + t));
            s1 = (int)threadIdx.x < S ? p.x : 0.0f;
            s2 = (int)threadIdx.x < S ? p.y : 0.0f;
        }
        BnCursor cur(it.u0, it.u1, upp, c, it.ch);
        const bool pre = !kSingle && gx && cur.more(3);
        int64_t i0, i1, i2, i3;
        i0 = i1 = i2 = i3 = (int64_t)it.ch * upp;
        if (pre) i0 = cur.next(), i1 = cur.next(), i2 = cur.next(), i3 = cur.next();
        V g0 = V(), g1 = V(), g2 = V(), g3 = V(), x0 = V(), x1 = V(), x2 = V(), x3 = V();
        if constexpr (!kSingle) {
            g0 = bn_gy<V, kMask>(gy, y, i0), g1 = bn_gy<V, kMask>(gy, y, i1), g2 = bn_gy<V, kMask>(gy, y, i2), g3 = bn_gy<V, kMask>(gy, y, i3);
            x0 = at<V>(x, i0), x1 = at<V>(x, i1), x2 = at<V>(x, i2), x3 = at<V>(x, i3);
        }
        if (kSingle) bn_bwd_sums<V, kMask>(gy, x, y, it.u0, it.u1, upp, c, it.ch, mean, invstd, &s1, &s2);
        block_sum2(&s1, &s2, lds);
        if (it.s == 0 && threadIdx.x == 0) {
            gbeta[it.ch] = (acc & 4) ? gbeta[it.ch] + s1 : s1;
            ggamma[it.ch] = (acc & 2) ? ggamma[it.ch] + s2 : s2;
        }
        if (!gx) continue;
        const float a = gamma[it.ch] * invstd;
        const float c1 = batch_stats ? s1 / fm : 0.0f, c2 = batch_stats ? s2 / fm : 0.0f;
        const bool add = (acc & 1) != 0;
        auto emit = [&](int64_t i, const V &g, const V &xv) {
            V r = batch_stats ? vmap([=](float gv, float xe) { return a * (gv - c1 - ((xe - mean) * invstd) * c2); }, g, xv)
                              : vmap([=](float gv) { return a * gv; }, g);
            if (add) r = vmap([](float rv, float old) { return old + rv; }, r, at<V>(gx, i));
            put(gx, i, r);
        };
        if (pre) {
            emit(i0, g0, x0);
            emit(i1, g1, x1);
            emit(i2, g2, x2);
            emit(i3, g3, x3);
        }
        bn_walk(cur, [&](int64_t i) { emit(i, bn_gy<V, kMask>(gy, y, i), at<V>(x, i)); });
    }
}

// ---- the column form: hw == 1 ----
// x is [n][c]: a channel is a column, neighbouring channels are neighbouring floats.  A workgroup takes kColTile = 64 channels, one per
// lane (a wave's load is 256 contiguous bytes), its four waves the rows r0 + wave, + 4, ...; item w = tile * S + share of the rows.  The
// sums of the four waves meet in LDS in a fixed order; partials are [item][lane]{s1, s2}; the fold of a tile's S partials is wave by
// wave (s = wave, + 4, ...) and then the same LDS step.  The shift K of a channel: its first row's element.
constexpr int kColTile = 64;
constexpr int kColRowsMin = 32;   // rows of a share at least (8 per wave: two trips of four loads in flight)

struct ColItem {
    int tile, s, ch, r0, r1;
    bool on;   // this lane's channel exists
};
__device__ __forceinline__ ColItem col_item(int w, int S, int n, int c) {
    ColItem it;
    it.tile = w / S;
    it.s = w - it.tile * S;
    it.ch = it.tile * kColTile + (threadIdx.x & 63);
    it.on = it.ch < c;
    const int q = n / S, r = n - q * S;
    it.r0 = it.s * q + (it.s < r ? it.s : r);
    it.r1 = it.r0 + q + (it.s < r ? 1 : 0);
    return it;
}
// use(i) for this lane's rows of [r0, r1), i = the element's index; four rows per trip
template <class Use>
__device__ __forceinline__ void col_walk(const ColItem &it, int c, Use use) {
    if (!it.on) return;
    int r = it.r0 + (threadIdx.x >> 6);
    for (; r + 12 < it.r1; r += 16) {
        const int64_t i = (int64_t)r * c + it.ch;
        use(i);
        use(i + 4 * (int64_t)c);
        use(i + 8 * (int64_t)c);
        use(i + 12 * (int64_t)c);
    }
    for (; r < it.r1; r += 4) use((int64_t)r * c + it.ch);
}
// every wave leaves with the four waves' sums per lane (s: 2 * 4 * 64 floats of LDS; the trailing barrier frees it)
__device__ __forceinline__ void col_sum2(float *a, float *b, float *s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s[wave * 64 + lane] = *a;
    s[256 + wave * 64 + lane] = *b;
    lds_barrier();
    *a = (s[lane] + s[64 + lane]) + (s[128 + lane] + s[192 + lane]);
    *b = (s[256 + lane] + s[320 + lane]) + (s[384 + lane] + s[448 + lane]);
    lds_barrier();
}
__device__ __forceinline__ float col_shift(const float *__restrict__ x, const ColItem &it, int n, int c) {
    return it.on ? x[it.ch] : 0.0f;
}
__device__ __forceinline__ void col_fold(const float *__restrict__ part, const ColItem &it, int S, float *s1, float *s2) {
    float a = 0.0f, b = 0.0f;
#pragma unroll 8
    for (int k = threadIdx.x >> 6; k < S; k += 4) {   // (unrolled: the partials' loads are in flight together, the adds keep their order)
        const float2 v = *reinterpret_cast<const float2 *>(part + 2 * (((int64_t)it.tile * S + k) * kColTile + (threadIdx.x & 63)));
        a += v.x;
        b += v.y;
    }
    *s1 = a;
    *s2 = b;
}
__device__ __forceinline__ void col_put_part(float *__restrict__ part, int w, float s1, float s2) {
    if (threadIdx.x < 64) {
        const int64_t p = 2 * ((int64_t)w * kColTile + threadIdx.x);
        part[p] = s1;
        part[p + 1] = s2;
    }
}

__global__ __launch_bounds__(kBnThreads) void col_fwd_parts_kernel(const float *__restrict__ x, float *__restrict__ part, int n, int c, int tiles, int S) {
    __shared__ float lds[512];
    for (int w = blockIdx.x; w < tiles * S; w += gridDim.x) {
        const ColItem it = col_item(w, S, n, c);
        const float k = col_shift(x, it, n, c);
        float s1 = 0.0f, s2 = 0.0f;
        col_walk(it, c, [&](int64_t i) {
            const float d = x[i] - k;
            s1 += d;
            s2 += d * d;
        });
        col_sum2(&s1, &s2, lds);
        col_put_part(part, w, s1, s2);
    }
}

template <bool kSingle>
__global__ __launch_bounds__(kBnThreads) void col_fwd_train_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                   float *__restrict__ y, float *__restrict__ running_mean, float *__restrict__ running_var,
                                                                   float *__restrict__ save_mean, float *__restrict__ save_invstd,
                                                                   const float *__restrict__ part, int n, int c, int tiles, int S, float eps, float momentum,
                                                                   int relu) {
    __shared__ float lds[512];
    const float floor_ = relu ? 0.0f : -INFINITY;
    for (int w = blockIdx.x; w < tiles * S; w += gridDim.x) {
        const ColItem it = col_item(w, S, n, c);
        const float k = col_shift(x, it, n, c);
        float s1 = 0.0f, s2 = 0.0f;
        if (kSingle) {
            col_walk(it, c, [&](int64_t i) {
                const float d = x[i] - k;
                s1 += d;
                s2 += d * d;
            });
        } else {
            col_fold(part, it, S, &s1, &s2);
        }
        col_sum2(&s1, &s2, lds);
        const float fm = (float)n, d = s1 / fm;
        const float mean = k + d;
        const float var = fmaxf((s2 - s1 * d) / fm, 0.0f);
        const float invstd = __fdiv_rn(1.0f, __fsqrt_rn(var + eps));
        if (it.s == 0 && threadIdx.x < 64 && it.on) {
            save_mean[it.ch] = mean;
            save_invstd[it.ch] = invstd;
            running_mean[it.ch] = (1.0f - momentum) * running_mean[it.ch] + momentum * mean;
            running_var[it.ch] = (1.0f - momentum) * running_var[it.ch] + momentum * (var * (fm / (fm - 1.0f)));
        }
        const float a = it.on ? invstd * gamma[it.ch] : 0.0f, b = it.on ? beta[it.ch] : 0.0f;
        col_walk(it, c, [&](int64_t i) { y[i] = fmaxf((x[i] - mean) * a + b, floor_); });
    }
}

__global__ __launch_bounds__(kBnThreads) void col_fwd_eval_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                  float *__restrict__ y, const float *__restrict__ running_mean,
                                                                  const float *__restrict__ running_var, float *__restrict__ save_mean,
                                                                  float *__restrict__ save_invstd, int n, int c, int tiles, int S, float eps, int relu) {
    const float floor_ = relu ? 0.0f : -INFINITY;
    for (int w = blockIdx.x; w < tiles * S; w += gridDim.x) {
        const ColItem it = col_item(w, S, n, c);
        if (!it.on) continue;
        const float mean = running_mean[it.ch];
        const float invstd = __fdiv_rn(1.0f, __fsqrt_rn(running_var[it.ch] + eps));
        if (it.s == 0 && threadIdx.x < 64) {
            save_mean[it.ch] = mean;
            save_invstd[it.ch] = invstd;
        }
        const float a = invstd * gamma[it.ch], b = beta[it.ch];
        col_walk(it, c, [&](int64_t i) { y[i] = fmaxf((x[i] - mean) * a + b, floor_); });
    }
}

__global__ __launch_bounds__(kBnThreads) void col_bwd_parts_kernel(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ y,
                                                                   const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
                                                                   float *__restrict__ part, int n, int c, int tiles, int S) {
    __shared__ float lds[512];
    for (int w = blockIdx.x; w < tiles * S; w += gridDim.x) {
        const ColItem it = col_item(w, S, n, c);
        const float mean = it.on ? save_mean[it.ch] : 0.0f, invstd = it.on ? save_invstd[it.ch] : 0.0f;
        float s1 = 0.0f, s2 = 0.0f;
        col_walk(it, c, [&](int64_t i) {
            const float g = y ? bn_masked(gy[i], y[i]) : gy[i];
            s1 += g;
            s2 += g * ((x[i] - mean) * invstd);
        });
        col_sum2(&s1, &s2, lds);
        col_put_part(part, w, s1, s2);
    }
}

template <bool kSingle>
__global__ __launch_bounds__(kBnThreads) void col_bwd_final_kernel(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ y,
                                                                   const float *__restrict__ gamma, const float *__restrict__ save_mean,
                                                                   const float *__restrict__ save_invstd, float *__restrict__ gx, float *__restrict__ ggamma,
                                                                   float *__restrict__ gbeta, const float *__restrict__ part, int n, int c, int tiles, int S,
                                                                   int batch_stats, int acc) {
    __shared__ float lds[512];
    const float fm = (float)n;
    for (int w = blockIdx.x; w < tiles * S; w += gridDim.x) {
        const ColItem it = col_item(w, S, n, c);
        const float mean = it.on ? save_mean[it.ch] : 0.0f, invstd = it.on ? save_invstd[it.ch] : 0.0f;
        float s1 = 0.0f, s2 = 0.0f;
        if (kSingle) {
            col_walk(it, c, [&](int64_t i) {
                const float g = y ? bn_masked(gy[i], y[i]) : gy[i];
                s1 += g;
                s2 += g * ((x[i] - mean) * invstd);
            });
        } else {
            col_fold(part, it, S, &s1, &s2);
        }
        col_sum2(&s1, &s2, lds);
        if (it.s == 0 && threadIdx.x < 64 && it.on) {
            gbeta[it.ch] = (acc & 4) ? gbeta[it.ch] + s1 : s1;
            ggamma[it.ch] = (acc & 2) ? ggamma[it.ch] + s2 : s2;
        }
        if (!gx) continue;
        const float a = it.on ? gamma[it.ch] * invstd : 0.0f;
        const float c1 = batch_stats ? s1 / fm : 0.0f, c2 = batch_stats ? s2 / fm : 0.0f;
        const bool add = (acc & 1) != 0;
        col_walk(it, c, [&](int64_t i) {
            const float g = y ? bn_masked(gy[i], y[i]) : gy[i];
            const float r = batch_stats ? a * (g - c1 - ((x[i] - mean) * invstd) * c2) : a * g;
            gx[i] = add ? gx[i] + r : r;
        });
    }
}

// shares of the rows of a column tile
static int col_split(int n, int tiles) {
    int64_t s = n / kColRowsMin;
    s = std::min<int64_t>(s, std::max(1, kBnGrid / tiles));
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, kBnMaxSplit));
}

// shares of a channel of m elements when there are c channels
static int bn_split(int64_t m, int c) {
    int64_t s = (m + kBnSplitMin - 1) / kBnSplitMin;
    s = std::min<int64_t>(s, std::max(1, kBnGrid / c));
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, kBnMaxSplit));
}
static int bn_grid(int c, int S) { return S > 1 ? c * S : std::min(c, 8 * kNumCU); }   // (S > 1: c * S <= kBnGrid)

static bool bn_vec(int hw, std::initializer_list<const void *> ptrs) {
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= (uintptr_t)p;
    return hw % 4 == 0 && (bits & 15) == 0;
}

}  // namespace th

using namespace th;

extern "C" {

int th_batchnorm2d_split(int n, int c, int hw) {
    if (!(n > 0 && c > 0 && hw > 0)) return 0;
    return hw == 1 ? col_split(n, ceil_div(c, kColTile)) : bn_split((int64_t)n * hw, c);
}

int th_batchnorm2d_fwd(th_ctx *ctx, const float *d_x, const float *d_gamma, const float *d_beta, float *d_y, float *d_running_mean,
                       float *d_running_var, float *d_save_mean, float *d_save_invstd, int n, int c, int hw, float eps, float momentum, int training,
                       int relu) {
    TH_REQUIRE(ctx && d_x && d_gamma && d_beta && d_y && d_running_mean && d_running_var && d_save_mean && d_save_invstd,
               "th_batchnorm2d_fwd: null argument");
    TH_REQUIRE(n > 0 && c > 0 && hw > 0, "th_batchnorm2d_fwd: n, c and hw must be positive (got %d, %d, %d)", n, c, hw);
    TH_REQUIRE((int64_t)n * hw < ((int64_t)1 << 31), "th_batchnorm2d_fwd: %lld elements per channel: fewer than 2^31 are supported", (long long)n * hw);
    TH_REQUIRE(std::isfinite(eps) && eps > 0.0f, "th_batchnorm2d_fwd: eps must be finite and positive (got %g)", (double)eps);
    TH_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "th_batchnorm2d_fwd: momentum must be in [0, 1] (got %g)", (double)momentum);
    const int64_t m = (int64_t)n * hw;
    TH_REQUIRE(!(training && m == 1), "th_batchnorm2d_fwd: Expected more than 1 value per channel when training");
    if (hw == 1) {   // the column form
        const int tiles = ceil_div(c, kColTile), S = col_split(n, tiles);
        const dim3 g(std::min(tiles * S, 8 * kNumCU)), b(kBnThreads);
        if (!training) {
            hipLaunchKernelGGL(col_fwd_eval_kernel, g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, n, c, tiles, S, eps, relu);
            TH_LAUNCH_CHECK();
            return 0;
        }
        if (S == 1) {
            hipLaunchKernelGGL(col_fwd_train_kernel<true>, g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, (const float *)nullptr, n, c, tiles, S, eps, momentum, relu);
            TH_LAUNCH_CHECK();
            return 0;
        }
        void *part = nullptr;
        if (th_malloc(ctx, (size_t)tiles * S * kColTile * 2 * sizeof(float), &part)) return 1;
        hipLaunchKernelGGL(col_fwd_parts_kernel, g, b, 0, ctx->stream, d_x, (float *)part, n, c, tiles, S);
        TH_LAUNCH_CHECK();
        hipLaunchKernelGGL(col_fwd_train_kernel<false>, g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, (const float *)part, n, c, tiles, S, eps, momentum, relu);
        TH_LAUNCH_CHECK();
        return th_free(ctx, part);
    }
    const int S = bn_split(m, c), grid = bn_grid(c, S);
    const bool vec = bn_vec(hw, {d_x, d_y});
    const dim3 g(grid), b(kBnThreads);
    if (!training) {
        if (vec) hipLaunchKernelGGL(bn_fwd_eval_kernel<float4>, g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, n, c, hw, S, eps, relu);
        else hipLaunchKernelGGL(bn_fwd_eval_kernel<float>, g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, n, c, hw, S, eps, relu);
        TH_LAUNCH_CHECK();
        return 0;
    }
    if (S == 1) {
        if (vec) hipLaunchKernelGGL((bn_fwd_train_kernel<float4, true>), g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, (const float *)nullptr, n, c, hw, S, eps, momentum, relu);
        else hipLaunchKernelGGL((bn_fwd_train_kernel<float, true>), g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, (const float *)nullptr, n, c, hw, S, eps, momentum, relu);
        TH_LAUNCH_CHECK();
        return 0;
    }
    void *part = nullptr;
    if (th_malloc(ctx, (size_t)c * S * 2 * sizeof(float), &part)) return 1;
    if (vec) hipLaunchKernelGGL(bn_fwd_parts_kernel<float4>, g, b, 0, ctx->stream, d_x, (float *)part, n, c, hw, S);
    else hipLaunchKernelGGL(bn_fwd_parts_kernel<float>, g, b, 0, ctx->stream, d_x, (float *)part, n, c, hw, S);
    TH_LAUNCH_CHECK();
    if (vec) hipLaunchKernelGGL((bn_fwd_train_kernel<float4, false>), g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, (const float *)part, n, c, hw, S, eps, momentum, relu);
    else hipLaunchKernelGGL((bn_fwd_train_kernel<float, false>), g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, (const float *)part, n, c, hw, S, eps, momentum, relu);
    TH_LAUNCH_CHECK();
    return th_free(ctx, part);
}

int th_batchnorm2d_bwd(th_ctx *ctx, const float *d_gy, const float *d_x, const float *d_y_or_null, const float *d_gamma, const float *d_save_mean,
                       const float *d_save_invstd, float *d_gx_or_null, float *d_ggamma, float *d_gbeta, int n, int c, int hw, int batch_stats,
                       int accumulate_mask) {
    TH_REQUIRE(ctx && d_gy && d_x && d_gamma && d_save_mean && d_save_invstd && d_ggamma && d_gbeta, "th_batchnorm2d_bwd: null argument");
    TH_REQUIRE(n > 0 && c > 0 && hw > 0, "th_batchnorm2d_bwd: n, c and hw must be positive (got %d, %d, %d)", n, c, hw);
    TH_REQUIRE((int64_t)n * hw < ((int64_t)1 << 31), "th_batchnorm2d_bwd: %lld elements per channel: fewer than 2^31 are supported", (long long)n * hw);
    TH_REQUIRE((accumulate_mask & ~7) == 0, "th_batchnorm2d_bwd: accumulate_mask has bits 0 (gx), 1 (ggamma) and 2 (gbeta) (got %d)", accumulate_mask);
    if (hw == 1) {   // the column form
        const int tiles = ceil_div(c, kColTile), S = col_split(n, tiles);
        const dim3 g(std::min(tiles * S, 8 * kNumCU)), b(kBnThreads);
        if (S == 1) {
            hipLaunchKernelGGL(col_bwd_final_kernel<true>, g, b, 0, ctx->stream, d_gy, d_x, d_y_or_null, d_gamma, d_save_mean, d_save_invstd, d_gx_or_null, d_ggamma, d_gbeta, (const float *)nullptr, n, c, tiles, S, batch_stats, accumulate_mask);
            TH_LAUNCH_CHECK();
            return 0;
        }
        void *part = nullptr;
        if (th_malloc(ctx, (size_t)tiles * S * kColTile * 2 * sizeof(float), &part)) return 1;
        hipLaunchKernelGGL(col_bwd_parts_kernel, g, b, 0, ctx->stream, d_gy, d_x, d_y_or_null, d_save_mean, d_save_invstd, (float *)part, n, c, tiles, S);
        TH_LAUNCH_CHECK();
        hipLaunchKernelGGL(col_bwd_final_kernel<false>, g, b, 0, ctx->stream, d_gy, d_x, d_y_or_null, d_gamma, d_save_mean, d_save_invstd, d_gx_or_null, d_ggamma, d_gbeta, (const float *)part, n, c, tiles, S, batch_stats, accumulate_mask);
        TH_LAUNCH_CHECK();
        return th_free(ctx, part);
    }
    const int S = bn_split((int64_t)n * hw, c), grid = bn_grid(c, S);
    const bool vec = bn_vec(hw, {d_gy, d_x, d_y_or_null, d_gx_or_null}), mask = d_y_or_null != nullptr;
    const dim3 g(grid), b(kBnThreads);
#define BN_BWD_LAUNCH(kernel, single, ...)                                                                                         \
    do {                                                                                                                           \
        if (vec && mask) hipLaunchKernelGGL((kernel<float4, single, true>), g, b, 0, ctx->stream, __VA_ARGS__);                    \
        else if (vec) hipLaunchKernelGGL((kernel<float4, single, false>), g, b, 0, ctx->stream, __VA_ARGS__);                      \
        else if (mask) hipLaunchKernelGGL((kernel<float, single, true>), g, b, 0, ctx->stream, __VA_ARGS__);                       \
        else hipLaunchKernelGGL((kernel<float, single, false>), g, b, 0, ctx->stream, __VA_ARGS__);                                \
        TH_LAUNCH_CHECK();                                                                                                         \
    } while (0)
    if (S == 1) {
        BN_BWD_LAUNCH(bn_bwd_final_kernel, true, d_gy, d_x, d_y_or_null, d_gamma, d_save_mean, d_save_invstd, d_gx_or_null, d_ggamma, d_gbeta, (const float *)nullptr, n, c, hw, S, batch_stats, accumulate_mask);
        return 0;
    }
    void *part = nullptr;
    if (th_malloc(ctx, (size_t)c * S * 2 * sizeof(float), &part)) return 1;
    if (vec && mask) hipLaunchKernelGGL((bn_bwd_parts_kernel<float4, true>), g, b, 0, ctx->stream, d_gy, d_x, d_y_or_null, d_save_mean, d_save_invstd, (float *)part, n, c, hw, S);
    else if (vec) hipLaunchKernelGGL((bn_bwd_parts_kernel<float4, false>), g, b, 0, ctx->stream, d_gy, d_x, d_y_or_null, d_save_mean, d_save_invstd, (float *)part, n, c, hw, S);
    else if (mask) hipLaunchKernelGGL((bn_bwd_parts_kernel<float, true>), g, b, 0, ctx->stream, d_gy, d_x, d_y_or_null, d_save_mean, d_save_invstd, (float *)part, n, c, hw, S);
    else hipLaunchKernelGGL((bn_bwd_parts_kernel<float, false>), g, b, 0, ctx->stream, d_gy, d_x, d_y_or_null, d_save_mean, d_save_invstd, (float *)part, n, c, hw, S);
    TH_LAUNCH_CHECK();
    // (without a map the second launch only folds: one workgroup per channel would do, the items s > 0 leave at once)
    BN_BWD_LAUNCH(bn_bwd_final_kernel, false, d_gy, d_x, d_y_or_null, d_gamma, d_save_mean, d_save_invstd, d_gx_or_null, d_ggamma, d_gbeta, (const float *)part, n, c, hw, S, batch_stats, accumulate_mask);
    return th_free(ctx, part);
#undef BN_BWD_LAUNCH
}

}  // extern "C"
