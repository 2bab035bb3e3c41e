// batchnorm.hip -- BatchNorm2d over an NCHW map, batch statistics on the device (torch.nn.BatchNorm2d's semantics: upstream announces the
// layer in nn.rs:829-857 and never writes it):
//
//   th_batchnorm2d_fwd   training: per-channel mean / biased variance over the M = n * hw elements of a channel, the running update
//                        (unbiased variance) and y = (x - mean) * (invstd * gamma) + beta [+ ReLU]; eval: the same map on the running pair
//   th_batchnorm2d_bwd   gbeta = sum gy, ggamma = sum gy * xh, gx = gamma * invstd * (gy - gbeta / M - xh * ggamma / M)
//   th_bn_residual_fwd   the same forward with a skip connection added in the map: y = ((x - mean) * a + b) + r [+ ReLU, after the add]
//   th_bn_residual_bwd   the same backward, whose map pass also writes the residual's gradient gr = gy (masked by y > 0 with the ReLU)
//
// One set of kernels over two geometries.  The five kernel templates (fwd_parts, fwd_train, fwd_eval, bwd_parts, bwd_final) hold the
// passes and every per-channel formula once; a GEOMETRY says which elements a workgroup's lanes own and how their sums meet:
//
//   PlaneGeo<V>  hw > 1.  Channel ch owns the planes (b * c + ch) * hw, b < n, walked in UNITS of V: float4s when hw % 4 == 0 and every
//                pointer is 16-byte aligned (then every plane base is), single floats otherwise.  Unit u of a channel is unit u % upp of
//                plane u / upp (upp = units per plane); a lane keeps {plane, offset} and advances both by the workgroup's stride without
//                a division, so a workgroup's 256 lanes stay busy whatever hw is.  A workgroup is one channel; an item is a share of the
//                channel's units; the sums of the 256 lanes meet in a butterfly and 8 floats of LDS.
//   ColGeo       hw == 1.  x is [n][c]: a channel is a column, neighbouring channels are neighbouring floats.  A workgroup takes a tile of
//                64 channels, one per lane (a wave's load is 256 contiguous bytes), its four waves the rows r0 + wave, + 4, ...; an item
//                is a share of the tile's rows; the sums of the four waves meet per lane in 512 floats of LDS.
//
// Work items.  A channel's units (a tile's rows) are cut into S contiguous shares (bn_plan: at least kBnSplitMin elements or kColRowsMin
// rows each, at most kBnGrid items in all, S <= 256); item w = group * S + s, a workgroup takes the items w = blockIdx.x, + gridDim.x, ...
//
// Passes.  S > 1: two launches each way -- per-item partial sums {s1, s2} into a pooled block, then every item folds its group's S
// partials itself (the same fixed order in every workgroup: no hand-off between workgroups, no atomics) and maps its share; item s = 0
// also writes the per-channel outputs (saved statistics and the running update; ggamma / gbeta).  S == 1: ONE launch, the workgroup sums
// its share and reads it a second time for the map, out of L2.  Eval: one launch.  bn_run is that ladder, once.
//
// The residual (kRes) is a template parameter of the three kernels that hold a map (fwd_train, fwd_eval, bwd_final); every statement it
// adds stands under `if constexpr`, so the plain instances are the kernels they were.  The sums do not involve the residual: fwd_parts
// and bwd_parts serve both.
//
// Numerics.  The sums of the forward are taken of x - K, K = the channel's first element, the same in every workgroup:
// mean = K + s1 / M, var = (s2 - s1 * s1 / M) / M -- the cancellation is that of a channel centred within its own spread, whatever
// |mean| / std is, and a constant channel gives mean = K exactly and var = 0 exactly.  Every sum has one order, bit-identical from run
// to run (tests/golden/batchnorm_bits.npz pins it): lane-local adds in walk order, (x + y) + (z + w) inside a float4; planes: a 64-lane
// butterfly, then (w0 + w1) + (w2 + w3) over the waves; columns: (w0 + w1) + (w2 + w3) per lane, the fold of S partials by wave
// k = wave, wave + 4, ... first.
#include "common.h"
#include "stream_dev.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <type_traits>

namespace th {

constexpr int kBnThreads = kStreamThreads;
constexpr int kBnMaxSplit = 256;           // shares of a channel at most: one lane of the plane fold each
constexpr int64_t kBnSplitMin = 4096;      // elements of a plane share at least (16 KiB: 4 float4s per lane)
constexpr int kBnGrid = 2048;              // work items at most when channels are split (8 per CU)
constexpr int kColTile = 64;               // channels of a column tile
constexpr int kColRowsMin = 32;            // rows of a column share at least (8 per wave: two trips of four loads in flight)

// what every kernel is told of the tensor and its plan (bn_plan)
struct BnDims {
    int n, c, hw, S, items;
};

__device__ __forceinline__ float hsum(float a) { return a; }
__device__ __forceinline__ float hsum(const float4 &a) { return (a.x + a.y) + (a.z + a.w); }

// share s of S of `total`: [*lo, *hi), the first total % S shares hold one more
__device__ __forceinline__ void bn_share(unsigned total, int S, int s_, unsigned *lo, unsigned *hi) {
    const unsigned q = total / (unsigned)S, r = total - q * (unsigned)S, s = (unsigned)s_;
    *lo = s * q + (s < r ? s : r);
    *hi = *lo + q + (s < r ? 1u : 0u);
}

// ---- the plane geometry ----
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

template <class V>
struct PlaneGeo {
    using Unit = V;
    using Cursor = BnCursor;
    static constexpr int kLds = 8;
    static constexpr bool kPrefetch = true;   // the split second launch asks for its first trip ahead of the fold
    struct Item {
        int ch, s;
        unsigned u0, u1;
    };
    struct Trip {   // four units asked for ahead of the walk (pre: this lane has a whole trip)
        bool pre;
        int64_t i0, i1, i2, i3;
    };
    int c, hw, S, upp, n_items;
    unsigned units;

    __device__ __forceinline__ explicit PlaneGeo(const BnDims &d)
        : c(d.c), hw(d.hw), S(d.S), upp(d.hw / (int)(sizeof(V) / sizeof(float))), n_items(d.items), units((unsigned)d.n * (unsigned)upp) {}
    __device__ __forceinline__ int items() const { return n_items; }
    __device__ __forceinline__ Item item(int w) const {
        Item it;
        it.ch = w / S;
        it.s = w - it.ch * S;
        bn_share(units, S, it.s, &it.u0, &it.u1);
        return it;
    }
    __device__ __forceinline__ bool on(const Item &) const { return true; }
    __device__ __forceinline__ bool lead(const Item &it) const { return it.s == 0 && threadIdx.x == 0; }
    // the shift of a channel's sums: the channel's first element (one uniform load; every workgroup of the channel takes the same)
    __device__ __forceinline__ float shift(const float *__restrict__ x, const Item &it) const { return x[(int64_t)it.ch * hw]; }
    __device__ __forceinline__ Cursor cursor(const Item &it) const { return BnCursor(it.u0, it.u1, upp, c, it.ch); }
    // use(i) for the rest of a cursor; four units per trip so that their loads are in flight together
    template <class Use>
    __device__ __forceinline__ void walk(Cursor cur, Use use) const {
        while (cur.more(3)) {
            const int64_t i0 = cur.next(), i1 = cur.next(), i2 = cur.next(), i3 = cur.next();
            use(i0);
            use(i1);
            use(i2);
            use(i3);
        }
        while (cur.more()) use(cur.next());
    }
    // (lanes without a whole trip get the channel's first unit four times: they load it without a branch and drop it)
    __device__ __forceinline__ Trip trip(Cursor &cur, const Item &it, bool want) const {
        Trip t;
        t.pre = want && cur.more(3);
        t.i0 = t.i1 = t.i2 = t.i3 = (int64_t)it.ch * upp;
        if (t.pre) t.i0 = cur.next(), t.i1 = cur.next(), t.i2 = cur.next(), t.i3 = cur.next();
        return t;
    }
    __device__ __forceinline__ void sum2(float *a, float *b, float *lds) const { block_sum2(a, b, lds); }
    // lane t < S asks for partial t of the channel (every lane loads, lanes past S a partial they drop: no branch, so the wait in front
    // of the fold can count and leaves the younger loads of the trip out)
    __device__ __forceinline__ void load_parts(const float *__restrict__ part, const Item &it, float *s1, float *s2) const {
        const int t = (int)threadIdx.x < S ? (int)threadIdx.x : S - 1;
        const float2 p = *reinterpret_cast<const float2 *>(part + 2 * ((int64_t)it.ch * S + t));
        *s1 = (int)threadIdx.x < S ? p.x : 0.0f;
        *s2 = (int)threadIdx.x < S ? p.y : 0.0f;
    }
    __device__ __forceinline__ void put_part(float *__restrict__ part, int w, float s1, float s2) const {
        if (threadIdx.x == 0) {
            part[2 * (int64_t)w] = s1;
            part[2 * (int64_t)w + 1] = s2;
        }
    }
};

// ---- the column geometry ----
struct ColGeo {
    using Unit = float;
    static constexpr int kLds = 512;
    static constexpr bool kPrefetch = false;
    struct Item {
        int tile, s, ch;
        unsigned r0, r1;
        bool on;   // this lane's channel exists
    };
    using Cursor = Item;
    struct Trip {   // no trip ahead of the fold
        static constexpr bool pre = false;
        static constexpr int64_t i0 = 0, i1 = 0, i2 = 0, i3 = 0;
    };
    int n, c, S, n_items;

    __device__ __forceinline__ explicit ColGeo(const BnDims &d) : n(d.n), c(d.c), S(d.S), n_items(d.items) {}
    __device__ __forceinline__ int items() const { return n_items; }
    __device__ __forceinline__ Item item(int w) const {
        Item it;
        it.tile = w / S;
        it.s = w - it.tile * S;
        it.ch = it.tile * kColTile + (threadIdx.x & 63);
        it.on = it.ch < c;
        bn_share((unsigned)n, S, it.s, &it.r0, &it.r1);
        return it;
    }
    __device__ __forceinline__ bool on(const Item &it) const { return it.on; }
    __device__ __forceinline__ bool lead(const Item &it) const { return it.s == 0 && threadIdx.x < 64 && it.on; }
    // the shift of a channel: its first row's element
    __device__ __forceinline__ float shift(const float *__restrict__ x, const Item &it) const { return it.on ? x[it.ch] : 0.0f; }
    __device__ __forceinline__ const Cursor &cursor(const Item &it) const { return it; }
    // use(i) for this lane's rows of [r0, r1), i = the element's index; four rows per trip
    template <class Use>
    __device__ __forceinline__ void walk(const Cursor &it, Use use) const {
        if (!it.on) return;
        int r = (int)it.r0 + (threadIdx.x >> 6);
        for (; r + 12 < (int)it.r1; r += 16) {
            const int64_t i = (int64_t)r * c + it.ch;
            use(i);
            use(i + 4 * (int64_t)c);
            use(i + 8 * (int64_t)c);
            use(i + 12 * (int64_t)c);
        }
        for (; r < (int)it.r1; r += 4) use((int64_t)r * c + it.ch);
    }
    __device__ __forceinline__ Trip trip(const Cursor &, const Item &, bool) const { return Trip(); }
    // every wave leaves with the four waves' sums per lane (s: 2 * 4 * 64 floats of LDS; the trailing barrier frees it)
    __device__ __forceinline__ void sum2(float *a, float *b, float *s) const {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        s[wave * 64 + lane] = *a;
        s[256 + wave * 64 + lane] = *b;
        lds_barrier();
        *a = (s[lane] + s[64 + lane]) + (s[128 + lane] + s[192 + lane]);
        *b = (s[256 + lane] + s[320 + lane]) + (s[384 + lane] + s[448 + lane]);
        lds_barrier();
    }
    // partials are [item][lane]{s1, s2}; a wave folds the tile's partials k = wave, + 4, ... and sum2 does the rest
    __device__ __forceinline__ void load_parts(const float *__restrict__ part, const Item &it, float *s1, float *s2) const {
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
    __device__ __forceinline__ void put_part(float *__restrict__ part, int w, float s1, float s2) const {
        if (threadIdx.x < 64) {
            const int64_t p = 2 * ((int64_t)w * kColTile + threadIdx.x);
            part[p] = s1;
            part[p + 1] = s2;
        }
    }
};

// ---- the per-channel formulas, once each ----
// y of x: max((v - mean) * a + b, floor)
struct BnAffine {
    float mean, a, b, floor_;
    __device__ __forceinline__ BnAffine(float mean_, float a_, float b_, int relu) : mean(mean_), a(a_), b(b_), floor_(relu ? 0.0f : -INFINITY) {}
    __device__ __forceinline__ float operator()(float v) const { return fmaxf((v - mean) * a + b, floor_); }
    // with a residual: the plain map's value (before its floor), then the add, then the floor -- each rounded once, in this order
    __device__ __forceinline__ float operator()(float v, float r) const { return fmaxf(((v - mean) * a + b) + r, floor_); }
};

// the batch statistics of a channel from its shifted sums; the lead lane saves them and updates the running pair
__device__ __forceinline__ void bn_batch_stats(bool lead, int ch, float k, float s1, float s2, float fm, float eps, float momentum,
                                               float *__restrict__ running_mean, float *__restrict__ running_var, float *__restrict__ save_mean,
                                               float *__restrict__ save_invstd, float *mean_out, float *invstd_out) {
    const float d = s1 / fm;
    const float mean = k + d;
    const float var = fmaxf((s2 - s1 * d) / fm, 0.0f);
    const float invstd = __fdiv_rn(1.0f, __fsqrt_rn(var + eps));
    if (lead) {
        save_mean[ch] = mean;
        save_invstd[ch] = invstd;
        running_mean[ch] = (1.0f - momentum) * running_mean[ch] + momentum * mean;
        running_var[ch] = (1.0f - momentum) * running_var[ch] + momentum * (var * (fm / (fm - 1.0f)));
    }
    *mean_out = mean;
    *invstd_out = invstd;
}

// the statistics of eval mode: the running pair, which the lead lane saves for the backward
__device__ __forceinline__ void bn_running_stats(bool lead, int ch, float eps, const float *__restrict__ running_mean,
                                                 const float *__restrict__ running_var, float *__restrict__ save_mean, float *__restrict__ save_invstd,
                                                 float *mean_out, float *invstd_out) {
    const float mean = running_mean[ch];
    const float invstd = __fdiv_rn(1.0f, __fsqrt_rn(running_var[ch] + eps));
    if (lead) {
        save_mean[ch] = mean;
        save_invstd[ch] = invstd;
    }
    *mean_out = mean;
    *invstd_out = invstd;
}

// gy with the fused ReLU's mask (ops.rs:358-369: a gradient is kept where the output is > 0)
template <class V, bool kMask>
__device__ __forceinline__ V bn_gy(const float *__restrict__ gy, const float *__restrict__ y, int64_t i) {
    const V g = at<V>(gy, i);
    if constexpr (kMask) return vmap([](float gv, float yv) { return yv > 0.0f ? gv : 0.0f; }, g, at<V>(y, i));
    else return g;
}

// ggamma / gbeta of a channel, over what is there when their bit of acc is set (bit 0 gx, 1 ggamma, 2 gbeta)
__device__ __forceinline__ void bn_put_grads(int ch, int acc, float s1, float s2, float *__restrict__ ggamma, float *__restrict__ gbeta) {
    gbeta[ch] = (acc & 4) ? gbeta[ch] + s1 : s1;
    ggamma[ch] = (acc & 2) ? ggamma[ch] + s2 : s2;
}

// this lane's sums of x - k and (x - k)^2 over a cursor
template <class G>
__device__ __forceinline__ void fwd_sums(const G &g, const float *__restrict__ x, const typename G::Cursor &cur, float k, float *s1, float *s2) {
    using V = typename G::Unit;
    float a = 0.0f, b = 0.0f;
    g.walk(cur, [&](int64_t i) {
        const V d = vmap([k](float v) { return v - k; }, at<V>(x, i));
        a += hsum(d);
        b += hsum(vmap([](float v) { return v * v; }, d));
    });
    *s1 = a;
    *s2 = b;
}

// this lane's sums of gy and gy * xh over a cursor
template <class G, bool kMask>
__device__ __forceinline__ void bwd_sums(const G &g, const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ y,
                                         const typename G::Cursor &cur, float mean, float invstd, float *s1, float *s2) {
    using V = typename G::Unit;
    float a = 0.0f, b = 0.0f;
    g.walk(cur, [&](int64_t i) {
        const V gv = bn_gy<V, kMask>(gy, y, i);
        a += hsum(gv);
        b += hsum(vmap([=](float gs, float xv) { return gs * ((xv - mean) * invstd); }, gv, at<V>(x, i)));
    });
    *s1 = a;
    *s2 = b;
}

// ---- forward ----
// first launch of a split forward: the partial of item w = sum (x - K), sum (x - K)^2 over its share
template <class G>
__global__ __launch_bounds__(kBnThreads) void fwd_parts(const float *__restrict__ x, float *__restrict__ part, BnDims d) {
    __shared__ float lds[G::kLds];
    const G g(d);
    for (int w = blockIdx.x; w < g.items(); w += gridDim.x) {
        const auto it = g.item(w);
        float s1, s2;
        fwd_sums(g, x, g.cursor(it), g.shift(x, it), &s1, &s2);
        g.sum2(&s1, &s2, lds);
        g.put_part(part, w, s1, s2);
    }
}

// y of a unit: f(x), or f(x, r) with the residual
template <class V, bool kRes>
__device__ __forceinline__ V bn_y(const BnAffine &f, const V &v, const V &r) {
    if constexpr (kRes) return vmap(f, v, r);
    else return vmap(f, v);
}

// the training forward's statistics, running update and map.  kSingle: S == 1, the sums are taken here (part unused).  kRes: res is added
// in the map (null otherwise)
template <class G, bool kSingle, bool kRes>
__global__ __launch_bounds__(kBnThreads) void fwd_train(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                        float *__restrict__ y, float *__restrict__ running_mean, float *__restrict__ running_var,
                                                        float *__restrict__ save_mean, float *__restrict__ save_invstd, const float *__restrict__ part,
                                                        BnDims d, float eps, float momentum, int relu, const float *__restrict__ res) {
    using V = typename G::Unit;
    __shared__ float lds[G::kLds];
    const G g(d);
    const float fm = (float)((int64_t)d.n * d.hw);
    for (int w = blockIdx.x; w < g.items(); w += gridDim.x) {
        const auto it = g.item(w);
        const float k = g.shift(x, it);
        // the split form asks for its partials, then (planes) for its first trip, and folds while the trip's loads fly (the partials come
        // back first: the wait in front of the fold leaves the four younger loads out)
        float s1 = 0.0f, s2 = 0.0f;
        if constexpr (!kSingle) g.load_parts(part, it, &s1, &s2);
        auto cur = g.cursor(it);
        const auto t = g.trip(cur, it, !kSingle);
        V v0 = V(), v1 = V(), v2 = V(), v3 = V();
        if constexpr (!kSingle && G::kPrefetch) v0 = at<V>(x, t.i0), v1 = at<V>(x, t.i1), v2 = at<V>(x, t.i2), v3 = at<V>(x, t.i3);
        // (the residual's trip the same way, unbranched and younger than the partials: the wait in front of the fold counts eight loads out)
        V r0 = V(), r1 = V(), r2 = V(), r3 = V();
        if constexpr (kRes && !kSingle && G::kPrefetch) r0 = at<V>(res, t.i0), r1 = at<V>(res, t.i1), r2 = at<V>(res, t.i2), r3 = at<V>(res, t.i3);
        if constexpr (kSingle) fwd_sums(g, x, cur, k, &s1, &s2);
        g.sum2(&s1, &s2, lds);
        float mean, invstd;
        bn_batch_stats(g.lead(it), it.ch, k, s1, s2, fm, eps, momentum, running_mean, running_var, save_mean, save_invstd, &mean, &invstd);
        const BnAffine f(mean, g.on(it) ? invstd * gamma[it.ch] : 0.0f, g.on(it) ? beta[it.ch] : 0.0f, relu);
        if (t.pre) {
            put(y, t.i0, bn_y<V, kRes>(f, v0, r0));
            put(y, t.i1, bn_y<V, kRes>(f, v1, r1));
            put(y, t.i2, bn_y<V, kRes>(f, v2, r2));
            put(y, t.i3, bn_y<V, kRes>(f, v3, r3));
        }
        g.walk(cur, [&](int64_t i) {
            if constexpr (kRes) put(y, i, vmap(f, at<V>(x, i), at<V>(res, i)));
            else put(y, i, vmap(f, at<V>(x, i)));
        });
    }
}

template <class G, bool kRes>
__global__ __launch_bounds__(kBnThreads) void fwd_eval(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       float *__restrict__ y, const float *__restrict__ running_mean,
                                                       const float *__restrict__ running_var, float *__restrict__ save_mean,
                                                       float *__restrict__ save_invstd, BnDims d, float eps, int relu,
                                                       const float *__restrict__ res) {
    using V = typename G::Unit;
    const G g(d);
    for (int w = blockIdx.x; w < g.items(); w += gridDim.x) {
        const auto it = g.item(w);
        if (!g.on(it)) continue;
        float mean, invstd;
        bn_running_stats(g.lead(it), it.ch, eps, running_mean, running_var, save_mean, save_invstd, &mean, &invstd);
        const BnAffine f(mean, invstd * gamma[it.ch], beta[it.ch], relu);
        g.walk(g.cursor(it), [&](int64_t i) {
            if constexpr (kRes) put(y, i, vmap(f, at<V>(x, i), at<V>(res, i)));
            else put(y, i, vmap(f, at<V>(x, i)));
        });
    }
}

// ---- backward ----
// first launch of a split backward: the partial of item w = sum gy, sum gy * xh over its share
template <class G, bool kMask>
__global__ __launch_bounds__(kBnThreads) void bwd_parts(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ y,
                                                        const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
                                                        float *__restrict__ part, BnDims d) {
    __shared__ float lds[G::kLds];
    const G g(d);
    for (int w = blockIdx.x; w < g.items(); w += gridDim.x) {
        const auto it = g.item(w);
        const float mean = g.on(it) ? save_mean[it.ch] : 0.0f, invstd = g.on(it) ? save_invstd[it.ch] : 0.0f;
        float s1, s2;
        bwd_sums<G, kMask>(g, gy, x, y, g.cursor(it), mean, invstd, &s1, &s2);
        g.sum2(&s1, &s2, lds);
        g.put_part(part, w, s1, s2);
    }
}

// the channel sums (kSingle: taken here), ggamma / gbeta by item s = 0, and the map unless gx is null.  acc: bit 0 gx, 1 ggamma, 2 gbeta.
// kRes: the map also writes gr = the masked gy (acc bit 3: += into gr), and runs for gr alone when gx is null
template <class G, bool kSingle, bool kMask, bool kRes>
__global__ __launch_bounds__(kBnThreads) void bwd_final(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ y,
                                                        const float *__restrict__ gamma, const float *__restrict__ save_mean,
                                                        const float *__restrict__ save_invstd, float *__restrict__ gx, float *__restrict__ ggamma,
                                                        float *__restrict__ gbeta, const float *__restrict__ part, BnDims d, int batch_stats, int acc,
                                                        float *__restrict__ gr) {
    using V = typename G::Unit;
    __shared__ float lds[G::kLds];
    const G g(d);
    const float fm = (float)((int64_t)d.n * d.hw);
    for (int w = blockIdx.x; w < g.items(); w += gridDim.x) {
        const auto it = g.item(w);
        const float mean = g.on(it) ? save_mean[it.ch] : 0.0f, invstd = g.on(it) ? save_invstd[it.ch] : 0.0f;
        // (as in the forward: the split form asks for its partials, then for its first trip, and folds while that trip's loads fly)
        float s1 = 0.0f, s2 = 0.0f;
        if constexpr (!kSingle) g.load_parts(part, it, &s1, &s2);
        auto cur = g.cursor(it);
        const auto t = g.trip(cur, it, !kSingle && (kRes || gx));
        V g0 = V(), g1 = V(), g2 = V(), g3 = V(), x0 = V(), x1 = V(), x2 = V(), x3 = V();
        if constexpr (!kSingle && G::kPrefetch) {
            g0 = bn_gy<V, kMask>(gy, y, t.i0), g1 = bn_gy<V, kMask>(gy, y, t.i1), g2 = bn_gy<V, kMask>(gy, y, t.i2), g3 = bn_gy<V, kMask>(gy, y, t.i3);
            x0 = at<V>(x, t.i0), x1 = at<V>(x, t.i1), x2 = at<V>(x, t.i2), x3 = at<V>(x, t.i3);
        }
        if constexpr (kSingle) bwd_sums<G, kMask>(g, gy, x, y, cur, mean, invstd, &s1, &s2);
        g.sum2(&s1, &s2, lds);
        if (g.lead(it)) bn_put_grads(it.ch, acc, s1, s2, ggamma, gbeta);
        if constexpr (!kRes) {
            if (!gx) continue;
        }
        // gx of gy and x: a * (g - c1 - xh * c2) with the batch's statistics, a * g with the running pair; added to what is there on bit 0
        const float a = g.on(it) ? gamma[it.ch] * invstd : 0.0f;
        const float c1 = batch_stats ? s1 / fm : 0.0f, c2 = batch_stats ? s2 / fm : 0.0f;
        const bool add = (acc & 1) != 0;
        auto emit = [&](int64_t i, const V &gv, const V &xv) {
            if constexpr (kRes) {   // the residual's gradient is the masked gy, which sits in a register here
                put(gr, i, (acc & 8) ? vmap([](float gs, float old) { return old + gs; }, gv, at<V>(gr, i)) : gv);
                if (!gx) return;
            }
            V r = batch_stats ? vmap([=](float gs, float xe) { return a * (gs - c1 - ((xe - mean) * invstd) * c2); }, gv, xv)
                              : vmap([=](float gs) { return a * gs; }, gv);
            if (add) r = vmap([](float rv, float old) { return old + rv; }, r, at<V>(gx, i));
            put(gx, i, r);
        };
        if (t.pre) {
            emit(t.i0, g0, x0);
            emit(t.i1, g1, x1);
            emit(t.i2, g2, x2);
            emit(t.i3, g3, x3);
        }
        g.walk(cur, [&](int64_t i) { emit(i, bn_gy<V, kMask>(gy, y, i), at<V>(x, i)); });
    }
}

// ---- the plan and the launches ----
struct BnPlan {
    bool col, vec;       // the column form; float4 units (planes only)
    int S, grid;         // shares of a channel (of a tile's rows); workgroups
    size_t part_bytes;   // the partials block of a split pass
    BnDims dims;
};

// `ptrs`: every tensor the pass walks (null ones do not count)
static BnPlan bn_plan(int n, int c, int hw, std::initializer_list<const void *> ptrs) {
    BnPlan p;
    p.col = hw == 1;
    const int groups = p.col ? ceil_div(c, kColTile) : c;   // a workgroup's items belong to one group: a tile of channels, or a channel
    int64_t s = p.col ? n / kColRowsMin : ((int64_t)n * hw + kBnSplitMin - 1) / kBnSplitMin;
    s = std::min<int64_t>(s, std::max(1, kBnGrid / groups));
    p.S = (int)std::max<int64_t>(1, std::min<int64_t>(s, kBnMaxSplit));
    uintptr_t bits = 0;
    for (const void *q : ptrs) bits |= (uintptr_t)q;
    p.vec = !p.col && hw % 4 == 0 && (bits & 15) == 0;
    const int items = groups * p.S;
    p.grid = std::min(items, 8 * kNumCU);
    p.part_bytes = (size_t)items * (p.col ? kColTile : 1) * 2 * sizeof(float);
    p.dims = BnDims{n, c, hw, p.S, items};
    return p;
}

template <class G> struct BnGeoTag { using type = G; };

// f(geometry tag, std::bool_constant<mask>), chosen once
template <class F>
static int bn_dispatch(const BnPlan &p, bool mask, F f) {
    auto with_mask = [&](auto geo) { return mask ? f(geo, std::true_type()) : f(geo, std::false_type()); };
    if (p.col) return with_mask(BnGeoTag<ColGeo>());
    return p.vec ? with_mask(BnGeoTag<PlaneGeo<float4>>()) : with_mask(BnGeoTag<PlaneGeo<float>>());
}

// One pass from a plan.  split: parts(block) and then second(std::false_type, block) with a pooled partials block between them; otherwise
// second(std::true_type, null) alone
template <class Parts, class Second>
static int bn_run(th_ctx *ctx, const BnPlan &p, bool split, Parts parts, Second second) {
    if (!split) {
        second(std::true_type(), (const float *)nullptr);
        TH_LAUNCH_CHECK();
        return 0;
    }
    void *part = nullptr;
    if (th_malloc(ctx, p.part_bytes, &part)) return 1;
    parts((float *)part);
    TH_LAUNCH_CHECK();
    second(std::false_type(), (const float *)part);
    TH_LAUNCH_CHECK();
    return th_free(ctx, part);
}

// The launches of a forward whose arguments the entry point has checked.  kRes: d_residual is added in the map (null otherwise); it
// counts for the plan, so that an unaligned residual takes the scalar instance
template <bool kRes>
static int bn_forward(th_ctx *ctx, const float *d_x, const float *d_residual, const float *d_gamma, const float *d_beta, float *d_y,
                      float *d_running_mean, float *d_running_var, float *d_save_mean, float *d_save_invstd, int n, int c, int hw, float eps,
                      float momentum, int training, int relu) {
    const BnPlan p = bn_plan(n, c, hw, {d_x, d_y, d_residual});
    const dim3 g(p.grid), b(kBnThreads);
    return bn_dispatch(p, false, [&](auto geo, auto) {
        using G = typename decltype(geo)::type;
        return bn_run(
            ctx, p, training && p.S > 1, [&](float *part) { hipLaunchKernelGGL(fwd_parts<G>, g, b, 0, ctx->stream, d_x, part, p.dims); },
            [&](auto single, const float *part) {
                if (training)
                    hipLaunchKernelGGL((fwd_train<G, decltype(single)::value, kRes>), g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y,
                                       d_running_mean, d_running_var, d_save_mean, d_save_invstd, part, p.dims, eps, momentum, relu, d_residual);
                else
                    hipLaunchKernelGGL((fwd_eval<G, kRes>), g, b, 0, ctx->stream, d_x, d_gamma, d_beta, d_y, d_running_mean, d_running_var,
                                       d_save_mean, d_save_invstd, p.dims, eps, relu, d_residual);
            });
    });
}

// The launches of a checked backward.  kRes: d_gr gets the residual's gradient in the map pass (null otherwise)
template <bool kRes>
static int bn_backward(th_ctx *ctx, const float *d_gy, const float *d_x, const float *d_y_or_null, const float *d_gamma, const float *d_save_mean,
                       const float *d_save_invstd, float *d_gx_or_null, float *d_gr, float *d_ggamma, float *d_gbeta, int n, int c, int hw,
                       int batch_stats, int accumulate_mask) {
    const BnPlan p = bn_plan(n, c, hw, {d_gy, d_x, d_y_or_null, d_gx_or_null, d_gr});
    const dim3 g(p.grid), b(kBnThreads);
    return bn_dispatch(p, d_y_or_null != nullptr, [&](auto geo, auto mask) {
        using G = typename decltype(geo)::type;
        constexpr bool kMask = decltype(mask)::value;
        // (without a map the second launch only folds: one workgroup per channel would do, the items s > 0 leave at once)
        return bn_run(
            ctx, p, p.S > 1,
            [&](float *part) {
                hipLaunchKernelGGL((bwd_parts<G, kMask>), g, b, 0, ctx->stream, d_gy, d_x, d_y_or_null, d_save_mean, d_save_invstd, part, p.dims);
            },
            [&](auto single, const float *part) {
                hipLaunchKernelGGL((bwd_final<G, decltype(single)::value, kMask, kRes>), g, b, 0, ctx->stream, d_gy, d_x, d_y_or_null, d_gamma,
                                   d_save_mean, d_save_invstd, d_gx_or_null, d_ggamma, d_gbeta, part, p.dims, batch_stats, accumulate_mask, d_gr);
            });
    });
}

}  // namespace th

using namespace th;

extern "C" {

int th_batchnorm2d_split(int n, int c, int hw) {
    if (!(n > 0 && c > 0 && hw > 0)) return 0;
    return bn_plan(n, c, hw, {}).S;
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
    TH_REQUIRE(!(training && (int64_t)n * hw == 1), "th_batchnorm2d_fwd: Expected more than 1 value per channel when training");
    return bn_forward<false>(ctx, d_x, nullptr, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, n, c, hw, eps,
                             momentum, training, relu);
}

int th_bn_residual_fwd(th_ctx *ctx, const float *d_x, const float *d_residual, const float *d_gamma, const float *d_beta, float *d_y,
                       float *d_running_mean, float *d_running_var, float *d_save_mean, float *d_save_invstd, int n, int c, int hw, float eps,
                       float momentum, int training, int relu) {
    TH_REQUIRE(ctx && d_x && d_residual && d_gamma && d_beta && d_y && d_running_mean && d_running_var && d_save_mean && d_save_invstd,
               "th_bn_residual_fwd: null argument");
    TH_REQUIRE(d_residual != d_y, "th_bn_residual_fwd: d_residual may not be d_y (it is only read; it may be d_x)");
    TH_REQUIRE(n > 0 && c > 0 && hw > 0, "th_bn_residual_fwd: n, c and hw must be positive (got %d, %d, %d)", n, c, hw);
    TH_REQUIRE((int64_t)n * hw < ((int64_t)1 << 31), "th_bn_residual_fwd: %lld elements per channel: fewer than 2^31 are supported", (long long)n * hw);
    TH_REQUIRE(std::isfinite(eps) && eps > 0.0f, "th_bn_residual_fwd: eps must be finite and positive (got %g)", (double)eps);
    TH_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "th_bn_residual_fwd: momentum must be in [0, 1] (got %g)", (double)momentum);
    TH_REQUIRE(!(training && (int64_t)n * hw == 1), "th_bn_residual_fwd: Expected more than 1 value per channel when training");
    return bn_forward<true>(ctx, d_x, d_residual, d_gamma, d_beta, d_y, d_running_mean, d_running_var, d_save_mean, d_save_invstd, n, c, hw, eps,
                            momentum, training, relu);
}

int th_batchnorm2d_bwd(th_ctx *ctx, const float *d_gy, const float *d_x, const float *d_y_or_null, const float *d_gamma, const float *d_save_mean,
                       const float *d_save_invstd, float *d_gx_or_null, float *d_ggamma, float *d_gbeta, int n, int c, int hw, int batch_stats,
                       int accumulate_mask) {
    TH_REQUIRE(ctx && d_gy && d_x && d_gamma && d_save_mean && d_save_invstd && d_ggamma && d_gbeta, "th_batchnorm2d_bwd: null argument");
    TH_REQUIRE(n > 0 && c > 0 && hw > 0, "th_batchnorm2d_bwd: n, c and hw must be positive (got %d, %d, %d)", n, c, hw);
    TH_REQUIRE((int64_t)n * hw < ((int64_t)1 << 31), "th_batchnorm2d_bwd: %lld elements per channel: fewer than 2^31 are supported", (long long)n * hw);
    TH_REQUIRE((accumulate_mask & ~7) == 0, "th_batchnorm2d_bwd: accumulate_mask has bits 0 (gx), 1 (ggamma) and 2 (gbeta) (got %d)", accumulate_mask);
    return bn_backward<false>(ctx, d_gy, d_x, d_y_or_null, d_gamma, d_save_mean, d_save_invstd, d_gx_or_null, nullptr, d_ggamma, d_gbeta, n, c, hw,
                              batch_stats, accumulate_mask);
}

int th_bn_residual_bwd(th_ctx *ctx, const float *d_gy, const float *d_x, const float *d_y_or_null, const float *d_gamma, const float *d_save_mean,
                       const float *d_save_invstd, float *d_gx_or_null, float *d_gr, float *d_ggamma, float *d_gbeta, int n, int c, int hw,
                       int batch_stats, int accumulate_mask) {
    TH_REQUIRE(ctx && d_gy && d_x && d_gamma && d_save_mean && d_save_invstd && d_gr && d_ggamma && d_gbeta, "th_bn_residual_bwd: null argument");
    TH_REQUIRE(d_gr != d_gx_or_null, "th_bn_residual_bwd: d_gr may not be d_gx (two gradients, two buffers)");
    TH_REQUIRE(n > 0 && c > 0 && hw > 0, "th_bn_residual_bwd: n, c and hw must be positive (got %d, %d, %d)", n, c, hw);
    TH_REQUIRE((int64_t)n * hw < ((int64_t)1 << 31), "th_bn_residual_bwd: %lld elements per channel: fewer than 2^31 are supported", (long long)n * hw);
    TH_REQUIRE((accumulate_mask & ~15) == 0, "th_bn_residual_bwd: accumulate_mask has bits 0 (gx), 1 (ggamma), 2 (gbeta) and 3 (gr) (got %d)",
               accumulate_mask);
    return bn_backward<true>(ctx, d_gy, d_x, d_y_or_null, d_gamma, d_save_mean, d_save_invstd, d_gx_or_null, d_gr, d_ggamma, d_gbeta, n, c, hw,
                             batch_stats, accumulate_mask);
}

}  // extern "C"
