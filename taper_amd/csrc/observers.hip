// observers.hip -- the quantization observers' statistics (src/quantization/observers.rs), kept and updated on the device:
//
//   th_obs_minmax_first / _update   MinMaxObserver::observe: the per-element running min / max (the first observation copies the data
//                                   into both vectors, a later one folds the first min(m, len) elements in with f32::min / f32::max)
//   th_obs_fold                     global_min / global_max: the NaN-ignoring folds from +inf / -inf (infinities take part -- this is not
//                                   the finite-only min / max of fake_quant.hip); two floats leave the device, not the vectors
//   th_obs_hist_edges               HistogramObserver's first observation: min / max fold of the data, then the num_bins + 1 edges written
//                                   on the device with the reference's rounding order (one division, then a multiply and an add per edge)
//   th_obs_hist_count               the counting pass: one read of the tensor, nothing written but counters (4 bytes per element)
//   th_obs_hist_stats               total count, sum of i * count and the largest count, as three 64-bit integers
//
// The counting pass up to kObsLdsMaxBins bins keeps the edge table and 32-bit counters of a workgroup (one of 1 024 lanes per CU) in LDS.  A value's bin is the
// reference's linear scan (find_bin: the first edge with val <= edge, minus one, saturating; past the last edge and every NaN -> the last
// bin); when the edges are finite and non-decreasing -- every workgroup checks that while it loads them -- an arithmetic guess checked
// against the table (a binary search when the guess is not the bin) gives exactly the scan's answer.  Elements that fall into
// the bin a wave currently sees most (half of a post-ReLU tensor sits in bin 0) are counted with one ballot into a wave-uniform register
// and never reach the LDS; the rest are LDS integer adds.  The merge into the 64-bit global bins is integer atomics, non-zero counters
// only, each workgroup starting at a different bin: integer sums do not depend on the order of arrival, so the bins are bit-identical
// from run to run.  More bins than that, or edges that are not finite (an infinity or only NaNs in the first observation: the literal scan
// is the definition there): a second form with a search per element over the edges in global memory and atomics on the global bins.
#include "common.h"
#include "hist_dev.h"
#include "stream_dev.h"

namespace th {

constexpr int kObsThreads = kStreamThreads;
constexpr int kObsParts = 512;                     // workgroups of a fold's first pass (2 per CU)
constexpr int64_t kObsPartMin = 4 * 256 * 8;       // elements per fold workgroup at least
constexpr int kObsMapGrid = 2048;                  // workgroups of the element-wise passes at most (8 per CU)

constexpr int kHistGlobalGrid = 1024;              // (the LDS form's sizes: hist_dev.h)

// ---- MinMaxObserver::observe ----
__global__ __launch_bounds__(kObsThreads) void obs_minmax_first_kernel(const float *__restrict__ x, float *__restrict__ mn, float *__restrict__ mx, int64_t n) {
    span_walk<2>(aligned16(x, mn, mx), n, grid_t0(), grid_stride(), [=](int64_t j, const auto &a) {
        put(mn, j, a);
        put(mx, j, a);
    }, x);
}

// f32::min / f32::max: a NaN operand loses to a number (fminf / fmaxf); six loads in flight per lane
__global__ __launch_bounds__(kObsThreads) void obs_minmax_update_kernel(const float *__restrict__ x, float *__restrict__ mn, float *__restrict__ mx, int64_t n) {
    span_walk<2>(aligned16(x, mn, mx), n, grid_t0(), grid_stride(), [=](int64_t j, const auto &a, const auto &lo, const auto &hi) {
        put(mn, j, vmap([](float l, float v) { return fminf(l, v); }, lo, a));
        put(mx, j, vmap([](float h, float v) { return fmaxf(h, v); }, hi, a));
    }, x, mn, mx);
}

// ---- the NaN-ignoring folds (stream_dev.h's MinMaxNanIgnoring: min over a[0, n), max over b[0, n); a == b for a histogram's first observation) ----
__global__ __launch_bounds__(kObsThreads) void obs_fold_final_kernel(const float *__restrict__ part, int n_parts, float *__restrict__ out2) {
    __shared__ float s[8];
    float mn, mx;
    fold_parts(part, n_parts, &mn, &mx, s);
    if (threadIdx.x == 0) {
        out2[0] = mn;
        out2[1] = mx;
    }
}

// observers.rs:170-178: bin_width = (max - min) / num_bins as f32; edge[i] = min + i as f32 * bin_width -- every operation rounded once
__global__ __launch_bounds__(kObsThreads) void obs_edges_kernel(const float *__restrict__ part, int n_parts, int num_bins, float *__restrict__ edges) {
    __shared__ float s[8];
    float mn, mx;
    fold_parts(part, n_parts, &mn, &mx, s);
    const float width = __fdiv_rn(__fsub_rn(mx, mn), (float)num_bins);
    for (int i = threadIdx.x; i <= num_bins; i += kObsThreads) edges[i] = __fadd_rn(mn, __fmul_rn((float)i, width));
}

// ---- find_bin ----
// observers.rs:194-201 as written: the first edge with val <= edge, minus one (saturating); none (past the last edge, or a NaN) -> the last bin
__device__ __forceinline__ int obs_bin_scan(const float *__restrict__ e, int nb, float v) {
    for (int i = 0; i <= nb; ++i)
        if (v <= e[i]) return i > 0 ? i - 1 : 0;
    return nb - 1;
}

// the same answer by a search, for finite non-decreasing edges and a v that is not a NaN
__device__ __forceinline__ int obs_bin_search(const float *e, int nb, float v) {
    int lo = 0, hi = nb + 1;   // the first i in [0, nb] with v <= e[i], nb + 1 when there is none
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v <= e[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo > nb ? nb - 1 : (lo > 0 ? lo - 1 : 0);
}

// ... and by an arithmetic guess checked against a table in LDS: t[0] = -inf, t[i] = e[i] for 0 < i < nb, t[nb] = +inf.  The scan's bin
// is the one k in [0, nb) with t[k] < v <= t[k + 1] (bin 0 takes everything up to e[1], e[0] included; the last bin everything above
// e[nb - 1]); -inf, which no such k holds, and a NaN go to the search below, as does a wrong guess (an element next to an edge; runs
// of equal edges, where the width is below the edges' spacing).  inv = 1 / bin width (+inf for a zero width: everything above the
// edges guesses the last bin, everything else bin 0).
__device__ inline int obs_bin_table_search(const float *t, int nb, float v) {
    if (v != v) return nb - 1;
    int lo = 1, hi = nb;   // the first i in [1, nb] with v <= t[i] -- t[nb] = +inf: there is one -- minus one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v <= t[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
}
__device__ __forceinline__ int obs_bin_index(int nb, float v, float e0, float inv) {   // the guess, in [0, nb)
    return (int)fminf(fmaxf((v - e0) * inv, 0.0f), (float)(nb - 1));   // (fmaxf drops a NaN: that of v, or of 0 * inf)
}
__device__ __forceinline__ bool obs_bin_holds(const float *t, int k, float v) { return t[k] < v && v <= t[k + 1]; }
__device__ __forceinline__ int obs_bin_guess(const float *t, int nb, float v, float e0, float inv) {
    const int k = obs_bin_index(nb, v, e0, inv);
    return __builtin_expect(obs_bin_holds(t, k, v), 1) ? k : obs_bin_table_search(t, nb, v);
}

// the scan may be replaced iff no edge is NaN or infinite and they never decrease: all lanes leave with the verdict for e[0, nb]
__device__ __forceinline__ bool obs_edges_regular(const float *__restrict__ e, int nb) {
    int bad = 0;
    for (int i = threadIdx.x; i <= nb; i += blockDim.x) {
        const float a = e[i];
        bad |= !isfinite(a) || (i < nb && !(a <= e[i + 1]));
    }
    return __syncthreads_or(bad) == 0;
}

// ---- the counting pass, LDS form ----
// dynamic LDS: the nb + 1 entries of the table, then nb 32-bit counters.  A workgroup sees fewer than 2^32 elements (the host checks n).
__global__ __launch_bounds__(kHistThreads) void obs_hist_lds_kernel(const float *__restrict__ x, int64_t n, const float *__restrict__ edges, int nb,
                                                                   unsigned long long *__restrict__ bins) {
    extern __shared__ float lds[];
    float *e = lds;
    unsigned *cnt = (unsigned *)(lds + nb + 1);
    // the table t above and zeroed counters, and in the same pass over the edges the verdict of obs_edges_regular
    int bad = 0;
    for (int i = threadIdx.x; i <= nb; i += kHistThreads) {
        const float a = edges[i];
        bad |= !isfinite(a) || (i < nb && !(a <= edges[i + 1]));
        e[i] = i == 0 ? -INFINITY : (i == nb ? INFINITY : a);
    }
    for (int i = threadIdx.x; i < nb; i += kHistThreads) cnt[i] = 0u;
    if (__syncthreads_or(bad)) {   // (uniform over the grid: every workgroup reads the same edges) the literal scan, straight into the global bins
        for (int64_t i = (int64_t)blockIdx.x * kHistThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kHistThreads)
            atomicAdd(&bins[obs_bin_scan(edges, nb, x[i])], 1ull);
        return;
    }
    const float e0 = edges[0], span = edges[nb] - e0;
    const float inv = span > 0.0f ? (float)nb / span : INFINITY;

    // the wave's hot bin, the walk by whole waves and the merge are hist_dev.h's; the bin of a value is this pass's own
    HotBin hb{cnt};
    auto count = [&](float v, bool valid) {   // the loops of the ends: lanes past the end count nothing
        hb.count(valid ? obs_bin_guess(e, nb, v, e0, inv) : -1);
    };
    int last = 0;
    auto count4 = [&](float4 a) {   // the four bins first (their table reads overlap), then the counters
        int k0 = obs_bin_index(nb, a.x, e0, inv), k1 = obs_bin_index(nb, a.y, e0, inv);
        int k2 = obs_bin_index(nb, a.z, e0, inv), k3 = obs_bin_index(nb, a.w, e0, inv);
        const bool ok0 = obs_bin_holds(e, k0, a.x), ok1 = obs_bin_holds(e, k1, a.y), ok2 = obs_bin_holds(e, k2, a.z), ok3 = obs_bin_holds(e, k3, a.w);
        if (__builtin_expect(!(ok0 & ok1 & ok2 & ok3), 0)) {   // one branch for the four: the table reads above are in flight together
            if (!ok0) k0 = obs_bin_table_search(e, nb, a.x);
            if (!ok1) k1 = obs_bin_table_search(e, nb, a.y);
            if (!ok2) k2 = obs_bin_table_search(e, nb, a.z);
            if (!ok3) k3 = obs_bin_table_search(e, nb, a.w);
        }
        hb.tally(k0); hb.tally(k1); hb.tally(k2); hb.tally(k3);
        last = k3;
    };
    hist_wave_walk(x, n, count4, [&] { hb.retarget(last, 16 * 64); }, count);
    hb.flush();
    __syncthreads();
    hist_merge(cnt, nb, bins);
}

// ---- the counting pass, global form: any number of bins ----
__global__ __launch_bounds__(kObsThreads) void obs_hist_global_kernel(const float *__restrict__ x, int64_t n, const float *__restrict__ edges, int nb,
                                                                     unsigned long long *__restrict__ bins) {
    const bool regular = obs_edges_regular(edges, nb);
    const int lane = threadIdx.x & 63;
    for (int64_t iw = (int64_t)blockIdx.x * kObsThreads + threadIdx.x - lane; iw < n; iw += (int64_t)gridDim.x * kObsThreads) {   // by whole waves
        const int64_t i = iw + lane;
        int k = -1;
        if (i < n) {
            const float v = x[i];
            k = !regular ? obs_bin_scan(edges, nb, v) : (v != v ? nb - 1 : obs_bin_search(edges, nb, v));
        }
        // one atomic per distinct bin of the wave: the lanes of a bin elect their first, which adds their number
        unsigned long long rest = __ballot(k >= 0);
        while (rest) {
            const int first = __ffsll((long long)rest) - 1;
            const int b = __shfl(k, first, 64);
            const unsigned long long same = __ballot(k == b);
            if (lane == first) atomicAdd(&bins[b], (unsigned long long)__popcll(same));
            rest &= ~same;
        }
    }
}

// ---- HistogramObserver::get_stats ----
__global__ __launch_bounds__(kObsThreads) void obs_hist_stats_kernel(const unsigned long long *__restrict__ bins, int nb, unsigned long long *__restrict__ out3) {
    __shared__ unsigned long long s[3 * kObsThreads];
    unsigned long long total = 0, weighted = 0, most = 0;
    for (int i = threadIdx.x; i < nb; i += kObsThreads) {
        const unsigned long long c = bins[i];
        total += c;
        weighted += (unsigned long long)i * c;
        most = c > most ? c : most;
    }
    s[threadIdx.x] = total;
    s[kObsThreads + threadIdx.x] = weighted;
    s[2 * kObsThreads + threadIdx.x] = most;
    __syncthreads();
    for (int off = kObsThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s[threadIdx.x] += s[threadIdx.x + off];
            s[kObsThreads + threadIdx.x] += s[kObsThreads + threadIdx.x + off];
            const unsigned long long o = s[2 * kObsThreads + threadIdx.x + off];
            if (o > s[2 * kObsThreads + threadIdx.x]) s[2 * kObsThreads + threadIdx.x] = o;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out3[0] = s[0];
        out3[1] = s[kObsThreads];
        out3[2] = s[2 * kObsThreads];
    }
}

static int obs_map_grid(int64_t n) { return stream_grid(n, 4 * kObsThreads, kObsMapGrid); }

// the first pass of a fold into a pooled block of partials (freed by the caller after the second pass is enqueued)
static int obs_minmax_parts_launch(th_ctx *ctx, const float *d_a, const float *d_b, int64_t n, void **part, int *n_parts) {
    *n_parts = n > 0 ? stream_grid(n, kObsPartMin, kObsParts) : 0;
    if (th_malloc(ctx, (size_t)std::max(*n_parts, 1) * 2 * sizeof(float), part)) return 1;
    if (*n_parts == 0) return 0;
    if (d_a == d_b) hipLaunchKernelGGL((minmax_parts_kernel<MinMaxNanIgnoring, true>), dim3(*n_parts), dim3(kObsThreads), 0, ctx->stream, d_a, d_b, n, (float *)*part);
    else hipLaunchKernelGGL((minmax_parts_kernel<MinMaxNanIgnoring, false>), dim3(*n_parts), dim3(kObsThreads), 0, ctx->stream, d_a, d_b, n, (float *)*part);
    TH_LAUNCH_CHECK();
    return 0;
}

}  // namespace th

using namespace th;

extern "C" {

int th_obs_minmax_first(th_ctx *ctx, const float *d_x, float *d_min, float *d_max, int64_t n) {
    TH_REQUIRE(ctx && n >= 0 && (n == 0 || (d_x && d_min && d_max)), "th_obs_minmax_first: null argument or negative length");
    if (n == 0) return 0;
    hipLaunchKernelGGL(obs_minmax_first_kernel, dim3(obs_map_grid(n)), dim3(kObsThreads), 0, ctx->stream, d_x, d_min, d_max, n);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_obs_minmax_update(th_ctx *ctx, const float *d_x, float *d_min, float *d_max, int64_t n) {
    TH_REQUIRE(ctx && n >= 0 && (n == 0 || (d_x && d_min && d_max)), "th_obs_minmax_update: null argument or negative length");
    if (n == 0) return 0;
    hipLaunchKernelGGL(obs_minmax_update_kernel, dim3(obs_map_grid(n)), dim3(kObsThreads), 0, ctx->stream, d_x, d_min, d_max, n);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_obs_fold(th_ctx *ctx, const float *d_min, const float *d_max, int64_t n, float *d_out2) {
    TH_REQUIRE(ctx && d_out2 && n >= 0 && (n == 0 || (d_min && d_max)), "th_obs_fold: null argument or negative length");
    void *part = nullptr;
    int n_parts = 0;
    if (obs_minmax_parts_launch(ctx, d_min, d_max, n, &part, &n_parts)) return 1;
    hipLaunchKernelGGL(obs_fold_final_kernel, dim3(1), dim3(kObsThreads), 0, ctx->stream, (const float *)part, n_parts, d_out2);
    TH_LAUNCH_CHECK();
    return th_free(ctx, part);
}

int th_obs_hist_edges(th_ctx *ctx, const float *d_x, int64_t n, int num_bins, float *d_edges) {
    TH_REQUIRE(ctx && d_edges && n >= 0 && (n == 0 || d_x), "th_obs_hist_edges: null argument or negative length");
    TH_REQUIRE(num_bins >= 1, "th_obs_hist_edges: num_bins must be at least 1 (got %d)", num_bins);
    void *part = nullptr;
    int n_parts = 0;
    if (obs_minmax_parts_launch(ctx, d_x, d_x, n, &part, &n_parts)) return 1;
    hipLaunchKernelGGL(obs_edges_kernel, dim3(1), dim3(kObsThreads), 0, ctx->stream, (const float *)part, n_parts, num_bins, d_edges);
    TH_LAUNCH_CHECK();
    return th_free(ctx, part);
}

int th_obs_hist_lds_max_bins(void) { return kObsLdsMaxBins; }

int th_obs_hist_count(th_ctx *ctx, const float *d_x, int64_t n, const float *d_edges, int num_bins, uint64_t *d_bins) {
    TH_REQUIRE(ctx && d_edges && d_bins && n >= 0 && (n == 0 || d_x), "th_obs_hist_count: null argument or negative length");
    TH_REQUIRE(num_bins >= 1, "th_obs_hist_count: num_bins must be at least 1 (got %d)", num_bins);
    TH_REQUIRE(n < ((int64_t)1 << 40), "th_obs_hist_count: %lld elements in one observation: a workgroup's 32-bit counters hold fewer than 2^32",
               (long long)n);
    if (n == 0) return 0;
    if (num_bins <= kObsLdsMaxBins) {
        const size_t lds = (size_t)(2 * num_bins + 1) * sizeof(float);
        TH_SET_MAX_LDS(ctx, obs_hist_lds_kernel, lds);
        hipLaunchKernelGGL(obs_hist_lds_kernel, dim3(stream_grid(n, kHistWgMin, kHistGrid)), dim3(kHistThreads), lds, ctx->stream, d_x, n, d_edges,
                           num_bins, (unsigned long long *)d_bins);
    } else {
        hipLaunchKernelGGL(obs_hist_global_kernel, dim3(stream_grid(n, kObsThreads, kHistGlobalGrid)), dim3(kObsThreads), 0, ctx->stream, d_x, n,
                           d_edges, num_bins, (unsigned long long *)d_bins);
    }
    TH_LAUNCH_CHECK();
    return 0;
}

int th_obs_hist_stats(th_ctx *ctx, const uint64_t *d_bins, int num_bins, uint64_t *d_out3) {
    TH_REQUIRE(ctx && d_bins && d_out3 && num_bins >= 1, "th_obs_hist_stats: null argument or no bins");
    hipLaunchKernelGGL(obs_hist_stats_kernel, dim3(1), dim3(kObsThreads), 0, ctx->stream, (const unsigned long long *)d_bins, num_bins,
                       (unsigned long long *)d_out3);
    TH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
