// qcalib.hip -- percentile calibration of a static int8 layer's activation scale: a histogram of |x| over the range that
// th_act_range_update found, and the scale of the smallest clip that keeps a given share of the elements.
//
//   th_act_hist_update      every finite element of a tensor into num_bins 64-bit counters over [0, amax], amax = max(|min|, |max|) of the
//                           device pair: one read of the tensor, nothing written but counters (4 bytes per element)
//   th_act_scale_from_hist  one workgroup: the first bin k whose cumulative count reaches keep_ppm millionths of the total, the threshold
//                           T = (k + 1) amax / num_bins (exactly amax in the last bin) and scale = T / 127
//
// The counting pass is observers.hip's LDS form with the edge table taken out (hist_dev.h holds what the two share): a workgroup's 32-bit
// counters in LDS, the bin a wave currently sees most counted by ballot (half of a post-ReLU tensor sits in bin 0), the merge into the
// global bins by integer atomics, non-zero counters only, each workgroup from a bin of its own.  Integer sums do not depend on the order of
// arrival: the counters are bit-identical from run to run.  Both entry points only enqueue work: nothing is read back, nothing allocated.
#include "common.h"
#include "hist_dev.h"
#include "stream_dev.h"

namespace th {

constexpr int kActHistMinBins = 16;
constexpr int kScanThreads = kStreamThreads;

__device__ __forceinline__ float act_amax(const float *__restrict__ range2) { return fmaxf(fabsf(range2[0]), fabsf(range2[1])); }

// The bin of a finite v: min((int)(|v| * inv), nb - 1).  The product can be +inf (a v above the range times a large inv, or inv = +inf for
// an amax of zero) or a NaN (0 * inf, or a NaN amax): fminf hands the cast nb - 1 for both, so the cast only ever sees [0, nb - 1].
// NaN and +-inf elements count nowhere: -1.
__device__ __forceinline__ int act_bin(float v, float inv, int nb) {
    return isfinite(v) ? (int)fminf(__fmul_rn(fabsf(v), inv), (float)(nb - 1)) : -1;
}

// dynamic LDS: nb 32-bit counters.  A workgroup sees fewer than 2^32 elements (the host checks n).
__global__ __launch_bounds__(kHistThreads) void act_hist_kernel(const float *__restrict__ x, int64_t n, const float *__restrict__ range2, int nb,
                                                               unsigned long long *__restrict__ bins) {
    extern __shared__ unsigned cnt[];
    for (int i = threadIdx.x; i < nb; i += kHistThreads) cnt[i] = 0u;
    const float inv = __fdiv_rn((float)nb, act_amax(range2));
    __syncthreads();

    HotBin hb{cnt};
    int last = 0;   // this lane's latest bin, for the retarget: a lane whose element counted nowhere offers the hot bin itself (no candidate)
    auto count4 = [&](float4 a) {
        const int k0 = act_bin(a.x, inv, nb), k1 = act_bin(a.y, inv, nb), k2 = act_bin(a.z, inv, nb), k3 = act_bin(a.w, inv, nb);
        hb.count(k0); hb.count(k1); hb.count(k2); hb.count(k3);
        last = k3 >= 0 ? k3 : hb.hot;
    };
    hist_wave_walk(x, n, count4, [&] { hb.retarget(last, 16 * 64); }, [&](float v, bool valid) { hb.count(valid ? act_bin(v, inv, nb) : -1); });
    hb.flush();
    __syncthreads();
    hist_merge(cnt, nb, bins);
}

// One workgroup.  Lane t owns the bins [t per, (t + 1) per): their sum, an exclusive scan of the 256 sums through LDS, then each lane
// walks its bins for the first one that reaches the target; the smallest such bin over the lanes is k.  cum * 10^6 and total * keep_ppm
// stay below 2^63 for total < 2^43.
__global__ __launch_bounds__(kScanThreads) void act_scale_from_hist_kernel(const unsigned long long *__restrict__ bins, int nb, const float *__restrict__ range2,
                                                                          int keep_ppm, float *__restrict__ d_scale, unsigned long long *__restrict__ stats4) {
    __shared__ unsigned long long part[kScanThreads];
    __shared__ int first;
    const int t = threadIdx.x, per = (nb + kScanThreads - 1) / kScanThreads, lo = min(t * per, nb), hi = min(lo + per, nb);
    unsigned long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += bins[i];
    part[t] = sum;
    if (t == 0) first = nb;
    __syncthreads();
    unsigned long long before = 0, total = 0;   // the counts below this lane's bins; all of them
    for (int i = 0; i < kScanThreads; ++i) {
        const unsigned long long p = part[i];
        before += i < t ? p : 0ull;
        total += p;
    }
    const float mn = range2[0], mx = range2[1], amax = act_amax(range2);
    // the rules of a range that gives no histogram stay th_act_range_update's: its scale stands, and the report names the last bin
    const bool fallback = mn == mx || !isnormal(amax) || total == 0;
    if (fallback) {
        if (t == 0) {
            stats4[0] = (unsigned long long)(nb - 1);
            stats4[1] = total;
            stats4[2] = total;
            stats4[3] = bins[nb - 1];
        }
        return;
    }
    const unsigned long long target = total * (unsigned long long)keep_ppm;
    unsigned long long cum = before;
    for (int i = lo; i < hi; ++i) {
        cum += bins[i];
        if (cum * 1000000ull >= target) {
            atomicMin(&first, i);
            break;
        }
    }
    __syncthreads();
    const int k = first;   // (cum[nb - 1] = total reaches every target: k < nb)
    if (k < lo || k >= hi) return;
    cum = before;
    for (int i = lo; i <= k; ++i) cum += bins[i];
    const float T = k == nb - 1 ? amax : __fmul_rn((float)(k + 1), __fdiv_rn(amax, (float)nb));
    d_scale[0] = __fdiv_rn(T, 127.0f);
    stats4[0] = (unsigned long long)k;
    stats4[1] = total;
    stats4[2] = cum;
    stats4[3] = bins[k];
}

}  // namespace th

using namespace th;

extern "C" {

int th_act_hist_max_bins(void) { return kObsLdsMaxBins; }

int th_act_hist_update(th_ctx *ctx, const float *d_x, int64_t n, const float *d_range2, int num_bins, uint64_t *d_bins) {
    TH_REQUIRE(ctx && n >= 0 && (n == 0 || d_x) && d_range2 && d_bins, "th_act_hist_update: null argument or negative length");
    TH_REQUIRE(num_bins >= kActHistMinBins && num_bins <= kObsLdsMaxBins, "th_act_hist_update: num_bins must be in [%d, %d] (got %d)", kActHistMinBins,
               kObsLdsMaxBins, num_bins);
    TH_REQUIRE(n < ((int64_t)1 << 40), "th_act_hist_update: %lld elements in one call: a workgroup's 32-bit counters hold fewer than 2^32", (long long)n);
    if (n == 0) return 0;
    const size_t lds = (size_t)num_bins * sizeof(unsigned);
    hipLaunchKernelGGL(act_hist_kernel, dim3(stream_grid(n, kHistWgMin, kHistGrid)), dim3(kHistThreads), lds, ctx->stream, d_x, n, d_range2, num_bins,
                       (unsigned long long *)d_bins);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_act_scale_from_hist(th_ctx *ctx, const uint64_t *d_bins, int num_bins, const float *d_range2, int keep_ppm, float *d_scale, uint64_t *d_stats4) {
    TH_REQUIRE(ctx && d_bins && d_range2 && d_scale && d_stats4, "th_act_scale_from_hist: null argument");
    TH_REQUIRE(num_bins >= kActHistMinBins && num_bins <= kObsLdsMaxBins, "th_act_scale_from_hist: num_bins must be in [%d, %d] (got %d)", kActHistMinBins,
               kObsLdsMaxBins, num_bins);
    TH_REQUIRE(keep_ppm >= 1 && keep_ppm <= 1000000, "th_act_scale_from_hist: keep_ppm must be in [1, 1000000] (got %d)", keep_ppm);
    hipLaunchKernelGGL(act_scale_from_hist_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, (const unsigned long long *)d_bins, num_bins, d_range2, keep_ppm,
                       d_scale, (unsigned long long *)d_stats4);
    TH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
