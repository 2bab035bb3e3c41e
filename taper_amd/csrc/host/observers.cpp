// observers.cpp -- the quantization observers (src/quantization/observers.rs): MinMaxObserver, HistogramObserver and ObserverManager over
// pooled device buffers.  The arithmetic is on the device (csrc/observers.hip); observe() enqueues and returns, the read-outs wait.
#include <cmath>
#include <limits>

#include "nn_internal.h"

namespace taper {

namespace {
template <class T>
std::vector<T> download(const void *d, size_t n) {   // (th_memcpy_d2h waits for the stream)
    std::vector<T> v(n);
    if (n) TH(th_memcpy_d2h(Device::ctx(), v.data(), d, n * sizeof(T)));
    return v;
}
constexpr size_t kWordsPerCount = sizeof(uint64_t) / sizeof(float);
}  // namespace

// ---- MinMaxObserver ----
void MinMaxObserver::observe(const Tensor &t) {
    if (!enabled_) return;
    const size_t m = t.len();
    if (!min_) {                     // observers.rs:57-60 (an empty first observation leaves the vectors empty: the next one is first again)
        if (m) {
            auto lo = Buffer::alloc(m), hi = Buffer::alloc(m);
            TH(th_obs_minmax_first(Device::ctx(), t.dptr(), lo->d, hi->d, (int64_t)m));
            min_ = lo;
            max_ = hi;
        }
    } else if (m) {                  // observers.rs:63-68: elements past the vectors' length are ignored, shapes are not compared
        TH(th_obs_minmax_update(Device::ctx(), t.dptr(), min_->d, max_->d, (int64_t)std::min(m, min_->n)));
    }
    ++count_;
}

std::vector<float> MinMaxObserver::min_values() const { return min_ ? download<float>(min_->d, min_->n) : std::vector<float>(); }
std::vector<float> MinMaxObserver::max_values() const { return max_ ? download<float>(max_->d, max_->n) : std::vector<float>(); }

void MinMaxObserver::reset() {
    min_.reset();
    max_.reset();
    count_ = 0;
}

ObserverStats MinMaxObserver::get_stats() const {
    float mm[2] = {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};   // the folds' seeds (observers.rs:85-98)
    if (min_) {
        auto out = Buffer::alloc(2);
        TH(th_obs_fold(Device::ctx(), min_->d, max_->d, (int64_t)min_->n, out->d));
        TH(th_memcpy_d2h(Device::ctx(), mm, out->d, sizeof(mm)));
    }
    return ObserverStats{count_, mm[0], mm[1], mm[1] - mm[0]};
}

// ---- HistogramObserver ----
HistogramObserver::HistogramObserver(size_t num_bins) : num_bins_(num_bins) {
    // observers.rs:200 computes num_bins - 1 in usize: zero bins would underflow there
    TAPER_ASSERT(num_bins >= 1, "HistogramObserver: num_bins must be at least 1 (the reference's find_bin underflows with 0 bins)");
    TAPER_ASSERT(num_bins <= ((size_t)1 << 30), "HistogramObserver: num_bins must be at most 2^30");
}

void HistogramObserver::observe(const Tensor &t) {
    if (!enabled_) return;
    th_ctx *ctx = Device::ctx();
    const float *x = t.defined() ? t.dptr() : nullptr;
    if (!bins_) {
        auto b = Buffer::alloc(num_bins_ * kWordsPerCount);
        TH(th_fill_f32(ctx, b->d, 0.0f, b->n));   // (all-zero bits: integer zeros)
        bins_ = b;
    }
    if (!edges_) {                   // observers.rs:168-179: the first observation (also the first after reset()) fixes the edges
        auto e = Buffer::alloc(num_bins_ + 1);
        TH(th_obs_hist_edges(ctx, x, (int64_t)t.len(), (int)num_bins_, e->d));
        edges_ = e;
    }
    TH(th_obs_hist_count(ctx, x, (int64_t)t.len(), edges_->d, (int)num_bins_, reinterpret_cast<uint64_t *>(bins_->d)));
    ++count_;
}

std::vector<uint64_t> HistogramObserver::bins() const {
    return bins_ ? download<uint64_t>(bins_->d, num_bins_) : std::vector<uint64_t>(num_bins_, 0);
}
std::vector<float> HistogramObserver::bin_edges() const { return edges_ ? download<float>(edges_->d, num_bins_ + 1) : std::vector<float>(); }

void HistogramObserver::reset() {   // observers.rs:219-223
    bins_.reset();
    edges_.reset();
    count_ = 0;
}

HistogramStats HistogramObserver::get_stats() const {   // observers.rs:226-245
    uint64_t s[3] = {0, 0, 0};
    if (bins_) {
        auto out = Buffer::alloc(3 * kWordsPerCount);
        TH(th_obs_hist_stats(Device::ctx(), reinterpret_cast<const uint64_t *>(bins_->d), (int)num_bins_, reinterpret_cast<uint64_t *>(out->d)));
        TH(th_memcpy_d2h(Device::ctx(), s, out->d, sizeof(s)));
    }
    const float mean_bin = s[0] > 0 ? (float)s[1] / (float)s[0] : 0.0f;
    return HistogramStats{count_, s[0], mean_bin, s[2]};
}

// ---- ObserverManager ----
void ObserverManager::add_minmax_observer(const std::string &name) { minmax_[name] = std::make_unique<MinMaxObserver>(); }
void ObserverManager::add_histogram_observer(const std::string &name, size_t num_bins) {
    histogram_[name] = std::make_unique<HistogramObserver>(num_bins);   // (a refused num_bins leaves an existing observer as it was)
}
void ObserverManager::observe_minmax(const std::string &name, const Tensor &t) {
    auto it = minmax_.find(name);
    if (it != minmax_.end()) it->second->observe(t);
}
void ObserverManager::observe_histogram(const std::string &name, const Tensor &t) {
    auto it = histogram_.find(name);
    if (it != histogram_.end()) it->second->observe(t);
}
bool ObserverManager::get_minmax_stats(const std::string &name, ObserverStats *out) const {
    auto it = minmax_.find(name);
    if (it == minmax_.end()) return false;
    *out = it->second->get_stats();
    return true;
}
bool ObserverManager::get_histogram_stats(const std::string &name, HistogramStats *out) const {
    auto it = histogram_.find(name);
    if (it == histogram_.end()) return false;
    *out = it->second->get_stats();
    return true;
}
void ObserverManager::reset_all() {
    for (auto &kv : minmax_) kv.second->reset();
    for (auto &kv : histogram_) kv.second->reset();
}
std::vector<std::string> ObserverManager::get_observer_names() const {   // (the reference's order is a HashMap's: unspecified)
    std::vector<std::string> names;
    for (const auto &kv : minmax_) names.push_back(kv.first);
    for (const auto &kv : histogram_) names.push_back(kv.first);
    return names;
}

}  // namespace taper
