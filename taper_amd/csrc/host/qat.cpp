// qat.cpp -- quantization-aware training (src/quantization/{qat_config,qat_layers,qat_manager,fake_quantize}.rs): the process-wide QAT
// state, the QAT layers and the one-launch-pair weight pass the Trainer runs each step.  The arithmetic is on the device
// (csrc/fake_quant.hip); what the reference leaves unfinished is done as it means it ("Quantization-aware training").
#include <map>
#include <mutex>

#include "nn_internal.h"

namespace taper {

void QATConfig::check() const {
    if (qtype == QType::Int4 || qtype == QType::BFloat16 || qtype == QType::NF4)
        throw Error("QAT quantization type " + std::string(qtype == QType::Int4 ? "Int4" : qtype == QType::BFloat16 ? "BFloat16" : "NF4") +
                    " is not supported: the reference's codec for it is a placeholder that returns zeros");
    if (qtype != QType::Int8 && qtype != QType::Float16) throw Error("QAT: unknown quantization type");
    if (!symmetric)
        throw Error("QAT with symmetric = false is not supported: the reference's asymmetric zero point and clamp cut off the upper half "
                    "of the range (fake_quantize.rs:84-91, 164-172)");
    if (per_channel) throw Error("QAT with per_channel = true is not supported: the reference never implements per-channel scales");
}

// ---- qat_manager.rs: one manager per process ----
namespace qat {
namespace {
std::mutex g_mu;
bool g_enabled = false, g_training = true;   // qat_manager.rs:28-34, 80-82
std::map<std::string, bool> g_modules;
}  // namespace

void enable(bool on) { std::lock_guard<std::mutex> l(g_mu); g_enabled = on; }
bool enabled() { std::lock_guard<std::mutex> l(g_mu); return g_enabled; }
void set_training_mode(bool on) { std::lock_guard<std::mutex> l(g_mu); g_training = on; }
bool is_training() { std::lock_guard<std::mutex> l(g_mu); return g_training; }
void set_module(const std::string &id, bool on) { std::lock_guard<std::mutex> l(g_mu); g_modules[id] = on; }
bool module_enabled(const std::string &id) {   // qat_manager.rs:59-71
    std::lock_guard<std::mutex> l(g_mu);
    if (!g_enabled) return false;
    auto it = g_modules.find(id);
    return it == g_modules.end() || it->second;
}
Status status() {   // qat_manager.rs:123-133
    std::lock_guard<std::mutex> l(g_mu);
    Status s{g_enabled, g_training, g_modules.size(), 0};
    for (const auto &kv : g_modules) s.enabled_modules += kv.second ? 1 : 0;
    return s;
}
}  // namespace qat

// ---- the layers ----
QATModule::QATModule(const QATConfig &c, std::string id) : config(c), module_id(std::move(id)) {
    config.check();   // before anything touches the device
}

void QATModule::enable_qat(bool on) {   // qat_layers.rs:68-71
    qat_enabled = on;
    qat::set_module(module_id, on);
}

void QATModule::alloc_buffers() {
    wq_ = Buffer::alloc(master_weight().len());
    if (master_bias().defined()) bq_ = Buffer::alloc(master_bias().len());
    obs_ = Buffer::alloc(5);
    TH(th_fill_f32(Device::ctx(), obs_->d, 0.0f, 5));
}

void QATModule::items(std::vector<th_fq_item> *out) const {
    const Tensor &w = master_weight(), &b = master_bias();
    out->push_back(th_fq_item{w.dptr(), wq_->d, obs_->d, (int64_t)w.len(), codec()});
    if (b.defined()) out->push_back(th_fq_item{b.dptr(), bq_->d, obs_->d + 3, (int64_t)b.len(), codec()});
}

void QATModule::fake_quant_params(Tensor *w, Tensor *b) const {
    if (!prepared) {
        if (!own_pass_) own_pass_ = std::make_shared<QATWeightPass>();
        own_pass_->run(std::vector<const QATModule *>{this});
    }
    prepared = false;
    // straight-through estimator for the parameters (fake_quantize.rs:137-153): each round trip shares its master's grad slot, so every
    // gradient written for it -- and every fused Adam update found through that slot -- lands on the master
    *w = master_weight();
    w->data_ = wq_;
    *b = master_bias();
    if (b->defined()) b->data_ = bq_;
}

Tensor QATModule::fake_quantized(int which) const {
    const Tensor &m = which == 0 ? master_weight() : master_bias();
    TAPER_ASSERT(which == 0 || which == 1, "fake_quantized: 0 = weight, 1 = bias");
    TAPER_ASSERT(m.defined(), "fake_quantized: the layer has no bias");
    Tensor c = Tensor::empty(m.shape());
    TH(th_memcpy_d2d(Device::ctx(), c.dptr(), (which == 0 ? wq_ : bq_)->d, m.len() * sizeof(float)));
    return c;
}

Tensor QATModule::fake_quant_activation(const Tensor &y) const {
    Tensor out = Tensor::empty(y.shape());
    TH(th_fake_quant_act(Device::ctx(), y.dptr(), out.dptr(), (int64_t)y.len(), codec(), obs_->d + 2));
    if (y.get_requires_grad()) {
        out.set_requires_grad(true);
        Tensor in = y, r = out;
        Tape::push(out, true, [in, r]() {   // fake_quantize.rs:137-153: the gradient passes through unchanged
            if (!r.has_grad()) return;
            if (!in.has_grad() && !in.grad_->buf_is_arena && !r.grad_->shared_const && !r.grad_->buf_is_arena) {
                // nothing there yet: the output's gradient IS the input's -- adopt the buffer, no pass of its own (r has no other reader)
                in.grad_->buf = r.grad_->buf;
                in.grad_->has = true;
                in.grad_->known_zero = false;
                return;
            }
            bool none;
            float *g = in.grad_for_write(&none);
            if (none) TH(th_memcpy_d2d(Device::ctx(), g, r.grad_dptr(), in.len() * sizeof(float)));
            else TH(th_axpy(Device::ctx(), 1.0f, r.grad_dptr(), g, in.len()));
        });
    }
    return out;
}

void QATModule::observed(float out[3]) const { TH(th_memcpy_d2h(Device::ctx(), out, obs_->d, 3 * sizeof(float))); }

QATLinear::QATLinear(size_t in_features, size_t out_features, bool with_bias, const QATConfig &c, std::string id, uint64_t seed)
    : QATModule(c, std::move(id)), inner(in_features, out_features, with_bias, seed) {
    alloc_buffers();
}

Tensor QATLinear::forward(const Tensor &x) const {   // qat_layers.rs:91-122
    if (!active()) return inner.forward(x);
    Tensor w, b;
    fake_quant_params(&w, &b);
    Tensor y = x.linear(w, b, false);
    return config.activations ? fake_quant_activation(y) : y;
}

QATConv2d::QATConv2d(size_t in_ch, size_t out_ch, std::pair<int, int> kernel, std::pair<int, int> stride, std::pair<int, int> padding,
                     bool with_bias, bool relu, const QATConfig &c, std::string id, uint64_t seed)
    : QATModule(c, std::move(id)), inner(in_ch, out_ch, kernel, stride, padding, with_bias, seed) {
    inner.fuse_relu = relu;
    alloc_buffers();
}

Tensor QATConv2d::forward(const Tensor &x) const {   // qat_layers.rs:220-252; the ReLU of a Conv2dReLU follows the activation fake-quant
    if (!active()) return inner.forward(x);
    Tensor w, b;
    fake_quant_params(&w, &b);
    if (!config.activations) return x.conv2d(w, b, inner.stride, inner.padding, inner.dilation, inner.fuse_relu);
    Tensor y = fake_quant_activation(x.conv2d(w, b, inner.stride, inner.padding, inner.dilation, false));
    return inner.fuse_relu ? y.relu() : y;
}

void qat_modules(const Module &m, std::vector<const QATModule *> *out, bool active_only) {
    if (auto *s = dynamic_cast<const Sequential *>(&m)) {
        for (const auto &l : s->layers) qat_modules(*l, out, active_only);
        return;
    }
    if (auto *q = dynamic_cast<const QATModule *>(&m))
        if (!active_only || q->active()) out->push_back(q);
}

// ---- the weight pass ----
static bool same_items(const std::vector<th_fq_item> &a, const std::vector<th_fq_item> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].d_x != b[i].d_x || a[i].d_y != b[i].d_y || a[i].d_params != b[i].d_params || a[i].n != b[i].n || a[i].qtype != b[i].qtype)
            return false;
    return true;
}

bool QATWeightPass::sync(const std::vector<const QATModule *> &mods) {
    std::vector<th_fq_item> items;
    for (const QATModule *q : mods) q->items(&items);
    if (items.empty() || (d_items_ && same_items(items, items_))) return false;
    // a new list (first step, a layer switched, parameters re-homed): a fresh buffer, a synchronising copy -- never inside a capture.  The
    // old buffer goes back to the pool: whoever captured launches that read it keys them on generation() and drops them (Trainer)
    d_items_ = Buffer::alloc((items.size() * sizeof(th_fq_item) + sizeof(float) - 1) / sizeof(float));
    TH(th_memcpy_h2d(Device::ctx(), d_items_->d, items.data(), items.size() * sizeof(th_fq_item)));
    items_ = items;
    ++generation_;
    return true;
}

size_t QATWeightPass::run(const Module &m) {
    std::vector<const QATModule *> mods;
    qat_modules(m, &mods, true);
    return run(mods);
}

size_t QATWeightPass::run(const std::vector<const QATModule *> &mods) {
    if (mods.empty()) return 0;
    sync(mods);
    TH(th_fake_quant_multi(Device::ctx(), reinterpret_cast<const th_fq_item *>(d_items_->d), (int)items_.size()));
    for (const QATModule *q : mods) q->prepared = true;
    return mods.size();
}

}  // namespace taper
