// batchnorm.cpp -- BatchNorm2d, BasicBlock (nn.rs:829-857 announces both; torch.nn.BatchNorm2d's semantics) and ResidualBlock.  The arithmetic is on the
// device (csrc/batchnorm.hip): the forward leaves the statistics it used for the backward and updates the running pair in stream order,
// so a captured step replays it with no host work.
#include <cmath>

#include "nn_internal.h"

namespace taper {

// (the checks come first: a refused layer never reaches the device)
static size_t checked_features(size_t num_features, float eps, float momentum) {
    TAPER_ASSERT(num_features > 0 && num_features <= 0x7fffffffu, "BatchNorm2d: num_features must be positive");
    TAPER_ASSERT(std::isfinite(eps) && eps > 0.0f, "BatchNorm2d: eps must be finite and positive");
    TAPER_ASSERT(momentum >= 0.0f && momentum <= 1.0f, "BatchNorm2d: momentum must be in [0, 1]");
    return num_features;
}

BatchNorm2d::BatchNorm2d(size_t nf, float eps_, float momentum_, bool relu)
    : num_features(checked_features(nf, eps_, momentum_)), eps(eps_), momentum(momentum_), fuse_relu(relu) {
    gamma = Tensor(std::vector<float>(nf, 1.0f), {nf}).requires_grad();
    beta = Tensor(std::vector<float>(nf, 0.0f), {nf}).requires_grad();
    running_mean = Tensor(std::vector<float>(nf, 0.0f), {nf});
    running_var = Tensor(std::vector<float>(nf, 1.0f), {nf});
}

void BatchNorm2d::set_running_stats(const std::vector<float> &mean, const std::vector<float> &var) {
    TAPER_ASSERT(mean.size() == num_features && var.size() == num_features, "BatchNorm2d::set_running_stats: num_features values each expected");
    running_mean.set_data(mean);
    running_var.set_data(var);
}

Tensor BatchNorm2d::forward(const Tensor &x) const {
    TAPER_ASSERT(x.shape().size() == 4, "BatchNorm2d: expected a 4-D input [N, C, H, W]");
    TAPER_ASSERT(x.shape()[1] == num_features, "BatchNorm2d: input has " + std::to_string(x.shape()[1]) + " channels, the layer " +
                                                   std::to_string(num_features));
    const size_t hw_ = x.shape()[2] * x.shape()[3];
    TAPER_ASSERT(x.shape()[0] <= 0x7fffffffu && hw_ <= 0x7fffffffu, "BatchNorm2d: input too large");
    const int n = (int)x.shape()[0], c = (int)num_features, hw = (int)hw_;
    const bool batch_stats = training_;
    Tensor out = Tensor::empty(x.shape());
    auto saved = Buffer::alloc(2 * num_features);   // {mean, invstd} this forward normalised with
    TH(th_batchnorm2d_fwd(Device::ctx(), x.dptr(), gamma.dptr(), beta.dptr(), out.dptr(), running_mean.dptr(), running_var.dptr(), saved->d,
                          saved->d + num_features, n, c, hw, eps, momentum, batch_stats ? 1 : 0, fuse_relu ? 1 : 0));
    if ((x.get_requires_grad() || gamma.get_requires_grad() || beta.get_requires_grad()) && !NoGradScope::active()) {
        out.set_requires_grad(true);
        Tensor in = x, r = out, g = gamma, b = beta;
        const bool relu = fuse_relu;
        Tape::push(out, true, [in, r, g, b, saved, n, c, hw, batch_stats, relu]() {
            if (!r.has_grad()) return;
            // gradients go straight into the slots: += where one is Some already, overwritten otherwise; a frozen gamma / beta gets scratch
            int mask = 0;
            bool none;
            float *gx = nullptr, *gg = nullptr, *gb = nullptr;
            std::shared_ptr<Buffer> scratch;
            if (in.get_requires_grad()) {
                gx = in.grad_for_write(&none);
                if (!none) mask |= 1;
            }
            if (g.get_requires_grad()) {
                gg = g.grad_for_write(&none);
                if (!none) mask |= 2;
            }
            if (b.get_requires_grad()) {
                gb = b.grad_for_write(&none);
                if (!none) mask |= 4;
            }
            if (!gg || !gb) {
                scratch = Buffer::alloc(2 * (size_t)c);
                if (!gg) gg = scratch->d;
                if (!gb) gb = scratch->d + c;
            }
            TH(th_batchnorm2d_bwd(Device::ctx(), r.grad_dptr(), in.dptr(), relu ? r.dptr() : nullptr, g.dptr(), saved->d, saved->d + c, gx, gg, gb,
                                  n, c, hw, batch_stats ? 1 : 0, mask));
        });
    }
    return out;
}

// y = relu?(bn(x) + residual) in the normalisation's own map (th_bn_residual_fwd), one tape node; the closure's one call leaves the
// residual's gradient beside gx, ggamma and gbeta (th_bn_residual_bwd)
Tensor BatchNorm2d::forward_add(const Tensor &x, const Tensor &residual) const {
    TAPER_ASSERT(x.shape().size() == 4, "BatchNorm2d::forward_add: expected a 4-D input [N, C, H, W]");
    TAPER_ASSERT(x.shape()[1] == num_features, "BatchNorm2d::forward_add: input has " + std::to_string(x.shape()[1]) + " channels, the layer " +
                                                   std::to_string(num_features));
    TAPER_ASSERT(residual.defined() && residual.shape() == x.shape(), "BatchNorm2d::forward_add: the residual's shape differs from the input's");
    // (two gradients go to two slots in one launch: a tensor cannot be both operands -- 2 * bn(x) is not a skip connection)
    TAPER_ASSERT(residual.dptr() != x.dptr(), "BatchNorm2d::forward_add: the residual shares its storage with the input");
    const size_t hw_ = x.shape()[2] * x.shape()[3];
    TAPER_ASSERT(x.shape()[0] <= 0x7fffffffu && hw_ <= 0x7fffffffu, "BatchNorm2d::forward_add: input too large");
    const int n = (int)x.shape()[0], c = (int)num_features, hw = (int)hw_;
    const bool batch_stats = training_;
    Tensor out = Tensor::empty(x.shape());
    auto saved = Buffer::alloc(2 * num_features);   // {mean, invstd} this forward normalised with
    TH(th_bn_residual_fwd(Device::ctx(), x.dptr(), residual.dptr(), gamma.dptr(), beta.dptr(), out.dptr(), running_mean.dptr(), running_var.dptr(),
                          saved->d, saved->d + num_features, n, c, hw, eps, momentum, batch_stats ? 1 : 0, fuse_relu ? 1 : 0));
    if ((x.get_requires_grad() || residual.get_requires_grad() || gamma.get_requires_grad() || beta.get_requires_grad()) && !NoGradScope::active()) {
        out.set_requires_grad(true);
        Tensor in = x, res = residual, r = out, g = gamma, b = beta;
        const bool relu = fuse_relu;
        Tape::push(out, true, [in, res, r, g, b, saved, n, c, hw, batch_stats, relu]() {
            if (!r.has_grad()) return;
            // as in forward: += where a slot is Some already (bit 3: the residual's), overwritten otherwise; a frozen gamma / beta and a
            // residual that takes no gradient get scratch
            int mask = 0;
            bool none;
            float *gx = nullptr, *gr = nullptr, *gg = nullptr, *gb = nullptr;
            std::shared_ptr<Buffer> scratch, rscratch;
            if (in.get_requires_grad()) {
                gx = in.grad_for_write(&none);
                if (!none) mask |= 1;
            }
            if (res.get_requires_grad()) {
                gr = res.grad_for_write(&none);
                if (!none) mask |= 8;
            } else {
                rscratch = Buffer::alloc(res.len());
                gr = rscratch->d;
            }
            if (g.get_requires_grad()) {
                gg = g.grad_for_write(&none);
                if (!none) mask |= 2;
            }
            if (b.get_requires_grad()) {
                gb = b.grad_for_write(&none);
                if (!none) mask |= 4;
            }
            if (!gg || !gb) {
                scratch = Buffer::alloc(2 * (size_t)c);
                if (!gg) gg = scratch->d;
                if (!gb) gb = scratch->d + c;
            }
            TH(th_bn_residual_bwd(Device::ctx(), r.grad_dptr(), in.dptr(), relu ? r.dptr() : nullptr, g.dptr(), saved->d, saved->d + c, gx, gr, gg,
                                  gb, n, c, hw, batch_stats ? 1 : 0, mask));
        });
    }
    return out;
}

// the flag a block hands to its convs of this stride: the exact strided convolution exists for stride 2 alone
static bool exact_for(const char *block, size_t stride, bool exact_stride) {
    TAPER_ASSERT(!exact_stride || stride == 1 || stride == 2,
                 std::string(block) + " exact_stride: the stride must be 1 or 2 (got " + std::to_string(stride) + ")");
    return exact_stride && stride == 2;
}

BasicBlock::BasicBlock(size_t in_ch, size_t out_ch, size_t stride, uint64_t seed, bool exact_stride)
    : conv(in_ch, out_ch, {3, 3}, {(int)stride, (int)stride}, {1, 1}, true, seed, 1, exact_for("BasicBlock", stride, exact_stride)),
      bn(out_ch, 1e-5f, 0.1f, true) {}

static size_t checked_block(size_t in_ch, size_t out_ch, size_t stride, bool pointwise_shortcut = false) {
    TAPER_ASSERT(in_ch > 0 && out_ch > 0 && stride > 0 && in_ch <= 0x7fffffffu && out_ch <= 0x7fffffffu && stride <= 0x7fffffffu,
                 "ResidualBlock: in_channels, out_channels and stride must be positive");
    // the pointwise convolution exists for strides 1 and 2 alone
    TAPER_ASSERT(!pointwise_shortcut || stride == 1 || stride == 2,
                 "ResidualBlock pointwise_shortcut: the stride must be 1 or 2 (got " + std::to_string(stride) + ")");
    return in_ch;
}

ResidualBlock::ResidualBlock(size_t in_ch, size_t out_ch, size_t stride, uint64_t seed, bool exact_stride, bool pointwise_shortcut)
    : conv1(checked_block(in_ch, out_ch, stride, pointwise_shortcut), out_ch, {3, 3}, {(int)stride, (int)stride}, {1, 1}, false, seed, 1,
            exact_for("ResidualBlock", stride, exact_stride)),
      bn1(out_ch, 1e-5f, 0.1f, true),
      conv2(out_ch, out_ch, {3, 3}, {1, 1}, {1, 1}, false, seed + 1),
      bn2(out_ch, 1e-5f, 0.1f, true) {
    if (in_ch != out_ch || stride != 1) {
        if (pointwise_shortcut)
            shortcut_conv = std::make_unique<Conv2d>(Conv2d::pointwise(in_ch, out_ch, stride, seed + 2));
        else
            shortcut_conv = std::make_unique<Conv2d>(in_ch, out_ch, std::make_pair(3, 3), std::make_pair((int)stride, (int)stride),
                                                     std::make_pair(1, 1), false, seed + 2, 1, exact_for("ResidualBlock", stride, exact_stride));
        shortcut_bn = std::make_unique<BatchNorm2d>(out_ch, 1e-5f, 0.1f, false);
    }
}

Tensor ResidualBlock::forward(const Tensor &x) const {
    const Tensor h = conv2.forward(bn1.forward(conv1.forward(x)));
    return bn2.forward_add(h, shortcut_conv ? shortcut_bn->forward(shortcut_conv->forward(x)) : x);
}

std::vector<BatchNorm2d *> ResidualBlock::batchnorms() {
    std::vector<BatchNorm2d *> b{&bn1, &bn2};
    if (shortcut_bn) b.push_back(shortcut_bn.get());
    return b;
}

std::vector<Tensor> ResidualBlock::parameters() const {
    std::vector<Tensor> p{conv1.weight, bn1.gamma, bn1.beta, conv2.weight, bn2.gamma, bn2.beta};
    if (shortcut_conv) {
        p.push_back(shortcut_conv->weight);
        p.push_back(shortcut_bn->gamma);
        p.push_back(shortcut_bn->beta);
    }
    return p;
}

std::vector<Tensor> ResidualBlock::buffers() const {
    std::vector<Tensor> b{bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var};
    if (shortcut_bn) {
        b.push_back(shortcut_bn->running_mean);
        b.push_back(shortcut_bn->running_var);
    }
    return b;
}

static size_t checked_bottleneck(size_t in_ch, size_t mid_ch, size_t out_ch, size_t stride) {
    TAPER_ASSERT(in_ch > 0 && mid_ch > 0 && out_ch > 0 && stride > 0 && in_ch <= 0x7fffffffu && mid_ch <= 0x7fffffffu && out_ch <= 0x7fffffffu &&
                     stride <= 0x7fffffffu,
                 "BottleneckBlock: in_channels, mid_channels, out_channels and stride must be positive");
    TAPER_ASSERT(stride == 1 || stride == 2, "BottleneckBlock: the stride must be 1 or 2 (got " + std::to_string(stride) + ")");
    return in_ch;
}

BottleneckBlock::BottleneckBlock(size_t in_ch, size_t mid_ch, size_t out_ch, size_t stride, uint64_t seed)
    : conv1(Conv2d::pointwise(checked_bottleneck(in_ch, mid_ch, out_ch, stride), mid_ch, 1, seed)),
      bn1(mid_ch, 1e-5f, 0.1f, true),
      conv2(mid_ch, mid_ch, {3, 3}, {(int)stride, (int)stride}, {1, 1}, false, seed + 1, 1, stride == 2),
      bn2(mid_ch, 1e-5f, 0.1f, true),
      conv3(Conv2d::pointwise(mid_ch, out_ch, 1, seed + 2)),
      bn3(out_ch, 1e-5f, 0.1f, true) {
    if (in_ch != out_ch || stride != 1) {
        shortcut_conv = std::make_unique<Conv2d>(Conv2d::pointwise(in_ch, out_ch, stride, seed + 3));
        shortcut_bn = std::make_unique<BatchNorm2d>(out_ch, 1e-5f, 0.1f, false);
    }
}

Tensor BottleneckBlock::forward(const Tensor &x) const {
    const Tensor h = conv3.forward(bn2.forward(conv2.forward(bn1.forward(conv1.forward(x)))));
    return bn3.forward_add(h, shortcut_conv ? shortcut_bn->forward(shortcut_conv->forward(x)) : x);
}

std::vector<BatchNorm2d *> BottleneckBlock::batchnorms() {
    std::vector<BatchNorm2d *> b{&bn1, &bn2, &bn3};
    if (shortcut_bn) b.push_back(shortcut_bn.get());
    return b;
}

std::vector<Tensor> BottleneckBlock::parameters() const {
    std::vector<Tensor> p{conv1.weight, bn1.gamma, bn1.beta, conv2.weight, bn2.gamma, bn2.beta, conv3.weight, bn3.gamma, bn3.beta};
    if (shortcut_conv) {
        p.push_back(shortcut_conv->weight);
        p.push_back(shortcut_bn->gamma);
        p.push_back(shortcut_bn->beta);
    }
    return p;
}

std::vector<Tensor> BottleneckBlock::buffers() const {
    std::vector<Tensor> b{bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var, bn3.running_mean, bn3.running_var};
    if (shortcut_bn) {
        b.push_back(shortcut_bn->running_mean);
        b.push_back(shortcut_bn->running_var);
    }
    return b;
}

bool holds_exact_pointwise(const Module &m) {
    if (auto *s = dynamic_cast<const Sequential *>(&m)) {
        for (const auto &l : s->layers)
            if (holds_exact_pointwise(*l)) return true;
        return false;
    }
    if (auto *cv = dynamic_cast<const Conv2d *>(&m)) return cv->exact_pointwise;
    if (auto *bb = dynamic_cast<const BasicBlock *>(&m)) return bb->conv.exact_pointwise;
    if (auto *rb = dynamic_cast<const ResidualBlock *>(&m)) return rb->shortcut_conv && rb->shortcut_conv->exact_pointwise;
    return dynamic_cast<const BottleneckBlock *>(&m) != nullptr;
}

std::vector<Tensor> BasicBlock::parameters() const {
    std::vector<Tensor> p = conv.parameters();
    for (const Tensor &t : bn.parameters()) p.push_back(t);
    return p;
}

std::vector<Tensor> Sequential::buffers() const {
    std::vector<Tensor> b;
    for (auto &l : layers)
        for (auto &t : l->buffers()) b.push_back(t);
    return b;
}

void batchnorm_modules(Module &m, std::vector<BatchNorm2d *> *out) {
    if (auto *s = dynamic_cast<Sequential *>(&m)) {
        for (const auto &l : s->layers) batchnorm_modules(*l, out);
    } else if (auto *bb = dynamic_cast<BasicBlock *>(&m)) {
        out->push_back(&bb->bn);
    } else if (auto *rb = dynamic_cast<ResidualBlock *>(&m)) {
        for (BatchNorm2d *b : rb->batchnorms()) out->push_back(b);
    } else if (auto *nb = dynamic_cast<BottleneckBlock *>(&m)) {
        for (BatchNorm2d *b : nb->batchnorms()) out->push_back(b);
    } else if (auto *bn = dynamic_cast<BatchNorm2d *>(&m)) {
        out->push_back(bn);
    }
}

void set_training(Module &m, bool on) {
    if (auto *s = dynamic_cast<Sequential *>(&m)) {
        for (const auto &l : s->layers) set_training(*l, on);
    } else if (auto *bb = dynamic_cast<BasicBlock *>(&m)) {
        bb->bn.set_training(on);
    } else if (auto *rb = dynamic_cast<ResidualBlock *>(&m)) {
        for (BatchNorm2d *b : rb->batchnorms()) b->set_training(on);
    } else if (auto *nb = dynamic_cast<BottleneckBlock *>(&m)) {
        for (BatchNorm2d *b : nb->batchnorms()) b->set_training(on);
    } else if (auto *bn = dynamic_cast<BatchNorm2d *>(&m)) {
        bn->set_training(on);
    } else if (auto *d = dynamic_cast<Dropout *>(&m)) {
        if (on) d->train();
        else d->eval();
    }
}

}  // namespace taper
