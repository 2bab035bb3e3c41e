// quantized.cpp -- post-training quantization of a trained model (src/nn.rs:14-23 `Module::quantize`, the quantized twins of
// nn.rs:62-504, tensor.rs:2084-2108 `Tensor::quantize`).  Every code is made on the device by the storage codecs (th_quantize_int8 /
// th_f32_to_f16) from the live parameters; the source model is only read.  A twin keeps its codes and nothing else: no f32 copy of a
// weight outlives a forward call (the reference caches one in QuantizedLinear -- storage only, the values are the same).
#include "nn_internal.h"

namespace taper {

namespace {

size_t code_bytes(int qtype, size_t n) { return qtype == TH_QTYPE_INT8 ? n : 2 * n; }

QTensor quantize_tensor(const Tensor &t, int qtype) {   // tensor.rs:2084-2108 for the two codecs that do real work
    QTensor q;
    q.qtype = qtype;
    q.n = t.len();
    q.shape = t.shape();
    q.codes = Buffer::alloc((code_bytes(qtype, q.n) + 3) / 4);
    th_ctx *ctx = Device::ctx();
    if (qtype == TH_QTYPE_INT8) {
        q.params = Buffer::alloc(2);
        TH(th_quantize_int8(ctx, t.dptr(), reinterpret_cast<int8_t *>(q.codes->d), q.n, q.params->d));
    } else {
        TH(th_f32_to_f16(ctx, t.dptr(), reinterpret_cast<uint16_t *>(q.codes->d), q.n));
    }
    return q;
}

// An int8 weight with one pair per channel (th_quantize_int8_channels): element k of channel c at t[c * chan_stride + k * elem_stride]
QTensor quantize_channels(const Tensor &t, size_t channels, size_t chan_stride, size_t elem_stride) {
    QTensor q;
    q.n = t.len();
    q.shape = t.shape();
    q.channels = channels, q.chan_stride = chan_stride, q.elem_stride = elem_stride;
    q.codes = Buffer::alloc((q.n + 3) / 4);
    q.params = Buffer::alloc(2 * channels);
    TH(th_quantize_int8_channels(Device::ctx(), t.dptr(), (int)channels, (int64_t)(q.n / channels), (int64_t)chan_stride, (int64_t)elem_stride,
                                 reinterpret_cast<int8_t *>(q.codes->d), q.params->d));
    return q;
}

// the reference's parameter-free layers: their twins run the float layer itself (values pass through unchanged)
class QPass : public QuantizedModule {
   public:
    explicit QPass(std::shared_ptr<Module> m) : m_(std::move(m)) {}
    Tensor forward(const Tensor &x) const override { return m_->forward(x); }
    bool is_relu() const { return dynamic_cast<const ReLU *>(m_.get()) != nullptr; }
    const MaxPool2d *max_pool() const { return dynamic_cast<const MaxPool2d *>(m_.get()); }
    const Flatten *flatten() const { return dynamic_cast<const Flatten *>(m_.get()); }

   private:
    std::shared_ptr<Module> m_;
};

// The calibrated activation of a static twin, on the device: {finite min, finite max} of the calibration inputs, then the scale they
// give.  Empty in a weight-only twin.
// Percentile calibration adds, while quantize_static runs, `hist`: the layer's own counters over the final range, made and
// zeroed at its first input of pass two and given back once the scale is written; `stats`, the four integers of the report, stays.
struct ActScale {
    std::shared_ptr<Buffer> buf;
    mutable std::shared_ptr<Buffer> hist, stats;   // (calibration fills a twin it only reads otherwise)
    mutable int bins = 0;
    explicit operator bool() const { return buf != nullptr; }
    void alloc() { buf = Buffer::alloc(3); }
    const float *scale() const { return buf->d + 2; }
    uint64_t *counters() const { return reinterpret_cast<uint64_t *>(hist->d); }
    uint64_t *report() const { return reinterpret_cast<uint64_t *>(stats->d); }
    // calibration: the finite min / max of one more float input of the layer, and the scale of the range so far
    void observe(const Tensor &x, bool first) const { TH(th_act_range_update(Device::ctx(), x.dptr(), (int64_t)x.len(), first ? 1 : 0, buf->d, buf->d + 2)); }
    // pass two: one more float input of the layer into its histogram of |x| against the final range
    void observe_hist(const Tensor &x, int num_bins) const {
        th_ctx *ctx = Device::ctx();
        if (!hist) {
            hist = Buffer::alloc(2 * (size_t)num_bins);
            stats = Buffer::alloc(8);
            bins = num_bins;
            TH(th_fill_f32(ctx, hist->d, 0.0f, 2 * (size_t)num_bins));   // (the bits of 0.0f are those of a zero counter)
        }
        TH(th_act_hist_update(ctx, x.dptr(), (int64_t)x.len(), buf->d, bins, counters()));
    }
    // after pass two: the scale of the clip that keeps keep_ppm millionths, the report, and the counters back to the pool
    void scale_from_hist(int keep_ppm) const {
        if (!hist) return;
        TH(th_act_scale_from_hist(Device::ctx(), counters(), bins, buf->d, keep_ppm, buf->d + 2, report()));
        hist.reset();   // (stream order keeps it alive for the launch above)
    }
    void list(std::vector<const float *> *out) const {
        if (buf) out->push_back(scale());
    }
    void list(std::vector<ActCalibration> *out) const {
        if (buf) out->push_back(ActCalibration{buf->d, stats ? report() : nullptr, bins});
    }
};

// a twin's bias as the kernels take it: codes and codec parameters, both null without one (f16 codes have no parameters)
struct BiasPtrs {
    const void *codes = nullptr;
    const float *params = nullptr;
    explicit BiasPtrs(const std::unique_ptr<QTensor> &b) {
        if (b) codes = b->codes->d, params = b->params ? b->params->d : nullptr;
    }
    const int8_t *i8() const { return static_cast<const int8_t *>(codes); }
};

// where a product goes: f32 (the default), or the codes of the next layer -- made with its `scale`, rows (a Linear's) or pixels (a
// conv's) `pitch` bytes apart; a conv's product leaves the pixel sums out when `sums` is false (a pool that follows makes them, a Linear
// sums its own rows).  The next layer fills it: QConv::dest, QLinear::dest.
struct QDest {
    const float *scale = nullptr;
    size_t pitch = 0;
    bool sums = true;
    explicit operator bool() const { return scale != nullptr; }
};

class QLinear : public QuantizedModule {   // nn.rs:62-69, 88-120
   public:
    // o.linears: the static int8 twin (quantize_static) -- the weight codes re-laid once with rows padded to the product's K step, and one
    // activation scale on the device that calibration fixes; o.per_channel (static only): one weight pair per row
    // keep_packed: the packed codes stay until the enclosing Sequential has resolved its links (a Flatten link re-lays from them)
    QLinear(const Linear &l, int qtype, QuantizeOptions o = {}, bool keep_packed = false)
        : w_(o.linears && o.per_channel ? quantize_channels(l.weight, l.weight.shape()[0], l.weight.shape()[1], 1) : quantize_tensor(l.weight, qtype)),
          k_(l.weight.shape()[1]),
          n_(l.weight.shape()[0]) {
        if (l.bias.defined()) b_ = std::make_unique<QTensor>(quantize_tensor(l.bias, qtype));
        if (!o.linears) return;
        const size_t step = (size_t)th_qlinear_i8_kstep();
        w_.pitch = (k_ + step - 1) / step * step;
        auto padded = Buffer::alloc(n_ * w_.pitch / 4);
        TH(th_pad_rows_int8(Device::ctx(), reinterpret_cast<const int8_t *>(w_.codes->d), (int)n_, (int)k_, reinterpret_cast<int8_t *>(padded->d), (int)w_.pitch));
        if (keep_packed) packed_ = w_.codes;
        w_.codes = padded;     // (the packed copy goes back to the pool: stream order keeps it alive for the launch above)
        act_.alloc();
    }
    // A Flatten link ahead: the input arrives as channel-last codes [hw][cpitch] of c channels, so the rows [c][hw] are re-laid
    // once as [hw][cpitch] (the conv weight pack with hw taps) and replace the padded copy; K becomes hw * cpitch code bytes a row.
    void link_flatten(size_t c, size_t hw, size_t cpitch) {
        TAPER_ASSERT(packed_ && act_ && c * hw == k_, "QuantizedLinear: a Flatten link needs the packed codes of a static layer");
        auto relaid = Buffer::alloc(n_ * hw * cpitch / 4);
        TH(th_pack_conv_weight_int8(Device::ctx(), reinterpret_cast<const int8_t *>(packed_->d), (int)n_, (int)c, (int)hw, 1, reinterpret_cast<int8_t *>(relaid->d),
                                    (int)cpitch));
        w_.codes = relaid;
        w_.pitch = hw * cpitch;
        w_.relaid_c = c, w_.relaid_cpitch = cpitch;
    }
    void drop_packed() { packed_.reset(); }
    bool is_static() const { return (bool)act_; }
    size_t in_features() const { return k_; }
    size_t flat_hw() const { return w_.relaid_c ? k_ / w_.relaid_c : 0; }   // > 0: behind a Flatten link
    // this layer as the destination of the product ahead: its scale, and the pitch of the code rows it reads (a conv ahead: of a pixel)
    QDest dest() const { return QDest{act_.scale(), w_.relaid_c ? w_.relaid_cpitch : pitch_x(), /*sums=*/false}; }
    // int8 codes of x and their row sums (pooled), with this layer's scale
    struct Codes {
        std::shared_ptr<Buffer> q, rs;   // rs empty: the product sums the rows itself
        size_t batch = 0;
    };
    Codes encode(const Tensor &x) const {
        TAPER_ASSERT(x.shape().size() == 2 && x.shape()[1] == k_, "QuantizedLinear: input must be [batch, in_features]");
        TAPER_ASSERT(!w_.relaid_c, "QuantizedLinear: a layer behind a Flatten link takes codes");
        const size_t batch = x.shape()[0];
        Codes in{Buffer::alloc(std::max<size_t>(batch * pitch_x() / 4, 1)), Buffer::alloc(std::max<size_t>(batch, 1)), batch};
        TH(th_quantize_act_int8(Device::ctx(), x.dptr(), (int)batch, (int)k_, act_.scale(), reinterpret_cast<int8_t *>(in.q->d), (int)pitch_x(),
                                reinterpret_cast<int *>(in.rs->d)));
        return in;
    }
    struct Output {   // what the QDest asked for; the other member stays empty
        Tensor y;
        Codes codes;
    };
    // the integer product on codes made with this layer's scale, rows pitch_x() apart (behind a Flatten link: the hw * cpitch bytes of an image)
    Output product(const Codes &in, bool relu, QDest d = {}) const {
        const BiasPtrs b(b_);
        const size_t kk = w_.relaid_c ? w_.pitch : k_;   // code bytes of K a row (re-laid: the padded channels are zeros on both sides)
        Output out;
        float *y = nullptr;
        int8_t *qy = nullptr;
        if (d) {
            out.codes = Codes{Buffer::alloc(std::max<size_t>(in.batch * d.pitch / 4, 1)), nullptr, in.batch};
            qy = reinterpret_cast<int8_t *>(out.codes.q->d);
        } else {
            out.y = Tensor::empty({in.batch, n_});
            y = out.y.dptr();
        }
        TH(th_linear_q8q8_fwd_link(Device::ctx(), reinterpret_cast<const int8_t *>(in.q->d), (int)pitch_x(), in.rs ? reinterpret_cast<const int *>(in.rs->d) : nullptr,
                                   act_.scale(), (int)in.batch, (int)kk, reinterpret_cast<const int8_t *>(w_.codes->d), (int)w_.pitch, (int)n_, w_.params->d,
                                   w_.per_channel() ? 1 : 0, b.i8(), b.params, relu ? 1 : 0, y, d.scale, qy, (int)d.pitch));
        return out;
    }
    Tensor forward(const Tensor &x) const override { return forward_relu(x, false); }
    // x . deq(W)^T + deq(b), and the ReLU behind it in the same launch when the Sequential twin pairs them
    Tensor forward_relu(const Tensor &x, bool relu) const {
        TAPER_ASSERT(x.shape().size() == 2 && x.shape()[1] == k_, "QuantizedLinear: input must be [batch, in_features]");
        TAPER_ASSERT(!w_.relaid_c, "QuantizedLinear: a layer behind a Flatten link takes codes");
        const size_t batch = x.shape()[0];
        Tensor y = Tensor::empty({batch, n_});
        th_ctx *ctx = Device::ctx();
        const BiasPtrs b(b_);
        if (act_) {   // int8 codes of x and their row sums (pooled, returned when this scope ends), then the integer product
            const size_t pitch = (k_ + 15) / 16 * 16;
            auto qx = Buffer::alloc(batch * pitch / 4), rs = Buffer::alloc(batch);
            TH(th_quantize_act_int8(ctx, x.dptr(), (int)batch, (int)k_, act_.scale(), reinterpret_cast<int8_t *>(qx->d), (int)pitch, reinterpret_cast<int *>(rs->d)));
            const auto product = w_.per_channel() ? th_linear_q8q8_fwd_pc : th_linear_q8q8_fwd;   // (a pair per row, or one)
            TH(product(ctx, reinterpret_cast<const int8_t *>(qx->d), (int)pitch, reinterpret_cast<const int *>(rs->d), act_.scale(), (int)batch, (int)k_,
                       reinterpret_cast<const int8_t *>(w_.codes->d), (int)w_.pitch, (int)n_, w_.params->d, b.i8(), b.params, relu ? 1 : 0, y.dptr()));
        } else if (w_.qtype == TH_QTYPE_INT8)
            TH(th_linear_q8_fwd(ctx, x.dptr(), (int)batch, (int)k_, reinterpret_cast<const int8_t *>(w_.codes->d), (int)n_, w_.params->d, b.i8(), b.params,
                                relu ? 1 : 0, y.dptr()));
        else
            TH(th_linear_h16_fwd(ctx, x.dptr(), (int)batch, (int)k_, reinterpret_cast<const uint16_t *>(w_.codes->d), (int)n_,
                                 static_cast<const uint16_t *>(b.codes), relu ? 1 : 0, y.dptr()));
        return y;
    }
    void tensors(std::vector<const QTensor *> *out) const override {
        out->push_back(&w_);
        if (b_) out->push_back(b_.get());
    }
    void act_scales(std::vector<const float *> *out) const override { act_.list(out); }
    void calibrations(std::vector<ActCalibration> *out) const override { act_.list(out); }
    const ActScale &act() const { return act_; }

   private:
    // bytes from one row of input codes to the next: in_features rounded up to a piece; behind a Flatten link the image's hw * cpitch
    size_t pitch_x() const { return w_.relaid_c ? w_.pitch : (k_ + 15) / 16 * 16; }
    QTensor w_;
    std::unique_ptr<QTensor> b_;
    size_t k_, n_;
    ActScale act_;                     // static only
    std::shared_ptr<Buffer> packed_;   // the packed codes, while the links are being resolved
};

// A BatchNorm2d frozen on its running pair: {a, b} per channel, made on the device when the twin is made -- a snapshot, the
// source goes on training.  Behind a static conv the conv's epilogue applies it (QSequential::resolve); anywhere else forward() does.
class QBatchNorm : public QuantizedModule {
   public:
    explicit QBatchNorm(const BatchNorm2d &b) : c_(b.num_features), relu_(b.fuse_relu), affine_(Buffer::alloc(2 * b.num_features)) {
        TH(th_fold_batchnorm2d(Device::ctx(), b.gamma.dptr(), b.beta.dptr(), b.running_mean.dptr(), b.running_var.dptr(), b.eps, (int)c_, affine_->d));
    }
    Tensor forward(const Tensor &x) const override {
        TAPER_ASSERT(x.shape().size() == 4 && x.shape()[1] == c_, "QuantizedBatchNorm2d: input must be [batch, num_features, h, w]");
        const size_t hw = x.shape()[2] * x.shape()[3];
        TAPER_ASSERT(x.shape()[0] <= 0x7fffffffu && hw <= 0x7fffffffu, "QuantizedBatchNorm2d: input too large");
        Tensor y = Tensor::empty(x.shape());
        TH(th_channel_affine_fwd(Device::ctx(), x.dptr(), affine_->d, (int)x.shape()[0], (int)c_, (int)hw, relu_ ? 1 : 0, y.dptr()));
        return y;
    }
    void affines(std::vector<std::pair<const float *, size_t>> *out) const override { out->push_back({affine_->d, c_}); }
    const float *pairs() const { return affine_->d; }
    size_t channels() const { return c_; }
    bool fuse_relu() const { return relu_; }

   private:
    size_t c_;
    bool relu_;
    std::shared_ptr<Buffer> affine_;   // [c][2] = {a, b}
};

// an activation as channel-last int8 codes [n][h][w][cpitch] with the int32 sum of every pixel's codes: what a static conv's product reads
struct QCodes {
    std::shared_ptr<Buffer> q, sums;   // (pooled: they go back when the last holder lets go)
    size_t n = 0, c = 0, h = 0, w = 0, cpitch = 0;
    int8_t *codes() const { return reinterpret_cast<int8_t *>(q->d); }
    int *pixsum() const { return reinterpret_cast<int *>(sums->d); }
    static QCodes alloc(size_t n, size_t c, size_t h, size_t w, size_t cpitch) {
        return QCodes{Buffer::alloc(std::max<size_t>(n * h * w * cpitch / 4, 1)), Buffer::alloc(std::max<size_t>(n * h * w, 1)), n, c, h, w, cpitch};
    }
};

// what a static conv's product folds into its epilogue: a ReLU behind the layer (its own is added there), and a frozen BatchNorm2d right
// behind the layer (whose own ReLU is off), applied before that ReLU
struct QEpilogue {
    bool relu = false;
    const QBatchNorm *bn = nullptr;
};
// a block's shortcut in the last conv's epilogue: an f32 map of the output's shape (a projected shortcut), or the codes the
// block's first conv read with their scale (the identity shortcut); exactly one when set
struct QResidual {
    const Tensor *map = nullptr;
    const QCodes *codes = nullptr;
    const float *scale = nullptr;
    explicit operator bool() const { return map || codes; }
};
class QConv : public QuantizedModule {   // nn.rs:336-429 (Conv2dReLU, 481-504: the same with the ReLU fused)
   public:
    // The integer product is a convolution, so it stands in for the float layer only where the float path is one: 3x3, stride 1, one
    // group, no dilation (th_conv3x3_fwd, with the weight buffer read as [c_in k_h k_w][c_out]: tensor.rs:1262).  The float 1x1 and general
    // paths keep the reference's scrambled gathers (tensor.rs:1799-1801, 1931): a twin of those stays weight-only, on the same kernels.
    // exact (QuantizeOptions::blocks): the exact strided 3x3 and the exact pointwise convs are convolutions as well, on the same
    // weight_layout 0 buffer, so the product stands in for them through the same re-lay
    static bool can_be_static(const Conv2d &c, bool exact = false) {
        const Shape &ws = c.weight.shape();
        if (exact && (c.exact_stride || c.exact_pointwise)) return true;   // (the constructor fixed their geometry: one group, no dilation)
        return c.groups == 1 && c.dilation == std::make_pair(1, 1) && c.stride == std::make_pair(1, 1) && ws[2] == 3 && ws[3] == 3;
    }
    // o.convs: the static int8 twin (quantize_static with convs) -- the weight codes re-laid once channel-last for the product (an internal
    // copy: tensors() keeps reporting the packed codes), and one activation scale on the device that calibration fixes; o.per_channel
    // (static only): one weight pair per effective output channel co, whose elements lie at (ci taps + tap) c_out + co of the buffer
    QConv(const Conv2d &c, int qtype, QuantizeOptions o = {})
        : geom_(std::make_shared<Conv2d>(c)),
          w_(o.convs && o.per_channel && can_be_static(c, o.blocks) ? quantize_channels(c.weight, c.weight.shape()[0], 1, c.weight.shape()[0]) : quantize_tensor(c.weight, qtype)) {
        if (c.bias.defined()) b_ = std::make_unique<QTensor>(quantize_tensor(c.bias, qtype));
        geom_->weight = Tensor();   // the twin keeps the geometry only, not the source's f32 storage
        geom_->bias = Tensor();
        if (!o.convs || !can_be_static(c, o.blocks)) return;
        const Shape &ws = w_.shape;   // [c_out, c_in, k_h, k_w]
        cpitch_ = (size_t)th_qconv_i8_cpitch((int)ws[1]);
        relaid_ = Buffer::alloc(ws[0] * ws[2] * ws[3] * cpitch_ / 4);
        TH(th_pack_conv_weight_taper_int8(Device::ctx(), reinterpret_cast<const int8_t *>(w_.codes->d), (int)ws[0], (int)ws[1], (int)ws[2], (int)ws[3],
                                    reinterpret_cast<int8_t *>(relaid_->d), (int)cpitch_));
        act_.alloc();
    }
    bool is_static() const { return (bool)act_; }
    size_t out_channels() const { return w_.shape[0]; }
    bool own_relu() const { return geom_->fuse_relu; }
    // the codec: codes and pixel sums of x with this layer's scale
    QCodes encode(const Tensor &x) const {
        const Shape &ws = w_.shape;
        TAPER_ASSERT(x.shape().size() == 4 && x.shape()[1] == ws[1], "QuantizedConv2d: input must be [batch, in_channels, h, w]");
        QCodes in = QCodes::alloc(x.shape()[0], ws[1], x.shape()[2], x.shape()[3], cpitch_);
        TH(th_quantize_act_nhwc_int8(Device::ctx(), x.dptr(), (int)in.n, (int)in.c, (int)in.h, (int)in.w, act_.scale(), in.codes(), (int)cpitch_, in.pixsum()));
        return in;
    }
    struct Output {   // what the QDest asked for; the other member stays empty
        Tensor y;
        QCodes codes;
    };
    QDest dest(bool sums) const { return QDest{act_.scale(), cpitch_, sums}; }   // this layer as the destination of the product ahead
    // the integer product on codes made with this layer's scale; `r`: a block's shortcut, added behind e.bn and in front of the ReLU
    Output product(const QCodes &in, QEpilogue e, QDest d = {}, QResidual r = {}) const {
        const Shape &ws = w_.shape;
        TAPER_ASSERT(in.c == ws[1] && in.cpitch == cpitch_, "QuantizedConv2d: input must be [batch, in_channels, h, w]");
        const int sh = geom_->stride.first, sw = geom_->stride.second, ph = geom_->padding.first, pw = geom_->padding.second;
        TAPER_ASSERT(in.h + 2 * ph >= ws[2] && in.w + 2 * pw >= ws[3], "QuantizedConv2d: the kernel is larger than the padded input");
        const size_t ho = (in.h + 2 * ph - ws[2]) / sh + 1, wo = (in.w + 2 * pw - ws[3]) / sw + 1;
        const BiasPtrs b(b_);
        const int fold = e.relu || geom_->fuse_relu ? 1 : 0, pc = w_.per_channel() ? 1 : 0;   // (pc: a pair per output channel, or one)
        TAPER_ASSERT(!e.bn || (e.bn->channels() == ws[0] && !geom_->fuse_relu), "QuantizedConv2d: a BatchNorm2d of another width, or behind a fused ReLU");
        // every entry point takes the same operands and then its own tail
        auto run = [&](auto entry, auto... tail) {
            TH(entry(Device::ctx(), in.codes(), (int)cpitch_, in.pixsum(), act_.scale(), (int)in.n, (int)ws[1], (int)in.h, (int)in.w,
                     reinterpret_cast<const int8_t *>(relaid_->d), (int)ws[0], (int)ws[2], (int)ws[3], sh, sw, ph, pw, w_.params->d, b.i8(), b.params, fold, tail...));
        };
        Output out;
        if (r) {   // th_conv2d_q8q8_fwd_residual / _codes_residual: the affine entries' lists, then the residual's four
            TAPER_ASSERT(e.bn, "QuantizedConv2d: a residual needs a BatchNorm2d in the epilogue");
            const bool fits = r.map ? r.map->shape() == Shape{in.n, ws[0], ho, wo} : r.codes->n == in.n && r.codes->c == ws[0] && r.codes->h == ho && r.codes->w == wo;
            TAPER_ASSERT(fits, "QuantizedConv2d: the residual's shape differs from the output's");
            const float *map = r.map ? r.map->dptr() : nullptr;
            const int8_t *codes = r.codes ? r.codes->codes() : nullptr;
            const int cpitch_r = r.codes ? (int)r.codes->cpitch : 0;
            if (!d) {
                out.y = Tensor::empty({in.n, ws[0], ho, wo});
                run(th_conv2d_q8q8_fwd_residual, out.y.dptr(), pc, e.bn->pairs(), map, codes, cpitch_r, r.scale);
            } else {
                QCodes &q = out.codes = QCodes::alloc(in.n, ws[0], ho, wo, d.pitch);
                run(th_conv2d_q8q8_fwd_codes_residual, d.scale, q.codes(), (int)q.cpitch, d.sums ? q.pixsum() : nullptr, pc, e.bn->pairs(), map, codes, cpitch_r,
                    r.scale);
            }
            return out;
        }
        if (!d) {
            out.y = Tensor::empty({in.n, ws[0], ho, wo});
            if (e.bn) run(th_conv2d_q8q8_fwd_affine, out.y.dptr(), pc, e.bn->pairs());
            else run(pc ? th_conv2d_q8q8_fwd_pc : th_conv2d_q8q8_fwd, out.y.dptr());
            return out;
        }
        QCodes &q = out.codes = QCodes::alloc(in.n, ws[0], ho, wo, d.pitch);
        int *sums = d.sums ? q.pixsum() : nullptr;
        if (e.bn) run(th_conv2d_q8q8_fwd_codes_affine, d.scale, q.codes(), (int)q.cpitch, sums, pc, e.bn->pairs());
        else run(pc ? th_conv2d_q8q8_fwd_codes_pc : th_conv2d_q8q8_fwd_codes, d.scale, q.codes(), (int)q.cpitch, sums);
        return out;
    }
    void act_scales(std::vector<const float *> *out) const override { act_.list(out); }
    void calibrations(std::vector<ActCalibration> *out) const override { act_.list(out); }
    const ActScale &act() const { return act_; }
    Tensor forward(const Tensor &x) const override {   // alone: dequantize its own two tensors
        if (is_static()) return product(encode(x), {}).y;   // two launches: the codec (its buffers pooled, returned with this expression), then the product
        std::vector<const QConv *> one{this};
        std::vector<std::pair<float *, float *>> at;
        auto ws = dequantize(one, &at);
        return forward_with(x, at[0].first, at[0].second);
    }
    // nn.rs:336-429 on weights another call dequantized (d_w, d_b: slices of that call's workspace)
    Tensor forward_with(const Tensor &x, float *d_w, float *d_b) const {
        return geom_->forward_with(x, Tensor::from_device(d_w, w_.shape), d_b ? Tensor::from_device(d_b, b_->shape) : Tensor());
    }
    void tensors(std::vector<const QTensor *> *out) const override {
        out->push_back(&w_);
        if (b_) out->push_back(b_.get());
    }
    // ONE launch (th_dequantize_multi) for the weights and biases of `convs` into one pooled workspace; at[i] = {weight, bias} of convs[i]
    static std::shared_ptr<Buffer> dequantize(const std::vector<const QConv *> &convs, std::vector<std::pair<float *, float *>> *at) {
        auto up = [](size_t n) { return (n + 15) / 16 * 16; };   // 64-byte aligned slices
        size_t total = 0;
        for (const QConv *c : convs) total += up(c->w_.n) + (c->b_ ? up(c->b_->n) : 0);
        auto ws = Buffer::alloc(total);
        std::vector<th_qtensor> items;
        size_t off = 0;
        for (const QConv *c : convs) {
            float *dw = ws->d + off, *db = nullptr;
            items.push_back(c->w_.item(dw));
            off += up(c->w_.n);
            if (c->b_) {
                db = ws->d + off;
                items.push_back(c->b_->item(db));
                off += up(c->b_->n);
            }
            at->push_back({dw, db});
        }
        TH(th_dequantize_multi(Device::ctx(), items.data(), (int)items.size()));
        return ws;
    }

   private:
    std::shared_ptr<Conv2d> geom_;
    QTensor w_;
    std::unique_ptr<QTensor> b_;
    std::shared_ptr<Buffer> relaid_;   // static only: [c_out][k_h k_w][cpitch] codes
    ActScale act_;                     // static only
    size_t cpitch_ = 0;
};

// MaxPool2d on codes: a maximum commutes with the codec, so these are the codes of the pooled float map
QCodes max_pool_codes(const QCodes &in, const MaxPool2d &mp) {
    const std::pair<int, int> k = mp.kernel, s = mp.stride.first == 0 ? mp.kernel : mp.stride, p = mp.padding;   // (Tensor::max_pool2d's default)
    TAPER_ASSERT(k.first > 0 && k.second > 0 && in.h + 2 * p.first >= (size_t)k.first && in.w + 2 * p.second >= (size_t)k.second, "max_pool2d: bad geometry");
    QCodes out = QCodes::alloc(in.n, in.c, (in.h + 2 * p.first - k.first) / s.first + 1, (in.w + 2 * p.second - k.second) / s.second + 1, in.cpitch);
    TH(th_maxpool2d_nhwc_int8(Device::ctx(), in.codes(), (int)in.n, (int)in.c, (int)in.h, (int)in.w, (int)in.cpitch, k.first, k.second, s.first, s.second,
                              p.first, p.second, out.codes(), out.pixsum()));
    return out;
}

// A ResidualBlock or a BottleneckBlock as its twin sees it: the main branch's conv + BatchNorm2d pairs in order, and the projection's
// pair (null: the identity shortcut).  Empty for any other module.
struct BlockView {
    const char *name = nullptr;
    std::vector<std::pair<const Conv2d *, const BatchNorm2d *>> main;
    const Conv2d *proj = nullptr;
    const BatchNorm2d *proj_bn = nullptr;
    explicit operator bool() const { return name != nullptr; }
    std::vector<const Conv2d *> convs() const {   // in the order of the block's parameters()
        std::vector<const Conv2d *> out;
        for (const auto &p : main) out.push_back(p.first);
        if (proj) out.push_back(proj);
        return out;
    }
};
BlockView block_view(const Module &m) {
    BlockView v;
    if (auto *rb = dynamic_cast<const ResidualBlock *>(&m)) {
        v.name = "ResidualBlock";
        v.main = {{&rb->conv1, &rb->bn1}, {&rb->conv2, &rb->bn2}};
        v.proj = rb->shortcut_conv.get(), v.proj_bn = rb->shortcut_bn.get();
    } else if (auto *nb = dynamic_cast<const BottleneckBlock *>(&m)) {
        v.name = "BottleneckBlock";
        v.main = {{&nb->conv1, &nb->bn1}, {&nb->conv2, &nb->bn2}, {&nb->conv3, &nb->bn3}};
        v.proj = nb->shortcut_conv.get(), v.proj_bn = nb->shortcut_bn.get();
    }
    return v;
}

// The twin of a ResidualBlock or a BottleneckBlock (QuantizeOptions::blocks): the main branch as a run of static stages, each
// BatchNorm2d in its conv's epilogue, and the skip connection added in f32 in the last conv's epilogue behind its BatchNorm2d and in
// front of the ReLU -- where th_bn_residual_fwd adds it in the float block.  The block reads codes made with conv1's scale.  Identity
// shortcut: those codes are the residual (th_conv2d_q8q8_fwd_residual's d_res_q with conv1's scale) in every form of the twin.
// Projected shortcut: the projection is one more static stage on the same codes (its scale is conv1's bit for bit: both observed the
// same tensor), its BatchNorm2d in its epilogue, no ReLU, f32 out; the last stage takes that map (d_res).  With `chain` every boundary
// inside the main branch whose producing conv has at most th_qconv_i8_chain_max_cout() output channels is a link.
class QBlock : public QuantizedModule {
   public:
    QBlock(const BlockView &v, int qtype, QuantizeOptions o) {
        for (const auto &p : v.main) main_.push_back(Part{std::make_unique<QConv>(*p.first, qtype, o), std::make_unique<QBatchNorm>(*p.second)});
        if (v.proj) proj_ = Part{std::make_unique<QConv>(*v.proj, qtype, o), std::make_unique<QBatchNorm>(*v.proj_bn)};
        for (size_t i = 0; i + 1 < main_.size(); ++i) link_.push_back(o.chain && main_[i].conv->out_channels() <= (size_t)th_qconv_i8_chain_max_cout());
        for (const Part &p : main_) TAPER_ASSERT(p.conv->is_static(), std::string(v.name) + ": every conv of a block twin must be static");
    }
    const QConv &head() const { return *main_[0].conv; }   // the conv whose scale the block's input codes are made with
    const QConv &conv(size_t i) const { return *main_[i].conv; }
    const QConv *proj() const { return proj_.conv.get(); }
    size_t out_channels() const { return main_.back().conv->out_channels(); }
    // the block on the codes of its input (made with head()'s scale), into f32 or the next stage's codes
    QConv::Output run(const QCodes &in, QDest d = {}) const {
        Tensor shortcut;
        if (proj_.conv) shortcut = proj_.conv->product(in, QEpilogue{proj_.bn->fuse_relu(), proj_.bn.get()}).y;
        QCodes cur = in;
        for (size_t i = 0; i + 1 < main_.size(); ++i) {
            const Part &p = main_[i];
            const QConv &next = *main_[i + 1].conv;
            const QEpilogue e{p.bn->fuse_relu(), p.bn.get()};
            cur = link_[i] ? p.conv->product(cur, e, next.dest(/*sums=*/true)).codes : next.encode(p.conv->product(cur, e).y);
        }
        const Part &last = main_.back();
        const QResidual r = proj_.conv ? QResidual{&shortcut, nullptr, nullptr} : QResidual{nullptr, &in, head().act().scale()};
        return last.conv->product(cur, QEpilogue{last.bn->fuse_relu(), last.bn.get()}, d, r);
    }
    Tensor forward(const Tensor &x) const override { return run(head().encode(x)).y; }   // alone: one codec, then the stages
    void tensors(std::vector<const QTensor *> *out) const override { each([&](const Part &p) { p.conv->tensors(out); }); }
    void act_scales(std::vector<const float *> *out) const override { each([&](const Part &p) { p.conv->act_scales(out); }); }
    void calibrations(std::vector<ActCalibration> *out) const override { each([&](const Part &p) { p.conv->calibrations(out); }); }
    void affines(std::vector<std::pair<const float *, size_t>> *out) const override { each([&](const Part &p) { p.bn->affines(out); }); }
    int chain_links() const override { return (int)std::count(link_.begin(), link_.end(), true); }   // the inner boundaries crossed in int8
    void each_act(const std::function<void(const ActScale &)> &f) const { each([&](const Part &p) { f(p.conv->act()); }); }

   private:
    struct Part {
        std::unique_ptr<QConv> conv;
        std::unique_ptr<QBatchNorm> bn;
    };
    template <class F>
    void each(F f) const {   // conv1, conv2, [conv3], [projection]: the order of the source's parameters()
        for (const Part &p : main_) f(p);
        if (proj_.conv) f(proj_);
    }
    std::vector<Part> main_;
    Part proj_;
    std::vector<bool> link_;   // link_[i]: main_[i]'s product writes main_[i + 1]'s codes
};

class QSequential : public QuantizedModule {   // nn.rs:153-177
   public:
    std::vector<std::unique_ptr<QuantizedModule>> layers;
    // A static conv's place in a run: `fold.bn` = a frozen BatchNorm2d right behind it that its epilogue applies (a conv with a ReLU of
    // its own leaves the layer standing: the ReLU comes first there); `fold.relu` = the ReLU folded in behind both -- the BatchNorm's own
    // or a ReLU layer; with `chain`, whether a link starts here -- `pool` (or nullptr) and the static conv `next`, the run's next stage,
    // that takes the codes.
    // A block's twin is a stage as well: `block` instead of `conv`, nothing folded (its tail holds its own BatchNorm2d and
    // ReLU); it reads the codes made with its first conv's scale, so as `next` it is that conv.
    struct Stage {
        const QConv *conv = nullptr;
        const QBlock *block = nullptr;
        QEpilogue fold;
        const MaxPool2d *pool = nullptr;
        const QConv *next = nullptr;
    };
    // A static Linear's place in a run of them: `relu` = the ReLU layer behind it, in its epilogue
    struct LinStage {
        const QLinear *lin = nullptr;
        bool relu = false;
    };
    // What forward runs, in order; one of five kinds.  Every layer of `layers` belongs to exactly one step: the one that runs it or folds it.
    struct Step {
        const QuantizedModule *plain = nullptr;   // any other layer (a nested Sequential's twin among them): its own forward
        const QLinear *lin = nullptr;             // a Linear, `relu`: with the ReLU behind it in the same launch
        bool relu = false;
        const QConv *weight_only = nullptr;       // a weight-only conv, its weights at `slot` of the call's dequantize workspace
        size_t slot = 0;
        std::vector<Stage> run;                   // static convs: one codec, codes across every link, the last stage writes f32
        // with `links`, static Linears: the first takes f32 (one codec) or, behind `run` across a Flatten link (`flat`: the run's last stage
        // writes this Linear's codes, through `pool` if set, and the Flatten layer is folded), codes; every inner boundary is a link; the
        // last writes f32
        std::vector<LinStage> lrun;
        bool flat = false;
    };
    // The steps, once `layers` is complete: nothing they depend on changes afterwards (is_static() is fixed when a conv twin is made,
    // calibration only fills scales).  chain = quantize_static's chain: activations stay int8 across a link; links: through the Linears too.
    void resolve(bool chain, bool links = false) {
        auto pass = [&](size_t j) { return j < layers.size() ? dynamic_cast<const QPass *>(layers[j].get()) : nullptr; };
        auto stat = [&](size_t j) {
            auto *c = j < layers.size() ? dynamic_cast<const QConv *>(layers[j].get()) : nullptr;
            return c && c->is_static() ? c : nullptr;
        };
        auto blk = [&](size_t j) { return j < layers.size() ? dynamic_cast<const QBlock *>(layers[j].get()) : nullptr; };
        // the conv that reads the codes a stage at layer j takes: a static conv itself, a block's first conv
        auto head = [&](size_t j) -> const QConv * { return stat(j) ? stat(j) : blk(j) ? &blk(j)->head() : nullptr; };
        auto slin = [&](size_t j) {
            auto *l = j < layers.size() ? dynamic_cast<QLinear *>(layers[j].get()) : nullptr;
            return l && l->is_static() ? l : nullptr;
        };
        // the run of static Linears that begins at layer i: [ReLU] and the next static Linear directly behind is a link
        auto linear_run = [&](size_t &i, Step &s) {
            for (const QLinear *l = slin(i); l; l = slin(i)) {
                LinStage st{l, pass(i + 1) && pass(i + 1)->is_relu()};
                i += st.relu ? 2 : 1;
                s.lrun.push_back(st);
            }
        };
        for (size_t i = 0; i < layers.size();) {
            Step s;
            if (links && slin(i)) {
                linear_run(i, s);
            } else if ((s.lin = dynamic_cast<const QLinear *>(layers[i].get()))) {
                s.relu = pass(i + 1) && pass(i + 1)->is_relu();   // Linear + ReLU: one launch, the ReLU in its epilogue
                i += s.relu ? 2 : 1;
            } else if (head(i)) {   // conv + ReLU: the ReLU in the product's epilogue
                for (const QConv *hd = head(i); hd; hd = s.run.back().next) {
                    Stage st;
                    size_t after = i + 1;   // the first layer behind everything the stage folds
                    if ((st.block = blk(i))) {
                        // (a block folds nothing: a ReLU layer behind it would be its own ReLU a second time, and runs as a layer)
                    } else {
                        const QConv *cv = st.conv = hd;
                        if (!cv->own_relu() && after < layers.size() && (st.fold.bn = dynamic_cast<const QBatchNorm *>(layers[after].get()))) {
                            st.fold.relu = st.fold.bn->fuse_relu();
                            ++after;
                        }
                        if (pass(after) && pass(after)->is_relu()) {   // (behind a BatchNorm with a ReLU of its own: the same ReLU a second time)
                            st.fold.relu = true;
                            ++after;
                        }
                    }
                    i = after;
                    const size_t c = st.block ? st.block->out_channels() : st.conv->out_channels();
                    if (chain && c <= (size_t)th_qconv_i8_chain_max_cout()) {
                        size_t j = after;
                        if (pass(j) && pass(j)->max_pool()) st.pool = pass(j++)->max_pool();
                        QLinear *fl = links && pass(j) && pass(j)->flatten() && pass(j)->flatten()->start_dim == 1 ? slin(j + 1) : nullptr;
                        const size_t cpitch = (size_t)th_qconv_i8_cpitch((int)c);
                        if ((st.next = head(j))) {
                            i = j;   // a link: the run goes on there
                        } else if (fl && fl->in_features() % c == 0 && fl->in_features() / c * cpitch <= (size_t)th_q8q8_max_k()) {
                            fl->link_flatten(c, fl->in_features() / c, cpitch);   // a Flatten link: the Linears take over from there
                            s.flat = true;
                            i = j + 1;
                        } else {
                            st.pool = nullptr;   // (a pool counts only when a static conv or a Flatten link follows it)
                        }
                    }
                    s.run.push_back(st);
                }
                if (s.flat) linear_run(i, s);
            } else if ((s.weight_only = dynamic_cast<const QConv *>(layers[i].get()))) {
                s.slot = weight_only_.size();
                weight_only_.push_back(s.weight_only);
                ++i;
            } else {
                s.plain = layers[i++].get();
            }
            steps_.push_back(std::move(s));
        }
        for (auto &l : layers)
            if (auto *ql = dynamic_cast<QLinear *>(l.get())) ql->drop_packed();
    }
    Tensor forward(const Tensor &input) const override {
        // every weight-only conv step's weights in one dequantize launch, into one workspace that lives for this call
        std::vector<std::pair<float *, float *>> at;
        std::shared_ptr<Buffer> ws;
        if (!weight_only_.empty()) ws = QConv::dequantize(weight_only_, &at);
        Tensor x = input;
        for (const Step &s : steps_) {
            QLinear::Codes rows;   // what the Linear run reads
            if (s.lin) {
                x = s.lin->forward_relu(x, s.relu);
            } else if (s.weight_only) {
                x = s.weight_only->forward_with(x, at[s.slot].first, at[s.slot].second);
            } else if (s.plain) {
                x = s.plain->forward(x);
            } else if (!s.run.empty()) {   // a run: one codec, then codes from product to product (pooled buffers, each returned when `cur` moves on)
                QCodes cur = (s.run[0].block ? s.run[0].block->head() : *s.run[0].conv).encode(x);
                for (const Stage &st : s.run) {
                    const bool last = !st.next;
                    auto produce = [&](QDest d) { return st.block ? st.block->run(cur, d) : st.conv->product(cur, st.fold, d); };
                    if (last && !s.flat) {
                        x = produce({}).y;
                    } else {
                        QCodes out = produce(last ? s.lrun[0].lin->dest() : st.next->dest(/*sums=*/!st.pool)).codes;
                        cur = st.pool ? max_pool_codes(out, *st.pool) : out;
                    }
                }
                if (s.flat) {   // the map as rows of h w cpitch code bytes: what Flatten would give the Linear, channel-last
                    TAPER_ASSERT(cur.h * cur.w == s.lrun[0].lin->flat_hw(), "QuantizedLinear: input must be [batch, in_features]");
                    rows = QLinear::Codes{cur.q, nullptr, cur.n};
                }
            } else {
                rows = s.lrun[0].lin->encode(x);
            }
            for (size_t k = 0; k < s.lrun.size(); ++k) {   // codes from product to product, the last writes f32
                const LinStage &st = s.lrun[k];
                auto out = st.lin->product(rows, st.relu, k + 1 < s.lrun.size() ? s.lrun[k + 1].lin->dest() : QDest{});
                rows = out.codes;
                x = out.y;
            }
        }
        return x;
    }
    void tensors(std::vector<const QTensor *> *out) const override {
        for (const auto &l : layers) l->tensors(out);
    }
    void act_scales(std::vector<const float *> *out) const override {
        for (const auto &l : layers) l->act_scales(out);
    }
    void calibrations(std::vector<ActCalibration> *out) const override {
        for (const auto &l : layers) l->calibrations(out);
    }
    void affines(std::vector<std::pair<const float *, size_t>> *out) const override {
        for (const auto &l : layers) l->affines(out);
    }
    int chain_links() const override {
        int links = 0;
        for (const Step &s : steps_) {
            if (s.plain) links += s.plain->chain_links();
            for (const Stage &st : s.run)
                if (st.block) links += st.block->chain_links();   // the links inside a block's main branch
            links += (s.run.empty() ? 0 : (int)s.run.size() - 1) + (s.flat ? 1 : 0) + (s.lrun.empty() ? 0 : (int)s.lrun.size() - 1);
        }
        return links;
    }

   private:
    std::vector<Step> steps_;
    std::vector<const QConv *> weight_only_;   // the weight-only conv steps, by slot
};

// nn.rs:15: every module without a quantize() of its own (Dropout among them) panics.  batchnorm: whether BatchNorm2d and BasicBlock
// have one -- in the static twins; the weight-only quantize() keeps the reference's refusal.  blocks (QuantizeOptions::blocks,
// DESIGN 6t): the exact convs, and a ResidualBlock / BottleneckBlock whose convs are all convolutions, have one as well
void check_quantizable(const Module &m, bool batchnorm, bool blocks = false) {
    if (auto *s = dynamic_cast<const Sequential *>(&m)) {
        for (const auto &l : s->layers) check_quantizable(*l, batchnorm, blocks);
        return;
    }
    if (const BlockView v = block_view(m); v && blocks) {
        for (const Conv2d *c : v.convs())
            if (!QConv::can_be_static(*c, /*exact=*/true))
                throw Error(std::string(v.name) + ": the block holds a default strided or 1x1 Conv2d, whose float path is no convolution (SURVEY Q4 / Q9): " +
                            "build the block with exact_stride / pointwise_shortcut to quantize it");
        return;
    }
    // without `blocks` the exact convs keep their refusal (the int8 product of a default strided conv stands in for the general gather, Q9)
    const auto *cv = dynamic_cast<const Conv2d *>(&m);
    if (const auto *bb = dynamic_cast<const BasicBlock *>(&m)) cv = &bb->conv;
    if (cv && cv->exact_stride && !blocks) throw Error("exact-stride Conv2d: quantized twins are a follow-up");
    if (cv && cv->exact_pointwise && !blocks) throw Error("exact-pointwise Conv2d: quantized twins are a follow-up");
    if (dynamic_cast<const Linear *>(&m) || dynamic_cast<const Conv2d *>(&m) || dynamic_cast<const QATModule *>(&m) || dynamic_cast<const ReLU *>(&m) ||
        dynamic_cast<const Sigmoid *>(&m) || dynamic_cast<const MaxPool2d *>(&m) || dynamic_cast<const AvgPool2d *>(&m) ||
        dynamic_cast<const AdaptiveAvgPool2d *>(&m) || dynamic_cast<const Flatten *>(&m) ||
        (batchnorm && (dynamic_cast<const BatchNorm2d *>(&m) || dynamic_cast<const BasicBlock *>(&m))))
        return;
    throw Error("Quantization not implemented for this module type");
}

template <class M>
std::shared_ptr<Module> copy_of(const Module &m) {
    auto *p = dynamic_cast<const M *>(&m);
    return p ? std::make_shared<M>(*p) : nullptr;
}

// The leaf layers of `m` as the twin sees them, in order: a Sequential gives its children, a BasicBlock its conv and its BatchNorm2d (so
// that a link can cross the block's boundary), a QAT layer its inner layer (it deploys as that: qat_layers.rs:126-133, the packed codes
// are the fake-quantized weights it trained with).  A nested Sequential is one leaf: it stays a twin of its own.
std::vector<const Module *> leaves_of(const Module &m) {
    std::vector<const Module *> out;
    auto leaf = [&](const Module &l) {
        if (auto *bb = dynamic_cast<const BasicBlock *>(&l)) out.insert(out.end(), {&bb->conv, &bb->bn});
        else if (auto *ql = dynamic_cast<const QATLinear *>(&l)) out.push_back(&ql->inner);
        else if (auto *qc = dynamic_cast<const QATConv2d *>(&l)) out.push_back(&qc->inner);
        else out.push_back(&l);
    };
    if (auto *s = dynamic_cast<const Sequential *>(&m))
        for (const auto &l : s->layers) leaf(*l);
    else
        leaf(m);
    return out;
}

// nested: `m` is a layer of a Sequential twin in the making (which resolves the links of its layers when they are complete)
std::unique_ptr<QuantizedModule> quantize_checked(const Module &m, int qtype, QuantizeOptions o = {}, bool nested = false) {
    const std::vector<const Module *> leaves = leaves_of(m);
    if (dynamic_cast<const Sequential *>(&m) || leaves.size() > 1) {   // (more than one leaf of another module: a Sequential twin of them)
        auto q = std::make_unique<QSequential>();
        for (const Module *l : leaves) q->layers.push_back(quantize_checked(*l, qtype, o, /*nested=*/true));
        q->resolve(o.chain, o.links);
        return q;
    }
    const Module &l = *leaves[0];
    if (auto *bn = dynamic_cast<const BatchNorm2d *>(&l)) return std::make_unique<QBatchNorm>(*bn);
    if (auto *lin = dynamic_cast<const Linear *>(&l)) return std::make_unique<QLinear>(*lin, qtype, o, /*keep_packed=*/nested && o.links && o.chain);
    if (auto *c = dynamic_cast<const Conv2d *>(&l)) return std::make_unique<QConv>(*c, qtype, o);
    if (const BlockView v = block_view(l); v && o.blocks) return std::make_unique<QBlock>(v, qtype, o);
    std::shared_ptr<Module> p;
    if (!(p = copy_of<ReLU>(l)) && !(p = copy_of<Sigmoid>(l)) && !(p = copy_of<MaxPool2d>(l)) && !(p = copy_of<AvgPool2d>(l)) &&
        !(p = copy_of<AdaptiveAvgPool2d>(l)) && !(p = copy_of<Flatten>(l)))
        throw Error("Quantization not implemented for this module type");
    return std::make_unique<QPass>(p);
}

// the layers of type L of a model as quantize_checked meets them, nested Sequentials included
template <class L>
void layers_of(const Module &m, std::vector<const L *> *out) {
    for (const Module *l : leaves_of(m)) {
        if (auto *p = dynamic_cast<const L *>(l)) out->push_back(p);
        else if (l != &m) layers_of(*l, out);
        else if constexpr (std::is_same_v<L, Conv2d>)   // a block is one leaf: its convs are its twin's
            for (const Conv2d *c : block_view(*l).convs()) out->push_back(c);
    }
}

// One calibration tensor through the plain float layers of `m` (a QAT layer: its inner layer, whatever the QAT switch says), every
// Linear twin and every static conv twin in `q` shown its float input.  The parameters go in as views that require no gradient: no tape node is recorded.
// A Sequential twin's layers are the twins of leaves_of(m), one each and in that order (quantize_checked made them so).
// A BatchNorm2d runs in eval mode on its running pair whatever its flag says, by the kernel itself: the layer is only read.
// hist_bins > 0: pass two of the percentile calibration -- the same walk, every static layer adds its input to its histogram instead.
Tensor calibrate(const Module &m, const QuantizedModule &q, const Tensor &x, bool first, int hist_bins = 0) {
    auto plain = [](const Tensor &t) { return t.defined() ? Tensor::from_device(t.dptr(), t.shape()) : Tensor(); };
    const std::vector<const Module *> leaves = leaves_of(m);
    if (auto *qs = dynamic_cast<const QSequential *>(&q)) {
        TAPER_ASSERT(leaves.size() == qs->layers.size(), "calibrate: the twin is not this model's");
        Tensor h = x;
        auto twin = qs->layers.begin();
        for (const Module *l : leaves) h = calibrate(*l, **twin++, h, first, hist_bins);
        return h;
    }
    const Module &l = *leaves[0];
    // a BatchNorm2d in eval mode, by the kernels themselves; with `residual` the skip connection added in the same map (th_bn_residual_fwd)
    auto bn_eval = [](const BatchNorm2d &bn, const Tensor &x, const Tensor *residual) {
        TAPER_ASSERT(x.shape().size() == 4 && x.shape()[1] == bn.num_features, "BatchNorm2d: expected a 4-D input [N, num_features, H, W]");
        TAPER_ASSERT(!residual || residual->shape() == x.shape(), "BatchNorm2d: the residual's shape differs from the input's");
        const size_t hw = x.shape()[2] * x.shape()[3];
        TAPER_ASSERT(x.shape()[0] <= 0x7fffffffu && hw <= 0x7fffffffu, "BatchNorm2d: input too large");
        Tensor y = Tensor::empty(x.shape());
        auto saved = Buffer::alloc(2 * bn.num_features);
        const int n = (int)x.shape()[0], c = (int)bn.num_features, relu = bn.fuse_relu ? 1 : 0;
        if (residual)
            TH(th_bn_residual_fwd(Device::ctx(), x.dptr(), residual->dptr(), bn.gamma.dptr(), bn.beta.dptr(), y.dptr(), bn.running_mean.dptr(),
                                  bn.running_var.dptr(), saved->d, saved->d + bn.num_features, n, c, (int)hw, bn.eps, bn.momentum, /*training=*/0, relu));
        else
            TH(th_batchnorm2d_fwd(Device::ctx(), x.dptr(), bn.gamma.dptr(), bn.beta.dptr(), y.dptr(), bn.running_mean.dptr(), bn.running_var.dptr(), saved->d,
                                  saved->d + bn.num_features, n, c, (int)hw, bn.eps, bn.momentum, /*training=*/0, relu));
        return y;
    };
    if (auto *bn = dynamic_cast<const BatchNorm2d *>(&l)) return bn_eval(*bn, x, nullptr);
    if (const BlockView v = block_view(l)) {   // the float block, every conv of its twin shown its input; conv1 and the projection see the same tensor
        auto &qb = dynamic_cast<const QBlock &>(q);
        auto see = [&](const QConv &qc, const Tensor &t) { hist_bins ? qc.act().observe_hist(t, hist_bins) : qc.act().observe(t, first); };
        auto conv = [&](const Conv2d &cv, const Tensor &t) { return cv.forward_with(t, plain(cv.weight), plain(cv.bias)); };
        Tensor shortcut = x, h = x;
        for (size_t i = 0; i < v.main.size(); ++i) {
            see(qb.conv(i), h);
            if (i + 1 < v.main.size()) {
                h = bn_eval(*v.main[i].second, conv(*v.main[i].first, h), nullptr);
                continue;
            }
            if (v.proj) {
                see(*qb.proj(), x);
                shortcut = bn_eval(*v.proj_bn, conv(*v.proj, x), nullptr);
            }
            h = bn_eval(*v.main[i].second, conv(*v.main[i].first, h), &shortcut);
        }
        return h;
    }
    if (auto *lin = dynamic_cast<const Linear *>(&l)) {
        const ActScale &act = dynamic_cast<const QLinear &>(q).act();
        hist_bins ? act.observe_hist(x, hist_bins) : act.observe(x, first);
        return x.linear(plain(lin->weight), plain(lin->bias), false);
    }
    if (auto *cv = dynamic_cast<const Conv2d *>(&l)) {
        auto &qcv = dynamic_cast<const QConv &>(q);
        if (qcv.is_static()) hist_bins ? qcv.act().observe_hist(x, hist_bins) : qcv.act().observe(x, first);
        return cv->forward_with(x, plain(cv->weight), plain(cv->bias));
    }
    return l.forward(x);
}

// every static layer's ActScale of a twin, nested Sequential twins included
void each_act_scale(const QuantizedModule &q, const std::function<void(const ActScale &)> &f) {
    if (auto *qs = dynamic_cast<const QSequential *>(&q)) {
        for (const auto &l : qs->layers) each_act_scale(*l, f);
    } else if (auto *l = dynamic_cast<const QLinear *>(&q)) {
        if (l->is_static()) f(l->act());
    } else if (auto *c = dynamic_cast<const QConv *>(&q)) {
        if (c->is_static()) f(c->act());
    } else if (auto *b = dynamic_cast<const QBlock *>(&q)) {
        b->each_act(f);
    }
}

}  // namespace

th_qtensor QTensor::item(float *d_out) const { return th_qtensor{codes->d, params ? params->d : nullptr, d_out, (int64_t)n, qtype}; }

std::unique_ptr<QuantizedModule> quantize(const Module &m, QType qtype, bool enabled) {
    check_quantizable(m, /*batchnorm=*/false);   // before anything is allocated
    int qt = TH_QTYPE_F16;  // tensor.rs:2085-2088: disabled quantization gives Float16
    if (enabled) {
        switch (qtype) {
            case QType::Int8: qt = TH_QTYPE_INT8; break;
            case QType::Float16: qt = TH_QTYPE_F16; break;
            case QType::Int4:
            case QType::BFloat16:
            case QType::NF4:   // tensor.rs:2154-2188: placeholders whose codes are all zero
                throw Error("Quantization type " + std::string(qtype == QType::Int4 ? "Int4" : qtype == QType::BFloat16 ? "BFloat16" : "NF4") +
                            " is not supported: the reference's codec for it is a placeholder that returns zeros");
            default: throw Error("unknown quantization type");
        }
    }
    return quantize_checked(m, qt);
}

std::unique_ptr<QuantizedModule> quantize_static(const Module &m, const std::vector<Tensor> &calib, QuantizeOptions o) {
    o.linears = true;
    o.convs = o.convs || o.chain;
    // every refusal before anything is allocated
    TAPER_ASSERT(!o.blocks || o.convs, "quantize_static: blocks needs convs (a block's twin is a run of static convs)");
    check_quantizable(m, /*batchnorm=*/true, o.blocks);
    const Calibration &cal = o.calibration;
    const bool percentile = cal.method == CalibMethod::Percentile;
    TAPER_ASSERT(percentile || cal.method == CalibMethod::MinMax, "quantize_static: unknown calibration method " + std::to_string((int)cal.method));
    if (percentile) {
        TAPER_ASSERT(cal.keep_ppm >= 1 && cal.keep_ppm <= 1000000, "quantize_static: keep_ppm must be in [1, 1000000] (got " + std::to_string(cal.keep_ppm) + ")");
        TAPER_ASSERT(cal.num_bins >= 16 && cal.num_bins <= th_act_hist_max_bins(),
                     "quantize_static: num_bins must be in [16, " + std::to_string(th_act_hist_max_bins()) + "] (got " + std::to_string(cal.num_bins) + ")");
    }
    TAPER_ASSERT(!calib.empty(), "quantize_static: at least one calibration tensor is needed");
    for (const Tensor &c : calib) TAPER_ASSERT(c.defined(), "quantize_static: undefined calibration tensor");
    std::vector<const Linear *> lins;
    layers_of(m, &lins);
    const size_t max_k = (size_t)th_q8q8_max_k();
    const std::string above = " is above " + std::to_string(max_k) + ", where the int32 sum of the int8 product can overflow";
    for (const Linear *l : lins)
        TAPER_ASSERT(l->weight.shape()[1] <= max_k, "quantize_static: a Linear with in_features " + std::to_string(l->weight.shape()[1]) + above);
    if (o.convs) {
        std::vector<const Conv2d *> cvs;
        layers_of(m, &cvs);
        for (const Conv2d *c : cvs) {
            const Shape &ws = c->weight.shape();
            TAPER_ASSERT(!QConv::can_be_static(*c, o.blocks) || ws[1] * ws[2] * ws[3] <= max_k,
                         "quantize_static: a Conv2d with in_channels * k_h * k_w = " + std::to_string(ws[1] * ws[2] * ws[3]) + above);
        }
    }
    auto q = quantize_checked(m, TH_QTYPE_INT8, o);
    NoGradScope no_grad;
    for (size_t i = 0; i < calib.size(); ++i) {
        Tensor x = Tensor::from_device(calib[i].dptr(), calib[i].shape());   // (a view that requires no gradient)
        calibrate(m, *q, x, i == 0);
    }
    if (percentile) {   // pass two against the final ranges, then one scale launch per static layer
        for (const Tensor &c : calib) calibrate(m, *q, Tensor::from_device(c.dptr(), c.shape()), false, cal.num_bins);
        each_act_scale(*q, [&](const ActScale &a) { a.scale_from_hist(cal.keep_ppm); });
    }
    return q;
}

}  // namespace taper
