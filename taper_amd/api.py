"""Python face of the host mirror (include/taper_host.h): the reference's
public surface -- src/lib.rs:1-17: Tensor, Tape, nn, loss, optim, data, train
-- with the reference's names and argument meaning.  Every call crosses the
C ABI into libtaper_host.so (C++), which reaches the GPU only through
libtaper_hip.so (hand-written HIP for gfx950).  No arithmetic happens here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import TaperError, host, tp_check

_p = C.c_void_p
EXACT_STRIDE = 1   # TP_CONV_EXACT_STRIDE: bit 0 of the flags word of tp_conv2d_ex and the *_new_ex constructors
EXACT_POINTWISE = 16   # TP_CONV_EXACT_POINTWISE: the exact 1x1 convolution (tp_residual_block_new_ex: the pointwise shortcut)


def _shape_arr(shape):
    return (C.c_size_t * len(shape))(*[int(s) for s in shape])


def _new_handle():
    return _p()


class Device:
    @staticmethod
    def set_device(i: int):
        tp_check(host.tp_device_set(int(i)), "tp_device_set")

    @staticmethod
    def sync():
        tp_check(host.tp_device_sync(), "tp_device_sync")

    @staticmethod
    def ctx_handle() -> int:
        h = host.tp_device_ctx()
        if not h:
            raise TaperError(host.tp_last_error().decode())
        return h


class Tape:
    """src/tape.rs"""

    @staticmethod
    def reset():
        tp_check(host.tp_tape_reset(), "tp_tape_reset")

    @staticmethod
    def len() -> int:
        n = C.c_size_t()
        tp_check(host.tp_tape_len(C.byref(n)), "tp_tape_len")
        return n.value

    @staticmethod
    def set_compat_zero_sentinel(on: bool):
        tp_check(host.tp_tape_set_compat_zero_sentinel(1 if on else 0), "tp_tape_set_compat_zero_sentinel")


def set_full_backward(on: bool):
    """False (default) = faithful to the reference (conv weights never get gradients, quirk Q2)."""
    tp_check(host.tp_set_full_backward(1 if on else 0), "tp_set_full_backward")


def set_conv_chain(on: bool):
    """Trainer steps: the convolutional front of a Sequential as ONE launch where an instance is compiled (default), or layer by layer"""
    tp_check(host.tp_set_conv_chain(1 if on else 0), "tp_set_conv_chain")


def set_conv_chain_head(on: bool):
    """Trainer steps: the classifier behind such a front row by row inside the same launch where compiled (default), or as its own launches"""
    tp_check(host.tp_set_conv_chain_head(1 if on else 0), "tp_set_conv_chain_head")


class Tensor:
    """src/tensor.rs Tensor: a shared handle to device storage + grad slot + tape node."""

    def __init__(self, data=None, shape=None, _h=None):
        if _h is not None:
            self._h = _h
            return
        a = np.ascontiguousarray(np.asarray(data, dtype=np.float32))
        if shape is None:
            shape = a.shape if a.ndim else (1,)
        a = a.reshape(-1)
        if a.size != int(np.prod(shape)):
            raise TaperError("Tensor::new: data length does not match shape")
        h = _p()
        tp_check(host.tp_tensor_new(a.ctypes.data, _shape_arr(shape), len(shape), C.byref(h)), "tp_tensor_new")
        self._h = h.value

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                host.tp_tensor_free(h)
            except Exception:
                pass

    @staticmethod
    def scalar(v):
        return Tensor([float(v)], (1,))

    @staticmethod
    def randn(shape, seed=0):
        h = _p()
        tp_check(host.tp_tensor_randn(_shape_arr(shape), len(shape), int(seed), C.byref(h)), "tp_tensor_randn")
        return Tensor(_h=h.value)

    def requires_grad(self):
        tp_check(host.tp_tensor_set_requires_grad(self._h, 1), "set_requires_grad")
        return self

    def clone(self):
        h = _p()
        tp_check(host.tp_tensor_clone(self._h, C.byref(h)), "tp_tensor_clone")
        return Tensor(_h=h.value)

    def shape(self):
        nd = C.c_int()
        tp_check(host.tp_tensor_ndim(self._h, C.byref(nd)), "tp_tensor_ndim")
        s = (C.c_size_t * 4)()
        tp_check(host.tp_tensor_shape(self._h, s), "tp_tensor_shape")
        return tuple(int(s[i]) for i in range(nd.value))

    def numel(self):
        n = C.c_size_t()
        tp_check(host.tp_tensor_len(self._h, C.byref(n)), "tp_tensor_len")
        return n.value

    def data(self) -> np.ndarray:
        out = np.empty(self.numel(), dtype=np.float32)
        tp_check(host.tp_tensor_data(self._h, out.ctypes.data), "tp_tensor_data")
        return out.reshape(self.shape())

    def set_data(self, a):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(-1)
        assert a.size == self.numel()
        tp_check(host.tp_tensor_set_data(self._h, a.ctypes.data), "tp_tensor_set_data")

    def grad(self):
        has = C.c_int()
        tp_check(host.tp_tensor_has_grad(self._h, C.byref(has)), "tp_tensor_has_grad")
        if not has.value:
            return None
        out = np.empty(self.numel(), dtype=np.float32)
        tp_check(host.tp_tensor_grad(self._h, out.ctypes.data), "tp_tensor_grad")
        return out.reshape(self.shape())

    grad_ref = grad

    def set_grad(self, g):
        if g is None:
            tp_check(host.tp_tensor_set_grad(self._h, None), "tp_tensor_set_grad")
        else:
            a = np.ascontiguousarray(np.asarray(g, dtype=np.float32)).reshape(-1)
            assert a.size == self.numel()
            tp_check(host.tp_tensor_set_grad(self._h, a.ctypes.data), "tp_tensor_set_grad")

    def tape_node(self):
        n = C.c_size_t()
        tp_check(host.tp_tensor_tape_node(self._h, C.byref(n)), "tp_tensor_tape_node")
        return n.value

    def dptr(self) -> int:
        p = _p()
        tp_check(host.tp_tensor_dptr(self._h, C.byref(p)), "tp_tensor_dptr")
        return p.value

    def backward(self):
        tp_check(host.tp_tensor_backward(self._h), "tp_tensor_backward")

    def zero_grad(self):
        tp_check(host.tp_tensor_zero_grad(self._h), "tp_tensor_zero_grad")

    # -- ops ---------------------------------------------------------------
    def _bin(self, fn, o, name):
        h = _p()
        tp_check(fn(self._h, o._h, C.byref(h)), name)
        return Tensor(_h=h.value)

    def _un(self, fn, name, *args):
        h = _p()
        tp_check(fn(self._h, *args, C.byref(h)), name)
        return Tensor(_h=h.value)

    def __add__(self, o): return self._bin(host.tp_add, o, "add")
    def __sub__(self, o): return self._bin(host.tp_sub, o, "sub")
    def __mul__(self, o): return self._bin(host.tp_mul, o, "mul")
    def __truediv__(self, o): return self._bin(host.tp_div, o, "div")
    def matmul(self, o): return self._bin(host.tp_matmul, o, "matmul")
    def add_broadcast(self, o): return self._bin(host.tp_add_broadcast, o, "add_broadcast")
    def sub_broadcast_rows(self, o): return self._bin(host.tp_sub_broadcast_rows, o, "sub_broadcast_rows")
    def relu(self): return self._un(host.tp_relu, "relu")
    def sigmoid(self): return self._un(host.tp_sigmoid, "sigmoid")
    def transpose(self): return self._un(host.tp_transpose, "transpose")
    def exp(self): return self._un(host.tp_exp, "exp")
    def log(self): return self._un(host.tp_log, "log")
    def mean(self): return self._un(host.tp_mean, "mean")
    def pow(self, e): return self._un(host.tp_pow, "pow", float(e))
    def sqrt(self): return self.pow(0.5)
    def sum(self, dim=None, keepdim=False): return self._un(host.tp_sum, "sum", -1 if dim is None else int(dim), 1 if keepdim else 0)
    def reshape(self, shape): return self._un(host.tp_reshape, "reshape", _shape_arr(shape), len(shape))
    view = reshape
    def flatten(self, start_dim): return self._un(host.tp_flatten, "flatten", int(start_dim))
    def squeeze(self, dim=None): return self._un(host.tp_squeeze, "squeeze", -1 if dim is None else int(dim))
    def slice_channels(self, start, end): return self._un(host.tp_slice_channels, "slice_channels", int(start), int(end))   # nn.rs:862-886

    @staticmethod
    def cat(tensors, dim):   # nn.rs:928-1014
        arr = (C.c_void_p * len(tensors))(*[t._h for t in tensors])
        out = _p()
        tp_check(host.tp_cat(arr, len(tensors), int(dim), C.byref(out)), "cat")
        return Tensor(_h=out.value)
    def unsqueeze(self, dim): return self._un(host.tp_unsqueeze, "unsqueeze", int(dim))

    def max(self, dim=None):
        v, i = _p(), _p()
        tp_check(host.tp_max(self._h, -1 if dim is None else int(dim), C.byref(v), C.byref(i)), "max")
        return Tensor(_h=v.value), Tensor(_h=i.value)

    def argmax(self, dim=None):
        return self.max(dim)[1]

    def linear(self, weight, bias=None, relu=False):
        return self._un(host.tp_linear, "linear", weight._h, bias._h if bias is not None else None, 1 if relu else 0)

    def conv2d(self, weight, bias, stride=(1, 1), padding=(0, 0), dilation=(1, 1), relu=False, exact_stride=False, exact_pointwise=False):
        """exact_stride: the exact 3x3 / stride (2, 2) / padding (1, 1) convolution, which takes weight and input gradients under
        set_full_backward(True); any other geometry with the flag is refused by name.  Without it a strided call keeps the reference's
        general gather, which is no convolution and has no gradient.
        exact_pointwise: the exact 1x1 convolution with stride (1, 1) or (2, 2) and no padding, with the same gradients; any other geometry
        with the flag, and both flags together, are refused by name.  Without it a 1x1 call keeps the reference's reinterpretation (SURVEY
        Q4), which is no convolution for more than one input channel, takes no stride and has no gradient."""
        b = bias._h if bias is not None else None
        if exact_stride or exact_pointwise:
            return self._un(host.tp_conv2d_ex, "conv2d", weight._h, b, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1],
                            1 if relu else 0, (EXACT_STRIDE if exact_stride else 0) | (EXACT_POINTWISE if exact_pointwise else 0))
        return self._un(host.tp_conv2d, "conv2d", weight._h, b, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1],
                        1 if relu else 0)

    def conv2d_relu(self, weight, bias, stride=(1, 1), padding=(0, 0), dilation=(1, 1), exact_stride=False, exact_pointwise=False):
        return self.conv2d(weight, bias, stride, padding, dilation, relu=True, exact_stride=exact_stride, exact_pointwise=exact_pointwise)

    def max_pool2d(self, kernel_size, stride=None, padding=(0, 0)):
        s = stride or (0, 0)
        return self._un(host.tp_max_pool2d, "max_pool2d", kernel_size[0], kernel_size[1], s[0], s[1], padding[0], padding[1])

    def avg_pool2d(self, kernel_size, stride=None, padding=(0, 0)):
        s = stride or (0, 0)
        return self._un(host.tp_avg_pool2d, "avg_pool2d", kernel_size[0], kernel_size[1], s[0], s[1], padding[0], padding[1])


# -- src/loss.rs ------------------------------------------------------------
def _t1(fn, name, x, *args):
    h = _p()
    tp_check(fn(x._h, *args, C.byref(h)), name)
    return Tensor(_h=h.value)


def log_softmax(x, dim=-1): return _t1(host.tp_log_softmax, "log_softmax", x)
def softmax(x, dim=-1): return _t1(host.tp_softmax, "softmax", x)
def cross_entropy_loss(logits, targets): return _t1(host.tp_cross_entropy_loss, "cross_entropy_loss", logits, targets._h)
def one_hot(idx, num_classes): return _t1(host.tp_one_hot, "one_hot", idx, int(num_classes))
def mse_loss(pred, targets): return _t1(host.tp_mse_loss, "mse_loss", pred, targets._h)
def bce_loss(pred, targets): return _t1(host.tp_bce_loss, "bce_loss", pred, targets._h)
def cross_entropy_loss_onehot(logits, targets): return _t1(host.tp_cross_entropy_loss_onehot, "cross_entropy_loss_onehot", logits, targets._h)


def accuracy(pred, targets) -> float:
    out = C.c_float()
    tp_check(host.tp_accuracy(pred._h, targets._h, C.byref(out)), "accuracy")
    return float(out.value)


_QSTATIC_CONVS, _QSTATIC_CHAIN, _QSTATIC_PER_CHANNEL, _QSTATIC_LINKS = 1, 2, 4, 16      # include/taper_host.h's TP_QSTATIC_* flags
_QBLOCKS = 32                                                                           # ... its TP_QBLOCKS (residual models)
_CALIB_MINMAX, _CALIB_PERCENTILE = 0, 1                                               # ... and its TP_CALIB_* methods


# -- src/nn.rs, src/activation.rs ------------------------------------------------
class Module:
    def __init__(self, h):
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            host.tp_module_free(h)

    def forward(self, x: Tensor) -> Tensor:
        h = _p()
        tp_check(host.tp_module_forward(self._h, x._h, C.byref(h)), "forward")
        return Tensor(_h=h.value)

    def parameters(self):
        n = C.c_int()
        tp_check(host.tp_module_num_parameters(self._h, C.byref(n)), "num_parameters")
        out = []
        for i in range(n.value):
            h = _p()
            tp_check(host.tp_module_parameter(self._h, i, C.byref(h)), "parameter")
            out.append(Tensor(_h=h.value))
        return out

    def buffers(self):
        """state that is saved but not trained (BatchNorm2d's running statistics), children's concatenated; shares storage with the model"""
        n = C.c_int()
        tp_check(host.tp_module_num_buffers(self._h, C.byref(n)), "num_buffers")
        out = []
        for i in range(n.value):
            h = _p()
            tp_check(host.tp_module_buffer(self._h, i, C.byref(h)), "buffer")
            out.append(Tensor(_h=h.value))
        return out

    def train(self):
        """training mode for every BatchNorm2d and every Dropout inside this module"""
        tp_check(host.tp_module_set_training(self._h, 1), "Module::train")

    def eval(self):
        tp_check(host.tp_module_set_training(self._h, 0), "Module::eval")

    def quantize(self, qtype="int8", enabled=True):
        """nn.rs:14-23 Module::quantize -> QuantizedModule (post-training, on the device; this model is not touched).
        qtype: "int8" | "float16" ("int4", "bfloat16", "nf4" are placeholders in the reference and are refused);
        enabled=False gives float16 (tensor.rs:2085-2088)."""
        code = QuantizedModule.QTYPES.get(qtype)
        if code is None:
            raise TaperError(f"quantize: unknown qtype {qtype!r}")
        h = _p()
        tp_check(host.tp_module_quantize(self._h, code, 1 if enabled else 0, C.byref(h)), "Module::quantize")
        return QuantizedModule(h.value)

    def quantize_static(self, calib):
        """Static int8 post-training quantization -> QuantizedModule: the weights packed as quantize("int8") packs them, and one activation
        scale per Linear from the float model's activations on `calib` (a Tensor or a sequence of them).  Linear layers then run
        int8 x int8 on the integer matrix cores at every batch size; this model is only read."""
        return self._quantize_static(host.tp_module_quantize_static, "quantize_static", calib)

    def quantize_static_conv(self, calib):
        """quantize_static with the convolutions static too: every 3x3, stride-1 Conv2d / Conv2dReLU with one group gets its own activation
        scale and runs int8 x int8 as an implicit GEMM on the integer matrix cores (any other conv stays weight-only).
        act_scales() lists one scale per static layer, Linear or conv, in layer order; tensors() is quantize("int8")'s."""
        return self._quantize_static(host.tp_module_quantize_static_conv, "quantize_static_conv", calib)

    def quantize_static_chain(self, calib):
        """quantize_static_conv whose activations stay int8 from one static conv to the next: a conv of at most 128 output channels writes
        the next conv's codes from its epilogue, and one MaxPool2d between the two runs on the codes.  The same scales, tensors and, on
        finite activations, the same output bits as quantize_static_conv's twin; chain_links() counts the boundaries crossed in int8."""
        return self._quantize_static(host.tp_module_quantize_static_chain, "quantize_static_chain", calib)

    def quantize_static_per_channel(self, calib, convs=True, chain=True):
        """quantize_static / quantize_static_conv / quantize_static_chain (by `convs` and `chain`) with one {min_val, scale} pair per output
        channel for the weight of every static layer: a Linear's rows, a static conv's effective output channels.  Biases and every layer
        that stays weight-only keep one pair; act_scales() and chain_links() are the per-tensor twin's.  tensors() gives such a weight's
        pairs as an ndarray of shape (channels, 2), channel_layout(i) where a channel's codes lie."""
        flags = (_QSTATIC_CONVS if convs or chain else 0) | (_QSTATIC_CHAIN if chain else 0) | _QSTATIC_PER_CHANNEL
        return self._quantize_static(host.tp_module_quantize_static_ex, "quantize_static_per_channel", calib, flags)

    def quantize_static_linked(self, calib, per_channel=False):
        """quantize_static_chain whose activations stay int8 through the classifier as well: a conv run's last stage (at most 128 output
        channels, optionally one MaxPool2d, then Flatten(1)) writes the first Linear's codes channel-last, and a Linear writes the codes of
        the Linear directly behind it (a ReLU between the two folded in) from its epilogue; a consumer sums its own rows.  One codec
        launch at the first static layer, no f32 tensor up to the logits.  The same scales, tensors and output bits as the twin without
        the links (per_channel: as quantize_static_per_channel's); chain_links() counts every boundary crossed in int8."""
        flags = _QSTATIC_CONVS | _QSTATIC_CHAIN | _QSTATIC_LINKS | (_QSTATIC_PER_CHANNEL if per_channel else 0)
        return self._quantize_static(host.tp_module_quantize_static_ex, "quantize_static_linked", calib, flags)

    def quantize_static_calibrated(self, calib, percentile=99.99, bins=2048, convs=True, chain=True, per_channel=False, links=False):
        """Any static twin (by `convs`, `chain`, `per_channel` and `links`, as the calls above) whose activation scales come from a
        percentile of each static layer's |input| over `calib` instead of its min / max: the calibration set runs twice, the second
        time into a histogram of `bins` bins per layer on the device, and each scale is the upper edge of the first bin that keeps
        `percentile` per cent of the layer's finite input elements, over 127 -- one outlier no longer sets the scale of a layer.
        keep_ppm = round(percentile * 1e4) must lie in [1, 1 000 000]; percentile=100 gives the min / max scales bit for bit.  Packing,
        tensors, links and refusals are those of the same flags; calibration() reports what each layer kept."""
        flags = ((_QSTATIC_CONVS if convs or chain else 0) | (_QSTATIC_CHAIN if chain else 0) | (_QSTATIC_PER_CHANNEL if per_channel else 0)
                 | (_QSTATIC_LINKS if links else 0))
        return self._quantize_static(host.tp_module_quantize_static_cal, "quantize_static_calibrated", calib, flags, _CALIB_PERCENTILE,
                                     int(round(float(percentile) * 1e4)), int(bins))

    def quantize_static_residual(self, calib, chain=True, per_channel=False, links=False, percentile=None, bins=2048):
        """The static conv twin of a residual model (TP_QBLOCKS with TP_QSTATIC_CONVS): the exact strided 3x3 and the exact 1x1 convs are
        static like the stride-1 3x3, and a ResidualBlock / BottleneckBlock built from such convs runs its main branch as static stages
        with the skip connection added in f32 inside the last conv's epilogue, y = max(((v * a) + b) + r, 0): r from the codes of the
        block's input (identity shortcut) or from the projection's f32 map.  `chain`: a block is a stage of the enclosing Sequential's
        run and the boundaries inside it are links; `per_channel`, `links` and `percentile` / `bins` combine as in the calls above
        (percentile=None: min / max calibration).  The same scales, tensors and output bits with and without `chain` / `links`.  A block
        with a default strided or 1x1 conv is refused by name: build it with exact_stride / pointwise_shortcut."""
        flags = (_QSTATIC_CONVS | _QBLOCKS | (_QSTATIC_CHAIN if chain else 0) | (_QSTATIC_PER_CHANNEL if per_channel else 0)
                 | (_QSTATIC_LINKS if links else 0))
        if percentile is None:
            return self._quantize_static(host.tp_module_quantize_static_ex, "quantize_static_residual", calib, flags)
        return self._quantize_static(host.tp_module_quantize_static_cal, "quantize_static_residual", calib, flags, _CALIB_PERCENTILE,
                                     int(round(float(percentile) * 1e4)), int(bins))

    def _quantize_static(self, entry, name, calib, *flags):
        """one static quantize call of the host library: the calibration tensors marshalled, `flags` for the entry point that takes them"""
        tensors = [calib] if isinstance(calib, Tensor) else list(calib)
        arr = (C.c_void_p * max(len(tensors), 1))(*[t._h if t is not None else None for t in tensors])
        h = _p()
        tp_check(entry(self._h, arr, len(tensors), *flags, C.byref(h)), "Module::" + name)
        return QuantizedModule(h.value)


class QuantizedModule:
    """nn.rs:20-23: forward from the packed codes (no tape node, the output needs no gradient)"""
    QTYPES = {"int8": 0, "float16": 1, "int4": 2, "bfloat16": 3, "nf4": 4}

    def __init__(self, h):
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            host.tp_qmodule_free(h)

    def forward(self, x: Tensor) -> Tensor:
        h = _p()
        tp_check(host.tp_qmodule_forward(self._h, x._h, C.byref(h)), "QuantizedModule::forward")
        return Tensor(_h=h.value)

    __call__ = forward

    def storage_bytes(self) -> int:
        n = C.c_size_t()
        tp_check(host.tp_qmodule_storage_bytes(self._h, C.byref(n)), "QuantizedModule::storage_bytes")
        return n.value

    def chain_links(self) -> int:
        """the layer boundaries a forward crosses in int8 -- conv -> conv (quantize_static_chain), and with quantize_static_linked also
        Flatten into a Linear and Linear -> Linear; 0 for every other twin"""
        n = C.c_int()
        tp_check(host.tp_qmodule_chain_links(self._h, C.byref(n)), "QuantizedModule::chain_links")
        return n.value

    def act_scales(self) -> np.ndarray:
        """the calibrated activation scale of every static layer of a quantize_static / quantize_static_conv twin, in layer order (empty for
        a weight-only twin)"""
        n = C.c_int()
        tp_check(host.tp_qmodule_act_scales(self._h, None, 0, C.byref(n)), "QuantizedModule::act_scales")
        out = np.zeros(n.value, np.float32)
        if n.value:
            tp_check(host.tp_qmodule_act_scales(self._h, out.ctypes.data, n.value, C.byref(n)), "QuantizedModule::act_scales")
        return out

    def calibration(self):
        """one dict per static layer, in act_scales() order: the finite `min` and `max` of the layer's float inputs over the calibration
        set, the clip `threshold` and `scale` = threshold / 127, and of a quantize_static_calibrated twin the histogram's `bin` the
        threshold ends, `total` finite elements counted, `kept` of them at or below that bin and `bin_count` in the bin itself (0 for a
        min / max twin, whose threshold is max(|min|, |max|))"""
        n = C.c_int()
        tp_check(host.tp_qmodule_act_scales(self._h, None, 0, C.byref(n)), "QuantizedModule::calibration")
        out = []
        for i in range(n.value):
            f, u = np.zeros(4, np.float32), np.zeros(4, np.uint64)
            tp_check(host.tp_qmodule_calibration(self._h, i, f.ctypes.data, u.ctypes.data), "QuantizedModule::calibration")
            out.append(dict(min=f[0], max=f[1], threshold=f[2], scale=f[3], bin=int(u[0]), total=int(u[1]), kept=int(u[2]), bin_count=int(u[3])))
        return out

    def affines(self):
        """the frozen BatchNorm2d layers of the twin in layer order: a list of float32 arrays of shape (channels, 2) = {a, b}, the layer on
        its running pair as y = x * a + b (empty for a model without BatchNorm2d)"""
        n = C.c_int()
        tp_check(host.tp_qmodule_num_affines(self._h, C.byref(n)), "QuantizedModule::affines")
        out = []
        for i in range(n.value):
            k = C.c_size_t()
            tp_check(host.tp_qmodule_affine(self._h, i, None, 0, C.byref(k)), "QuantizedModule::affines")
            pairs = np.zeros((k.value, 2), np.float32)
            tp_check(host.tp_qmodule_affine(self._h, i, pairs.ctypes.data, k.value, C.byref(k)), "QuantizedModule::affines")
            out.append(pairs)
        return out

    def tensors(self):
        """[(qtype, codes, (min_val, scale))] in parameter order (a BatchNorm2d's gamma and beta are not packed: see affines()): codes int8 with its pair for "int8", uint16 half bits and
        (0, 0) for "float16".  A per-channel tensor (quantize_static_per_channel) has an ndarray of shape (channels, 2) as its third element."""
        n = C.c_int()
        tp_check(host.tp_qmodule_num_tensors(self._h, C.byref(n)), "QuantizedModule::tensors")
        out = []
        for i in range(n.value):
            ln = C.c_size_t()
            tp_check(host.tp_qmodule_tensor_len(self._h, i, C.byref(ln)), "QuantizedModule::tensors")
            qt = C.c_int()
            tp_check(host.tp_qmodule_tensor(self._h, i, None, None, C.byref(qt)), "QuantizedModule::tensors")
            codes = np.zeros(ln.value, np.int8 if qt.value == 0 else np.uint16)
            channels, chan_stride, _ = self.channel_layout(i)
            if chan_stride:
                pairs, n_pairs = np.zeros((channels, 2), np.float32), C.c_size_t()
                tp_check(host.tp_qmodule_tensor(self._h, i, codes.ctypes.data if ln.value else None, None, None), "QuantizedModule::tensors")
                tp_check(host.tp_qmodule_tensor_params(self._h, i, pairs.ctypes.data, channels, C.byref(n_pairs)), "QuantizedModule::tensors")
                out.append(("int8", codes, pairs))
                continue
            params = np.zeros(2, np.float32)
            tp_check(host.tp_qmodule_tensor(self._h, i, codes.ctypes.data if ln.value else None, params.ctypes.data, None),
                     "QuantizedModule::tensors")
            out.append(("int8" if qt.value == 0 else "float16", codes, (params[0], params[1])))
        return out

    def channel_layout(self, i):
        """(channels, chan_stride, elem_stride) of tensor i: element k of channel c is code c * chan_stride + k * elem_stride; (1, 0, 1) for
        a tensor with one pair"""
        ch, cs, es = C.c_size_t(), C.c_size_t(), C.c_size_t()
        tp_check(host.tp_qmodule_tensor_channels(self._h, int(i), C.byref(ch), C.byref(cs), C.byref(es)), "QuantizedModule::channel_layout")
        return ch.value, cs.value, es.value


def _mk(fn, name, *args):
    h = _p()
    tp_check(fn(*args, C.byref(h)), name)
    return h.value


class Linear(Module):
    def __init__(self, in_features, out_features, with_bias=True, seed=1):
        super().__init__(_mk(host.tp_linear_new, "Linear::new", int(in_features), int(out_features), 1 if with_bias else 0, int(seed)))

    @property
    def weight(self): return self.parameters()[0]

    @property
    def bias(self):
        p = self.parameters()
        return p[1] if len(p) > 1 else None


class ReLU(Module):
    def __init__(self): super().__init__(_mk(host.tp_relu_new, "ReLU"))


class Sigmoid(Module):
    def __init__(self): super().__init__(_mk(host.tp_sigmoid_new, "Sigmoid"))


class Conv2d(Module):
    """exact_stride: the layer is the exact 3x3 convolution with stride (2, 2) and padding (1, 1) (one group), and under
    set_full_backward(True) its weight and its input take gradients like a stride-1 layer's; the constructor refuses any other geometry
    with the flag by name.  Without it a strided Conv2d keeps the reference's general gather: not a convolution, no gradient.
    The flag is constructor state (a checkpoint holds the parameters alone); quantize* refuse such a layer, except
    quantize_static_residual, where it is a static conv.
    exact_pointwise: the layer is the exact 1x1 convolution with stride (1, 1) or (2, 2) and no padding (one group), with the same
    gradients, constructor state and quantize* refusal (quantize_static_residual takes it).  Without it a 1x1 Conv2d keeps the reference's reinterpretation."""

    def __init__(self, in_ch, out_ch, kernel_size, stride=None, padding=None, dilation=None, groups=None, bias=True,
                 seed=1, _relu=False, exact_stride=False, exact_pointwise=False):
        if dilation not in (None, (1, 1)):
            raise TaperError("Conv2d: dilation is out of scope (SURVEY.md section 2 row 8)")
        s, p = stride or (1, 1), padding or (0, 0)
        if exact_stride or exact_pointwise:
            if int(groups or 1) != 1:
                raise TaperError(f"Conv2d {'exact_stride' if exact_stride else 'exact_pointwise'}: groups must be 1 (got {int(groups)})")
            super().__init__(_mk(host.tp_conv2d_new_ex, "Conv2d::new", int(in_ch), int(out_ch), kernel_size[0], kernel_size[1],
                                 s[0], s[1], p[0], p[1], 1 if bias else 0, 1 if _relu else 0, int(seed),
                                 (EXACT_STRIDE if exact_stride else 0) | (EXACT_POINTWISE if exact_pointwise else 0)))
            return
        # groups > 1 (nn.rs:289-332): slice / conv per group / cat, forward only like the reference
        super().__init__(_mk(host.tp_conv2d_grouped_new, "Conv2d::new", int(in_ch), int(out_ch), kernel_size[0], kernel_size[1],
                             s[0], s[1], p[0], p[1], int(groups or 1), 1 if bias else 0, 1 if _relu else 0, int(seed)))


class Conv2dReLU(Conv2d):
    def __init__(self, in_ch, out_ch, kernel_size, stride=None, padding=None, dilation=None, groups=None, bias=True, seed=1, exact_stride=False,
                 exact_pointwise=False):
        super().__init__(in_ch, out_ch, kernel_size, stride, padding, dilation, groups, bias, seed, _relu=True, exact_stride=exact_stride,
                         exact_pointwise=exact_pointwise)


class MaxPool2d(Module):
    def __init__(self, kernel_size, stride=None, padding=None):
        s, p = stride or (0, 0), padding or (0, 0)
        super().__init__(_mk(host.tp_maxpool2d_new, "MaxPool2d::new", kernel_size[0], kernel_size[1], s[0], s[1], p[0], p[1]))


class AvgPool2d(Module):
    def __init__(self, kernel_size, stride=None, padding=None):
        s, p = stride or (0, 0), padding or (0, 0)
        super().__init__(_mk(host.tp_avgpool2d_new, "AvgPool2d::new", kernel_size[0], kernel_size[1], s[0], s[1], p[0], p[1]))


class AdaptiveAvgPool2d(Module):
    def __init__(self, output_size):
        super().__init__(_mk(host.tp_adaptive_avgpool2d_new, "AdaptiveAvgPool2d::new", output_size[0], output_size[1]))

    @staticmethod
    def global_():
        return AdaptiveAvgPool2d((1, 1))


class Flatten(Module):
    def __init__(self, start_dim=1):
        super().__init__(_mk(host.tp_flatten_new, "Flatten::new", int(start_dim)))


class Dropout(Module):
    """nn.rs:773-827; the mask comes from a counter-based generator (the reference's RNG is unseeded)"""

    def __init__(self, p, seed=0x64726F70):
        super().__init__(_mk(host.tp_dropout_new, "Dropout::new", float(p), int(seed)))

    def eval(self): tp_check(host.tp_dropout_set_training(self._h, 0), "Dropout::eval")
    def train(self): tp_check(host.tp_dropout_set_training(self._h, 1), "Dropout::train")

    def last_mask(self) -> Tensor:
        h = _p()
        tp_check(host.tp_dropout_last_mask(self._h, C.byref(h)), "Dropout::last_mask")
        return Tensor(_h=h.value)


class BatchNorm2d(Module):
    """torch.nn.BatchNorm2d's semantics over [N, C, H, W] (upstream announces the layer in nn.rs:829-857 and never writes it): batch
    statistics in training mode (default), the running pair in eval mode; fuse_relu applies max(y, 0) in the same pass."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, fuse_relu=False):
        self.num_features = int(num_features)
        super().__init__(_mk(host.tp_batchnorm2d_new, "BatchNorm2d::new", int(num_features), float(eps), float(momentum), 1 if fuse_relu else 0))

    def train(self): tp_check(host.tp_batchnorm2d_set_training(self._h, 1), "BatchNorm2d::train")
    def eval(self): tp_check(host.tp_batchnorm2d_set_training(self._h, 0), "BatchNorm2d::eval")

    def is_training(self) -> bool:
        out = C.c_int()
        tp_check(host.tp_batchnorm2d_is_training(self._h, C.byref(out)), "BatchNorm2d::is_training")
        return bool(out.value)

    def _running(self, which):
        a = np.zeros(self.num_features, np.float32)
        tp_check(host.tp_batchnorm2d_running_stats(self._h, a.ctypes.data if which == 0 else None, a.ctypes.data if which == 1 else None),
                 "BatchNorm2d::running_stats")
        return a

    @property
    def running_mean(self) -> np.ndarray: return self._running(0)

    @property
    def running_var(self) -> np.ndarray: return self._running(1)

    def set_running_stats(self, mean, var):
        m, v = np.ascontiguousarray(mean, np.float32).ravel(), np.ascontiguousarray(var, np.float32).ravel()
        if m.size != self.num_features or v.size != self.num_features:
            raise TaperError("BatchNorm2d::set_running_stats: num_features values each expected")
        tp_check(host.tp_batchnorm2d_set_running_stats(self._h, m.ctypes.data, v.ctypes.data), "BatchNorm2d::set_running_stats")

    def forward_add(self, x: Tensor, residual: Tensor) -> Tensor:
        """bn(x) + residual, then the layer's ReLU (fuse_relu: after the add), inside the normalisation's own launches: a residual block's
        tail as one tape node.  The residual has x's shape and its own storage."""
        h = _p()
        tp_check(host.tp_batchnorm2d_forward_add(self._h, x._h, residual._h, C.byref(h)), "BatchNorm2d::forward_add")
        return Tensor(_h=h.value)

    @property
    def gamma(self): return self.parameters()[0]

    @property
    def beta(self): return self.parameters()[1]


class BasicBlock(Module):
    """nn.rs:829-857 as announced: Conv2d::conv3x3(in, out, stride, 1) -> BatchNorm2d(out) -> ReLU; parameters(): the conv's, then gamma, beta.
    BasicBlock.exact_stride(...) builds the block whose conv, at stride 2, is Conv2d(exact_stride=True); nothing changes at stride 1; any
    other stride is refused by name."""

    def __init__(self, in_channels, out_channels, stride=1, seed=1):
        super().__init__(_mk(host.tp_basic_block_new, "BasicBlock::new", int(in_channels), int(out_channels), int(stride), int(seed)))

    @classmethod
    def exact_stride(cls, in_channels, out_channels, stride=1, seed=1):
        """the block with the exact strided convolution (tp_basic_block_new_ex, TP_CONV_EXACT_STRIDE); the constructor's arguments"""
        blk = cls.__new__(cls)
        Module.__init__(blk, _mk(host.tp_basic_block_new_ex, "BasicBlock::new", int(in_channels), int(out_channels), int(stride), int(seed),
                                 EXACT_STRIDE))
        return blk


class ResidualBlock(Module):
    """conv3x3(in, out, stride) -> BatchNorm2d + ReLU -> conv3x3(out, out) -> BatchNorm2d + shortcut -> ReLU, the add and the last ReLU inside
    the second normalisation's kernels.  Shortcut: the input when in == out and stride == 1, else conv3x3(in, out, stride) -> BatchNorm2d
    (a 3x3 projection by default; ResidualBlock.pointwise_shortcut(...) builds the block with the 1x1 projection every ResNet uses).  No conv
    has a bias.  parameters(): conv1 w, bn1 gamma beta, conv2 w, bn2 gamma beta, [shortcut conv w,
    gamma beta]; buffers(): the running pairs in that order.

    A downsampling block (stride 2) by default keeps the reference's strided path in conv1 and in the projection: the general gather of
    SURVEY Q9, which is no convolution and records no weight or input gradient, so those two convs stay at their initial values.
    ResidualBlock.exact_stride(in, out, 2) is the block to train with: both strided convs are Conv2d(exact_stride=True) -- true 3x3 /
    stride 2 / pad 1 convolutions on the matrix cores whose weights and inputs take gradients under set_full_backward(True).  With
    stride 1 it builds the same block as the constructor; any other stride is refused by name."""

    def __init__(self, in_channels, out_channels, stride=1, seed=1):
        super().__init__(_mk(host.tp_residual_block_new, "ResidualBlock::new", int(in_channels), int(out_channels), int(stride), int(seed)))

    @classmethod
    def exact_stride(cls, in_channels, out_channels, stride=1, seed=1):
        """the block with the exact strided convolutions (tp_residual_block_new_ex, TP_CONV_EXACT_STRIDE); the constructor's arguments"""
        blk = cls.__new__(cls)
        Module.__init__(blk, _mk(host.tp_residual_block_new_ex, "ResidualBlock::new", int(in_channels), int(out_channels), int(stride),
                                 int(seed), EXACT_STRIDE))
        return blk

    @classmethod
    def pointwise_shortcut(cls, in_channels, out_channels, stride=1, seed=1, exact_stride=True):
        """the block whose projection is Conv2d(in, out, (1, 1), stride, exact_pointwise=True, bias=False) -> BatchNorm2d in place of the 3x3
        (tp_residual_block_new_ex, TP_CONV_EXACT_POINTWISE): a ninth of the projection's arithmetic and weights, same seed + 2; exact_stride
        as in ResidualBlock.exact_stride (conv1 at stride 2).  Strides 1 and 2; with an identity shortcut it is the constructor's block."""
        blk = cls.__new__(cls)
        Module.__init__(blk, _mk(host.tp_residual_block_new_ex, "ResidualBlock::new", int(in_channels), int(out_channels), int(stride),
                                 int(seed), EXACT_POINTWISE | (EXACT_STRIDE if exact_stride else 0)))
        return blk


class BottleneckBlock(Module):
    """pointwise(in, mid) -> BatchNorm2d + ReLU -> conv3x3(mid, mid, stride; the exact strided convolution at stride 2) -> BatchNorm2d + ReLU ->
    pointwise(mid, out) -> BatchNorm2d + shortcut -> ReLU, the add and the last ReLU inside the third normalisation's kernels.  Shortcut: the
    input when in == out and stride == 1, else pointwise(in, out, stride) -> BatchNorm2d.  Every 1x1 is Conv2d(exact_pointwise=True); no conv has
    a bias; seeds seed .. seed + 3 in that order; stride 1 or 2.  parameters(): conv1 w, bn1 gamma beta, conv2 w, bn2 gamma beta, conv3 w, bn3
    gamma beta, [shortcut conv w, gamma beta]; buffers(): the running pairs in that order.  Trains under set_full_backward(True)."""

    def __init__(self, in_channels, mid_channels, out_channels, stride=1, seed=1):
        super().__init__(_mk(host.tp_bottleneck_block_new, "BottleneckBlock::new", int(in_channels), int(mid_channels), int(out_channels),
                             int(stride), int(seed)))


class Sequential(Module):
    def __init__(self, layers, fuse=True):
        self.layers = list(layers)  # keep the children alive
        arr = (_p * len(self.layers))(*[l._h for l in self.layers])
        super().__init__(_mk(host.tp_sequential_new, "Sequential::new", arr, len(self.layers), 1 if fuse else 0))



# -- src/quantization/{qat_config,qat_layers,qat_manager}.rs ---------------------------
class QATConfig:
    """qat_config.rs: the codec the QAT layers train against ("int8" | "float16") and whether their outputs are fake-quantized too.
    int4 / bfloat16 / nf4, symmetric=False and per_channel=True are refused here, before anything reaches the device."""
    QTYPES = QuantizedModule.QTYPES

    def __init__(self, qtype="int8", activations=True, symmetric=True, per_channel=False):
        if qtype not in self.QTYPES:
            raise TaperError(f"QATConfig: unknown qtype {qtype!r}")
        if qtype in ("int4", "bfloat16", "nf4"):
            raise TaperError(f"QAT quantization type {qtype} is not supported: the reference's codec for it is a placeholder that returns zeros")
        if not symmetric:
            raise TaperError("QAT with symmetric = false is not supported: the reference's asymmetric zero point and clamp cut off the "
                             "upper half of the range")
        if per_channel:
            raise TaperError("QAT with per_channel = true is not supported: the reference never implements per-channel scales")
        self.qtype, self.activations, self.symmetric, self.per_channel = qtype, bool(activations), bool(symmetric), bool(per_channel)

    def _args(self):
        return self.QTYPES[self.qtype], int(self.activations), int(self.symmetric), int(self.per_channel)


class _QATLayer(Module):
    def enable_qat(self, enabled=True):
        """qat_layers.rs:68-71: the layer's own flag and the QAT manager's entry of its id"""
        tp_check(host.tp_qat_module_set_enabled(self._h, 1 if enabled else 0), "enable_qat")

    def observed(self):
        """the observer readout of the last fake-quantized forward: weight (min_val, scale) and the activation scale (int8)"""
        out = (C.c_float * 3)()
        tp_check(host.tp_qat_module_observed(self._h, out), "QAT observed")
        return dict(weight_min=float(out[0]), weight_scale=float(out[1]), activation_scale=float(out[2]))

    def fake_quantized(self, which="weight") -> Tensor:
        """the round trip of the weight ("weight") or the bias ("bias") the last active forward ran with (a copy)"""
        h = _p()
        tp_check(host.tp_qat_module_fake_quantized(self._h, 0 if which == "weight" else 1, C.byref(h)), "QAT fake_quantized")
        return Tensor(_h=h.value)

    @property
    def weight(self): return self.parameters()[0]

    @property
    def bias(self):
        p = self.parameters()
        return p[1] if len(p) > 1 else None


class QATLinear(_QATLayer):
    """qat_layers.rs:10-134: a Linear (same initial weights for the same seed) trained against its quantized weights"""

    def __init__(self, in_features, out_features, with_bias=True, config=None, module_id=None, seed=1):
        c = config or QATConfig()
        super().__init__(_mk(host.tp_qat_linear_new, "QATLinear::new", int(in_features), int(out_features), 1 if with_bias else 0,
                             *c._args(), module_id.encode() if module_id else None, int(seed)))


class QATConv2d(_QATLayer):
    """qat_layers.rs:136-265 (groups 1); relu=True stands in for Conv2dReLU, its ReLU behind the activation fake-quant"""

    def __init__(self, in_ch, out_ch, kernel_size, stride=None, padding=None, bias=True, relu=False, config=None, module_id=None, seed=1):
        c = config or QATConfig()
        s, p = stride or (1, 1), padding or (0, 0)
        super().__init__(_mk(host.tp_qat_conv2d_new, "QATConv2d::new", int(in_ch), int(out_ch), kernel_size[0], kernel_size[1], s[0], s[1],
                             p[0], p[1], 1 if bias else 0, 1 if relu else 0, *c._args(), module_id.encode() if module_id else None, int(seed)))


class qat:
    """qat_manager.rs `global::`: the process-wide QAT switches"""

    @staticmethod
    def enable(): tp_check(host.tp_qat_enable(1), "qat.enable")

    @staticmethod
    def disable(): tp_check(host.tp_qat_enable(0), "qat.disable")

    @staticmethod
    def set_training_mode(training: bool): tp_check(host.tp_qat_set_training(1 if training else 0), "qat.set_training_mode")

    @staticmethod
    def is_training() -> bool:
        out = C.c_int()
        tp_check(host.tp_qat_is_training(C.byref(out)), "qat.is_training")
        return bool(out.value)

    @staticmethod
    def status():
        g, t, n, e = C.c_int(), C.c_int(), C.c_size_t(), C.c_size_t()
        tp_check(host.tp_qat_status(C.byref(g), C.byref(t), C.byref(n), C.byref(e)), "qat.status")
        return dict(global_enabled=bool(g.value), training_mode=bool(t.value), module_count=n.value, enabled_modules=e.value,
                    is_active=bool(g.value) and bool(t.value))


# -- src/quantization/observers.rs -------------------------------------------------
class _Observer:
    """An observer's statistics live on the device: observe() only enqueues work on the stream; the read-outs wait."""
    _KIND = None

    def __init__(self, num_bins=0):
        h = _p()
        tp_check(host.tp_observer_new(self._KIND, int(num_bins), C.byref(h)), f"{type(self).__name__}::new")
        self._h = h.value

    def __del__(self):
        if getattr(self, "_h", None):
            host.tp_observer_free(self._h)
            self._h = None

    def set_enabled(self, enabled: bool): tp_check(host.tp_observer_set_enabled(self._h, 1 if enabled else 0), "Observer::set_enabled")

    def is_enabled(self) -> bool:
        out = C.c_int()
        tp_check(host.tp_observer_is_enabled(self._h, C.byref(out)), "Observer::is_enabled")
        return bool(out.value)

    def observe(self, tensor: Tensor): tp_check(host.tp_observer_observe(self._h, tensor._h), "Observer::observe")

    def num_observations(self) -> int:
        out = C.c_size_t()
        tp_check(host.tp_observer_num_observations(self._h, C.byref(out)), "Observer::num_observations")
        return out.value

    def reset(self): tp_check(host.tp_observer_reset(self._h), "Observer::reset")


def _minmax_stats(call, what):
    n, lo, hi, rng = C.c_size_t(), C.c_float(), C.c_float(), C.c_float()
    if not call(C.byref(n), C.byref(lo), C.byref(hi), C.byref(rng), what):
        return None
    f = np.float32
    return dict(num_observations=n.value, global_min=f(lo.value), global_max=f(hi.value), range=f(rng.value))


def _histogram_stats(call, what):
    n, total, mean, most = C.c_size_t(), C.c_uint64(), C.c_float(), C.c_uint64()
    if not call(C.byref(n), C.byref(total), C.byref(mean), C.byref(most), what):
        return None
    return dict(num_observations=n.value, total_count=total.value, mean_bin=np.float32(mean.value), max_bin_count=most.value)


class MinMaxObserver(_Observer):
    """observers.rs:11-121: the running min / max PER ELEMENT of the flat data.  The first observation fixes the vectors' length; a later
    one of m elements updates the first min(m, len).  min / max are f32::min / f32::max (a NaN loses to a number)."""
    _KIND = 0

    def __init__(self):
        super().__init__(0)

    def _values(self, which):
        n = C.c_size_t()
        tp_check(host.tp_observer_minmax_len(self._h, C.byref(n)), "MinMaxObserver::len")
        out = np.empty(n.value, np.float32)
        ptr = out.ctypes.data if n.value else None
        tp_check(host.tp_observer_minmax_values(self._h, ptr if which == 0 else None, ptr if which == 1 else None), "MinMaxObserver::values")
        return out

    def min_values(self) -> np.ndarray: return self._values(0)
    def max_values(self) -> np.ndarray: return self._values(1)
    def global_min(self): return self.get_stats()["global_min"]
    def global_max(self): return self.get_stats()["global_max"]

    def get_stats(self):
        """ObserverStats: num_observations, global_min, global_max, range (the folds run on the device; +inf / -inf / -inf when empty)"""
        def call(n, lo, hi, rng, what):
            tp_check(host.tp_observer_minmax_stats(self._h, n, lo, hi, rng), what)
            return True
        return _minmax_stats(call, "MinMaxObserver::get_stats")

    stats = get_stats


class HistogramObserver(_Observer):
    """observers.rs:125-246: num_bins 64-bit counts between num_bins + 1 edges that the first observation fixes; bin k is
    (edge[k], edge[k + 1]], bin 0 also takes everything below, the last bin everything above and every NaN."""
    _KIND = 1

    def __init__(self, num_bins):
        if int(num_bins) < 1:
            raise TaperError("HistogramObserver: num_bins must be at least 1 (the reference's find_bin underflows with 0 bins)")
        super().__init__(num_bins)
        self.num_bins = int(num_bins)

    def bins(self) -> np.ndarray:
        out = np.empty(self.num_bins, np.uint64)
        tp_check(host.tp_observer_hist_bins(self._h, out.ctypes.data), "HistogramObserver::bins")
        return out

    def bin_edges(self) -> np.ndarray:
        n = C.c_size_t()
        tp_check(host.tp_observer_hist_num_edges(self._h, C.byref(n)), "HistogramObserver::bin_edges")
        out = np.empty(n.value, np.float32)
        if n.value:
            tp_check(host.tp_observer_hist_edges(self._h, out.ctypes.data), "HistogramObserver::bin_edges")
        return out

    edges = bin_edges

    def get_stats(self):
        """HistogramStats: num_observations, total_count, mean_bin, max_bin_count"""
        def call(n, total, mean, most, what):
            tp_check(host.tp_observer_hist_stats(self._h, n, total, mean, most), what)
            return True
        return _histogram_stats(call, "HistogramObserver::get_stats")

    stats = get_stats


class ObserverManager:
    """observers.rs:268-345: observers by name, one map per kind (a name may be in both).  Adding an existing name replaces its observer
    with a fresh one; observing an unknown name does nothing and its stats are None."""

    def __init__(self):
        h = _p()
        tp_check(host.tp_observer_manager_new(C.byref(h)), "ObserverManager::new")
        self._h = h.value

    def __del__(self):
        if getattr(self, "_h", None):
            host.tp_observer_manager_free(self._h)
            self._h = None

    def add_minmax_observer(self, name: str):
        tp_check(host.tp_observer_manager_add_minmax(self._h, name.encode()), "ObserverManager::add_minmax_observer")

    def add_histogram_observer(self, name: str, num_bins: int):
        if int(num_bins) < 1:
            raise TaperError("HistogramObserver: num_bins must be at least 1 (the reference's find_bin underflows with 0 bins)")
        tp_check(host.tp_observer_manager_add_histogram(self._h, name.encode(), int(num_bins)), "ObserverManager::add_histogram_observer")

    def observe_minmax(self, name: str, tensor: Tensor):
        tp_check(host.tp_observer_manager_observe_minmax(self._h, name.encode(), tensor._h), "ObserverManager::observe_minmax")

    def observe_histogram(self, name: str, tensor: Tensor):
        tp_check(host.tp_observer_manager_observe_histogram(self._h, name.encode(), tensor._h), "ObserverManager::observe_histogram")

    def get_minmax_stats(self, name: str):
        def call(n, lo, hi, rng, what):
            found = C.c_int()
            tp_check(host.tp_observer_manager_minmax_stats(self._h, name.encode(), C.byref(found), n, lo, hi, rng), what)
            return bool(found.value)
        return _minmax_stats(call, "ObserverManager::get_minmax_stats")

    def get_histogram_stats(self, name: str):
        def call(n, total, mean, most, what):
            found = C.c_int()
            tp_check(host.tp_observer_manager_histogram_stats(self._h, name.encode(), C.byref(found), n, total, mean, most), what)
            return bool(found.value)
        return _histogram_stats(call, "ObserverManager::get_histogram_stats")

    def reset_all(self): tp_check(host.tp_observer_manager_reset_all(self._h), "ObserverManager::reset_all")

    def get_observer_names(self):
        """the minmax names, then the histogram names, each sorted"""
        count, needed = C.c_size_t(), C.c_size_t()
        tp_check(host.tp_observer_manager_names(self._h, None, 0, C.byref(count), C.byref(needed)), "ObserverManager::get_observer_names")
        buf = C.create_string_buffer(needed.value)
        tp_check(host.tp_observer_manager_names(self._h, buf, needed.value, None, None), "ObserverManager::get_observer_names")
        return buf.value.decode().split("\n") if count.value else []


# -- src/optim.rs -----------------------------------------------------------------
class _Optim:
    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            host.tp_optim_free(h)

    def step(self): tp_check(host.tp_optim_step(self._h), "Optimizer::step")
    def zero_grad(self): tp_check(host.tp_optim_zero_grad(self._h), "Optimizer::zero_grad")

    def total(self) -> int:
        n = C.c_int64()
        tp_check(host.tp_optim_total(self._h, C.byref(n)), "tp_optim_total")
        return n.value


class Adam(_Optim):
    def __init__(self, params, lr, betas=None, eps=None, weight_decay=None):
        betas = betas or (0.9, 0.999)
        self.params = list(params)
        arr = (_p * len(self.params))(*[p._h for p in self.params])
        self._h = _mk(host.tp_adam_new, "Adam::new", arr, len(self.params), float(lr), float(betas[0]), float(betas[1]),
                      float(1e-8 if eps is None else eps), float(0.0 if weight_decay is None else weight_decay))

    def set_lr(self, lr): tp_check(host.tp_adam_set_lr(self._h, float(lr)), "Adam::set_lr")

    def get_lr(self):
        v = C.c_float()
        tp_check(host.tp_adam_get_lr(self._h, C.byref(v)), "Adam::get_lr")
        return float(v.value)

    def t(self):
        v = C.c_int()
        tp_check(host.tp_adam_t(self._h, C.byref(v)), "Adam::t")
        return v.value

    def moments(self):
        n = sum(p.numel() for p in self.params)
        m, v = np.empty(n, np.float32), np.empty(n, np.float32)
        tp_check(host.tp_adam_moments(self._h, m.ctypes.data, v.ctypes.data), "Adam::moments")
        return m, v


    def load_state(self, t, m, v):
        m, v = np.ascontiguousarray(m, np.float32), np.ascontiguousarray(v, np.float32)
        tp_check(host.tp_adam_load_state(self._h, int(t), m.ctypes.data, v.ctypes.data), "Adam::load_state")


class AdamW(Adam):
    """optim.rs:130-180: decoupled decay on every weight, then Adam with weight_decay = 0"""

    def __init__(self, params, lr, betas=None, eps=None, weight_decay=None):
        betas = betas or (0.9, 0.999)
        self.params = list(params)
        arr = (_p * len(self.params))(*[p._h for p in self.params])
        self._h = _mk(host.tp_adamw_new, "AdamW::new", arr, len(self.params), float(lr), float(betas[0]), float(betas[1]),
                      float(1e-8 if eps is None else eps), float(0.0 if weight_decay is None else weight_decay))


class _Scheduler:
    """optim.rs:183-188 LRScheduler: step(metrics: Option<f32>), get_lr()"""

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            host.tp_sched_free(h)

    def step(self, metrics=None):
        m = None if metrics is None else C.byref(C.c_float(float(metrics)))
        tp_check(host.tp_sched_step(self._h, m), "LRScheduler::step")

    def get_lr(self) -> float:
        v = C.c_float()
        tp_check(host.tp_sched_get_lr(self._h, C.byref(v)), "LRScheduler::get_lr")
        return float(v.value)


class StepLR(_Scheduler):
    def __init__(self, base_lr, step_size, gamma):
        self._h = _mk(host.tp_sched_step_lr, "StepLR::new", float(base_lr), int(step_size), float(gamma))


class ExponentialLR(_Scheduler):
    def __init__(self, base_lr, gamma):
        self._h = _mk(host.tp_sched_exponential, "ExponentialLR::new", float(base_lr), float(gamma))


class CosineAnnealingLR(_Scheduler):
    def __init__(self, base_lr, t_max, min_lr=None):
        self._h = _mk(host.tp_sched_cosine, "CosineAnnealingLR::new", float(base_lr), int(t_max), float(min_lr or 0.0))


class ReduceLROnPlateau(_Scheduler):
    def __init__(self, initial_lr, factor, patience, min_lr=None, mode=None):
        self._h = _mk(host.tp_sched_plateau, "ReduceLROnPlateau::new", float(initial_lr), float(factor), int(patience),
                      float(1e-6 if min_lr is None else min_lr), 1 if (mode or "min") == "max" else 0)


def format_f32(v) -> str:
    """an f32 as Rust's `{}` prints it (the checkpoint's number format, train.rs:283-285)"""
    buf = C.create_string_buffer(160)
    tp_check(host.tp_format_f32(float(v), buf, len(buf)), "format_f32")
    return buf.value.decode()


class SGD(_Optim):
    def __init__(self, params, lr, momentum=None):
        self.params = list(params)
        arr = (_p * len(self.params))(*[p._h for p in self.params])
        self._h = _mk(host.tp_sgd_new, "SGD::new", arr, len(self.params), float(lr))


# -- src/data/mnist.rs --------------------------------------------------------------
class MNISTDataset:
    def __init__(self, h):
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            host.tp_dataset_free(h)

    @staticmethod
    def from_host(images, labels, train=True):
        im = np.ascontiguousarray(images, dtype=np.float32).reshape(-1, 784)
        lb = np.ascontiguousarray(labels, dtype=np.float32).reshape(-1)
        return MNISTDataset(_mk(host.tp_dataset_from_host, "MNISTDataset::from_host", im.ctypes.data, lb.ctypes.data, lb.size, 1 if train else 0))

    @staticmethod
    def from_idx(images_path, labels_path, train=True):
        return MNISTDataset(_mk(host.tp_dataset_from_idx, "MNISTDataset::from_idx", str(images_path).encode(), str(labels_path).encode(), 1 if train else 0))

    @staticmethod
    def synthetic(n, seed=0x7461706572, train=True):
        return MNISTDataset(_mk(host.tp_dataset_synthetic, "MNISTDataset::synthetic", int(n), int(seed), 1 if train else 0))

    def len(self):
        n = C.c_size_t()
        tp_check(host.tp_dataset_len(self._h, C.byref(n)), "len")
        return n.value

    def tensors(self):
        a, b = _p(), _p()
        tp_check(host.tp_dataset_tensors(self._h, C.byref(a), C.byref(b)), "tensors")
        return Tensor(_h=a.value), Tensor(_h=b.value)


class DataLoader:
    def __init__(self, dataset, batch_size, shuffle, seed=0x7461706572):
        self.dataset = dataset
        self._h = _mk(host.tp_loader_new, "DataLoader::new", dataset._h, int(batch_size), 1 if shuffle else 0, int(seed))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            host.tp_loader_free(h)

    def reset(self): tp_check(host.tp_loader_reset(self._h), "DataLoader::reset")

    def num_batches(self):
        # (dataset length and batch size are fixed at construction: asked once -- the Trainer wrappers ask on every call)
        n = getattr(self, "_nb", None)
        if n is None:
            c = C.c_size_t()
            tp_check(host.tp_loader_num_batches(self._h, C.byref(c)), "num_batches")
            n = self._nb = c.value
        return n

    def __iter__(self):
        return self

    def __next__(self):
        a, b, has = _p(), _p(), C.c_int()
        tp_check(host.tp_loader_next(self._h, C.byref(a), C.byref(b), C.byref(has)), "DataLoader::next")
        if not has.value:
            raise StopIteration
        return Tensor(_h=a.value), Tensor(_h=b.value)


# -- data parallel --------------------------------------------------------------------
class Communicator:
    """RCCL communicator, one process per GPU; the 128-byte id travels out of band."""

    BLOB_BYTES = 192

    def __init__(self, n_ranks, rank, uid: bytes | None = None, _h=None):
        self.n_ranks, self.rank = n_ranks, rank
        self._p2p = _h is not None
        if _h is not None:
            self._h = _h
            return
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._h = _mk(host.tp_comm_new, "Communicator::new", int(n_ranks), int(rank), buf)

    @staticmethod
    def p2p(n_ranks, rank):
        """peer-to-peer communicator (one node, <= 8 ranks): one-shot all-reduce of the gradient arena fused with Adam"""
        return Communicator(n_ranks, rank, _h=_mk(host.tp_comm_new_p2p, "Communicator::p2p", int(n_ranks), int(rank)))

    @staticmethod
    def loopback():
        """W = 2 with this process as its own peer: the exchange inside the gradient launch (th_mlp_tail_dp) runs every push, flag, poll
        and load of its protocol through local memory; results are the single-GPU step's, bit for bit"""
        return Communicator(2, 0, _h=_mk(host.tp_comm_new_loopback, "Communicator::loopback"))

    def set_inkernel(self, on: bool):
        """False: never the in-launch exchange (the three-launch form: gradient launch, then all-reduce + Adam) -- A/B runs"""
        tp_check(host.tp_comm_set_inkernel(self._h, 1 if on else 0), "Communicator::set_inkernel")

    def inkernel_launches(self) -> int:
        out = C.c_int64()
        tp_check(host.tp_comm_inkernel_launches(self._h, C.byref(out)), "Communicator::inkernel_launches")
        return int(out.value)

    def exchange_selftest(self, slots: int = 16, rounds: int = 3) -> int:
        """collective: the in-launch exchange alone on known patterns; -> mismatches + time-outs seen by this rank"""
        out = C.c_int()
        tp_check(host.tp_comm_exchange_selftest(self._h, int(slots), int(rounds), C.byref(out)), "Communicator::exchange_selftest")
        return int(out.value)

    def exchange_form(self) -> int:
        """0: no in-launch exchange; 1: one-shot (every rank reduces every slice); 2: two-shot (slice s reduced by rank s % W; 4 ranks and more)"""
        out = C.c_int()
        tp_check(host.tp_comm_exchange_form(self._h, C.byref(out)), "Communicator::exchange_form")
        return int(out.value)

    def ranks_on_this_device(self) -> int:
        out = C.c_int()
        tp_check(host.tp_comm_ranks_on_this_device(self._h, C.byref(out)), "Communicator::ranks_on_this_device")
        return int(out.value)

    def tail_exchange_ok(self, batch: int, in_features: int, hidden: int, classes: int) -> bool:
        out = C.c_int()
        tp_check(host.tp_comm_tail_exchange_ok(self._h, int(batch), int(in_features), int(hidden), int(classes), C.byref(out)), "Communicator::tail_exchange_ok")
        return bool(out.value)

    def export_arena(self, optimizer, fine_grained: bool = False) -> bytes:
        """register the optimizer's gradient arena; fine_grained: move it into fine-grained (cross-agent coherent) device memory first"""
        buf = (C.c_uint8 * self.BLOB_BYTES)()
        tp_check(host.tp_comm_export_arena_ex(self._h, optimizer._h, 1 if fine_grained else 0, buf), "Communicator::export_arena")
        return bytes(buf)

    def connect(self, blobs: bytes):
        buf = (C.c_uint8 * len(blobs)).from_buffer_copy(blobs)
        tp_check(host.tp_comm_connect(self._h, buf, len(blobs)), "Communicator::connect")

    def is_p2p(self) -> bool:
        return self._p2p

    def self_check(self, optimizer, rounds: int = 3) -> bool:
        """collective: `rounds` all-reduces of per-rank / per-round / per-element patterns through the SAME arena addresses, through the
        in-place kernel and the fused all-reduce + Adam kernel (p / m / v against the closed form; state restored)"""
        ok = C.c_int()
        tp_check(host.tp_comm_self_check_rounds(self._h, optimizer._h, int(rounds), C.byref(ok)), "Communicator::self_check")
        return bool(ok.value)

    def failed(self) -> bool:
        """a peer never arrived at some all-reduce (host-visible error word; no stream synchronisation)"""
        out = C.c_int()
        tp_check(host.tp_comm_failed(self._h, C.byref(out)), "Communicator::failed")
        return bool(out.value)

    def set_timeout_ms(self, ms: int):
        tp_check(host.tp_comm_set_timeout_ms(self._h, int(ms)), "Communicator::set_timeout_ms")

    def set_fuse_adam(self, on: bool):
        tp_check(host.tp_comm_set_fuse_adam(self._h, 1 if on else 0), "Communicator::set_fuse_adam")

    def stats(self):
        out = (C.c_int64 * 2)()
        tp_check(host.tp_comm_stats(self._h, out), "Communicator::stats")
        return dict(inplace=int(out[0]), fused=int(out[1]))

    def timed_out(self) -> bool:
        out = C.c_int()
        tp_check(host.tp_comm_timed_out(self._h, C.byref(out)), "Communicator::timed_out")
        return bool(out.value)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            host.tp_comm_free(h)

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        tp_check(host.tp_comm_unique_id(buf), "Communicator::unique_id")
        return bytes(buf)

    def allreduce_mean(self, d_ptr: int, n: int):
        tp_check(host.tp_comm_allreduce_mean(self._h, d_ptr, int(n)), "allreduce_mean")

    def count(self) -> int:
        """ranks the communicator spans (RCCL: ncclCommCount)"""
        out = C.c_int()
        tp_check(host.tp_comm_count(self._h, C.byref(out)), "Communicator::count")
        return int(out.value)

    def time_exchange(self, optimizer, reps: int = 200) -> float:
        """collective: us per gradient exchange + Adam as a Trainer step issues it (events on the stream); moves the optimizer state"""
        out = C.c_float()
        tp_check(host.tp_comm_time_exchange(self._h, optimizer._h, int(reps), C.byref(out)), "Communicator::time_exchange")
        return float(out.value)


# -- src/train.rs ---------------------------------------------------------------------
class Trainer:
    """train.rs:74-172 + the captured-graph epoch driver."""

    EAGER, GRAPH, EVAL = 0, 1, 2

    def __init__(self, model: Module, optimizer: Adam, sample_shape=None, comm: Communicator | None = None,
                 graph_chunk: int = 128, fuse_head: bool | int = True, fuse_adam: bool = True, scheduler=None):
        self.model, self.optimizer, self.comm, self.scheduler = model, optimizer, comm, scheduler
        self._h = _mk(host.tp_trainer_new, "Trainer::new", model._h, optimizer._h)
        # fuse_head: False / 0 = off, 1 = classifier head only, True / 2 = head + hidden-layer backward in one launch
        level = 2 if fuse_head is True else int(fuse_head)
        tp_check(host.tp_trainer_set_options(self._h, int(graph_chunk), level, 1 if fuse_adam else 0), "set_options")
        if sample_shape:
            tp_check(host.tp_trainer_set_sample_shape(self._h, _shape_arr(sample_shape), len(sample_shape)), "set_sample_shape")
        if comm is not None:
            tp_check(host.tp_trainer_set_comm(self._h, comm._h), "set_comm")
        if scheduler is not None:
            tp_check(host.tp_trainer_set_scheduler(self._h, scheduler._h), "set_scheduler")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            host.tp_trainer_free(h)

    def train_step(self, images: Tensor, labels: Tensor):
        loss, acc = C.c_float(), C.c_float()
        tp_check(host.tp_trainer_train_step(self._h, images._h, labels._h, C.byref(loss), C.byref(acc)), "train_step")
        return float(loss.value), float(acc.value)

    def run_epoch(self, loader: DataLoader, mode=GRAPH, max_steps=0):
        # (the out-parameters and the per-step buffer are kept between calls: a 20-step call is 250 us, and allocating them was 3 of it)
        nb_max = loader.num_batches()
        st = getattr(self, "_epoch_out", None)
        if st is None or st[0].size < 2 * nb_max:
            st = (np.empty(2 * nb_max, dtype=np.float32), C.c_float(), C.c_float(), C.c_size_t(), C.c_size_t(), C.c_size_t())
            st = st + (st[0].ctypes.data, tuple(C.byref(v) for v in st[1:6]))
            self._epoch_out = st
        per, avg, acc, tc, ts, nb, per_ptr, refs = st
        tp_check(host.tp_trainer_run_epoch(self._h, loader._h, int(mode), int(max_steps), *refs, per_ptr, per.size), "run_epoch")
        n = nb.value
        return dict(avg_loss=avg.value, accuracy=acc.value, total_correct=tc.value, total_samples=ts.value,
                    num_batches=n, losses=per[0:2 * n:2].copy(), ncorrect=per[1:2 * n:2].copy())

    def train_epoch(self, loader): return self.run_epoch(loader, self.EAGER)
    def train_epoch_graph(self, loader, max_steps=0): return self.run_epoch(loader, self.GRAPH, max_steps)
    def evaluate(self, loader): return self.run_epoch(loader, self.EVAL)

    def last_replays(self):
        """what the last train_epoch_graph call did, in order: [(kind, steps)] with kind 0 the state reset on its own, 1 steps enqueued
        eagerly, 2 / 3 a step graph captured / replayed, 4 / 5 a whole-call graph captured / replayed (read-only)"""
        n = C.c_size_t()
        tp_check(host.tp_trainer_last_replays(self._h, None, 0, C.byref(n)), "last_replays")
        buf = np.zeros(2 * n.value, np.int64)
        tp_check(host.tp_trainer_last_replays(self._h, buf.ctypes.data, n.value, None), "last_replays")
        return [(int(k), int(s)) for k, s in buf.reshape(-1, 2)]

    # -- train.rs:175-292 ---------------------------------------------------------
    def fit(self, train_loader: DataLoader, val_loader: DataLoader, epochs: int, verbose: bool = False, graph: bool = True):
        tp_check(host.tp_trainer_fit(self._h, train_loader._h, val_loader._h, int(epochs), 1 if verbose else 0, 1 if graph else 0), "fit")
        return self.metrics()

    def metrics(self):
        out = {}
        for which, name in enumerate(("train_loss", "train_acc", "val_loss", "val_acc", "epoch_times")):
            n = C.c_size_t()
            tp_check(host.tp_trainer_metrics(self._h, which, None, 0, C.byref(n)), "metrics")
            buf = np.zeros(n.value, np.float32)
            tp_check(host.tp_trainer_metrics(self._h, which, buf.ctypes.data, buf.size, None), "metrics")
            out[name] = buf
        return out

    def metrics_text(self, summary=False) -> str:
        buf = C.create_string_buffer(2048)
        tp_check(host.tp_trainer_metrics_text(self._h, 1 if summary else 0, buf, len(buf)), "metrics_text")
        return buf.value.decode()

    def save_checkpoint(self, path): tp_check(host.tp_trainer_save_checkpoint(self._h, str(path).encode()), "save_checkpoint")
    def load_checkpoint(self, path): tp_check(host.tp_trainer_load_checkpoint(self._h, str(path).encode()), "load_checkpoint")
    def save_optimizer_state(self, path): tp_check(host.tp_trainer_save_optimizer_state(self._h, str(path).encode()), "save_optimizer_state")
    def load_optimizer_state(self, path): tp_check(host.tp_trainer_load_optimizer_state(self._h, str(path).encode()), "load_optimizer_state")
