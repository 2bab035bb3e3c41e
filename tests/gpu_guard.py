"""Guarded device buffers shared by the exact GPU test modules (tests/test_gpu_sgemm_forms.py, tests/test_gpu_conv_forms.py): operands inside
NaN margins, outputs inside guard words, and the pool's in-use figure."""
import ctypes as C

import numpy as np

f32 = np.float32
MARGIN = 256               # words on either side of every operand and of C
GUARD_BITS = 0xFFA5C3E1    # a NaN payload no computation produces (th_fill_f32's NaN is 0x7FC00000)


def in_use(ctx):
    """bytes of the context's pool that are handed out"""
    from taper_amd._lib import hip
    r, u = C.c_size_t(), C.c_size_t()
    assert hip.th_pool_stats(ctx.h, C.byref(r), C.byref(u)) == 0
    return u.value


def operand(ctx, a, off=0):
    """`a` in device memory `off` bytes past a 16-byte boundary, NaN all around it -> (the allocation, the pointer)"""
    lead = MARGIN + off // 4
    host = np.full(lead + a.size + MARGIN, np.nan, f32)
    host[lead:lead + a.size] = a.reshape(-1)
    buf = ctx.upload(host)
    assert int(buf) % 16 == 0
    return buf, buf.offset(4 * lead)


class Out:
    """C [m, n] inside a buffer of guard words, `off` bytes past a 16-byte boundary; c0 None: NaN (what beta == 0 must overwrite unread)"""

    def __init__(self, ctx, m, n, off, c0=None):
        self.ctx, self.shape, self.lead = ctx, (m, n), MARGIN + off // 4
        host = np.full(self.lead + m * n + MARGIN, GUARD_BITS, np.uint32)
        host[self.lead:self.lead + m * n] = (np.full((m, n), np.nan, f32) if c0 is None else c0).reshape(-1).view(np.uint32)
        self.buf = ctx.upload(host)
        assert int(self.buf) % 16 == 0
        self.ptr = self.buf.offset(4 * self.lead)

    def check(self, ref, what):
        m, n = self.shape
        got = self.ctx.download(self.buf, (self.lead + m * n + MARGIN,), np.uint32)
        body = got[self.lead:self.lead + m * n].view(f32).reshape(m, n)
        np.testing.assert_array_equal(body, ref, err_msg=f"{what}: C")
        assert (got[:self.lead] == GUARD_BITS).all() and (got[self.lead + m * n:] == GUARD_BITS).all(), f"{what}: a write outside C"
        return body


