// quant_dev.h -- the reference's IEEE half codec as device functions (src/tensor.rs:2191-2287), shared by the storage codecs
// (quant.hip) and the quantized forward (qlinear.hip), plus the int8 dequantisation of one code (tensor.rs:353-360).
#pragma once
#include "common.h"

namespace th {

// tensor.rs:2191-2238
__device__ __forceinline__ uint16_t f32_to_f16_bits(float value) {
    const uint32_t bits = __float_as_uint(value);
    const uint32_t sign = (bits >> 31) & 0x1, exponent = (bits >> 23) & 0xFF, mantissa = bits & 0x7FFFFF;
    if (exponent == 0xFF) return (uint16_t)((sign << 15) | (0x1Fu << 10) | (mantissa != 0 ? 0x200u : 0u));   // inf / NaN
    if (exponent == 0 && mantissa == 0) return (uint16_t)(sign << 15);                                          // +-0
    const int f16_exponent = (int)exponent - 127 + 15;
    if (f16_exponent >= 0x1F) return (uint16_t)((sign << 15) | (0x1Fu << 10));                                  // overflow -> inf
    if (f16_exponent <= 0) {
        if (f16_exponent < -10) return (uint16_t)(sign << 15);                                                  // underflow -> 0
        const int shift = 1 - f16_exponent;
        const uint32_t m = (mantissa | 0x800000u) >> (shift + 13);                                             // truncating
        return (uint16_t)((sign << 15) | m);
    }
    const uint32_t m = (mantissa + 0x1000u) >> 13;                                                              // round half up; a carry (0x400) is OR-ed below
    return (uint16_t)((sign << 15) | ((uint32_t)f16_exponent << 10) | m);
}

// tensor.rs:2241-2287
__device__ __forceinline__ float f16_bits_to_f32(uint16_t value) {
    const uint32_t bits = value, sign = (bits >> 15) & 0x1, exponent = (bits >> 10) & 0x1F, mantissa = bits & 0x3FF;
    if (exponent == 0x1F) return __uint_as_float((sign << 31) | (0xFFu << 23) | (mantissa != 0 ? mantissa << 13 : 0u));
    if (exponent == 0) {
        if (mantissa == 0) return __uint_as_float(sign << 31);
        int exp = -14;
        uint32_t mant = mantissa;
        while ((mant & 0x400) == 0) {
            mant <<= 1;
            exp -= 1;
        }
        mant &= 0x3FF;
        return __uint_as_float((sign << 31) | (((uint32_t)(exp + 127) & 0xFF) << 23) | (mant << 13));
    }
    return __uint_as_float((sign << 31) | (((exponent + 127 - 15) & 0xFF) << 23) | (mantissa << 13));
}

__device__ __forceinline__ float f16_round_trip(float v) { return f16_bits_to_f32(f32_to_f16_bits(v)); }

// tensor.rs:2127-2134: {min_val, scale} from the finite min / max (widened by 0.1 each way when they are equal); qrange = 255
__device__ __forceinline__ void int8_params(float mn, float mx, float *min_val, float *scale) {
    if (mn == mx) {
        mn -= 0.1f;
        mx += 0.1f;
    }
    *min_val = mn;
    *scale = (mx - mn) / 255.0f;
}

__device__ __forceinline__ int rust_f32_as_i32(float v) {   // `as i32`: saturating, NaN -> 0
    if (v != v) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return (int)0x80000000;
    return (int)v;
}

// tensor.rs:2136-2143: q = round((x - min) / scale) as i32 + qmin, clamped to [-128, 127] (f32::round: half away from zero)
__device__ __forceinline__ int quant_int8(float x, float min_val, float scale) {
    const int v = rust_f32_as_i32(roundf((x - min_val) / scale));
    const long w = (long)v + (-128);
    return (int)(w < -128 ? -128 : (w > 127 ? 127 : w));
}

// the symmetric int8 activation code of calibrated inference (qgemm_i8.hip, qconv_i8.hip): th_fake_quant_act's code with a scale fixed
// beforehand -- clamp(round(v / scale) as i32, -128, 127), NaN -> 0, +-inf saturate
__device__ __forceinline__ int act_code(float v, float scale) {
    const int q = rust_f32_as_i32(roundf(v / scale));
    return q < -128 ? -128 : (q > 127 ? 127 : q);
}

// (q - zero_point) * scale + min_val with zero_point = -128: two roundings, never contracted (tensor.rs:357)
__device__ __forceinline__ float dequant_int8(int q, float scale, float min_val) { return __fadd_rn(__fmul_rn((float)(q + 128), scale), min_val); }

// A frozen BatchNorm2d behind a value: y = v a + b with the channel's folded pair, one multiply and one add rounded once
// each and never contracted, then the ReLU.  The int8 conv epilogue (qconv_i8.hip) and the standalone layer (quant.hip) both call this.
__device__ __forceinline__ float affine_value(float v, float a, float b, int relu) {
    const float y = __fadd_rn(__fmul_rn(v, a), b);
    return relu ? (y > 0.f ? y : 0.f) : y;
}

// The same with a skip connection's value r added behind the affine and in front of the ReLU, where th_bn_residual_fwd adds
// it in the float model: one more add, rounded once.
__device__ __forceinline__ float affine_residual_value(float v, float a, float b, float r, int relu) {
    const float y = __fadd_rn(__fadd_rn(__fmul_rn(v, a), b), r);
    return relu ? (y > 0.f ? y : 0.f) : y;
}

}  // namespace th
