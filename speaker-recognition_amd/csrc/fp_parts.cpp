// fp_parts.cpp -- host fp32 <-> fp16 / bf16 conversions and the part splits (fp_parts.hpp).
#include "fp_parts.hpp"

#include <cstring>

namespace sr {

static inline uint32_t f32_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}
static inline float bits_f32(uint32_t u) {
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}
static inline uint32_t bf16_rne_bits(float v) {   // fp32 bit pattern of v rounded to bf16
    const uint32_t u = f32_bits(v);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
}

void split_bf16x3(float v, uint16_t out[3]) {
    const uint32_t h = bf16_rne_bits(v);
    const float r1 = v - bits_f32(h);            // exact in fp32
    const uint32_t m = bf16_rne_bits(r1);
    const float r2 = r1 - bits_f32(m);           // exact
    const uint32_t l = bf16_rne_bits(r2);
    out[0] = (uint16_t)(h >> 16);
    out[1] = (uint16_t)(m >> 16);
    out[2] = (uint16_t)(l >> 16);
}

// IEEE binary16 <-> binary32 on the host (round-to-nearest-even, gradual underflow, saturating to
// +-inf like v_cvt_f16_f32); the packers must produce exactly what the device conversion would.
uint16_t f32_to_f16_rne(float v) {
    const uint32_t u = f32_bits(v);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const uint32_t a = u & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return (uint16_t)(sign | 0x7C00u | ((a > 0x7F800000u) ? 0x200u : 0u));
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);           // rounds to >= 65520 -> inf
    if (a < 0x33000001u) return (uint16_t)sign;                         // <= 2^-25 -> 0 (ties to even)
    int e = (int)(a >> 23) - 127;
    uint32_t mant = (a & 0x7FFFFFu) | 0x800000u;                        // 24 bits
    int shift = (e >= -14) ? 13 : (13 + (-14 - e));                     // bits dropped
    uint32_t q = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (q & 1u))) q++;
    uint32_t out;
    if (e >= -14)
        out = ((uint32_t)(e + 15) << 10) + (q - 0x400u);                // a carry out of q bumps the exponent
    else
        out = q;                                                        // subnormal (q == 0x400 becomes the smallest normal)
    return (uint16_t)(sign | out);
}

float f16_to_f32(uint16_t h) {
    const uint32_t sign = ((uint32_t)h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    if (e == 0x1F) return bits_f32(sign | 0x7F800000u | (m << 13));
    if (e == 0) {
        const float v = (float)m * 5.9604644775390625e-08f;            // m * 2^-24
        return sign ? -v : v;
    }
    return bits_f32(sign | ((e + 112u) << 23) | (m << 13));
}

void split_f16x2(float v, uint16_t out[2]) {
    out[0] = f32_to_f16_rne(v);
    const float r = v - f16_to_f32(out[0]);      // exact in fp32
    out[1] = f32_to_f16_rne(r);
}

}  // namespace sr
