// float <-> IEEE binary16 bit patterns, the same on the device (v_cvt) and in the CPU replay (round to nearest even):
// the hi / lo operand split of the binary16 matrix-core kernels (resample_mfma.h, the fused MFCC's DCT fragments).
#pragma once
#include <cstring>
#include <cstdint>
#include "hd.h"

namespace aamd {
namespace rsm {

AAMD_HD uint16_t f16_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f));
#else
  uint32_t u;                                   // round to nearest even, subnormals kept (what v_cvt_f16_f32 does)
  std::memcpy(&u, &f, 4);
  const uint32_t sign = u & 0x80000000u;
  u ^= sign;
  uint16_t o;
  if (u >= ((127u + 16u) << 23)) {
    o = (u > (255u << 23)) ? 0x7e00 : 0x7c00;
  } else if (u < (113u << 23)) {
    const uint32_t magic = ((127u - 15u) + (23u - 10u) + 1u) << 23;
    float t, mf;
    std::memcpy(&t, &u, 4);
    std::memcpy(&mf, &magic, 4);
    t += mf;
    uint32_t tu;
    std::memcpy(&tu, &t, 4);
    o = (uint16_t)(tu - magic);
  } else {
    const uint32_t odd = (u >> 13) & 1u;
    u += ((15u - 127u) << 23) + 0xfffu;
    u += odd;
    o = (uint16_t)(u >> 13);
  }
  return (uint16_t)(o | (sign >> 16));
#endif
}
AAMD_HD float f16_value(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
  return static_cast<float>(__builtin_bit_cast(_Float16, h));
#else
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 31u, m = h & 1023u, u;
  if (e == 0) {
    if (m == 0) { u = sign; }
    else {
      int sh = 0;
      while (!(m & 1024u)) { m <<= 1; ++sh; }
      u = sign | ((uint32_t)(113 - sh) << 23) | ((m & 1023u) << 13);
    }
  } else if (e == 31) {
    u = sign | 0x7f800000u | (m << 13);
  } else {
    u = sign | ((e + 112u) << 23) | (m << 13);
  }
  float f;
  std::memcpy(&f, &u, 4);
  return f;
#endif
}

}  // namespace rsm
}  // namespace aamd
