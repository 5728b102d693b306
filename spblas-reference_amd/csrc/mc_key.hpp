// The fixed vertex priorities of the graph algorithms that run in rounds (multicolor.hip, aggregate.hip; not part of the ABI).
//   key(v) = (uint64(h(v)) << 32) | v, compared unsigned;  h(v) = mix(uint32(v + 1) * 0x9E3779B1u);
//   mix(x): x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16  (32-bit wraparound).
// The low word is the vertex itself, so two vertices never share a key and a key names its vertex.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spb {

__device__ __forceinline__ uint64_t mc_key(int v) {
  uint32_t x = ((uint32_t) v + 1u) * 0x9E3779B1u;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return ((uint64_t) x << 32) | (uint32_t) v;
}

} // namespace spb
