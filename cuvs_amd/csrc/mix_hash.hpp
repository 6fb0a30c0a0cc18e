// The one 32-bit hash of (seed, i) that fixes the library's pseudo-random choices: the HNSW levels (hnsw_host.hpp level_hash,
// DESIGN 3.1r) and the landmark draw of the ball cover (ball_cover_host.hpp). Files and test twins depend on its
// values (tests/hnsw_ref.py level_hash restates it), so it does not change. Pure C++, no HIP include.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CUVS_AMD_MIX_HD __host__ __device__
#else
#define CUVS_AMD_MIX_HD
#endif

namespace cuvs_amd {

// the finalizer of MurmurHash3 over i + seed * golden ratio
CUVS_AMD_MIX_HD inline uint32_t mix_hash(uint32_t seed, uint32_t i)
{
  uint32_t x = i + seed * 0x9E3779B9u;
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

}  // namespace cuvs_amd
