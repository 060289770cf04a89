// Philox4x32-10 (Salmon et al., SC 2011), the project's one counter-based generator: the sampler (sample.hip) and the
// training windows (windows_gather.hip) include this body; nbdist.philox4x32 is the same function on the host.
#pragma once
#include <hip/hip_runtime.h>

struct PhiloxWords { unsigned x, y, z, w; };

// ten rounds, the key bumped by the Weyl constants between them
__device__ inline PhiloxWords ftn_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;  c1 = l1;
    c2 = h0 ^ c3 ^ k1;  c3 = l0;
    k0 += 0x9E3779B9u;  k1 += 0xBB67AE85u;
  }
  return {c0, c1, c2, c3};
}
