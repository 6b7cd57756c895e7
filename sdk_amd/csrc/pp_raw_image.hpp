// The raw image of a client's public parameters, built on the device from the wire image (sp_pp_expand, sp_pp_expand_into; the
// descriptor is beside PpRawDesc in kernels.hpp): what sp_pp_deserialize builds on the host -- row 0 of every matrix from the seed's
// ChaCha20 stream as modulus - (ks % modulus) (client.rs:47-49), the other rows the wire's words as sent.
//
// One workgroup per polynomial, one thread per ChaCha block: 16 keystream words = 8 output words, 256 blocks per polynomial, so a
// polynomial's keystream starts on a block boundary and thread t of the workgroup takes block (first word / 8) + t.  The table entry is
// the workgroup's (scalar), so a workgroup is all keystream or all copy.  The key is words 0 .. 7 of the wire image, the same for every
// thread: it is read with uniform loads and costs no vector register.
// Included by elementwise.hip only.
#pragma once

namespace spiral {

__device__ __forceinline__ u32 pri_rotl(u32 v, int c) { return (v << c) | (v >> (32 - c)); }
#define SP_PRI_QR(a, b, c, d)                         \
  a += b; d = pri_rotl(d ^ a, 16);                    \
  c += d; b = pri_rotl(b ^ c, 12);                    \
  a += b; d = pri_rotl(d ^ a, 8);                     \
  c += d; b = pri_rotl(b ^ c, 7);

// block `ctr` of rand_chacha's ChaCha20Rng (64-bit counter in words 12 | 13, stream 0) -> out[8], u64 k = words 2k (low) | 2k + 1
__device__ __forceinline__ void pri_chacha_block(const u32* key, u64 ctr, u64 out[8]) {
  const u32 c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u, c3 = 0x6b206574u;
  const u32 k0 = key[0], k1 = key[1], k2 = key[2], k3 = key[3], k4 = key[4], k5 = key[5], k6 = key[6], k7 = key[7];
  const u32 n0 = (u32)ctr, n1 = (u32)(ctr >> 32);
  u32 x0 = c0, x1 = c1, x2 = c2, x3 = c3, x4 = k0, x5 = k1, x6 = k2, x7 = k3, x8 = k4, x9 = k5, x10 = k6, x11 = k7, x12 = n0, x13 = n1,
      x14 = 0, x15 = 0;
  // (a loop of ten double rounds, not 960 straight-line instructions: unrolled, the compiler keeps several hundred values of the
  // first, partly uniform, rounds live and spills them)
#pragma unroll 1
  for (int rnd = 0; rnd < 10; rnd++) {
    SP_PRI_QR(x0, x4, x8, x12) SP_PRI_QR(x1, x5, x9, x13) SP_PRI_QR(x2, x6, x10, x14) SP_PRI_QR(x3, x7, x11, x15)
    SP_PRI_QR(x0, x5, x10, x15) SP_PRI_QR(x1, x6, x11, x12) SP_PRI_QR(x2, x7, x8, x13) SP_PRI_QR(x3, x4, x9, x14)
  }
  out[0] = (u64)(x0 + c0) | ((u64)(x1 + c1) << 32);
  out[1] = (u64)(x2 + c2) | ((u64)(x3 + c3) << 32);
  out[2] = (u64)(x4 + k0) | ((u64)(x5 + k1) << 32);
  out[3] = (u64)(x6 + k2) | ((u64)(x7 + k3) << 32);
  out[4] = (u64)(x8 + k4) | ((u64)(x9 + k5) << 32);
  out[5] = (u64)(x10 + k6) | ((u64)(x11 + k7) << 32);
  out[6] = (u64)(x12 + n0) | ((u64)(x13 + n1) << 32);
  out[7] = (u64)x14 | ((u64)x15 << 32);
}
#undef SP_PRI_QR

// grid (polynomials), 256 threads.  Words at or past d.n_words are not written (a keystream request that ends inside a block).
// Eight waves per SIMD: a thread holds the 16 working words, 8 outputs and addresses.
__global__ __launch_bounds__(256, 8) void k_pp_raw_image(PpRawDesc d) {
  const u64 entry = d.table[blockIdx.x];
  const u64 first = entry & ~PP_RAW_WIRE;
  const u64 o = (u64)blockIdx.x * N + 8u * threadIdx.x;
  if (o >= d.n_words) return;
  u64 w[8];
  if (entry & PP_RAW_WIRE) {
    const u64* src = d.wire + first + 8u * threadIdx.x;
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = src[k];
  } else {
    pri_chacha_block(reinterpret_cast<const u32*>(d.wire), (first >> 3) + threadIdx.x, w);
    if (d.modulus) {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        // ks % modulus: the quotient estimate is at most 2 short (modulus < 2^63); a remainder of 0 gives the word `modulus`
        u64 r = w[k] - __umul64hi(w[k], d.modulus_inv) * d.modulus;
        while (r >= d.modulus) r -= d.modulus;
        w[k] = d.modulus - r;
      }
    }
  }
  u64* dst = d.dst + o;
  if (o + 8 <= d.n_words) {
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = w[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (o + (u64)k < d.n_words) dst[k] = w[k];
  }
}

void launch_pp_raw_image(const PpRawDesc& d, int n_polys, hipStream_t s) {
  if (n_polys <= 0 || d.n_words == 0) return;
  hipLaunchKernelGGL(k_pp_raw_image, dim3((unsigned)n_polys), dim3(256), 0, s, d);
  launched(0, "k_pp_raw_image");
}

}  // namespace spiral
