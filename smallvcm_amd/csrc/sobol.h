// sobol.h -- the second sampler: a padded two-dimensional Sobol sequence with hash-based Owen scrambling (Burley,
// "Practical Hash-based Owen Scrambling", JCGT 2020), host+device, beside philox.h.  No direction-number tables.
//
// Float k of stream (seed, path, kind) at sample index i = the renderer's local iteration:
//   pair j = k >> 1, component c = k & 1
//   (s0, s1, s2) = words 0..2 of philox4x32_10(counter = (path, kind, j, 1), key = (seed, 0)): a function of the stream
//                  and the pair, NOT of i; counter word 3 = 1 keeps them apart from every Philox stream (word 3 = 0)
//   i' = brev(lk(brev(i), s0))                the index, shuffled per pair by an Owen scramble of its reversed bits (blocks
//                                             a 2^m .. (a + 1) 2^m - 1 map to such blocks): pairs of a path are decorrelated
//   c = 0: w = brev(lk(i', s1))               Sobol dimension 0 (the radical inverse), Owen-scrambled
//   c = 1: w = brev(lk(T(i'), s2))            Sobol dimension 1 (brev(T(x)): the Pascal matrix mod 2), Owen-scrambled
//   float  = rng_word_to_float(w)             as under Philox: an odd multiple of 2^-24 in (0, 1)
// For fixed (seed, path, kind, j) the points of i = a 2^m .. (a + 1) 2^m - 1 form a (0, m, 2)-net in base 2, also after
// the truncation to the 23 bits the float keeps (m <= 23).
//
// A draw group of a path starts on the parity that makes its 2-D uses pairs (sobol_align; DESIGN.md "Sampler").  The
// skipped position is never generated but counts as drawn.  Bound on k: a light path draws 6 + 4 per bounce, a camera
// path 2 + at most 8 per vertex (1 skipped + 3 direct illumination + 4 scattering), so k <= 2 + 8 * 255 = 2042 at the
// largest supported maxPathLength (255): far inside 32 bits.  The per-path count byte of vcm_get_rng_counts holds k
// exactly up to maxPathLength 31 (k <= 250), which is every wavefront iteration, and k mod 256 beyond, as under Philox.
#ifndef SMALLVCM_AMD_SOBOL_H
#define SMALLVCM_AMD_SOBOL_H
#include "philox.h"

namespace vcm {

VCM_HD uint32_t sobol_brev(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    return (x >> 16) | (x << 16);
#endif
}
/* Laine-Karras: a hash in which bit b of the result depends on bits <= b of x only, i.e. an Owen scramble of brev(x) */
VCM_HD uint32_t sobol_lk(uint32_t x, uint32_t s)
{
    x += s;
    x ^= x * 0x6c50b47cu;
    x ^= x * 0xb82f1e52u;
    x ^= x * 0xc7afe638u;
    x ^= x * 0x8d22f6e6u;
    return x;
}
/* brev(T(x)) = the second Sobol dimension of index x (the Pascal matrix mod 2) */
VCM_HD uint32_t sobol_t(uint32_t x)
{
    x ^= (x >> 1) & 0x55555555u;
    x ^= (x >> 2) & 0x33333333u;
    x ^= (x >> 4) & 0x0f0f0f0fu;
    x ^= (x >> 8) & 0x00ff00ffu;
    x ^= (x >> 16) & 0x0000ffffu;
    return x;
}
/* both words of pair j */
VCM_HD void sobol_pair(uint32_t seed, uint32_t i, uint32_t path, uint32_t kind, uint32_t j, uint32_t &w0, uint32_t &w1)
{
    uint32_t s0, s1, s2, s3;
    philox4x32_10(path, kind, j, 1u, seed, 0u, s0, s1, s2, s3);
    (void)s3;
    const uint32_t is = sobol_brev(sobol_lk(sobol_brev(i), s0));
    w0 = sobol_brev(sobol_lk(is, s1));
    w1 = sobol_brev(sobol_lk(sobol_t(is), s2));
}
/* the word of float k: the definition (known answers, tests); the path code uses sobol_peek */
VCM_HD uint32_t sobol_word(uint32_t seed, uint32_t i, uint32_t path, uint32_t kind, uint32_t k)
{
    uint32_t w0, w1;
    sobol_pair(seed, i, path, kind, k >> 1, w0, w1);
    return (k & 1u) ? w1 : w0;
}
/* the position at or after k with the parity `odd` (0 / 1) */
VCM_HD uint32_t sobol_align(uint32_t k, uint32_t odd) { return ((k + 1u - odd) & ~1u) | odd; }

/* rng_peek's counterpart: floats k0 .. k0+n-1 of the path's stream (key1 = the sample index), n <= 8.  The n floats
   touch at most n/2 + 1 pairs, all generated at this one site by all lanes; the parity of k0 selects, no dynamic
   indexing.  Every site of the path code passes an aligned k0, whose parity the compiler sees. */
VCM_HD void sobol_peek(const PathRng &r, uint32_t k0, float *out, int n)
{
    uint32_t w[10];
    const uint32_t j0 = k0 >> 1, o = k0 & 1u;
    const int np = (n + 2) >> 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int p = 0; p < np; p++) {
        if (p == np - 1 && (n & 1) == 0 && o == 0u) { w[2 * p] = 0u; w[2 * p + 1] = 0u; continue; }   /* an even run from an even k0 ends one pair earlier */
        sobol_pair(r.key0, r.key1, r.path, r.kind, j0 + (uint32_t)p, w[2 * p], w[2 * p + 1]);
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < n; t++) out[t] = rng_word_to_float(o ? w[t + 1] : w[t]);
}

} // namespace vcm
#endif
