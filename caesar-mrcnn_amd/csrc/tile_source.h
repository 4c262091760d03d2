// Read accessors of the bit-mask sources of include/mrcnn_hip.h (mrcnn_tile_source), shared by tilemerge.hip and
// srcparams.hip: rows / words outside a source, padding bits past its width and addresses past the pool read as zero.
#pragma once
#include "common.h"

typedef mrcnn_tile_source TmSrc;

// Word k of local row `row` of a source; 0 outside the source or the pool, padding bits cleared.
__device__ __forceinline__ unsigned tm_word(const unsigned* __restrict__ pool, long long pool_words, const TmSrc& d, int row, int k) {
    if ((unsigned)row >= (unsigned)d.h || (unsigned)k >= (unsigned)d.words_per_row) return 0u;
    const long long a = (long long)d.word_offset + (long long)row * d.words_per_row + k;
    if (a < 0 || a >= pool_words) return 0u;
    unsigned v = pool[a];
    const int valid = d.w - 32 * k;                          // bits of this word inside the box
    if (valid < 32) v &= valid <= 0 ? 0u : (0xFFFFFFFFu >> (32 - valid));
    return v;
}

// The 32 bits of local row `row` that start at local bit `xbit` (any integer: negative or past the row reads zeros): a
// funnel shift across the two words that cover them.
__device__ __forceinline__ unsigned tm_bits(const unsigned* __restrict__ pool, long long pool_words, const TmSrc& d, int row, int xbit) {
    if ((unsigned)row >= (unsigned)d.h || xbit <= -32 || xbit >= d.w) return 0u;
    const int k = xbit >> 5, s = xbit & 31;                  // arithmetic shift: floor for negative xbit
    const unsigned lo = tm_word(pool, pool_words, d, row, k);
    if (!s) return lo;
    const unsigned hi = tm_word(pool, pool_words, d, row, k + 1);
    return (lo >> s) | (hi << (32 - s));
}

__device__ __forceinline__ bool tm_valid(const TmSrc& d) {
    return d.w > 0 && d.h > 0 && d.words_per_row >= ((d.w + 31) >> 5) && d.word_offset >= 0;
}
