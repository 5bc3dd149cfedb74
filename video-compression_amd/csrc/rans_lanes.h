// Per-lane steps of the interleaved range coder (include/vc_hip.h: "Interleaved range coder"), compiled for the host
// reference (rans_host.cpp, plain C++) and for the kernels (rans_device.hip): one statement of the arithmetic, the table
// lookup, the escape split and the header walk, so the two sides cannot drift apart.  Nothing here touches memory other
// than through the row pointer / word reader it is handed, and every loop is counted.
#pragma once
#include <stdint.h>

#ifdef __HIP__
#define IRL_HD __host__ __device__ __forceinline__
#else
#define IRL_HD inline
#endif

namespace irl {
constexpr int kLanes = 64;                    // lanes of a wave = states of a sub-stream
constexpr uint32_t kProbBits = 16;
constexpr uint64_t kLow = 1ull << 31;         // lower bound of a state; renormalisation moves one 32-bit word
constexpr uint32_t kHeaderWords = 1 + 2 * kLanes;   // u32 word count + 64 u64 states = 516 bytes

struct Row {                                  // one table of a packed set (vc_irans_pack_tables)
    int32_t start;                            // first u16 entry of the row
    int32_t size;                             // cdf_size: size - 1 slots, slot size - 2 is the escape
    int32_t offset;
    int32_t mode;                             // widest slot: where the search starts
};

IRL_HD bool waves_ok(int w) { return w >= 1 && w <= 16 && (w & (w - 1)) == 0; }

// Slots of a packed row.  Entries 0 .. size - 2 hold their true values (< 65536); the last one, 65536, wraps to 0 and is only
// ever read as the END of the last slot, where the u16 difference is the right frequency (1 .. 65535: rows are strictly increasing).
IRL_HD uint32_t slot_start(const uint16_t *row, int s) { return row[s]; }
IRL_HD uint32_t slot_freq(const uint16_t *row, int s) { return (uint16_t)(row[s + 1] - row[s]); }

// The slot that holds cumulative value `cum`: the largest s in [0, size - 2] with row[s] <= cum.  Gallops outwards from the
// mode, then bisects the bracket: a value near the mode costs two or three dependent reads whatever the row's length.
// Reads stay inside entries 0 .. size - 2 for any `cum`; at most 17 + 17 iterations (size <= 65537).
IRL_HD int lookup(const uint16_t *row, int size, int mode, uint32_t cum)
{
    int lo = 0, hi = size - 1;                // row[lo] <= cum; hi == size - 1 or row[hi] > cum
    int step = 1;
    if (row[mode] <= cum) {
        lo = mode;
        for (int k = 0; k < 17; ++k) {
            const int c = lo + step;
            if (c >= size - 1) break;
            if (row[c] > cum) { hi = c; break; }
            lo = c;
            step <<= 1;
        }
    } else {
        hi = mode;
        for (int k = 0; k < 17; ++k) {
            const int c = hi - step;
            if (c <= 0) break;
            if (row[c] <= cum) { lo = c; break; }
            hi = c;
            step <<= 1;
        }
    }
    for (int k = 0; k < 17 && hi - lo > 1; ++k) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] <= cum) lo = mid; else hi = mid;
    }
    return lo;
}

// Encoder step: a state at or above freq * 2^47 first moves its low word out (at most one: x < 2^63 always)
IRL_HD bool put_emits(uint64_t x, uint32_t freq) { return x >= ((uint64_t)freq << 47); }
IRL_HD uint64_t put(uint64_t x, uint32_t start, uint32_t freq) { return ((x / freq) << kProbBits) + (x % freq) + start; }
// Decoder step and its renormalisation (at most one word: the new state is >= 2^15)
IRL_HD uint32_t cum_of(uint64_t x) { return (uint32_t)(x & 0xffffu); }
IRL_HD uint64_t get(uint64_t x, uint32_t start, uint32_t freq) { return (uint64_t)freq * (x >> kProbBits) + (x & 0xffffu) - start; }
IRL_HD bool needs_word(uint64_t x) { return x < kLow; }
IRL_HD uint64_t take_word(uint64_t x, uint32_t w) { return (x << 32) | w; }

// Escape split.  A symbol whose value symbol - offset lies outside [0, size - 2) takes the escape slot, then two uniform
// 16-bit steps (frequency 1, start = the half) carry the zig-zag of the value modulo 2^32, low half first on the decoder.
IRL_HD int slot_of(int32_t symbol, const Row &r, bool &escaped)
{
    const int64_t v = (int64_t)symbol - r.offset;
    escaped = !(v >= 0 && v < r.size - 2);
    return escaped ? r.size - 2 : (int)v;
}
IRL_HD int32_t symbol_of(int slot, int32_t offset) { return (int32_t)((uint32_t)slot + (uint32_t)offset); }   // wraps like the escape path
IRL_HD uint32_t zigzag(int32_t symbol, int32_t offset)
{
    const uint32_t v = (uint32_t)symbol - (uint32_t)offset;
    return (v << 1) ^ (0u - (v >> 31));
}
IRL_HD int32_t unzigzag(uint32_t z, int32_t offset)
{
    const uint32_t v = (z >> 1) ^ (0u - (z & 1u));
    return (int32_t)(v + (uint32_t)offset);
}

// Header walk of a payload of `nwords` u32 read through word(i): W sub-streams of  count | 64 states | count words.  Fills
// base[w] (first word of sub-stream w, counted from base0) and count[w]; false when a header or a count does not fit or the
// sub-streams do not end exactly at nwords.  Nothing past nwords is read.
template <class WordAt>
IRL_HD bool walk_headers(WordAt word, uint64_t nwords, int waves, uint64_t base0, uint32_t *base, uint32_t *count)
{
    uint64_t pos = 0;
    for (int w = 0; w < waves; ++w) {
        if (nwords - pos < kHeaderWords) return false;
        const uint32_t c = word(pos);
        if (c > nwords - pos - kHeaderWords) return false;
        if (base0 + pos + kHeaderWords + c > 0xffffffffull) return false;
        base[w] = (uint32_t)(base0 + pos + kHeaderWords);
        count[w] = c;
        pos += kHeaderWords + c;
    }
    return pos == nwords;
}
}  // namespace irl
