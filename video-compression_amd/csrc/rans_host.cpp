// Host range coder of the product: rans64 (32-bit word renormalisation, L = 2^31), 16-bit table
// probabilities, 4-bit bypass escape -- the bitstream format of CompressAI's ans module that the
// reference reaches through EntropyModel.compress/decompress (LHBDC/model/layers.py:97-112).
//
// The state machine is inherently serial, so it runs on a host core while the GPU produces the next
// frame's symbols.  Unlike the queue-then-flush formulation, the encoder walks the symbols once,
// backwards, expanding escapes in reverse on the fly and writing 32-bit words from the end of the
// caller's buffer -- no intermediate symbol queue, no allocation.
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>
#include "vc_hip.h"
#include "rans_lanes.h"

namespace {
// every table must fit its row and hold at least one real bin + the escape bin
bool tables_ok(const int32_t *cdf_sizes, int n_tables, int cdf_stride)
{
    if (n_tables < 1 || cdf_stride < 3) return false;
    for (int t = 0; t < n_tables; ++t)
        if (cdf_sizes[t] < 3 || cdf_sizes[t] > cdf_stride) return false;
    return true;
}

constexpr uint32_t kProbBits = 16;
constexpr uint32_t kBypassBits = 4;
constexpr uint32_t kBypassMax = (1u << kBypassBits) - 1u;
constexpr uint64_t kLow = 1ull << 31;

struct Encoder {
    uint64_t x = kLow;
    uint32_t *p;      // next free word (grows downwards)
    uint32_t *floor;  // lowest legal address
    bool overflow = false;

    inline void emit()
    {
        if (p == floor) { overflow = true; return; }
        *--p = static_cast<uint32_t>(x);
        x >>= 32;
    }
    inline void put(uint32_t start, uint32_t range)
    {
        const uint64_t lim = ((kLow >> kProbBits) << 32) * range;
        if (x >= lim) emit();
        x = ((x / range) << kProbBits) + (x % range) + start;
    }
    inline void put_nibble(uint32_t v)
    {
        const uint64_t lim = ((kLow >> 16) << 32) * static_cast<uint64_t>(1u << (16 - kBypassBits));
        if (x >= lim) emit();
        x = (x << kBypassBits) | v;
    }
};
}  // namespace

extern "C" size_t vc_rans_bound(size_t count) { return 4 * (2 * count + 4); }

extern "C" long long vc_rans_encode_with_indexes(const int32_t *symbols, const int32_t *indexes, size_t count,
                                                 const int32_t *cdfs, int n_tables, int cdf_stride,
                                                 const int32_t *cdf_sizes, const int32_t *offsets, uint8_t *out, size_t out_cap)
{
    if ((count && (!symbols || !indexes)) || !cdfs || !cdf_sizes || !offsets || !out || out_cap < 8) return VC_EINVAL;
    if (reinterpret_cast<uintptr_t>(out) % 4) return VC_EINVAL;
    if (!tables_ok(cdf_sizes, n_tables, cdf_stride)) return VC_EINVAL;
    const size_t cap_words = out_cap / 4;
    uint32_t *base = reinterpret_cast<uint32_t *>(out);
    Encoder enc;
    enc.p = base + cap_words;
    enc.floor = base + 2;  // keep room for the final flush
    for (size_t i = count; i-- > 0;) {
        const int32_t t = indexes[i];
        if (static_cast<uint32_t>(t) >= static_cast<uint32_t>(n_tables)) return VC_EINVAL;
        const int32_t *cdf = cdfs + static_cast<size_t>(t) * cdf_stride;
        const int32_t escape = cdf_sizes[t] - 2;
        // (64-bit: a symbol rounded from an inf / NaN latent is INT_MIN or huge, and `symbol - offset`, `-2 v - 1`,
        //  `2 (v - escape)` must not overflow before the range check below refuses it)
        const int64_t v = static_cast<int64_t>(symbols[i]) - offsets[t];
        if (v >= 0 && v < escape) {
            enc.put(static_cast<uint32_t>(cdf[v]), static_cast<uint32_t>(cdf[v + 1] - cdf[v]));
            continue;
        }
        // out-of-table value: sign/magnitude folded into `raw`, sent as nibbles after the escape bin
        const int64_t raw64 = v < 0 ? -2 * v - 1 : 2 * (v - escape);
        // (the format's own encoder counts nibbles with `raw >> (n*4)` on a 32-bit value: undefined from 2^28 on, so
        //  magnitudes that need an eighth nibble have no defined encoding -- refuse them)
        if (raw64 >> 28) return VC_EINVAL;
        const uint32_t raw = static_cast<uint32_t>(raw64);
        int32_t nibbles = 0;
        while ((raw >> (nibbles * kBypassBits)) != 0) ++nibbles;
        for (int32_t j = nibbles - 1; j >= 0; --j) enc.put_nibble((raw >> (j * kBypassBits)) & kBypassMax);
        // nibble count in base-15 "unary" chunks; forward order is 15,15,...,rest -> reverse: rest first
        enc.put_nibble(static_cast<uint32_t>(nibbles) % kBypassMax);
        for (int32_t c = nibbles / static_cast<int32_t>(kBypassMax); c > 0; --c) enc.put_nibble(kBypassMax);
        enc.put(static_cast<uint32_t>(cdf[escape]), static_cast<uint32_t>(cdf[escape + 1] - cdf[escape]));
    }
    if (enc.overflow) return VC_ENOMEM;
    enc.p -= 2;
    enc.p[0] = static_cast<uint32_t>(enc.x);
    enc.p[1] = static_cast<uint32_t>(enc.x >> 32);
    const size_t nbytes = static_cast<size_t>((base + cap_words) - enc.p) * 4;
    std::memmove(out, enc.p, nbytes);
    return static_cast<long long>(nbytes);
}

namespace {
// Decoder core, resumable: `x` / `pos` = coder state and index of the next unread 32-bit word.  A fresh stream starts
// with pos == 0 (the first two words initialise x).
int decode_core(const uint8_t *data, size_t nbytes, uint64_t &x, size_t &pos, const int32_t *indexes, size_t count,
                const int32_t *cdfs, int n_tables, int cdf_stride, const int32_t *cdf_sizes, const int32_t *offsets, int32_t *out)
{
    const size_t nwords = nbytes / 4;
    auto next_word = [&](uint32_t &w) -> bool {
        if (pos >= nwords) return false;
        std::memcpy(&w, data + 4 * pos, 4);
        ++pos;
        return true;
    };
    if (pos == 0) {
        uint32_t lo = 0, hi = 0;
        if (!next_word(lo) || !next_word(hi)) return VC_EDATA;
        x = static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32);
    }
    bool bad = false;
    auto refill = [&]() {
        if (x < kLow) {
            uint32_t w = 0;
            if (!next_word(w)) bad = true;
            x = (x << 32) | w;
        }
    };
    auto nibble = [&]() -> uint32_t {
        const uint32_t v = static_cast<uint32_t>(x & kBypassMax);
        x >>= kBypassBits;
        refill();
        return v;
    };
    // Symbol lookup: the format's reference decoder scans the table linearly.  Here every table gets a 256-entry
    // jump table over the top 8 bits of the cumulative value (first bin that can contain it), built once per call
    // (n_tables x 256 steps, negligible next to the symbols); the scan then starts at most a few bins before the
    // answer whatever the table length -- the decoder is what a frame's host time is made of (1 M symbols).
    constexpr int kLutBits = 8;
    thread_local std::vector<uint16_t> lut;
    lut.resize(static_cast<size_t>(n_tables) << kLutBits);
    for (int t = 0; t < n_tables; ++t) {
        const int32_t *cdf = cdfs + static_cast<size_t>(t) * cdf_stride;
        const int32_t n = cdf_sizes[t];
        uint16_t *row = lut.data() + (static_cast<size_t>(t) << kLutBits);
        int32_t j = 0;
        for (uint32_t b = 0; b < (1u << kLutBits); ++b) {
            const uint32_t lo = b << (16 - kLutBits);
            while (j + 1 < n - 1 && static_cast<uint32_t>(cdf[j + 1]) <= lo) ++j;   // last bin starting at or before lo
            row[b] = static_cast<uint16_t>(j);
        }
    }
    for (size_t i = 0; i < count; ++i) {
        const int32_t t = indexes[i];
        if (static_cast<uint32_t>(t) >= static_cast<uint32_t>(n_tables)) return VC_EINVAL;
        const int32_t *cdf = cdfs + static_cast<size_t>(t) * cdf_stride;
        const int32_t n = cdf_sizes[t], escape = n - 2;
        const uint32_t cum = static_cast<uint32_t>(x & 0xFFFFu);
        int32_t sidx = lut[(static_cast<size_t>(t) << kLutBits) + (cum >> (16 - kLutBits))];
        while (sidx + 1 < n - 1 && static_cast<uint32_t>(cdf[sidx + 1]) <= cum) ++sidx;
        const uint32_t start = static_cast<uint32_t>(cdf[sidx]);
        const uint32_t range = static_cast<uint32_t>(cdf[sidx + 1]) - start;
        x = static_cast<uint64_t>(range) * (x >> kProbBits) + (x & 0xFFFFu) - start;
        refill();
        int32_t v = sidx;
        if (v == escape) {
            uint32_t got = nibble(), nibbles = got;
            while (got == kBypassMax) {
                got = nibble();
                nibbles += got;
                if (bad || nibbles > 7) break;
            }
            if (nibbles > 7) return VC_EDATA;      // no encoder of this format emits more than 7 (see the encoder)
            uint32_t raw = 0;
            for (uint32_t k = 0; k < nibbles; ++k) raw |= nibble() << (k * kBypassBits);
            v = static_cast<int32_t>(raw >> 1);
            if (raw & 1u) v = -v - 1; else v += escape;
        }
        if (bad) return VC_EDATA;
        out[i] = v + offsets[t];
    }
    return VC_OK;
}
}  // namespace

extern "C" int vc_rans_decode_with_indexes(const uint8_t *data, size_t nbytes, const int32_t *indexes, size_t count,
                                           const int32_t *cdfs, int n_tables, int cdf_stride, const int32_t *cdf_sizes,
                                           const int32_t *offsets, int32_t *out)
{
    if (!data || nbytes < 8 || (nbytes % 4) || (count && (!indexes || !out)) || !cdfs || !cdf_sizes || !offsets) return VC_EINVAL;
    if (!tables_ok(cdf_sizes, n_tables, cdf_stride)) return VC_EINVAL;
    uint64_t x = 0;
    size_t pos = 0;
    return decode_core(data, nbytes, x, pos, indexes, count, cdfs, n_tables, cdf_stride, cdf_sizes, offsets, out);
}

extern "C" int vc_rans_decode_stream(const uint8_t *data, size_t nbytes, uint64_t *state, const int32_t *indexes, size_t count,
                                     const int32_t *cdfs, int n_tables, int cdf_stride, const int32_t *cdf_sizes,
                                     const int32_t *offsets, int32_t *out)
{
    if (!data || nbytes < 8 || (nbytes % 4) || !state || (count && (!indexes || !out)) || !cdfs || !cdf_sizes || !offsets) return VC_EINVAL;
    if (!tables_ok(cdf_sizes, n_tables, cdf_stride)) return VC_EINVAL;
    uint64_t x = state[0];
    size_t pos = static_cast<size_t>(state[1]);
    if (pos == 1 || pos > nbytes / 4) return VC_EINVAL;
    const int rc = decode_core(data, nbytes, x, pos, indexes, count, cdfs, n_tables, cdf_stride, cdf_sizes, offsets, out);
    state[0] = x;
    state[1] = pos;
    return rc;
}

extern "C" int vc_pmf_to_quantized_cdf(const float *pmf, int n, int precision, uint32_t *cdf)
{
    if (!pmf || !cdf || n < 1 || precision != 16) return VC_EINVAL;
    const uint32_t one = 1u << precision;
    std::vector<uint32_t> freq(static_cast<size_t>(n) + 1, 0u);
    for (int i = 0; i < n; ++i) {
        // a probability; anything else (NaN from a broken checkpoint, negative, > 1) has no defined conversion to an integer
        if (!(pmf[i] >= 0.0f && pmf[i] <= 1.0f)) return VC_EDATA;
        freq[i + 1] = static_cast<uint32_t>(std::round(pmf[i] * static_cast<float>(one)));
    }
    const uint32_t total = std::accumulate(freq.begin(), freq.end(), 0u);
    if (total == 0) return VC_EDATA;
    for (auto &f : freq) f = static_cast<uint32_t>((static_cast<uint64_t>(one) * f) / total);
    std::partial_sum(freq.begin(), freq.end(), cdf);
    cdf[n] = one;
    for (int i = 0; i < n; ++i) {
        if (cdf[i] != cdf[i + 1]) continue;
        uint32_t best = ~0u;
        int donor = -1;
        for (int j = 0; j < n; ++j) {
            const uint32_t f = cdf[j + 1] - cdf[j];
            if (f > 1 && f < best) { best = f; donor = j; }
        }
        if (donor < 0) return VC_EDATA;
        if (donor < i) for (int j = donor + 1; j <= i; ++j) --cdf[j];
        else for (int j = i + 1; j <= donor; ++j) ++cdf[j];
    }
    return VC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Interleaved coder, host reference: the 64 W lanes emulated with loops over the per-lane steps of rans_lanes.h, which
// the kernels of rans_device.hip run in lockstep.  The yardstick of those kernels and what the CPU tests exercise.
// ------------------------------------------------------------------------------------------------------------------
extern "C" size_t vc_irans_wave_words(size_t count, int waves)
{
    if (!irl::waves_ok(waves)) return 0;
    const size_t lanes = static_cast<size_t>(irl::kLanes) * waves;
    return 3 * irl::kLanes * (count / lanes + (count % lanes != 0));
}

extern "C" size_t vc_irans_bound(size_t count, int waves)
{
    if (!irl::waves_ok(waves)) return 0;
    return static_cast<size_t>(waves) * (VC_IRANS_SUBSTREAM_HEADER + 4 * vc_irans_wave_words(count, waves));
}

extern "C" long long vc_irans_pack_tables(const int32_t *cdfs, int n_tables, int cdf_stride, const int32_t *cdf_sizes,
                                          const int32_t *offsets, uint16_t *cdf16_out, int32_t *rows_out)
{
    if (!cdfs || !cdf_sizes || !offsets || !tables_ok(cdf_sizes, n_tables, cdf_stride)) return VC_EINVAL;
    long long total = 0;
    for (int t = 0; t < n_tables; ++t) {
        const int32_t *cdf = cdfs + static_cast<size_t>(t) * cdf_stride;
        const int32_t n = cdf_sizes[t];
        if (n > 65537 || cdf[0] != 0 || cdf[n - 1] != 65536) return VC_EINVAL;
        int32_t mode = 0, widest = 0;
        for (int32_t i = 0; i + 1 < n; ++i) {
            if (cdf[i + 1] <= cdf[i]) return VC_EINVAL;               // every slot can be coded, none is wider than 65535
            if (cdf[i + 1] - cdf[i] > widest) { widest = cdf[i + 1] - cdf[i]; mode = i; }
        }
        if (total + n > 0x7fffff00ll) return VC_EINVAL;
        if (cdf16_out)
            for (int32_t i = 0; i < n; ++i) cdf16_out[total + i] = static_cast<uint16_t>(cdf[i]);
        if (rows_out) {
            rows_out[4 * t + 0] = static_cast<int32_t>(total);
            rows_out[4 * t + 1] = n;
            rows_out[4 * t + 2] = offsets[t];
            rows_out[4 * t + 3] = mode;
        }
        total += n;
    }
    const long long padded = (total + 7) / 8 * 8;
    if (cdf16_out)
        for (long long i = total; i < padded; ++i) cdf16_out[i] = 0;
    return padded;
}

namespace {
struct PackedSet {
    std::vector<uint16_t> cdf16;
    std::vector<irl::Row> rows;
};

int pack_sets(const vc_irans_tables *sets, int n_sets, std::vector<PackedSet> &packed)
{
    if (!sets || n_sets < 1) return VC_EINVAL;
    packed.resize(static_cast<size_t>(n_sets));
    for (int k = 0; k < n_sets; ++k) {
        const vc_irans_tables &s = sets[k];
        const long long n = vc_irans_pack_tables(s.cdfs, s.n_tables, s.cdf_stride, s.cdf_sizes, s.offsets, nullptr, nullptr);
        if (n < 0) return static_cast<int>(n);
        packed[k].cdf16.resize(static_cast<size_t>(n));
        packed[k].rows.resize(static_cast<size_t>(s.n_tables));
        static_assert(sizeof(irl::Row) == 4 * sizeof(int32_t), "Row is the [n_tables][4] int32 layout");
        vc_irans_pack_tables(s.cdfs, s.n_tables, s.cdf_stride, s.cdf_sizes, s.offsets, packed[k].cdf16.data(),
                             reinterpret_cast<int32_t *>(packed[k].rows.data()));
    }
    return VC_OK;
}

bool segments_ok(const vc_irans_segment *segs, int n_segs, int n_sets)
{
    if (n_segs < 0 || (n_segs && !segs)) return false;
    for (int s = 0; s < n_segs; ++s) {
        if (segs[s].table_set < 0 || segs[s].table_set >= n_sets) return false;
        if (segs[s].count && (!segs[s].symbols || !segs[s].indexes)) return false;
    }
    return true;
}

struct WordsAt {                               // u32 i of a byte buffer of any alignment
    const uint8_t *p;
    uint32_t operator()(uint64_t i) const
    {
        uint32_t w;
        std::memcpy(&w, p + 4 * i, 4);
        return w;
    }
};
}  // namespace

extern "C" long long vc_irans_encode_host(const vc_irans_segment *segs, int n_segs, const vc_irans_tables *sets, int n_sets, int waves,
                                          uint8_t *out, size_t out_cap)
{
    if (!out || !irl::waves_ok(waves) || !segments_ok(segs, n_segs, n_sets)) return VC_EINVAL;
    std::vector<PackedSet> packed;
    if (const int rc = pack_sets(sets, n_sets, packed)) return rc;
    const size_t lanes = static_cast<size_t>(irl::kLanes) * waves;
    std::vector<uint64_t> x(lanes, irl::kLow);
    std::vector<std::vector<uint32_t>> emitted(static_cast<size_t>(waves));    // per wave, in the order the encoder emits: the decoder's, reversed
    for (int s = n_segs; s-- > 0;) {
        const vc_irans_segment &seg = segs[s];
        const PackedSet &set = packed[seg.table_set];
        const int n_tables = static_cast<int>(set.rows.size());
        for (size_t i = 0; i < seg.count; ++i)
            if (static_cast<uint32_t>(seg.indexes[i]) >= static_cast<uint32_t>(n_tables)) return VC_EINVAL;
        const size_t rounds = seg.count / lanes + (seg.count % lanes != 0);
        for (size_t r = rounds; r-- > 0;)
            for (int step = 2; step >= 0; --step)             // high half, low half, the symbol's slot: the decoder's three sub-steps backwards
                for (size_t g = lanes; g-- > 0;) {            // descending lanes: the decoder takes its words in ascending lane order
                    const size_t i = r * lanes + g;
                    if (i >= seg.count) continue;
                    const irl::Row &row = set.rows[seg.indexes[i]];
                    const uint16_t *cdf = set.cdf16.data() + row.start;
                    bool escaped;
                    const int slot = irl::slot_of(seg.symbols[i], row, escaped);
                    if (step && !escaped) continue;
                    const uint32_t zz = irl::zigzag(seg.symbols[i], row.offset);
                    const uint32_t start = step == 2 ? zz >> 16 : step == 1 ? (zz & 0xffffu) : irl::slot_start(cdf, slot);
                    const uint32_t freq = step ? 1u : irl::slot_freq(cdf, slot);
                    if (irl::put_emits(x[g], freq)) {
                        emitted[g / irl::kLanes].push_back(static_cast<uint32_t>(x[g]));
                        x[g] >>= 32;
                    }
                    x[g] = irl::put(x[g], start, freq);
                }
    }
    size_t need = 0;
    for (const auto &e : emitted) need += VC_IRANS_SUBSTREAM_HEADER + 4 * e.size();
    if (need > out_cap) return VC_ENOMEM;
    uint8_t *p = out;
    for (int w = 0; w < waves; ++w) {
        const std::vector<uint32_t> &e = emitted[w];
        if (e.size() > 0xffffffffull) return VC_EINVAL;
        const uint32_t count = static_cast<uint32_t>(e.size());
        std::memcpy(p, &count, 4);
        std::memcpy(p + 4, x.data() + static_cast<size_t>(w) * irl::kLanes, 8 * irl::kLanes);
        p += VC_IRANS_SUBSTREAM_HEADER;
        for (size_t k = e.size(); k-- > 0; p += 4) std::memcpy(p, &e[k], 4);
    }
    return static_cast<long long>(need);
}

extern "C" int vc_irans_decode_host(const uint8_t *data, size_t nbytes, const vc_irans_segment *segs, int n_segs,
                                    const vc_irans_tables *sets, int n_sets, int waves)
{
    if (!data || !irl::waves_ok(waves) || !segments_ok(segs, n_segs, n_sets)) return VC_EINVAL;
    std::vector<PackedSet> packed;
    if (const int rc = pack_sets(sets, n_sets, packed)) return rc;
    if (nbytes % 4) return VC_EDATA;
    const WordsAt word{data};
    uint32_t base[VC_IRANS_MAX_WAVES], count[VC_IRANS_MAX_WAVES], cursor[VC_IRANS_MAX_WAVES] = {};
    if (!irl::walk_headers(word, nbytes / 4, waves, 0, base, count)) return VC_EDATA;
    const size_t lanes = static_cast<size_t>(irl::kLanes) * waves;
    std::vector<uint64_t> x(lanes);
    for (size_t g = 0; g < lanes; ++g) {
        const uint64_t at = base[g / irl::kLanes] - irl::kHeaderWords + 1 + 2 * (g % irl::kLanes);
        x[g] = static_cast<uint64_t>(word(at)) | (static_cast<uint64_t>(word(at + 1)) << 32);
    }
    std::vector<uint8_t> escaped(lanes);
    std::vector<uint32_t> low(lanes);
    for (int s = 0; s < n_segs; ++s) {
        const vc_irans_segment &seg = segs[s];
        const PackedSet &set = packed[seg.table_set];
        const int n_tables = static_cast<int>(set.rows.size());
        const size_t rounds = seg.count / lanes + (seg.count % lanes != 0);
        for (size_t r = 0; r < rounds; ++r)
            for (int step = 0; step < 3; ++step)
                for (size_t g = 0; g < lanes; ++g) {
                    const size_t i = r * lanes + g;
                    if (i >= seg.count) continue;
                    if (step && !escaped[g]) continue;
                    const int32_t t = seg.indexes[i];
                    if (static_cast<uint32_t>(t) >= static_cast<uint32_t>(n_tables)) return VC_EINVAL;
                    const irl::Row &row = set.rows[t];
                    if (step == 0) {
                        const uint16_t *cdf = set.cdf16.data() + row.start;
                        const int slot = irl::lookup(cdf, row.size, row.mode, irl::cum_of(x[g]));
                        x[g] = irl::get(x[g], irl::slot_start(cdf, slot), irl::slot_freq(cdf, slot));
                        escaped[g] = slot == row.size - 2;
                        seg.symbols[i] = irl::symbol_of(slot, row.offset);
                    } else {
                        const uint32_t half = irl::cum_of(x[g]);
                        x[g] = irl::get(x[g], half, 1u);
                        if (step == 1) low[g] = half;
                        else seg.symbols[i] = irl::unzigzag(low[g] | (half << 16), row.offset);
                    }
                    if (irl::needs_word(x[g])) {
                        const int w = static_cast<int>(g / irl::kLanes);
                        if (cursor[w] >= count[w]) return VC_EDATA;
                        x[g] = irl::take_word(x[g], word(static_cast<uint64_t>(base[w]) + cursor[w]++));
                    }
                }
    }
    for (int w = 0; w < waves; ++w)
        if (cursor[w] != count[w]) return VC_EDATA;
    return VC_OK;
}

// ABI number: bumped whenever a struct of include/vc_hip.h changes size or layout (vc_conv_desc grew in rounds 4 and 5); the Python
// binding refuses a library whose number differs from the header it was written against
extern "C" int vc_abi_version(void) { return VC_ABI_VERSION; }
extern "C" const char *vc_version(void) { return "vc_hip 0.5 (abi 5)"; }
extern "C" const char *vc_target_arch(void) { return "gfx950"; }
