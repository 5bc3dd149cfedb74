// Device side of the interleaved range coder (include/vc_hip.h: "Interleaved range coder"; format and measurements in DESIGN.md
// section 4d).  One wave = one workgroup = one sub-stream: the 64 lanes hold the 64 states, run the per-lane steps of
// rans_lanes.h (the very functions the host reference loops over) in lockstep, and share the sub-stream's words through a
// ballot + prefix count -- the lanes that renormalise in a step take / leave consecutive words in ascending lane order.
//
// Decoder: one launch per segment, states and cursors in a vc_irans_dstate between launches.  A round's reads depend on one
// another (state -> cumulative value -> table search -> state), so the tables are staged in LDS whenever the set fits the 64 KiB
// a workgroup gets without opting in (the 64 Gaussian tables are 54 KiB as u16), and the search gallops out from the row's
// mode.  It cannot fault or hang on any payload: loops are counted by the segment's symbol count, words are read only below
// the sub-stream's count (checked against the uploaded length by vc_irans_decode_begin), the search stays inside the row;
// a violation sets the wave's error word (and the image's sticky one, for the host): the wave decodes zeros from there on, every
// wave of the image from the next launch on -- a wave looks at its siblings' words only as earlier launches left them, so the
// zeros do not depend on which wave runs first.  The fused forms (vc_irans_decode_eb / vc_irans_decode_gc: the LHBDC stream codec,
// DESIGN.md section 4e; vc_irans_decode_gc_ckbd: one checkerboard parity of the ELIC intra codec, section 4g) run the same round
// loop, take the table index from the channel / the scale and write the de-quantised latent; behind a violation they write the
// de-quantisation of 0.  vc_irans_tables_in_lds describes all four: the Gaussian forms
// keep their scale table (64 floats) behind the cdf rows and, for the sets between 64 KiB - 256 bytes and 64 KiB, asks for the
// 256 bytes past 64 KiB by opting in, so the boundary between the staged and the global form does not move.
//
// Encoder: one launch per payload, walking segments, rounds and sub-steps backwards; tables read from global memory and a
// plain 64-by-32-bit division per step (not on any critical path: the encoder waits for the networks, not they for it).
#include "common.h"
#include "rans_lanes.h"
#include "entropy_shared.h"

namespace {
constexpr int kLdsTableBytes = 64 * 1024;
constexpr int kScaleSlots = 64;                // floats of LDS the fused Gaussian form keeps its scale table in

struct EncArgs {
    vc_irans_dsegment segs[VC_IRANS_MAX_SEGMENTS];
    vc_irans_dtables sets[VC_IRANS_MAX_TABLE_SETS];
    int n_segs, waves;
    uint32_t cap;            // words a wave's region holds behind its header
    uint32_t *out, *counts;
};

__device__ __forceinline__ uint32_t rank_below(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }
__device__ __forceinline__ irl::Row row_of(const vc_irans_dtables &t, int index) { return *reinterpret_cast<const irl::Row *>(t.rows + 4 * index); }

__global__ __launch_bounds__(64) void irans_encode_kernel(const EncArgs a)
{
    const int lane = threadIdx.x, image = blockIdx.x / a.waves, wave = blockIdx.x % a.waves;
    uint32_t *region = a.out + static_cast<size_t>(blockIdx.x) * (irl::kHeaderWords + a.cap);
    uint32_t *words = region + irl::kHeaderWords;
    const uint32_t lanes = irl::kLanes * a.waves;
    uint32_t p = a.cap;                        // words[p ..] are written; uniform
    uint64_t x = irl::kLow;
    bool bad = false;                          // an index out of range (lane) / the capacity exhausted (uniform)
    for (int s = a.n_segs - 1; s >= 0; --s) {
        const vc_irans_dsegment seg = a.segs[s];
        const vc_irans_dtables set = a.sets[seg.table_set];
        const int32_t *sym = seg.symbols + static_cast<size_t>(image) * seg.count;
        const int32_t *idx = seg.indexes + static_cast<size_t>(image) * seg.count;
        const uint32_t rounds = seg.count / lanes + (seg.count % lanes != 0);
        for (uint32_t r = rounds; r-- > 0;) {
            const uint32_t i = r * lanes + wave * irl::kLanes + lane;
            bool active = i < seg.count, escaped = false;
            irl::Row row = {0, 3, 0, 0};
            int slot = 0;
            uint32_t zz = 0;
            if (active) {
                const int32_t t = idx[i];
                if (static_cast<uint32_t>(t) >= static_cast<uint32_t>(set.n_tables)) {
                    bad = true;
                    active = false;
                } else {
                    row = row_of(set, t);
                    const int32_t v = sym[i];
                    slot = irl::slot_of(v, row, escaped);
                    zz = irl::zigzag(v, row.offset);
                }
            }
            const uint16_t *cdf = set.cdf16 + row.start;
            for (int step = __ballot(escaped) ? 2 : 0; step >= 0; --step) {
                const bool on = active && (step == 0 || escaped);
                uint32_t start = 0, freq = 1;
                if (on) {
                    start = step == 2 ? zz >> 16 : step == 1 ? (zz & 0xffffu) : irl::slot_start(cdf, slot);
                    if (step == 0) freq = irl::slot_freq(cdf, slot);
                }
                const bool emits = on && irl::put_emits(x, freq);
                const unsigned long long mask = __ballot(emits);
                const uint32_t k = __popcll(mask);
                if (k > p) {
                    bad = true;                // cannot happen with the capacity the host entry point insists on; never write below the region
                } else if (k) {
                    if (emits) words[p - k + rank_below(mask, lane)] = static_cast<uint32_t>(x);
                    p -= k;
                }
                if (emits) x >>= 32;
                if (on) x = irl::put(x, start, freq);
            }
        }
    }
    const uint32_t count = a.cap - p;
    uint32_t *sub = region + p;                // count | states | words[p ..]
    sub[1 + 2 * lane] = static_cast<uint32_t>(x);
    sub[2 + 2 * lane] = static_cast<uint32_t>(x >> 32);
    const bool failed = __ballot(bad) != 0;
    if (lane == 0) {
        sub[0] = count;
        a.counts[blockIdx.x] = failed ? 0xffffffffu : count;
    }
}

struct PayloadWords {
    const uint32_t *p;
    __device__ uint32_t operator()(uint64_t i) const { return p[i]; }
};

__global__ __launch_bounds__(64) void irans_begin_kernel(const uint32_t *payloads, uint64_t payload_words, const uint32_t *where, int waves,
                                                         vc_irans_dstate *states)
{
    __shared__ uint32_t base[VC_IRANS_MAX_WAVES], count[VC_IRANS_MAX_WAVES], ok_s;
    const int lane = threadIdx.x, image = blockIdx.x;
    vc_irans_dstate *st = states + image;
    if (lane == 0) {
        const uint64_t off = where[2 * image], bytes = where[2 * image + 1];
        bool ok = bytes % 4 == 0 && off <= payload_words && bytes / 4 <= payload_words - off;
        ok = ok && irl::walk_headers(PayloadWords{payloads + off}, bytes / 4, waves, off, base, count);
        ok_s = ok;
        st->error = ok ? 0u : VC_IRANS_ERR_HEADER;
        st->waves = static_cast<uint32_t>(waves);
    }
    __syncthreads();
    const bool ok = ok_s != 0;
    if (lane < VC_IRANS_MAX_WAVES) {
        const bool used = ok && lane < waves;
        st->base[lane] = used ? base[lane] : 0u;
        st->count[lane] = used ? count[lane] : 0u;
        st->cursor[lane] = 0u;
        st->wave_error[lane] = ok ? 0u : VC_IRANS_ERR_HEADER;      // launch stamp 0: seen by every launch
        st->launches[lane] = 0u;
    }
    for (int w = 0; w < waves; ++w) {
        uint64_t x = irl::kLow;
        if (ok) {
            const uint32_t *s = payloads + base[w] - irl::kHeaderWords + 1 + 2 * lane;
            x = static_cast<uint64_t>(s[0]) | (static_cast<uint64_t>(s[1]) << 32);
        }
        st->x[w][lane] = x;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Decoder.  ONE round loop (irans_decode_segment) for the four entry points; what differs between them is where a symbol's table
// index comes from and where the decoded integer goes -- an `Io`:
//     Item fetch(image, i)                 everything symbol i needs that does NOT depend on the coder state: its table index and
//                                          whatever the store wants later (a median, a mean, the position)
//     void store(image, i, item, symbol)   the decoded integer (0 behind a violation) to its destination
// PlainIo: index tensor in, integer tensor out (vc_irans_decode).  EbIo: the index is the channel i / (h w), the store writes
// z_hat as vc_eb_dequant would (vc_irans_decode_eb).  GcIo: the index is scale_index of the NHWC scale, the store writes y_hat as
// vc_gc_dequant would (vc_irans_decode_gc); GcCkbdIo: the same struct at one checkerboard parity, symbol i being an element of the
// squeezed order (vc_irans_decode_gc_ckbd); all through the expressions of entropy_shared.h that entropy.hip itself uses.
// fetch() for round r + 1 is issued before the state chain of round r (state -> cumulative value -> search -> state -> words), so
// its loads (and the 63 compares of scale_index) are in flight while that chain is waited on.
// ------------------------------------------------------------------------------------------------------------------------------
struct PlainIo {
    struct Item { int32_t index; };
    const int32_t *indexes;
    int32_t *out;
    uint32_t count;
    __device__ __forceinline__ Item fetch(int image, uint32_t i) const { return {indexes[static_cast<size_t>(image) * count + i]}; }
    __device__ __forceinline__ void store(int image, uint32_t i, const Item &, int32_t symbol) const
    {
        out[static_cast<size_t>(image) * count + i] = symbol;
    }
};

// symbol i of an image = element (c, y, x) of its NCHW raster
struct Raster {
    uint32_t hw, w;
    __device__ __forceinline__ void split(uint32_t i, int &c, int &y, int &x) const
    {
        const uint32_t cc = i / hw, rem = i - cc * hw, yy = rem / w;
        c = static_cast<int>(cc);
        y = static_cast<int>(yy);
        x = static_cast<int>(rem - yy * w);
    }
};

struct EbIo {
    struct Item { int32_t index; float med; int y, x; };
    Raster ras;
    const float *params, *out_gain;
    vc_view zh;
    int32_t *symbols;                          // nullable: dense [images][count]
    uint32_t count;
    __device__ __forceinline__ Item fetch(int, uint32_t i) const
    {
        Item it;
        ras.split(i, it.index, it.y, it.x);    // the table of a hyper-latent is its channel's
        it.med = params[static_cast<long long>(it.index) * VC_EB_PARAMS_PER_CHANNEL + 58];
        return it;
    }
    __device__ __forceinline__ void store(int image, uint32_t i, const Item &it, int32_t symbol) const
    {
        zh.p[view_off(zh, image, it.y, it.x) + it.index] = vc_eb_dequant_value(symbol, it.med, out_gain, it.index);
        if (symbols) symbols[static_cast<size_t>(image) * count + i] = symbol;
    }
};

// kCkbd = false: symbol i = element (c, y, x) of the NCHW raster of the views.  kCkbd = true: one checkerboard parity of them -- symbol
// i = element (c, y, xs) of the squeezed order [c][h][w/2] that vc_gc_forward_ckbd writes (`ras` describes that order), at
// full-resolution column ckbd_column(xs, y, parity); the other parity is neither read nor written.
template <bool kCkbd>
struct GcIoT {
    struct Item { int32_t index; float mean; int c, y, x; };
    Raster ras;
    vc_view sc, mu, yh;
    const float *table;                        // the scale table, staged in LDS by the kernel
    int n_scales;
    const float *out_gain;
    int32_t *symbols;                          // nullable: dense [images][count], in symbol order
    uint32_t count;
    int parity;                                // kCkbd only
    __device__ __forceinline__ Item fetch(int image, uint32_t i) const
    {
        Item it;
        ras.split(i, it.c, it.y, it.x);
        if (kCkbd) it.x = ckbd_column(it.x, it.y, parity);
        it.index = scale_index(vc_lower_bound_scale(sc.p[view_off(sc, image, it.y, it.x) + it.c]), table, n_scales);
        it.mean = mu.p[view_off(mu, image, it.y, it.x) + it.c];
        return it;
    }
    __device__ __forceinline__ void store(int image, uint32_t i, const Item &it, int32_t symbol) const
    {
        yh.p[view_off(yh, image, it.y, it.x) + it.c] = vc_gc_dequant_value(symbol, it.mean, out_gain, it.c);
        if (symbols) symbols[static_cast<size_t>(image) * count + i] = symbol;
    }
};
using GcIo = GcIoT<false>;
using GcCkbdIo = GcIoT<true>;

// One segment of one (image, wave): `staged` = the workgroup's LDS for the cdf rows (kLds) -- whatever else a kernel keeps in LDS it
// has written AND synchronised before it calls this.
template <bool kLds, class Io>
__device__ __forceinline__ void irans_decode_segment(const uint32_t *payloads, vc_irans_dstate *states, int waves, uint32_t count,
                                                     const vc_irans_dtables &tab, uint16_t *staged, const Io &io)
{
    const int lane = threadIdx.x, image = blockIdx.x / waves, wave = blockIdx.x % waves;
    const uint16_t *cdf16 = tab.cdf16;
    if (kLds) {                                // entries is a multiple of 8: whole 16-byte chunks
        const vc_u32x4 *src = reinterpret_cast<const vc_u32x4 *>(tab.cdf16);
        vc_u32x4 *dst = reinterpret_cast<vc_u32x4 *>(staged);
        for (int i = lane; i < tab.entries / 8; i += irl::kLanes) dst[i] = src[i];
        __syncthreads();
        cdf16 = staged;
    }
    vc_irans_dstate *st = states + image;
    uint64_t x = st->x[wave][lane];
    uint32_t cursor = st->cursor[wave];
    const uint32_t have = st->count[wave];
    const uint32_t *words = payloads + st->base[wave];
    const uint32_t launch = st->launches[wave];                    // written by this wave alone
    bool dead = false;                         // uniform: a wave of the image met a violation in an EARLIER launch
    for (int w = 0; w < waves; ++w) {
        const uint32_t e = st->wave_error[w];
        dead |= e != 0 && (e >> 3) <= launch;
    }
    uint32_t err = 0;
    const uint32_t lanes = irl::kLanes * waves;
    const uint32_t rounds = count / lanes + (count % lanes != 0);

    // the lanes of `on` whose state fell below 2^31 take the next words in ascending lane order; false = past the sub-stream's end
    auto refill = [&](bool on) -> bool {
        const bool need = on && irl::needs_word(x);
        const unsigned long long mask = __ballot(need);
        if (!mask) return true;
        const uint32_t k = __popcll(mask);
        if (k > have - cursor) return false;   // (cursor <= have always)
        if (need) x = irl::take_word(x, words[cursor + rank_below(mask, lane)]);
        cursor += k;
        return true;
    };

    uint32_t i = wave * irl::kLanes + lane;    // (count < 2^31, lanes <= 1024: i + lanes cannot wrap)
    typename Io::Item next = {};
    if (i < count) next = io.fetch(image, i);
    for (uint32_t r = 0; r < rounds; ++r, i += lanes) {
        const bool active = i < count;
        const typename Io::Item cur = next;
        if (i + lanes < count) next = io.fetch(image, i + lanes);  // round r + 1: nothing in it depends on x
        int32_t symbol = 0;
        if (!dead) {
            bool escaped = false, bad_index = false;
            irl::Row row = {0, 3, 0, 0};
            if (active) {
                const int32_t t = cur.index;
                bad_index = static_cast<uint32_t>(t) >= static_cast<uint32_t>(tab.n_tables);
                if (!bad_index) {
                    row = row_of(tab, t);
                    const uint16_t *cdf = cdf16 + row.start;
                    const int slot = irl::lookup(cdf, row.size, row.mode, irl::cum_of(x));
                    x = irl::get(x, irl::slot_start(cdf, slot), irl::slot_freq(cdf, slot));
                    escaped = slot == row.size - 2;
                    symbol = irl::symbol_of(slot, row.offset);
                }
            }
            if (__ballot(bad_index)) {
                err |= VC_IRANS_ERR_INDEX;
                dead = true;
            } else if (!refill(active)) {
                err |= VC_IRANS_ERR_WORD;
                dead = true;
            } else if (__ballot(escaped)) {    // two masked sub-steps: the 16-bit halves of the escaped lanes' values
                uint32_t low = 0, high = 0;
                if (escaped) {
                    low = irl::cum_of(x);
                    x = irl::get(x, low, 1u);
                }
                bool fine = refill(escaped);
                if (fine) {
                    if (escaped) {
                        high = irl::cum_of(x);
                        x = irl::get(x, high, 1u);
                    }
                    fine = refill(escaped);
                }
                if (!fine) {
                    err |= VC_IRANS_ERR_WORD;
                    dead = true;
                } else if (escaped) {
                    symbol = irl::unzigzag(low | (high << 16), row.offset);
                }
            }
        }
        if (active) io.store(image, i, cur, dead ? 0 : symbol);
    }
    st->x[wave][lane] = x;
    if (lane == 0) {
        st->cursor[wave] = cursor;
        st->launches[wave] = launch + 1;
        if (err) {
            st->wave_error[wave] = ((launch + 1) << 3) | err;      // (err != 0 implies this wave was not dead: its word was 0)
            atomicOr(&st->error, err);
        }
    }
}

extern __shared__ __attribute__((aligned(16))) uint16_t irans_lds[];

template <bool kLds>
__global__ __launch_bounds__(64) void irans_decode_kernel(const uint32_t *payloads, vc_irans_dstate *states, int waves, const int32_t *indexes,
                                                          uint32_t count, const vc_irans_dtables tab, int32_t *out)
{
    irans_decode_segment<kLds>(payloads, states, waves, count, tab, irans_lds, PlainIo{indexes, out, count});
}

template <bool kLds>
__global__ __launch_bounds__(64) void irans_decode_eb_kernel(const uint32_t *payloads, vc_irans_dstate *states, int waves, uint32_t count,
                                                             const vc_irans_dtables tab, const EbIo io)
{
    irans_decode_segment<kLds>(payloads, states, waves, count, tab, irans_lds, io);
}

// LDS: the cdf rows (kLds; 2 * entries bytes, a multiple of 16), then the kScaleSlots floats of the scale table.  Io: GcIo / GcCkbdIo
template <bool kLds, class Io>
__global__ __launch_bounds__(64) void irans_decode_gc_kernel(const uint32_t *payloads, vc_irans_dstate *states, int waves, uint32_t count,
                                                             const vc_irans_dtables tab, Io io)
{
    float *table = reinterpret_cast<float *>(irans_lds + (kLds ? tab.entries : 0));
    if (static_cast<int>(threadIdx.x) < io.n_scales) table[threadIdx.x] = io.table[threadIdx.x];      // n_scales <= kScaleSlots = 64 lanes
    __syncthreads();
    io.table = table;
    irans_decode_segment<kLds>(payloads, states, waves, count, tab, irans_lds, io);
}

bool dtables_ok(const vc_irans_dtables &t)
{
    return t.cdf16 && t.rows && t.n_tables >= 1 && t.entries >= 8 && t.entries % 8 == 0 && reinterpret_cast<uintptr_t>(t.cdf16) % 16 == 0 &&
           reinterpret_cast<uintptr_t>(t.rows) % 16 == 0;
}
}  // namespace

extern "C" int vc_irans_tables_in_lds(int entries) { return entries > 0 && 2ll * entries <= kLdsTableBytes; }

extern "C" int vc_irans_encode(vc_stream s, const vc_irans_dsegment *segs, int n_segs, const vc_irans_dtables *sets, int n_sets, int images,
                               int waves, uint32_t *out, size_t wave_cap_words, uint32_t *counts)
{
    if (!segs || !sets || !out || !counts || n_segs < 1 || n_segs > VC_IRANS_MAX_SEGMENTS || n_sets < 1 || n_sets > VC_IRANS_MAX_TABLE_SETS ||
        images < 1 || !irl::waves_ok(waves) || images > (1 << 20))
        return VC_EINVAL;
    EncArgs a = {};
    size_t need = 0;
    for (int k = 0; k < n_sets; ++k) {
        if (!dtables_ok(sets[k])) return VC_EINVAL;
        a.sets[k] = sets[k];
    }
    for (int k = 0; k < n_segs; ++k) {
        if (segs[k].table_set < 0 || segs[k].table_set >= n_sets || segs[k].count > 0x7fffffffu) return VC_EINVAL;
        if (segs[k].count && (!segs[k].symbols || !segs[k].indexes)) return VC_EINVAL;
        a.segs[k] = segs[k];
        need += vc_irans_wave_words(segs[k].count, waves);
    }
    if (wave_cap_words < need || wave_cap_words > 0x7fffffffu) return VC_EINVAL;
    a.n_segs = n_segs;
    a.waves = waves;
    a.cap = static_cast<uint32_t>(wave_cap_words);
    a.out = out;
    a.counts = counts;
    hipLaunchKernelGGL(irans_encode_kernel, dim3(images * waves), dim3(irl::kLanes), 0, as_stream(s), a);
    VC_LAUNCH_CHECK();
    return VC_OK;
}

extern "C" int vc_irans_decode_begin(vc_stream s, const uint32_t *payloads, size_t payload_words, const uint32_t *where, int images, int waves,
                                     vc_irans_dstate *states)
{
    if (!payloads || !where || !states || images < 1 || images > (1 << 20) || !irl::waves_ok(waves) || payload_words > 0xffffffffull)
        return VC_EINVAL;
    hipLaunchKernelGGL(irans_begin_kernel, dim3(images), dim3(irl::kLanes), 0, as_stream(s), payloads, static_cast<uint64_t>(payload_words),
                       where, waves, states);
    VC_LAUNCH_CHECK();
    return VC_OK;
}

extern "C" int vc_irans_decode(vc_stream s, const uint32_t *payloads, vc_irans_dstate *states, int images, int waves, const int32_t *indexes,
                               size_t count, vc_irans_dtables tables, int32_t *symbols_out)
{
    if (!payloads || !states || images < 1 || images > (1 << 20) || !irl::waves_ok(waves) || count > 0x7fffffffu || !dtables_ok(tables))
        return VC_EINVAL;
    if (count == 0) return VC_OK;
    if (!indexes || !symbols_out) return VC_EINVAL;
    const dim3 grid(images * waves), block(irl::kLanes);
    if (vc_irans_tables_in_lds(tables.entries))
        hipLaunchKernelGGL(irans_decode_kernel<true>, grid, block, 2 * static_cast<size_t>(tables.entries), as_stream(s), payloads, states, waves,
                           indexes, static_cast<uint32_t>(count), tables, symbols_out);
    else
        hipLaunchKernelGGL(irans_decode_kernel<false>, grid, block, 0, as_stream(s), payloads, states, waves, indexes,
                           static_cast<uint32_t>(count), tables, symbols_out);
    VC_LAUNCH_CHECK();
    return VC_OK;
}

namespace {
bool fused_view_ok(const vc_view &v, int images) { return v.p && v.n == images && v.h >= 1 && v.w >= 1 && v.c >= 1; }
bool same_shape(const vc_view &a, const vc_view &b) { return a.n == b.n && a.h == b.h && a.w == b.w && a.c == b.c; }
// count == c * h * w, below 2^31
bool fused_count_ok(const vc_view &v, size_t count)
{
    const unsigned long long hw = static_cast<unsigned long long>(v.h) * static_cast<unsigned long long>(v.w);
    return hw <= 0x7fffffffull && hw * static_cast<unsigned long long>(v.c) <= 0x7fffffffull && count == hw * static_cast<unsigned long long>(v.c);
}
bool fused_common_ok(const uint32_t *payloads, const vc_irans_dstate *states, int images, int waves, const vc_irans_dtables &tables)
{
    return payloads && states && images >= 1 && images <= (1 << 20) && irl::waves_ok(waves) && dtables_ok(tables);
}
}  // namespace

extern "C" int vc_irans_decode_eb(vc_stream s, const uint32_t *payloads, vc_irans_dstate *states, int images, int waves, size_t count,
                                  vc_irans_dtables tables, const float *eb_params, const float *out_gain, vc_view z_hat, int32_t *symbols_out)
{
    if (!fused_common_ok(payloads, states, images, waves, tables) || !eb_params || !fused_view_ok(z_hat, images) || !fused_count_ok(z_hat, count))
        return VC_EINVAL;
    const EbIo io = {{static_cast<uint32_t>(z_hat.h) * static_cast<uint32_t>(z_hat.w), static_cast<uint32_t>(z_hat.w)}, eb_params, out_gain, z_hat,
                     symbols_out, static_cast<uint32_t>(count)};
    const dim3 grid(images * waves), block(irl::kLanes);
    if (vc_irans_tables_in_lds(tables.entries))
        hipLaunchKernelGGL(irans_decode_eb_kernel<true>, grid, block, 2 * static_cast<size_t>(tables.entries), as_stream(s), payloads, states,
                           waves, static_cast<uint32_t>(count), tables, io);
    else
        hipLaunchKernelGGL(irans_decode_eb_kernel<false>, grid, block, 0, as_stream(s), payloads, states, waves, static_cast<uint32_t>(count),
                           tables, io);
    VC_LAUNCH_CHECK();
    return VC_OK;
}

namespace {
// the launch of the two Gaussian forms: same grid, same LDS layout (one opt-in per instantiation)
template <class Io>
int launch_decode_gc(vc_stream s, const uint32_t *payloads, vc_irans_dstate *states, int images, int waves, size_t count,
                     const vc_irans_dtables &tables, const Io &io)
{
    const dim3 grid(images * waves), block(irl::kLanes);
    constexpr size_t table_bytes = kScaleSlots * sizeof(float);
    if (vc_irans_tables_in_lds(tables.entries)) {
        static vc_lds_raised raised;           // (only the sets within 256 bytes of 64 KiB get here past the default limit)
        const size_t lds = 2 * static_cast<size_t>(tables.entries) + table_bytes;
        if (!vc_raise_lds_limit(reinterpret_cast<const void *>(&irans_decode_gc_kernel<true, Io>), lds, raised)) return VC_ELAUNCH;
        hipLaunchKernelGGL((irans_decode_gc_kernel<true, Io>), grid, block, lds, as_stream(s), payloads, states, waves,
                           static_cast<uint32_t>(count), tables, io);
    } else {
        hipLaunchKernelGGL((irans_decode_gc_kernel<false, Io>), grid, block, table_bytes, as_stream(s), payloads, states, waves,
                           static_cast<uint32_t>(count), tables, io);
    }
    VC_LAUNCH_CHECK();
    return VC_OK;
}
}  // namespace

extern "C" int vc_irans_decode_gc(vc_stream s, const uint32_t *payloads, vc_irans_dstate *states, int images, int waves, size_t count,
                                  vc_irans_dtables tables, vc_view scales, vc_view means, const float *scale_table, int n_scales,
                                  const float *out_gain, vc_view y_hat, int32_t *symbols_out)
{
    if (!fused_common_ok(payloads, states, images, waves, tables) || !scale_table || n_scales < 2 || n_scales > kScaleSlots ||
        !fused_view_ok(y_hat, images) || !fused_view_ok(scales, images) || !fused_view_ok(means, images) || !same_shape(scales, y_hat) ||
        !same_shape(means, y_hat) || !fused_count_ok(y_hat, count))
        return VC_EINVAL;
    const GcIo io = {{static_cast<uint32_t>(y_hat.h) * static_cast<uint32_t>(y_hat.w), static_cast<uint32_t>(y_hat.w)}, scales, means, y_hat,
                     scale_table, n_scales, out_gain, symbols_out, static_cast<uint32_t>(count), 0};
    return launch_decode_gc(s, payloads, states, images, waves, count, tables, io);
}

extern "C" int vc_irans_decode_gc_ckbd(vc_stream s, const uint32_t *payloads, vc_irans_dstate *states, int images, int waves, size_t count,
                                       vc_irans_dtables tables, vc_view scales, vc_view means, int parity, const float *scale_table,
                                       int n_scales, const float *out_gain, vc_view y_hat, int32_t *symbols_out)
{
    if (!fused_common_ok(payloads, states, images, waves, tables) || !scale_table || n_scales < 2 || n_scales > kScaleSlots ||
        !fused_view_ok(y_hat, images) || !fused_view_ok(scales, images) || !fused_view_ok(means, images) || !same_shape(scales, y_hat) ||
        !same_shape(means, y_hat) || (parity != 0 && parity != 1) || (y_hat.w & 1))
        return VC_EINVAL;
    vc_view half = y_hat;                      // the squeezed order's shape: count == c * h * (w / 2)
    half.w = y_hat.w / 2;
    if (!fused_count_ok(half, count)) return VC_EINVAL;
    const GcCkbdIo io = {{static_cast<uint32_t>(half.h) * static_cast<uint32_t>(half.w), static_cast<uint32_t>(half.w)}, scales, means, y_hat,
                         scale_table, n_scales, out_gain, symbols_out, static_cast<uint32_t>(count), parity};
    return launch_decode_gc(s, payloads, states, images, waves, count, tables, io);
}
