// Memory-safety fuzz of the interleaved range coder's host reference (csrc/rans_host.cpp: vc_irans_*, with the per-lane steps
// of csrc/rans_lanes.h that the kernels share), built by tests/test_irans_cpu.py with g++ -fsanitize=address,undefined.  Its
// own main: never loaded into python, never run on a GPU machine.  Deterministic (a 64-bit LCG): (1) encode -> decode round
// trips over random table sets, segment tables, wave counts and escapes of every magnitude, into exactly-sized buffers at
// odd addresses; (2) decodes of truncated payloads, of payloads with corrupted word counts, flipped bits and of plain
// garbage; (3) malformed tables, indexes, wave counts and segment tables.  Every call must return VC_OK or an error code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vc_hip.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

struct Set {
    int n_tables, stride;
    std::vector<int32_t> cdfs, sizes, offs;
    vc_irans_tables view() const { return {cdfs.data(), n_tables, stride, sizes.data(), offs.data()}; }
};

static Set random_set()
{
    Set s;
    s.n_tables = 1 + (int)(rnd() % 6);
    s.stride = 3 + (int)(rnd() % 200);
    s.cdfs.assign((size_t)s.n_tables * s.stride, 0);
    s.sizes.resize(s.n_tables);
    s.offs.resize(s.n_tables);
    for (int t = 0; t < s.n_tables; ++t) {
        const int n = 3 + (int)(rnd() % (s.stride - 2));
        const int slots = n - 1;
        std::vector<uint32_t> f(slots, 1);                     // every slot at least 1, the rest thrown at random slots in lumps
        uint32_t left = 65536u - (uint32_t)slots;
        while (left) {
            const uint32_t lump = 1 + rnd() % left;
            f[rnd() % slots] += lump;
            left -= lump;
        }
        int32_t c = 0;
        for (int i = 0; i < slots; ++i) { c += (int32_t)f[i]; s.cdfs[(size_t)t * s.stride + i + 1] = c; }
        s.sizes[t] = n;
        const int32_t extremes[] = {0, -(n / 2), INT32_MAX, INT32_MIN, 1 << 30};
        s.offs[t] = extremes[rnd() % 5];
    }
    return s;
}

static int32_t random_symbol(const Set &s, int t)
{
    switch (rnd() % 8) {
    case 0: return (int32_t)(rnd() * 2u + (rnd() & 1u));                         // anything
    case 1: { const int32_t e[] = {INT32_MIN, INT32_MIN + 1, INT32_MAX, 1 << 30, -(1 << 30), 0}; return e[rnd() % 6]; }
    default: return (int32_t)((uint32_t)s.offs[t] + rnd() % (uint32_t)(s.sizes[t] - 1));   // in the table (or just the escape boundary)
    }
}

int main()
{
    long cases = 0, refused = 0;
    for (int round = 0; round < 400; ++round) {
        const int n_sets = 1 + (int)(rnd() % 3);
        std::vector<Set> sets;
        std::vector<vc_irans_tables> views;
        for (int k = 0; k < n_sets; ++k) sets.push_back(random_set());
        for (const Set &s : sets) views.push_back(s.view());
        const int waves = 1 << (rnd() % 5);
        const int n_segs = (int)(rnd() % 5);
        std::vector<std::vector<int32_t>> sym(n_segs), idx(n_segs), got(n_segs);
        std::vector<vc_irans_segment> enc(n_segs), dec(n_segs);
        size_t cap = vc_irans_bound(0, waves);
        for (int k = 0; k < n_segs; ++k) {
            const size_t edges[] = {0, 1, 63, 64, 65, (size_t)64 * waves - 1, (size_t)64 * waves + 1, 1 + rnd() % 3000};
            const size_t count = edges[rnd() % 8];
            const int which = (int)(rnd() % n_sets);
            sym[k].resize(count);
            idx[k].resize(count);
            got[k].assign(count, 0);
            for (size_t i = 0; i < count; ++i) {
                idx[k][i] = (int32_t)(rnd() % sets[which].n_tables);
                sym[k][i] = random_symbol(sets[which], idx[k][i]);
            }
            enc[k] = {sym[k].data(), idx[k].data(), count, which};
            dec[k] = {got[k].data(), idx[k].data(), count, which};
            cap += vc_irans_bound(count, waves);
        }
        std::vector<uint8_t> buf(cap + 1);
        uint8_t *out = buf.data() + 1;                          // odd address: nothing may assume alignment
        const long long n = vc_irans_encode_host(enc.data(), n_segs, views.data(), n_sets, waves, out, cap);
        if (n < 0) { std::printf("round %d: encode failed (%lld)\n", round, n); return 2; }
        if (vc_irans_encode_host(enc.data(), n_segs, views.data(), n_sets, waves, out, (size_t)n - 1) != VC_ENOMEM) { std::puts("short buffer accepted"); return 3; }
        std::vector<uint8_t> exact(out, out + n);               // exactly sized: any read past the end is a sanitizer report
        if (vc_irans_decode_host(exact.data(), exact.size(), dec.data(), n_segs, views.data(), n_sets, waves) != VC_OK) { std::printf("round %d: decode failed\n", round); return 4; }
        for (int k = 0; k < n_segs; ++k)
            if (got[k] != sym[k]) { std::printf("round %d: segment %d differs\n", round, k); return 5; }
        ++cases;
        for (int attempt = 0; attempt < 24; ++attempt) {        // corrupted payloads: an error code or some symbols, never a report
            std::vector<uint8_t> bad(exact);
            switch (attempt % 6) {
            case 0: bad.resize(rnd() % (bad.size() + 1)); break;
            case 1: bad.resize(bad.size() / 4 * 4 > 4 ? (rnd() % (bad.size() / 4)) * 4 : 0); break;
            case 2: { const uint32_t c = rnd(); std::memcpy(bad.data(), &c, 4); break; }
            case 3: for (int f = 1 + (int)(rnd() % 6); f > 0; --f) bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() % 8)); break;
            case 4: for (auto &b : bad) b = (uint8_t)rnd(); break;
            default: bad.insert(bad.end(), 4 * (1 + rnd() % 4), (uint8_t)rnd()); break;
            }
            std::vector<uint8_t> tight(bad);                    // (a fresh allocation of exactly the corrupted length)
            const int rc = vc_irans_decode_host(tight.empty() ? (const uint8_t *)"" : tight.data(), tight.size(), dec.data(), n_segs,
                                                views.data(), n_sets, waves);
            if (rc != VC_OK && rc != VC_EDATA && rc != VC_EINVAL) { std::printf("unexpected code %d\n", rc); return 6; }
            refused += rc != VC_OK;
            ++cases;
        }
        if (n_segs) {                                           // indexes out of range, segment tables that point nowhere, bad wave counts
            const int k = (int)(rnd() % n_segs);
            if (!idx[k].empty()) {
                const size_t at = rnd() % idx[k].size();
                const int32_t keep = idx[k][at];
                const int32_t bads[] = {sets[enc[k].table_set].n_tables, -1, INT32_MAX, INT32_MIN};
                idx[k][at] = bads[rnd() % 4];
                if (vc_irans_encode_host(enc.data(), n_segs, views.data(), n_sets, waves, out, cap) != VC_EINVAL) { std::puts("bad index encoded"); return 7; }
                const int rc = vc_irans_decode_host(exact.data(), exact.size(), dec.data(), n_segs, views.data(), n_sets, waves);
                if (rc == VC_OK) { std::puts("bad index decoded"); return 8; }
                idx[k][at] = keep;
                cases += 2;
            }
            enc[k].table_set = n_sets;
            if (vc_irans_encode_host(enc.data(), n_segs, views.data(), n_sets, waves, out, cap) != VC_EINVAL) { std::puts("bad table set accepted"); return 9; }
            enc[k].table_set = dec[k].table_set;
            const int bad_waves[] = {0, 3, 6, 17, 32, -4};
            for (int w : bad_waves)
                if (vc_irans_encode_host(enc.data(), n_segs, views.data(), n_sets, w, out, cap) != VC_EINVAL ||
                    vc_irans_decode_host(exact.data(), exact.size(), dec.data(), n_segs, views.data(), n_sets, w) != VC_EINVAL || vc_irans_bound(10, w) != 0) {
                    std::puts("bad wave count accepted");
                    return 10;
                }
            cases += 7;
        }
        {   // malformed tables: not starting at 0, not ending at 65536, a flat step, a size beyond the row
            Set s = sets[0];
            const int t = (int)(rnd() % s.n_tables);
            switch (rnd() % 4) {
            case 0: s.cdfs[(size_t)t * s.stride] = 1; break;
            case 1: s.cdfs[(size_t)t * s.stride + s.sizes[t] - 1] = 65535; break;
            case 2: s.cdfs[(size_t)t * s.stride + 1] = 0; break;
            default: s.sizes[t] = s.stride + 1; break;
            }
            const vc_irans_tables v = s.view();
            if (vc_irans_pack_tables(v.cdfs, v.n_tables, v.cdf_stride, v.cdf_sizes, v.offsets, nullptr, nullptr) != VC_EINVAL) { std::puts("bad table accepted"); return 11; }
            ++cases;
        }
    }
    std::printf("%ld cases (%ld corrupted payloads refused), no sanitizer report\n", cases, refused);
    return 0;
}
