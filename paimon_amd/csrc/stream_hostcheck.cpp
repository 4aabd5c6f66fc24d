// Stand-alone host check of the stream walkers in stream_core.h, meant to be
// built with -fsanitize=address,undefined (make hostcheck): Parquet hybrid
// RLE (def levels, dictionary ids), DELTA_BINARY_PACKED, ORC RLEv2, byte-RLE
// and PRESENT over well-formed, truncated and malformed streams held in
// exactly-sized heap blocks (so one byte read past a stream is an ASan
// report). The streams come from the small builders below; the chunks the
// walkers emit are decoded by a bit-by-bit reference written apart from the
// core. No GPU, no HIP.
#include "stream_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

using namespace pmh;
typedef std::vector<uint8_t> Bytes;

static int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__,         \
                    __LINE__, #cond);                                      \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// an exactly-sized heap copy of a stream
struct Heap {
    uint8_t *p;
    int64_t n;
    explicit Heap(const Bytes &b) : n((int64_t)b.size()) {
        p = (uint8_t *)malloc(b.size() ? b.size() : 1);
        if (!b.empty()) memcpy(p, b.data(), b.size());
    }
    ~Heap() { free(p); }
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static uint64_t low_bits(uint64_t v, int w) {
    return w >= 64 ? v : v & ((1ull << w) - 1);
}

// ------------------------------------------------------------ builders

static void put_uleb(Bytes &s, uint64_t v) {
    while (v >= 0x80) {
        s.push_back((uint8_t)(v | 0x80));
        v >>= 7;
    }
    s.push_back((uint8_t)v);
}
static uint64_t zz(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }

// bit packers: append `w` bits of v at bit position *bit of s
static void put_lsb(Bytes &s, int64_t *bit, uint64_t v, int w) {
    for (int b = 0; b < w; b++, (*bit)++) {
        if ((size_t)(*bit >> 3) >= s.size()) s.push_back(0);
        s[(size_t)(*bit >> 3)] |= (uint8_t)(((v >> b) & 1) << (*bit & 7));
    }
}
static void put_msb(Bytes &s, int64_t *bit, uint64_t v, int w) {
    for (int b = w - 1; b >= 0; b--, (*bit)++) {
        if ((size_t)(*bit >> 3) >= s.size()) s.push_back(0);
        s[(size_t)(*bit >> 3)] |= (uint8_t)(((v >> b) & 1) << (7 - (*bit & 7)));
    }
}

// hybrid RLE: a run, and whole 8-value groups (zero padded)
static void hy_run(Bytes &s, int bw, uint64_t count, uint32_t v) {
    put_uleb(s, count << 1);
    for (int i = 0; i < (bw + 7) / 8; i++) s.push_back((uint8_t)(v >> (8 * i)));
}
static void hy_packed(Bytes &s, int bw, const std::vector<uint32_t> &vals) {
    const size_t groups = (vals.size() + 7) / 8;
    put_uleb(s, (groups << 1) | 1);
    Bytes body(groups * bw, 0);
    int64_t bit = 0;
    for (uint32_t v : vals) put_lsb(body, &bit, v, bw);
    s.insert(s.end(), body.begin(), body.end());
}

// ---------------------------------------------- bit-by-bit references

static uint64_t get_lsb(const uint8_t *s, int64_t bit, int w) {
    uint64_t v = 0;
    for (int b = 0; b < w; b++, bit++)
        v |= (uint64_t)((s[bit >> 3] >> (bit & 7)) & 1) << b;
    return v;
}
static uint64_t get_msb(const uint8_t *s, int64_t bit, int w) {
    uint64_t v = 0;
    for (int b = 0; b < w; b++, bit++)
        v = (v << 1) | ((s[bit >> 3] >> (7 - (bit & 7))) & 1);
    return v;
}

// RleChunk: kind 0 repeats value, kind 1 = LSB-first groups of bit_width at
// image + src
static void ref_rle(const std::vector<RleChunk> &ch, const uint8_t *image,
                    std::vector<uint32_t> &out) {
    for (const RleChunk &c : ch)
        for (int32_t i = 0; i < c.count; i++) {
            if ((size_t)(c.out_start + i) >= out.size()) {
                CHECK(!"chunk writes past the values");
                return;
            }
            out[(size_t)(c.out_start + i)] =
                c.kind == 0 ? c.value
                            : (uint32_t)get_lsb(image + c.src,
                                                (int64_t)i * c.bit_width,
                                                c.bit_width);
        }
}

// Rlev2Chunk kinds 0..5 (payloads MSB-first); values as 64-bit patterns
static void ref_rlev2(const std::vector<Rlev2Chunk> &ch, const uint8_t *s,
                      std::vector<uint64_t> &out) {
    for (const Rlev2Chunk &c : ch) {
        std::vector<uint64_t> v((size_t)c.count);
        const int w = c.width;
        if (c.kind == 0 || c.kind == 4) {
            for (auto &x : v) x = (uint64_t)c.base;
        } else if (c.kind == 1) {
            for (int i = 0; i < c.count; i++) {
                const uint64_t raw = get_msb(s + c.src, (int64_t)i * w, w);
                v[i] = c.is_signed ? (raw >> 1) ^ (0 - (raw & 1)) : raw;
            }
        } else if (c.kind == 2) {
            for (int i = 0; i < c.count; i++)
                v[i] = get_msb(s + c.src, (int64_t)i * w, w);
            int64_t at = 0;
            for (int i = 0; i < c.patch_pl; i++) {
                const uint64_t e = get_msb(s + c.patch_src,
                                           (int64_t)i * c.patch_cfb,
                                           c.patch_cfb);
                at += (int64_t)(e >> c.patch_pw);
                CHECK(at < c.count);
                if (at < c.count)
                    v[at] |= low_bits(e, c.patch_pw) << w;
            }
            for (auto &x : v) x += (uint64_t)c.base;
        } else if (c.kind == 3) {
            uint64_t cur = (uint64_t)c.base;
            for (int i = 0; i < c.count; i++) {
                if (i == 1 || (i > 1 && w == 0)) cur += (uint64_t)c.delta;
                if (i > 1 && w > 0) {
                    const uint64_t d =
                        get_msb(s + c.src, (int64_t)(i - 2) * w, w);
                    cur = c.delta < 0 ? cur - d : cur + d;
                }
                v[i] = cur;
            }
        } else {
            for (int i = 0; i < c.count; i++)
                v[i] = (uint64_t)(int64_t)(int8_t)s[c.src + i];
        }
        for (int i = 0; i < c.count; i++)
            if ((size_t)(c.out_start + i) < out.size())
                out[(size_t)(c.out_start + i)] = v[i];
    }
}

// DeltaStream + DeltaChunks: first value, then per block min_delta + the
// LSB-first miniblock bits at the widths packed in `widths`
static void ref_delta(const std::vector<DeltaChunk> &ch,
                      const std::vector<DeltaStream> &st, const uint8_t *s,
                      std::vector<int64_t> &out) {
    for (const DeltaStream &d : st) {
        uint64_t cur = (uint64_t)d.first;
        out[(size_t)d.out0] = (int64_t)cur;
        for (int64_t k = d.chunk_lo; k < d.chunk_hi; k++) {
            const DeltaChunk &c = ch[(size_t)k];
            for (int32_t i = 0; i < c.count; i++) {
                const int mini = i / c.vpm;
                int64_t bit = 0;
                for (int m = 0; m < mini; m++)
                    bit += (int64_t)c.vpm * ((c.widths >> (8 * m)) & 0xFF);
                const int w = (int)((c.widths >> (8 * mini)) & 0xFF);
                bit += (int64_t)(i % c.vpm) * w;
                cur += (uint64_t)c.min_delta + get_lsb(s + c.src, bit, w);
                out[(size_t)(c.out_start + i)] = (int64_t)cur;
            }
        }
    }
}

// --------------------------------------------------------- hybrid RLE

// def levels of `bits` through prescan_def and def_levels_have_nulls
static void check_def_stream(const Bytes &s, const std::vector<uint32_t> &bits,
                             int64_t n) {
    Heap h(s);
    std::vector<RleChunk> ch;
    const char *why = "";
    int64_t dense = 5;  // a cursor already under way
    CHECK(prescan_def(h.p, h.n, n, 0, 0, &dense, ch, &why));
    std::vector<uint32_t> out((size_t)n, 9);
    ref_rle(ch, h.p, out);
    int64_t ones = 0;
    size_t k = 0;
    bool nulls = false;
    for (int64_t i = 0; i < n; i++) {
        if (k < ch.size() && ch[k].out_start == i) {
            CHECK(ch[k].aux == 5 + ones && ch[k].count <= 512);
            k++;
        }
        CHECK(out[(size_t)i] == bits[(size_t)i]);
        ones += bits[(size_t)i];
        nulls |= bits[(size_t)i] == 0;
    }
    CHECK(k == ch.size() && dense == 5 + ones);
    CHECK(def_levels_have_nulls(h.p, h.n, n) == nulls);
}

static void check_hybrid() {
    for (int64_t n : {1, 7, 8, 9, 511, 512, 513, 1025}) {
        std::vector<uint32_t> bits((size_t)n + 16);
        for (auto &b : bits) b = rnd() % 3 != 0;
        Bytes s;
        // all packed: n ends inside an 8-value group
        hy_packed(s, 1, std::vector<uint32_t>(bits.begin(), bits.begin() + n));
        check_def_stream(s, bits, n);
        // one run longer than n: n ends inside the run
        for (uint32_t v : {0u, 1u}) {
            s.clear();
            hy_run(s, 1, (uint64_t)n + 5, v);
            check_def_stream(s, std::vector<uint32_t>((size_t)n, v), n);
        }
        // mixed: run, two groups, a long run, the rest packed
        std::vector<uint32_t> mix;
        s.clear();
        hy_run(s, 1, 3, 1);
        mix.insert(mix.end(), 3, 1);
        hy_packed(s, 1, std::vector<uint32_t>(bits.begin(), bits.begin() + 16));
        mix.insert(mix.end(), bits.begin(), bits.begin() + 16);
        hy_run(s, 1, 600, 0);
        mix.insert(mix.end(), 600, 0);
        hy_packed(s, 1, bits);
        mix.insert(mix.end(), bits.begin(), bits.end());
        check_def_stream(s, mix, n);
    }
    // def_levels_have_nulls at the edge of the wanted values
    {
        std::vector<uint32_t> ones(16, 1);
        Bytes s;
        hy_packed(s, 1, ones);
        CHECK(!def_levels_have_nulls(Heap(s).p, (int64_t)s.size(), 13));
        ones[12] = 0;  // the last wanted value
        s.clear();
        hy_packed(s, 1, ones);
        CHECK(def_levels_have_nulls(Heap(s).p, (int64_t)s.size(), 13));
        CHECK(!def_levels_have_nulls(Heap(s).p, (int64_t)s.size(), 12));
        ones[12] = 1;
        ones[13] = 0;  // padding beyond n
        s.clear();
        hy_packed(s, 1, ones);
        CHECK(!def_levels_have_nulls(Heap(s).p, (int64_t)s.size(), 13));
        CHECK(def_levels_have_nulls(Heap(s).p, (int64_t)s.size(), 17));
    }
    // dictionary ids. Bit width 0 is real: the width is a byte of the page
    // (stage_page_ids passes it on as read) and a one-entry dictionary is
    // written at width 0.
    for (int bw : {0, 1, 7, 8, 9, 24, 32})
        for (int64_t n : {16383, 16384, 16385}) {
            std::vector<uint32_t> vals((size_t)n + 8);
            for (auto &v : vals) v = (uint32_t)low_bits(rnd(), bw);
            for (int shape = 0; shape < 3; shape++) {
                Bytes s;
                std::vector<uint32_t> want;
                if (shape == 0) {  // all packed, n inside the last group
                    want.assign(vals.begin(), vals.begin() + n);
                    hy_packed(s, bw, want);
                } else if (shape == 1) {  // one run, n inside it
                    want.assign((size_t)n, vals[0]);
                    hy_run(s, bw, (uint64_t)n + 3, vals[0]);
                } else {  // run, three groups, a run cut by n
                    hy_run(s, bw, 5, vals[1]);
                    want.assign(5, vals[1]);
                    hy_packed(s, bw, std::vector<uint32_t>(vals.begin(),
                                                           vals.begin() + 24));
                    want.insert(want.end(), vals.begin(), vals.begin() + 24);
                    hy_run(s, bw, 20000, vals[2]);
                    want.resize((size_t)n, vals[2]);
                }
                Heap h(s);
                std::vector<RleChunk> ch;
                const char *why = "";
                CHECK(prescan_rle(h.p, h.n, bw, n, 0, 0, 0, ch, &why));
                std::vector<uint32_t> out((size_t)n, 0xDEAD);
                ref_rle(ch, h.p, out);
                CHECK(out == want);
                for (const RleChunk &c : ch) CHECK(c.count <= 16384);
            }
        }
}

// ------------------------------------------------- DELTA_BINARY_PACKED

// A page of `total` values, bs values per block in mpb miniblocks, every
// miniblock at width w (min_delta random); miniblocks without values get a
// width byte (7: it must not count) and no data.
static Bytes build_delta(int64_t total, int bs, int mpb, int w,
                         std::vector<int64_t> &vals) {
    Bytes s;
    put_uleb(s, (uint64_t)bs);
    put_uleb(s, (uint64_t)mpb);
    put_uleb(s, (uint64_t)total);
    uint64_t cur = rnd();
    put_uleb(s, zz((int64_t)cur));
    vals.assign(1, (int64_t)cur);
    const int vpm = bs / mpb;
    for (int64_t left = total - 1; left > 0; left -= bs) {
        const int64_t mind = (int64_t)rnd() >> 20;
        put_uleb(s, zz(mind));
        for (int m = 0; m < mpb; m++)
            s.push_back((uint8_t)(left - (int64_t)m * vpm > 0 ? w : 7));
        for (int m = 0; m < mpb && left - (int64_t)m * vpm > 0; m++) {
            Bytes body((size_t)(vpm * w + 7) / 8, 0);
            int64_t bit = 0;
            for (int j = 0; j < vpm; j++) {
                // the widest and the narrowest delta both occur
                const uint64_t d = j == 0 ? low_bits(~0ull, w)
                                          : j == 1 ? 0 : low_bits(rnd(), w);
                put_lsb(body, &bit, d, w);
                if ((int64_t)m * vpm + j < left) {
                    cur += (uint64_t)mind + d;
                    vals.push_back((int64_t)cur);
                }
            }
            s.insert(s.end(), body.begin(), body.end());
        }
    }
    return s;
}

static void check_delta() {
    const int bs = 128, mpb = 4;
    for (int64_t total : {1, 2, bs, bs + 1, 2 * bs + 3})
        for (int w : {0, 1, 31, 32, 33, 64}) {
            std::vector<int64_t> want, got;
            const Bytes s = build_delta(total, bs, mpb, w, want);
            Heap h(s);
            const char *why = "";
            CHECK(host_delta_i64(h.p, h.n, got, &why) == h.n);
            CHECK(got == want);
            std::vector<DeltaChunk> ch;
            std::vector<DeltaStream> st;
            CHECK(prescan_delta(h.p, h.n, total, 3, 0, 0, 0, 8, ch, st, &why));
            CHECK(st.size() == 1 && (int64_t)ch.size() == (total - 1 + bs - 1) / bs);
            std::vector<int64_t> out((size_t)total + 3, 0);
            ref_delta(ch, st, h.p, out);
            for (int64_t i = 0; i < total; i++)
                CHECK(out[(size_t)i + 3] == want[(size_t)i]);
            // a last block whose trailing miniblocks hold no values
            if (total == 2 * bs + 3)
                CHECK(ch.back().count == 2 &&
                      ch.back().widths == (uint64_t)w);
        }
}

// ------------------------------------------------------------ ORC RLEv2

static const int FBS[32] = {1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11,
                            12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22,
                            23, 24, 26, 28, 30, 32, 40, 48, 56, 64};
static int width_code(int w) {
    for (int i = 0; i < 32; i++)
        if (FBS[i] == w) return i;
    CHECK(!"not an RLEv2 width");
    return 0;
}
static uint64_t wire(uint64_t v, bool sgn) { return sgn ? zz((int64_t)v) : v; }

struct Rlev2Builder {
    Bytes s;
    std::vector<uint64_t> vals;  // decoded values, as 64-bit patterns
    bool sgn;
    void head(int kind, int code, int count) {
        s.push_back((uint8_t)(kind << 6 | code << 1 | (count - 1) >> 8));
        s.push_back((uint8_t)(count - 1));
    }
    void pack(const std::vector<uint64_t> &v, int w) {
        Bytes body;
        int64_t bit = 0;
        for (uint64_t x : v) put_msb(body, &bit, x, w);
        s.insert(s.end(), body.begin(), body.end());
    }
    void short_repeat(uint64_t v, int nbytes, int count) {
        s.push_back((uint8_t)((nbytes - 1) << 3 | (count - 3)));
        const uint64_t raw = wire(v, sgn);
        for (int i = nbytes - 1; i >= 0; i--) s.push_back((uint8_t)(raw >> (8 * i)));
        vals.insert(vals.end(), (size_t)count, v);
    }
    void direct(int w, int count) {
        head(1, width_code(w), count);
        std::vector<uint64_t> raw;
        for (int i = 0; i < count; i++) {
            raw.push_back(low_bits(rnd(), w));
            vals.push_back(sgn ? (raw.back() >> 1) ^ (0 - (raw.back() & 1))
                               : raw.back());
        }
        pack(raw, w);
    }
    // patches at positions `at` (ascending); a gap above 255 takes an
    // extension entry (gap 255, patch 0)
    void patched_base(int64_t base, int w, int pw, int count,
                      const std::vector<int> &at) {
        const int pgw = 8, bw = 3;
        std::vector<uint64_t> red, entries;
        for (int i = 0; i < count; i++) red.push_back(low_bits(rnd(), w));
        std::vector<uint64_t> full = red;
        int prev = 0;
        for (int pos : at) {
            int gap = pos - prev;
            for (; gap > 255; gap -= 255) entries.push_back(255ull << pw);
            const uint64_t patch = low_bits(rnd(), pw) | 1;
            entries.push_back((uint64_t)gap << pw | patch);
            full[(size_t)pos] |= patch << w;
            prev = pos;
        }
        head(2, width_code(w), count);
        s.push_back((uint8_t)((bw - 1) << 5 | width_code(pw)));
        s.push_back((uint8_t)((pgw - 1) << 5 | entries.size()));
        const uint64_t mag = (uint64_t)(base < 0 ? -base : base) |
                             (base < 0 ? 1ull << (bw * 8 - 1) : 0);
        for (int i = bw - 1; i >= 0; i--) s.push_back((uint8_t)(mag >> (8 * i)));
        pack(red, w);
        pack(entries, rlev2_closest_fixed_bits(pw + pgw));
        for (uint64_t x : full) vals.push_back((uint64_t)base + x);
    }
    // w == 0: fixed delta; else |delta0| then packed magnitudes
    void delta(uint64_t base, int64_t d0, int w, int count) {
        head(3, w ? width_code(w) : 0, count);
        put_uleb(s, wire(base, sgn));
        put_uleb(s, zz(d0));
        uint64_t cur = base;
        vals.push_back(cur);
        std::vector<uint64_t> mags;
        for (int i = 1; i < count; i++) {
            uint64_t d = (uint64_t)d0;
            if (i > 1 && w) {
                mags.push_back(low_bits(rnd(), w));
                d = d0 < 0 ? 0 - mags.back() : mags.back();
            }
            cur += d;
            vals.push_back(cur);
        }
        pack(mags, w);
    }
};

static void check_rlev2() {
    for (bool sgn : {false, true}) {
        Rlev2Builder b;
        b.sgn = sgn;
        b.short_repeat(sgn ? (uint64_t)-77 : 77, 1, 3);
        b.short_repeat(0x0123456789ABCDull, 8, 10);
        for (int count : {1, 2, 3, 512})
            for (int w : {1, 3, 8, 13, 24, 32, 40, 64}) b.direct(w, count);
        b.patched_base(-1000, 5, 12, 3, {1});
        b.patched_base(70000, 9, 3, 512, {2, 300, 301, 511});  // 298: extension
        for (int count : {1, 2, 3, 512}) {
            b.delta(sgn ? (uint64_t)-5 : 5, 3, 0, count);
            b.delta(1000000, -7, 0, count);
            b.delta(12, 4, 11, count);
            b.delta(1ull << 40, -9, 17, count);
        }
        Heap h(b.s);
        const int64_t n = (int64_t)b.vals.size();
        const char *why = "";
        std::vector<Rlev2Chunk> ch;
        CHECK(prescan_rlev2(h.p, h.n, n, sgn, 8, 0, 0, 0, ch, &why));
        std::vector<uint64_t> out((size_t)n, 0xDEAD), host;
        ref_rlev2(ch, h.p, out);
        CHECK(out == b.vals);
        CHECK(host_rlev2(h.p, h.n, n, sgn, host, &why) && host == b.vals);
        // n = -1: until the stream is exhausted
        CHECK(host_rlev2(h.p, h.n, -1, sgn, host, &why) && host == b.vals);
        // n inside the last run: the run still decodes whole
        CHECK(host_rlev2(h.p, h.n, n - 100, sgn, host, &why) &&
              host == b.vals);
    }
}

// ------------------------------------------------ byte-RLE and PRESENT

static void br_run(Bytes &s, Bytes &bytes, int k, uint8_t v) {
    s.push_back((uint8_t)(k - 3));
    s.push_back(v);
    bytes.insert(bytes.end(), (size_t)k, v);
}
static void br_lit(Bytes &s, Bytes &bytes, int k, int seed) {
    s.push_back((uint8_t)(256 - k));
    for (int i = 0; i < k; i++) {
        s.push_back((uint8_t)(seed + i * 37));
        bytes.push_back((uint8_t)(seed + i * 37));
    }
}

static void check_byterle() {
    Bytes s, bytes;
    br_run(s, bytes, 3, 0xB1);
    br_lit(s, bytes, 1, 200);
    br_run(s, bytes, 130, 0x00);
    br_lit(s, bytes, 128, 9);
    br_run(s, bytes, 130, 0xFF);
    br_lit(s, bytes, 2, 0x5A);
    br_run(s, bytes, 5, 0x0F);
    Heap h(s);
    const int64_t total = (int64_t)bytes.size();
    // tinyint values: n whole, inside the last run, inside the last literal
    for (int64_t n : {total, total - 2, total - 6, (int64_t)1}) {
        std::vector<Rlev2Chunk> ch;
        const char *why = "";
        CHECK(prescan_byterle(h.p, h.n, n, 1, 0, 0, 0, ch, &why));
        std::vector<uint64_t> out((size_t)n, 0xDEAD);
        ref_rlev2(ch, h.p, out);
        for (int64_t i = 0; i < n; i++)
            CHECK(out[(size_t)i] == (uint64_t)(int64_t)(int8_t)bytes[(size_t)i]);
        CHECK(ch.back().out_start + ch.back().count == n);
    }
    // PRESENT: the same bytes as MSB-first bits; n cut inside the last byte,
    // inside the last literal, inside the 0xFF run
    for (int64_t n : {total * 8, total * 8 - 3, total * 8 - 5 * 8 - 9,
                      (int64_t)(3 + 1 + 130 + 128 + 7) * 8 + 1, (int64_t)1}) {
        Bytes levels(3, 0xEE);  // the column's buffer already holds levels
        std::vector<RleChunk> ch;
        int64_t dense = 11;
        const char *why = "";
        CHECK(prescan_present(h.p, h.n, n, 0, levels, ch, &dense, &why));
        std::vector<uint32_t> out((size_t)n, 9);
        ref_rle(ch, levels.data(), out);
        int64_t ones = 0;
        size_t k = 0;
        for (int64_t i = 0; i < n; i++) {
            if (k < ch.size() && ch[k].out_start == i)
                CHECK(ch[k++].aux == 11 + ones);
            const uint32_t bit = (bytes[(size_t)(i >> 3)] >> (7 - (i & 7))) & 1;
            CHECK(out[(size_t)i] == bit);
            ones += bit;
        }
        CHECK(k == ch.size() && dense == 11 + ones);
    }
}

// ----------------------------------------------------------- refusals

// every proper prefix of s must be refused with a reason
static void refuse_cuts(const Bytes &s,
                        const std::function<bool(const uint8_t *, int64_t,
                                                 const char **)> &walk) {
    const char *why = "";
    CHECK(walk(Heap(s).p, (int64_t)s.size(), &why));
    for (size_t cut = 0; cut < s.size(); cut++) {
        Heap h(Bytes(s.begin(), s.begin() + cut));
        why = "";
        CHECK(!walk(h.p, h.n, &why));
        CHECK(why[0] != 0);
    }
}
static void refuse(const Bytes &s,
                   const std::function<bool(const uint8_t *, int64_t,
                                            const char **)> &walk) {
    Heap h(s);
    const char *why = "";
    CHECK(!walk(h.p, h.n, &why));
    CHECK(why[0] != 0);
}

static void check_refusals() {
    std::vector<RleChunk> rc;
    std::vector<Rlev2Chunk> vc;
    std::vector<DeltaChunk> dc;
    std::vector<DeltaStream> ds;
    std::vector<int64_t> iv;
    std::vector<uint64_t> uv;
    Bytes lv;
    int64_t dense = 0;
    auto def = [&](int64_t n) {
        return [&, n](const uint8_t *p, int64_t len, const char **why) {
            const bool ok = prescan_def(p, len, n, 0, 0, &dense, rc, why);
            // the null check answers true on whatever prescan_def refuses
            if (!ok) CHECK(def_levels_have_nulls(p, len, n));
            return ok;
        };
    };
    auto rle = [&](int bw, int64_t n) {
        return [&, bw, n](const uint8_t *p, int64_t len, const char **why) {
            return prescan_rle(p, len, bw, n, 0, 0, 0, rc, why);
        };
    };
    auto delta = [&](int64_t n) {
        return [&, n](const uint8_t *p, int64_t len, const char **why) {
            const bool host = host_delta_i64(p, len, iv, why) >= 0;
            const bool dev = prescan_delta(p, len, n, 0, 0, 0, 0, 8, dc, ds, why);
            CHECK(host || !dev);  // the prescan is the stricter one
            return dev;
        };
    };
    auto host_delta = [&](const uint8_t *p, int64_t len, const char **why) {
        return host_delta_i64(p, len, iv, why) >= 0;
    };
    auto rlev2 = [&](int64_t n) {
        return [&, n](const uint8_t *p, int64_t len, const char **why) {
            const bool dev = prescan_rlev2(p, len, n, 1, 8, 0, 0, 0, vc, why);
            CHECK(host_rlev2(p, len, n, true, uv, why) == dev);
            return dev;
        };
    };
    auto byterle = [&](int64_t n) {
        return [&, n](const uint8_t *p, int64_t len, const char **why) {
            return prescan_byterle(p, len, n, 1, 0, 0, 0, vc, why);
        };
    };
    auto present = [&](int64_t n) {
        return [&, n](const uint8_t *p, int64_t len, const char **why) {
            return prescan_present(p, len, n, 0, lv, rc, &dense, why);
        };
    };

    // every truncation point of a short stream of each kind
    Bytes s;
    hy_run(s, 1, 200, 1);
    hy_packed(s, 1, std::vector<uint32_t>(24, 1));
    hy_run(s, 1, 3, 1);
    refuse_cuts(s, def(227));
    s.clear();
    hy_run(s, 12, 9, 0xABC);
    hy_packed(s, 12, std::vector<uint32_t>(16, 0x123));
    refuse_cuts(s, rle(12, 25));
    std::vector<int64_t> want;
    refuse_cuts(build_delta(131, 128, 4, 9, want), delta(131));
    refuse_cuts(build_delta(131, 128, 4, 9, want), host_delta);
    Rlev2Builder b;
    b.sgn = true;
    b.short_repeat(5, 2, 4);
    b.direct(13, 5);
    b.patched_base(-9, 7, 10, 20, {3, 17});
    b.delta(100, 2, 0, 4);
    b.delta(100, -2, 6, 9);
    refuse_cuts(b.s, rlev2((int64_t)b.vals.size()));
    Bytes bytes;
    s.clear();
    br_run(s, bytes, 4, 0x81);
    br_lit(s, bytes, 3, 1);
    br_run(s, bytes, 3, 0xFF);
    refuse_cuts(s, byterle(10));
    refuse_cuts(s, present(80));

    // varints: 10 bytes reach bit 63 and no further
    {
        Bytes v(9, 0x80);
        v.push_back(0x01);
        int64_t p = 0;
        uint64_t x = 0;
        CHECK(uleb64(Heap(v).p, 10, &p, &x) && x == 1ull << 63 && p == 10);
        v[9] = 0x02;  // bit 64
        p = 0;
        CHECK(!uleb64(Heap(v).p, 10, &p, &x));
        v[9] = 0x80;  // an 11th byte
        v.push_back(0x00);
        p = 0;
        CHECK(!uleb64(Heap(v).p, 11, &p, &x));
        refuse(v, def(1));
        refuse(v, rle(8, 1));
        refuse(v, host_delta);
        CHECK(unzigzag(zz(INT64_MIN)) == INT64_MIN && unzigzag(1) == -1);
    }
    // hybrid RLE: a lone continuation byte; more groups than bytes; a run
    // without its value; a width the run value cannot hold
    refuse({0x80}, def(1));
    refuse({0x80}, rle(8, 1));
    refuse({0x05, 0xFF}, def(16));
    refuse({0x05, 0xFF, 0xFF, 0xFF}, rle(3, 16));
    refuse({0x10}, def(8));
    refuse({0x10, 0x01}, rle(9, 8));
    refuse({0x10, 1, 2, 3, 4, 5}, rle(33, 8));
    // a last group its writer cut short is taken while the wanted values
    // are there
    {
        Heap h(Bytes{0x05, 0xFF});
        const char *why = "";
        rc.clear();
        CHECK(prescan_def(h.p, h.n, 8, 0, 0, &dense, rc, &why));
        CHECK(rc.size() == 1 && rc[0].count == 8);
    }
    // delta: mpb = 0; bs % mpb != 0; width 65; the count disagreeing; more
    // miniblocks than the kernel takes (host decode only)
    refuse({128, 1, 0, 5, 2}, delta(5));
    refuse({128, 1, 0, 5, 2}, host_delta);
    refuse({130, 1, 4, 5, 2}, host_delta);
    {
        Bytes d = build_delta(10, 128, 4, 3, want);
        refuse(d, delta(11));
        const size_t widths = d.size() - 12 - 4;  // one stored miniblock
        CHECK(d[widths] == 3);
        d[widths] = 65;
        refuse(d, delta(10));
        refuse(d, host_delta);
        d = build_delta(10, 128, 16, 3, want);
        refuse(d, delta(10));
        const char *why = "";
        CHECK(host_delta_i64(Heap(d).p, (int64_t)d.size(), iv, &why) ==
              (int64_t)d.size() && iv == want);
    }
    // RLEv2: a patch entry of pw + pgw = 64 + 1 bits
    refuse({0x80 | 2 << 1, 2, 31, 0 << 5 | 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
            0, 0, 0, 0},
           rlev2(3));
    // PRESENT: a run without its byte; a literal short of its bytes, even
    // where the rows wanted end before the gap
    refuse({0x00}, present(8));
    refuse({0xFE, 0xAA}, present(16));
    refuse({0xFE, 0xAA}, present(8));
    refuse({0xFE, 0xAA}, byterle(2));
}

int main() {
    check_hybrid();
    check_delta();
    check_rlev2();
    check_byterle();
    check_refusals();
    if (failures) {
        fprintf(stderr, "stream_hostcheck: %d failure(s)\n", failures);
        return 1;
    }
    printf("stream_hostcheck OK\n");
    return 0;
}
