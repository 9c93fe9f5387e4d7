// An inflater for one zlib stream (RFC 1950 / 1951), written so that the same text runs as a plain host function (g++, no HIP) and as
// the body of a wave on the device (tiff_inflate.hip): the core below is serial code over a context `Ctx` that supplies the input
// words, takes the output tokens and owns the tables.  On the host the context is a few loops (HostCtx at the end of this file); on
// the device every lane of the wave runs the core with the same values, and the context's hooks are where the 64 lanes do different
// things (staging, table fill, copies, Adler sums).
//
// What the core guarantees whatever the input (the device is shared; a stream is data from a file):
//   - the input is only asked for by word index through ctx.word(i); the context returns 0 beyond the stream's bytes, and the core
//     stops with kInfInput once more bits are consumed than the stream holds;
//   - ctx.literal / ctx.match are only called for bytes inside [0, out_n) and for sources inside [0, pos): the contexts need no checks;
//   - every loop iteration consumes at least one input bit or produces at least one output byte, both of which are bounded, so no
//     input makes the decoder run on.
//
// The context:
//   uint32_t word(uint32_t i)                 little-endian word i of the stream, bytes beyond its end read as 0
//   T uni(T v)                                v, marked as the same in every lane (readfirstlane on the device)
//   InfTables& tables()
//   void for_each(uint32_t n, F f)            f(i) for i < n, in any order, complete on return (table fill)
//   void literal(uint32_t pos, uint32_t b)    out[pos] = b
//   void match(uint32_t pos, uint32_t dist, uint32_t len)     out[pos + k] = out[pos - dist + k], k < len, in ascending order of k
//   uint32_t adler(uint32_t n)                Adler-32 of out[0, n) once every token is out
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MI_INF_HD __host__ __device__ __forceinline__
#else
#define MI_INF_HD inline
#endif

namespace mi_inflate {

// status of a stream: 0 or why it ended
enum InfStatus : int32_t {
    kInfOk = 0,
    kInfHeader = 1,          // zlib header: CM != 8, CINFO > 7, FCHECK, FDICT
    kInfBlockType = 2,       // BTYPE 3
    kInfStoredLen = 3,       // LEN != ~NLEN
    kInfCodeOver = 4,        // code set: over-subscribed
    kInfCodeIncomplete = 5,  // code set: incomplete (other than one code of one bit, or an unused distance code)
    kInfCodeNoEob = 6,       // code set: no end-of-block code
    kInfSymbol = 7,          // a bit pattern that is no code; symbols 286 / 287 / distance 30 / 31; a bad code-length repeat or count
    kInfDistance = 8,        // a match that begins before the first byte
    kInfInput = 9,           // the input ended early
    kInfOutput = 10,         // more or fewer bytes than expected
    kInfChecksum = 11,       // Adler-32
    kInfStatusCount = 12
};

MI_INF_HD const char* status_name(int s) {
    switch (s) {
        case kInfOk: return "ok";
        case kInfHeader: return "zlib header";
        case kInfBlockType: return "block type";
        case kInfStoredLen: return "stored length";
        case kInfCodeOver: return "over-subscribed code";
        case kInfCodeIncomplete: return "incomplete code";
        case kInfCodeNoEob: return "no end-of-block code";
        case kInfSymbol: return "invalid symbol";
        case kInfDistance: return "distance before the start";
        case kInfInput: return "input exhausted";
        case kInfOutput: return "output size";
        case kInfChecksum: return "checksum";
        default: return "unknown";
    }
}

constexpr int kLitFastBits = 10, kDistFastBits = 8;

// a canonical prefix code (RFC 1951 3.2.2): per length the number of codes, the first code and where its symbols begin in `sorted`
struct InfCode {
    uint16_t count[16], first[16], offs[16], next[16];
    uint32_t maxlen;
};

struct InfTables {
    uint8_t len[288 + 32];                        // code lengths as read: literal / length codes, then distance codes
    uint16_t lit_sorted[288], dist_sorted[32], cl_sorted[19];
    InfCode lit, dist, cl;
    uint16_t lit_fast[1 << kLitFastBits];         // [next bits] = symbol << 4 | length; 0: a longer code or none
    uint16_t dist_fast[1 << kDistFastBits];
};

// the low 15 bits of x in reverse order (the stream's first bit becomes the most significant)
MI_INF_HD uint32_t reverse15(uint32_t x) {
    uint32_t r = x & 0xffffu;
    r = ((r & 0x5555u) << 1) | ((r >> 1) & 0x5555u);
    r = ((r & 0x3333u) << 2) | ((r >> 2) & 0x3333u);
    r = ((r & 0x0f0fu) << 4) | ((r >> 4) & 0x0f0fu);
    r = ((r & 0x00ffu) << 8) | ((r >> 8) & 0x00ffu);
    return r >> 1;
}

// symbol << 4 | length of the code that begins rev15 (codes of at most `limit` bits), 0 when there is none
MI_INF_HD uint32_t canonical(const InfCode& c, const uint16_t* sorted, uint32_t rev15, uint32_t limit) {
    for (uint32_t l = 1; l <= limit; ++l) {
        const uint32_t idx = (rev15 >> (15 - l)) - (uint32_t)c.first[l];
        if (idx < (uint32_t)c.count[l]) return (uint32_t)sorted[c.offs[l] + idx] << 4 | l;
    }
    return 0;
}

// the code of len[0, n): its description and symbols; kInfCodeOver / kInfCodeIncomplete, or 0.  An incomplete code is taken when it
// is a single code of one bit (`one_ok`) or has no code at all (`none_ok`: a distance code that the block never uses)
// Serial code (as is the reading of the code lengths in inflate_zlib): it reads and rewrites the same table entries step by step
// (count[len[i]] + 1, next[l]).  On the device every lane of the one wave runs it with the same addresses and values -- a wave's
// lanes execute an instruction together and its LDS accesses complete in program order, so each step sees the step before; no
// lane reads here what only ANOTHER lane wrote.  That is not true of code run by several waves: a context whose work-group is
// wider than a wave must run these parts on one wave between barriers.
template <class Ctx>
MI_INF_HD int build_code(Ctx& ctx, const uint8_t* len, uint32_t n, InfCode& c, uint16_t* sorted, bool one_ok, bool none_ok) {
    for (uint32_t l = 0; l < 16; ++l) c.count[l] = 0;
    for (uint32_t i = 0; i < n; ++i) c.count[len[i]] = (uint16_t)(c.count[len[i]] + 1);
    c.count[0] = 0;
    int32_t left = 1;
    uint32_t code = 0, at = 0, maxlen = 0, used = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        const uint32_t k = ctx.uni((uint32_t)c.count[l]);
        left = (left << 1) - (int32_t)k;
        if (left < 0) return kInfCodeOver;
        code = (code + ctx.uni((uint32_t)c.count[l - 1])) << 1;   // (count[0] is 0)
        c.first[l] = (uint16_t)code;
        c.offs[l] = (uint16_t)at;
        c.next[l] = (uint16_t)at;
        at += k;
        used += k;
        if (k) maxlen = l;
    }
    c.maxlen = maxlen;
    if (left > 0) {
        const bool one = used == 1 && maxlen == 1;
        if (!((one && one_ok) || (used == 0 && none_ok))) return kInfCodeIncomplete;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = ctx.uni((uint32_t)len[i]);
        if (l) {
            const uint32_t p = ctx.uni((uint32_t)c.next[l]);
            sorted[p] = (uint16_t)i;
            c.next[l] = (uint16_t)(p + 1);
        }
    }
    return 0;
}

template <class Ctx>
MI_INF_HD void fill_fast(Ctx& ctx, const InfCode& c, const uint16_t* sorted, uint16_t* fast, uint32_t bits) {
    const uint32_t limit = c.maxlen < bits ? c.maxlen : bits;
    ctx.for_each(1u << bits, [&](uint32_t i) { fast[i] = (uint16_t)canonical(c, sorted, reverse15(i), limit); });
}

// the bit reader: at least 33 bits after fill()
template <class Ctx>
struct InfBits {
    uint64_t buf = 0;
    uint32_t n = 0, widx = 0;
    MI_INF_HD void fill(Ctx& ctx) {
        if (n <= 32) {
            buf |= (uint64_t)ctx.word(widx) << n;
            widx += 1;
            n += 32;
        }
    }
    MI_INF_HD uint32_t peek(uint32_t k) const { return (uint32_t)buf & ((1u << k) - 1u); }
    MI_INF_HD void drop(uint32_t k) {
        buf >>= k;
        n -= k;
    }
    MI_INF_HD uint32_t take(uint32_t k) {
        const uint32_t v = peek(k);
        drop(k);
        return v;
    }
    MI_INF_HD uint64_t consumed() const { return (uint64_t)widx * 32u - n; }
};

// symbol << 4 | length of the next code in the reader (not dropped), 0: none
template <class Ctx>
MI_INF_HD uint32_t next_code(Ctx& ctx, const InfBits<Ctx>& b, const InfCode& c, const uint16_t* sorted, const uint16_t* fast, uint32_t fast_bits) {
    uint32_t e = ctx.uni((uint32_t)fast[b.peek(fast_bits)]);
    if (e == 0 && c.maxlen > fast_bits) e = ctx.uni(canonical(c, sorted, reverse15(b.peek(15)), c.maxlen));
    return e;
}

// The status of a bit pattern that is no code of a code of at most `maxlen` bits: the walk over the code looked at maxlen bits; when
// all of them are bits of the stream the pattern is an invalid symbol, when zeros past the stream's end were among them the end
// came first.
MI_INF_HD int no_code(uint64_t consumed, uint32_t maxlen, uint64_t in_bits) { return consumed + maxlen > in_bits ? kInfInput : kInfSymbol; }

// One zlib stream of in_n bytes that must give exactly out_n bytes.  Bytes after the Adler-32 are ignored.
template <class Ctx>
MI_INF_HD int inflate_zlib(Ctx& ctx, uint32_t in_n, uint32_t out_n) {
    InfTables& t = ctx.tables();
    InfBits<Ctx> b;
    const uint64_t in_bits = (uint64_t)in_n * 8u;
    b.fill(ctx);
    const uint32_t cmf = b.take(8), flg = b.take(8);
    if (in_n < 2 || (cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8 | flg) % 31u) != 0u || (flg & 32u)) return kInfHeader;
    uint32_t pos = 0;
    for (uint32_t last = 0; !last;) {
        b.fill(ctx);
        last = b.take(1);
        const uint32_t type = b.take(2);
        if (b.consumed() > in_bits) return kInfInput;
        if (type == 3) return kInfBlockType;
        if (type == 0) {
            b.drop(b.n & 7u);   // to the byte boundary (the reader holds whole words, so its fill is the stream's position mod 8)
            b.fill(ctx);
            const uint32_t len = b.take(16);
            b.fill(ctx);
            const uint32_t nlen = b.take(16);
            if (b.consumed() > in_bits) return kInfInput;
            if ((len ^ 0xffffu) != nlen) return kInfStoredLen;
            if (len > out_n - pos) return kInfOutput;
            if (b.consumed() + (uint64_t)len * 8u > in_bits) return kInfInput;
            for (uint32_t k = 0; k < len; ++k) {
                b.fill(ctx);
                ctx.literal(pos, b.take(8));
                pos += 1;
            }
            continue;
        }
        if (type == 1) {
            for (uint32_t i = 0; i < 288; ++i) t.len[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
            for (uint32_t i = 0; i < 32; ++i) t.len[288 + i] = 5;
            (void)build_code(ctx, t.len, 288, t.lit, t.lit_sorted, false, false);
            (void)build_code(ctx, t.len + 288, 32, t.dist, t.dist_sorted, false, false);
        } else {
            b.fill(ctx);
            const uint32_t nlit = b.take(5) + 257, ndist = b.take(5) + 1, ncl = b.take(4) + 4;
            if (nlit > 286 || ndist > 30) return kInfSymbol;
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint8_t* cl_len = t.len + 288;   // (free until the distance lengths are moved there)
            for (uint32_t i = 0; i < 19; ++i) cl_len[i] = 0;
            for (uint32_t i = 0; i < ncl; ++i) {
                b.fill(ctx);
                cl_len[order[i]] = (uint8_t)b.take(3);
            }
            if (b.consumed() > in_bits) return kInfInput;
            const int rc = build_code(ctx, cl_len, 19, t.cl, t.cl_sorted, false, false);
            if (rc) return rc;
            // the nlit + ndist code lengths, in one sequence: runs may cross from the literal code into the distance code
            uint16_t* seq = t.lit_fast;   // (one length per entry; the table is filled after this)
            uint32_t have = 0, prev = 0;
            while (have < nlit + ndist) {
                b.fill(ctx);
                const uint32_t e = ctx.uni(canonical(t.cl, t.cl_sorted, reverse15(b.peek(15)), t.cl.maxlen));
                if (e == 0) return no_code(b.consumed(), t.cl.maxlen, in_bits);
                b.drop(e & 15u);
                const uint32_t sym = e >> 4;
                uint32_t rep = 1, val = sym;
                if (sym == 16) {
                    if (have == 0) return kInfSymbol;
                    val = prev;
                    rep = 3 + b.take(2);
                } else if (sym == 17) {
                    val = 0;
                    rep = 3 + b.take(3);
                } else if (sym == 18) {
                    val = 0;
                    rep = 11 + b.take(7);
                }
                if (b.consumed() > in_bits) return kInfInput;
                if (have + rep > nlit + ndist) return kInfSymbol;
                for (uint32_t k = 0; k < rep; ++k) seq[have + k] = (uint16_t)val;
                have += rep;
                prev = val;
            }
            for (uint32_t i = 0; i < 288; ++i) t.len[i] = i < nlit ? (uint8_t)seq[i] : (uint8_t)0;
            for (uint32_t i = 0; i < 32; ++i) t.len[288 + i] = i < ndist ? (uint8_t)seq[nlit + i] : (uint8_t)0;
            if (ctx.uni((uint32_t)t.len[256]) == 0) return kInfCodeNoEob;
            const int rl = build_code(ctx, t.len, 288, t.lit, t.lit_sorted, true, false);
            if (rl) return rl;
            const int rd = build_code(ctx, t.len + 288, 32, t.dist, t.dist_sorted, true, true);
            if (rd) return rd;
        }
        fill_fast(ctx, t.lit, t.lit_sorted, t.lit_fast, kLitFastBits);
        fill_fast(ctx, t.dist, t.dist_sorted, t.dist_fast, kDistFastBits);
        for (;;) {
            b.fill(ctx);
            const uint32_t e = next_code(ctx, b, t.lit, t.lit_sorted, t.lit_fast, kLitFastBits);
            if (e == 0) return no_code(b.consumed(), t.lit.maxlen, in_bits);
            b.drop(e & 15u);
            if (b.consumed() > in_bits) return kInfInput;
            const uint32_t sym = e >> 4;
            if (sym < 256) {
                if (pos >= out_n) return kInfOutput;
                ctx.literal(pos, sym);
                pos += 1;
                continue;
            }
            if (sym == 256) break;
            if (sym > 285) return kInfSymbol;
            uint32_t len;
            if (sym < 265) len = sym - 254;
            else if (sym == 285) len = 258;
            else {
                const uint32_t eb = (sym - 261) >> 2;
                len = 3 + ((4 + ((sym - 261) & 3u)) << eb) + b.take(eb);
            }
            b.fill(ctx);
            const uint32_t d = next_code(ctx, b, t.dist, t.dist_sorted, t.dist_fast, kDistFastBits);
            if (d == 0) return no_code(b.consumed(), t.dist.maxlen, in_bits);
            b.drop(d & 15u);
            const uint32_t dsym = d >> 4;
            if (dsym > 29) return kInfSymbol;
            uint32_t dist;
            if (dsym < 4) dist = dsym + 1;
            else {
                const uint32_t eb = (dsym >> 1) - 1;
                dist = 1 + ((2 + (dsym & 1u)) << eb) + b.take(eb);
            }
            if (b.consumed() > in_bits) return kInfInput;
            if (dist > pos) return kInfDistance;
            if (len > out_n - pos) return kInfOutput;
            ctx.match(pos, dist, len);
            pos += len;
        }
    }
    if (pos != out_n) return kInfOutput;
    b.drop(b.n & 7u);
    uint32_t want = 0;
    for (int k = 0; k < 4; ++k) {
        b.fill(ctx);
        want = want << 8 | b.take(8);
    }
    if (b.consumed() > in_bits) return kInfInput;
    if (ctx.adler(out_n) != want) return kInfChecksum;
    return kInfOk;
}

// the context of a host call: one thread does everything
struct HostCtx {
    const unsigned char* in;
    uint32_t in_n;
    unsigned char* out;
    InfTables t;
    inline uint32_t word(uint32_t i) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t at = (uint64_t)i * 4u + k;
            if (at < in_n) v |= (uint32_t)in[at] << (8 * k);
        }
        return v;
    }
    template <class T> inline T uni(T v) const { return v; }
    inline InfTables& tables() { return t; }
    template <class F> inline void for_each(uint32_t n, F f) const {
        for (uint32_t i = 0; i < n; ++i) f(i);
    }
    inline void literal(uint32_t pos, uint32_t b) { out[pos] = (unsigned char)b; }
    inline void match(uint32_t pos, uint32_t dist, uint32_t len) {
        for (uint32_t k = 0; k < len; ++k) out[pos + k] = out[pos - dist + k];
    }
    inline uint32_t adler(uint32_t n) const {
        uint32_t s1 = 1, s2 = 0;
        for (uint32_t i = 0; i < n; ++i) {
            s1 += out[i];
            if (s1 >= 65521u) s1 -= 65521u;
            s2 += s1;
            if (s2 >= 65521u) s2 -= 65521u;
        }
        return s2 << 16 | s1;
    }
};

// in[0, in_n) -> out[0, out_n) on the calling thread; an InfStatus
inline int inflate_host(const unsigned char* in, uint32_t in_n, unsigned char* out, uint32_t out_n) {
    HostCtx ctx{in, in_n, out, {}};
    return inflate_zlib(ctx, in_n, out_n);
}

}  // namespace mi_inflate
