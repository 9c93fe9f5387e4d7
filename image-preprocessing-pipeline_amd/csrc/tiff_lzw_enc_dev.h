// An encoder for one TIFF LZW strip, the mirror of tiff_lzw_dev.h and written like it: serial code over a context `Ctx` that supplies
// the strip's bytes, owns the dictionary and takes the codes, so that the same text is a plain host function (g++, no HIP) and the
// body of a wave on the device (tiff3d_lzw_enc.hip).
//
// The schedule is libtiff's LZWEncode as lzw_encode in tiff3d.hip restates it, code for code: Clear (256) first; codes of 9 to 12
// bits, most significant bit first; one table entry per emitted code (258..); the width grows when the next free code passes 511,
// 1023 or 2047; when the next free code reaches 4094 the code is followed by Clear at the old width and everything starts over;
// after the last code the next free code is counted once more (the decoder adds an entry there) and Clear or a wider EOI follows
// from it; then EOI (257) and zero bits up to a whole byte.  The stream of a strip is determined by its bytes alone, so every
// context gives the same bytes.
//
// What the core guarantees whatever the strip:
//   - ctx.byte(i) is asked for i = 0, 1, .. n - 1, each once and in that order; every iteration of the loop consumes one byte, so
//     the loop ends after n - 1 iterations;
//   - between two ctx.reset() calls ctx.find_or_add adds at most min(kEncEntries, n - 1) entries: a table of table_slots(n) slots
//     is never more than half full, so an open-addressing probe meets an empty slot and is bounded by the slot count;
//   - the codes leave through ctx.put(code, width) with 9 <= width <= 12 and code < 2^width; at most n + n / 3836 + 4 of them.
// Where the codes go, and that they stay inside the strip's slot, is the context's part (EncBits below: it counts on and stops storing).
//
// The context:
//   uint32_t byte(uint32_t i)                            byte i of the strip
//   void reset()                                         the dictionary becomes empty
//   uint32_t find_or_add(uint32_t key, uint32_t code)    the code stored under key = prefix << 8 | byte, or kEncNone after storing `code` there
//   void put(uint32_t code, uint32_t width)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MI_LZWE_HD __host__ __device__ __forceinline__
#else
#define MI_LZWE_HD inline
#endif

namespace mi_lzw_enc {

enum EncStatus : int32_t {
    kEncOk = 0,
    kEncOverflow = 1,   // the stream is longer than the strip's slot: what fits is stored, the length is the whole stream's
    kEncStatusCount = 2
};

constexpr uint32_t kEncClear = 256, kEncEoi = 257, kEncFirst = 258, kEncFull = 4094;
constexpr uint32_t kEncEntries = kEncFull - kEncFirst;   // 3836 entries between two Clears
constexpr uint32_t kEncNone = 0xffffffffu;
// a table slot: key (20 bits) << 12 | code (12 bits); no key is 0xfffff (a prefix is at most 4093)
constexpr uint32_t kEncEmpty = 0xffffffffu;

// the slot of a strip of n bytes that always suffices (the host writer's bound)
MI_LZWE_HD uint64_t slot_bound(uint64_t n) { return n * 3u / 2u + 16u; }

// slots of the open-addressing table of a strip of n bytes: a power of two, at least twice the entries it can hold (64 at least: the
// device probes 64 slots at a time)
MI_LZWE_HD uint32_t table_slots(uint32_t n) {
    const uint32_t e = n < kEncEntries ? n : kEncEntries;
    uint32_t s = 64;
    while (s < 2u * e) s <<= 1;
    return s;
}

MI_LZWE_HD uint32_t table_hash(uint32_t key, uint32_t slots) { return ((key * 2654435761u) >> 12) & (slots - 1u); }

template <class Ctx>
MI_LZWE_HD void lzw_encode_strip(Ctx& ctx, uint32_t n) {
    uint32_t nbits = 9, maxcode = 511, free_ent = kEncFirst;
    ctx.reset();
    ctx.put(kEncClear, nbits);
    if (n == 0) {
        ctx.put(kEncEoi, nbits);
        return;
    }
    uint32_t ent = ctx.byte(0);
    for (uint32_t i = 1; i < n; ++i) {
        const uint32_t c = ctx.byte(i);
        const uint32_t found = ctx.find_or_add(ent << 8 | c, free_ent);
        if (found != kEncNone) {
            ent = found;
            continue;
        }
        ctx.put(ent, nbits);
        ent = c;
        free_ent += 1;
        if (free_ent == kEncFull) {
            ctx.reset();
            free_ent = kEncFirst;
            ctx.put(kEncClear, nbits);
            nbits = 9;
            maxcode = 511;
        } else if (free_ent > maxcode) {
            nbits += 1;
            maxcode = (1u << nbits) - 1u;
        }
    }
    ctx.put(ent, nbits);
    free_ent += 1;   // the decoder adds an entry after the last code and may widen before it reads EOI
    if (free_ent == kEncFull) {
        ctx.put(kEncClear, nbits);
        nbits = 9;
    } else if (free_ent > maxcode) {
        nbits += 1;
    }
    ctx.put(kEncEoi, nbits);
}

// the bit writer of a host call: bytes [0, cap) of out are stored, the rest is counted
struct EncBits {
    unsigned char* out;
    uint64_t cap, n = 0;
    uint64_t acc = 0;
    uint32_t bits = 0;
    inline void put(uint32_t code, uint32_t width) {
        acc = (acc << width) | code;
        bits += width;
        while (bits >= 8) {
            bits -= 8;
            if (n < cap) out[n] = (unsigned char)(acc >> bits);
            n += 1;
        }
    }
    inline void flush() {
        if (bits > 0) {
            if (n < cap) out[n] = (unsigned char)(acc << (8 - bits));
            n += 1;
            bits = 0;
        }
    }
};

// the context of a host call: one thread does everything; `table` has `slots` = table_slots(n) words
struct HostEncCtx {
    const unsigned char* src;
    uint32_t* table;
    uint32_t slots;
    EncBits bw;
    inline uint32_t byte(uint32_t i) const { return src[i]; }
    inline void reset() {
        for (uint32_t k = 0; k < slots; ++k) table[k] = kEncEmpty;
    }
    inline uint32_t find_or_add(uint32_t key, uint32_t code) {
        uint32_t h = table_hash(key, slots);
        for (uint32_t k = 0; k < slots; ++k) {   // (bounded by the slot count; half the slots are empty)
            const uint32_t e = table[h];
            if (e == kEncEmpty) {
                table[h] = key << 12 | code;
                return kEncNone;
            }
            if (e >> 12 == key) return e & 0xfffu;
            h = (h + 1u) & (slots - 1u);
        }
        return kEncNone;
    }
    inline void put(uint32_t code, uint32_t width) { bw.put(code, width); }
};

// src[0, n) -> dst[0, cap) on the calling thread with a table of table_slots(n) words; *len is the stream's length whether it fit or not
inline int lzw_encode_host(const unsigned char* src, uint32_t n, uint32_t* table, unsigned char* dst, uint64_t cap, uint64_t* len) {
    HostEncCtx ctx{src, table, table_slots(n), EncBits{dst, cap}};
    lzw_encode_strip(ctx, n);
    ctx.bw.flush();
    *len = ctx.bw.n;
    return ctx.bw.n > cap ? kEncOverflow : kEncOk;
}

}  // namespace mi_lzw_enc
