// A decoder for one TIFF LZW strip (TIFF 6.0 section 13, as libtiff's tif_lzw.c reads it and as the encoder in tiff3d.hip writes
// it), written like tiff_inflate_dev.h: serial code over a context `Ctx` that supplies the input words, keeps the table and takes
// the output, so that the same text is a plain host function (g++, no HIP) and the body of a wave on the device (tiff3d_read.hip).
//
// The format: codes of 9 to 12 bits, most significant bit first; 256 is Clear, 257 is EOI (end of information), 258.. are table
// entries.  The width grows when the next free code reaches 511, 1023 or 2047 ("early change").  Entries go up to 4093 (the encoders
// send Clear before 4094 would be added).  A strip may begin with Clear or without it: decoding starts in the cleared state.  It ends
// when the strip's rows are full: EOI may be missing and whatever follows is not looked at.
//
// The table: every string of the dictionary is a piece of the output already produced -- the entry added while code c is handled is
// the string of the code before c plus the first byte of c's string, and those bytes lie where the code before c was emitted.  So an
// entry is (offset into the strip's output, length) and decoding a code is copy(pos, offset, length), the operation of a deflate
// match.  The code that names the entry being added (KwKwK) copies length = distance + 1 bytes and repeats its source.  No walk
// along a prefix chain and no reversal.
//
// What the core guarantees whatever the input (the device is shared; a strip is data from a file):
//   - the input is only asked for by word index through ctx.word(i); the context returns 0 beyond the strip's bytes, and the core
//     stops with kLzwInput once more bits are consumed than the strip holds;
//   - ctx.literal / ctx.copy are only called with pos + len <= out_n and offset + len <= pos + 1 (a source inside what is out, or
//     one byte over it for KwKwK, where every byte read still lies before pos: byte k comes from offset + k % (pos - offset));
//   - ctx.set_entry(i, ...) has i < min(kLzwEntries, out_n - 1): an entry is added per code but the first, a code gives at least a
//     byte, and the code that fills the rows adds none -- a launch over strips of at most B bytes needs min(kLzwEntries, B) entries;
//   - every loop iteration consumes a code of at least 9 bits, and the bits are bounded, so no input makes the decoder run on.
//
// The context:
//   uint32_t word(uint32_t i)                              bytes 4i .. 4i+3 of the strip, the first in the top byte; 0 beyond its end
//   uint32_t uni(uint32_t v)                               v, marked as the same in every lane (readfirstlane on the device)
//   void set_entry(uint32_t i, uint32_t off, uint32_t len) entry 258 + i
//   void get_entry(uint32_t i, uint32_t& off, uint32_t& len)
//   void literal(uint32_t pos, uint32_t b)                 out[pos] = b
//   void copy(uint32_t pos, uint32_t off, uint32_t len)    out[pos + k] = out[off + (k % (pos - off))], k < len (off < pos)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MI_LZW_HD __host__ __device__ __forceinline__
#else
#define MI_LZW_HD inline
#endif

namespace mi_lzw {

// status of a strip: 0 or why it ended
enum LzwStatus : int32_t {
    kLzwOk = 0,
    kLzwCode = 1,        // a code above the next free entry
    kLzwFirst = 2,       // the first code of the strip, or after Clear, is not a literal
    kLzwInput = 3,       // the input ended (or EOI came) before the rows were full
    kLzwOutput = 4,      // a string would pass the end of the rows
    kLzwOldStyle = 5,    // the bit-reversed stream of LZW writers before TIFF 5.0 (libtiff's "compat" decoder)
    kLzwTable = 6,       // entry 4094 asked for: the table is full and no Clear came
    kLzwStatusCount = 7
};

MI_LZW_HD const char* status_name(int s) {
    switch (s) {
        case kLzwOk: return "ok";
        case kLzwCode: return "code above the next free entry";
        case kLzwFirst: return "first code is not a literal";
        case kLzwInput: return "input exhausted";
        case kLzwOutput: return "output passes the rows";
        case kLzwOldStyle: return "old-style LSB-first stream";
        case kLzwTable: return "table overflow without Clear";
        default: return "unknown";
    }
}

constexpr uint32_t kLzwClear = 256, kLzwEoi = 257, kLzwFirstEntry = 258, kLzwLastEntry = 4093;
constexpr uint32_t kLzwEntries = kLzwLastEntry - kLzwFirstEntry + 1;   // 3836

// entries a strip of out_n raw bytes can add
MI_LZW_HD uint32_t table_entries(uint32_t out_n) { return out_n < kLzwEntries ? out_n : kLzwEntries; }

// the bit reader, most significant bit first: at least 33 bits after fill()
template <class Ctx>
struct LzwBits {
    uint64_t buf = 0;   // the low n bits are the next bits of the stream
    uint32_t n = 0, widx = 0;
    MI_LZW_HD void fill(Ctx& ctx) {
        if (n <= 32) {
            buf = (buf << 32) | (uint64_t)ctx.word(widx);
            widx += 1;
            n += 32;
        }
    }
    MI_LZW_HD uint32_t take(uint32_t k) {
        n -= k;
        return (uint32_t)(buf >> n) & ((1u << k) - 1u);
    }
    MI_LZW_HD uint64_t consumed() const { return (uint64_t)widx * 32u - n; }
};

// One strip of in_n bytes that must give exactly out_n bytes.
template <class Ctx>
MI_LZW_HD int lzw_decode(Ctx& ctx, uint32_t in_n, uint32_t out_n) {
    if (out_n == 0) return kLzwOk;
    const uint64_t in_bits = (uint64_t)in_n * 8u;
    // libtiff's test (LZWPreDecode): the first byte 0 and the lowest bit of the second set is Clear read from the low bit up
    if (in_n >= 2) {
        const uint32_t w0 = ctx.word(0);
        if ((w0 >> 24) == 0u && ((w0 >> 16) & 1u)) return kLzwOldStyle;
    }
    LzwBits<Ctx> b;
    uint32_t nbits = 9, free_ent = kLzwFirstEntry, pos = 0;
    uint32_t prev_pos = 0, prev_len = 0;   // where the code before was emitted; prev_len 0: none since the start or Clear
    for (;;) {
        b.fill(ctx);
        const uint32_t code = ctx.uni(b.take(nbits));
        if (b.consumed() > in_bits) return kLzwInput;
        if (code == kLzwEoi) return kLzwInput;   // (the rows are not full: a full strip has returned below)
        if (code == kLzwClear) {
            nbits = 9;
            free_ent = kLzwFirstEntry;
            prev_len = 0;
            continue;
        }
        if (code > free_ent) return kLzwCode;
        uint32_t off = 0, len = 1;
        if (code >= kLzwFirstEntry) {
            if (prev_len == 0) return kLzwFirst;
            if (code < free_ent) ctx.get_entry(code - kLzwFirstEntry, off, len);
            else {
                off = prev_pos;
                len = prev_len + 1;
            }
        }
        if (len > out_n - pos) return kLzwOutput;
        if (prev_len != 0) {
            if (free_ent > kLzwLastEntry) return kLzwTable;
            ctx.set_entry(free_ent - kLzwFirstEntry, prev_pos, prev_len + 1);
            free_ent += 1;
            if (free_ent + 1 >= (1u << nbits) && nbits < 12) nbits += 1;
        }
        if (code < 256) ctx.literal(pos, code);
        else ctx.copy(pos, off, len);
        prev_pos = pos;
        prev_len = len;
        pos += len;
        if (pos == out_n) return kLzwOk;
    }
}

// the context of a host call: one thread does everything
struct HostCtx {
    const unsigned char* in;
    uint32_t in_n;
    unsigned char* out;
    uint32_t* off;    // table_entries(out_n) each
    uint16_t* len;
    inline uint32_t word(uint32_t i) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t at = (uint64_t)i * 4u + k;
            if (at < in_n) v |= (uint32_t)in[at] << (24 - 8 * k);
        }
        return v;
    }
    inline uint32_t uni(uint32_t v) const { return v; }
    inline void set_entry(uint32_t i, uint32_t o, uint32_t l) {
        off[i] = o;
        len[i] = (uint16_t)l;
    }
    inline void get_entry(uint32_t i, uint32_t& o, uint32_t& l) const {
        o = off[i];
        l = len[i];
    }
    inline void literal(uint32_t pos, uint32_t b) { out[pos] = (unsigned char)b; }
    inline void copy(uint32_t pos, uint32_t o, uint32_t l) {
        for (uint32_t k = 0; k < l; ++k) out[pos + k] = out[o + k];   // ascending: a source byte at or past pos is already written
    }
};

// in[0, in_n) -> out[0, out_n) on the calling thread with a table of table_entries(out_n) entries at off / len; an LzwStatus
inline int lzw_host(const unsigned char* in, uint32_t in_n, unsigned char* out, uint32_t out_n, uint32_t* off, uint16_t* len) {
    HostCtx ctx{in, in_n, out, off, len};
    return lzw_decode(ctx, in_n, out_n);
}

}  // namespace mi_lzw
