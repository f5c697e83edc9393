// TIFF 6.0 section 13 LZW, the one coder (and, below it, the one decoder) of the library: satcv_lzw_encode_host runs it on the CPU, lzw_tiles_kernel (csrc/raster.hip)
// runs the same code with one wavefront per tile.  The stream is made unique by these rules (include/satcv.h, satcv_lzw_tiles):
//   MSB-first bit packing; Clear (256) first, at 9 bits; greedy longest match; the first free code is 258;
//   after an entry is added: next free code 4094 -> Clear at the current width, start over at 9 bits; 512 / 1024 / 2048 -> one bit wider
//   (libtiff's "early change"); after the last data code the same counter step once more; then EOI (257), zero-padded to a byte.
// Dictionary: an open-addressed table of SLOTS 32-bit words, (20-bit key = prefix code << 8 | byte) << 12 | 12-bit code, EMPTY = all ones
// (no key is 0xfffff: a prefix is at most 4093).  At most 3836 entries live between two Clears -- load factor <= 0.47 -- and the probe
// loop is bounded by SLOTS, so no loop here has a bound that depends on the data.
// Sink: void byte(unsigned) receives the stream; void clear(uint32_t* table) empties the table (the device sink does it with all lanes).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LZW_HD __host__ __device__ __forceinline__
#else
#define LZW_HD inline
#endif

namespace satcv_lzw {

constexpr int SLOTS = 8192;
constexpr uint32_t EMPTY = 0xffffffffu;
constexpr int CLEAR = 256, EOI = 257, FIRST = 258, LIMIT = 4094;

template <class Sink>
struct Coder {
  uint32_t* table;
  Sink* sink;
  int next, width, prefix;
  uint32_t acc;      // the low `nacc` bits wait for a full byte
  int nacc;

  LZW_HD void put(int code) {
    acc = (acc << width) | (uint32_t)code;
    nacc += width;                       // <= 7 + 12
    if (nacc >= 8) { nacc -= 8; sink->byte((acc >> nacc) & 0xffu); }
    if (nacc >= 8) { nacc -= 8; sink->byte((acc >> nacc) & 0xffu); }
  }
  // the counter step after an entry (or, at the end, the last data code); true: a Clear went out and the table is to be emptied
  LZW_HD bool bump() {
    ++next;
    if (next == LIMIT) {
      put(CLEAR);
      next = FIRST;
      width = 9;
      return true;
    }
    if (next == 512 || next == 1024 || next == 2048) ++width;
    return false;
  }
  LZW_HD void start() {
    sink->clear(table);
    next = FIRST;
    width = 9;
    prefix = -1;
    acc = 0;
    nacc = 0;
    put(CLEAR);
  }
  LZW_HD void feed(unsigned b) {
    if (prefix < 0) { prefix = (int)b; return; }
    const uint32_t key = ((uint32_t)prefix << 8) | b;
    uint32_t h = (key * 2654435761u) >> 19;       // 13 bits
    for (int probe = 0; probe < SLOTS; ++probe) {
      const uint32_t s = table[h];
      if (s == EMPTY) break;
      if ((s >> 12) == key) { prefix = (int)(s & 0xfffu); return; }
      h = (h + 1) & (SLOTS - 1);
    }
    put(prefix);
    table[h] = (key << 12) | (uint32_t)next;
    if (bump()) sink->clear(table);
    prefix = (int)b;
  }
  LZW_HD void finish() {
    if (prefix >= 0) {
      put(prefix);
      bump();                            // (a Clear here leaves a table nobody reads again)
    }
    put(EOI);
    if (nacc > 0) sink->byte((acc << (8 - nacc)) & 0xffu);
  }
};

// ---------------------------------------------------------------- the decoder
// Accepts every TIFF 6.0 section 13 stream libtiff accepts (MSB-first; not the LSB-first "old-style" variant): the initial state is the
// state after a Clear, a Clear may come anywhere, EOI may be missing (decoding ends when `cap` bytes are out), and a full table takes no
// more entries while the width stays 12.  Widths follow the reader's side of "early change": one bit wider once the NEXT FREE code is
// 511, 1023 or 2047 (the writer's counter in Coder::bump is one entry ahead).
// Dictionary: entry k is the previous code's string followed by the first byte of the current one, and those bytes lie next to each
// other in the output, so an entry is (position of its string in the output, length): pos[4096] and len[4096], no prefix chain.  A code
// is decoded by copying len bytes from an earlier output position to the current one; the one string that is not complete when it is
// referenced is code == next free ("KwKwK"): its last byte is its own first byte (`wrap`).  Every entry is made from positions the
// decoder itself wrote, so pos + len <= bytes written whatever the stream holds, and len <= 4096 - 257.
// Source: unsigned byte(long long i), i < in_bytes.  Sink: void literal(long long at, unsigned b); void copy(long long from, int len,
// long long at, bool wrap) -- out[at + j] = out[from + (wrap && j == len - 1 ? 0 : j)], j < len, from + len <= at + (wrap ? 1 : 0).
// Loop bounds: the codes of in_bytes bytes (each at least 9 bits); a copy is the sink's, at most 4096 bytes.
constexpr int DEC_OK = 0, DEC_TRUNCATED = 1, DEC_BAD_CODE = 2, DEC_OVERLONG = 3;
constexpr int TABLE = 4096;

template <class Source, class Sink>
struct Decoder {
  uint32_t* pos;     // TABLE entries; those below FIRST are not used
  uint16_t* len;
  Source* src;
  Sink* sink;

  // -> status; *produced: the bytes written (<= cap).  Nothing is read at or past in_bytes, nothing is written at or past cap.
  LZW_HD int run(long long in_bytes, long long cap, long long* produced) {
    long long n = 0, ibyte = 0;
    uint32_t acc = 0;
    int nacc = 0, next = FIRST, width = 9, status = DEC_TRUNCATED;
    bool has_prev = false;
    long long prev_pos = 0;
    int prev_len = 0;
    const long long max_codes = in_bytes * 8 / 9;
    if (cap <= 0) status = DEC_OK;
    else
      for (long long k = 0; k < max_codes; ++k) {
        if (nacc < width && ibyte < in_bytes) { acc = (acc << 8) | src->byte(ibyte++); nacc += 8; }
        if (nacc < width && ibyte < in_bytes) { acc = (acc << 8) | src->byte(ibyte++); nacc += 8; }
        if (nacc < width) break;                                           // input exhausted inside a code
        nacc -= width;
        const int code = (int)((acc >> nacc) & ((1u << width) - 1u));
        if (code == EOI) { status = DEC_OK; break; }
        if (code == CLEAR) { next = FIRST; width = 9; has_prev = false; continue; }
        long long sp = n;
        int sl = 1;
        bool wrap = false;
        if (!has_prev) {
          if (code > 255) { status = DEC_BAD_CODE; break; }                // the first code after a Clear is a literal
        } else {
          const bool added = next < TABLE;
          if (added) { pos[next] = (uint32_t)prev_pos; len[next] = (uint16_t)(prev_len + 1); }
          if (code > 255) {
            if (code >= next + (added ? 1 : 0)) { status = DEC_BAD_CODE; break; }
            sp = pos[code];
            sl = len[code];
            wrap = code == next;
          }
          if (added) ++next;
        }
        if (n + sl > cap) { status = DEC_OVERLONG; break; }
        if (code < 256) sink->literal(n, (unsigned)code);
        else sink->copy(sp, sl, n, wrap);
        prev_pos = n;
        prev_len = sl;
        has_prev = true;
        n += sl;
        if (next == 511 || next == 1023 || next == 2047) ++width;
        if (n >= cap) { status = DEC_OK; break; }                          // the block is full: EOI is not required
      }
    *produced = n;
    return status;
  }
};

}  // namespace satcv_lzw
