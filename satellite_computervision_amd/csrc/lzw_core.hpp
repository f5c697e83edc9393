// TIFF 6.0 section 13 LZW, the one coder of the library: satcv_lzw_encode_host runs it on the CPU, lzw_tiles_kernel (csrc/raster.hip)
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

}  // namespace satcv_lzw
