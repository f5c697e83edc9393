/* Sanitizer driver of the host entries of the GeoTIFF writer (tests/test_raster_cpu.py::test_host_entries_under_asan_ubsan).
 *
 * Linked, in the normal way, against csrc/_obj_asan/libsatcv_hostasan.so -- every source of the library compiled with `--cuda-host-only
 * -fsanitize=address,undefined`: no kernel exists in it, nothing can launch -- and itself built with the same clang and sanitizers.
 * It drives satcv_lzw_encode_host -- the coder the device runs per tile -- on exactly sized heap buffers, so that a byte read past the
 * input or written past `cap` is a sanitizer report: against a bitwise decoder on every input, with `cap` one byte too small (an
 * error, nothing written past cap), and the descriptor refusals of satcv_raster_convert / _overview / _tiles, satcv_lzw_tiles and
 * satcv_bytes_compact.  Exit code 0 and no sanitizer report = pass.  No GPU is touched. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "satcv.h"

/* the library was linked without device code: its module constructors must not hand (empty) device binaries to the HIP runtime */
void** __hipRegisterFatBinary(const void* data) { static void* handle; (void)data; return &handle; }
void __hipUnregisterFatBinary(void** h) { (void)h; }
void __hipRegisterFunction(void** h, const void* f, char* df, const char* dn, unsigned tl, void* tid, void* bid, void* bd, void* gd, int* ws) {
  (void)h; (void)f; (void)df; (void)dn; (void)tl; (void)tid; (void)bid; (void)bd; (void)gd; (void)ws; }
void __hipRegisterVar(void** h, void* v, char* hv, char* dv, int ext, size_t size, int constant, int global) {
  (void)h; (void)v; (void)hv; (void)dv; (void)ext; (void)size; (void)constant; (void)global; }
void __hipRegisterManagedVar(void* h, void** p, void* init, const char* name, size_t size, unsigned align) {
  (void)h; (void)p; (void)init; (void)name; (void)size; (void)align; }

static int fails = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++fails; } } while (0)

/* TIFF LZW decoder, the width rule of a reader: widen after its own table reaches 511, 1023 or 2047 entries.  Returns the decoded
 * length, or -1 for a malformed stream. */
static long lzw_decode(const unsigned char* s, long ns, unsigned char* out, long cap) {
  static int prefix_of[4096]; static unsigned char last_of[4096], first_of[4096]; static unsigned char stack[4096];
  long bitpos = 0, n = 0; int width = 9, next = 258, prev = -1;
  for (;;) {
    if (bitpos + width > ns * 8) return -1;
    int code = 0;
    for (int k = 0; k < width; ++k, ++bitpos) code = (code << 1) | ((s[bitpos >> 3] >> (7 - (bitpos & 7))) & 1);
    if (code == 257) return n;
    if (code == 256) { width = 9; next = 258; prev = -1; continue; }
    int cur = code;
    if (prev >= 0) {
      if (code > next || next >= 4096) return -1;
      prefix_of[next] = prev;
      first_of[next] = prev < 256 ? (unsigned char)prev : first_of[prev];
      last_of[next] = code == next ? first_of[next] : (code < 256 ? (unsigned char)code : first_of[code]);
      ++next;
    } else if (code >= 256) return -1;
    int sp = 0;
    while (cur >= 256) { stack[sp++] = last_of[cur]; cur = prefix_of[cur]; }
    stack[sp++] = (unsigned char)cur;
    while (sp > 0) { if (n >= cap) return -1; out[n++] = stack[--sp]; }
    prev = code;
    if (next == 511 || next == 1023 || next == 2047) ++width;
  }
}

static uint32_t rng_state = 12345u;
static unsigned rnd(void) { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 24; }

/* encode n bytes made by `fill` (0 constant, 1 random, 2 class grid 160 wide blown up 8 x, 3 random 16-bit low entropy) */
static void round_trip(long n, int fill, const char* what) {
  unsigned char* src = (unsigned char*)malloc(n ? (size_t)n : 1);
  for (long i = 0; i < n; ++i)
    src[i] = fill == 0 ? 3 : fill == 1 ? (unsigned char)rnd() : fill == 2 ? (unsigned char)((((i / 160) / 8) * 7 + ((i % 160) / 8) * 3) % 5) : (unsigned char)((i & 1) ? rnd() & 3 : rnd());
  const long cap = 2 * n + 16;
  unsigned char* dst = (unsigned char*)malloc((size_t)cap);
  int64_t size = -1;
  EXPECT(satcv_lzw_encode_host(src, n, dst, cap, &size) == 0 && size > 0 && size <= cap, "%s: encode: %s", what, satcv_last_error());
  unsigned char* back = (unsigned char*)malloc(n ? (size_t)n : 1);
  const long got = lzw_decode(dst, (long)size, back, n);
  EXPECT(got == n && memcmp(back, src, (size_t)n) == 0, "%s: decodes to %ld of %ld bytes", what, got, n);
  /* cap one byte too small, in a buffer of exactly that size: an error, and ASan sees any byte past it */
  if (size > 0) {
    unsigned char* tight = (unsigned char*)malloc((size_t)size - 1 ? (size_t)size - 1 : 1);
    int64_t need = -1;
    EXPECT(satcv_lzw_encode_host(src, n, tight, size - 1, &need) != 0 && need == size, "%s: cap one byte short must fail and report the need", what);
    EXPECT(strstr(satcv_last_error(), "needs") != NULL, "%s: message: %s", what, satcv_last_error());
    free(tight);
    unsigned char* exact = (unsigned char*)malloc((size_t)size);
    EXPECT(satcv_lzw_encode_host(src, n, exact, size, &need) == 0 && need == size && memcmp(exact, dst, (size_t)size) == 0, "%s: cap exact", what);
    free(exact);
  }
  free(back); free(dst); free(src);
}

int main(void) {
  round_trip(0, 0, "empty");
  round_trip(1, 1, "one byte");
  round_trip(6300, 0, "constant");
  round_trip(13000, 1, "random, several table resets");
  round_trip(160 * 160, 2, "class grid");
  round_trip(8192, 3, "16-bit samples");
  for (long n = 3960; n <= 3990; ++n) round_trip(n, 1, "random strip around one full table");
  for (long n = 2; n <= 40; ++n) round_trip(n, 1, "short");

  int64_t size = 0;
  unsigned char b[32] = {0};
  EXPECT(satcv_lzw_encode_host(b, 4, b + 16, 16, NULL) != 0, "NULL size");
  EXPECT(satcv_lzw_encode_host(NULL, 4, b, 16, &size) != 0, "NULL src");
  EXPECT(satcv_lzw_encode_host(b, 4, NULL, 16, &size) != 0, "NULL dst");
  EXPECT(satcv_lzw_encode_host(b, -1, b + 16, 16, &size) != 0 && satcv_lzw_encode_host(b, (int64_t)1 << 30, b + 16, 16, &size) != 0, "n out of range");
  EXPECT(satcv_lzw_encode_host(b, 4, b + 16, -1, &size) != 0, "negative cap");
  EXPECT(satcv_lzw_encode_host(NULL, 0, NULL, 0, &size) != 0 && size == 3, "the empty stream needs 3 bytes, cap 0 is refused: %lld", (long long)size);

  /* ---- descriptor refusals: nothing is dereferenced, nothing launches */
  satcv_raster_desc d; memset(&d, 0, sizeof(d));
  int (*entries[3])(const satcv_raster_desc*, void*) = {satcv_raster_convert, satcv_raster_overview, satcv_raster_tiles};
  for (int e = 0; e < 3; ++e) {
    EXPECT(entries[e](NULL, NULL) != 0, "NULL raster desc");
    EXPECT(entries[e](&d, NULL) != 0 && strstr(satcv_last_error(), "null"), "zeroed raster desc: %s", satcv_last_error());
    satcv_raster_desc t; memset(&t, 0, sizeof(t));
    t.src = b; t.dst = b; t.h = 4; t.w_ = 4; t.c = 1; t.ld = 1; t.blocksize = 16;
    satcv_raster_desc u = t; u.c = 17; u.ld = 17;
    EXPECT(entries[e](&u, NULL) != 0 && strstr(satcv_last_error(), "at most 16"), "c > 16: %s", satcv_last_error());
    u = t; u.src_kind = 4;
    EXPECT(entries[e](&u, NULL) != 0 && strstr(satcv_last_error(), "unknown kind"), "kind 4: %s", satcv_last_error());
    u = t; u.dst_kind = -1;
    EXPECT(entries[e](&u, NULL) != 0 && strstr(satcv_last_error(), "unknown kind"), "kind -1: %s", satcv_last_error());
    u = t; u.h = 0x7fffffff; u.w_ = 0x7fffffff;
    EXPECT(entries[e](&u, NULL) != 0, "extents beyond 2^31 pixels");
    u = t; u.h = -3;
    EXPECT(entries[e](&u, NULL) != 0, "negative extent");
    u = t; u.coff = 0x7fffffff; u.ld = 0x7fffffff;
    EXPECT(entries[e](&u, NULL) != 0, "channel range");
  }
  {
    satcv_raster_desc t; memset(&t, 0, sizeof(t));
    t.src = b; t.dst = b; t.h = 4; t.w_ = 4; t.c = 1; t.ld = 1; t.blocksize = 16;
    satcv_raster_desc u = t; u.blocksize = 24;
    EXPECT(satcv_raster_tiles(&u, NULL) != 0 && strstr(satcv_last_error(), "multiple of 16"), "blocksize 24: %s", satcv_last_error());
    u = t; u.blocksize = -16;
    EXPECT(satcv_raster_tiles(&u, NULL) != 0, "negative blocksize");
    u = t; u.blocksize = 0x7ffffff0; u.c = 16; u.ld = 16; u.src_kind = u.dst_kind = 5;
    EXPECT(satcv_raster_tiles(&u, NULL) != 0 && strstr(satcv_last_error(), "2^30"), "tile bytes: %s", satcv_last_error());
    u = t; u.src_kind = u.dst_kind = 2; u.predictor = 1;
    EXPECT(satcv_raster_tiles(&u, NULL) != 0 && strstr(satcv_last_error(), "predictor"), "predictor on float: %s", satcv_last_error());
    u = t; u.src_kind = u.dst_kind = 2; u.resampling = 2;
    EXPECT(satcv_raster_overview(&u, NULL) != 0 && strstr(satcv_last_error(), "mode"), "mode on float: %s", satcv_last_error());
    u = t; u.resampling = 0x7fffffff;
    EXPECT(satcv_raster_overview(&u, NULL) != 0, "unknown resampling");
    u = t; u.scale = 2.f;
    EXPECT(satcv_raster_convert(&u, NULL) != 0 && strstr(satcv_last_error(), "scale"), "scale on an integer source: %s", satcv_last_error());
  }
  int32_t sizes[4] = {0};
  int64_t offs[4] = {0};
  EXPECT(satcv_lzw_tiles(NULL, 1, 256, b, sizes, NULL) != 0 && satcv_lzw_tiles(b, 1, 256, NULL, sizes, NULL) != 0 && satcv_lzw_tiles(b, 1, 256, b, NULL, NULL) != 0, "lzw_tiles: null");
  EXPECT(satcv_lzw_tiles(b, 0, 256, b, sizes, NULL) != 0 && satcv_lzw_tiles(b, -1, 256, b, sizes, NULL) != 0, "lzw_tiles: n");
  EXPECT(satcv_lzw_tiles(b, 1, (int64_t)1 << 30, b, sizes, NULL) != 0 && strstr(satcv_last_error(), "2^30"), "lzw_tiles: tile_bytes 2^30: %s", satcv_last_error());
  EXPECT(satcv_lzw_tiles(b, 1, 0, b, sizes, NULL) != 0 && satcv_lzw_tiles(b, 1, -16, b, sizes, NULL) != 0 && satcv_lzw_tiles(b, 1, 24, b, sizes, NULL) != 0, "lzw_tiles: tile_bytes");
  EXPECT(satcv_lzw_tiles(b + 1, 1, 256, b + 1, sizes, NULL) != 0, "lzw_tiles: alignment");
  EXPECT(satcv_bytes_compact(NULL, 16, sizes, offs, 1, b, 16, NULL) != 0 && satcv_bytes_compact(b, 16, NULL, offs, 1, b, 16, NULL) != 0 &&
         satcv_bytes_compact(b, 16, sizes, NULL, 1, b, 16, NULL) != 0 && satcv_bytes_compact(b, 16, sizes, offs, 1, NULL, 16, NULL) != 0, "bytes_compact: null");
  EXPECT(satcv_bytes_compact(b, 0, sizes, offs, 1, b, 16, NULL) != 0 && satcv_bytes_compact(b, -1, sizes, offs, 1, b, 16, NULL) != 0 &&
         satcv_bytes_compact(b, INT64_MAX, sizes, offs, 1, b, 16, NULL) != 0, "bytes_compact: slot_bytes");
  EXPECT(satcv_bytes_compact(b, 16, sizes, offs, 0, b, 16, NULL) != 0 && satcv_bytes_compact(b, 16, sizes, offs, 1, b, 0, NULL) != 0, "bytes_compact: n, dst_bytes");

  printf("raster host driver: %d failures\n", fails);
  return fails ? 1 : 0;
}
