/* Sanitizer driver of the LZW decoder on the host (tests/test_raster_read_cpu.py::test_host_decoder_on_malformed_streams_under_asan_ubsan).
 *
 * Linked, in the normal way, against csrc/_obj_asan/libsatcv_hostasan.so -- every source of the library compiled with `--cuda-host-only
 * -fsanitize=address,undefined`: no kernel exists in it, nothing can launch -- and itself built with the same clang and sanitizers.
 * satcv_lzw_decode_host runs the decoder of csrc/lzw_core.hpp, the one the device runs per block, so what is shown here for its index
 * arithmetic holds for the kernel's too.  The stream lies in a heap block of exactly its length (a byte read past it is a sanitizer
 * report), the output in a block of `cap` bytes followed by a canary.  On a good stream of about 200 bytes: every truncation length,
 * every single-bit flip and an output cap one byte short; on a stream that reaches 12-bit codes: a code above the next free one planted
 * at each width.  Required every time: a status of 0 ... 3, a size of at most cap, an untouched canary; exit code 0 and no sanitizer
 * report = pass.  No GPU is touched. */
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
static long runs = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++fails; } } while (0)
#define CANARY 32

static uint32_t rng_state = 2024u;
static unsigned rnd(void) { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 24; }

/* decode `ns` bytes of stream into at most cap bytes; the stream is copied into a block of exactly ns bytes.  Returns the status,
 * *got the size; `want` (may be NULL): what status 0 with a full output must equal */
static int decode(const unsigned char* s, long ns, long cap, const unsigned char* want, long* got, const char* what) {
  unsigned char* in = (unsigned char*)malloc(ns ? (size_t)ns : 1);
  memcpy(in, s, (size_t)ns);
  unsigned char* out = (unsigned char*)malloc((size_t)cap + CANARY);
  memset(out, 0x5a, (size_t)cap + CANARY);
  int64_t size = -1;
  int32_t status = -1;
  const int rc = satcv_lzw_decode_host(ns ? in : NULL, ns, out, cap, &size, &status);
  ++runs;
  EXPECT(rc == 0, "%s: the call failed: %s", what, satcv_last_error());
  EXPECT(status >= 0 && status <= 3, "%s: status %d", what, (int)status);
  EXPECT(size >= 0 && size <= cap, "%s: size %lld of cap %ld", what, (long long)size, cap);
  for (int k = 0; k < CANARY; ++k) EXPECT(out[cap + k] == 0x5a, "%s: canary byte %d was written", what, k);
  if (want && status == 0 && size == cap) EXPECT(memcmp(out, want, (size_t)cap) == 0, "%s: status 0 with other bytes", what);
  if (got) *got = (long)size;
  free(out);
  free(in);
  return status;
}

static void put_bits(unsigned char* s, long bitpos, int width, unsigned value) {
  for (int k = 0; k < width; ++k, ++bitpos) {
    const unsigned bit = (value >> (width - 1 - k)) & 1u;
    s[bitpos >> 3] = (unsigned char)((s[bitpos >> 3] & ~(0x80u >> (bitpos & 7))) | (bit ? (0x80u >> (bitpos & 7)) : 0u));
  }
}

/* the bit position of the first data code of `width` bits that follows another data code, by the reader's counter rules; -1: none */
static long first_code_of_width(const unsigned char* s, long ns, int target, int* next_there) {
  long bitpos = 0;
  int width = 9, next = 258, has_prev = 0;
  while (bitpos + width <= ns * 8) {
    unsigned code = 0;
    for (int k = 0; k < width; ++k) code = (code << 1) | ((s[(bitpos + k) >> 3] >> (7 - ((bitpos + k) & 7))) & 1u);
    if (code == 257) return -1;
    if (code != 256 && has_prev && width == target) { *next_there = next; return bitpos; }
    bitpos += width;
    if (code == 256) { width = 9; next = 258; has_prev = 0; continue; }
    if (has_prev && next < 4096) ++next;
    has_prev = 1;
    if (next == 511 || next == 1023 || next == 2047) ++width;
  }
  return -1;
}

int main(void) {
  /* ---- a good stream of about 200 bytes: low-entropy bytes, so that it holds literals, table codes and KwKwK strings */
  unsigned char src[2048];
  for (int i = 0; i < 2048; ++i) src[i] = (unsigned char)((i / 7) % 3 == 0 ? 0 : rnd() & 3);
  unsigned char stream[4200];
  long n = 0;
  int64_t size = 0;
  for (n = 64; n <= 2048; ++n) {
    EXPECT(satcv_lzw_encode_host(src, n, stream, sizeof(stream), &size) == 0, "encode: %s", satcv_last_error());
    if (size >= 200) break;
  }
  EXPECT(size >= 200 && size < 260, "the good stream has %lld bytes", (long long)size);
  long got = -1;
  EXPECT(decode(stream, (long)size, n, src, &got, "good stream") == 0 && got == n, "the good stream decodes to %ld of %ld bytes", got, n);
  EXPECT(decode(stream, (long)size, n + 100, NULL, &got, "good stream, roomy cap") == 0 && got == n, "EOI ends the stream: %ld", got);

  /* ---- every truncation length */
  for (long cut = 0; cut < size; ++cut) {
    const int st = decode(stream, cut, n, src, &got, "truncated");
    EXPECT(st == 1 || (st == 0 && got == n), "cut at %ld: status %d with %ld bytes", cut, st, got);
  }
  /* ---- every single-bit flip */
  for (long bit = 0; bit < size * 8; ++bit) {
    stream[bit >> 3] ^= (unsigned char)(0x80u >> (bit & 7));
    decode(stream, (long)size, n, NULL, &got, "bit flip");
    decode(stream, (long)size, n / 2, NULL, &got, "bit flip, half the room");
    stream[bit >> 3] ^= (unsigned char)(0x80u >> (bit & 7));
  }
  /* ---- an output cap one byte short, and every shorter one */
  for (long cap = 0; cap < n; ++cap) {
    const int st = decode(stream, (long)size, cap, NULL, &got, "short cap");
    EXPECT(st == 0 || st == 3, "cap %ld of %ld: status %d", cap, n, st);
    if (st == 0) EXPECT(got == cap, "cap %ld: status 0 with %ld bytes", cap, got);
  }

  /* ---- a code above the next free one, planted at each width: a stream of random bytes reaches 12 bits */
  const long big_n = 6000;
  unsigned char* big = (unsigned char*)malloc((size_t)big_n);
  for (long i = 0; i < big_n; ++i) big[i] = (unsigned char)rnd();
  unsigned char* bs = (unsigned char*)malloc(2 * (size_t)big_n + 16);
  EXPECT(satcv_lzw_encode_host(big, big_n, bs, 2 * big_n + 16, &size) == 0, "encode: %s", satcv_last_error());
  EXPECT(decode(bs, (long)size, big_n, big, &got, "random stream") == 0 && got == big_n, "the random stream decodes to %ld bytes", got);
  for (int width = 9; width <= 12; ++width) {
    int next = 0;
    const long at = first_code_of_width(bs, (long)size, width, &next);
    EXPECT(at >= 0, "no code of %d bits", width);
    if (at < 0) continue;
    unsigned char* bad = (unsigned char*)malloc((size_t)size);
    memcpy(bad, bs, (size_t)size);
    put_bits(bad, at, width, (1u << width) - 1u);          /* all ones: above the next free code, which is at most 2^width - 2 here */
    EXPECT((int)((1u << width) - 1u) > next + 1, "width %d: next free %d", width, next);
    EXPECT(decode(bad, (long)size, big_n, NULL, &got, "planted code") == 2, "a code above next free at %d bits must give status 2", width);
    put_bits(bad, at, width, (unsigned)next + 2u);         /* just above: next + 1 is the first code that cannot exist (next itself is KwKwK) */
    EXPECT(decode(bad, (long)size, big_n, NULL, &got, "planted code, just above") == 2, "code next + 2 at %d bits must give status 2", width);
    free(bad);
  }
  free(bs);
  free(big);

  /* ---- a full table, as a foreign writer may leave it: zeros coded as 0, 258, 259, ... 4095 (each the KwKwK string, one byte longer than
   * the last) without a Clear, then 4095 ten times more at 12 bits -- no entry is added, the width stays 12 -- and EOI */
  {
    unsigned char* fs = (unsigned char*)calloc(8192, 1);
    long bitpos = 0, total = 1;
    int width = 9;
    put_bits(fs, bitpos, width, 256); bitpos += width;
    put_bits(fs, bitpos, width, 0); bitpos += width;
    for (int c = 258; c <= 4095; ++c) {
      put_bits(fs, bitpos, width, (unsigned)c); bitpos += width;
      total += c - 256;
      if (c + 1 == 511 || c + 1 == 1023 || c + 1 == 2047) ++width;
    }
    for (int k = 0; k < 10; ++k) { put_bits(fs, bitpos, 12, 4095); bitpos += 12; total += 4095 - 256; }
    put_bits(fs, bitpos, 12, 257); bitpos += 12;
    const long fsize = (bitpos + 7) / 8;
    unsigned char* zeros = (unsigned char*)calloc((size_t)total, 1);
    EXPECT(decode(fs, fsize, total, zeros, &got, "full table") == 0 && got == total, "the full-table stream decodes to %ld of %ld bytes", got, total);
    EXPECT(decode(fs, fsize, total - 1, zeros, &got, "full table, cap one short") == 3, "the last string passes the cap");
    EXPECT(decode(fs, fsize - 2, total, NULL, &got, "full table, cut") == 1, "cut before EOI with room left");
    free(zeros);
    free(fs);
  }

  /* ---- refusals: nothing is dereferenced */
  int32_t status = 0;
  unsigned char b[16] = {0};
  EXPECT(satcv_lzw_decode_host(b, 4, b, 4, NULL, &status) != 0 && satcv_lzw_decode_host(b, 4, b, 4, &size, NULL) != 0, "NULL size / status");
  EXPECT(satcv_lzw_decode_host(NULL, 4, b, 4, &size, &status) != 0 && satcv_lzw_decode_host(b, 4, NULL, 4, &size, &status) != 0, "NULL src / dst");
  EXPECT(satcv_lzw_decode_host(b, -1, b, 4, &size, &status) != 0 && satcv_lzw_decode_host(b, 4, b, -1, &size, &status) != 0, "negative n / cap");
  EXPECT(satcv_lzw_decode_host(b, 4, b, (int64_t)1 << 30, &size, &status) != 0, "cap 2^30");
  EXPECT(satcv_lzw_decode_tiles(NULL, 16, (const int64_t*)b, (const int32_t*)b, 1, 16, b, 16, &status, NULL, NULL) != 0, "decode_tiles: null payload");
  EXPECT(satcv_lzw_decode_tiles(b, 16, (const int64_t*)b, (const int32_t*)b, 0, 16, b, 16, &status, NULL, NULL) != 0, "decode_tiles: n = 0");
  EXPECT(satcv_lzw_decode_tiles(b, 16, (const int64_t*)b, (const int32_t*)b, 1, 16, b, 8, &status, NULL, NULL) != 0, "decode_tiles: stride below the block");
  satcv_untile_desc u;
  memset(&u, 0, sizeof(u));
  EXPECT(satcv_raster_untile(NULL, NULL) != 0 && satcv_raster_untile(&u, NULL) != 0, "untile: null");
  u.src = b; u.dst = b; u.blocks = (const int32_t*)b; u.nblocks = 1; u.bh = 2; u.bw = 2; u.across = 1; u.spp = 1; u.planar = 1; u.h = 2; u.w_ = 2; u.ld = 1; u.src_stride = 16;
  satcv_untile_desc v = u; v.spp = 17;
  EXPECT(satcv_raster_untile(&v, NULL) != 0 && strstr(satcv_last_error(), "bands"), "untile: spp 17: %s", satcv_last_error());
  v = u; v.planar = 3;
  EXPECT(satcv_raster_untile(&v, NULL) != 0 && strstr(satcv_last_error(), "planar"), "untile: planar 3: %s", satcv_last_error());
  v = u; v.kind = 2; v.predictor = 2; v.src_stride = 16;
  EXPECT(satcv_raster_untile(&v, NULL) != 0 && strstr(satcv_last_error(), "predictor"), "untile: predictor on f32: %s", satcv_last_error());
  v = u; v.predictor = 3;
  EXPECT(satcv_raster_untile(&v, NULL) != 0 && strstr(satcv_last_error(), "predictor"), "untile: predictor 3: %s", satcv_last_error());
  v = u; v.band_map[0] = 1;
  EXPECT(satcv_raster_untile(&v, NULL) != 0 && strstr(satcv_last_error(), "band_map"), "untile: band_map past ld: %s", satcv_last_error());
  v = u; v.src_stride = 3;
  EXPECT(satcv_raster_untile(&v, NULL) != 0 && strstr(satcv_last_error(), "src_stride"), "untile: stride below the block: %s", satcv_last_error());
  v = u; v.bh = 1 << 20; v.bw = 1 << 20;
  EXPECT(satcv_raster_untile(&v, NULL) != 0 && strstr(satcv_last_error(), "2^30"), "untile: block bytes: %s", satcv_last_error());
  v = u; v.h = 0x7fffffff; v.w_ = 0x7fffffff;
  EXPECT(satcv_raster_untile(&v, NULL) != 0, "untile: window beyond 2^31 pixels");

  printf("lzw decode driver: %ld runs, %d failures\n", runs, fails);
  return fails ? 1 : 0;
}
