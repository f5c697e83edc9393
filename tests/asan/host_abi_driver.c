/* Sanitizer driver of the HOST side of the C ABI (tests/test_host_cpu.py::test_host_side_of_the_c_abi_under_asan_ubsan).
 *
 * Linked against csrc/_obj_asan/libsatcv_hostasan.so -- every source of the library compiled with `--cuda-host-only
 * -fsanitize=address,undefined`: no kernel exists in it, nothing can launch -- and itself built with the same clang and sanitizers.
 * It drives the code that runs on the host before any launch: descriptor validation (null / zeroed / inconsistent descriptors must be
 * REFUSED with a message, never dereferenced), the tile / split-K / weight-gradient planning behind the dry-run and workspace queries over
 * a sweep of shapes (integer overflow, out-of-range table indices, misaligned pointers), the job-size queries of the batched launches,
 * the option table, and the CRC-32C of the TFRecord framing against a bitwise restatement at every length and alignment up to 70 bytes.
 * Exit code 0 and no sanitizer report = pass.  No GPU is touched. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "satcv.h"

/* the library was linked without device code: its module constructors must not hand (empty) device binaries to the HIP runtime.  The
 * executable's definitions of the registration entry points take precedence over libamdhip64's */
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

static uint32_t crc32c_bitwise(const unsigned char* p, size_t n, uint32_t crc) {
  crc = ~crc;
  for (size_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0x82F63B78u & (0u - (crc & 1u)));
  }
  return ~crc;
}

int main(void) {
  /* ---- identification and the error channel */
  EXPECT(satcv_version() && strlen(satcv_version()) > 0, "version string");
  EXPECT(satcv_last_error() != NULL, "last_error must never be NULL");

  /* ---- CRC-32C (masked CRC of the TFRecord length / payload fields: utils/prediction_tools.py:159-226 readers) */
  unsigned char buf[96];
  for (int i = 0; i < 96; ++i) buf[i] = (unsigned char)(i * 37 + 11);
  for (int off = 0; off < 9; ++off)
    for (int n = 0; n <= 70; ++n) {
      const uint32_t a = satcv_crc32c(buf + off, (uint64_t)n, 0), b = crc32c_bitwise(buf + off, (size_t)n, 0);
      EXPECT(a == b, "crc32c len %d offset %d: %08x vs %08x", n, off, a, b);
      const int h = n / 2;      /* continuation */
      EXPECT(satcv_crc32c(buf + off + h, (uint64_t)(n - h), satcv_crc32c(buf + off, (uint64_t)h, 0)) == b, "crc32c continuation len %d", n);
    }
  EXPECT(satcv_crc32c("123456789", 9, 0) == 0xE3069283u, "crc32c check value");

  /* ---- options */
  int32_t v = -1;
  EXPECT(satcv_set_option("no_such_option", 1) != 0, "unknown option must be refused");
  EXPECT(satcv_get_option("no_such_option", &v) != 0, "unknown option must be refused");
  EXPECT(satcv_get_option("igemm_m16", &v) == 0 && v >= 0, "igemm_m16 option");
  EXPECT(satcv_set_option("igemm_m16", 2) == 0 && satcv_get_option("igemm_m16", &v) == 0 && v == 2, "set/get round trip");
  EXPECT(satcv_set_option(NULL, 1) != 0, "NULL key");
  /* the whole table by enumeration: every key reads; a set either round-trips (and is put back) or is refused with a message and changes nothing */
  int nkeys = 0, nsettable = 0;
  EXPECT(satcv_option_key(-1) == NULL, "option_key(-1)");
  for (const char* key; (key = satcv_option_key(nkeys)) != NULL; ++nkeys) {
    int32_t was = -12345, now = -12345;
    EXPECT(satcv_get_option(key, &was) == 0, "get_option(%s)", key);
    EXPECT(satcv_get_option(key, NULL) != 0, "get_option(%s, NULL)", key);
    if (satcv_set_option(key, was + 1) == 0) {
      ++nsettable;
      EXPECT(satcv_get_option(key, &now) == 0 && now == was + 1, "%s: set/get round trip", key);
      EXPECT(satcv_set_option(key, was) == 0, "%s: restore", key);
    } else {
      EXPECT(strstr(satcv_last_error(), key) != NULL, "%s: the refusal names the key: %s", key, satcv_last_error());
      EXPECT(satcv_get_option(key, &now) == 0 && now == was, "%s: a refused set must change nothing", key);
    }
  }
  EXPECT(satcv_option_key(nkeys + 1) == NULL && satcv_option_key(INT32_MAX) == NULL, "option_key past the end");
  EXPECT(nkeys == 34 && nsettable == 10, "%d keys, %d settable (include/satcv.h lists 34 and 10)", nkeys, nsettable);
  EXPECT(satcv_set_option("m16p_launches", 0) != 0 && satcv_set_option("wgrad_wgs", 256) != 0, "counters and startup-only keys are read-only");

  /* ---- null and zeroed descriptors: refused with a message, no dereference */
  satcv_conv_desc cd; memset(&cd, 0, sizeof(cd));
  EXPECT(satcv_conv2d_igemm(NULL, NULL) != 0, "NULL conv desc");
  EXPECT(satcv_conv2d_igemm(&cd, NULL) != 0 && strstr(satcv_last_error(), "null"), "zeroed conv desc: %s", satcv_last_error());
  EXPECT(satcv_conv2d_igemm_pipelined(NULL) == 0 && satcv_conv2d_igemm_pipelined(&cd) == 0, "dry run of an invalid descriptor answers 0");
  satcv_conv_plan_info ci;
  EXPECT(satcv_conv2d_igemm_plan_info(NULL, 256, &ci) != 0 && satcv_conv2d_igemm_plan_info(&cd, 256, NULL) != 0 && satcv_conv2d_igemm_plan_info(&cd, 256, &ci) != 0 &&
         satcv_conv2d_igemm_plan_info(&cd, -1, &ci) != 0, "invalid conv plan query");
  {
    /* channel counts, taps, extents and option-like fields out of range: refused with a message, nothing indexed by them */
    satcv_conv_desc bd2; memset(&bd2, 0, sizeof(bd2));
    bd2.c0 = 64; bd2.ldy = 64; bd2.n = 2; bd2.h = 8; bd2.w_ = 32; bd2.cout = 64; bd2.cout_pad = 64; bd2.kh = bd2.kw = 3; bd2.dil = 1; bd2.cstat = 64; bd2.dtype = SATCV_BF16;
    EXPECT(satcv_conv2d_igemm_plan_info(&bd2, 256, &ci) == 0 && ci.lds_bytes > 0 && ci.workgroups > 0, "null tensors are fine in a plan query: %s", satcv_last_error());
    satcv_conv_desc t = bd2; t.c0 = 24;
    EXPECT(satcv_conv2d_igemm_plan_info(&t, 256, &ci) != 0, "c0 not a multiple of 16");
    t = bd2; t.kh = 4;
    EXPECT(satcv_conv2d_igemm_plan_info(&t, 256, &ci) != 0, "even taps");
    t = bd2; t.mode_out = 1; t.f = 0;
    EXPECT(satcv_conv2d_igemm_plan_info(&t, 256, &ci) != 0, "depth-to-space without a factor");
    t = bd2; t.stride = 2;
    EXPECT(satcv_conv2d_igemm_plan_info(&t, 256, &ci) != 0, "stride without the input extents");
    t = bd2; t.pair_n = 3;
    EXPECT(satcv_conv2d_igemm_plan_info(&t, 256, &ci) != 0, "pair store of an odd batch");
    t = bd2; t.dtype = 77;
    EXPECT(satcv_conv2d_igemm_plan_info(&t, 256, &ci) != 0, "unknown dtype");
    t = bd2; t.n = 0x7fffffff; t.h = 0x7fffffff; t.w_ = 0x7fffffff;
    EXPECT(satcv_conv2d_igemm_plan_info(&t, 256, &ci) != 0, "extents beyond 2^31 pixels");
    t = bd2; t.tile_policy = 0x7fffffff; t.pool_f = -5; t.bst_ld = -1;
    (void)satcv_conv2d_igemm_plan_info(&t, 0x7fffffff, &ci);
  }
  satcv_wgrad_desc wd; memset(&wd, 0, sizeof(wd));
  EXPECT(satcv_conv2d_wgrad(NULL, NULL) != 0 && satcv_conv2d_wgrad(&wd, NULL) != 0, "invalid wgrad desc");
  EXPECT(satcv_conv2d_wgrad_workspace(NULL) < 0, "wgrad workspace of NULL");
  satcv_wgrad_plan_info wi;
  EXPECT(satcv_conv2d_wgrad_plan_info(NULL, &wi) != 0 && satcv_conv2d_wgrad_plan_info(&wd, NULL) != 0 && satcv_conv2d_wgrad_plan_info(&wd, &wi) != 0,
         "invalid wgrad plan query");
  satcv_bwdf_desc fd; memset(&fd, 0, sizeof(fd));
  EXPECT(satcv_conv2d_bwd_fused(NULL, NULL) != 0 && satcv_conv2d_bwd_fused(&fd, NULL) != 0, "invalid fused desc");
  EXPECT(satcv_conv2d_bwd_fused_workspace(NULL) < 0 && satcv_conv2d_bwd_fused_workspace(&fd) < 0, "fused workspace of an invalid desc");
  {
    /* the fused backward kernels' plan queries: null / zeroed / out-of-limits descriptors are refused with a message; a served one reports a
     * geometry that adds up, for any CU count, with no device */
    satcv_bwdf_plan_info fi; satcv_ctbf_plan_info ti;
    satcv_ctbf_desc td; memset(&td, 0, sizeof(td));
    EXPECT(satcv_conv2d_bwd_fused_plan_info(NULL, 256, &fi) != 0 && satcv_conv2d_bwd_fused_plan_info(&fd, 256, NULL) != 0 &&
           satcv_conv2d_bwd_fused_plan_info(&fd, 256, &fi) != 0 && satcv_conv2d_bwd_fused_plan_info(&fd, -1, &fi) != 0, "invalid fused plan query");
    EXPECT(satcv_convt_bwd_fused_plan_info(NULL, 256, &ti) != 0 && satcv_convt_bwd_fused_plan_info(&td, 256, NULL) != 0 &&
           satcv_convt_bwd_fused_plan_info(&td, 256, &ti) != 0 && satcv_convt_bwd_fused_plan_info(&td, -1, &ti) != 0, "invalid convT fused plan query");
    EXPECT(satcv_convt_bwd_fused_workspace(NULL) < 0 && satcv_convt_bwd_fused_workspace(&td) < 0 && satcv_convt_bwd_fused(&td, NULL) != 0, "invalid convT fused desc");
    void* fk = (void*)(uintptr_t)0x7f0000001000ull;
    static const int FC[][2] = {{32, 32}, {64, 32}, {64, 64}, {32, 64}, {48, 32}, {64, 128}};
    static const int NCU[] = {1, 8, 255, 256, 304, 0x7fffffff};
    int served = 0;
    for (unsigned c = 0; c < sizeof(FC) / sizeof(FC[0]); ++c)
      for (int n = 1; n <= 64; n *= 4)
        for (int h = 8; h <= 264; h += 64)
          for (int w = 32; w <= 288; w += 64)
            for (unsigned k = 0; k < sizeof(NCU) / sizeof(NCU[0]); ++k) {
              satcv_bwdf_desc d; memset(&d, 0, sizeof(d));
              d.g = fk; d.yraw = fk; d.ldg = FC[c][1]; d.x0 = fk; d.c0 = FC[c][0]; d.w_dgrad = fk; d.dx = fk; d.lddx = FC[c][0]; d.dw = (float*)fk;
              d.cin = FC[c][0]; d.cout = FC[c][1]; d.n = n; d.h = h; d.w_ = w; d.kh = d.kw = 3; d.dil = 1; d.dtype = SATCV_BF16;
              (void)satcv_set_option("no_such_option", 1);
              if (satcv_conv2d_bwd_fused_plan_info(&d, NCU[k], &fi) == 0) {
                ++served;
                EXPECT(fi.workgroups > 0 && fi.workgroups <= fi.tiles && fi.tiles == (int64_t)n * (h / 8) * (w / 32) && fi.tiles_min >= 1 &&
                       fi.tiles_max - fi.tiles_min <= 1 && fi.tiles_min * fi.workgroups <= fi.tiles && fi.tiles_max * fi.workgroups >= fi.tiles &&
                       fi.lds_bytes > 0 && fi.lds_bytes <= 160 * 1024 && fi.ws_bytes == fi.workgroups * 9 * fi.cin * fi.cout * 4, "fused plan geometry");
              } else EXPECT(!strstr(satcv_last_error(), "no_such_option"), "a refused fused plan query says why");
              satcv_ctbf_desc t; memset(&t, 0, sizeof(t));
              t.g = fk; t.ldg = 2 * FC[c][1]; t.yup = fk; t.ldy = FC[c][1]; t.x = fk; t.ldx = 2 * FC[c][0]; t.w_dgrad = fk; t.w_npad = 2 * FC[c][0]; t.dx = fk; t.lddx = 2 * FC[c][0];
              t.dw = (float*)fk; t.cin = 2 * FC[c][0]; t.cout = FC[c][1]; t.n = n; t.h = h; t.w_ = w; t.f = 2; t.dtype = SATCV_BF16;
              (void)satcv_set_option("no_such_option", 1);
              if (satcv_convt_bwd_fused_plan_info(&t, NCU[k], &ti) == 0) {
                ++served;
                EXPECT(ti.slabs > 0 && ti.slabs <= ti.tiles && ti.nblk * ti.cblk == t.cin && ti.tiles == (int64_t)n * h * (w / ti.px) && ti.tiles_min >= 1 &&
                       ti.tiles_max - ti.tiles_min <= 1 && ti.tiles_min * ti.slabs <= ti.tiles && ti.tiles_max * ti.slabs >= ti.tiles &&
                       ti.lds_bytes > 0 && ti.lds_bytes <= 160 * 1024 && ti.ws_bytes == ti.slabs * t.cin * ti.cout4 * 4, "convT fused plan geometry");
              } else EXPECT(!strstr(satcv_last_error(), "no_such_option"), "a refused convT fused plan query says why");
            }
    EXPECT(served > 500, "fused plan queries answered (%d)", served);
    satcv_bwdf_desc d; memset(&d, 0, sizeof(d));
    d.g = fk; d.yraw = fk; d.ldg = 32; d.x0 = fk; d.c0 = 32; d.w_dgrad = fk; d.dx = fk; d.lddx = 32; d.dw = (float*)fk; d.cin = 32; d.cout = 32;
    d.n = 0x7fffffff; d.h = 0x7ffffff8; d.w_ = 32; d.kh = d.kw = 3; d.dil = 1; d.dtype = SATCV_BF16;
    EXPECT(satcv_conv2d_bwd_fused_plan_info(&d, 256, &fi) != 0 && satcv_conv2d_bwd_fused_workspace(&d) < 0, "fused plan: extents beyond 2^31 pixels");
  }
  satcv_bnbwd_desc bd; memset(&bd, 0, sizeof(bd));
  EXPECT(satcv_bn_bwd_reduce(&bd, NULL) != 0 && satcv_bn_bwd_apply(&bd, NULL) != 0, "zeroed bn-backward desc");
  satcv_head_desc hd; memset(&hd, 0, sizeof(hd));
  EXPECT(satcv_head_fwd(&hd, NULL) != 0 && satcv_head_bwd(&hd, NULL) != 0, "zeroed head desc");
  satcv_reduce_job rj; memset(&rj, 0, sizeof(rj));
  EXPECT(satcv_reduce_job_items(NULL) < 0 && satcv_reduce_job_items(&rj) < 0, "invalid reduce job");
  EXPECT(satcv_reduce_slabs_batched(NULL, NULL, 0, 0, NULL) != 0, "empty batched reduce");
  EXPECT(satcv_conv2d_wgrad_reduce_job(&wd, &rj) != 0 && satcv_conv2d_bwd_fused_reduce_job(&fd, &rj) != 0, "reduce job of invalid descs");
  satcv_pack_job pj; memset(&pj, 0, sizeof(pj));
  (void)satcv_pack_job_items(&pj);
  EXPECT(satcv_pack_weights_batched(NULL, NULL, 0, 0, SATCV_BF16, NULL) != 0, "empty batched pack");

  /* ---- planning sweeps.  Pointers are fabricated (aligned, never dereferenced: dry runs and workspace queries only read the descriptor) */
  void* fake = (void*)(uintptr_t)0x7f0000001000ull;
  static const int HW[][2] = {{1, 1}, {4, 4}, {8, 8}, {12, 20}, {16, 16}, {20, 24}, {32, 32}, {40, 72}, {64, 64}, {100, 36}, {128, 128}, {256, 256}, {8, 264}, {512, 512}, {1024, 1024}};
  static const int CH[] = {16, 32, 48, 64, 96, 128, 192, 256, 512, 1024, 2048};
  static const int KD[][2] = {{1, 1}, {3, 1}, {3, 2}, {3, 3}, {3, 6}, {3, 12}, {3, 64}, {5, 1}, {7, 1}};
  long long planned = 0, accepted = 0, conv_plans = 0;
  for (unsigned hi = 0; hi < sizeof(HW) / sizeof(HW[0]); ++hi)
    for (unsigned ci = 0; ci < sizeof(CH) / sizeof(CH[0]); ++ci)
      for (unsigned co = 0; co < sizeof(CH) / sizeof(CH[0]); ++co)
        for (unsigned ki = 0; ki < sizeof(KD) / sizeof(KD[0]); ++ki)
          for (int n = 1; n <= 64; n *= 8)
            for (int dt = 0; dt <= 3; ++dt) {
              satcv_conv_desc d; memset(&d, 0, sizeof(d));
              d.x0 = fake; d.w = fake; d.y = fake; d.c0 = CH[ci]; d.ldy = CH[co]; d.n = n; d.h = HW[hi][0]; d.w_ = HW[hi][1];
              d.cout = CH[co]; d.cout_pad = (CH[co] + 63) / 64 * 64; d.kh = d.kw = KD[ki][0]; d.dil = KD[ki][1]; d.cstat = CH[co]; d.dtype = dt;
              d.stride = 1; d.f = 1;
              if (dt == 3 && (d.c0 % 64)) continue;
              accepted += satcv_conv2d_igemm_pipelined(&d);
              ++planned;
              /* the plan query walks the launch's own chain: an fp32 / bf16 descriptor always has a form (the generic kernel at the least) or an error
               * message, never a crash; what it reports stays inside the LDS */
              for (int ncu = 8; ncu <= 256; ncu *= 32) {
                satcv_conv_plan_info pi;
                (void)satcv_set_option("no_such_option", 1);        /* a known message in the error channel: a refusal must replace it */
                const int rc = satcv_conv2d_igemm_plan_info(&d, ncu, &pi);
                if (rc == 0) { EXPECT(pi.lds_bytes > 0 && pi.lds_bytes <= 160 * 1024 && pi.workgroups > 0 && pi.ksplit >= 1, "conv plan query geometry"); ++conv_plans; }
                else EXPECT(strlen(satcv_last_error()) > 0 && !strstr(satcv_last_error(), "no_such_option"), "a refused plan query says why: %s", satcv_last_error());
              }
              /* two-source input (decoder_block's concat) and a statistics target: other planning branches */
              d.x1 = fake; d.c1 = CH[ci]; d.stats = (satcv_stat_t*)fake; d.stats_ld = CH[co];
              if (!(dt == 3 && (d.c1 % 64))) {
                accepted += satcv_conv2d_igemm_pipelined(&d); ++planned;
                satcv_conv_plan_info pi;
                d.tile_policy = 2;
                if (satcv_conv2d_igemm_plan_info(&d, 256, &pi) == 0) { EXPECT(pi.lds_bytes <= 160 * 1024 && pi.workgroups > 0, "conv plan query geometry (two sources)"); ++conv_plans; }
                d.tile_policy = 0;
              }
              if (dt <= 1 && (KD[ki][0] == 1 || KD[ki][0] == 3)) {
                satcv_wgrad_desc w; memset(&w, 0, sizeof(w));
                w.x0 = fake; w.c0 = CH[ci]; w.dy = fake; w.lddy = CH[co]; w.dw = (float*)fake; w.cin = CH[ci]; w.cout = CH[co];
                w.n = n; w.h = HW[hi][0]; w.w_ = HW[hi][1]; w.kh = w.kw = KD[ki][0]; w.dil = KD[ki][1]; w.f = 1; w.dtype = dt;
                const int64_t nb = satcv_conv2d_wgrad_workspace(&w);
                EXPECT(nb != 0, "wgrad workspace 0 bytes");
                if (nb > 0 && w.c0 % 8 == 0) {        /* the plan query: null-free, host only, consistent with the workspace */
                  satcv_wgrad_plan_info pi;
                  EXPECT(satcv_conv2d_wgrad_plan_info(&w, &pi) == 0, "wgrad plan query: %s", satcv_last_error());
                  EXPECT(pi.ws_bytes == (int64_t)pi.nsplit * pi.ntaps * pi.kpad * pi.npad * 4 && pi.ws_bytes <= nb && pi.lds_bytes <= 160 * 1024,
                         "wgrad plan query geometry");
                }
                if (nb > 0) {
                  w.workspace = (float*)fake; w.workspace_bytes = nb;
                  satcv_reduce_job j;
                  if (satcv_conv2d_wgrad_reduce_job(&w, &j) == 0) {
                    EXPECT(j.nslab >= 1 && j.lanes >= 1 && j.lanes <= 16 && j.kpad >= w.cin && j.npad >= w.cout, "reduce job geometry");
                    EXPECT(satcv_reduce_job_items(&j) > 0, "reduce job items");
                  }
                }
                ++planned;
              }
            }
  EXPECT(conv_plans > 10000, "conv plan queries answered (%lld)", conv_plans);
  EXPECT(planned > 10000 && accepted > 1000, "planning sweep ran (%lld planned, %lld on the pipelined kernel)", planned, accepted);
  /* extreme extents: must be refused or planned without overflow */
  {
    satcv_conv_desc d; memset(&d, 0, sizeof(d));
    d.x0 = fake; d.w = fake; d.y = fake; d.c0 = 1 << 20; d.ldy = 1 << 20; d.n = 1 << 15; d.h = 1 << 15; d.w_ = 1 << 15; d.cout = 1 << 20; d.cout_pad = 1 << 20;
    d.kh = d.kw = 3; d.dil = 1; d.cstat = 1 << 20; d.dtype = SATCV_BF16; d.stride = 1; d.f = 1;
    (void)satcv_conv2d_igemm_pipelined(&d);
    d.n = 0x7fffffff; d.h = 0x7fffffff; d.w_ = 0x7fffffff;
    (void)satcv_conv2d_igemm_pipelined(&d);
  }
  printf("host ABI driver: %lld plans, %lld accepted by the pipelined kernel, %d failures\n", planned, accepted, fails);
  return fails ? 1 : 0;
}
