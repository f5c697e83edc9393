// Every runtime switch of the library: one row per switch, and nothing else declares or parses one.
//
//   X(key, environment variable, default, reader, kind, meaning)
//
// key      field of `g_opt` and the name satcv_get_option / satcv_set_option / satcv_option_key know it by
// reader   how the variable's text becomes the value (below); a clamp lives here and nowhere else
// kind     SETTABLE  satcv_set_option changes it at run time (tests and probes A/B variants in one process)
//          STARTUP   read-only after load: satcv_set_option refuses it.  Several of these size workspaces or answers that plans cache
//                    (ew_per_cu -> satcv_bias_grad_workspace; wgrad_wgs / wgrad_dma / wgrad_pix256 -> the slab counts of
//                    satcv_conv2d_wgrad_workspace and the reduce jobs), so a change behind a built plan could overrun a buffer
//          COUNTER   launches a path has served in this process (tests assert "path taken"); no variable, read-only
//
// Every variable is read ONCE, when the library is loaded (api.hip defines `g_opt` from this table).  The STARTUP rows used to be read
// at the first use of their call site instead; every test and tool sets the environment before it starts the process, so nothing
// observable moved.  include/satcv.h (above satcv_set_option) and DESIGN.md ("Switches") list the same rows for readers without
// this file; tests/test_host_cpu.py holds the three together and pins every default.
#pragma once
#include <cstdlib>

static inline int opt_int(const char* e, int dflt) { return e ? atoi(e) : dflt; }
// a value below LO reads as the default
template <int LO> static inline int opt_int_from(const char* e, int dflt) { const int v = opt_int(e, dflt); return v >= LO ? v : dflt; }
// a word, of which the first letter decides: SATCV_IGEMM=generic
static inline int opt_starts_with_g(const char* e, int) { return e && e[0] == 'g'; }

#define SATCV_OPTIONS(X) \
  /* ---- conv_igemm_fast.hip: tile choice of the implicit-GEMM convolutions */ \
  X(igemm_db, "SATCV_DB", 1, opt_int, SETTABLE, "0 the single-buffered 128x128 tile (and 32-channel chunks for deep 1x1) only, 1 automatic, 2 the double-buffered 256x128 tile wherever its shape limits allow (profiles/r03_db_vs_single.txt)") \
  X(igemm_sched, "SATCV_IGEMM_SCHED", 0, opt_int, SETTABLE, "experiment bits handed to the deep tile (DESIGN.md section 3: half-chunk stagger, no gain); none wired at present") \
  X(igemm_thin, "SATCV_THIN", 1, opt_int, SETTABLE, "persistent weights-stationary kernel of the thin 3x3 layers (conv_igemm_ws.hip, conv_thin_roles.hip): 0 off, 1 / 2 on wherever the shape limits allow, whatever the batch size") \
  X(igemm_m16, "SATCV_M16", 1, opt_int, SETTABLE, "the 16x16x32 deep 3x3 tiles (conv_igemm_m16.hip, conv_igemm_m16p.hip): 0 off, 1 launches that write statistics (training), 2 every eligible launch; a training plan's tile_policy raises 1 to 2 (profiles/r05_ab_m16_step.txt)") \
  X(splitk, "SATCV_SPLITK", 0, opt_int, SETTABLE, "split-K of under-filled plain (halo-tile / 1x1) launches, opt-in because the K order then depends on the workgroup count: 1 every eligible launch, 2 launches of fewer than 64 workgroups (the DeepLab inference plans; profiles/r04_ab_splitk.txt)") \
  X(splitk_tl, "SATCV_SPLITK_TL", 1, opt_int, STARTUP, "split-K of under-filled tap-loop launches (dilated / strided convolutions); 0 off") \
  X(convt_wide, "SATCV_CONVT_WIDE", 1, opt_int, STARTUP, "transposed-conv tiles span several sub-pixel positions (input read once, whole-line stores); 0 one position per tile") \
  X(wdma, "SATCV_WDMA", 1, opt_int, STARTUP, "deep 3x3 tile: weights by LDS-DMA into a three-slot ring (profiles/r04_ab_weight_ring_dma.txt); 0 register-staged weights") \
  X(db64, "SATCV_DB64", 1, opt_int, STARTUP, "512-pixel x 64-channel double-buffered tile for 64 output channels with deep K (profiles/r03_ab_late_switches.txt): 0 off, 2 also other multiples of 64, 3 also below 128 input channels") \
  X(db_tl, "SATCV_DB_TL", 1, opt_int, STARTUP, "double-buffered 256x128 tap-loop tile with 64-channel chunks (profiles/r04_deeplab_ab_double_buffered_taploop.txt): 0 off, 1 from 96 tiles on, n > 1 from n tiles on") \
  X(db1x1, "SATCV_DB1X1", 1, opt_int, STARTUP, "deep 1x1 / transposed convolutions on the double-buffered 256x128 tile (profiles/r03_ab_late_switches.txt); 0 the single-buffered tile") \
  X(db1x1_small, "SATCV_DB1X1_SMALL", 1, opt_int, STARTUP, "... also where even 128-pixel tiles leave CUs idle (profiles/r04_deeplab_ab_db1x1_small.txt); 0 off") \
  X(igemm_generic, "SATCV_IGEMM", 0, opt_starts_with_g, STARTUP, "SATCV_IGEMM=generic: every convolution on the generic kernel of conv_igemm.hip (ablation; the value is 1 when the word starts with g)") \
  /* ---- conv_igemm_m16.hip, conv_igemm_m16p.hip, conv_thin_roles.hip */ \
  X(m16_ws, "SATCV_M16_WS", 1, opt_int, STARTUP, "wave roles in the one-tile 16x16x32 kernel: 0 never (symmetric kernel), 1 from 256 input channels on, 2 always (profiles/r05_ablation_m16.txt)") \
  X(m16p, "SATCV_M16P", 1, opt_int, SETTABLE, "persistent 16x16x32 kernel: 0 off, 1 where a workgroup gets at least two tiles, 2 every eligible launch (profiles/r06_ab_m16p_step.txt)") \
  X(m16p_prio, "SATCV_M16P_PRIO", 30, opt_int, SETTABLE, "s_setprio of its staging waves, decimal digits (plain launches)(launches with the fused input BatchNorm)(launches with the fused BatchNorm-backward sums), each 0 ... 3 (30: profiles/r06_ab_m16p_prio_step.txt)") \
  X(m16p_prio64, "SATCV_M16P_PRIO64", -1, opt_int, STARTUP, "the same digits for its 64-channel output block; negative: as m16p_prio") \
  X(m16p_bn64, "SATCV_M16P_BN64", 1, opt_int, STARTUP, "its 64-channel output block (profiles/r06_ab_m16p_bn64_step.txt); 0 the 64-filter layers stay on the one-tile kernels") \
  X(thin_roles, "SATCV_THIN_ROLES", 1, opt_int, SETTABLE, "wave-role kernel of the thin 3x3 layers: 0 off, 1 the shapes it measured faster on, 2 every shape it serves (profiles/r05_ab_thin_roles_step.txt)") \
  /* ---- conv_transpose_thin.hip */ \
  X(convt_thin, "SATCV_CONVT_THIN", 1, opt_int, STARTUP, "streaming kernels of the thin transposed convolutions and their data gradient (profiles/r03_ab_convt_thin.txt): 0 off (tiled kernels), non-zero on, >= 2 also the 64 <- 4 x 32 data gradient, where the tiled kernel measured faster") \
  X(convt_wps, "SATCV_CONVT_WPS", 3, opt_int, STARTUP, "waves per SIMD of the 64 -> 4 x 32 forward: 2, anything else 3") \
  X(convt_mid, "SATCV_CONVT_MID", 1, opt_int, STARTUP, "256 -> 4 x 128 on the streaming kernel, one position per workgroup; 0 the tiled kernel") \
  /* ---- conv_wgrad.hip */ \
  X(wgrad_db, "SATCV_WGRAD_DB", 1, opt_int, SETTABLE, "double-buffered weight-gradient kernel where its limits allow: 0 the single-buffered one, 2 the 64x128 block for 1x1 / transposed-conv gradients instead of 128x256") \
  X(wgrad_m16, "SATCV_WGRAD_M16", 0, opt_int, SETTABLE, "wgrad_dma_kernel on v_mfma_f32_16x16x32_bf16: measured slower, off (profiles/r06_ab_wgrad_m16.txt)") \
  X(wgrad_pix256, "SATCV_WGRAD_PIX256", 1, opt_int, STARTUP, "thin layers stage 256 pixels per step; 0 always 128") \
  X(wgrad_dma, "SATCV_WGRAD_DMA", 1, opt_int, STARTUP, "deep 3x3 layers: the 64x128 block with dY by LDS-DMA (profiles/r04_ab_wgrad_dma.txt); 0 the 32x128 block") \
  X(wgrad_wgs, "SATCV_WGRAD_WGS", 128, opt_int_from<8>, STARTUP, "workgroups of a double-buffered weight-gradient launch that shares the chip (profiles/r04_ab_wgrad_workgroups.txt); below 8 reads as 128") \
  /* ---- elementwise.hip, scene.hip */ \
  X(ew_per_cu, "SATCV_EW_PER_CU", 6, opt_int_from<1>, STARTUP, "workgroups per CU of the grid-stride elementwise kernels (3 ... 16 within 0.3 % of the step, elementwise.hip); below 1 reads as 6") \
  X(bn_apply, "SATCV_BN_APPLY", 1, opt_int, STARTUP, "BatchNorm-backward apply on its own kernel; 0 the round-3 loop for every apply launch (a null in the step: profiles/r06_ab_env_switches.txt)") \
  X(bn_rev, "SATCV_BN_REV", 1, opt_int, STARTUP, "BatchNorm-backward apply walks the pixels in reversed order; 0 forward (ablation of a single kernel choice, DESIGN.md section 6)") \
  X(loss_fast, "SATCV_LOSS_FAST", 1, opt_int, STARTUP, "vectorised softmax cross-entropy kernel for 2 / 4 classes; 0 the general loss kernel") \
  /* ---- "path taken" counters */ \
  X(igemm_thin_launches, nullptr, 0, opt_int, COUNTER, "launches served by the persistent thin-layer kernels (conv_igemm_ws.hip and conv_thin_roles.hip)") \
  X(thin_roles_launches, nullptr, 0, opt_int, COUNTER, "... of them by conv_thin_roles.hip") \
  X(m16p_launches, nullptr, 0, opt_int, COUNTER, "launches served by conv_igemm_m16p.hip")

struct satcv_options {
#define X(key, env, dflt, reader, kind, meaning) int key;
  SATCV_OPTIONS(X)
#undef X
};
extern satcv_options g_opt;      // api.hip

// cap of an elementwise grid: ew_per_cu workgroups on each of the 256 CUs
static inline int ew_grid_cap() { return 256 * g_opt.ew_per_cu; }
