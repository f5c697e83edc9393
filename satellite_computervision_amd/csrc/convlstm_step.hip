// One ConvLSTM2D inference step in ONE launch (utils/model_tools.py:685-720): the recurrent 3x3 convolution of h_{t-1} on MFMA with the
// gate arithmetic of convlstm_gates_fwd_kernel (convlstm.hip) as its epilogue.  The pair of launches it replaces writes the convolution
// result hg (npix x 4 F, storage type) to HBM and reads it back; here the pre-activations never leave the accumulators:
//
//   z   = xg + conv3x3_same(h_prev, recurrent_kernel)        xg seeds the fp32 accumulators, the K loop adds the convolution
//   i, f, g, o = ra(z_i), ra(z_f), act(z_c), ra(z_o);   c_t = f c_prev + i g  (float32);   h_t = o act(c_t)  (storage type)
//
// Gate-interleaved channel order (satcv.h, lstm_infer.gate_order).  A lane of v_mfma_f32_32x32x16 owns ONE column (lane & 31) of every
// 32-wide N tile, so the four pre-activations of a filter meet in one lane when they sit 32 columns apart: the 4 F output channels of the
// recurrent kernel, of the input kernel and of the bias are permuted on the host, before packing, to
//   position  blk * 4 G + gate * G + j   <-   natural channel  gate * F + blk * G + j          G = min(F, 32), blk < F / G, j < G
// F >= 32: a wave owns one block of 128 columns = 4 N tiles = the gates i, f, g, o of 32 filters.  F = 16 (G = 16): the 64 columns are
// two N tiles, columns (i | f) and (g | o); the lane halves (lane & 16) hold (i, g) and (f, o) of filter lane & 15 and exchange the two
// products of c_t with one cross-lane move.  c and h stay in natural channel order.
//
// Workgroup: 4 waves, a 16 x 8 pixel patch of one image and ALL 4 F output channels; the h_prev halo tile (18 x 10 pixels x F, zero outside
// the image -- a tile never spans two images) is staged in LDS once, [F/8][10][pitch][8] as in conv_igemm.hip; K = 9 F.  The weights
// (ops.pack_weights forward image of the permuted kernel, [tap][F/8][4 F][8]) stream per tap and k-step from L2 straight into the B
// fragments, one step ahead of the MFMAs.  float32 storage runs the same code on 8 x v_mfma_f32_32x32x2f32 per fragment (not tuned).
#include "igemm_common.hpp"

namespace {

constexpr int STEP_TW = 16, STEP_TH = 8, STEP_BM = STEP_TW * STEP_TH, STEP_THREADS = 256;

__device__ __forceinline__ float step_rec_act(float z, int kind) {
  return kind == 0 ? fminf(fmaxf(0.2f * z + 0.5f, 0.f), 1.f) : 1.f / (1.f + expf(-z));
}
__device__ __forceinline__ float step_act(float z, int kind) { return kind ? tanhf(z) : z; }

template <typename T, int F>
__global__ __launch_bounds__(STEP_THREADS) void convlstm_step_kernel(const satcv_lstm_step_desc d, const int tiles_x, const int tiles_y) {
  constexpr int G = F >= 32 ? 32 : 16;
  constexpr int NT = 4 * G / 32;                       // N tiles of a wave: 4 (one gate each) or 2 (two gates each)
  constexpr int WN = F / G, WM = 4 / WN, MT = STEP_BM / (WM * 32);
  constexpr int SLOTS = F / 8, KS = F / 16, C4 = 4 * F;
  constexpr int RL = STEP_TH + 2, CL = STEP_TW + 2;
  constexpr int PITCH = sizeof(T) == 2 ? igemm_pitch(STEP_TW, CL, false) : CL;
  constexpr int SLOT_STRIDE = RL * PITCH * 8;
  static_assert(WM * MT * 32 == STEP_BM && WM * WN * 64 == STEP_THREADS, "tile");
  __shared__ __attribute__((aligned(16))) T ldsA[SLOTS * SLOT_STRIDE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int r = lane & 31, hh = lane >> 5;
  int bid = blockIdx.x;
  const int tx = bid % tiles_x; bid /= tiles_x;
  const int ty = bid % tiles_y;
  const int n = bid / tiles_y;
  const int y0 = ty * STEP_TH, x0 = tx * STEP_TW;
  const long long img0 = (long long)n * d.h * d.w_;
  const int colbase = wn * 4 * G;

  // pixel of accumulator register i of M tile m (AccMap<false>): false outside the image
  auto pixel_of = [&](int m, int i, long long& p) {
    const int q = (wm * MT + m) * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
    const int y = y0 + q / STEP_TW, x = x0 + q % STEP_TW;
    p = img0 + (long long)y * d.w_ + x;
    return y < d.h && x < d.w_;
  };

  // ---- the accumulators start as xg (bias inside), so that z = xg + conv is summed in fp32 and these loads fly during the K loop
  const T* xg = reinterpret_cast<const T*>(d.xg);
  f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      long long p;
      const bool ok = pixel_of(m, i, p);
#pragma unroll
      for (int nn = 0; nn < NT; ++nn) acc[m][nn][i] = ok ? (float)xg[p * d.ldx + colbase + nn * 32 + r] : 0.f;
    }

  if (d.h_prev) {
    // ---- stage the halo tile of h_prev (zero outside the image)
    const T* hp = reinterpret_cast<const T*>(d.h_prev);
    for (int it = tid; it < RL * CL * SLOTS; it += STEP_THREADS) {
      const int slot = it % SLOTS, pix = it / SLOTS;
      const int c = pix % CL, L = pix / CL;
      const int y = y0 - 1 + L, x = x0 - 1 + c;
      Raw8<T> v = zero8<T>();
      if (y >= 0 && y < d.h && x >= 0 && x < d.w_) v = gload8<T>(hp + (img0 + (long long)y * d.w_ + x) * d.ldh_prev + slot * 8);
      lstore8<T>(ldsA + (slot * RL + L) * PITCH * 8 + c * 8, v);
    }
    __syncthreads();
    int a_off[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int q = (wm * MT + m) * 32 + r;
      a_off[m] = ((q / STEP_TW) * PITCH + q % STEP_TW) * 8;
    }
    const T* wp = reinterpret_cast<const T*>(d.w) + (size_t)(colbase + r) * 8;
    auto load_b = [&](FragT<T> (&b)[NT], int ks) {      // k-step ks = tap * KS + s: slot (ks / KS) * SLOTS + (ks % KS) * 2 + hh of the image
      const int run = (ks / KS) * SLOTS + (ks % KS) * 2 + hh;
#pragma unroll
      for (int nn = 0; nn < NT; ++nn) b[nn] = lds_frag<T>(wp + ((size_t)run * C4 + nn * 32) * 8);
    };
    FragT<T> cur[NT], nxt[NT];
    load_b(cur, 0);
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx) {
        const int tap = ky * 3 + kx, tap_off = (ky * PITCH + kx) * 8;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int ks = tap * KS + s;
          load_b(nxt, ks + 1 < 9 * KS ? ks + 1 : ks);
          FragT<T> af[MT];
#pragma unroll
          for (int m = 0; m < MT; ++m) af[m] = lds_frag<T>(ldsA + (s * 2 + hh) * SLOT_STRIDE + a_off[m] + tap_off);
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int nn = 0; nn < NT; ++nn) mma32<T>(acc[m][nn], af[m], cur[nn]);
#pragma unroll
          for (int nn = 0; nn < NT; ++nn) cur[nn] = nxt[nn];
        }
      }
  }

  // ---- gates (the arithmetic of convlstm_gates_fwd_kernel), c_t and h_t in natural channel order
  T* hout = reinterpret_cast<T*>(d.h_out);
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      long long p;
      const bool ok = pixel_of(m, i, p);
      if constexpr (G == 32) {
        if (ok) {
          const int ch = wn * 32 + r;
          const float cp = d.c_prev ? d.c_prev[p * F + ch] : 0.f;
          const float gi = step_rec_act(acc[m][0][i], d.rec_act), gf = step_rec_act(acc[m][1][i], d.rec_act);
          const float gg = step_act(acc[m][2][i], d.act), go = step_rec_act(acc[m][3][i], d.rec_act);
          const float cn = gf * cp + gi * gg;
          d.c_out[p * F + ch] = cn;
          hout[p * d.ldh + ch] = (T)(go * step_act(cn, d.act));
        }
      } else {
        // lanes r < 16 hold (i, g) of filter r, lanes r >= 16 (f, o) of filter r - 16: each forms one product of c_t
        const int j = r & 15, up = r >> 4;
        const float a = step_rec_act(acc[m][0][i], d.rec_act);
        const float b = up ? step_rec_act(acc[m][1][i], d.rec_act) : step_act(acc[m][1][i], d.act);
        const float cp = (up && ok && d.c_prev) ? d.c_prev[p * F + j] : 0.f;
        const float part = up ? a * cp : a * b;
        const float cn = part + __shfl_xor(part, 16, 64);
        if (ok) {
          if (up) hout[p * d.ldh + j] = (T)(b * step_act(cn, d.act));
          else d.c_out[p * F + j] = cn;
        }
      }
    }
}

template <typename T, int F>
int step_launch(const satcv_lstm_step_desc& d, hipStream_t st) {
  const int tiles_x = cdiv(d.w_, STEP_TW), tiles_y = cdiv(d.h, STEP_TH);
  const long long blocks = (long long)d.n * tiles_x * tiles_y;
  if (blocks <= 0 || blocks > 0x7fffffffLL) { satcv_set_error("convlstm_step_fwd: bad grid %lld", blocks); return SATCV_ERR_INVALID; }
  hipLaunchKernelGGL((convlstm_step_kernel<T, F>), dim3((unsigned)blocks), dim3(STEP_THREADS), 0, st, d, tiles_x, tiles_y);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { satcv_set_error("convlstm_step_fwd launch: %s", hipGetErrorString(e)); return SATCV_ERR_HIP; }
  return SATCV_OK;
}

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" int satcv_convlstm_step_supported(int32_t filters, int32_t dtype) {
  return ((filters == 16 || filters == 32 || filters == 64) && (dtype == SATCV_F32 || dtype == SATCV_BF16)) ? 1 : 0;
}

extern "C" int satcv_convlstm_step_fwd(const satcv_lstm_step_desc* d, void* stream) {
  SATCV_CHECK(d && d->xg && d->c_out && d->h_out, "convlstm_step_fwd: null pointer");
  SATCV_CHECK(d->dtype == SATCV_F32 || d->dtype == SATCV_BF16, "convlstm_step_fwd: bad dtype %d", d->dtype);
  SATCV_CHECK(satcv_convlstm_step_supported(d->filters, d->dtype), "convlstm_step_fwd: filters must be 16, 32 or 64 (got %d)", d->filters);
  SATCV_CHECK(satcv_pixels_ok(d->n, d->h, d->w_, 1), "convlstm_step_fwd: bad image grid %d x %d x %d", d->n, d->h, d->w_);
  SATCV_CHECK(d->rec_act >= 0 && d->rec_act <= 1 && d->act >= 0 && d->act <= 1, "convlstm_step_fwd: rec_act / act must be 0 or 1");
  const int F = d->filters;
  const size_t es = d->dtype == SATCV_BF16 ? 2 : 4, npix = (size_t)d->n * d->h * d->w_;
  SATCV_CHECK(d->ldx >= 4 * F && d->ldx % 8 == 0 && d->ldh >= F && d->ldh % 8 == 0, "convlstm_step_fwd: bad leading dimensions (ldx %d, ldh %d)", d->ldx, d->ldh);
  if (d->h_prev) {
    SATCV_CHECK(d->w, "convlstm_step_fwd: h_prev without weights");
    SATCV_CHECK(d->ldh_prev >= F && d->ldh_prev % 8 == 0, "convlstm_step_fwd: bad leading dimension ldh_prev %d", d->ldh_prev);
    SATCV_CHECK((uintptr_t)d->h_prev % 16 == 0 && (uintptr_t)d->w % 16 == 0, "convlstm_step_fwd: h_prev and w must be 16-byte aligned");
    SATCV_CHECK(!ranges_overlap(d->h_prev, npix * d->ldh_prev * es, d->h_out, npix * d->ldh * es), "convlstm_step_fwd: h_out aliases h_prev");
  }
  SATCV_CHECK(!d->c_prev || !ranges_overlap(d->c_prev, npix * F * 4, d->c_out, npix * F * 4), "convlstm_step_fwd: c_out aliases c_prev");
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == SATCV_BF16) {
    if (F == 16) return step_launch<bf16, 16>(*d, st);
    if (F == 32) return step_launch<bf16, 32>(*d, st);
    return step_launch<bf16, 64>(*d, st);
  }
  if (F == 16) return step_launch<float, 16>(*d, st);
  if (F == 32) return step_launch<float, 32>(*d, st);
  return step_launch<float, 64>(*d, st);
}
