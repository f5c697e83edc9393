// Device-side TFRecord training pipeline: what to_tuple of the reference (utils/processing.py:335-392) does per
// record on the host -- aug_tensor_color (:129-152), rescale_tensor (:281-322) or normalize_tensor (:225-279), tf.one_hot of the
// categorical features and the response, aug_tensor_morph of the concatenated stack (:169-183), labels > 1 -> 1 -- for one BATCH of
// parsed records, with per-record parameters read from a device table.
//   satcv_record_stats     per (sample, continuous plane) mean / min / max / population variance over (h, w): double sums of the fp32
//                          samples in a fixed order (several workgroups per plane write partials, a second kernel adds them in order)
//   satcv_record_to_tuple  the fused transform.  One workgroup per (sample, T x T output tile): the source tile of every plane is read
//                          row by row (coalesced along x whatever the rotation) into an LDS tile padded by one float per row, then every
//                          thread takes whole output pixels, reads its planes from LDS (for odd rotations down a column: the pad keeps
//                          that free of bank conflicts) and writes the channels of the pixel, which are contiguous in NHWC, together.
// The colour and rescale expressions are separate correctly rounded fp32 operations in NumPy's order (no contraction into FMA), so all
// results that do not depend on a mean are bit-identical to the host path.
#include "common.hpp"

namespace {

constexpr int kStatThreads = 256;

// number of workgroups that share one plane: a function of the plane size ONLY, so that the summation order -- and with it every
// bit of the mean -- does not depend on how many samples share the batch
__host__ __device__ inline int stat_splits(int hw) {
  int s = hw / 4096;
  return s < 1 ? 1 : (s > SATCV_RECORD_STAT_SPLITS ? SATCV_RECORD_STAT_SPLITS : s);
}

// partial (sum, sum of squares) about the plane's first sample (a shift removes the cancellation of E[x^2] - E[x]^2), min, max
__global__ void record_stats_partial_kernel(const satcv_record_desc d, int splits) {
  const int plane = blockIdx.x / splits, part = blockIdx.x % splits;
  if (d.kind[plane % d.k] != SATCV_PLANE_BAND) return;
  const int hw = d.h * d.w_;
  const float* p = d.src + (size_t)plane * hw;
  const int chunk = (hw + splits - 1) / splits;
  const int lo = part * chunk, hi = min(hw, lo + chunk);
  const double shift = (double)p[0];
  double s = 0.0, q = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = lo + threadIdx.x; i < hi; i += kStatThreads) {
    const float v = p[i];
    const double t = (double)v - shift;
    s += t; q += t * t;
    mn = fminf(mn, v); mx = fmaxf(mx, v);             // NaNs are skipped, as np.nanmin / tf.reduce_min of finite tiles
  }
  __shared__ double ss[kStatThreads], sq[kStatThreads];
  __shared__ float smn[kStatThreads], smx[kStatThreads];
  ss[threadIdx.x] = s; sq[threadIdx.x] = q; smn[threadIdx.x] = mn; smx[threadIdx.x] = mx;
  __syncthreads();
  for (int o = kStatThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      ss[threadIdx.x] += ss[threadIdx.x + o]; sq[threadIdx.x] += sq[threadIdx.x + o];
      smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + o]); smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* o = d.stats_ws + ((size_t)plane * splits + part) * 4;
    o[0] = ss[0]; o[1] = sq[0]; o[2] = (double)smn[0]; o[3] = (double)smx[0];
  }
}

__global__ void record_stats_finalize_kernel(const satcv_record_desc d, int splits) {
  const int plane = blockIdx.x * blockDim.x + threadIdx.x;
  if (plane >= d.n * d.k || d.kind[plane % d.k] != SATCV_PLANE_BAND) return;
  const int hw = d.h * d.w_;
  const double* w = d.stats_ws + (size_t)plane * splits * 4;
  double s = 0.0, q = 0.0, mn = w[2], mx = w[3];
  for (int i = 0; i < splits; ++i) { s += w[4 * i]; q += w[4 * i + 1]; mn = fmin(mn, w[4 * i + 2]); mx = fmax(mx, w[4 * i + 3]); }
  const double ms = s / hw;
  double var = q / hw - ms * ms;
  double* o = d.stats + (size_t)plane * 4;
  o[0] = (double)d.src[(size_t)plane * hw] + ms; o[1] = mn; o[2] = mx; o[3] = var < 0.0 ? 0.0 : var;
}

// inverse of aug_tensor_morph: output pixel (yo, xo) of flip_lr -> flip_ud -> np.rot90(k) <- source (y, x); square tiles when k is odd
__device__ __forceinline__ void morph_src(int yo, int xo, int h, int w, int flr, int fud, int rot, int& y, int& x) {
  int a, b;
  switch (rot & 3) {
    case 0: a = yo; b = xo; break;
    case 1: a = xo; b = w - 1 - yo; break;           // np.rot90(m)[i][j] = m[j][W-1-i]
    case 2: a = h - 1 - yo; b = w - 1 - xo; break;
    default: a = h - 1 - xo; b = yo; break;          // np.rot90(m, 3)[i][j] = m[H-1-j][i]
  }
  y = fud ? h - 1 - a : a;
  x = flr ? w - 1 - b : b;
}

// per continuous channel, per sample: v -> ((v - m) * contra + m * bright  [colour]  - lo) / den
struct ChanCoef { float m, contra, bright, lo, den; };

#pragma clang fp contract(off)
__device__ __forceinline__ float colour(float v, const ChanCoef& c) {
  const float t1 = (v - c.m) * c.contra;
  const float t2 = c.m * c.bright;
  return t1 + t2;
}

#pragma clang fp contract(off)
template <int T>
__global__ void __launch_bounds__(256) record_to_tuple_kernel(const satcv_record_desc d, int nband, int npass) {
  extern __shared__ float lds[];
  constexpr int TP = T + 1;
  __shared__ ChanCoef coef[SATCV_RECORD_MAX_PLANES];
  __shared__ int band_plane[SATCV_RECORD_MAX_PLANES];      // continuous channel -> plane
  const int tiles_x = (d.w_ + T - 1) / T, tiles_y = (d.h + T - 1) / T;
  const int b = blockIdx.x / (tiles_x * tiles_y);
  const int tile = blockIdx.x % (tiles_x * tiles_y);
  const int oy0 = (tile / tiles_x) * T, ox0 = (tile % tiles_x) * T;
  const int th = min(T, d.h - oy0), tw = min(T, d.w_ - ox0);
  const int hw = d.h * d.w_;

  int flr = 0, fud = 0, rot = 0;
  const float* prm = d.params ? d.params + (size_t)b * d.ld_params : nullptr;
  if (d.morph) {
    flr = prm[2 * nband] != 0.f; fud = prm[2 * nband + 1] != 0.f; rot = ((int)prm[2 * nband + 2]) & 3;
  }

  // ---- per-channel coefficients of this sample (one thread each; double where a mean or a variance is involved)
  if (threadIdx.x == 0) {
    int c = 0;
    for (int j = 0; j < d.k; ++j) if (d.kind[j] == SATCV_PLANE_BAND) band_plane[c++] = j;
  }
  __syncthreads();
  if ((int)threadIdx.x < nband) {
    const int c = threadIdx.x;
    const double* st = d.stats ? d.stats + ((size_t)b * d.k + band_plane[c]) * 4 : nullptr;
    ChanCoef k;
    k.m = 0.f; k.contra = 1.f; k.bright = 1.f; k.lo = 0.f; k.den = 1.f;
    if (d.color) {
      k.m = d.mean_in ? d.mean_in[(size_t)b * nband + c] : (float)st[0];
      k.contra = prm[c]; k.bright = prm[nband + c];
    }
    coef[c] = k;
  }
  __syncthreads();
  if ((int)threadIdx.x < nband && d.mode != SATCV_RECORD_NONE && d.stat_src != SATCV_STAT_PIXEL) {
    const int c = threadIdx.x;
    int g = -1;
    for (int i = 0; i < d.ngroups; ++i) if (c >= d.gstart[i] && c < d.gstart[i] + d.glen[i]) g = i;
    float lo = 0.f, den = 1.f;
    if (g >= 0) {
      if (d.stat_src == SATCV_STAT_MOMENTS) {
        if (d.mode == SATCV_RECORD_RESCALE) { lo = d.mom_a[c]; den = (d.mom_b[c] - d.mom_a[c]) + d.eps; }
        else { lo = d.mom_a[c]; den = __fsqrt_rn(d.mom_b[c] + d.eps); }
      } else {
        const int c0 = d.stat_src == SATCV_STAT_GROUP ? d.gstart[g] : c, c1 = d.stat_src == SATCV_STAT_GROUP ? d.gstart[g] + d.glen[g] : c + 1;
        if (d.mode == SATCV_RECORD_RESCALE) {
          // the colour map is monotone (contra > 0): its fp32 image of the raw min / max IS the min / max of the coloured plane
          float mn = INFINITY, mx = -INFINITY;
          for (int e = c0; e < c1; ++e) {
            const double* se = d.stats + ((size_t)b * d.k + band_plane[e]) * 4;
            float a = (float)se[1], z = (float)se[2];
            if (d.color) { a = colour(a, coef[e]); z = colour(z, coef[e]); }
            mn = fminf(mn, fminf(a, z)); mx = fmaxf(mx, fmaxf(a, z));
          }
          lo = mn; den = (mx - mn) + d.eps;
        } else {
          // mean' = (mean - m) contra + m bright, var' = contra^2 var per channel; a group pools E[x] and E[x^2] of its channels
          auto moments = [&](int e, double& mu, double& var) {
            const double* se = d.stats + ((size_t)b * d.k + band_plane[e]) * 4;
            mu = se[0]; var = se[3];
            if (d.color) {
              const double m = (double)coef[e].m, ct = (double)coef[e].contra, br = (double)coef[e].bright;
              mu = (mu - m) * ct + m * br; var = ct * ct * var;
            }
          };
          double s1 = 0.0, s2 = 0.0, mu_e, var_e;
          for (int e = c0; e < c1; ++e) { moments(e, mu_e, var_e); s1 += mu_e; }
          const double mu = s1 / (c1 - c0);
          for (int e = c0; e < c1; ++e) { moments(e, mu_e, var_e); s2 += var_e + (mu_e - mu) * (mu_e - mu); }
          const double var = s2 / (c1 - c0);
          lo = (float)mu; den = __fsqrt_rn((float)var + d.eps);
        }
      }
    }
    coef[c].lo = lo; coef[c].den = den;
  }

  // ---- source tile of every plane -> LDS, rows of the SOURCE (coalesced whatever the rotation)
  int y0, x0, y1, x1;
  morph_src(oy0, ox0, d.h, d.w_, flr, fud, rot, y0, x0);
  morph_src(oy0 + th - 1, ox0 + tw - 1, d.h, d.w_, flr, fud, rot, y1, x1);
  const int sy0 = max(0, min(y0, y1)), sx0 = max(0, min(x0, x1));
  const int sh = (rot & 1) ? tw : th, sw = (rot & 1) ? th : tw;
  const float* base = d.src + (size_t)b * d.k * hw;
  for (int j = 0; j < d.k; ++j) {
    const float* p = base + (size_t)j * hw;
    float* l = lds + j * T * TP;
    for (int i = threadIdx.x; i < T * T; i += 256) {
      const int r = i / T, c = i % T;
      const int y = sy0 + r, x = sx0 + c;
      if (r < sh && c < sw && y < d.h && x < d.w_) l[r * TP + c] = p[(size_t)y * d.w_ + x];
    }
  }
  __syncthreads();

  // ---- one output pixel per thread and pass: all channels of the pixel
  for (int i = threadIdx.x; i < T * T; i += 256) {
    const int ty = i / T, tx = i % T;
    if (ty >= th || tx >= tw) continue;
    int y, x;
    morph_src(oy0 + ty, ox0 + tx, d.h, d.w_, flr, fud, rot, y, x);
    const int r = y - sy0, c = x - sx0;           // inside the tile for every table: rot is masked to 0..3, the flips are booleans
    const float* l = lds + r * TP + c;
    const size_t pix = ((size_t)b * d.h + oy0 + ty) * d.w_ + ox0 + tx;
    float* ox = d.x + pix * d.ld_x + d.coff_x;
    float* oy = d.y ? d.y + pix * d.ld_y + d.coff_y : nullptr;

    // continuous bands
    if (d.mode != SATCV_RECORD_NONE && d.stat_src == SATCV_STAT_PIXEL) {
      // statistics over the channels of a group, per pixel: the coloured values are recomputed from LDS rather than kept in an
      // indexed register array.  Channels outside every group (normalize_tensor's remainder) pass through
      auto val = [&](int ch) { const float v = l[band_plane[ch] * T * TP]; return d.color ? colour(v, coef[ch]) : v; };
      int done = 0;
      for (int g = 0; g < d.ngroups; ++g) {
        const int c0 = d.gstart[g], c1 = c0 + d.glen[g];
        for (int ch = done; ch < c0; ++ch) ox[ch] = val(ch);
        float lo, den;
        if (d.mode == SATCV_RECORD_RESCALE) {
          float mn = INFINITY, mx = -INFINITY;
          for (int ch = c0; ch < c1; ++ch) { const float v = val(ch); mn = fminf(mn, v); mx = fmaxf(mx, v); }
          lo = mn; den = (mx - mn) + d.eps;
        } else {
          // np.mean / np.var over a short contiguous axis: sequential fp32 sums
          float s = 0.f;
          for (int ch = c0; ch < c1; ++ch) s = s + val(ch);
          const float mu = s / (float)(c1 - c0);
          float q = 0.f;
          for (int ch = c0; ch < c1; ++ch) { const float t = val(ch) - mu; q = q + t * t; }
          lo = mu; den = __fsqrt_rn(q / (float)(c1 - c0) + d.eps);
        }
        for (int ch = c0; ch < c1; ++ch) ox[ch] = (val(ch) - lo) / den;
        done = c1 > done ? c1 : done;
      }
      for (int ch = done; ch < nband; ++ch) ox[ch] = val(ch);
    } else {
      for (int ch = 0; ch < nband; ++ch) {
        float v = l[band_plane[ch] * T * TP];
        if (d.color) v = colour(v, coef[ch]);
        if (d.mode != SATCV_RECORD_NONE) v = (v - coef[ch].lo) / coef[ch].den;
        ox[ch] = v;
      }
    }
    // passthrough bands, one-hot features (after the bands, in plane order), response
    int cp = nband, ch_hot = nband + npass, cy = 0;
    for (int j = 0; j < d.k; ++j) {
      const float v = l[j * T * TP];
      const int kind = d.kind[j];
      if (kind == SATCV_PLANE_PASS) ox[cp++] = v;
      else if (kind == SATCV_PLANE_ONEHOT) {
        const int cls = (int)(unsigned char)(int)v;                   // .astype(np.uint8)
        for (int e = 0; e < d.depth[j]; ++e) ox[ch_hot++] = cls == e ? 1.f : 0.f;
      } else if (kind == SATCV_PLANE_RESPONSE) {
        oy[cy++] = v > 1.f ? 1.f : v;                                 // labels > 1 -> 1
      } else if (kind == SATCV_PLANE_RESPONSE_ONEHOT) {
        const int cls = (int)(unsigned char)(int)v;
        for (int e = 0; e < d.depth[j]; ++e) oy[cy++] = cls == e ? 1.f : 0.f;
      }
    }
  }
}

int check_common(const satcv_record_desc* d, const char* who) {
  SATCV_CHECK(d, "%s: null descriptor", who);
  SATCV_CHECK(d->src, "%s: null source", who);
  SATCV_CHECK(d->k > 0 && d->k <= SATCV_RECORD_MAX_PLANES, "%s: k must be 1..%d", who, SATCV_RECORD_MAX_PLANES);
  SATCV_CHECK(satcv_pixels_ok(d->n, d->h, d->w_, 1) && (long long)d->n * d->k * d->h * d->w_ < (1LL << 40), "%s: bad dims", who);
  for (int j = 0; j < d->k; ++j) {
    SATCV_CHECK(d->kind[j] >= SATCV_PLANE_BAND && d->kind[j] <= SATCV_PLANE_PASS, "%s: unknown plane kind %d of plane %d", who, d->kind[j], j);
    if (d->kind[j] == SATCV_PLANE_ONEHOT || d->kind[j] == SATCV_PLANE_RESPONSE_ONEHOT)
      SATCV_CHECK(d->depth[j] > 0 && d->depth[j] <= 256, "%s: one-hot depth %d of plane %d", who, d->depth[j], j);
  }
  return SATCV_OK;
}

// everything satcv_record_to_tuple refuses, without launching
int check_transform(const satcv_record_desc* d, int& nband, int& npass, int& nx, int& ny) {
  int rc = check_common(d, "record_to_tuple");
  if (rc) return rc;
  int nhot = 0;
  nband = npass = ny = 0;
  for (int j = 0; j < d->k; ++j) {
    switch (d->kind[j]) {
      case SATCV_PLANE_BAND: ++nband; break;
      case SATCV_PLANE_PASS: ++npass; break;
      case SATCV_PLANE_ONEHOT: nhot += d->depth[j]; break;
      case SATCV_PLANE_RESPONSE: ++ny; break;
      default: ny += d->depth[j]; break;
    }
  }
  nx = nband + npass + nhot;
  SATCV_CHECK(d->x && d->coff_x >= 0 && d->ld_x >= d->coff_x + nx, "record_to_tuple: ld_x %d cannot hold %d feature channels at offset %d", d->ld_x, nx, d->coff_x);
  SATCV_CHECK(ny == 0 || (d->y && d->coff_y >= 0 && d->ld_y >= d->coff_y + ny), "record_to_tuple: ld_y %d cannot hold %d label channels at offset %d", d->ld_y, ny, d->coff_y);
  SATCV_CHECK(!d->morph || d->h == d->w_, "record_to_tuple: flip / rot90 augmentation needs square tiles (%d x %d)", d->h, d->w_);
  SATCV_CHECK(!(d->morph || d->color) || (d->params && d->ld_params >= 2 * nband + 3), "record_to_tuple: null or short parameter table");
  SATCV_CHECK(d->mode >= SATCV_RECORD_NONE && d->mode <= SATCV_RECORD_NORMALIZE, "record_to_tuple: mode %d", d->mode);
  SATCV_CHECK(d->stat_src >= SATCV_STAT_MOMENTS && d->stat_src <= SATCV_STAT_GROUP, "record_to_tuple: stat_src %d", d->stat_src);
  const bool need_stats = (d->color && !d->mean_in) || (d->mode != SATCV_RECORD_NONE && (d->stat_src == SATCV_STAT_CHANNEL || d->stat_src == SATCV_STAT_GROUP));
  SATCV_CHECK(!need_stats || d->stats, "record_to_tuple: null statistics table");
  if (d->mode != SATCV_RECORD_NONE) {
    SATCV_CHECK(d->ngroups >= 0 && d->ngroups <= SATCV_RECORD_MAX_PLANES, "record_to_tuple: ngroups %d", d->ngroups);
    for (int g = 0; g < d->ngroups; ++g)
      SATCV_CHECK(d->gstart[g] >= 0 && d->glen[g] > 0 && d->gstart[g] + d->glen[g] <= nband, "record_to_tuple: group %d [%d, +%d) outside the %d bands",
                  g, d->gstart[g], d->glen[g], nband);
  }
  return SATCV_OK;
}

}  // namespace

extern "C" int satcv_record_stats(const satcv_record_desc* d, void* stream) {
  int rc = check_common(d, "record_stats");
  if (rc) return rc;
  SATCV_CHECK(d->stats, "record_stats: null statistics table");
  if (d->x) {                                  // the descriptor of a whole transform: a refused one starts no launch at all
    int nband, npass, nx, ny;
    rc = check_transform(d, nband, npass, nx, ny);
    if (rc) return rc;
  }
  const int splits = stat_splits(d->h * d->w_);
  const long long planes = (long long)d->n * d->k;
  const long long need = planes * splits * 4 * (long long)sizeof(double);
  SATCV_CHECK(d->stats_ws && d->stats_ws_bytes >= need, "record_stats: workspace of %lld bytes needed", need);
  SATCV_CHECK(planes * splits < (1LL << 31), "record_stats: too many planes");
  hipLaunchKernelGGL(record_stats_partial_kernel, dim3((unsigned)(planes * splits)), dim3(kStatThreads), 0, (hipStream_t)stream, *d, splits);
  hipLaunchKernelGGL(record_stats_finalize_kernel, dim3((unsigned)((planes + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *d, splits);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { satcv_set_error("record_stats launch: %s", hipGetErrorString(e)); return SATCV_ERR_HIP; }
  return SATCV_OK;
}

extern "C" int satcv_record_to_tuple(const satcv_record_desc* d, void* stream) {
  int nband, npass, nx, ny;
  int rc = check_transform(d, nband, npass, nx, ny);
  if (rc) return rc;
  const bool big = d->k <= 8;
  const int T = big ? 32 : 16;
  const long long tiles = (long long)d->n * ((d->h + T - 1) / T) * ((d->w_ + T - 1) / T);
  SATCV_CHECK(tiles < (1LL << 31), "record_to_tuple: too many tiles");
  const size_t lds = (size_t)d->k * T * (T + 1) * sizeof(float);
  if (big) hipLaunchKernelGGL(record_to_tuple_kernel<32>, dim3((unsigned)tiles), dim3(256), lds, (hipStream_t)stream, *d, nband, npass);
  else hipLaunchKernelGGL(record_to_tuple_kernel<16>, dim3((unsigned)tiles), dim3(256), lds, (hipStream_t)stream, *d, nband, npass);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { satcv_set_error("record_to_tuple launch: %s", hipGetErrorString(e)); return SATCV_ERR_HIP; }
  return SATCV_OK;
}
