// The device half of the Cloud-Optimized GeoTIFF writer (raster_tools.write_cog): what numpy_to_raster / arrays_to_cog
// (utils/raster_tools.py:367-461) and write_geotiff_prediction(s) (utils/prediction_tools.py:447-536) leave to rasterio and GDAL's COG
// driver, on a map that is already resident.
//   satcv_raster_convert   dtype conversion with nodata (rasterio's astype + `nodata`)                      one thread per sample
//   satcv_raster_overview  one level of the overview pyramid, nearest / average / mode, nodata-aware          one thread per sample
//   satcv_raster_tiles     tile-major, pixel-interleaved layout with TIFF predictor 2                         one thread per sample
//   satcv_lzw_tiles        TIFF LZW of every tile at once (COMPRESS=LZW): ONE WAVEFRONT PER TILE.  The coder (lzw_core.hpp) is sequential,
//                          so every lane of the wave runs it on the same values -- control flow is wave-uniform by construction -- with
//                          the dictionary in LDS (32 KB: four tiles per CU).  What the lanes share is the memory traffic: a 1 KB input
//                          chunk arrives by one 16-byte load per lane, the packed codes leave by one 16-byte store per lane per KB,
//                          and the table is emptied by all lanes at a Clear.
//   satcv_bytes_compact    the compressed tiles, each in its slot, gathered to their file offsets: one device-to-host copy of the payload
//   satcv_lzw_encode_host  the same coder on the CPU (a host function, as satcv_crc32c is)
// and the device half of the reader (raster_tools.read_cog), the mirror image:
//   satcv_lzw_decode_tiles TIFF LZW of every block at once, ONE WAVEFRONT PER BLOCK, the decoder of lzw_core.hpp with wave-uniform control
//                          flow.  The dictionary is (position in the output, length) per code (24 KB of LDS); a code is a copy of `len`
//                          bytes from an earlier output position, done by the 64 lanes together.  The last 16 KB of output live in an LDS
//                          ring that leaves in 1 KB pieces, one 16-byte store per lane; a copy whose source has left the ring reads it
//                          back from global memory, where it was stored at least one flush -- one __syncthreads() -- ago.  DESIGN.md,
//                          "Reading GeoTIFFs", has the LDS budget and the memory-ordering argument.
//   satcv_lzw_decode_host  the same decoder on the CPU
//   satcv_raster_untile    decoded blocks -> a window of a resident raster, predictor 2 undone by one wavefront per block row
// Every kernel is a grid-stride loop over 64-bit indices; descriptors are refused on the host before any launch.
#include "common.hpp"
#include "lzw_core.hpp"
#include "raster_kinds.hpp"
#include <cmath>
#include <cstring>

namespace {

constexpr int RS_BLOCK = 256;
constexpr int RS_MAX_GRID = 1 << 16;
constexpr int LZ_CHUNK = 1024;       // bytes per input chunk and per output flush: 64 lanes x 16 bytes

int grid_for(long long items) {
  long long g = (items + RS_BLOCK - 1) / RS_BLOCK;
  return (int)(g < 1 ? 1 : g > RS_MAX_GRID ? RS_MAX_GRID : g);
}

// ---------------------------------------------------------------- convert
template <typename S, typename D>
__device__ __forceinline__ D convert_one(S v, float scale, bool has_nd, D nd) {
  if constexpr (std::is_same<D, float>::value) {
    if constexpr (std::is_same<S, float>::value) return scale != 0.f ? v * scale : v;
    else return (float)v;
  } else if constexpr (std::is_same<S, float>::value) {
    const float t = scale != 0.f ? v * scale : v;
    if (t != t) return has_nd ? nd : (D)0;
    const float r = rintf(t);                                        // half to even
    const float lo = (float)std::numeric_limits<D>::min(), hi = (float)std::numeric_limits<D>::max();      // (float)INT32_MAX is 2^31: >= saturates
    if (r <= lo) return std::numeric_limits<D>::min();
    if (r >= hi) return std::numeric_limits<D>::max();
    return (D)r;
  } else {
    const long long x = (long long)v, lo = (long long)std::numeric_limits<D>::min(), hi = (long long)std::numeric_limits<D>::max();
    return (D)(x < lo ? lo : x > hi ? hi : x);
  }
}

template <typename S, typename D>
__global__ __launch_bounds__(RS_BLOCK) void convert_kernel(const S* __restrict__ src, D* __restrict__ dst, long long total, int c, int ld, int coff,
                                                            float scale, int has_nd, D nd) {
  for (long long i = (long long)blockIdx.x * RS_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * RS_BLOCK) {
    const long long p = i / c;
    const int b = (int)(i - p * c);
    dst[i] = convert_one<S, D>(src[p * ld + coff + b], scale, has_nd != 0, nd);
  }
}

// ---------------------------------------------------------------- overview
template <typename T>
__global__ __launch_bounds__(RS_BLOCK) void overview_kernel(const T* __restrict__ src, T* __restrict__ dst, int h, int w, int c, int oh, int ow,
                                                             int resampling, int has_nd, T nd) {
  const long long total = (long long)oh * ow * c;
  for (long long i = (long long)blockIdx.x * RS_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * RS_BLOCK) {
    const long long p = i / c;
    const int b = (int)(i - p * c), oy = (int)(p / ow), ox = (int)(p - (long long)oy * ow);
    const int y0 = 2 * oy, x0 = 2 * ox;                    // always inside the image
    if (resampling == 0) {
      dst[i] = src[((long long)y0 * w + x0) * c + b];
      continue;
    }
    T v[4];
    int n = 0;                                            // the valid samples of the block, row-major
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx) {
        const int y = y0 + dy, x = x0 + dx;
        if (y < h && x < w) {
          const T s = src[((long long)y * w + x) * c + b];
          if (sample_valid(s, has_nd != 0, nd)) v[n++] = s;
        }
      }
    T out;
    if (n == 0) {
      if constexpr (std::is_same<T, float>::value) out = has_nd ? nd : NAN;
      else out = nd;                                      // (integers without nodata always have a valid sample)
    } else if (resampling == 1) {
      if constexpr (std::is_same<T, float>::value) {
        float s = v[0];
        for (int k = 1; k < n; ++k) s = s + v[k];
        out = s / (float)n;
      } else {
        long long s = 0;
        for (int k = 0; k < n; ++k) s += (long long)v[k];
        const long long num = 2 * s + n, den = 2 * n;
        long long q = num / den;
        if (num % den < 0) --q;                           // floor
        out = (T)q;
      }
    } else {
      int best = 0;
      out = v[0];
      for (int k = 0; k < n; ++k) {
        int cnt = 0;
        for (int j = 0; j < n; ++j) cnt += v[j] == v[k];
        if (cnt > best || (cnt == best && v[k] < out)) { best = cnt; out = v[k]; }
      }
    }
    dst[i] = out;
  }
}

// ---------------------------------------------------------------- tiles
// U: the unsigned integer of the sample's width -- the predictor's arithmetic is modular in it, and a float passes as its bits
template <typename U>
__global__ __launch_bounds__(RS_BLOCK) void tiles_kernel(const U* __restrict__ src, U* __restrict__ dst, int h, int w, int c, int bs, int ntx,
                                                          long long total, int predictor, U fill) {
  for (long long i = (long long)blockIdx.x * RS_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * RS_BLOCK) {
    long long r = i / c;
    const int b = (int)(i - r * c);
    const int px = (int)(r % bs);
    r /= bs;
    const int py = (int)(r % bs);
    const long long tile = r / bs;
    const int ty = (int)(tile / ntx), tx = (int)(tile - (long long)ty * ntx);
    const int y = ty * bs + py, x = tx * bs + px;
    const bool row_in = y < h;
    const U cur = (row_in && x < w) ? src[((long long)y * w + x) * c + b] : fill;
    U out = cur;
    if (predictor && px > 0) {
      const U left = (row_in && x - 1 < w) ? src[((long long)y * w + (x - 1)) * c + b] : fill;
      out = (U)(cur - left);
    }
    dst[i] = out;
  }
}

// ---------------------------------------------------------------- LZW, one wavefront per tile
struct DevSink {
  unsigned char* buf;          // LZ_CHUNK bytes of LDS
  unsigned char* gdst;         // the tile's slot
  long long flushed, slot_bytes;
  int pos, lane;
  __device__ __forceinline__ void flush() {                // every lane of the wave is here: the coder's state is wave-uniform
    __syncthreads();
    const long long off = flushed + lane * 16;
    if (lane * 16 < pos && off + 16 <= slot_bytes) *reinterpret_cast<uint4*>(gdst + off) = *reinterpret_cast<const uint4*>(buf + lane * 16);
    __syncthreads();
    flushed += pos;
    pos = 0;
  }
  __device__ __forceinline__ void byte(unsigned b) {
    buf[pos++] = (unsigned char)b;
    if (pos == LZ_CHUNK) flush();
  }
  __device__ __forceinline__ void clear(uint32_t* table) {
    __syncthreads();
    for (int k = lane; k < satcv_lzw::SLOTS; k += 64) table[k] = satcv_lzw::EMPTY;
    __syncthreads();
  }
};

__global__ __launch_bounds__(64) void lzw_tiles_kernel(const unsigned char* __restrict__ src, int n, long long tile_bytes, unsigned char* __restrict__ dst,
                                                        long long slot_bytes, int* __restrict__ sizes) {
  __shared__ __attribute__((aligned(16))) uint32_t table[satcv_lzw::SLOTS];
  __shared__ __attribute__((aligned(16))) unsigned char in[LZ_CHUNK];
  __shared__ __attribute__((aligned(16))) unsigned char outb[LZ_CHUNK];
  const int lane = threadIdx.x;
  for (int tile = blockIdx.x; tile < n; tile += gridDim.x) {
    const unsigned char* s = src + (long long)tile * tile_bytes;
    DevSink sink{outb, dst + (long long)tile * slot_bytes, 0, slot_bytes, 0, lane};
    satcv_lzw::Coder<DevSink> coder;
    coder.table = table;
    coder.sink = &sink;
    coder.start();
    for (long long base = 0; base < tile_bytes; base += LZ_CHUNK) {
      __syncthreads();                                     // the previous chunk is consumed
      const long long off = base + lane * 16;
      if (off + 16 <= tile_bytes) *reinterpret_cast<uint4*>(in + lane * 16) = *reinterpret_cast<const uint4*>(s + off);      // tile_bytes % 16 == 0
      __syncthreads();
      const int m = (int)(tile_bytes - base < LZ_CHUNK ? tile_bytes - base : LZ_CHUNK);      // a multiple of 16
      for (int k = 0; k < m; k += 16) {                    // one LDS read per 16 input bytes: the probe is the only LDS latency per byte
        const uint4 q = *reinterpret_cast<const uint4*>(in + k);
        const unsigned w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) coder.feed((w4[j >> 2] >> (8 * (j & 3))) & 0xffu);
      }
    }
    coder.finish();
    const long long size = sink.flushed + sink.pos;
    sink.flush();
    if (lane == 0) sizes[tile] = (int)size;
    __syncthreads();                                       // the next tile reuses the LDS buffers
  }
}

// ---------------------------------------------------------------- LZW decode, one wavefront per block
constexpr int LZ_RING = 16384;       // bytes of output kept in LDS; a string is at most 4096 - 257 bytes, a flush lags by less than LZ_CHUNK

// the compressed slice starts anywhere: chunk c holds the bytes of the 16-byte-aligned window [c * LZ_CHUNK, (c + 1) * LZ_CHUNK) counted
// from the slice start rounded down to 16; a 16-byte group that lies wholly inside the slice comes by one load per lane, the head and
// the tail byte by byte, so nothing outside the slice is read
struct DevSource {
  unsigned char* in;           // LZ_CHUNK bytes of LDS
  const unsigned char* g;      // the slice
  long long size;
  int shift, lane;             // g - shift is 16-byte aligned
  long long chunk, word_at;    // what `in` and `word` hold (-1: nothing)
  uint32_t word;
  __device__ __forceinline__ void load(long long c) {      // every lane of the wave is here
    __syncthreads();
    const long long first = c * LZ_CHUNK + lane * 16 - shift;      // slice index of this lane's group
    if (first >= 0 && first + 16 <= size) *reinterpret_cast<uint4*>(in + lane * 16) = *reinterpret_cast<const uint4*>(g + first);
    else
      for (int k = 0; k < 16; ++k)
        if (first + k >= 0 && first + k < size) in[lane * 16 + k] = g[first + k];
    __syncthreads();
    chunk = c;
  }
  __device__ __forceinline__ unsigned byte(long long i) {
    const long long v = i + shift;
    if ((v >> 10) != chunk) load(v >> 10);
    if ((v >> 2) != word_at) {
      word = *reinterpret_cast<const uint32_t*>(in + (v & (LZ_CHUNK - 4)));
      word_at = v >> 2;
    }
    return (word >> (8 * (int)(v & 3))) & 0xffu;
  }
};

struct DevDecSink {
  unsigned char* ring;         // LZ_RING bytes of LDS: output byte p lives at ring[p % LZ_RING] until p + LZ_RING bytes are out
  unsigned char* gdst;         // the block's slot (read back by `copy`: not __restrict__)
  long long flushed;           // bytes of the block in global memory, a multiple of LZ_CHUNK; every flush ended with a barrier
  int lane;
  bool wide;                   // gdst is 16-byte aligned
  __device__ __forceinline__ void flush() {
    const long long at = flushed + lane * 16;
    if (wide) *reinterpret_cast<uint4*>(gdst + at) = *reinterpret_cast<const uint4*>(ring + (at & (LZ_RING - 1)));
    else
      for (int k = 0; k < 16; ++k) gdst[at + k] = ring[(at + k) & (LZ_RING - 1)];
    flushed += LZ_CHUNK;
    __syncthreads();           // workgroup-scope fence: these stores are visible to the wave's later loads
  }
  // the bytes up to `end` are in the ring: make them visible to the next code's reads, then let full KBs leave
  __device__ __forceinline__ void wrote(long long end) {
    __syncthreads();
    for (int r = 0; r < satcv_lzw::TABLE / LZ_CHUNK + 1; ++r)
      if (flushed + LZ_CHUNK <= end) flush();
  }
  __device__ __forceinline__ void literal(long long at, unsigned b) {
    ring[at & (LZ_RING - 1)] = (unsigned char)b;
    wrote(at + 1);
  }
  // The source [from, from + len) was written by earlier codes.  It is still in the ring when from + LZ_RING >= at + len (this code's own
  // bytes then overwrite nothing of it); otherwise from + len < at + 2 len - LZ_RING <= at - 8192 < flushed: it is read from the slot.
  __device__ __forceinline__ void copy(long long from, int len, long long at, bool wrap) {
    const bool in_ring = from + LZ_RING >= at + len;
    for (int r = 0; r < satcv_lzw::TABLE; r += 64) {
      const int j = r + lane;
      if (j < len) {
        const long long q = from + ((wrap && j == len - 1) ? 0 : j);
        ring[(at + j) & (LZ_RING - 1)] = in_ring ? ring[q & (LZ_RING - 1)] : gdst[q];
      }
      if (r + 64 >= len) break;                            // (len is wave-uniform)
    }
    wrote(at + len);
  }
  __device__ __forceinline__ void finish(long long n) {    // the tail below one KB, byte by byte
    for (long long j = flushed + lane; j < n; j += 64) gdst[j] = ring[j & (LZ_RING - 1)];
    __syncthreads();
  }
};

__global__ __launch_bounds__(64) void lzw_decode_kernel(const unsigned char* __restrict__ payload, long long payload_bytes, const long long* __restrict__ offsets,
                                                         const int* __restrict__ sizes, int n, long long block_bytes, long long dst_stride, unsigned char* dst,
                                                         int* __restrict__ status, int* __restrict__ lengths) {
  __shared__ __attribute__((aligned(16))) uint32_t pos[satcv_lzw::TABLE];
  __shared__ __attribute__((aligned(16))) uint16_t len[satcv_lzw::TABLE];
  __shared__ __attribute__((aligned(16))) unsigned char ring[LZ_RING];
  __shared__ __attribute__((aligned(16))) unsigned char in[LZ_CHUNK];
  const int lane = threadIdx.x;
  for (int blk = blockIdx.x; blk < n; blk += gridDim.x) {
    long long off = offsets[blk], size = sizes[blk];
    if (off < 0 || off > payload_bytes || size < 0) { off = 0; size = 0; }      // a slice is clipped to the payload: it then ends as truncated
    if (size > payload_bytes - off) size = payload_bytes - off;
    unsigned char* g = dst + (long long)blk * dst_stride;
    DevSource source{in, payload + off, size, (int)((uintptr_t)(payload + off) & 15), lane, -1, -1, 0u};
    DevDecSink sink{ring, g, 0, lane, ((uintptr_t)g & 15) == 0};
    satcv_lzw::Decoder<DevSource, DevDecSink> dec{pos, len, &source, &sink};
    long long produced = 0;
    const int st = dec.run(size, block_bytes, &produced);
    sink.finish(produced);
    if (lane == 0) {
      status[blk] = st;
      if (lengths) lengths[blk] = (int)produced;
    }
    __syncthreads();                                       // the next block reuses the LDS buffers
  }
}

// ---------------------------------------------------------------- untile
struct UntileAt {
  bool ok;
  long long to;
};
// where sample (py, px, band) of decoded block j goes: the window test, the band map, the destination layout
__device__ __forceinline__ UntileAt untile_at(const satcv_untile_desc& d, int t, int py, int px, int b) {
  UntileAt r{false, 0};
  if (t < 0) return r;
  int plane = 0;
  if (d.planar == 2) { plane = t / d.per_plane; t -= plane * d.per_plane; }
  const int by = t / d.across, bx = t - by * d.across;
  const long long y = (long long)by * d.bh + py - d.row0, x = (long long)bx * d.bw + px - d.col0;
  const int band = d.planar == 2 ? plane : b;
  if (y < 0 || y >= d.h || x < 0 || x >= d.w_ || band >= d.spp) return r;
  const int m = d.band_map[band];
  if (m < 0) return r;
  r.ok = true;
  r.to = d.layout == 0 ? (y * d.w_ + x) * d.ld + d.coff + m : ((long long)(d.coff + m) * d.h + y) * d.w_ + x;
  return r;
}

template <typename U>
__global__ __launch_bounds__(RS_BLOCK) void untile_kernel(satcv_untile_desc d, int cb, long long total) {
  const unsigned char* src = (const unsigned char*)d.src;
  U* dst = (U*)d.dst;
  for (long long i = (long long)blockIdx.x * RS_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * RS_BLOCK) {
    long long r = i / cb;
    const int b = (int)(i - r * cb);
    const int px = (int)(r % d.bw);
    r /= d.bw;
    const int py = (int)(r % d.bh);
    const long long j = r / d.bh;
    const UntileAt a = untile_at(d, d.blocks[j], py, px, b);
    if (a.ok) dst[a.to] = reinterpret_cast<const U*>(src + j * d.src_stride)[((long long)py * d.bw + px) * cb + b];
  }
}

// predictor 2: one wavefront per block row; per band a 64-lane inclusive scan with a carry between rounds, from the block's first pixel on
template <typename U>
__global__ __launch_bounds__(RS_BLOCK) void untile_scan_kernel(satcv_untile_desc d, int cb, long long rows) {
  const unsigned char* src = (const unsigned char*)d.src;
  U* dst = (U*)d.dst;
  const int lane = threadIdx.x & 63, waves = RS_BLOCK / 64;
  for (long long it = (long long)blockIdx.x * waves + (threadIdx.x >> 6); it < rows; it += (long long)gridDim.x * waves) {
    const long long j = it / d.bh;
    const int py = (int)(it - j * d.bh);
    const int t = d.blocks[j];
    const U* row = reinterpret_cast<const U*>(src + j * d.src_stride) + (long long)py * d.bw * cb;
    for (int b = 0; b < cb; ++b) {
      uint32_t carry = 0;
      for (int px0 = 0; px0 < d.bw; px0 += 64) {
        const int px = px0 + lane;
        uint32_t v = px < d.bw ? (uint32_t)row[(long long)px * cb + b] : 0u;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
          const uint32_t up = __shfl_up(v, s, 64);
          if (lane >= s) v += up;
        }
        v += carry;
        carry = __shfl(v, 63, 64);
        if (px < d.bw) {
          const UntileAt a = untile_at(d, t, py, px, b);
          if (a.ok) dst[a.to] = (U)v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- compaction
__global__ __launch_bounds__(RS_BLOCK) void compact_kernel(const unsigned char* __restrict__ slots, long long slot_bytes, const int* __restrict__ sizes,
                                                            const long long* __restrict__ offsets, int n, long long chunks, unsigned char* __restrict__ dst,
                                                            long long dst_bytes) {
  constexpr int PER = 16;                                  // bytes per thread and item
  const long long items = (long long)n * chunks;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int tile = (int)(it / chunks);
    const long long first = (it - (long long)tile * chunks) * (RS_BLOCK * PER);
    long long size = sizes[tile];
    size = size < 0 ? 0 : size > slot_bytes ? slot_bytes : size;
    const long long to = offsets[tile];
    const unsigned char* s = slots + (long long)tile * slot_bytes;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const long long j = first + (long long)k * RS_BLOCK + threadIdx.x;
      if (j < size && to >= 0 && to + j < dst_bytes) dst[to + j] = s[j];
    }
  }
}

struct HostSink {
  unsigned char* dst;
  long long cap, pos;
  void byte(unsigned b) {
    if (pos < cap) dst[pos] = (unsigned char)b;
    ++pos;
  }
  void clear(uint32_t* table) { memset(table, 0xff, sizeof(uint32_t) * satcv_lzw::SLOTS); }
};

struct HostSource {
  const unsigned char* src;
  unsigned byte(long long i) const { return src[i]; }
};
struct HostDecSink {
  unsigned char* dst;
  void literal(long long at, unsigned b) { dst[at] = (unsigned char)b; }
  void copy(long long from, int len, long long at, bool wrap) {
    for (int j = 0; j < len; ++j) dst[at + j] = dst[from + ((wrap && j == len - 1) ? 0 : j)];
  }
};

// what the three raster entries share; same_kind: overview and tiles keep the kind and read a contiguous raster
int check_raster(const satcv_raster_desc* d, const char* who, bool same_kind) {
  SATCV_CHECK(d && d->src && d->dst, "%s: null pointer (descriptor, src or dst)", who);
  SATCV_CHECK(kind_ok(d->src_kind) && kind_ok(d->dst_kind), "%s: unknown kind %d -> %d (0 u8, 1 u16, 2 f32, 3 i16, 5 i32)", who, d->src_kind, d->dst_kind);
  SATCV_CHECK(d->h > 0 && d->w_ > 0 && d->c > 0, "%s: sizes must be positive", who);
  SATCV_CHECK(d->c <= 16, "%s: c = %d bands (at most 16)", who, d->c);
  SATCV_CHECK(satcv_pixels_ok(1, d->h, d->w_, 1), "%s: map beyond 2^31 pixels", who);
  SATCV_CHECK(d->ld > 0 && d->coff >= 0 && (long long)d->coff + d->c <= d->ld, "%s: channel range (coff + c <= ld)", who);
  SATCV_CHECK((uintptr_t)d->src % kind_bytes(d->src_kind) == 0 && (uintptr_t)d->dst % kind_bytes(d->dst_kind) == 0, "%s: misaligned pointer", who);
  if (same_kind) {
    SATCV_CHECK(d->src_kind == d->dst_kind, "%s: keeps the kind (src_kind %d, dst_kind %d)", who, d->src_kind, d->dst_kind);
    SATCV_CHECK(d->ld == d->c && d->coff == 0, "%s: reads a contiguous raster (ld == c, coff == 0)", who);
  }
  return SATCV_OK;
}

}  // namespace

extern "C" int satcv_raster_convert(const satcv_raster_desc* d, void* stream) {
  const int rc = check_raster(d, "raster_convert", false);
  if (rc != SATCV_OK) return rc;
  SATCV_CHECK(d->scale == 0.f || d->src_kind == 2, "raster_convert: scale is for f32 sources");
  const long long total = (long long)d->h * d->w_ * d->c;
  const hipStream_t st = (hipStream_t)stream;
  by_kind(d->src_kind, [&](auto sv) {
    using S = decltype(sv);
    return by_kind(d->dst_kind, [&](auto dv) {
      using D = decltype(dv);
      hipLaunchKernelGGL((convert_kernel<S, D>), dim3(grid_for(total)), dim3(RS_BLOCK), 0, st, (const S*)d->src, (D*)d->dst, total, d->c, d->ld, d->coff,
                         d->scale, d->has_nodata, nodata_as<D>(d->nodata));
      return 0;
    });
  });
  return launched("raster_convert");
}

extern "C" int satcv_raster_overview(const satcv_raster_desc* d, void* stream) {
  const int rc = check_raster(d, "raster_overview", true);
  if (rc != SATCV_OK) return rc;
  SATCV_CHECK(d->resampling >= 0 && d->resampling <= 2, "raster_overview: resampling %d (0 nearest, 1 average, 2 mode)", d->resampling);
  SATCV_CHECK(!(d->resampling == 2 && d->src_kind == 2), "raster_overview: mode resampling is for integer kinds");
  const int oh = (d->h + 1) / 2, ow = (d->w_ + 1) / 2;
  const long long total = (long long)oh * ow * d->c;
  const hipStream_t st = (hipStream_t)stream;
  by_kind(d->src_kind, [&](auto tv) {
    using T = decltype(tv);
    hipLaunchKernelGGL((overview_kernel<T>), dim3(grid_for(total)), dim3(RS_BLOCK), 0, st, (const T*)d->src, (T*)d->dst, d->h, d->w_, d->c, oh, ow,
                       d->resampling, d->has_nodata, nodata_as<T>(d->nodata));
    return 0;
  });
  return launched("raster_overview");
}

extern "C" int satcv_raster_tiles(const satcv_raster_desc* d, void* stream) {
  const int rc = check_raster(d, "raster_tiles", true);
  if (rc != SATCV_OK) return rc;
  const int bs = d->blocksize, eb = kind_bytes(d->src_kind);
  SATCV_CHECK(bs > 0 && bs % 16 == 0, "raster_tiles: blocksize %d is not a positive multiple of 16", bs);
  SATCV_CHECK(bs <= (1 << 15) && (long long)bs * bs * d->c * eb < (1LL << 30), "raster_tiles: blocksize %d gives tiles of 2^30 bytes or more", bs);
  SATCV_CHECK(!(d->predictor && d->src_kind == 2), "raster_tiles: the predictor is for integer kinds");
  const int ntx = (d->w_ + bs - 1) / bs, nty = (d->h + bs - 1) / bs;
  const long long total = (long long)nty * ntx * bs * bs * d->c;
  const hipStream_t st = (hipStream_t)stream;
  uint32_t fill = 0;                                       // the bits of nodata in the kind, 0 without
  if (d->has_nodata)
    by_kind(d->src_kind, [&](auto tv) {
      using T = decltype(tv);
      const T v = nodata_as<T>(d->nodata);
      memcpy(&fill, &v, sizeof(T));
      return 0;
    });
  const dim3 grid(grid_for(total)), block(RS_BLOCK);
  if (eb == 1)
    hipLaunchKernelGGL((tiles_kernel<uint8_t>), grid, block, 0, st, (const uint8_t*)d->src, (uint8_t*)d->dst, d->h, d->w_, d->c, bs, ntx, total, d->predictor, (uint8_t)fill);
  else if (eb == 2)
    hipLaunchKernelGGL((tiles_kernel<uint16_t>), grid, block, 0, st, (const uint16_t*)d->src, (uint16_t*)d->dst, d->h, d->w_, d->c, bs, ntx, total, d->predictor, (uint16_t)fill);
  else
    hipLaunchKernelGGL((tiles_kernel<uint32_t>), grid, block, 0, st, (const uint32_t*)d->src, (uint32_t*)d->dst, d->h, d->w_, d->c, bs, ntx, total, d->predictor, fill);
  return launched("raster_tiles");
}

extern "C" int satcv_lzw_tiles(const void* src, int32_t n, int64_t tile_bytes, void* dst, int32_t* sizes, void* stream) {
  SATCV_CHECK(src && dst && sizes, "lzw_tiles: null pointer (src, dst or sizes)");
  SATCV_CHECK(n > 0, "lzw_tiles: n = %d tiles", n);
  SATCV_CHECK(tile_bytes > 0 && tile_bytes < (1LL << 30), "lzw_tiles: tile_bytes = %lld (1 ... 2^30 - 1)", (long long)tile_bytes);
  SATCV_CHECK(tile_bytes % 16 == 0, "lzw_tiles: tile_bytes = %lld is not a multiple of 16", (long long)tile_bytes);
  SATCV_CHECK((uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0, "lzw_tiles: src and dst must be 16-byte aligned");
  const long long slot = 2 * tile_bytes + 16;
  const int grid = n < 4096 ? n : 4096;                    // four tiles per CU are resident; the rest is a grid-stride loop
  hipLaunchKernelGGL(lzw_tiles_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, (const unsigned char*)src, n, (long long)tile_bytes, (unsigned char*)dst, slot, sizes);
  return launched("lzw_tiles");
}

extern "C" int satcv_bytes_compact(const void* slots, int64_t slot_bytes, const int32_t* sizes, const int64_t* offsets, int32_t n, void* dst,
                                   int64_t dst_bytes, void* stream) {
  SATCV_CHECK(slots && sizes && offsets && dst, "bytes_compact: null pointer (slots, sizes, offsets or dst)");
  SATCV_CHECK(n > 0, "bytes_compact: n = %d slots", n);
  SATCV_CHECK(slot_bytes > 0 && slot_bytes <= (1LL << 31) + 16, "bytes_compact: slot_bytes = %lld", (long long)slot_bytes);
  SATCV_CHECK(dst_bytes > 0, "bytes_compact: dst_bytes = %lld", (long long)dst_bytes);
  const long long chunks = (slot_bytes + RS_BLOCK * 16 - 1) / (RS_BLOCK * 16);
  const long long items = (long long)n * chunks;
  const int grid = (int)(items > RS_MAX_GRID ? RS_MAX_GRID : items);
  hipLaunchKernelGGL(compact_kernel, dim3(grid), dim3(RS_BLOCK), 0, (hipStream_t)stream, (const unsigned char*)slots, (long long)slot_bytes, sizes,
                     (const long long*)offsets, n, chunks, (unsigned char*)dst, (long long)dst_bytes);
  return launched("bytes_compact");
}

extern "C" int satcv_lzw_encode_host(const void* src, int64_t n, void* dst, int64_t cap, int64_t* size) {
  SATCV_CHECK(size, "lzw_encode_host: null pointer (size)");
  *size = 0;
  SATCV_CHECK((src || n == 0) && (dst || cap == 0), "lzw_encode_host: null pointer (src or dst)");
  SATCV_CHECK(n >= 0 && n < (1LL << 30) && cap >= 0, "lzw_encode_host: n = %lld bytes (below 2^30), cap = %lld", (long long)n, (long long)cap);
  uint32_t table[satcv_lzw::SLOTS];
  HostSink sink{(unsigned char*)dst, cap, 0};
  satcv_lzw::Coder<HostSink> coder;
  coder.table = table;
  coder.sink = &sink;
  coder.start();
  const unsigned char* s = (const unsigned char*)src;
  for (int64_t i = 0; i < n; ++i) coder.feed(s[i]);
  coder.finish();
  *size = sink.pos;                                        // the size the stream needs, also when it did not fit
  SATCV_CHECK(sink.pos <= cap, "lzw_encode_host: the stream needs %lld bytes, cap = %lld", (long long)sink.pos, (long long)cap);
  return SATCV_OK;
}

extern "C" int satcv_lzw_decode_tiles(const void* payload, int64_t payload_bytes, const int64_t* offsets, const int32_t* sizes, int32_t n, int64_t block_bytes,
                                      void* dst, int64_t dst_stride, int32_t* status, int32_t* lengths, void* stream) {
  SATCV_CHECK(payload && offsets && sizes && dst && status, "lzw_decode_tiles: null pointer (payload, offsets, sizes, dst or status)");
  SATCV_CHECK(n > 0, "lzw_decode_tiles: n = %d blocks", n);
  SATCV_CHECK(payload_bytes > 0, "lzw_decode_tiles: payload_bytes = %lld", (long long)payload_bytes);
  SATCV_CHECK(block_bytes > 0 && block_bytes < (1LL << 30), "lzw_decode_tiles: block_bytes = %lld (1 ... 2^30 - 1)", (long long)block_bytes);
  SATCV_CHECK(dst_stride >= block_bytes && dst_stride < (1LL << 31), "lzw_decode_tiles: dst_stride = %lld is below block_bytes = %lld (or 2^31 and more)",
              (long long)dst_stride, (long long)block_bytes);
  SATCV_CHECK((uintptr_t)offsets % 8 == 0 && (uintptr_t)sizes % 4 == 0 && (uintptr_t)status % 4 == 0 && (uintptr_t)lengths % 4 == 0,
              "lzw_decode_tiles: misaligned pointer (offsets, sizes, status or lengths)");
  const int grid = n < 4096 ? n : 4096;                    // three blocks per CU are resident (41 KB of LDS each); the rest is a grid-stride loop
  hipLaunchKernelGGL(lzw_decode_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, (const unsigned char*)payload, (long long)payload_bytes,
                     (const long long*)offsets, sizes, n, (long long)block_bytes, (long long)dst_stride, (unsigned char*)dst, status, lengths);
  return launched("lzw_decode_tiles");
}

extern "C" int satcv_lzw_decode_host(const void* src, int64_t n, void* dst, int64_t cap, int64_t* size, int32_t* status) {
  SATCV_CHECK(size && status, "lzw_decode_host: null pointer (size or status)");
  *size = 0;
  *status = satcv_lzw::DEC_TRUNCATED;
  SATCV_CHECK((src || n == 0) && (dst || cap == 0), "lzw_decode_host: null pointer (src or dst)");
  SATCV_CHECK(n >= 0 && n < (1LL << 31) && cap >= 0 && cap < (1LL << 30), "lzw_decode_host: n = %lld bytes (below 2^31), cap = %lld (below 2^30)", (long long)n,
              (long long)cap);
  uint32_t pos[satcv_lzw::TABLE];
  uint16_t len[satcv_lzw::TABLE];
  HostSource source{(const unsigned char*)src};
  HostDecSink sink{(unsigned char*)dst};
  satcv_lzw::Decoder<HostSource, HostDecSink> dec{pos, len, &source, &sink};
  long long produced = 0;
  *status = dec.run(n, cap, &produced);
  *size = produced;
  return SATCV_OK;
}

extern "C" int satcv_raster_untile(const satcv_untile_desc* d, void* stream) {
  SATCV_CHECK(d && d->src && d->dst && d->blocks, "raster_untile: null pointer (descriptor, src, dst or blocks)");
  SATCV_CHECK(kind_ok(d->kind), "raster_untile: unknown kind %d (0 u8, 1 u16, 2 f32, 3 i16, 5 i32)", d->kind);
  SATCV_CHECK(d->nblocks > 0 && d->bh > 0 && d->bw > 0 && d->across > 0 && d->h > 0 && d->w_ > 0, "raster_untile: sizes must be positive");
  SATCV_CHECK(d->spp > 0 && d->spp <= 16, "raster_untile: spp = %d bands (1 ... 16)", d->spp);
  SATCV_CHECK(d->planar == 1 || (d->planar == 2 && d->per_plane > 0), "raster_untile: planar = %d (1 pixel-interleaved, 2 one block sequence per band with per_plane > 0)", d->planar);
  SATCV_CHECK(d->predictor == 0 || d->predictor == 2, "raster_untile: predictor %d (0 or 2)", d->predictor);
  SATCV_CHECK(!(d->predictor && d->kind == 2), "raster_untile: the predictor is for integer kinds");
  SATCV_CHECK(d->layout == 0 || d->layout == 1, "raster_untile: layout %d (0 (h, w, c), 1 (c, h, w))", d->layout);
  SATCV_CHECK(d->row0 >= 0 && d->col0 >= 0, "raster_untile: the window starts at (%d, %d)", d->row0, d->col0);
  SATCV_CHECK(satcv_pixels_ok(1, d->h, d->w_, 1), "raster_untile: window beyond 2^31 pixels");
  const int eb = kind_bytes(d->kind), cb = d->planar == 1 ? d->spp : 1;
  const long long block_bytes = (long long)d->bh * d->bw * cb * eb;
  SATCV_CHECK(d->bh <= (1 << 20) && d->bw <= (1 << 20) && block_bytes < (1LL << 30), "raster_untile: blocks of %d x %d give 2^30 bytes or more", d->bh, d->bw);
  SATCV_CHECK(d->src_stride >= block_bytes && d->src_stride % eb == 0, "raster_untile: src_stride = %lld (at least the block's %lld bytes, a multiple of the sample's)",
              (long long)d->src_stride, block_bytes);
  SATCV_CHECK((uintptr_t)d->src % eb == 0 && (uintptr_t)d->dst % eb == 0 && (uintptr_t)d->blocks % 4 == 0, "raster_untile: misaligned pointer");
  SATCV_CHECK(d->ld > 0 && d->coff >= 0 && d->coff < d->ld, "raster_untile: channel range (0 <= coff < ld)");
  int used = 0;
  for (int b = 0; b < d->spp; ++b) {
    const int m = d->band_map[b];
    SATCV_CHECK(m >= -1 && (long long)d->coff + m < d->ld, "raster_untile: band_map[%d] = %d (-1: dropped, else coff + band_map < ld)", b, m);
    used += m >= 0;
  }
  SATCV_CHECK(used > 0, "raster_untile: band_map keeps no band");
  const hipStream_t st = (hipStream_t)stream;
  if (d->predictor) {
    const long long rows = (long long)d->nblocks * d->bh;
    const long long g = (rows + RS_BLOCK / 64 - 1) / (RS_BLOCK / 64);
    const dim3 grid((unsigned)(g > RS_MAX_GRID ? RS_MAX_GRID : g)), block(RS_BLOCK);
    if (eb == 1) hipLaunchKernelGGL((untile_scan_kernel<uint8_t>), grid, block, 0, st, *d, cb, rows);
    else if (eb == 2) hipLaunchKernelGGL((untile_scan_kernel<uint16_t>), grid, block, 0, st, *d, cb, rows);
    else hipLaunchKernelGGL((untile_scan_kernel<uint32_t>), grid, block, 0, st, *d, cb, rows);
  } else {
    const long long total = (long long)d->nblocks * d->bh * d->bw * cb;
    const dim3 grid(grid_for(total)), block(RS_BLOCK);
    if (eb == 1) hipLaunchKernelGGL((untile_kernel<uint8_t>), grid, block, 0, st, *d, cb, total);
    else if (eb == 2) hipLaunchKernelGGL((untile_kernel<uint16_t>), grid, block, 0, st, *d, cb, total);
    else hipLaunchKernelGGL((untile_kernel<uint32_t>), grid, block, 0, st, *d, cb, total);
  }
  return launched("raster_untile");
}
