// What the raster kernels (raster.hip, warp.hip) share: the sample kinds of satcv_raster_desc, nodata in a kind, sample validity.
#pragma once
#include "common.hpp"
#include <cmath>
#include <limits>

namespace {

// ---------------------------------------------------------------- kinds
template <typename F>
int by_kind(int kind, F&& f) {
  switch (kind) {
    case 0: return f(uint8_t{});
    case 1: return f(uint16_t{});
    case 2: return f(float{});
    case 3: return f(int16_t{});
    default: return f(int32_t{});
  }
}
bool kind_ok(int k) { return k == 0 || k == 1 || k == 2 || k == 3 || k == 5; }
int kind_bytes(int k) { return k == 0 ? 1 : (k == 1 || k == 3) ? 2 : 4; }

// nodata in the destination kind (integers: saturated, NaN -> 0)
template <typename T>
T nodata_as(double v) {
  if constexpr (std::is_same<T, float>::value) return (float)v;
  else {
    if (!(v == v)) return 0;
    const double lo = (double)std::numeric_limits<T>::min(), hi = (double)std::numeric_limits<T>::max();
    return (T)(v < lo ? lo : v > hi ? hi : v);
  }
}

// a sample equal to nodata (with has_nd) is invalid, and so is NaN
template <typename T>
__device__ __forceinline__ bool sample_valid(T v, bool has_nd, T nd) {
  if constexpr (std::is_same<T, float>::value) return v == v && !(has_nd && v == nd);
  else return !(has_nd && v == nd);
}

int launched(const char* who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    satcv_set_error("%s launch: %s", who, hipGetErrorString(e));
    return SATCV_ERR_HIP;
  }
  return SATCV_OK;
}

}  // namespace
