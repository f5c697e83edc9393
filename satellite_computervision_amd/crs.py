"""The EPSG codes this library can reproject between, as the parameters of `satcv_crs` (include/satcv.h, "Reprojection between
coordinate systems").  Host only: no PROJ, no EPSG database and no WKT -- a table of the codes the reference meets (Sentinel-1 / -2
and NAIP scenes in UTM zones, longitude / latitude, the web Mercator of its map viewers):

    4326, 4269            geographic (x = longitude, y = latitude, degrees), WGS84 / NAD83
    3857                  spherical (web) Mercator on the WGS84 semi-major axis
    32601 ... 32660       UTM north, WGS84
    32701 ... 32760       UTM south, WGS84 (false northing 10 000 000 m)
    26901 ... 26923       UTM north, NAD83 (GRS80)

Datum: WGS84 and NAD83 coordinates are taken as the same point -- no datum shift is applied (at most 1-2 m; PROJ's default "ballpark"
transformation for these pairs).  Only the ellipsoid differs: WGS84 for 4326 / 326xx / 327xx / 3857, GRS80 for 4269 / 269xx.
"""
from .tiff_container import parse_crs

GEOGRAPHIC, TRANSVERSE_MERCATOR, SPHERICAL_MERCATOR = 0, 1, 2
WGS84 = (6378137.0, 298.257223563)
GRS80 = (6378137.0, 298.257222101)
SUPPORTED = 'EPSG:4326, 4269, 3857, 32601-32660 (UTM north), 32701-32760 (UTM south), 26901-26923 (NAD83 UTM north)'


def _utm(zone, ellipsoid, south=False):
    return dict(kind=TRANSVERSE_MERCATOR, a=ellipsoid[0], inv_f=ellipsoid[1], lon0=6.0 * zone - 183.0, k0=0.9996, fe=500000.0, fn=10000000.0 if south else 0.0)


def crs_params(crs):
    """'EPSG:n' or an int n -> the fields of `satcv_crs` as a dict: kind (0 geographic, 1 transverse Mercator, 2 spherical Mercator), a,
    inv_f, lon0 (degrees), k0, fe, fn.  ValueError, naming the supported set, for every other code.  WGS84 and NAD83 coordinates are
    taken as the same point (no datum shift, at most 1-2 m); only the ellipsoid differs."""
    n = parse_crs(crs)[0]
    if n in (4326, 4269):
        a, inv_f = WGS84 if n == 4326 else GRS80
        return dict(kind=GEOGRAPHIC, a=a, inv_f=inv_f, lon0=0.0, k0=1.0, fe=0.0, fn=0.0)
    if n == 3857:
        return dict(kind=SPHERICAL_MERCATOR, a=WGS84[0], inv_f=WGS84[1], lon0=0.0, k0=1.0, fe=0.0, fn=0.0)
    if 32601 <= n <= 32660:
        return _utm(n - 32600, WGS84)
    if 32701 <= n <= 32760:
        return _utm(n - 32700, WGS84, south=True)
    if 26901 <= n <= 26923:
        return _utm(n - 26900, GRS80)
    raise ValueError(f'EPSG:{n} cannot be reprojected: the supported codes are {SUPPORTED}')


def crs_struct(crs):
    """`crs_params` as the ctypes structure the C ABI takes"""
    from ._lib import Crs
    return Crs(**crs_params(crs))
