"""The GeoTIFF container on the host, without torch, the library or any import from the package: the tag tables, `parse_crs`, `overview_shapes`,
`tile_grid`, the writer's half (`build_container`, `write_tiles`) and the reader's half (`LevelInfo`, `read_info`, the window and block plan of a
level).  `raster_tools` imports these names and does everything that touches the device.
Written: little-endian classic TIFF, every IFD and every out-of-line value before the first tile byte, tile data from the smallest overview to the
full resolution (the order GDAL's COG driver writes, without its ghost header).  Read: little-endian classic TIFF, tiles or strips, planar
configuration 1 or 2, 8 / 16 / 32-bit samples of one kind, predictor 1 or 2.  Refused by name: big-endian files, BigTIFF, JPEG and every other
compression, the floating-point predictor, other sample widths, bands of differing kinds, more than 16 bands, blocks that point past the file."""
import struct

import numpy as np

DTYPES = {'uint8': (np.uint8, 0), 'uint16': (np.uint16, 1), 'float32': (np.float32, 2), 'int16': (np.int16, 3), 'int32': (np.int32, 5)}      # name -> (NumPy type, kind of satcv_raster_desc)
_SAMPLE_FORMAT = {'uint8': 1, 'uint16': 1, 'int16': 2, 'int32': 2, 'float32': 3}
_COMPRESSION = {None: 1, 'lzw': 5, 'deflate': 8}
_SHORT, _LONG, _ASCII, _DOUBLE = 3, 4, 2, 12
_TIFF_TYPES = {1: 'B', 2: 'c', 3: 'H', 4: 'I', 5: 'II', 6: 'b', 7: 'B', 8: 'h', 9: 'i', 10: 'ii', 11: 'f', 12: 'd', 16: 'Q'}
_COMPRESSION_NAMES = {1: None, 5: 'lzw', 8: 'deflate', 32946: 'deflate'}
_FOREIGN_COMPRESSION = {2: 'CCITT RLE', 3: 'CCITT fax 3', 4: 'CCITT fax 4', 6: 'old-style JPEG', 7: 'JPEG', 32773: 'PackBits', 34712: 'JPEG 2000',
                        34887: 'LERC', 34925: 'LZMA', 50000: 'ZSTD', 50001: 'WebP', 50002: 'JPEG XL'}
_KIND_OF_FORMAT = {(8, 1): 'uint8', (16, 1): 'uint16', (16, 2): 'int16', (32, 2): 'int32', (32, 3): 'float32'}


# ----------------------------------------------------------------------------------------------------------------- arguments
def parse_crs(crs):
    """'EPSG:n' or an int n -> (n, geographic).  The GeoKey model type is geographic iff 4000 <= n < 5000, otherwise projected: a
    documented rule, there is no EPSG database here.  Anything else, WKT included, raises ValueError."""
    if isinstance(crs, (int, np.integer)) and not isinstance(crs, bool):
        n = int(crs)
    elif isinstance(crs, str) and crs.strip().upper().startswith('EPSG:') and crs.strip()[5:].strip().isdigit():
        n = int(crs.strip()[5:])
    else:
        raise ValueError(f"crs must be 'EPSG:n' or an int, got {crs!r} (WKT and PROJ strings are not read)")
    if not 1 <= n <= 65535:
        raise ValueError(f'EPSG code {n} does not fit a GeoKey (1 ... 65535)')
    return n, 4000 <= n < 5000


def overview_shapes(h, w, blocksize, overviews='auto'):
    """[(h, w)] of the overview levels, largest first: every level halves the one before (ceil).  'auto' goes on until both sides are
    <= blocksize; an int is an explicit level count (0: none), limited by the 1 x 1 level."""
    shapes = []
    if overviews == 'auto':
        while max(h, w) > blocksize:
            h, w = (h + 1) // 2, (w + 1) // 2
            shapes.append((h, w))
        return shapes
    if isinstance(overviews, bool) or not isinstance(overviews, (int, np.integer)) or overviews < 0:
        raise ValueError(f"overviews must be 'auto' or a level count >= 0, got {overviews!r}")
    for _ in range(int(overviews)):
        if max(h, w) == 1:
            break
        h, w = (h + 1) // 2, (w + 1) // 2
        shapes.append((h, w))
    return shapes


def tile_grid(h, w, blocksize):
    return (h + blocksize - 1) // blocksize, (w + blocksize - 1) // blocksize


# ----------------------------------------------------------------------------------------------------------------- the writer's half
def _nodata_text(nodata, dtype):
    if dtype != 'float32' or float(nodata) == int(nodata):
        return str(int(nodata))
    return 'nan' if nodata != nodata else repr(float(nodata))


def _geo_tags(transform, epsg, geographic):
    a, b, c, d, e, f = transform
    tags = []
    if b == 0 and d == 0 and a > 0 and e < 0:                 # north-up: scale and tiepoint
        tags.append((33550, _DOUBLE, (a, -e, 0.0)))
        tags.append((33922, _DOUBLE, (0.0, 0.0, 0.0, c, f, 0.0)))
    else:
        tags.append((34264, _DOUBLE, (a, b, 0.0, c, d, e, 0.0, f, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)))
    keys = [(1024, 0, 1, 2 if geographic else 1), (1025, 0, 1, 1), (2048 if geographic else 3072, 0, 1, epsg)]
    tags.append((34735, _SHORT, (1, 1, 0, len(keys)) + tuple(v for k in keys for v in k)))
    return tags


def _pack_value(typ, values):
    if typ == _ASCII:
        return values.encode('ascii') + b'\0'
    return struct.pack('<%d%s' % (len(values), {_SHORT: 'H', _LONG: 'I', _DOUBLE: 'd'}[typ]), *values)


def build_container(shapes, dtype, bands, blocksize, compress, predictor, nodata, transform, crs, byte_counts):
    """The bytes of a COG in front of its tile data, and where every tile goes.

    shapes: [(h, w)] of the levels, full resolution first; byte_counts: per level (same order) the byte count of every tile, tiles
    row-major.  -> (head, offsets, total): `head` holds the header, every IFD (full resolution first, then the overviews by decreasing
    size) and the IFDs' out-of-line values; offsets: per level an int64 array of absolute file offsets; total: the file's size.  Tile
    data runs from the SMALLEST overview to the full resolution and every tile starts on an even offset.  ValueError naming BigTIFF when
    an offset would pass 2^32."""
    epsg, geographic = parse_crs(crs)
    itemsize = np.dtype(DTYPES[dtype][0]).itemsize
    counts = [np.asarray(c, np.int64).reshape(-1) for c in byte_counts]
    if len(counts) != len(shapes):
        raise ValueError(f'{len(shapes)} levels need {len(shapes)} byte count lists, got {len(counts)}')
    ifds = []
    for k, ((h, w), cnt) in enumerate(zip(shapes, counts)):
        nty, ntx = tile_grid(h, w, blocksize)
        if cnt.size != nty * ntx:
            raise ValueError(f'level {k} ({h} x {w}) has {nty * ntx} tiles, got {cnt.size} byte counts')
        tags = [(254, _LONG, (1 if k else 0,)), (256, _LONG, (w,)), (257, _LONG, (h,)), (258, _SHORT, (8 * itemsize,) * bands),
                (259, _SHORT, (_COMPRESSION[compress],)), (262, _SHORT, (1,)), (277, _SHORT, (bands,)), (284, _SHORT, (1,))]
        if predictor:
            tags.append((317, _SHORT, (2,)))
        tags += [(322, _LONG, (blocksize,)), (323, _LONG, (blocksize,)), (324, _LONG, None), (325, _LONG, tuple(int(v) for v in cnt))]
        if bands > 1:
            tags.append((338, _SHORT, (0,) * (bands - 1)))
        tags.append((339, _SHORT, (_SAMPLE_FORMAT[dtype],) * bands))
        if k == 0:
            tags += _geo_tags(transform, epsg, geographic)
        if nodata is not None:
            tags.append((42113, _ASCII, _nodata_text(nodata, dtype)))
        ifds.append(sorted(tags, key=lambda t: t[0]))
    # sizes first: IFDs back to back after the 8-byte header, then the out-of-line values (word-aligned), then the tile data
    pos = 8
    ifd_pos = []
    for tags in ifds:
        ifd_pos.append(pos)
        pos += 2 + 12 * len(tags) + 4

    def nbytes(typ, values, ntiles):
        if values is None:
            return 4 * ntiles
        return len(values) + 1 if typ == _ASCII else len(values) * {_SHORT: 2, _LONG: 4, _DOUBLE: 8}[typ]
    value_pos = {}
    for k, tags in enumerate(ifds):
        for tag, typ, values in tags:
            n = nbytes(typ, values, counts[k].size)
            if n > 4:
                value_pos[(k, tag)] = pos
                pos += n + (n & 1)
    data_start = pos
    offsets = [None] * len(shapes)
    for k in reversed(range(len(shapes))):                    # smallest overview first
        off = np.empty(counts[k].size, np.int64)
        for i, n in enumerate(counts[k]):
            off[i] = pos
            pos += int(n) + (int(n) & 1)
        offsets[k] = off
    total = pos
    if total > 0xffffffff:
        raise ValueError(f'the file would be {total} bytes: offsets past 2^32 need BigTIFF, which is not written')
    head = bytearray(data_start)
    head[0:8] = struct.pack('<2sHI', b'II', 42, ifd_pos[0])
    for k, tags in enumerate(ifds):
        p = ifd_pos[k]
        struct.pack_into('<H', head, p, len(tags))
        p += 2
        for tag, typ, values in tags:
            if values is None:
                values = tuple(int(v) for v in offsets[k])
            raw = _pack_value(typ, values)
            count = len(raw) if typ == _ASCII else len(values)
            struct.pack_into('<HHI', head, p, tag, typ, count)
            if len(raw) <= 4:
                head[p + 8:p + 8 + len(raw)] = raw
            else:
                at = value_pos[(k, tag)]
                struct.pack_into('<I', head, p + 8, at)
                head[at:at + len(raw)] = raw
            p += 12
        struct.pack_into('<I', head, p, ifd_pos[k + 1] if k + 1 < len(ifds) else 0)
    return bytes(head), offsets, total


def write_tiles(out_file, shapes, tiles, dtype, bands, blocksize, compress, predictor, nodata, transform, crs):
    """Write a COG from tiles that are already encoded: tiles[k][i] is the byte string of tile i (row-major) of level k, full resolution
    first, in the compression named by `compress`.  The layout is `build_container`'s."""
    head, offsets, total = build_container(shapes, dtype, bands, blocksize, compress=compress, predictor=predictor, nodata=nodata, transform=transform,
                                           crs=crs, byte_counts=[[len(t) for t in level] for level in tiles])
    with open(out_file, 'wb') as f:
        f.write(head)
        for k in reversed(range(len(shapes))):
            for off, t in zip(offsets[k], tiles[k]):
                f.seek(int(off))
                f.write(t)
        f.truncate(total)
    return out_file


# ----------------------------------------------------------------------------------------------------------------- the reader's half
class LevelInfo:
    """One IFD of a file, as `read_info` returns it: shape (h, w), bands, dtype (name), block_shape (bh, bw), tiled, compression (None,
    'lzw' or 'deflate'), predictor (bool: TIFF predictor 2), planar (1 or 2), nodata (float or None), transform (six numbers in Affine
    order, or None), epsg (int or None), crs ('EPSG:n' or None), overview (NewSubfileType bit 0), offsets / counts (int64 arrays of the
    block list) and index (the IFD's place in the file).  Derived, read-only: itemsize, block_samples (samples per pixel of a block:
    `bands` for planar 1, 1 for planar 2), block_bytes (of a decoded full block), across / down (blocks per row / column of blocks)."""
    __slots__ = ('index', 'shape', 'bands', 'dtype', 'block_shape', 'tiled', 'compression', 'predictor', 'planar', 'nodata', 'transform', 'epsg',
                 'overview', 'offsets', 'counts')

    crs = property(lambda self: None if self.epsg is None else f'EPSG:{self.epsg}')
    itemsize = property(lambda self: np.dtype(DTYPES[self.dtype][0]).itemsize)
    block_samples = property(lambda self: self.bands if self.planar == 1 else 1)
    block_bytes = property(lambda self: self.block_shape[0] * self.block_shape[1] * self.block_samples * self.itemsize)
    across = property(lambda self: -(-self.shape[1] // self.block_shape[1]))
    down = property(lambda self: -(-self.shape[0] // self.block_shape[0]))

    def __repr__(self):
        return 'LevelInfo(' + ', '.join(f'{k}={getattr(self, k)!r}' for k in self.__slots__[:-2]) + ')'


def _read_at(f, at, n, size, what):
    if at < 0 or at + n > size:
        raise ValueError(f'{what} at offset {at} ({n} bytes) points past the end of the file ({size} bytes)')
    f.seek(at)
    return f.read(n)


def _parse_ifd(f, pos, size, index):
    n = struct.unpack('<H', _read_at(f, pos, 2, size, what=f'IFD {index}'))[0]
    raw = _read_at(f, pos + 2, 12 * n + 4, size, what=f'IFD {index}')
    tags = {}
    for i in range(n):
        tag, typ, count, val = struct.unpack_from('<HHI4s', raw, 12 * i)
        if typ not in _TIFF_TYPES:
            continue
        nbytes = struct.calcsize('<' + _TIFF_TYPES[typ]) * count
        if nbytes > 4:
            val = _read_at(f, struct.unpack('<I', val)[0], nbytes, size, what=f'the value of tag {tag} of IFD {index}')
        val = val[:nbytes]
        if typ == 2:
            tags[tag] = val
        elif typ in (4, 16) and count > 64:
            tags[tag] = np.frombuffer(val, '<u4' if typ == 4 else '<u8').astype(np.int64)
        else:
            v = struct.unpack('<%d%s' % (count * len(_TIFF_TYPES[typ]), _TIFF_TYPES[typ][0]), val)
            tags[tag] = tuple(a / b if b else float('nan') for a, b in zip(v[::2], v[1::2])) if typ in (5, 10) else v
    return tags, struct.unpack_from('<I', raw, 12 * n)[0]


def _geo(tags):
    """(transform or None, epsg or None) of an IFD's GeoTIFF tags"""
    keys = {}
    gk = tags.get(34735)
    if gk is not None and len(gk) >= 4:
        for i in range(int(gk[3])):
            k = gk[4 + 4 * i:8 + 4 * i]
            if len(k) == 4 and k[1] == 0:
                keys[int(k[0])] = int(k[3])
    epsg = keys.get(3072, keys.get(2048))
    if epsg is not None and not 1 <= epsg < 32767:
        epsg = None                                           # 32767: user-defined, there is no EPSG database here
    transform = None
    if 34264 in tags and len(tags[34264]) == 16:
        m = tags[34264]
        transform = (m[0], m[1], m[3], m[4], m[5], m[7])
    elif 33550 in tags and 33922 in tags and len(tags[33922]) >= 6:
        (sx, sy), (i, j, _, x, y) = tags[33550][:2], tags[33922][:5]
        transform = (sx, 0.0, x - i * sx, 0.0, -sy, y + j * sy)
    if transform is not None and keys.get(1025) == 2:         # RasterPixelIsPoint: the tiepoint is a pixel centre
        a, b, c, d, e, f_ = transform
        transform = (a, b, c - 0.5 * (a + b), d, e, f_ - 0.5 * (d + e))
    return (tuple(float(v) for v in transform) if transform is not None else None), epsg


def _level_info(tags, index, size):
    def one(tag, default=None):
        v = tags.get(tag)
        return default if v is None or len(v) == 0 else int(v[0])
    who = f'IFD {index}'
    info = LevelInfo()
    info.index = index
    w, h = one(256), one(257)
    if not w or not h:
        raise ValueError(f'{who} has no ImageWidth / ImageLength')
    info.shape = (h, w)
    info.bands = spp = one(277, 1)
    if spp > 16:
        raise ValueError(f'{who} has {spp} bands: more than 16 bands are not read')
    comp = one(259, 1)
    if comp not in _COMPRESSION_NAMES:
        name = _FOREIGN_COMPRESSION.get(comp, 'unknown')
        raise ValueError(f'{who} is compressed with {name} (Compression = {comp}): only none (1), LZW (5) and deflate (8, 32946) are read'
                         + ('; JPEG blocks are out of scope' if 'JPEG' in name else ''))
    info.compression = _COMPRESSION_NAMES[comp]
    bits = tuple(int(v) for v in tags.get(258, (1,)))
    fmts = tuple(int(v) for v in tags.get(339, (1,) * len(bits)))
    if len(set(bits)) > 1 or len(set(fmts)) > 1:
        raise ValueError(f'{who} has bands of differing kinds (BitsPerSample {bits}, SampleFormat {fmts}): one kind per file is read')
    if bits[0] not in (8, 16, 32):
        raise ValueError(f'{who} has {bits[0]} bits per sample: 8, 16 and 32 are read')
    if (bits[0], fmts[0]) not in _KIND_OF_FORMAT:
        raise ValueError(f'{who} has {bits[0]}-bit samples of SampleFormat {fmts[0]}: uint8, uint16, int16, int32 and float32 are read')
    info.dtype = _KIND_OF_FORMAT[(bits[0], fmts[0])]
    pred = one(317, 1)
    if pred == 3:
        raise ValueError(f'{who} uses predictor 3 (floating-point), which is not read; predictor 1 and 2 are')
    if pred not in (1, 2) or (pred == 2 and info.dtype == 'float32'):
        raise ValueError(f'{who} uses predictor {pred} on {info.dtype} samples: 1 (none) and 2 (integer kinds) are read')
    info.predictor = pred == 2
    info.planar = one(284, 1)
    if info.planar not in (1, 2):
        raise ValueError(f'{who} has PlanarConfiguration {info.planar}')
    info.tiled = 322 in tags
    if info.tiled:
        bw, bh = one(322), one(323)
        offs, cnts = tags.get(324), tags.get(325)
    else:
        bw, bh = w, min(one(278, h) or h, h)
        offs, cnts = tags.get(273), tags.get(279)
    if not bw or not bh or offs is None or cnts is None:
        raise ValueError(f'{who} has no complete block list (tile or strip shape, offsets and byte counts)')
    info.block_shape = (bh, bw)
    nblocks = -(-h // bh) * -(-w // bw) * (spp if info.planar == 2 else 1)
    info.offsets, info.counts = np.asarray(offs, np.int64).reshape(-1), np.asarray(cnts, np.int64).reshape(-1)
    if info.offsets.size != nblocks or info.counts.size != nblocks:
        raise ValueError(f'{who} needs {nblocks} blocks, its lists have {info.offsets.size} offsets and {info.counts.size} byte counts')
    bad = np.nonzero((info.offsets + info.counts > size) | (info.counts < 0))[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f'{who}: block {i} at offset {int(info.offsets[i])} with {int(info.counts[i])} bytes points past the end of the file ({size} bytes)')
    if bh * bw * (spp if info.planar == 1 else 1) * (bits[0] // 8) >= 1 << 30:
        raise ValueError(f'{who} has blocks of {bh} x {bw}: blocks stay below 2^30 bytes')
    nd = tags.get(42113)
    info.nodata = None
    if nd is not None:
        try:
            info.nodata = float(bytes(nd).split(b'\0')[0].decode('ascii').strip())
        except ValueError:
            pass
    info.transform, info.epsg = _geo(tags)
    info.overview = bool(one(254, 0) & 1)
    return info


def read_info(path):
    """[LevelInfo] of every IFD of a GeoTIFF, in file order (a COG: the full resolution, then its overviews).  Only the container is
    read.  ValueError, naming what the file has, for: a big-endian (MM) file, BigTIFF, a compression other than none / LZW / deflate,
    predictor 3, bits per sample other than 8 / 16 / 32, bands of differing kinds, more than 16 bands, and block offsets or byte counts
    that point past the end of the file."""
    import os
    size = os.path.getsize(path)
    with open(path, 'rb') as f:
        head = f.read(8)
        if len(head) < 8 or head[:2] not in (b'II', b'MM'):
            raise ValueError(f'{path} is not a TIFF file')
        if head[:2] == b'MM':
            raise ValueError(f'{path} is a big-endian (MM) TIFF: only little-endian (II) files are read')
        version = struct.unpack('<H', head[2:4])[0]
        if version == 43:
            raise ValueError(f'{path} is a BigTIFF (version 43): only classic TIFF (version 42) is read')
        if version != 42:
            raise ValueError(f'{path} has TIFF version {version}, expected 42')
        pos = struct.unpack('<I', head[4:8])[0]
        infos, seen = [], set()
        while pos:
            if pos in seen:
                raise ValueError(f'{path}: the IFD chain loops at offset {pos}')
            seen.add(pos)
            tags, pos = _parse_ifd(f, pos, size, len(infos))
            infos.append(_level_info(tags, len(infos), size))
    if not infos:
        raise ValueError(f'{path} has no image')
    return infos


def _levels(infos):
    """the image and its overview chain: IFD 0, then every IFD marked as an overview"""
    return [infos[0]] + [i for i in infos[1:] if i.overview]


def _window_transform(base, full_hw, level_hw, row0, col0):
    if base is None:
        return None
    a, b, c, d, e, f = base
    sx, sy = full_hw[1] / level_hw[1], full_hw[0] / level_hw[0]
    a, b, d, e = a * sx, b * sy, d * sx, e * sy
    return (a, b, c + col0 * a + row0 * b, d, e, f + col0 * d + row0 * e)


def _plan_read(info, window, bands):
    """-> (row0, col0, h, w), band list, file indices of the blocks the window touches (row-major; planar 2: band after band)"""
    H, W = info.shape
    if window is None:
        window = (0, 0, H, W)
    if len(window) != 4 or any(isinstance(v, bool) or int(v) != v for v in window):
        raise ValueError(f'window is four integers (row0, col0, h, w), got {window!r}')
    row0, col0, h, w = (int(v) for v in window)
    if row0 < 0 or col0 < 0 or h < 1 or w < 1 or row0 + h > H or col0 + w > W:
        raise ValueError(f'window {(row0, col0, h, w)} lies outside the image of {H} x {W}')
    if bands is None:
        bands = list(range(info.bands))
    bands = [int(b) for b in bands]
    if not bands or len(set(bands)) != len(bands) or min(bands) < 0 or max(bands) >= info.bands:
        raise ValueError(f'bands must be distinct indices below {info.bands}, got {bands}')
    bh, bw = info.block_shape
    across = info.across
    plane = [by * across + bx for by in range(row0 // bh, (row0 + h - 1) // bh + 1) for bx in range(col0 // bw, (col0 + w - 1) // bw + 1)]
    blocks = plane if info.planar == 1 else [b * across * info.down + t for b in sorted(bands) for t in plane]
    return (row0, col0, h, w), bands, blocks


def _expected_bytes(info, blocks):
    """per block the bytes it must decode to: a full block, but only the rows inside the image for the last strip"""
    if info.tiled:
        return [info.block_bytes] * len(blocks)
    bh, bw = info.block_shape
    return [min(bh, info.shape[0] - (t % info.down) * bh) * bw * info.block_samples * info.itemsize for t in blocks]
