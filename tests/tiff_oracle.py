"""Pure Python / NumPy restatement of the Cloud-Optimized GeoTIFF writer (include/satcv.h "Cloud-Optimized GeoTIFF writer",
satellite_computervision_amd/raster_tools.py), for tests/test_raster_cpu.py and tests/test_raster_gpu.py:

  parse_tiff / read_level   a TIFF parser: IFD chain, tags, tile assembly (LZW, Deflate, none; predictor 2)
  lzw_decode                TIFF 6.0 section 13 LZW decoder; its width rule: widen after its own table reaches 511, 1023 or 2047 entries
  lzw_encode_ref            a slow encoder of the rules satcv_lzw_tiles states, with a dict for the dictionary
  convert_ref / overview_ref / tiles_ref / pyramid_ref     the per-sample rules of satcv_raster_convert / _overview / _tiles
Nothing here imports the package under test."""
import struct
import zlib

import numpy as np

TYPE_FMT = {1: 'B', 2: 'c', 3: 'H', 4: 'I', 5: 'II', 12: 'd', 16: 'Q'}
KIND_DTYPE = {0: np.uint8, 1: np.uint16, 2: np.float32, 3: np.int16, 5: np.int32}


# ------------------------------------------------------------------------------------------------------------ LZW
class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.n += width
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xff)
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 0xff)
        return bytes(self.out)


def lzw_encode_ref(data, info=None):
    """the stream of satcv_lzw_tiles for `data`; info (a dict) receives 'final_next': the next free code after the counter step that
    follows the last data code (4094: the last code filled the table exactly), and 'clears': Clears after the opening one"""
    data = bytes(data)
    bits = _Bits()
    table, nxt, width, clears, final_next = {}, 258, 9, 0, None
    bits.put(256, width)

    def bump():
        nonlocal nxt, width, table, clears
        nxt += 1
        reached = nxt
        if nxt == 4094:
            bits.put(256, width)
            table, nxt, width = {}, 258, 9
            clears += 1
        elif nxt in (512, 1024, 2048):
            width += 1
        return reached
    prefix = None
    for b in data:
        if prefix is None:
            prefix = b
            continue
        code = table.get((prefix, b))
        if code is not None:
            prefix = code
            continue
        bits.put(prefix, width)
        table[(prefix, b)] = nxt
        bump()
        prefix = b
    if prefix is not None:
        bits.put(prefix, width)
        final_next = bump()
    bits.put(257, width)
    if info is not None:
        info['final_next'], info['clears'] = final_next, clears
    return bits.done()


def lzw_decode(stream):
    stream = bytes(stream)
    total = len(stream) * 8
    pos, width = 0, 9
    acc = int.from_bytes(stream, 'big') if stream else 0
    table = [bytes([i]) for i in range(256)] + [b'', b'']
    out = bytearray()
    prev = None
    while pos + width <= total:
        code = (acc >> (total - pos - width)) & ((1 << width) - 1)
        pos += width
        if code == 257:
            break
        if code == 256:
            table = table[:258]
            width, prev = 9, None
            continue
        if prev is None:
            entry = table[code]
        else:
            if code < len(table):
                entry = table[code]
            elif code == len(table):
                entry = prev + prev[:1]
            else:
                raise ValueError(f'LZW: code {code} beyond the table ({len(table)} entries)')
            table.append(prev + entry[:1])
        out += entry
        prev = entry
        if len(table) in (511, 1023, 2047):
            width += 1
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------ TIFF
def parse_tiff(buf):
    """-> [ifd], ifd = {'offset', 'end', 'tags': {tag: (type, count, values tuple or bytes)}, 'order': [tag], 'value_spans': [(lo, hi)]}"""
    assert buf[:4] == b'II*\0', 'little-endian classic TIFF expected'
    ifds, pos = [], struct.unpack_from('<I', buf, 4)[0]
    while pos:
        n = struct.unpack_from('<H', buf, pos)[0]
        tags, order, spans = {}, [], []
        for i in range(n):
            tag, typ, count, raw = struct.unpack_from('<HHI4s', buf, pos + 2 + 12 * i)
            size = struct.calcsize('<' + TYPE_FMT[typ]) * count
            if size > 4:
                at = struct.unpack('<I', raw)[0]
                spans.append((at, at + size))
                raw = buf[at:at + size]
            raw = raw[:size]
            values = raw if typ == 2 else struct.unpack('<%d%s' % (count, TYPE_FMT[typ]), raw)
            tags[tag] = (typ, count, values)
            order.append(tag)
        end = pos + 2 + 12 * n + 4
        ifds.append({'offset': pos, 'end': end, 'tags': tags, 'order': order, 'value_spans': spans})
        pos = struct.unpack_from('<I', buf, end - 4)[0]
    return ifds


def tag(ifd, t, default=None):
    return ifd['tags'][t][2] if t in ifd['tags'] else default


def ifd_dtype(ifd):
    bits, fmt = tag(ifd, 258)[0], tag(ifd, 339, (1,))[0]
    return np.dtype({(8, 1): np.uint8, (16, 1): np.uint16, (16, 2): np.int16, (32, 2): np.int32, (32, 3): np.float32}[(bits, fmt)])


def read_level(buf, ifd):
    """the (h, w, c) pixels of one IFD of a tiled file"""
    w, h, c = tag(ifd, 256)[0], tag(ifd, 257)[0], tag(ifd, 277)[0]
    bs = tag(ifd, 322)[0]
    assert tag(ifd, 323)[0] == bs and tag(ifd, 284, (1,))[0] == 1
    dt = ifd_dtype(ifd)
    comp, pred = tag(ifd, 259)[0], tag(ifd, 317, (1,))[0]
    nty, ntx = -(-h // bs), -(-w // bs)
    offs, cnts = tag(ifd, 324), tag(ifd, 325)
    assert len(offs) == len(cnts) == nty * ntx
    out = np.zeros((nty * bs, ntx * bs, c), dt)
    for i, (o, n) in enumerate(zip(offs, cnts)):
        raw = buf[o:o + n]
        raw = lzw_decode(raw) if comp == 5 else zlib.decompress(raw) if comp == 8 else raw
        t = np.frombuffer(raw[:bs * bs * c * dt.itemsize], dt).reshape(bs, bs, c)
        if pred == 2:
            t = np.cumsum(t.astype(np.uint64), axis=1).astype('u%d' % dt.itemsize).view(dt)      # modular in the sample's width
        out[(i // ntx) * bs:(i // ntx + 1) * bs, (i % ntx) * bs:(i % ntx + 1) * bs] = t
    return out[:h, :w]


# ------------------------------------------------------------------------------------------------------------ per-sample rules
def _nodata_as(nodata, dt):
    dt = np.dtype(dt)
    if dt.kind == 'f':
        return dt.type(nodata)
    info = np.iinfo(dt)
    return dt.type(min(max(int(nodata), info.min), info.max))


def convert_ref(src, dtype, scale=None, nodata=None):
    """satcv_raster_convert: src (h, w, c) of a kind -> (h, w, c) of dtype"""
    src, dt = np.asarray(src), np.dtype(dtype)
    if dt == np.float32:
        if src.dtype == np.float32 and scale is not None:
            return src * np.float32(scale)
        return src.astype(np.float32)
    info = np.iinfo(dt)
    if src.dtype == np.float32:
        with np.errstate(invalid='ignore', over='ignore'):
            t = src * np.float32(scale) if scale is not None else src
            r = np.rint(t)                                  # half to even, fp32
            out = np.where(r <= np.float32(info.min), info.min, np.where(r >= np.float32(info.max), info.max, 0)).astype(np.int64)
            mid = (r > np.float32(info.min)) & (r < np.float32(info.max))
            out[mid] = r[mid].astype(np.int64)
        out[np.isnan(t)] = int(_nodata_as(nodata, dt)) if nodata is not None else 0
        return out.astype(dt)
    return np.clip(src.astype(np.int64), info.min, info.max).astype(dt)


def overview_ref(src, resampling='nearest', nodata=None):
    """satcv_raster_overview: (h, w, c) -> (ceil(h / 2), ceil(w / 2), c); a plain loop, the rules word for word"""
    h, w, c = src.shape
    dt = src.dtype
    oh, ow = (h + 1) // 2, (w + 1) // 2
    out = np.zeros((oh, ow, c), dt)
    nd = _nodata_as(nodata, dt) if nodata is not None else None
    if resampling == 'nearest':
        return np.ascontiguousarray(src[::2, ::2])
    for y in range(oh):
        for x in range(ow):
            for b in range(c):
                vals = []
                for yy in (2 * y, 2 * y + 1):
                    for xx in (2 * x, 2 * x + 1):
                        if yy < h and xx < w:
                            v = src[yy, xx, b]
                            if (dt.kind == 'f' and v != v) or (nd is not None and v == nd):
                                continue
                            vals.append(v)
                if not vals:
                    out[y, x, b] = nd if nd is not None else np.float32('nan')
                elif resampling == 'average':
                    if dt.kind == 'f':
                        s = np.float32(vals[0])
                        for v in vals[1:]:
                            s = np.float32(s + np.float32(v))
                        out[y, x, b] = np.float32(s / np.float32(len(vals)))
                    else:
                        s, n = sum(int(v) for v in vals), len(vals)
                        out[y, x, b] = (2 * s + n) // (2 * n)       # Python's // is a floor
                else:
                    best = max(vals.count(v) for v in vals)
                    out[y, x, b] = min(v for v in vals if vals.count(v) == best)
    return out


def pyramid_ref(base, shapes, resampling='nearest', nodata=None):
    """[base, level 1, ...]: level k + 1 is made from level k; shapes: the expected overview shapes [(h, w)]"""
    levels = [base]
    for hw in shapes:
        levels.append(overview_ref(levels[-1], resampling, nodata))
        assert levels[-1].shape[:2] == tuple(hw)
    return levels


def tiles_ref(src, blocksize, predictor=False, nodata=None):
    """satcv_raster_tiles: (h, w, c) -> (nty * ntx, blocksize, blocksize, c)"""
    h, w, c = src.shape
    dt, bs = src.dtype, blocksize
    nty, ntx = -(-h // bs), -(-w // bs)
    pad = np.full((nty * bs, ntx * bs, c), _nodata_as(nodata, dt) if nodata is not None else 0, dt)
    pad[:h, :w] = src
    t = pad.reshape(nty, bs, ntx, bs, c).transpose(0, 2, 1, 3, 4).reshape(nty * ntx, bs, bs, c)
    if predictor:
        u = t.view('u%d' % dt.itemsize)
        d = u.copy()
        d[:, :, 1:] = u[:, :, 1:] - u[:, :, :-1]             # unsigned arithmetic wraps: modular in the sample's width
        t = d.view(dt)
    return np.ascontiguousarray(t)


def auto_shapes(h, w, blocksize):
    shapes = []
    while max(h, w) > blocksize:
        h, w = (h + 1) // 2, (w + 1) // 2
        shapes.append((h, w))
    return shapes
