"""Writes the foreign GeoTIFF fixtures of tests/test_raster_read_cpu.py and tests/test_raster_read_gpu.py into tests/golden/tiff_read/:
stripped LZW files made by libtiff (through Pillow), so that the reader meets streams that this library's own coder never emits
(libtiff's encoder places its Clears by compression ratio), and tiff_read/expected.npz with the pixels that went in.

    python tests/golden/make_tiff_fixtures.py

The tests read only the committed files; Pillow is needed here alone."""
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tiff_read')


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:70, 0:90]
    smooth16 = (yy * 300 + xx * 170 + rng.integers(0, 6, (70, 90))).astype(np.uint16)
    images = {
        'classes_u8': np.kron(rng.integers(0, 4, (7, 9), dtype=np.uint8), np.ones((10, 10), np.uint8)),             # 70 x 90, values 0-3
        'noise_u16': rng.integers(0, 65536, (70, 90), dtype=np.uint16),
        'rgb_u8': np.stack([(yy * 3 + xx) % 256, (yy + xx * 2) % 256, rng.integers(0, 256, (70, 90))], -1).astype(np.uint8),
        'zeros_u8': np.zeros((300, 300), np.uint8),                                                                   # two strips, the longest strings
        'smooth_u16_pred2': smooth16,
    }
    for name, a in images.items():
        im = Image.fromarray(a)          # uint8 -> L / RGB, uint16 -> I;16
        kw = {'tiffinfo': {317: 2}} if name.endswith('pred2') else {}
        im.save(os.path.join(OUT, name + '.tif'), compression='tiff_lzw', **kw)
    np.savez_compressed(os.path.join(OUT, 'expected.npz'), **images)


if __name__ == '__main__':
    main()
