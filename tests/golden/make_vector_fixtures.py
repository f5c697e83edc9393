"""Golden vectors for the window helpers of satellite_computervision_amd/polygons.py, made by RUNNING the reference's own function
bodies (utils/raster_tools.py: convert, make_window, win_jitter, make_jittered_window), extracted by AST the way
make_reference_fixtures.py does.  Only recorded inputs and outputs are written -- no reference source travels:

    python tests/golden/make_vector_fixtures.py <path of the reference checkout>

writes tests/golden/vector_helpers_reference.npz.  If the interpreter can import matplotlib.path, the file also holds
`Path.contains_points` on the pixel centres of a grid for simple (star-shaped) polygons, of which only those are kept that have no
centre within 1e-6 of an edge: an independent statement of "the centre lies inside" for tests/test_rasterize_cpu.py.
"""
import ast
import contextlib
import io
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
NAMES = ('convert', 'make_window', 'win_jitter', 'make_jittered_window')


def extract_functions(path, names):
    tree = ast.parse(open(path).read())
    ns = {'np': np}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, 'exec'), ns)
    return ns


def helper_fixtures(ref):
    f = extract_functions(os.path.join(ref, 'utils', 'raster_tools.py'), NAMES)
    rng = np.random.default_rng(20240611)
    out = {}
    sizes = rng.integers(16, 4000, (24, 2))
    boxes = np.sort(rng.uniform(0, 4000, (24, 2, 2)), axis=1).transpose(0, 1, 2).reshape(24, 4)      # x0, y0, x1, y1 with x0 <= x1, y0 <= y1
    out['convert_size'], out['convert_box'] = sizes, boxes
    out['convert_out'] = np.array([f['convert'](tuple(int(v) for v in s), list(b)) for s, b in zip(sizes, boxes)], np.float64)
    cxy = np.concatenate([rng.uniform(0, 5000, (16, 2)), rng.integers(0, 5000, (8, 2)) + 0.5])      # (halves: `round` goes to even)
    ws = rng.integers(1, 1400, 24)
    out['window_cxy'], out['window_size'] = cxy, ws
    out['window_out'] = np.array([f['make_window'](float(c[0]), float(c[1]), int(w)) for c, w in zip(cxy, ws)], np.int64)
    seeds = np.arange(24) + 7
    dims = rng.integers(1300, 6000, (24, 2))
    wsz = rng.choice([256, 512, 1280], 24)
    frac = rng.choice([0.05, 0.1, 0.2], 24)
    centres = rng.uniform(-100, 6000, (24, 2))
    jit, win = [], []
    for k in range(24):
        np.random.seed(int(seeds[k]))
        jit.append(f['win_jitter'](int(wsz[k]), jitter_frac=float(frac[k])))
        np.random.seed(int(seeds[k]))
        with contextlib.redirect_stdout(io.StringIO()):
            win.append(f['make_jittered_window'](float(centres[k, 0]), float(centres[k, 1]), int(dims[k, 0]), int(dims[k, 1]), window_size=int(wsz[k]),
                                                 jitter_frac=float(frac[k])))
    out.update(jitter_seed=seeds, jitter_dims=dims, jitter_window=wsz, jitter_frac=frac, jitter_centre=centres, jitter_out=np.array(jit, np.int64),
               jittered_window_out=np.array(win, np.int64))
    return out


def _edge_distance(px, py, ring):
    """the distance of every point to the nearest edge of the closed ring"""
    best = np.full(px.shape, np.inf)
    for k in range(len(ring)):
        (ax, ay), (bx, by) = ring[k], ring[(k + 1) % len(ring)]
        dx, dy = bx - ax, by - ay
        if dx == 0 and dy == 0:
            best = np.minimum(best, np.hypot(px - ax, py - ay))
            continue
        t =np.clip(((px - ax) * dx + (py - ay) * dy) / (dx * dx + dy * dy), 0.0, 1.0)
        best = np.minimum(best, np.hypot(px - (ax + t * dx), py - (ay + t * dy)))
    return best


def path_fixtures():
    try:
        from matplotlib.path import Path
    except Exception:
        return {}
    H, W, NV = 29, 41, 9
    rng = np.random.default_rng(99)
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    rings, inside = [], []
    while len(rings) < 40:
        ang = np.sort(rng.uniform(0, 2 * np.pi, NV))
        if np.diff(np.concatenate([ang, [ang[0] + 2 * np.pi]])).max() > 0.9 * np.pi:      # (star-shaped around the centre: a simple polygon)
            continue
        rad = rng.uniform(3, 24, NV)
        c = rng.uniform((8, 6), (W - 8, H - 6))
        ring = np.stack([c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang)], axis=1)
        if len(rings) % 2:
            ring = np.round(ring * 4) / 4
        if _edge_distance(jj, ii, ring).min() <= 1e-6:
            continue
        rings.append(ring)
        inside.append(Path(np.concatenate([ring, ring[:1]])).contains_points(np.stack([jj.ravel(), ii.ravel()], axis=1)).reshape(H, W))
    return {'path_shape': np.array([H, W]), 'path_rings': np.array(rings), 'path_inside': np.array(inside).astype(np.uint8)}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = helper_fixtures(sys.argv[1])
    out.update(path_fixtures())
    np.savez_compressed(os.path.join(OUT, 'vector_helpers_reference.npz'), **out)
    print(sorted(out))


if __name__ == '__main__':
    main()
