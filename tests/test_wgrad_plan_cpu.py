"""The weight-gradient planner, asked on the host (satcv_conv2d_wgrad_plan_info: the launch path's own decision chain, nothing launched, no
device touched): every entry of tests/wgrad_cases.py reaches the template instantiation it names, the table as a whole reaches every
instantiation conv_wgrad.hip can choose, and the plan of the benchmark's fourteen weight-gradient launches is pinned."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import wgrad_cases as W  # noqa: E402


def workspace(d):
    from satellite_computervision_amd._lib import lib
    return int(lib.satcv_conv2d_wgrad_workspace(C.byref(d)))


def check_workspace(c, got):
    """satcv_conv2d_wgrad_workspace == nsplit * ntaps * kpad * npad * 4 of the planned launch -- or, for a 3x3 layer, of its per-tap 1x1
    plan where that one is larger (the library reserves room for the fallback of strongly dilated layers)"""
    own = got['nsplit'] * got['ntaps'] * got['kpad'] * got['npad'] * 4
    assert got['ws_bytes'] == own, (c['name'], got)
    nb = workspace(W.make_desc(c))
    if c['k'] == 3 and not got['per_tap']:
        t = W.plan_info(W.make_desc(dict(c, k=1)))
        assert nb == max(own, t['nsplit'] * t['kpad'] * t['npad'] * 4), (c['name'], nb, got, t)
    elif got['per_tap']:        # the query describes the 1x1 launches that run; the workspace is also sized for the refused 3x3 plan
        assert nb >= own, (c['name'], nb, got)
    else:
        assert nb == own, (c['name'], nb, got)
    assert 0 < got['lds_bytes'] <= 160 * 1024


@pytest.mark.parametrize('c', W.CASES, ids=[c['name'] for c in W.CASES])
def test_case_reaches_its_instantiation(c):
    with W.options(c['opts']):
        got = W.check_plan(c)
        check_workspace(c, got)


def test_table_reaches_every_instantiation():
    reached = set()
    for c in W.CASES:
        with W.options(c['opts']):
            reached.add(W.plan_info(W.make_desc(c))['key'])
    assert not set(W.UNREACHABLE) - W.ALL_KEYS
    assert reached == W.ALL_KEYS - set(W.UNREACHABLE), (sorted(W.ALL_KEYS - set(W.UNREACHABLE) - reached), sorted(reached - W.ALL_KEYS))


def test_every_template_sees_every_feature():
    """dual source + affine, cin below the stored count, accumulate, defer_reduce, whole_chip and each slab-sum kernel on each of the four
    kernel templates, minus the pairs the planner forbids (named in wgrad_cases.py)"""
    seen = {}
    for c in W.CASES:
        with W.options(c['opts']):
            g = W.plan_info(W.make_desc(c))
        t = g['kernel'] + ('-m16' if g['m16'] else '')
        s = seen.setdefault(t, set())
        s |= {k for k in ('affine', 'accumulate', 'defer_reduce', 'whole_chip') if c[k]}
        s |= {'dual'} if c['c1'] else set()
        s |= {'cin<stored'} if c['cin'] < c['c0'] + c['c1'] else set()
        s.add(g['reduce'])
    full = {'affine', 'dual', 'accumulate', 'defer_reduce', 'whole_chip', 'cin<stored', 'generic', 'reduce4', 'reduce16'}
    assert seen['single'] == full and seen['db'] == full, seen
    assert seen['dma'] == seen['dma-m16'] == full - {'cin<stored', 'generic'}, seen


def test_whole_chip_changes_the_slab_count():
    """`wgs = whole_chip ? 256 : wgrad_wgs`: on the double-buffered and the DMA kernels the flag doubles the slab count of a launch with 8
    blocks; the single-buffered kernel's slab count does not depend on it.  Both counts are pinned in the table."""
    for off, on in W.WHOLE_CHIP_PAIRS:
        if off.startswith('startup'):
            continue                                                   # the child process checks that pair
        a, b = W.BY_NAME[off], W.BY_NAME[on]
        assert {k: v for k, v in a.items() if k not in ('name', 'whole_chip', 'nsplit', 'reduce')} == \
               {k: v for k, v in b.items() if k not in ('name', 'whole_chip', 'nsplit', 'reduce')} and not a['whole_chip'] and b['whole_chip']
        with W.options(a['opts']):
            ga, gb = W.check_plan(a), W.check_plan(b)
        if ga['kernel'] == 'single':
            assert ga['nsplit'] == gb['nsplit'] == 32
        else:
            assert (ga['nsplit'], gb['nsplit']) == (16, 32), (off, ga['nsplit'], gb['nsplit'])
    assert {W.BY_NAME[on]['key'][1] + str(W.BY_NAME[on]['key'][-1]) for _, on in W.WHOLE_CHIP_PAIRS} == {'single0', 'db0', 'dma0', 'dma1'}


def test_dma_neighbours_fall_to_another_form():
    """the LDS-DMA kernel takes whole tiles only: ragged maps, a partial last image group, real channels below the stored count and a halo
    tile beyond its register staging all plan another kernel with its OWN slab geometry"""
    base = W.BY_NAME['dma-m16_0-tw32-w']
    assert W.check_plan(base)['dma'] == 1
    for change in (dict(h=5), dict(w=60), dict(cin=56), dict(n=2, h=2), dict(n=3, h=2), dict(dil=2), dict(dtype=W.F32)):
        g = W.plan_info(W.make_desc(dict(base, **change)))
        assert g['dma'] == 0 and (g['nci'], g['nco'], g['ntaps']) == (1, 4, 9) and g['npad'] == 128 and g['kpad'] == 64 and g['n_ci_blk'] == 2, (change, g)


def test_startup_option_cases_in_a_fresh_process():
    """wgrad_dma / wgrad_pix256 / wgrad_wgs are read when the library loads: ONE child with the environment of wgrad_cases.STARTUP_OPTS.
    The child's slab counts under wgrad_wgs = 64 must differ from this process's (default 128) for the same descriptors, and whole_chip
    must override the option there too."""
    code = (f'import sys, json; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import wgrad_cases as W, test_wgrad_plan_cpu as T\n'
            'ns = {}\n'
            'for c in W.STARTUP_CASES:\n'
            '    with W.options(c["opts"]):\n'
            '        g = W.check_plan(c); T.check_workspace(c, g); ns[c["name"]] = g["nsplit"]\n'
            'print("CHILD-OK", json.dumps(ns))')
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **W.startup_env(W.STARTUP_OPTS)), capture_output=True, text=True, timeout=300)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ''
    assert r.returncode == 0 and last.startswith('CHILD-OK '), (r.stdout[-2000:], r.stderr[-3000:])
    ns = json.loads(last[len('CHILD-OK '):])
    assert sorted(ns) == sorted(c['name'] for c in W.STARTUP_CASES)
    for dflt, wgs64 in W.WGS_PAIRS:
        a, b = W.BY_NAME[dflt], W.BY_NAME[wgs64]
        assert all(a[k] == b[k] for k in ('n', 'h', 'w', 'c0', 'c1', 'cin', 'cout', 'k', 'dil', 'f', 'dtype', 'whole_chip'))
        here = W.plan_info(W.make_desc(a))['nsplit']
        assert here == 2 * ns[wgs64], (dflt, here, wgs64, ns[wgs64])           # 128 / nblk against 64 / nblk
    assert (ns['startup-wgs-64-shared-chip'], ns['startup-wgs-64-whole-chip']) == (8, 32)
    # ... and in THIS process the startup-only switches cannot be moved
    from satellite_computervision_amd._lib import lib
    for k in W.STARTUP_ENV:
        assert lib.satcv_set_option(k.encode(), 0) != 0


def test_benchmark_launches_are_pinned():
    """bench.py's step -- get_unet_model(2, 4), 256 x 256, batch 64, bf16 -- and the satcv_conv2d_wgrad launches engine.py's wgrad_step
    builds for it: fourteen (the thin 32- / 64-filter layers run the fused backward kernels).  Their kernel form, slab count and slab sum
    today; a change of the plan must change wgrad_cases.BENCH_LAUNCHES knowingly."""
    assert len(W.BENCH_LAUNCHES) == 14
    for c in W.BENCH_LAUNCHES:
        assert c['nsplit'] is not None and c['reduce'] is not None
        check_workspace(c, W.check_plan(c))
    assert [c['key'][1] for c in W.BENCH_LAUNCHES].count('dma') == 10


def test_plan_query_refuses_what_the_launch_refuses():
    from satellite_computervision_amd import _lib
    info = _lib.WgradPlanInfo()
    for change in (dict(k=5), dict(c0=12), dict(cin=999), dict(n=0), dict(f=2, k=3)):
        c = dict(W.BY_NAME['db-22-tw16-w'], **change)
        d = W.make_desc(c)
        if change == dict(f=2, k=3):
            d.kh = d.kw = 3
        assert _lib.lib.satcv_conv2d_wgrad_plan_info(C.byref(d), C.byref(info)) != 0, change
    assert _lib.lib.satcv_conv2d_wgrad_plan_info(None, C.byref(info)) != 0
