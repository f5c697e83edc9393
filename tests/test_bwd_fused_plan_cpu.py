"""The dispatchers of the two fused backward kernels, asked on the host (satcv_conv2d_bwd_fused_plan_info, satcv_convt_bwd_fused_plan_info: the
launch path's own chain -- bwdf_shape_ok / bwdf_dispatch / bwdf_launch, ctbf_dispatch / ctbf_launch --, nothing launched, no device touched; the
CU count is passed in: 256).  No GPU needed.

  * every case of tests/bwd_fused_cases.py reaches the instantiation it names, and the union of the reached keys is ALL_KEYS, in both directions;
  * the cases cover every feature of FEATURES, for each kernel;
  * the multi-tile cases give every workgroup (slab) at least 2 (3) tiles and some one more, with row ends and image ends inside the ranges;
  * the reported workspace is workgroups x 9 x CIN x COUT x 4 bytes (slabs x cin x 4 cout x 4), what the workspace query answers where a device
    is present, and the dynamic LDS fits;
  * every descriptor of REFUSED, the nearest one outside a limit, is refused, and its neighbour inside is served;
  * the query needs no device, and with one leaves no HIP error behind.
"""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import bwd_fused_cases as W  # noqa: E402


@pytest.fixture(scope='module')
def reached():
    """{name: plan} of every case, each checked against the table"""
    return {c['name']: W.check_plan(c) for c in W.CASES}


def test_every_case_reaches_its_key(reached):
    assert len(reached) == len(W.CASES) >= 60


def test_reached_keys_are_all_keys(reached):
    got = {g['key'] for g in reached.values()}
    assert not (W.ALL_KEYS - got), f'keys of ALL_KEYS no case reaches: {sorted(W.ALL_KEYS - got)}'
    assert not (got - W.ALL_KEYS), f'reached keys that ALL_KEYS does not list: {sorted(got - W.ALL_KEYS)}'
    assert len(W.ALL_KEYS) == 9


def test_the_cases_cover_every_feature():
    for kind, want in W.FEATURES.items():
        seen = set()
        for c in W.CASES:
            if c['kind'] == kind:
                seen |= W.features(c)
        assert not (set(want) - seen), f'{kind}: no case with {sorted(set(want) - seen)}'
        assert not (seen - set(want)), f'{kind}: features {sorted(seen - set(want))} are not in FEATURES'


def test_every_key_has_a_multi_tile_and_a_one_tile_case(reached):
    for key in W.ALL_KEYS:
        mine = [c for c in W.CASES if c['key'] == key]
        multi = [c for c in mine if c['multi']]
        assert multi and any('one_tile' in W.features(c) for c in mine), key
        for c in multi:       # (check_plan asserted the conditions; the numbers the table's docstring quotes for 256 CUs)
            g = reached[c['name']]
            assert (g['tiles_min'], g['tiles_max']) == ((2, 3) if c['kind'] == 'bwdf' else (3, 4)), (c['name'], g)
        # the fused sums ride along wherever the form has them, and half the multi-tile cases leave their slabs to the batched sum
        assert all(bool(c['bst']) == bool(key[0] == 'ctbf' or W.BWDF_SUMS[c['form']]) for c in multi), key
    multi = [c for c in W.CASES if c['multi']]
    assert sum(c['defer'] for c in multi) == len(multi) // 2
    g = reached['multi-32-32']
    assert (g['tiles'], g['workgroups']) == (625, 256)          # 113 workgroups of 3 tiles, 143 of 2
    assert [reached[n]['slabs'] for n in ('multi-c32', 'multi-c32-two-blocks', 'multi-c64-128', 'multi-c64-64-three-blocks')] == [256, 128, 256, 85]


def test_small_maps_shrink_the_grid_to_the_tile_count(reached):
    for c in W.CASES:
        if not c['multi']:
            g = reached[c['name']]
            assert g['workgroups'] == g['tiles'] and g['tiles_min'] == g['tiles_max'] == 1, (c['name'], g)


def test_cu_count_moves_the_tile_ranges_only():
    for name in ('multi-32-32', 'multi-c64-64-three-blocks'):
        c = W.BY_NAME[name]
        a, b = W.plan_info(c['kind'], W.make_desc(c), 256), W.plan_info(c['kind'], W.make_desc(c), 304)
        assert a['key'] == b['key'] == c['key'] and a['tiles'] == b['tiles'] and a['lds_bytes'] == b['lds_bytes']
        assert b['workgroups'] == (304 if c['kind'] == 'bwdf' else 101) and b['tiles_min'] == 2
    c = W.BY_NAME['multi-32-32']
    assert W.plan_info('bwdf', W.make_desc(c), 1)['tiles_max'] == 625 and W.plan_info('bwdf', W.make_desc(c), 1 << 30)['workgroups'] == 625


@pytest.mark.parametrize('row', W.REFUSED, ids=[r[0].replace(' ', '-') for r in W.REFUSED])
def test_refused_neighbours(row):
    label, base, change, refused = row
    c = W.BY_NAME[base]
    d = W.make_desc(c)
    for k, v in change.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    got = W.plan_info(c['kind'], d)
    assert (got is None) == refused, f"{label}: {'served by ' + str(got['key']) if got else 'refused'}"
    # the workspace query agrees wherever it can answer without a device (the transposed-conv one plans for 256 CUs then)
    if c['kind'] == 'ctbf':
        from satellite_computervision_amd._lib import lib
        assert (lib.satcv_convt_bwd_fused_workspace(C.byref(d)) < 0) == refused, label


def test_invalid_queries_and_no_device_needed():
    from satellite_computervision_amd import _lib
    lib = _lib.lib
    c = W.BY_NAME['one-tile-32-32']
    d, info = W.make_desc(c), _lib.BwdfPlanInfo()
    assert lib.satcv_conv2d_bwd_fused_plan_info(None, W.NCU, C.byref(info)) == -1
    assert lib.satcv_conv2d_bwd_fused_plan_info(C.byref(d), W.NCU, None) == -1
    assert lib.satcv_conv2d_bwd_fused_plan_info(C.byref(d), -1, C.byref(info)) == -1
    t = W.BY_NAME['one-tile-c32']
    dt, it = W.make_desc(t), _lib.CtbfPlanInfo()
    assert lib.satcv_convt_bwd_fused_plan_info(None, W.NCU, C.byref(it)) == -1
    assert lib.satcv_convt_bwd_fused_plan_info(C.byref(dt), W.NCU, None) == -1
    assert lib.satcv_convt_bwd_fused_plan_info(C.byref(dt), -1, C.byref(it)) == -1
    for k in ('n', 'h', 'w_'):
        for kind, base in (('bwdf', c), ('ctbf', t)):
            z = W.make_desc(base)
            setattr(z, k, 0)
            assert W.plan_info(kind, z) is None, (kind, k)
    # with a CU count the query makes no HIP call: it answers on a machine without a device (every test of this module ran that way there), where
    # ncu = 0 -- ask the device, as the launch does -- fails cleanly for the thin-layer kernel and plans for 256 CUs for the transposed-conv one,
    # as its workspace query always did.  With a device the runtime's last-error slot must be clean after both kinds of query
    import torch
    if torch.cuda.is_available():
        # (the runtime this process uses: the copy beside torch, as _lib.py loads it; a machine where it cannot be found keeps the other assertions)
        path = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so')
        try:
            hip = C.CDLL(path if os.path.exists(path) else 'libamdhip64.so')
        except OSError:
            hip = None
        torch.cuda.init()
        if hip is not None:
            hip.hipGetLastError()               # (clear whatever earlier tests of the session left)
        assert W.check_plan(c)['workgroups'] == 1 and W.check_plan(t)['slabs'] == 1
        assert lib.satcv_conv2d_bwd_fused_plan_info(C.byref(d), 0, C.byref(info)) == 0 and lib.satcv_convt_bwd_fused_plan_info(C.byref(dt), 0, C.byref(it)) == 0
        assert hip is None or hip.hipPeekAtLastError() == 0
    else:
        assert lib.satcv_conv2d_bwd_fused_plan_info(C.byref(d), 0, C.byref(info)) == -2 and b'device' in lib.satcv_last_error()
        assert lib.satcv_convt_bwd_fused_plan_info(C.byref(dt), 0, C.byref(it)) == 0 and it.slabs == 1
        assert W.check_plan(c)['workgroups'] == 1 and W.check_plan(t)['slabs'] == 1
