"""The forward / data-gradient convolution dispatcher, asked on the host (satcv_conv2d_igemm_plan_info: the launch path's own decision chain --
igemm_dispatch of csrc/conv_igemm.hip --, nothing launched, no device touched; the CU count is passed in: 256).  No GPU needed.

  * every case of tests/conv_cases.py reaches the instantiation it names, the startup-option sets in one fresh child process each;
  * the union of the reached keys is ALL_KEYS minus UNREACHABLE, in both directions;
  * every kernel family sees every feature it accepts (ACCEPTS), and the pairs the chain forbids are refused or fall where REFUSED says;
  * lds_bytes <= 160 KB everywhere;
  * query and satcv_conv2d_igemm_pipelined agree on pipelined versus generic for the bf16 cases with a plain store;
  * the key and workgroup count of every launch of bench.py's workload, from a hand-built descriptor, are the pinned ones;
  * the e4m3 storage types: every reachable key has a value case, the shapes bf16 hands to the generic kernel are refused (REFUSALS), and the
    conditions the bit-exact e4m3 runs rest on -- multiplier bound, sensitivity, saturated share -- hold on the float64 reference.
"""
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
import conv_cases as W  # noqa: E402

# what each family's launcher accepts, read off its refusals (conv_igemm_*.hip, conv_thin_roles.hip, conv_transpose_thin.hip).  Not accepted
# anywhere: a fused max-pool of 3 (every tile height is a power of two: `TH % pool_f`).  The pairs a family refuses:
#   ws / tr     no depth-to-space / space-to-depth, stride, fused sums; tr no accumulate, no pair store; ws accumulate = 1 only, bare
#   m16 / m16p  3x3, dilation 1, unit stride, plain store; no multiplier, no pool (m16 takes ReLU, both accumulate modes and the pair store);
#               m16p also no ReLU, accumulate, pair store
#   convt_thin  the 2 x 2 transposed conv alone: loader affine, bias, multiplier + ReLU (without statistics), statistics
#   its dgrad   bare, or the fused sums over ONE raw-output tensor
#   generic     no multiplier / pool / fused sums / pair store (satcv_conv2d_igemm refuses them there); any depth-to-space factor
ACCEPTS = {
    'fast': set(W.FEATURES),
    'generic': {'bias', 'stats', 'dual', 'affine', 'out_relu', 'acc1', 'acc2', 'd2s2', 'd2s3', 's2d2', 's2d3', 'stride2', 'dilated', 'ragged_cout', 'padded_cin'},
    'm16': {'bias', 'stats', 'dual', 'affine', 'out_relu', 'acc1', 'acc2', 'pair', 'bst1', 'bst2', 'bst_lin', 'policy2', 'padded_cin'},
    'm16p': {'bias', 'stats', 'dual', 'affine', 'bst1', 'bst2', 'bst_lin', 'policy2', 'padded_cin'},
    'ws': {'bias', 'stats', 'dual', 'affine', 'out_relu', 'out_scale', 'acc1', 'pool2', 'pair', 'dilated', 'padded_cin'},
    'tr': {'bias', 'stats', 'dual', 'affine', 'out_relu', 'out_scale', 'pool2', 'padded_cin'},
    'convt_thin': {'bias', 'stats', 'affine', 'out_relu', 'out_scale', 'd2s2'},
    'convt_thin_dgrad': {'stats', 'bst1', 's2d2'},
}


# the e4m3 storage types: what the table SHOWS each family (every feature the folded fp8 plan emits, and the three the C API accepts beside
# them: a dual source on a tiled form, with the loader affine, and a padded Cin).  Statistics, fused sums, accumulate, stride and
# space-to-depth are accepted by the tiled forms too, but no lowering produces them in e4m3 and no case runs them.
_E = {'bias', 'out_relu', 'out_scale'}
SHOWN_E4M3 = {
    (W.FP8, 'fast'): _E | {'pool2', 'pair', 'd2s2', 'dilated', 'centre_tap', 'dual', 'affine', 'padded_cin'},      # (feat-fp8-ragged-cout: 48 of cout_pad = 64
                                                                                                                     #  columns, whole 16-byte vectors -- not the feature 'ragged_cout', cout % 16 != 0)
    (W.FP8X, 'fast'): _E | {'pool2', 'pair', 'd2s2', 'dilated', 'centre_tap'},
    (W.FP8, 'ws'): _E | {'pool2', 'pair', 'dual', 'affine'},
}


def all_cases():
    return W.CASES + [c for s in W.STARTUP_SETS for c in s['cases']]


def run_cases(cases):
    """[(name, key, family, lds_bytes)] of the cases, each checked against the table, under the options this process has"""
    out = []
    for c in cases:
        with W.options(c['opts']):
            g = W.check_plan(c)
        out.append((c['name'], list(g['key']), g['family'], g['lds_bytes']))
    return out


def child_main(i):
    print('CHILD-OK ' + json.dumps(run_cases(W.STARTUP_SETS[i]['cases'])))


@pytest.fixture(scope='module')
def reached():
    """every case checked against its key; returns the rows of run_cases over the main table and the startup sets"""
    rows = run_cases(W.CASES)
    for i, s in enumerate(W.STARTUP_SETS):
        code = f'import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import test_conv_plan_cpu as T; T.child_main({i})'
        r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **W.startup_env(s['opts'])), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (s['opts'], r.stdout[-2000:], r.stderr[-3000:])
        last = r.stdout.strip().splitlines()[-1]
        assert last.startswith('CHILD-OK '), r.stdout[-2000:]
        got = json.loads(last[len('CHILD-OK '):])
        assert len(got) == len(s['cases'])
        rows += [tuple(g) for g in got]
    return rows


def test_every_case_reaches_its_key(reached):
    assert len(reached) == len(all_cases())


def test_reached_keys_are_all_keys_minus_unreachable(reached):
    got = {tuple(k) for _, k, _, _ in reached}
    want = W.ALL_KEYS - set(W.UNREACHABLE)
    assert not (want - got), f'keys of ALL_KEYS no case reaches: {sorted(want - got, key=str)}'
    assert not (got - want), f'reached keys that ALL_KEYS does not list (or lists as unreachable): {sorted(got - want, key=str)}'
    assert set(W.UNREACHABLE) <= W.ALL_KEYS and all(len(r) > 40 for r in W.UNREACHABLE.values())


def test_every_family_sees_every_feature_it_accepts(reached):
    fam = {name: f for name, _, f, _ in reached}
    seen, seen8 = {}, {}
    for c in all_cases():
        if c['dtype'] in (W.FP8, W.FP8X):
            seen8.setdefault((c['dtype'], fam[c['name']]), set()).update(W.features(c))
        else:
            seen.setdefault(fam[c['name']], set()).update(W.features(c))
    for f, acc in ACCEPTS.items():
        assert acc <= seen[f], f'{f}: no case with {sorted(acc - seen[f])}'
        assert seen[f] <= acc, f'{f} served {sorted(seen[f] - acc)}, which ACCEPTS says it refuses'
    assert seen8 == SHOWN_E4M3, {k: sorted(v ^ SHOWN_E4M3.get(k, set())) for k, v in seen8.items()}


def test_lds_fits(reached):
    for name, _, _, lds in reached:
        assert 0 < lds <= 160 * 1024, (name, lds)


def plain_store(c):
    return not (c['out_scale'] or c['pool_f'] or c['bst'] or c['pair'])


def test_query_and_pipelined_agree():
    """satcv_conv2d_igemm_pipelined asks igemm_fast_launch alone (and the weights-stationary kernel for dilation-3 launches with fused sums); the
    launch asks the transposed-conv streaming kernels, the wave-role kernel and the weights-stationary kernel first.  For every bf16 case of the
    main table with a plain store the two agree: whatever those four take, igemm_fast_launch would have taken too."""
    from satellite_computervision_amd._lib import lib
    n = 0
    for c in W.CASES:
        if c['dtype'] != W.BF16 or not plain_store(c):
            continue
        # (m16p = 0 for both: satcv_conv2d_igemm_pipelined has no CU count to hand to the persistent 16x16x32 kernel and asks the device, which is
        #  not there in this test; with a device the GPU test compares the two under the case's own options)
        with W.options(dict(c['opts'], m16p=0)):
            d = W.make_desc(c)
            p, fam = lib.satcv_conv2d_igemm_pipelined(C.byref(d)), W.plan_info(d)['family']
        assert p == (fam != 'generic'), (c['name'], fam, p)
        n += 1
    assert n > 150


def test_pipelined_answers_no_where_only_the_streaming_kernel_carries_the_fused_sums():
    """the one place where satcv_conv2d_igemm_pipelined and the launch part (found by the GPU run of this table): a transposed conv's data gradient
    with fused sums on a map whose height is no multiple of the tile height.  The tiled kernel forms the sums on whole tiles only, so
    igemm_fast_launch -- all that satcv_conv2d_igemm_pipelined asks -- refuses; convt_thin_dgrad_launch, which the launch asks first, takes any
    height.  The answer 0 is the careful one: the caller keeps its separate reduce pass, no result changes."""
    from satellite_computervision_amd._lib import lib
    for name, want in (('convt-thin-dgrad-128-64-bst', 0), ('convt-thin-dgrad-128-64', 1)):
        c = W.BY_NAME[name]
        d = W.make_desc(c)
        assert W.plan_info(d)['family'] == 'convt_thin_dgrad' and lib.satcv_conv2d_igemm_pipelined(C.byref(d)) == want, name
    whole = dict(W.BY_NAME['convt-thin-dgrad-128-64-bst'], h=8)
    assert lib.satcv_conv2d_igemm_pipelined(C.byref(W.make_desc(whole))) == 1


def test_bench_launches_run_the_pinned_forms():
    assert len(W.BENCH_LAUNCHES) == 35
    for c in W.BENCH_LAUNCHES:
        g = W.check_plan(c)
        assert g['workgroups'] == c['workgroups'], (c['name'], g['workgroups'])


# ------------------------------------------------------------------------------------------------ the pairs the chain forbids
def refused(**kw):
    base = dict(name='x', n=2, h=8, w=32, c0=48, c1=0, cout=64, k=3, dil=1, stride=1, mode='conv', f=1, ldy=64, bias=False, stats=False, affine=False, out_relu=False,
                out_scale=False, accumulate=0, pool_f=0, pair=False, bst=0, bst_relu=1, tile_policy=0, dtype=W.BF16, stats_ld=0)
    base.update(kw)
    if base['bst'] or base['stats']:
        base['stats'], base['stats_ld'] = True, base['cout']
    from satellite_computervision_amd import _lib
    info = _lib.ConvPlanInfo()
    return _lib.lib.satcv_conv2d_igemm_plan_info(C.byref(W.make_desc(base)), W.NCU, C.byref(info)) != 0


def test_pool_of_three_is_refused_by_every_family():
    for (h, w) in ((24, 48), (12, 96), (48, 24)):
        assert refused(h=h, w=w, pool_f=3), (h, w)
    assert not refused(h=8, w=32, pool_f=2)


def test_fused_sums_need_whole_tiles():
    assert not refused(n=2, h=4, w=64, bst=1)
    assert refused(n=2, h=5, w=64, bst=1) and refused(n=2, h=4, w=60, bst=1) and refused(n=3, h=2, w=32, bst=1)
    assert refused(n=2, h=4, w=64, bst=1, cout=48, ldy=48)          # (48 columns on a 32-column tile: a half-empty last tile)


def test_two_row_maps_have_no_pipelined_3x3_form():
    """finding of the query: at tile width 32 two images of two rows per 4-row tile stage 2 x 4 x 34 pixels, 544 items against the 512 of the
    128-pixel instantiations -- the GENERIC kernel serves them, and what needs the pipelined kernel is refused"""
    for kw in (dict(out_scale=True), dict(pair=True, n=4, ldy=128), dict(pool_f=2)):
        assert refused(n=kw.pop('n', 3), h=2, w=32, **kw), kw
    assert refused(n=3, h=2, w=32, cout=32, ldy=32, out_scale=True)              # (four images per 8-row tile: 1088 items against 1024)
    assert not refused(n=3, h=4, w=32, out_scale=True) and not refused(n=3, h=4, w=16, out_scale=True)


def test_invalid_descriptors_and_null_pointers():
    from satellite_computervision_amd import _lib
    lib, info = _lib.lib, _lib.ConvPlanInfo()
    c = W.BY_NAME['t64-9-bf16-tw32-r']
    d = W.make_desc(c)
    assert lib.satcv_conv2d_igemm_plan_info(None, W.NCU, C.byref(info)) != 0
    assert lib.satcv_conv2d_igemm_plan_info(C.byref(d), W.NCU, None) != 0
    assert lib.satcv_conv2d_igemm_plan_info(C.byref(d), -1, C.byref(info)) != 0
    for change in (dict(c0=0), dict(c0=24), dict(kh=2), dict(n=0), dict(cstat=0), dict(dil=0), dict(n=1 << 20, h=1 << 10, w_=1 << 10)):
        d = W.make_desc(c)
        for k, v in change.items():
            setattr(d, k, v)
        assert lib.satcv_conv2d_igemm_plan_info(C.byref(d), W.NCU, C.byref(info)) != 0, change
    d = W.make_desc(c)
    d.x0 = d.w = d.y = None                      # null tensors: a query reads no pointer but for its alignment
    assert W.plan_info(d)['key'] == c['key']
    d.y = 4098                                   # a misaligned output: the pipelined kernels refuse it, the generic one stores by element
    assert W.plan_info(d)['family'] == 'generic'


def test_cu_count_moves_the_persistent_kernels_only():
    c = W.BY_NAME['m16p-default-two-tiles-per-workgroup']
    assert W.plan_info(W.make_desc(c), 256)['key'] == c['key'] and W.plan_info(W.make_desc(c), 304)['family'] == 'fast'      # 512 tiles < 2 x 304
    c = W.BY_NAME['tr-32-32']
    with W.options(c['opts']):
        assert [W.plan_info(W.make_desc(c), n)['workgroups'] for n in (2, 256)] == [2, 4]


# ------------------------------------------------------------------------------------------------ the e4m3 storage types
def e4m3_cases():
    return [c for c in all_cases() if c['dtype'] in (W.FP8, W.FP8X)]


def test_every_reachable_e4m3_key_has_a_value_case():
    """no e4m3 entry is keys-only: every case runs for values on the GPU, and together they reach every e4m3 key of ALL_KEYS but the
    unreachable ones"""
    cases = e4m3_cases()
    assert len(cases) > 100 and all(c['gpu'] for c in cases), [c['name'] for c in cases if not c['gpu']]
    want = {k for k in W.ALL_KEYS - set(W.UNREACHABLE) if k[0] in (W.FP8, W.FP8X)}
    assert {c['key'] for c in cases} == want
    # every tiled form sees the whole-tile, the ragged and the several-images-per-tile shape over its tile widths (a shape that is refused, or
    # falls to another form, is in the table under the form's name all the same)
    names = {c['name'] for c in cases} | {c['name'] for c in W.REFUSALS}
    for dt, forms in ((W.FP8, [f for f in W.FAST if f not in W.BF16_ONLY]), (W.FP8X, W.FP8X_FORMS)):
        for f in forms:
            kinds = {n.rsplit('-', 1)[1] for n in names if n.startswith(f'{f}-{dt}-tw')}
            assert kinds == set('wrm'), (f, dt, kinds)


def test_e4m3_shapes_beyond_the_pipelined_kernels_are_refused():
    """the e4m3 types have no generic kernel (and the scaled form no tap loop): where bf16 falls to one, the dispatcher answers
    SATCV_ERR_UNSUPPORTED with its message, and nothing is launched.  The same shape in bf16 is served."""
    from satellite_computervision_amd import _lib
    assert len(W.REFUSALS) == 8
    for c in W.REFUSALS:
        info = _lib.ConvPlanInfo()
        rc = _lib.lib.satcv_conv2d_igemm_plan_info(C.byref(W.make_desc(c)), W.NCU, C.byref(info))
        assert rc == -3 and W.REFUSAL_MESSAGE in _lib.lib.satcv_last_error().decode(), (c['name'], rc, _lib.lib.satcv_last_error())        # SATCV_ERR_UNSUPPORTED
        b = dict(c, dtype=W.BF16, out_scale=False)
        assert W.plan_info(W.make_desc(b))['family'] in ('generic', 'fast'), c['name']


def test_e4m3_reference_conditions():
    """what the bit-exact e4m3 runs rest on, asserted on the float64 reference alone (test_conv_plan_gpu.lattice_case; no device): the
    multiplier's bound (nothing saturates, every fp32 operation exact), the sensitivity condition -- one zeroed input channel at one tap changes at
    least 5 % of the stored reference -- and, for the two saturating cases, a saturated share between 2 % and 30 %."""
    import test_conv_plan_gpu as T
    for c in e4m3_cases():
        d, ref, L, notes = T.lattice_case(c, T.case_seed(c) + 1, 'fast')
        raw = ref['raw'] * L['unit']
        assert abs(raw).max() <= L['ymax'] and (raw == raw.round()).all(), c['name']
        assert (abs(ref['raw']).max() > T.E4M3_MAX) == (c['name'] in W.E4M3_SATURATING), c['name']
        assert (abs(ref['y']) <= T.E4M3_MAX).all() and any(n.startswith('sens') for n in notes)
