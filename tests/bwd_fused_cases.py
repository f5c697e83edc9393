"""Case table of the two fused backward kernels (tests/test_bwd_fused_plan_cpu.py, tests/test_bwd_fused_plan_gpu.py).

satcv_conv2d_bwd_fused (csrc/conv_bwd_fused.hip) and satcv_convt_bwd_fused (csrc/convt_bwd_fused.hip) are persistent kernels: a workgroup
(a slab of the transposed-conv kernel) owns a contiguous range of tiles and carries its weight-gradient accumulators and fused sums across
them.  An instantiation KEY names the template instantiation a descriptor runs:

    ('bwdf', cin, cout, nw, wps, pool, nodg, cins, hg)      bwd_fused_kernel        tiles of 8 x 32 pixels
    ('ctbf', cout4, px, cblk)                               convt_bwd_fused_kernel  tiles of px input pixels of one image row

ALL_KEYS is written out by hand from bwdf_dispatch and ctbf_dispatch.  CASES is the table, every entry with the key it must reach and the
features it carries.  The CPU test asks the plan queries (satcv_conv2d_bwd_fused_plan_info / satcv_convt_bwd_fused_plan_info: the launch
path's own chain, nothing launched, 256 CUs passed in) that every case lands on its key, that the keys and the features are all covered and that
every entry of REFUSED -- the nearest descriptor outside each limit of bwdf_shape_ok / ctbf_dispatch -- is refused; the GPU test runs the cases
bit-exactly on integer-lattice data.

Shapes, read off the two kernels:
    multi-tile   one per key.  bwdf: the grid is min(CUs x 1, tiles) for all six forms, so on 256 CUs 25 images of 40 x 160 are 625 tiles --
                 113 workgroups get 3, 143 get 2; rows of 5 tiles and images of 25 put row ends and image ends inside most ranges.
                 ctbf: slabs = CUs / channel blocks; 6 x 35 x 256 at 64 -> 32 is 840 tiles on 256 slabs (3 or 4 each), 3 x 35 x 256 at
                 128 -> 32 is 420 on 128, 6 x 35 x 128 at 128 -> 64 is 840 on 256, 2 x 35 x 128 at 192 -> 64 is 280 on 85 (35 rows, not 36:
                 with 36 every image end falls between two ranges on 256 CUs, and check_plan wants one inside a range).  The GPU test does
                 not trust these numbers: it asserts the tiles-per-workgroup conditions on the plan of the device it runs on.
    smallest     one tile (1 x 8 x 32; one tile per slab), and fewer tiles than CUs (the grid shrinks to the tile count: every slab of the
                 workspace is written by a workgroup that had a tile -- the NaN-filled workspace shows a slab that was summed but not written).
    features     on maps of at most 3 x 24 x 96 pixels.
"""
NCU = 256

BWDF_FORMS = {      # name: (cin, cout, nw, wps, pool, nodg, cins, hg) -- the six bwdf_launch<...> sites of bwdf_dispatch, in its order
    'pool': (32, 64, 4, 1, 1, 0, 32, 0), 'pool-nodx': (32, 32, 8, 2, 1, 1, 16, 0), 'hg': (32, 32, 8, 2, 0, 0, 32, 1),
    '32-32': (32, 32, 8, 2, 0, 0, 32, 0), '64-32': (64, 32, 8, 2, 0, 0, 64, 0), '64-64': (64, 64, 4, 1, 0, 0, 64, 0)}
CTBF_FORMS = {'c32': (128, 64, 64), 'c64-128': (256, 32, 128), 'c64-64': (256, 32, 64)}      # (cout4, px, cblk): the switch of ctbf_dispatch
# bst of the plan: the forms that carry the fused sums (not the dense one-wave-per-SIMD form, not the one without a data gradient)
BWDF_SUMS = {'pool': 1, 'pool-nodx': 0, 'hg': 1, '32-32': 1, '64-32': 1, '64-64': 0}
ALL_KEYS = {('bwdf',) + v for v in BWDF_FORMS.values()} | {('ctbf',) + v for v in CTBF_FORMS.values()}

# the features the table must cover (test_bwd_fused_plan_cpu.py asserts the union), per kernel
FEATURES = {
    'bwdf': ('multi', 'one_tile', 'few_tiles', 'dual16_16', 'dual8_24', 'dual40_24', 'dual32_32', 'affine_relu', 'affine_norelu', 'linear', 'bst', 'bst_act',
             'bst_prefill', 'accumulate', 'defer', 'wide_ldg', 'wide_lddx', 'wide_bst_ld', 'hg', 'hg_affine', 'hg_bst', 'pool_dx', 'pool_nodx', 'amax_kernel'),
    'ctbf': ('multi', 'one_tile', 'few_tiles', 'affine_relu', 'affine_norelu', 'linear', 'bst', 'bst_act', 'bst_prefill', 'accumulate', 'defer', 'wide_ldg',
             'wide_lddx', 'wide_bst_ld', 'wide_ldx', 'wide_npad'),
}

CASES = []


def bwdf(name, form, n, h, w, c0, cout, *, c1=0, cin=None, affine=0, in_relu=1, linear=0, bst='', prefill=0, accumulate=0, defer=0, ldg=None, goff=0,
         yoff=0, lddx=None, bst_ld=None, hg=0, pool='', amax='random', lddp=None, multi=0):
    """affine: the loader's in_scale / in_shift (in_relu with it); bst: '' / 'bn' (normal form) / 'act' (bst_act_form); goff / yoff: the channel
    offsets of g and yraw inside their (n, h, w, ldg) buffers; pool: '' / 'dx' / 'nodx'; amax: 'random' bytes or the ones of 'kernel'
    satcv_bn_relu_pool_amax"""
    cs = c0 + c1
    c = dict(kind='bwdf', name=name, form=form, key=('bwdf',) + BWDF_FORMS[form], n=n, h=h, w=w, c0=c0, c1=c1, cin=cin if cin is not None else cs, cout=cout,
             affine=affine, in_relu=in_relu if affine else 0, linear=linear, bst=bst, prefill=prefill, accumulate=accumulate, defer=defer,
             ldg=ldg if ldg is not None else cout, goff=goff, yoff=yoff, lddx=lddx if lddx is not None else cs, bst_ld=bst_ld if bst_ld is not None else cs,
             hg=hg, pool=pool, amax=amax, lddp=lddp if lddp is not None else cout, multi=multi)
    assert c['ldg'] >= max(goff, yoff) + cout and goff % 8 == 0 and yoff % 8 == 0 and not (bst == 'bn' and not (affine and in_relu)) and not (bst == 'act' and affine)
    CASES.append(c)


def ctbf(name, form, n, h, w, cin, cout, *, affine=0, in_relu=1, linear=0, bst='', prefill=0, accumulate=0, defer=0, ldg=None, goff=None, ldy=None, yoff=0,
         ldx=None, lddx=None, bst_ld=None, npad=None, multi=0):
    """(n, h, w): the INPUT grid.  ldg / goff: channel stride of the concatenation's gradient and the first `up` channel in it (default: cout
    skip channels in front); ldy / yoff likewise for the transposed convolution's stored output; npad: row pitch of the operand image"""
    c = dict(kind='ctbf', name=name, form=form, key=('ctbf',) + CTBF_FORMS[form], n=n, h=h, w=w, cin=cin, cout=cout, affine=affine, in_relu=in_relu if affine else 0,
             linear=linear, bst=bst, prefill=prefill, accumulate=accumulate, defer=defer, ldg=ldg if ldg is not None else 2 * cout,
             goff=goff if goff is not None else cout, ldy=ldy if ldy is not None else cout, yoff=yoff, ldx=ldx if ldx is not None else cin,
             lddx=lddx if lddx is not None else cin, bst_ld=bst_ld if bst_ld is not None else cin, npad=npad if npad is not None else cin, multi=multi)
    assert c['ldg'] >= c['goff'] + cout and c['ldy'] >= yoff + cout and c['goff'] % 8 == 0 and yoff % 8 == 0 and not (bst == 'bn' and not (affine and in_relu)) \
        and not (bst == 'act' and affine)
    CASES.append(c)


# ------------------------------------------------------------------------------------------------ multi-tile, one per key
M = dict(n=25, h=40, w=160, multi=1)
bwdf('multi-32-32', '32-32', c0=32, cout=32, affine=1, bst='bn', defer=1, **M)
bwdf('multi-hg', 'hg', c0=32, cout=32, hg=1, affine=1, bst='bn', **M)
bwdf('multi-64-32', '64-32', c0=32, c1=32, cout=32, affine=1, bst='bn', **M)
bwdf('multi-64-64', '64-64', c0=64, cout=64, affine=1, defer=1, **M)
bwdf('multi-pool', 'pool', c0=32, cout=64, pool='dx', bst='act', defer=1, **M)
bwdf('multi-pool-nodx', 'pool-nodx', c0=16, cin=4, cout=32, pool='nodx', **M)
ctbf('multi-c32', 'c32', 6, 35, 256, 64, 32, affine=1, bst='bn', defer=1, multi=1)
ctbf('multi-c32-two-blocks', 'c32', 3, 35, 256, 128, 32, affine=1, bst='bn', multi=1)
ctbf('multi-c64-128', 'c64-128', 6, 35, 128, 128, 64, affine=1, bst='bn', multi=1)
ctbf('multi-c64-64-three-blocks', 'c64-64', 2, 35, 128, 192, 64, affine=1, bst='bn', defer=1, multi=1)

# ------------------------------------------------------------------------------------------------ the smallest shapes
for _f, _kw in (('32-32', dict(c0=32, cout=32)), ('hg', dict(c0=32, cout=32, hg=1)), ('64-32', dict(c0=64, cout=32)), ('64-64', dict(c0=64, cout=64)),
                ('pool', dict(c0=32, cout=64, pool='dx')), ('pool-nodx', dict(c0=16, cin=4, cout=32, pool='nodx'))):
    bwdf(f'one-tile-{_f}', _f, 1, 8, 32, **_kw)
bwdf('few-tiles-32-32', '32-32', 3, 16, 64, 32, 32, affine=1, bst='bn')                       # 12 tiles: 12 workgroups on any device
bwdf('few-tiles-64-64', '64-64', 2, 24, 32, 64, 64)
ctbf('one-tile-c32', 'c32', 1, 1, 64, 64, 32)
ctbf('one-tile-c64-128', 'c64-128', 1, 1, 32, 128, 64)
ctbf('one-tile-c64-64', 'c64-64', 1, 1, 32, 64, 64)
ctbf('few-tiles-c32', 'c32', 2, 5, 64, 64, 32, affine=1, bst='bn')                            # 10 tiles, one per slab
ctbf('few-tiles-c64-64-three-blocks', 'c64-64', 1, 7, 64, 192, 64)                            # 14 tiles x 3 channel blocks

# ------------------------------------------------------------------------------------------------ features, on small maps
bwdf('dual-16-16', '32-32', 2, 16, 64, 16, 32, c1=16, affine=1, bst='bn')                     # the 16-filter U-Net's concat([skip, up])
bwdf('dual-8-24', '32-32', 1, 24, 32, 8, 32, c1=24)
bwdf('dual-40-24', '64-32', 2, 8, 96, 40, 32, c1=24, affine=1, bst='bn')
bwdf('dual-32-32-to-64', '64-64', 3, 8, 32, 32, 64, c1=32, affine=1)
bwdf('affine-norelu-32-32', '32-32', 2, 16, 32, 32, 32, affine=1, in_relu=0)
bwdf('affine-norelu-64-64', '64-64', 1, 16, 64, 64, 64, affine=1, in_relu=0)
bwdf('linear-32-32', '32-32', 2, 16, 32, 32, 32, affine=1, linear=1)
bwdf('linear-64-32', '64-32', 1, 8, 64, 64, 32, linear=1, affine=1, bst='bn')
bwdf('bst-act-32-32', '32-32', 2, 8, 64, 32, 32, bst='act')
bwdf('bst-prefill-64-32', '64-32', 3, 24, 32, 64, 32, affine=1, bst='bn', prefill=1)
bwdf('bst-act-prefill-pool', 'pool', 2, 16, 32, 32, 64, pool='dx', bst='act', prefill=1)
bwdf('accumulate-32-32', '32-32', 2, 16, 64, 32, 32, affine=1, accumulate=1)
bwdf('accumulate-defer-64-64', '64-64', 2, 8, 64, 64, 64, accumulate=1, defer=1)
bwdf('defer-64-32', '64-32', 3, 24, 96, 64, 32, affine=1, bst='bn', defer=1)
bwdf('wide-ld-32-32', '32-32', 2, 16, 64, 32, 32, affine=1, bst='bn', ldg=96, goff=64, yoff=32, lddx=48, bst_ld=40)        # yraw = y + yoff, ldg = ldy
bwdf('wide-ld-64-64', '64-64', 1, 24, 32, 64, 64, ldg=136, goff=8, yoff=72, lddx=72)
bwdf('wide-ld-pool', 'pool', 2, 8, 64, 32, 64, pool='dx', bst='act', ldg=128, goff=64, yoff=0, lddx=40, bst_ld=48, lddp=72)
bwdf('hg-affine-bst', 'hg', 3, 24, 32, 32, 32, hg=1, affine=1, bst='bn')
bwdf('hg-plain', 'hg', 2, 16, 64, 32, 32, hg=1)
bwdf('hg-act-bst-defer', 'hg', 1, 24, 96, 32, 32, hg=1, bst='act', defer=1, yoff=8, ldg=48)
bwdf('pool-dx', 'pool', 3, 24, 32, 32, 64, pool='dx')
bwdf('pool-dx-amax-from-the-pooling-kernel', 'pool', 2, 16, 64, 32, 64, pool='dx', amax='kernel', bst='act')
bwdf('pool-nodx', 'pool-nodx', 3, 24, 32, 16, 32, cin=4, pool='nodx')
bwdf('pool-nodx-amax-from-the-pooling-kernel', 'pool-nodx', 2, 8, 96, 16, 32, cin=4, pool='nodx', amax='kernel', accumulate=1)
bwdf('pool-nodx-16-real', 'pool-nodx', 1, 16, 32, 16, 32, cin=16, pool='nodx', defer=1)

ctbf('affine-norelu-c32', 'c32', 2, 3, 64, 64, 32, affine=1, in_relu=0)
ctbf('affine-norelu-c64-128', 'c64-128', 1, 5, 32, 128, 64, affine=1, in_relu=0)
ctbf('linear-c64-128', 'c64-128', 1, 5, 64, 128, 64, affine=1, linear=1)
ctbf('linear-c32', 'c32', 1, 4, 128, 64, 32, linear=1, affine=1, bst='bn')
ctbf('bst-act-c64-64', 'c64-64', 2, 4, 32, 64, 64, bst='act')
ctbf('bst-prefill-c32', 'c32', 3, 6, 64, 128, 32, affine=1, bst='bn', prefill=1)
ctbf('accumulate-c64-128', 'c64-128', 2, 6, 32, 128, 64, affine=1, accumulate=1)
ctbf('accumulate-defer-c32', 'c32', 1, 9, 64, 64, 32, accumulate=1, defer=1)
ctbf('defer-c64-64', 'c64-64', 2, 16, 32, 192, 64, affine=1, bst='bn', defer=1)
ctbf('wide-ld-c32', 'c32', 2, 8, 64, 64, 32, affine=1, bst='bn', ldg=96, goff=40, ldy=48, yoff=8, ldx=80, lddx=72, bst_ld=88, npad=96)      # g = gcat + ca, ldg = ctot
ctbf('wide-ld-c64-128', 'c64-128', 1, 6, 64, 128, 64, bst='act', ldg=160, goff=96, ldy=72, yoff=8, ldx=136, lddx=144, bst_ld=136, npad=160)
ctbf('wide-ld-c64-64', 'c64-64', 3, 2, 32, 64, 64, affine=1, bst='bn', ldg=128, goff=64, ldx=72, lddx=96, npad=128)

BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def features(c):
    """the feature names (FEATURES[c['kind']]) a case carries"""
    f = set()
    tiles = c['n'] * (c['h'] // 8) * (c['w'] // 32) if c['kind'] == 'bwdf' else c['n'] * c['h'] * (c['w'] // CTBF_FORMS[c['form']][1])
    if c['multi']:
        f.add('multi')
    elif tiles == 1 or (c['kind'] == 'ctbf' and c['n'] * c['h'] == 1):
        f.add('one_tile')
    elif tiles < 16:
        f.add('few_tiles')
    if c['affine']:
        f.add('affine_relu' if c['in_relu'] else 'affine_norelu')
    for k in ('linear', 'accumulate', 'defer'):
        if c[k]:
            f.add(k)
    if c['bst']:
        f.add('bst' if c['bst'] == 'bn' else 'bst_act')
        if c['prefill']:
            f.add('bst_prefill')
    cs = c['c0'] + c['c1'] if c['kind'] == 'bwdf' else c['cin']
    if c['ldg'] > c['cout'] and (c['goff'] or c['yoff']):
        f.add('wide_ldg')
    if c['lddx'] > cs and not (c['kind'] == 'bwdf' and c['pool'] == 'nodx'):
        f.add('wide_lddx')
    if c['bst'] and c['bst_ld'] > cs:
        f.add('wide_bst_ld')
    if c['kind'] == 'ctbf':
        if c['ldx'] > cs:
            f.add('wide_ldx')
        if c['npad'] > cs:
            f.add('wide_npad')
        return f
    if c['c1']:
        f.add(f"dual{c['c0']}_{c['c1']}")
    if c['hg']:
        f.add('hg')
        if c['affine']:
            f.add('hg_affine')
        if c['bst']:
            f.add('hg_bst')
    if c['pool']:
        f.add('pool_dx' if c['pool'] == 'dx' else 'pool_nodx')
        if c['amax'] == 'kernel':
            f.add('amax_kernel')
    return f


# ------------------------------------------------------------------------------------------------ descriptors and the plan queries
FAKE = 1 << 20          # a present, 16-byte aligned tensor in a host-only query (nothing is dereferenced)
BWDF_PTRS = ('g', 'yraw', 'bn_scale', 'bn_shift', 'bn_mean', 'bn_rstd', 'bn_coef', 'x0', 'x1', 'in_scale', 'in_shift', 'w_dgrad', 'dx', 'dw', 'workspace',
             'bst_sums', 'bst_mean', 'bst_rstd', 'dpool', 'amax', 'hg_dlogits', 'hg_w')
CTBF_PTRS = ('g', 'yup', 'bn_scale', 'bn_shift', 'bn_mean', 'bn_rstd', 'bn_c1', 'bn_c2', 'x', 'in_scale', 'in_shift', 'w_dgrad', 'dx', 'dw', 'workspace', 'bst_sums',
             'bst_mean', 'bst_rstd')


def wanted_ptrs(c):
    """the pointer fields of the descriptor the case sets"""
    if c['kind'] == 'bwdf':
        p = ['yraw', 'bn_scale', 'bn_shift', 'bn_mean', 'bn_rstd', 'bn_coef', 'x0', 'dw', 'workspace']
        p += ['hg_dlogits', 'hg_w'] if c['hg'] else ['g']
        p += ['x1'] if c['c1'] else []
        p += ['dx', 'w_dgrad'] if c['pool'] != 'nodx' else []
        p += ['dpool', 'amax'] if c['pool'] else []
    else:
        p = ['g', 'yup', 'bn_scale', 'bn_shift', 'bn_mean', 'bn_rstd', 'bn_c1', 'bn_c2', 'x', 'w_dgrad', 'dx', 'dw', 'workspace']
    p += ['in_scale', 'in_shift'] if c['affine'] else []
    p += ['bst_sums'] if c['bst'] else []
    p += ['bst_mean', 'bst_rstd'] if c['bst'] == 'bn' else []
    return p


def make_desc(c, ptrs=None):
    """the case's descriptor (satcv_bwdf_desc / satcv_ctbf_desc): with ptrs = None for the host-only query (fabricated aligned pointers), else
    with the device pointers of ptrs -- exactly the keys of wanted_ptrs(c)"""
    from satellite_computervision_amd import ops
    want = wanted_ptrs(c)
    p = {k: FAKE for k in want} if ptrs is None else dict(ptrs)
    assert sorted(p) == sorted(want), (c['name'], sorted(p), sorted(want))
    g = lambda k: p.get(k)
    common = dict(bn_scale=g('bn_scale'), bn_shift=g('bn_shift'), bn_mean=g('bn_mean'), bn_rstd=g('bn_rstd'), linear=c['linear'], in_scale=g('in_scale'),
                  in_shift=g('in_shift'), in_relu=c['in_relu'], w_dgrad=g('w_dgrad'), dx=g('dx'), lddx=c['lddx'], dw=g('dw'), cin=c['cin'], cout=c['cout'],
                  n=c['n'], h=c['h'], w_=c['w'], dtype=1, workspace=g('workspace'), accumulate=c['accumulate'], defer_reduce=c['defer'],
                  bst_sums=g('bst_sums'), bst_sums_ld=c['bst_ld'] if c['bst'] else 0, bst_mean=g('bst_mean'), bst_rstd=g('bst_rstd'), ldg=c['ldg'], g=g('g'))
    if c['kind'] == 'bwdf':
        return ops.make_bwdf_desc(yraw=g('yraw'), bn_coef=g('bn_coef'), x0=g('x0'), c0=c['c0'], x1=g('x1'), c1=c['c1'], bst_act_form=int(c['bst'] == 'act'),
                                  dpool=g('dpool'), lddp=c['lddp'] if c['pool'] else 0, amax=g('amax'), hg_dlogits=g('hg_dlogits'), hg_w=g('hg_w'),
                                  hg_ncls=2 if c['hg'] else 0, **common)
    return ops.make_ctbf_desc(yup=g('yup'), ldy=c['ldy'], bn_c1=g('bn_c1'), bn_c2=g('bn_c2'), x=g('x'), ldx=c['ldx'], w_npad=c['npad'], **common)


def plan_info(kind, d, ncu=NCU):
    """dict of the plan query of descriptor d with 'key' in the table's form, or None where the query answers 'unsupported'; any other error raises"""
    import ctypes
    from satellite_computervision_amd import _lib
    if kind == 'bwdf':
        info, fn, fields = _lib.BwdfPlanInfo(), _lib.lib.satcv_conv2d_bwd_fused_plan_info, ('cin', 'cout', 'nw', 'wps', 'pool', 'nodg', 'cins', 'hg')
    else:
        info, fn, fields = _lib.CtbfPlanInfo(), _lib.lib.satcv_convt_bwd_fused_plan_info, ('cout4', 'px', 'cblk')
    rc = fn(ctypes.byref(d), ncu, ctypes.byref(info))
    if rc == -3:            # SATCV_ERR_UNSUPPORTED
        return None
    _lib.check(rc)
    o = {k: int(getattr(info, k)) for k, _ in type(info)._fields_}
    o['key'] = (kind,) + tuple(o[k] for k in fields)
    if kind == 'ctbf':
        o['workgroups'] = o['slabs']        # (the units the tile ranges are dealt to: workgroups, slabs of nblk workgroups)
    return o


def check_plan(c, d=None, ncu=NCU):
    """the plan of the case (of descriptor d where given), checked against the table: the key, the geometry, the tiles-per-workgroup conditions
    of a multi-tile case"""
    g = plan_info(c['kind'], d if d is not None else make_desc(c), ncu)
    assert g is not None, f"{c['name']}: refused"
    assert g['key'] == c['key'], f"{c['name']}: runs {g['key']}, the table says {c['key']}"
    assert g['tiles_min'] >= 1 and g['tiles_max'] - g['tiles_min'] in (0, 1) and 0 < g['lds_bytes'] <= 160 * 1024, (c['name'], g)
    if c['kind'] == 'bwdf':
        assert g['tiles'] == c['n'] * (c['h'] // 8) * (c['w'] // 32) and g['bst'] == BWDF_SUMS[c['form']], (c['name'], g)
        assert g['ws_bytes'] == g['workgroups'] * 9 * g['cin'] * g['cout'] * 4, (c['name'], g)
    else:
        assert g['tiles'] == c['n'] * c['h'] * (c['w'] // g['px']) and g['nblk'] * g['cblk'] == c['cin'], (c['name'], g)
        assert g['ws_bytes'] == g['slabs'] * c['cin'] * 4 * c['cout'] * 4, (c['name'], g)
    if c['multi']:
        # every workgroup iterates its tile loop (bwdf: one prefetch in flight -> 2 tiles; ctbf: two register sets -> 3), and some do once more
        need = 2 if c['kind'] == 'bwdf' else 3
        assert g['tiles_min'] >= need and g['tiles_max'] == g['tiles_min'] + 1, \
            f"{c['name']}: {g['tiles']} tiles on {g['workgroups']} workgroups are {g['tiles_min']} .. {g['tiles_max']} each: not the multi-tile case the table means"
        # ... and the contiguous ranges (the first tiles % workgroups one tile longer) cross row ends and image ends inside a workgroup
        per_row = c['w'] // (32 if c['kind'] == 'bwdf' else g['px'])
        per_img = per_row * (c['h'] // 8 if c['kind'] == 'bwdf' else c['h'])
        wg, per, extra = g['workgroups'], g['tiles'] // g['workgroups'], g['tiles'] % g['workgroups']
        ranges = [(b * per + min(b, extra), b * per + min(b, extra) + per + (b < extra)) for b in range(wg)]
        assert ranges[-1][1] == g['tiles']
        rows = sum(lo // per_row != (hi - 1) // per_row for lo, hi in ranges)
        imgs = sum(lo // per_img != (hi - 1) // per_img for lo, hi in ranges)
        assert rows >= wg // 4 and imgs >= 1, f"{c['name']}: {rows} of {wg} ranges cross a row end, {imgs} an image end"
    else:
        assert g['tiles'] <= 32, (c['name'], g)              # (small maps: at most 3 x 24 x 96 pixels)
    return g


# ------------------------------------------------------------------------------------------------ the nearest descriptors outside each limit
# (label, case the descriptor starts from, descriptor fields changed, True where the change must be REFUSED -- False rows are the nearest
#  descriptor INSIDE the limit, so that a limit that moves either way shows)
REFUSED = [
    # bwdf_shape_ok
    ('h not a multiple of 8', 'few-tiles-32-32', dict(h=12), True),
    ('w not a multiple of 32', 'few-tiles-32-32', dict(w_=48), True),
    ('w a multiple of 16 only', 'one-tile-64-64', dict(w_=16), True),
    ('32 -> 64 without the pooled gradient', 'one-tile-32-32', dict(cout=64, ldg=64), True),
    ('16 -> 32 without the pooled gradient', 'one-tile-32-32', dict(c0=16, cin=16, lddx=16), True),
    ('48 -> 32', 'one-tile-32-32', dict(c0=48, cin=48, lddx=48), True),
    ('64 -> 128', 'one-tile-64-64', dict(cout=128, ldg=128), True),
    ('32 -> 16', 'one-tile-32-32', dict(cout=16), True),
    ('real input channels below the stored ones', 'one-tile-32-32', dict(cin=24), True),
    ('no data gradient without the pooled form', 'one-tile-32-32', dict(dx=None), True),
    ('fused sums on 64 -> 64', 'one-tile-64-64', dict(bst_sums=FAKE, bst_sums_ld=64, bst_act_form=1), True),
    ('fused sums on 64 -> 32', 'one-tile-64-32', dict(bst_sums=FAKE, bst_sums_ld=64, bst_act_form=1), False),
    ('head gradient with the pooled gradient', 'one-tile-pool', dict(hg_dlogits=FAKE, hg_w=FAKE, hg_ncls=2), True),
    ('head gradient at 64 input channels', 'one-tile-64-32', dict(hg_dlogits=FAKE, hg_w=FAKE, hg_ncls=2), True),
    ('head gradient at 64 -> 64', 'one-tile-64-64', dict(hg_dlogits=FAKE, hg_w=FAKE, hg_ncls=2), True),
    ('head gradient of three classes', 'one-tile-hg', dict(hg_ncls=3), True),
    ('head gradient without the head kernel', 'one-tile-hg', dict(hg_w=None), True),
    ('logit gradients off 8 bytes', 'one-tile-hg', dict(hg_dlogits=FAKE + 4), True),
    ('logit gradients on 8 bytes', 'one-tile-hg', dict(hg_dlogits=FAKE + 8), False),
    ('g off 16 bytes', 'one-tile-32-32', dict(g=FAKE + 8), True),
    ('yraw off 16 bytes', 'one-tile-32-32', dict(yraw=FAKE + 8), True),
    ('g at a channel offset of 8', 'one-tile-32-32', dict(g=FAKE + 16, ldg=40), False),
    ('dx off 16 bytes', 'one-tile-32-32', dict(dx=FAKE + 8), True),
    ('ldg not a multiple of 8', 'one-tile-32-32', dict(ldg=36), True),
    ('lddx not a multiple of 8', 'one-tile-32-32', dict(lddx=36), True),
    ('lddx a multiple of 8', 'one-tile-32-32', dict(lddx=40), False),
    ('first source not a multiple of 8 channels', 'dual-8-24', dict(c0=12, c1=20), True),
    ('w ldg = 2^23', 'one-tile-32-32', dict(w_=1 << 18), True),
    ('w ldg = 2^23 - 1024', 'one-tile-32-32', dict(w_=(1 << 18) - 32), False),
    ('2^31 pixels', 'one-tile-32-32', dict(n=1 << 20, h=1 << 6), True),
    ('fp32', 'one-tile-32-32', dict(dtype=0), True),
    ('1 x 1', 'one-tile-32-32', dict(kh=1, kw=1), True),
    ('dilation 2', 'one-tile-32-32', dict(dil=2), True),
    ('pooled: no arg-max bytes', 'one-tile-pool', dict(amax=None), True),
    ('pooled: arg-max bytes off 8 bytes', 'one-tile-pool', dict(amax=FAKE + 4), True),
    ('pooled: lddp not a multiple of 8', 'one-tile-pool', dict(lddp=68), True),
    ('pooled: dpool off 16 bytes', 'one-tile-pool', dict(dpool=FAKE + 8), True),
    ('pooled: two sources', 'one-tile-pool', dict(x1=FAKE, c0=16, c1=16), True),
    ('pooled with dx: 32 -> 32', 'one-tile-pool', dict(cout=32), True),
    ('pooled with dx: 64 -> 64', 'one-tile-pool', dict(c0=64, cin=64, lddx=64), True),
    ('pooled without dx: 32 stored channels', 'one-tile-pool-nodx', dict(c0=32), True),
    ('pooled without dx: 17 real channels', 'one-tile-pool-nodx', dict(cin=17), True),
    ('pooled without dx: 64 output channels', 'one-tile-pool-nodx', dict(cout=64, ldg=64), True),
    ('pooled without dx: fused sums', 'one-tile-pool-nodx', dict(bst_sums=FAKE, bst_sums_ld=16, bst_act_form=1), True),
    # ctbf_dispatch / ctbf_launch
    ('convT: cout 48', 'one-tile-c32', dict(cout=48, ldg=96, ldy=48), True),
    ('convT: cout 128', 'one-tile-c64-128', dict(cout=128, ldg=256, ldy=128), True),
    ('convT: cout 16', 'one-tile-c32', dict(cout=16), True),
    ('convT: cin 96', 'one-tile-c32', dict(cin=96, ldx=96, lddx=96, w_npad=96), True),
    ('convT: cin 32', 'one-tile-c32', dict(cin=32), True),
    ('convT: w 96 on 64-pixel tiles', 'one-tile-c32', dict(w_=96), True),
    ('convT: w 32 on 64-pixel tiles', 'one-tile-c32', dict(w_=32), True),
    ('convT: w 48 on 32-pixel tiles', 'one-tile-c64-128', dict(w_=48), True),
    ('convT: w 96 on 32-pixel tiles', 'one-tile-c64-128', dict(w_=96), False),
    ('convT: f = 3', 'one-tile-c32', dict(f=3), True),
    ('convT: fp32', 'one-tile-c32', dict(dtype=0), True),
    ('convT: ldg not a multiple of 8', 'one-tile-c32', dict(ldg=68), True),
    ('convT: ldy not a multiple of 8', 'one-tile-c32', dict(ldy=36), True),
    ('convT: ldx not a multiple of 8', 'one-tile-c32', dict(ldx=68), True),
    ('convT: lddx not a multiple of 8', 'one-tile-c32', dict(lddx=68), True),
    ('convT: lddx a multiple of 8', 'one-tile-c32', dict(lddx=72), False),
    ('convT: operand image rows below cin', 'one-tile-c32', dict(w_npad=56), True),
    ('convT: operand image rows not a multiple of 8', 'one-tile-c32', dict(w_npad=68), True),
    ('convT: operand image rows a multiple of 8', 'one-tile-c32', dict(w_npad=72), False),
    ('convT: g off 16 bytes', 'one-tile-c32', dict(g=FAKE + 8), True),
    ('convT: g at a channel offset of 8', 'one-tile-c32', dict(g=FAKE + 16), False),
    ('convT: yup off 16 bytes', 'one-tile-c32', dict(yup=FAKE + 8), True),
    ('convT: x off 16 bytes', 'one-tile-c32', dict(x=FAKE + 8), True),
    ('convT: dx off 16 bytes', 'one-tile-c32', dict(dx=FAKE + 8), True),
    ('convT: operand image off 16 bytes', 'one-tile-c32', dict(w_dgrad=FAKE + 8), True),
    ('convT: fused-sum rows narrower than cin', 'few-tiles-c32', dict(bst_sums_ld=56), True),
    ('convT: fused sums with an affine without ReLU', 'few-tiles-c32', dict(in_relu=0), True),
    ('convT: fused sums without the mean', 'few-tiles-c32', dict(bst_mean=None), True),
    ('convT: 2^31 output pixels', 'one-tile-c32', dict(n=1 << 13, h=1 << 10, w_=1 << 6), True),
    ('convT: 32-bit row offsets', 'one-tile-c32', dict(w_=1 << 23, ldg=128), True),
]
