"""Case table of the forward / data-gradient convolution tests (tests/test_conv_plan_cpu.py, tests/test_conv_plan_gpu.py).

satcv_conv2d_igemm serves Conv2D forward, its data gradient, Conv2DTranspose forward (depth-to-space store) and its data gradient
(space-to-depth load).  An instantiation KEY names the kernel template instantiation a descriptor runs:

    (dtype, 'fast',    tw, wm, wn, mt, nt, ks, taps, tl, db, wps, wdma, sk, m16, dyn)   igemm_fast_kernel   (conv_igemm_fast.hip)
    (dtype, 'generic', tw, wm, wn, mt, nt, ks)                                          igemm_kernel        (conv_igemm.hip)
    (dtype, 'm16',     tw, roles, bst)           igemm_m16_kernel (roles = 1) / igemm_m16sym_kernel, with / without the fused sums
    (dtype, 'm16p',    bn, bst)                  igemm_m16p_kernel<bst, bn>
    (dtype, 'ws',      cin, nt, wps, wn, dil)    igemm_ws_kernel
    (dtype, 'tr',      cin, cout, th)            igemm_tr_kernel
    (dtype, 'convt_thin', cin, cout, nw, wps, nsplit) / (dtype, 'convt_thin_dgrad', cin, cout, nw, wps)

ALL_KEYS is written out by hand from the `if` chains of fast_tw / igemm_fast_launch, igemm_m16_launch, igemm_m16p_launch, igemm_ws_launch,
igemm_tr_launch, the two convt_thin launchers and the generic launch_tw, for bf16 and fp32 storage and, as far as the chain names them, the
two e4m3 storage types SATCV_FP8 and SATCV_FP8X (value cases like the rest: every reachable e4m3 key runs on the GPU, bit-exactly, with the once-rounded,
saturating reference of tests/test_conv_plan_gpu.py; where bf16 would fall to the generic kernel, which e4m3 does not have, the table records the
refusal in REFUSALS).  CASES is the table, every entry with the key it is meant to reach.  The CPU test asks the library's plan query
(satcv_conv2d_igemm_plan_info: the launch path's own decision chain, nothing launched) that every case lands on its key and that the
union of the reached keys is ALL_KEYS minus UNREACHABLE; the GPU test runs the cases against a float64 oracle and, on integer data,
bit-exactly.

Shapes are the smallest that select a form, read off the chain:
    tile width      igemm_pick_tw(w): the widest of 8 / 16 / 32 with the least padding -- w = 8 / 24 -> 8, 16 / 48 -> 16, 32 / 60 -> 32
    tile height     BM / tw with BM = 32 wm mt pixels: 128-pixel tiles 16 / 8 / 4 rows, 256-pixel tiles 32 / 16 / 8, 512-pixel 64 / 32 / 16
    N tile          nspace % 128 == 0 -> 128 columns, % 64 == 0 -> 64, else 32 (wm = 4: 256 pixels)
    chunk           3x3: 16 channels; 1x1: 32 when cin % 32 == 0 ('ks2'), 64 when bf16, cin % 64 == 0 and cin >= 512 ('ks4')
    thresholds      igemm_db = 2 forces the double-buffered 3x3 tile (else 192 256-pixel tiles and cin >= 128); DB64 has no override:
                    192 tiles of 512 pixels (6 x 128 x 128 at 128 -> 64); the double-buffered tap loop 96 tiles (SATCV_DB_TL=2 in the child)
Every tiled form has a whole-tile case ('w'), a ragged one ('r': two images, rows no multiple of the tile height, w no multiple of tw) and
a several-images-per-tile one ('m': three images, two per tile, the last group half empty).  Kernels that take whole tiles only (ws, tr,
m16p, m16 with h >= TH, the fused-sums epilogues) have their ragged neighbours in the table with the key those fall to.
"""
F32, BF16, FP8, FP8X = 'f32', 'bf16', 'fp8', 'fp8x'
NCU = 256          # the CU count the CPU tests plan with (ew_grid_cap() of csrc/options.hpp assumes the same)
TWS = (8, 16, 32)

# ------------------------------------------------------------------------------------------------ every instantiation, by hand
# igemm_fast_kernel: (wm, wn, mt, nt, ks, taps, tl, db, wps, wdma, sk, m16) of every fast_cfg<...> site of fast_tw, by name
FAST = {
    # 3x3 halo tile, bf16 only: the double-buffered 256 x 128 tile with the weight ring / register-staged weights, the 512 x 64 tile
    'db-wdma': (4, 2, 2, 2, 1, 9, 0, 1, 0, 1, 0, 0), 'db': (4, 2, 2, 2, 1, 9, 0, 1, 0, 0, 0, 0), 'db64': (8, 1, 2, 2, 1, 9, 0, 1, 0, 0, 0, 0),
    # 3x3 halo tile, single-buffered, 16-channel chunks: 128 x 128 (its split-K attempt first, bf16), 128 x 64, 256 x 32
    'sk-t128-9': (2, 2, 2, 2, 1, 9, 0, 0, 0, 0, 1, 0), 't128-9': (2, 2, 2, 2, 1, 9, 0, 0, 0, 0, 0, 0), 't64-9': (2, 2, 2, 1, 1, 9, 0, 0, 0, 0, 0, 0),
    't32-9': (4, 1, 2, 1, 1, 9, 0, 0, 0, 0, 0, 0),
    # tap loop (dilated beyond the halo form, strided, 5x5 / 7x7): 16-channel chunks where cin % 32 != 0, else 32; bf16: split-K and the
    # double-buffered 64-channel form
    'tl16-64': (2, 2, 2, 1, 1, 1, 1, 0, 0, 0, 0, 0), 'tl16-32': (4, 1, 2, 1, 1, 1, 1, 0, 0, 0, 0, 0), 'sk-tl128': (2, 2, 2, 2, 2, 1, 1, 0, 0, 0, 1, 0),
    'db-tl': (4, 2, 2, 2, 4, 1, 1, 1, 0, 0, 0, 0), 'tl128': (2, 2, 2, 2, 2, 1, 1, 0, 0, 0, 0, 0), 'tl64': (2, 2, 2, 1, 2, 1, 1, 0, 0, 0, 0, 0),
    # 1x1 (and transposed conv / its data gradient), 32-channel chunks; bf16 deep K: 64-channel chunks (ks4), split-K, double-buffered
    'sk-ks4': (2, 2, 2, 2, 4, 1, 0, 0, 2, 0, 1, 0), 'db1x1': (4, 2, 2, 2, 4, 1, 0, 1, 0, 0, 0, 0), 'ks4': (2, 2, 2, 2, 4, 1, 0, 0, 2, 0, 0, 0),
    'sk-c128': (2, 2, 2, 2, 2, 1, 0, 0, 0, 0, 1, 0), 'c128': (2, 2, 2, 2, 2, 1, 0, 0, 0, 0, 0, 0), 'c64': (2, 2, 2, 1, 2, 1, 0, 0, 0, 0, 0, 0),
    'c32': (4, 1, 2, 1, 2, 1, 0, 0, 0, 0, 0, 0),
    # 1x1 with cin % 32 != 0: 16-channel chunks
    'sk-t128-1': (2, 2, 2, 2, 1, 1, 0, 0, 0, 0, 1, 0), 't128-1': (2, 2, 2, 2, 1, 1, 0, 0, 0, 0, 0, 0), 't64-1': (2, 2, 2, 1, 1, 1, 0, 0, 0, 0, 0, 0),
    't32-1': (4, 1, 2, 1, 1, 1, 0, 0, 0, 0, 0, 0),
}
BF16_ONLY = ('db-wdma', 'db', 'db64', 'sk-t128-9', 'sk-tl128', 'db-tl', 'sk-ks4', 'db1x1', 'ks4', 'sk-c128', 'sk-t128-1')
DYN_FORMS = ('t128-9', 't64-9', 't32-9')        # the dilated-halo kernel exists for TAPS == 9 without DB / WPS / SK
# generic igemm_kernel: (wm, wn, mt, nt, ks) of launch_tw
GENERIC = {'g128-ks2': (2, 2, 2, 2, 2), 'g128': (2, 2, 2, 2, 1), 'g64-ks2': (2, 2, 2, 1, 2), 'g64': (2, 2, 2, 1, 1), 'g32-ks2': (4, 1, 2, 1, 2),
           'g32': (4, 1, 2, 1, 1), 'g32-half': (2, 1, 2, 1, 1)}
WS = [(16, 1, 2, 1, 3), (32, 1, 2, 1, 3), (16, 1, 3, 1, 1), (32, 1, 3, 1, 1), (64, 1, 2, 1, 1), (16, 2, 2, 1, 1), (32, 2, 2, 1, 1), (64, 1, 1, 2, 1)]     # bf16 ws_cfg
TR = [(16, 32, 8), (32, 32, 8), (64, 32, 4), (16, 64, 8), (32, 64, 8)]
CONVT = [(64, 32, 4, 2, 1), (64, 32, 4, 3, 1), (128, 64, 8, 2, 1), (256, 128, 8, 2, 4)]
CONVT_DGRAD = [(64, 32, 4, 3), (128, 64, 8, 2)]


def fast_key(dt, tw, form, dyn=0):
    return (dt, 'fast', tw) + FAST[form] + (dyn,)


def generic_key(dt, tw, form):
    return (dt, 'generic', tw) + GENERIC[form]


ALL_KEYS = set()
for _dt in (F32, BF16):
    for _tw in TWS:
        for _f in FAST:
            if _dt == BF16 or _f not in BF16_ONLY:
                ALL_KEYS.add(fast_key(_dt, _tw, _f))
        for _f in DYN_FORMS:
            ALL_KEYS.add(fast_key(_dt, _tw, _f, 1))
        for _f in GENERIC:
            ALL_KEYS.add(generic_key(_dt, _tw, _f))
for _tw in (16, 32):                                   # igemm_m16_launch: tile widths 16 and 32, symmetric / wave roles, without / with the sums
    for _r in (0, 1):
        for _b in (0, 1):
            ALL_KEYS.add((BF16, 'm16', _tw, _r, _b))
for _bn in (128, 64):
    for _b in (0, 1):
        ALL_KEYS.add((BF16, 'm16p', _bn, _b))
ALL_KEYS |= {(BF16, 'ws') + k for k in WS} | {(BF16, 'tr') + k for k in TR} | {(BF16, 'convt_thin') + k for k in CONVT} | \
    {(BF16, 'convt_thin_dgrad') + k for k in CONVT_DGRAD}
# the e4m3 storage types, as far as the chain names them.  SATCV_FP8 (KTraits: 8-element items like bf16, no generic kernel): every fast_tw form
# that is not bf16-only, the dilated probe of igemm_fast_launch included (dyn), and igemm_ws_launch's four fp8 forms.  SATCV_FP8X (block-scaled,
# `KTraits<T>::SUB == 2`: 64-channel chunks): the two forms of that branch for 1x1 and 3x3 taps, and their dilated-halo kernel (a dilated FP8X
# launch skips the tap-loop probe and goes straight to fast_t<fp8s, 9>)
WS_FP8 = [(32, 1, 3, 1, 1), (64, 1, 2, 1, 1), (32, 2, 2, 1, 1), (64, 1, 1, 2, 1)]
FP8X_FORMS = ('t64-9', 't32-9', 't64-1', 't32-1')
for _tw in TWS:
    for _f in FAST:
        if _f not in BF16_ONLY:
            ALL_KEYS.add(fast_key(FP8, _tw, _f))
    for _f in DYN_FORMS:
        ALL_KEYS.add(fast_key(FP8, _tw, _f, 1))
    for _f in FP8X_FORMS:
        ALL_KEYS.add(fast_key(FP8X, _tw, _f))
    for _f in ('t64-9', 't32-9'):
        ALL_KEYS.add(fast_key(FP8X, _tw, _f, 1))
ALL_KEYS |= {(FP8, 'ws') + k for k in WS_FP8}
# fast: bf16 24 forms + 3 dyn, fp32 and fp8 13 + 3, fp8x 4 + 2, x 3 widths; generic 7 x 3 widths x 2 types; m16 8; m16p 4; ws 8 + 4 fp8; tr 5; convt 4 + 2
assert len(ALL_KEYS) == 3 * (27 + 16 + 16 + 6) + 3 * 7 * 2 + 8 + 4 + 8 + 4 + 5 + 4 + 2 == 272

# ------------------------------------------------------------------------------------------------ the table
# options: in-process (satcv_set_option) / startup-only (environment of a fresh child process)
SETTABLE = ('igemm_db', 'igemm_thin', 'igemm_m16', 'splitk', 'm16p', 'thin_roles')
STARTUP_ENV = {'db64': 'SATCV_DB64', 'db_tl': 'SATCV_DB_TL', 'db1x1': 'SATCV_DB1X1', 'db1x1_small': 'SATCV_DB1X1_SMALL', 'wdma': 'SATCV_WDMA',
               'm16_ws': 'SATCV_M16_WS', 'm16p_bn64': 'SATCV_M16P_BN64', 'convt_thin': 'SATCV_CONVT_THIN', 'convt_mid': 'SATCV_CONVT_MID',
               'convt_wps': 'SATCV_CONVT_WPS', 'convt_wide': 'SATCV_CONVT_WIDE', 'splitk_tl': 'SATCV_SPLITK_TL', 'igemm_generic': 'SATCV_IGEMM'}
FEATURES = ('bias', 'stats', 'dual', 'affine', 'out_relu', 'out_scale', 'acc1', 'acc2', 'pool2', 'pair', 'bst1', 'bst2', 'bst_lin',
            'd2s2', 'd2s3', 's2d2', 's2d3', 'stride2', 'dilated', 'centre_tap', 'policy2', 'ragged_cout', 'padded_cin')

CASES = []


def describe(name, n, h, w, c0, cout, key, *, c1=0, k=3, dil=1, stride=1, mode='conv', f=1, ldy=None, bias=False, stats=False, affine=False, out_relu=False,
             out_scale=False, accumulate=0, pool_f=0, pair=False, bst=0, bst_relu=1, tile_policy=0, opts=None, centre_tap=False, workgroups=None, gpu=True, stats_ld=None, cin=None):
    """mode 'conv': Conv2D forward (or, the same GEMM, its data gradient); 'convt': Conv2DTranspose(k == s == f) forward, cout filters, depth-to-space
    store; 'convt_dgrad': its data gradient, space-to-depth load of c0 channels at (h f, w f).  (n, h, w) is the GEMM pixel grid; with stride 2 the
    input is (2 h - 1, 2 w - 1).  c1 > 0: dual source; bst: raw-output tensors of the fused BatchNorm-backward sums (1 or 2); pair: pair store
    of n = 2 * pair_n images into a 2 * cout wide y; ldy: stored output channels (default cout rounded up to 16); cin: REAL input channels where the
    stored c0 are more (single source: the first layer's 4 bands in 16 stored channels) -- the stored rest carries data that must not reach the sum."""
    assert cin is None or (c1 == 0 and mode == 'conv' and cin < c0)
    ldy = ldy or ((cout + 15) // 16 * 16) * (2 if pair else 1)
    return dict(name=name, n=n, h=h, w=w, c0=c0, c1=c1, cout=cout, k=k, dil=dil, stride=stride, mode=mode, f=f, ldy=ldy, bias=bias, stats=stats or bst > 0,
                affine=affine, out_relu=out_relu, out_scale=out_scale, accumulate=accumulate, pool_f=pool_f, pair=pair, bst=bst, bst_relu=bst_relu,
                tile_policy=tile_policy, opts=dict(opts or {}), key=tuple(key), dtype=key[0], centre_tap=centre_tap, workgroups=workgroups, gpu=gpu,
                stats_ld=stats_ld or ((cout + 15) // 16 * 16 if (stats or bst) else 0), cin=cin or c0 + c1)


def case(name, *args, **kw):
    assert not any(c['name'] == name for c in CASES), name
    CASES.append(describe(name, *args, **kw))


REFUSALS = []          # e4m3 descriptors the dispatcher answers with SATCV_ERR_UNSUPPORTED (bf16 / fp32 would run the generic kernel): nothing is launched
REFUSAL_MESSAGE = "outside the pipelined kernel's limits"


def refusal(name, n, h, w, c0, cout, dtype, **kw):
    assert dtype in (FP8, FP8X) and not any(c['name'] == name for c in CASES + REFUSALS), name
    REFUSALS.append(describe(name, n, h, w, c0, cout, (dtype,), **kw))


def planned(n, h, w, c0, cout, dtype, ncu=0, **kw):
    """what satcv_conv2d_igemm runs for a shape under the current options (other tests assert the kernel they name through this); ncu = 0:
    the device's CU count"""
    return plan_info(make_desc(describe('query', n, h, w, c0, cout, (dtype,), **kw)), ncu)


def features(c):
    """the FEATURES a case exercises"""
    f = set()
    for k in ('bias', 'stats', 'affine', 'out_relu', 'out_scale', 'pair'):
        if c[k]:
            f.add(k)
    if c['c1']:
        f.add('dual')
    if c['accumulate']:
        f.add(f"acc{c['accumulate']}")
    if c['pool_f']:
        f.add(f"pool{c['pool_f']}")
    if c['bst']:
        f.add(f"bst{c['bst']}")
        if not c['bst_relu']:
            f.add('bst_lin')
    if c['mode'] == 'convt':
        f.add(f"d2s{c['f']}")
    if c['mode'] == 'convt_dgrad':
        f.add(f"s2d{c['f']}")
    if c['stride'] > 1:
        f.add('stride2')
    if c['dil'] > 1 and not c['centre_tap']:
        f.add('dilated')
    if c['centre_tap']:
        f.add('centre_tap')
    if c['tile_policy']:
        f.add('policy2')
    if c['mode'] == 'conv' and c['cout'] % 16:
        f.add('ragged_cout')
    if c['cin'] < c['c0'] + c['c1']:
        f.add('padded_cin')
    return f


# ------------------------------------------------------------------------------------------------ helpers shared by the two tests
def gemm_cout(c):
    return c['f'] * c['f'] * c['cout'] if c['mode'] == 'convt' else c['cout']


def make_desc(c, ptrs=None):
    """satcv_conv_desc of a case; ptrs: dict of device pointers, or None for the host-only plan query (features that are optional pointers
    are then marked by an aligned fake address: the query reads presence and alignment only)."""
    from satellite_computervision_amd import ops
    fake = 1 << 20
    p = ptrs if ptrs is not None else {}
    g = (lambda k: p.get(k)) if ptrs is not None else (lambda k: fake)
    f, mode = c['f'], c['mode']
    gc = gemm_cout(c)
    bst = None
    if c['bst']:
        bst = dict(y=g('bst_y'), ld=c['cout'] // c['bst'], scale=g('bst_scale'), shift=g('bst_shift'), mean=g('bst_mean'), rstd=g('bst_rstd'), relu=c['bst_relu'])
        if c['bst'] == 2:
            bst.update(y1=g('bst_y1'), ld1=c['cout'] // 2, split=c['cout'] // 2)
    s = c['stride']
    return ops.make_conv_desc(
        x0=g('x0'), c0=c['c0'], x1=g('x1') if c['c1'] else None, c1=c['c1'], w=g('w'), y=g('y'), ldy=c['ldy'], n=c['n'], h=c['h'], w_=c['w'], cout=gc,
        cout_pad=(gc + 31) // 32 * 32, dtype={F32: ops.F32, BF16: ops.BF16, FP8: ops.FP8, FP8X: ops.FP8X}[c['dtype']],
        in_scale=g('in_scale') if c['affine'] else None, in_shift=g('in_shift') if c['affine'] else None, in_relu=1 if c['affine'] else 0,
        bias=g('bias') if c['bias'] else None, stats=g('stats') if c['stats'] else None, stats_ld=c['stats_ld'],
        kh=c['k'], kw=c['k'], dil=c['dil'], mode_in=1 if mode == 'convt_dgrad' else 0, mode_out=1 if mode == 'convt' else 0, f=f, cstat=c['cout'],
        out_relu=1 if c['out_relu'] else 0, accumulate=c['accumulate'], stride=s, hin=2 * c['h'] - 1 if s > 1 else 0, win=2 * c['w'] - 1 if s > 1 else 0,
        out_scale=g('out_scale') if c['out_scale'] else None, pool_y=g('pool_y') if c['pool_f'] else None, pool_ld=c['cout'] if c['pool_f'] else 0, pool_f=c['pool_f'],
        bst=bst, tile_policy=c['tile_policy'], pair=(c['n'] // 2, 0, c['ldy'] // 2) if c['pair'] else None)


def plan_info(d, ncu=NCU):
    """dict of satcv_conv2d_igemm_plan_info(d, ncu) with 'key' in the table's form; raises on a refused descriptor."""
    import ctypes
    from satellite_computervision_amd import _lib
    info = _lib.ConvPlanInfo()
    _lib.check(_lib.lib.satcv_conv2d_igemm_plan_info(ctypes.byref(d), ncu, ctypes.byref(info)))
    o = {k: int(getattr(info, k)) for k, _ in _lib.ConvPlanInfo._fields_}
    o['family'] = _lib.CONV_FAMILIES[o['family']]
    o['key'] = ({_lib.BF16: BF16, _lib.F32: F32, _lib.FP8: 'fp8', _lib.FP8X: 'fp8x'}[o['dtype']], o['family']) + tuple(o[k] for k in _lib.CONV_KEY_FIELDS[o['family']])
    return o


class options:
    """with options({'igemm_db': 2}): ... -- the in-process switches of a case, put back on exit.  Startup-only ones must already hold."""

    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        import ctypes
        from satellite_computervision_amd._lib import lib, check
        self.old = {}
        for k, v in self.opts.items():
            cur = ctypes.c_int32()
            check(lib.satcv_get_option(k.encode(), ctypes.byref(cur)))
            if k in SETTABLE:
                self.old[k] = cur.value
                check(lib.satcv_set_option(k.encode(), v))
            else:
                assert cur.value == v, f'{k} is startup-only: this process has {cur.value}, the case needs {v}'
        return self

    def __exit__(self, *exc):
        from satellite_computervision_amd._lib import lib, check
        for k, v in self.old.items():
            check(lib.satcv_set_option(k.encode(), v))


def check_plan(c, d=None, ncu=NCU):
    """the plan query's answer for a case, asserted against what the table says; returns it."""
    got = plan_info(d if d is not None else make_desc(c), ncu)
    assert got['key'] == c['key'], f"{c['name']}: planned {got['key']}, the table says {c['key']}"
    assert bool(got['centre_tap']) == c['centre_tap'], (c['name'], got)
    if c['workgroups'] is not None and ncu == NCU:
        assert got['workgroups'] == c['workgroups'], (c['name'], got)
    return got


def startup_env(opts):
    return {STARTUP_ENV[k]: ('generic' if k == 'igemm_generic' and v else str(v)) for k, v in opts.items() if k in STARTUP_ENV}


# ------------------------------------------------------------------------------------------------ the cases
def shapes(bm, tw):
    """(n, h, w) of the whole-tile / ragged / several-images-per-tile case of a bm-pixel tile at tile width tw"""
    th = bm // tw
    return {'w': (1, th, tw), 'r': (2, th + th // 4 + 1, {8: 20, 16: 44, 32: 60}[tw]), 'm': (3, th // 2, tw)}


def fast_cases(form, dt, c0, cout, *, dyn=0, tag='', tws=TWS, kinds='wrm', k=None, **kw):
    """the three shapes of a fast_cfg form at every tile width.  Where the staged halo tile of the several-images-per-tile shape exceeds the
    form's register staging (fast_cfg: rl * cl * KC / EL > AI * NTHREADS) the table names the form the shape falls to:
      * 3x3 on the 4-row x 32-pixel tile, two 2-row images: 2 x (2 + 2) x 34 pixels x 2 items = 544 > 512 -> the GENERIC kernel of
        conv_igemm.hip (no pipelined form serves 2-row maps of 64 / 128 output columns at tile width 32; out_scale / pool / pair / fused sums
        are refused there: test_conv_plan_cpu.py::test_two_row_maps_have_no_pipelined_3x3_form).  The e4m3 types have no generic kernel
        (and the scaled form's four 16-channel items per pixel overflow the same way, 1088 > 1024): the shape is REFUSED, and recorded so;
      * the dilated-halo form with two images per tile -> the tap loop; the scaled e4m3 form has no tap loop: REFUSED."""
    wm, wn, mt, nt, ks, taps = FAST[form][:6]
    for tw in tws:
        for kind, (n, h, w) in shapes(32 * wm * mt, tw).items():
            if kind not in kinds:
                continue
            key = fast_key(dt, tw, form, dyn)
            if kind == 'm' and taps == 9 and FAST[form][7] == 0:
                # (the 256-pixel tile holds two dilated images below width 32 -- the scaled form, whose 1920 items of four per pixel meet a budget
                #  of 7 x 256 at width 16, at width 8 only)
                if dyn and not (form == 't32-9' and tw < (16 if dt == FP8X else 32)):
                    key = fast_key(dt, tw, 'tl16-32' if cout % 64 else 'tl16-64') if dt != FP8X else None
                elif not dyn and tw == 32 and wm * mt == 4:
                    key = generic_key(dt, tw, 'g128' if cout % 128 == 0 else 'g64') if dt in (F32, BF16) else None
            name = f'{form}{tag}-{dt}-tw{tw}-{kind}'
            if key is None:
                refusal(name, n, h, w, c0, cout, dt, k=k or (3 if taps == 9 else 1), **kw)
            else:
                case(name, n, h, w, c0, cout, key, k=k or (3 if taps == 9 else 1), **kw)


for dt in (F32, BF16):
    # ---- 3x3 halo tiles, 16-channel chunks (48 input channels: the persistent thin-layer kernels take 16 / 32 / 64)
    fast_cases('t128-9', dt, 48, 128, bias=True, stats=True)
    fast_cases('t64-9', dt, 48, 64, bias=True)
    fast_cases('t32-9', dt, 48, 32, stats=True)
    # ... dilated with the halo form (dyn): dilation 2 fits the register staging of every tile but the 4-row one (see UNREACHABLE)
    fast_cases('t128-9', dt, 48, 128, dyn=1, tag='-dyn', dil=2, tws=(8, 16), bias=True)
    fast_cases('t64-9', dt, 48, 64, dyn=1, tag='-dyn', dil=2, tws=(8, 16), stats=True)
    fast_cases('t32-9', dt, 48, 32, dyn=1, tag='-dyn', dil=2, bias=True)
    # ---- tap loop: dilation 6 never fits the halo form
    fast_cases('tl16-64', dt, 48, 64, dil=6, k=3, bias=True)
    fast_cases('tl16-32', dt, 48, 32, dil=6, k=3, stats=True)
    fast_cases('tl128', dt, 32, 128, dil=6, k=3, bias=True, stats=True)
    fast_cases('tl64', dt, 32, 64, dil=6, k=3)
    # ---- 1x1
    fast_cases('c128', dt, 32, 128, bias=True, stats=True)
    fast_cases('c64', dt, 32, 64, bias=True)
    fast_cases('c32', dt, 32, 32, stats=True)
    fast_cases('t128-1', dt, 48, 128, bias=True)
    fast_cases('t64-1', dt, 48, 64, stats=True)
    fast_cases('t32-1', dt, 48, 32, bias=True, stats=True)

# ---- bf16 only
# (igemm_m16 = 0: with statistics the 16x16x32 tile would take these shapes first)
fast_cases('db-wdma', BF16, 64, 128, opts={'igemm_db': 2, 'igemm_m16': 0}, bias=True, stats=True, kinds='wr')
# the weight ring beside an 8-pixel-wide halo tile fills the LDS to 512 bytes: with a 128-channel scale / shift table, or the taller halo tile of
# two images, it no longer fits and the register-staged form runs (tile widths 16 / 32: SATCV_WDMA=0, STARTUP_SETS)
fast_cases('db', BF16, 128, 128, opts={'igemm_db': 2, 'igemm_m16': 0}, bias=True, stats=True, affine=True, tws=(8,), kinds='wr')
for _tw in TWS:
    _n, _h, _w = shapes(256, _tw)['m']
    case(f'db-wdma-bf16-tw{_tw}-m', _n, _h, _w, 64, 128, fast_key(BF16, _tw, 'db' if _tw == 8 else 'db-wdma'), opts={'igemm_db': 2, 'igemm_m16': 0}, bias=True, stats=True)
fast_cases('sk-t128-9', BF16, 256, 128, opts={'splitk': 1}, bias=True, stats=True)
fast_cases('sk-tl128', BF16, 64, 128, dil=6, k=3, bias=True, stats=True)
fast_cases('sk-ks4', BF16, 512, 128, opts={'splitk': 1}, bias=True, stats=True)
fast_cases('db1x1', BF16, 512, 128, bias=True, stats=True)
fast_cases('sk-c128', BF16, 544, 128, opts={'splitk': 1}, bias=True)
fast_cases('sk-t128-1', BF16, 272, 128, opts={'splitk': 1}, stats=True)
# ks4, the single-buffered 64-channel-chunk tile: the double-buffered tile takes forward launches of up to 256 and from 192 x 2 tiles on, and
# no space-to-depth launch -- so the transposed conv's data gradient (K = 4 x 128) reaches it at small shapes
fast_cases('ks4', BF16, 128, 128, mode='convt_dgrad', f=2)
case('ks4-forward-between-the-thresholds', 9, 64, 64, 512, 128, fast_key(BF16, 32, 'ks4'), k=1, bias=True)
# the 512-pixel x 64-channel tile has no override: 192 tiles of 512 pixels
case('db64-tw32-w', 6, 128, 128, 128, 64, fast_key(BF16, 32, 'db64'), bias=True, stats=True)
case('db64-tw32-r', 7, 120, 124, 128, 64, fast_key(BF16, 32, 'db64'), bias=True)
case('db64-tw32-m', 385, 8, 32, 128, 64, fast_key(BF16, 32, 'db64'), stats=True)
case('db64-tw16-w', 48, 128, 16, 128, 64, fast_key(BF16, 16, 'db64'), bias=True)
case('db64-tw8-w', 96, 128, 8, 128, 64, fast_key(BF16, 8, 'db64'), bias=True)
case('db64-one-tile-short', 6, 128, 127, 128, 64, fast_key(BF16, 32, 't64-9'), bias=True, gpu=False)       # 6 x 128 x 127 is 191 tiles
# the double-buffered tap loop from 96 tiles of 256 pixels on (and more than 128 workgroups of 128 pixels, where split-K stops)
case('db-tl-tw32', 6, 64, 64, 64, 128, fast_key(BF16, 32, 'db-tl'), dil=6, bias=True, affine=True)
case('db-tl-tw32-dual-r', 7, 60, 60, 64, 128, fast_key(BF16, 32, 'db-tl'), c1=64, dil=6, stats=True)
case('db-tl-one-tile-short', 6, 64, 60, 64, 128, fast_key(BF16, 32, 'tl128'), dil=6, gpu=False)         # 6 x 64 x 60 is 90 tiles

# ---- the 16x16x32 tiles (conv_igemm_m16.hip, conv_igemm_m16p.hip): launches that write statistics (option igemm_m16 = 1) or every launch of
# a descriptor with tile_policy = 2; one-tile kernel behind igemm_db = 2, symmetric below 256 input channels, wave roles from there on
for tw in (16, 32):
    sh = shapes(256, tw)
    for kind in 'wr':           # (several images per tile: m16_cfg refuses h < TH -> the 32x32x16 double-buffered tile, below)
        n, h, w = sh[kind]
        case(f'm16-sym-tw{tw}-{kind}', n, h, w, 64, 128, (BF16, 'm16', tw, 0, 0), opts={'igemm_db': 2, 'm16p': 0}, bias=True, stats=True)
        case(f'm16-roles-tw{tw}-{kind}', n, h, w, 256, 128, (BF16, 'm16', tw, 1, 0), opts={'igemm_db': 2, 'm16p': 0}, tile_policy=2, bias=True)
    n, h, w = sh['w']
    case(f'm16-sym-bst-tw{tw}', 2, h, w, 64, 128, (BF16, 'm16', tw, 0, 1), opts={'igemm_db': 2, 'm16p': 0}, bst=1)
    case(f'm16-roles-bst2-lin-tw{tw}', 4, h, w, 256, 128, (BF16, 'm16', tw, 1, 1), opts={'igemm_db': 2, 'm16p': 0}, bst=2, bst_relu=0)
    # (the fused sums need whole tiles: a ragged map is refused, test_conv_plan_cpu.py::test_fused_sums_need_whole_tiles)
    n, h, w = sh['m']
    case(f'm16-falls-to-db-tw{tw}-m', n, h, w, 64, 128, fast_key(BF16, tw, 'db-wdma'), opts={'igemm_db': 2, 'm16p': 0}, bias=True, stats=True)
# persistent kernel: whole 8 x 32 tiles; by default only where a workgroup gets two tiles (m_total >= 2 * ncu / n_tiles), m16p = 2 everywhere
case('m16p-bn128', 2, 16, 64, 64, 128, (BF16, 'm16p', 128, 0), opts={'m16p': 2}, bias=True, stats=True)
case('m16p-bn128-dual-affine', 3, 8, 32, 64, 256, (BF16, 'm16p', 128, 0), c1=64, opts={'m16p': 2}, affine=True, bias=True, stats=True)
case('m16p-bn128-policy2', 2, 8, 32, 128, 128, (BF16, 'm16p', 128, 0), opts={'m16p': 2}, tile_policy=2, bias=True)
case('m16p-bn128-bst', 2, 8, 64, 64, 128, (BF16, 'm16p', 128, 1), opts={'m16p': 2}, bst=1)
case('m16p-bn128-bst2-lin', 2, 16, 32, 128, 128, (BF16, 'm16p', 128, 1), opts={'m16p': 2}, bst=2, bst_relu=0)
case('m16p-bn64', 2, 16, 32, 128, 64, (BF16, 'm16p', 64, 0), opts={'m16p': 2}, bias=True, stats=True)
case('m16p-bn64-bst', 3, 8, 32, 128, 64, (BF16, 'm16p', 64, 1), opts={'m16p': 2}, bst=1)
case('m16p-bn64-192', 1, 8, 64, 64, 192, (BF16, 'm16p', 64, 0), opts={'m16p': 2, 'igemm_thin': 0}, stats=True)
case('m16p-default-two-tiles-per-workgroup', 64, 64, 32, 64, 128, (BF16, 'm16p', 128, 0), stats=True, workgroups=256)      # 512 tiles, 256 ranges
case('m16p-ragged-falls-to-t128', 2, 12, 60, 64, 128, fast_key(BF16, 32, 't128-9'), opts={'m16p': 2}, bias=True, stats=True)
case('m16p-default-below-two-tiles', 63, 64, 32, 64, 128, fast_key(BF16, 32, 't128-9'), stats=True, gpu=False)     # 504 tiles < 2 x 256 CUs

# ---- persistent thin-layer kernels (whole 8 x 32 / 4 x 32 tiles, cout_pad == cout)
for (ci, nt, wps, wn, dil) in WS:
    co = 32 * nt * wn
    opts = {'thin_roles': 0}
    if dil == 3:
        case(f'ws-{ci}-dil3', 2, 8, 64, ci, 32, (BF16, 'ws', ci, nt, wps, wn, dil), dil=3, bias=True, stats=True, opts=opts)
        case(f'ws-{ci}-dil3-acc1', 1, 16, 32, ci, 32, (BF16, 'ws', ci, nt, wps, wn, dil), dil=3, accumulate=1, opts=opts)
        continue
    case(f'ws-{ci}-{co}', 2, 8, 64, ci, co, (BF16, 'ws', ci, nt, wps, wn, dil), bias=True, stats=True, opts=opts)
    case(f'ws-{ci}-{co}-affine-relu-pool2', 3, 8, 32, ci, co, (BF16, 'ws', ci, nt, wps, wn, dil), affine=True, bias=True, out_relu=True, out_scale=True, pool_f=2, opts=opts)
    if ci > 16:
        case(f'ws-{ci}-{co}-dual-acc1', 1, 16, 32, ci // 2, co, (BF16, 'ws', ci, nt, wps, wn, dil), c1=ci // 2, accumulate=1, opts=opts)
    case(f'ws-{ci}-{co}-pair', 2, 8, 32, ci, co, (BF16, 'ws', ci, nt, wps, wn, dil), pair=True, bias=True, opts=opts)
    key = fast_key(BF16, 32, 't64-9' if co == 64 else 't32-9')
    case(f'ws-{ci}-{co}-ragged-neighbour', 2, 11 if co == 32 else 5, 60, ci, co, key, bias=True, stats=True, opts=opts)
for (ci, co, th) in TR:
    case(f'tr-{ci}-{co}', 2, 8, 64, ci, co, (BF16, 'tr', ci, co, th), bias=True, stats=True, opts={'thin_roles': 2})
    case(f'tr-{ci}-{co}-affine-relu-pool2', 3, 8, 32, ci, co, (BF16, 'tr', ci, co, th), affine=True, bias=True, out_relu=True, out_scale=True, pool_f=2, opts={'thin_roles': 2})
    if ci > 16:
        case(f'tr-{ci}-{co}-dual', 1, 16, 32, ci // 2, co, (BF16, 'tr', ci, co, th), c1=ci // 2, stats=True, opts={'thin_roles': 2})
case('tr-default-takes-32-only', 2, 8, 64, 16, 32, (BF16, 'ws', 16, 1, 3, 1, 1), bias=True, stats=True)
case('tr-default-32-64', 2, 8, 64, 32, 64, (BF16, 'tr', 32, 64, 8), bias=True, stats=True)
case('tr-rows-not-whole-falls-to-t32', 2, 12, 32, 32, 32, fast_key(BF16, 32, 't32-9'), bias=True, stats=True)

# ---- transposed convolution and its data gradient
case('convt-thin-64-32', 1, 8, 32, 64, 32, (BF16, 'convt_thin', 64, 32, 4, 3, 1), k=1, mode='convt', f=2, bias=True, stats=True, affine=True)
case('convt-thin-64-32-r', 3, 5, 32, 64, 32, (BF16, 'convt_thin', 64, 32, 4, 3, 1), k=1, mode='convt', f=2, bias=True, out_relu=True, out_scale=True)
case('convt-thin-128-64', 2, 4, 32, 128, 64, (BF16, 'convt_thin', 128, 64, 8, 2, 1), k=1, mode='convt', f=2, bias=True, stats=True)
case('convt-thin-256-128', 1, 8, 32, 256, 128, (BF16, 'convt_thin', 256, 128, 8, 2, 4), k=1, mode='convt', f=2, bias=True, stats=True, affine=True)
case('convt-thin-narrow-falls-to-c128', 2, 8, 16, 64, 32, fast_key(BF16, 16, 'c128'), k=1, mode='convt', f=2, bias=True, stats=True)
case('convt-thin-dgrad-128-64', 1, 8, 32, 64, 128, (BF16, 'convt_thin_dgrad', 128, 64, 8, 2), k=1, mode='convt_dgrad', f=2)
case('convt-thin-dgrad-128-64-bst', 2, 5, 32, 64, 128, (BF16, 'convt_thin_dgrad', 128, 64, 8, 2), k=1, mode='convt_dgrad', f=2, bst=1)
for dt in (F32, BF16):
    case(f'convt-f2-{dt}-c128-r', 2, 11, 44, 32, 32, fast_key(dt, 16, 'c128'), k=1, mode='convt', f=2, bias=True, stats=True)
    case(f'convt-f3-{dt}-c32-r', 2, 9, 20, 32, 32, fast_key(dt, 8, 'c32'), k=1, mode='convt', f=3, bias=True, stats=True)        # 9 x 32 = 288 columns
    case(f'convt-f3-{dt}-c64', 1, 8, 16, 32, 64, fast_key(dt, 16, 'c64'), k=1, mode='convt', f=3, bias=True)               # 576 columns
    case(f'convt-dgrad-f2-{dt}-c64-r', 2, 9, 20, 32, 64, fast_key(dt, 8, 'c64'), k=1, mode='convt_dgrad', f=2)
    case(f'convt-dgrad-f3-{dt}-c32-m', 3, 4, 16, 32, 32, fast_key(dt, 16, 'c32'), k=1, mode='convt_dgrad', f=3)
case('convt-db1x1', 2, 8, 8, 512, 128, fast_key(BF16, 8, 'db1x1'), k=1, mode='convt', f=2, bias=True, stats=True, affine=True)

# ---- features on the general epilogue (t64-9 / c64: 48 / 32 -> 64), the double-buffered tile, tap loop
for dt in (F32, BF16):
    k9, k1 = fast_key(dt, 32, 't64-9'), fast_key(dt, 16, 'c64')
    case(f'feat-{dt}-dual-affine', 2, 5, 60, 32, 64, k9, c1=16, affine=True, bias=True, stats=True)
    case(f'feat-{dt}-out-relu-scale', 2, 5, 60, 48, 64, k9, bias=True, out_relu=True, out_scale=True)
    case(f'feat-{dt}-acc1', 2, 5, 60, 48, 64, k9, accumulate=1, bias=True)
    case(f'feat-{dt}-acc2', 3, 4, 16, 48, 64, fast_key(dt, 16, 't64-9'), accumulate=2, bias=True, out_scale=True)
    case(f'feat-{dt}-pool2', 2, 8, 64, 48, 64, k9, pool_f=2, bias=True, out_relu=True)
    case(f'feat-{dt}-ragged-cout', 2, 5, 60, 48, 30, fast_key(dt, 32, 't32-9'), ldy=48, bias=True, stats=True)
    case(f'feat-{dt}-1x1-ragged-cout-dual', 2, 11, 44, 32, 60, fast_key(dt, 16, 'c32'), k=1, c1=32, ldy=80, bias=True, stats=True, affine=True)
    case(f'feat-{dt}-stride2-1x1', 2, 11, 44, 32, 64, k1, k=1, stride=2, bias=True, stats=True, affine=True)
    case(f'feat-{dt}-stride2-3x3', 2, 9, 20, 32, 64, fast_key(dt, 8, 'tl64'), stride=2, bias=True, stats=True)
    case(f'feat-{dt}-stride2-7x7', 2, 16, 16, 16, 64, fast_key(dt, 16, 'tl16-64'), k=7, stride=2, bias=True, stats=True, affine=True)
    case(f'feat-{dt}-5x5', 2, 11, 20, 16, 32, fast_key(dt, 8, 'tl16-32'), k=5, bias=True)
    case(f'feat-{dt}-centre-tap', 3, 8, 8, 32, 64, fast_key(dt, 8, 'c64'), dil=8, centre_tap=True, bias=True, stats=True)
    case(f'feat-{dt}-dilation-one-below-centre-tap', 3, 8, 8, 32, 64, fast_key(dt, 8, 'tl64'), dil=7, bias=True)
case('feat-bf16-pair', 4, 5, 60, 48, 64, fast_key(BF16, 32, 't64-9'), pair=True, bias=True, out_relu=True)
case('feat-bf16-pair-several-images-per-tile', 6, 4, 16, 48, 64, fast_key(BF16, 16, 't64-9'), pair=True, bias=True)
case('feat-bf16-bst1', 2, 4, 64, 48, 64, fast_key(BF16, 32, 't64-9'), bst=1)
case('feat-bf16-bst2-lin', 2, 4, 32, 48, 128, fast_key(BF16, 32, 't128-9'), bst=2, bst_relu=0)
case('feat-bf16-bst1-1x1', 2, 8, 16, 32, 64, fast_key(BF16, 16, 'c64'), k=1, bst=1)
case('feat-db-dual-affine', 2, 19, 44, 64, 128, fast_key(BF16, 16, 'db-wdma'), c1=64, affine=True, bias=True, stats=True, opts={'igemm_db': 2, 'igemm_m16': 0})
case('feat-db-bst1', 2, 8, 32, 64, 128, fast_key(BF16, 32, 'db-wdma'), bst=1, opts={'igemm_db': 2, 'igemm_m16': 0})
case('feat-db-bst2', 1, 16, 32, 64, 256, fast_key(BF16, 32, 'db-wdma'), bst=2, opts={'igemm_db': 2, 'igemm_m16': 0})
case('feat-db-acc1-relu', 2, 19, 44, 64, 128, fast_key(BF16, 16, 'db-wdma'), accumulate=1, out_relu=True, bias=True, opts={'igemm_db': 2})
case('feat-db-pair', 4, 16, 16, 64, 128, fast_key(BF16, 16, 'db-wdma'), pair=True, bias=True, opts={'igemm_db': 2})
case('feat-db-policy0-keeps-32x32x16-without-stats', 1, 16, 16, 64, 128, fast_key(BF16, 16, 'db-wdma'), bias=True, opts={'igemm_db': 2})
case('feat-db-policy2-takes-16x16x32', 1, 16, 16, 64, 128, (BF16, 'm16', 16, 0, 0), bias=True, tile_policy=2, opts={'igemm_db': 2})
case('feat-db-policy2-tw8-keeps-32x32x16', 1, 32, 8, 64, 128, fast_key(BF16, 8, 'db-wdma'), bias=True, tile_policy=2, opts={'igemm_db': 2})     # (m16: maps at least 16 wide)
case('feat-tl-dual-affine', 2, 9, 20, 32, 64, fast_key(BF16, 8, 'tl64'), c1=32, dil=6, affine=True, bias=True, stats=True)
case('feat-tl-pair', 4, 9, 20, 32, 64, fast_key(BF16, 8, 'tl64'), dil=6, pair=True, bias=True)       # (a dilated pair launch takes the tap loop, never dyn)
case('feat-dyn-refuses-pair', 4, 21, 20, 48, 64, fast_key(BF16, 8, 'tl16-64'), dil=2, pair=True, bias=True)

# ---- the one-tile 16x16x32 kernel with every feature it accepts (no multiplier, no pool): dual source + loader affine are what the benchmark's
# decoder convs run on it; accumulate and the pair store reach it through tile_policy = 2 (they exclude statistics)
_m = {'igemm_db': 2, 'm16p': 0}
case('m16-sym-dual-affine-tw16-r', 2, 20, 44, 64, 128, (BF16, 'm16', 16, 0, 0), c1=64, affine=True, bias=True, stats=True, opts=_m)
case('m16-roles-dual-affine-tw32-r', 2, 9, 60, 128, 128, (BF16, 'm16', 32, 1, 0), c1=128, affine=True, bias=True, stats=True, opts=_m)
case('m16-roles-dual-affine-tw16-w', 1, 16, 16, 256, 128, (BF16, 'm16', 16, 1, 0), c1=256, affine=True, bias=True, stats=True, opts=_m)
case('m16-sym-out-relu-acc1-tw16-r', 2, 20, 44, 64, 128, (BF16, 'm16', 16, 0, 0), accumulate=1, out_relu=True, bias=True, tile_policy=2, opts=_m)
case('m16-roles-acc2-tw32-r', 2, 9, 60, 256, 128, (BF16, 'm16', 32, 1, 0), accumulate=2, bias=True, tile_policy=2, opts=_m)
case('m16-sym-pair-tw32', 4, 8, 32, 64, 128, (BF16, 'm16', 32, 0, 0), pair=True, bias=True, out_relu=True, tile_policy=2, opts=_m)
case('m16-roles-pair-tw16-r', 4, 20, 44, 256, 128, (BF16, 'm16', 16, 1, 0), pair=True, bias=True, tile_policy=2, opts=_m)

# ---- real input channels below the stored count (the first layer: 4 bands in 16 stored channels): the stored rest and its scale / shift entries
# carry lattice values, the packed weights are zero there -- on each family that can meet such a layer
case('padded-cin-ws-16-32', 2, 8, 64, 16, 32, (BF16, 'ws', 16, 1, 3, 1, 1), cin=4, bias=True, stats=True)                 # the benchmark's first layer
case('padded-cin-tr-16-32', 2, 8, 64, 16, 32, (BF16, 'tr', 16, 32, 8), cin=12, bias=True, stats=True, affine=True, opts={'thin_roles': 2})
for dt in (F32, BF16):
    case(f'padded-cin-{dt}-t64-9-r', 2, 5, 60, 16, 64, fast_key(dt, 32, 't64-9'), cin=4, bias=True, stats=True)
    case(f'padded-cin-{dt}-c64-affine', 2, 11, 44, 32, 64, fast_key(dt, 16, 'c64'), k=1, cin=20, bias=True, affine=True)
    case(f'padded-cin-{dt}-stem-7x7-stride2', 2, 16, 16, 16, 64, fast_key(dt, 16, 'tl16-64'), k=7, stride=2, cin=4, bias=True, stats=True)
case('padded-cin-db', 2, 19, 44, 64, 128, fast_key(BF16, 16, 'db-wdma'), cin=40, bias=True, affine=True, opts={'igemm_db': 2, 'igemm_m16': 0})
case('padded-cin-m16', 2, 20, 44, 64, 128, (BF16, 'm16', 16, 0, 0), cin=40, bias=True, stats=True, affine=True, opts=_m)
case('padded-cin-m16p', 2, 8, 64, 64, 128, (BF16, 'm16p', 128, 0), cin=40, bias=True, stats=True, affine=True, opts={'m16p': 2})
case('padded-cin-sk', 3, 8, 8, 256, 128, fast_key(BF16, 8, 'sk-t128-9'), cin=200, bias=True, stats=True, opts={'splitk': 1})

# ---- the e4m3 storage types, SATCV_FP8 and the block-scaled SATCV_FP8X: value cases like the rest.  Every launch carries the output multiplier, as
# every launch of the folded plan does (fp8_infer.py); the GPU test scales it so that nothing saturates, and runs two cases that saturate on purpose
# (E4M3_SATURATING).  Channel counts: 48 and 32 for FP8 (16- and 32-channel chunks; off the thin-layer kernel's 32 / 64 where the map is whole tiles),
# 64 for FP8X.  No stats, fused sums, accumulate, stride or space-to-depth: no lowering produces them in e4m3.
_e = dict(out_scale=True, bias=True, out_relu=True)


def e4m3_cases(form, dt, c0, cout, rot, *, tws=TWS, **kw):
    """one shape kind per tile width, rotated by rot: the three widths of a form together see the whole-tile, the ragged and the
    several-images-per-tile shape"""
    for i, tw in enumerate(TWS):
        if tw in tws:
            fast_cases(form, dt, c0, cout, tws=(tw,), kinds='wrm'[(i + rot) % 3], **dict(_e, **kw))


# 3x3 halo tiles.  The 128- and 64-column forms keep 'm' off tile width 32, where it is refused (fast_cases); the refusal is recorded beside them
e4m3_cases('t128-9', FP8, 48, 128, 1)
e4m3_cases('t64-9', FP8, 48, 64, 2)
e4m3_cases('t32-9', FP8, 48, 32, 0)
fast_cases('t128-9', FP8, 48, 128, tws=(32,), kinds='m', **_e)
fast_cases('t64-9', FP8, 48, 64, tws=(32,), kinds='m', **_e)
# the dilated-halo kernel exists at two widths for the 128- / 64-column forms: every kind at every width ('m' falls to the tap loop but for
# the 256-pixel tile below width 32)
fast_cases('t128-9', FP8, 48, 128, dyn=1, tag='-dyn', dil=2, tws=(8, 16), **_e)
fast_cases('t64-9', FP8, 48, 64, dyn=1, tag='-dyn', dil=2, tws=(8, 16), **_e)
fast_cases('t32-9', FP8, 48, 32, dyn=1, tag='-dyn', dil=2, **_e)
# tap loop: dilation 6, at every tile width
e4m3_cases('tl16-64', FP8, 48, 64, 1, dil=6, k=3)
e4m3_cases('tl16-32', FP8, 48, 32, 2, dil=6, k=3)
e4m3_cases('tl128', FP8, 32, 128, 0, dil=6, k=3)
e4m3_cases('tl64', FP8, 32, 64, 1, dil=6, k=3)
# 1x1: 32-channel chunks, and the 16-channel-chunk forms t*-1
e4m3_cases('c128', FP8, 32, 128, 2)
e4m3_cases('c64', FP8, 32, 64, 0)
e4m3_cases('c32', FP8, 32, 32, 1)
e4m3_cases('t128-1', FP8, 48, 128, 2)
e4m3_cases('t64-1', FP8, 48, 64, 0)
e4m3_cases('t32-1', FP8, 48, 32, 1)
# the scaled form: 64-channel chunks, 16-byte items; a dilated launch has the dilated-halo kernel alone (no tap loop: refused where it does not fit)
e4m3_cases('t64-9', FP8X, 64, 64, 1)
e4m3_cases('t32-9', FP8X, 64, 32, 0)
fast_cases('t64-9', FP8X, 64, 64, tws=(32,), kinds='m', **_e)
e4m3_cases('t64-1', FP8X, 64, 64, 2)
e4m3_cases('t32-1', FP8X, 64, 32, 1)
fast_cases('t64-9', FP8X, 64, 64, dyn=1, tag='-dyn', dil=2, tws=(8, 16), **_e)
fast_cases('t32-9', FP8X, 64, 32, dyn=1, tag='-dyn', dil=2, **_e)
refusal('fp8x-dilation-6-has-no-tap-loop', 2, 9, 20, 64, 64, FP8X, dil=6, **_e)
# thin-layer kernel (whole 8 x 32 tiles, 32 / 64 input channels), with the launch counter moving by one; pair store and dual source + loader affine
# as tests/test_fp8_gpu.py::test_fp8_thin_layer_kernel_bit_exact has them
for (ci, nt, wps, wn, dil) in WS_FP8:
    case(f'fp8-ws-{ci}-{32 * nt * wn}', 2, 8, 64, ci, 32 * nt * wn, (FP8, 'ws', ci, nt, wps, wn, dil), pool_f=2, **_e)
case('fp8-ws-64-64-pair', 2, 8, 32, 64, 64, (FP8, 'ws', 64, 1, 1, 2, 1), pair=True, **_e)
case('fp8-ws-64-32-dual-affine', 3, 8, 32, 32, 32, (FP8, 'ws', 64, 1, 2, 1, 1), c1=32, affine=True, **_e)
case('fp8-ws-ragged-neighbour', 2, 5, 60, 64, 64, fast_key(FP8, 32, 't64-9'), **_e)
# what the folded plan emits for e4m3 tensors, on the general epilogue at ragged shapes
_k9 = fast_key(FP8, 32, 't64-9')
case('feat-fp8-pool2', 2, 10, 60, 48, 64, _k9, pool_f=2, **_e)
case('feat-fp8-pair', 4, 5, 60, 48, 64, _k9, pair=True, **_e)
case('feat-fp8-pair-several-images-per-tile', 6, 4, 16, 48, 64, fast_key(FP8, 16, 't64-9'), pair=True, out_scale=True, bias=True)
case('feat-fp8-convt-f2-r', 2, 11, 44, 32, 32, fast_key(FP8, 16, 'c128'), k=1, mode='convt', f=2, ldy=48, **_e)        # (a channel slice: 32 of 48 stored)
case('feat-fp8-no-relu', 2, 5, 60, 48, 64, _k9, out_scale=True, bias=True)
case('feat-fp8-ragged-cout', 2, 5, 60, 48, 48, fast_key(FP8, 32, 't32-9'), **_e)                  # (48 of cout_pad = 64 columns, two 32-column tiles)
case('feat-fp8-centre-tap', 3, 8, 8, 32, 64, fast_key(FP8, 8, 'c64'), dil=8, centre_tap=True, **_e)
case('feat-fp8-dilation-one-below-centre-tap', 3, 8, 8, 32, 64, fast_key(FP8, 8, 'tl64'), dil=7, **_e)
_k9 = fast_key(FP8X, 32, 't64-9')
case('feat-fp8x-pool2', 2, 10, 60, 64, 64, _k9, pool_f=2, **_e)
case('feat-fp8x-pair', 4, 5, 60, 64, 64, _k9, pair=True, **_e)
case('feat-fp8x-convt-f2', 2, 11, 44, 64, 32, fast_key(FP8X, 16, 't64-1'), k=1, mode='convt', f=2, ldy=48, **_e)
case('feat-fp8x-centre-tap', 3, 8, 8, 64, 64, fast_key(FP8X, 8, 't64-1'), dil=8, centre_tap=True, **_e)
# what the C API accepts for e4m3 and no lowering uses
_k9 = fast_key(FP8, 32, 't64-9')
case('feat-fp8-dual', 2, 5, 60, 32, 64, _k9, c1=16, **_e)
case('feat-fp8-dual-affine', 2, 5, 60, 32, 64, _k9, c1=16, affine=True, **_e)
case('feat-fp8-padded-cin', 2, 5, 60, 16, 64, _k9, cin=4, **_e)
# the two cases the GPU test drives into saturation on purpose (one plain, one scaled; no ReLU: both signs must stop at 448)
E4M3_SATURATING = ('feat-fp8-no-relu-saturating', 'feat-fp8x-saturating')
case('feat-fp8-no-relu-saturating', 2, 5, 60, 48, 64, _k9, out_scale=True, bias=True)
case('feat-fp8x-saturating', 2, 5, 60, 64, 64, fast_key(FP8X, 32, 't64-9'), out_scale=True, bias=True)

# ---- startup-only options: each set is the environment of ONE fresh child process that runs the set's cases
STARTUP_SETS = []


def startup_set(opts):
    global CASES
    STARTUP_SETS.append(dict(opts=dict(opts), cases=[]))
    CASES = STARTUP_SETS[-1]['cases']
    return opts


_main = CASES
# set 0: the forms behind a startup switch that is off / lower by default
_o = startup_set({'wdma': 0, 'convt_wps': 2, 'convt_thin': 2, 'db_tl': 2, 'm16_ws': 2})
for _tw in (16, 32):
    for _kind in 'wr':
        _n, _h, _w = shapes(256, _tw)[_kind]
        case(f'startup-db-no-ring-tw{_tw}-{_kind}', _n, _h, _w, 64, 128, fast_key(BF16, _tw, 'db'), opts=dict(_o, igemm_db=2, igemm_m16=0), bias=True, stats=True)
case('startup-convt-thin-wps2', 3, 5, 32, 64, 32, (BF16, 'convt_thin', 64, 32, 4, 2, 1), k=1, mode='convt', f=2, bias=True, stats=True, affine=True, opts=_o)
case('startup-convt-thin-dgrad-64-32', 1, 8, 32, 32, 64, (BF16, 'convt_thin_dgrad', 64, 32, 4, 3), k=1, mode='convt_dgrad', f=2, opts=_o)
case('startup-convt-thin-dgrad-64-32-bst', 2, 5, 32, 32, 64, (BF16, 'convt_thin_dgrad', 64, 32, 4, 3), k=1, mode='convt_dgrad', f=2, bst=1, opts=_o)
# SATCV_DB_TL=2: the double-buffered tap loop from two tiles on.  Split-K is asked first and takes unit-stride launches of up to 128 workgroups,
# so the small shapes that reach it are strided (stride 2, 3x3: always the tap loop, never split)
for _tw in TWS:
    for _kind in 'wrm':
        _n, _h, _w = shapes(256, _tw)[_kind]
        case(f'startup-db-tl-tw{_tw}-{_kind}', max(_n, 2), _h, _w, 64, 128, fast_key(BF16, _tw, 'db-tl'), stride=2, opts=_o, bias=True, stats=_kind != 'w', affine=_kind == 'r')
case('startup-m16-roles-at-64-channels', 2, 16, 16, 64, 128, (BF16, 'm16', 16, 1, 0), opts=dict(_o, igemm_db=2, m16p=0), bias=True, stats=True)
case('startup-m16-roles-bst-tw16', 2, 16, 16, 64, 128, (BF16, 'm16', 16, 1, 1), opts=dict(_o, igemm_db=2, m16p=0), bst=1)
# set 1: SATCV_IGEMM=generic -- every instantiation of the generic kernel (conv_igemm.hip: 32-channel chunks for 1x1 only)
_o = startup_set({'igemm_generic': 1})
for _dt in (F32, BF16):
    for _tw in TWS:
        for _kind, (_n, _h, _w) in shapes(128, _tw).items():
            for _form, (_ci, _co, _k) in {'g128-ks2': (32, 128, 1), 'g128': (32, 128, 3), 'g64-ks2': (32, 64, 1), 'g64': (48, 64, 3), 'g32-ks2': (64, 30, 1), 'g32': (16, 32, 3)}.items():
                if _form.startswith('g32'):
                    _n, _h, _w = shapes(256, _tw)[_kind]
                case(f'generic-{_form}-{_dt}-tw{_tw}-{_kind}', _n, _h, _w, _ci, _co, generic_key(_dt, _tw, _form), k=_k, opts=_o, bias=True, stats=_kind != 'm',
                     affine=_kind == 'r', out_relu=_kind == 'm', accumulate=1 if _kind == 'm' and _form == 'g64' else 0, ldy=32 if _co == 30 else None)
    # the 128-pixel x 32-channel tile: many taps at stride 2, where the 256-pixel tile's halo image no longer fits the LDS beside the weight slab
    for (_n, _h, _w, _k, _dil) in {F32: [(2, 37, 20, 5, 3), (2, 19, 44, 5, 2), (2, 9, 60, 7, 1)], BF16: [(2, 37, 20, 9, 2), (2, 19, 44, 11, 1), (2, 9, 60, 11, 1)]}[_dt]:
        case(f'generic-g32-half-{_dt}-{_w}', _n, _h, _w, 16, 32, generic_key(_dt, {20: 8, 44: 16, 60: 32}[_w], 'g32-half'), k=_k, stride=2, dil=_dil, bias=True, stats=True, opts=_o)
    case(f'generic-{_dt}-convt-f2', 2, 5, 20, 32, 32, generic_key(_dt, 8, 'g32-ks2'), k=1, mode='convt', f=2, bias=True, stats=True, opts=_o)
    case(f'generic-{_dt}-convt-dgrad-f2', 2, 5, 20, 32, 64, generic_key(_dt, 8, 'g64-ks2'), k=1, mode='convt_dgrad', f=2, opts=_o)
    case(f'generic-{_dt}-stride2-dil2', 2, 9, 20, 32, 64, generic_key(_dt, 8, 'g64'), stride=2, dil=2, bias=True, opts=_o)
    case(f'generic-{_dt}-acc2', 2, 9, 20, 32, 64, generic_key(_dt, 8, 'g64'), accumulate=2, bias=True, opts=_o)
    case(f'generic-{_dt}-dual-affine', 2, 11, 44, 32, 64, generic_key(_dt, 16, 'g64'), c1=16, affine=True, bias=True, stats=True, opts=_o)
    case(f'generic-{_dt}-dual-1x1', 3, 4, 16, 32, 128, generic_key(_dt, 16, 'g128-ks2'), k=1, c1=32, bias=True, opts=_o)
    case(f'generic-{_dt}-convt-f3', 2, 5, 20, 32, 64, generic_key(_dt, 8, 'g64-ks2'), k=1, mode='convt', f=3, bias=True, stats=True, opts=_o)
    case(f'generic-{_dt}-convt-dgrad-f3', 2, 5, 20, 32, 32, generic_key(_dt, 8, 'g32-ks2'), k=1, mode='convt_dgrad', f=3, opts=_o)
    case(f'generic-{_dt}-padded-cin', 2, 9, 20, 16, 64, generic_key(_dt, 8, 'g64'), cin=4, bias=True, stats=True, affine=True, opts=_o)
# set 2: the startup switches turned off -- the shapes of the forms they guard, with the key those fall to
_o = startup_set({'convt_thin': 0, 'convt_mid': 0, 'm16_ws': 0, 'm16p_bn64': 0, 'db1x1': 0, 'db64': 0, 'db_tl': 0, 'splitk_tl': 0, 'convt_wide': 0})
case('off-convt-thin', 1, 8, 32, 64, 32, fast_key(BF16, 32, 'c32'), k=1, mode='convt', f=2, bias=True, stats=True, opts=_o)           # one position (32 columns) per tile
case('off-convt-wide-128', 1, 8, 32, 256, 128, fast_key(BF16, 32, 'c128'), k=1, mode='convt', f=2, bias=True, stats=True, opts=_o)
case('off-convt-thin-dgrad', 1, 8, 32, 64, 128, fast_key(BF16, 32, 'c128'), k=1, mode='convt_dgrad', f=2, opts=_o)
case('off-m16-roles', 1, 16, 16, 256, 128, (BF16, 'm16', 16, 0, 0), opts=dict(_o, igemm_db=2, m16p=0), tile_policy=2, bias=True)
case('off-m16p-bn64', 2, 16, 32, 128, 64, fast_key(BF16, 32, 't64-9'), opts=dict(_o, m16p=2), bias=True, stats=True)
case('off-db1x1', 2, 8, 16, 512, 128, fast_key(BF16, 16, 'ks4'), k=1, bias=True, stats=True, opts=_o)
case('off-db64', 6, 128, 128, 128, 64, fast_key(BF16, 32, 't64-9'), bias=True, opts=_o, gpu=False)
case('off-db-tl', 6, 64, 64, 64, 128, fast_key(BF16, 32, 'tl128'), dil=6, bias=True, opts=_o, gpu=False)
case('off-splitk-tl', 1, 8, 16, 64, 128, fast_key(BF16, 16, 'tl128'), dil=6, bias=True, stats=True, opts=_o)
CASES = _main
BY_NAME = {c['name']: c for c in CASES + [c for s in STARTUP_SETS for c in s['cases']]}

# ------------------------------------------------------------------------------------------------ the benchmark's launches
# bench.py's workload: get_unet_model(2, 4), five levels, 256 x 256 tiles, batch 64, bf16, training plan (tile_policy = 2 on every launch).
# The satcv_conv2d_igemm launches of one training step in the order engine.py emits them -- 21 forward (6 encoder convs, 5 x (transposed conv + 2 convs); the head
# is not a conv launch), then 14 data gradients -- with today's kernel form and workgroup count at 256 CUs.  The 32- and 64-filter layers'
# backward runs the fused backward kernels (conv_bwd_fused.hip, convt_bwd_fused.hip) and never reaches this dispatcher.
# tests/test_conv_plan_gpu.py::test_bench_table_is_what_the_engine_builds compares this table with the descriptors the engine builds.
#   (h, w, c0, c1, cout, k, mode, loader affine + ReLU, bias, statistics, fused-sums sources, key, workgroups)
BENCH_N = 64
_BENCH = [
    (256, 256, 16, 0, 32, 3, 'conv', 0, 1, 1, 0, ('ws', 16, 1, 3, 1, 1), 768),
    (128, 128, 32, 0, 64, 3, 'conv', 0, 1, 1, 0, ('tr', 32, 64, 8), 256),
    (64, 64, 64, 0, 128, 3, 'conv', 0, 1, 1, 0, ('m16p', 128, 0), 256),
    (32, 32, 128, 0, 256, 3, 'conv', 0, 1, 1, 0, ('m16p', 128, 0), 256),
    (16, 16, 256, 0, 512, 3, 'conv', 0, 1, 1, 0, ('m16', 16, 1, 0), 256),
    (8, 8, 512, 0, 1024, 3, 'conv', 0, 1, 1, 0, ('fast', 8) + FAST['t128-9'] + (0,), 256),        # the centre block: single-buffered 128 x 128 tile
    (8, 8, 1024, 0, 512, 1, 'convt', 1, 1, 1, 0, ('fast', 8) + FAST['db1x1'] + (0,), 256),
    (16, 16, 512, 512, 512, 3, 'conv', 1, 1, 1, 0, ('m16', 16, 1, 0), 256),
    (16, 16, 512, 0, 512, 3, 'conv', 1, 1, 1, 0, ('m16', 16, 1, 0), 256),
    (16, 16, 512, 0, 256, 1, 'convt', 1, 1, 1, 0, ('fast', 16) + FAST['db1x1'] + (0,), 512),
    (32, 32, 256, 256, 256, 3, 'conv', 1, 1, 1, 0, ('m16', 32, 1, 0), 512),                          # (the 512-channel table exceeds the persistent kernel's LDS)
    (32, 32, 256, 0, 256, 3, 'conv', 1, 1, 1, 0, ('m16p', 128, 0), 256),
    (32, 32, 256, 0, 128, 1, 'convt', 1, 1, 1, 0, ('convt_thin', 256, 128, 8, 2, 4), 256),
    (64, 64, 128, 128, 128, 3, 'conv', 1, 1, 1, 0, ('m16p', 128, 0), 256),
    (64, 64, 128, 0, 128, 3, 'conv', 1, 1, 1, 0, ('m16p', 128, 0), 256),
    (64, 64, 128, 0, 64, 1, 'convt', 1, 1, 1, 0, ('convt_thin', 128, 64, 8, 2, 1), 256),
    (128, 128, 64, 64, 64, 3, 'conv', 1, 1, 1, 0, ('m16p', 64, 0), 256),
    (128, 128, 64, 0, 64, 3, 'conv', 1, 1, 1, 0, ('ws', 64, 1, 1, 2, 1), 256),
    (128, 128, 64, 0, 32, 1, 'convt', 1, 1, 1, 0, ('convt_thin', 64, 32, 4, 3, 1), 768),
    (256, 256, 32, 32, 32, 3, 'conv', 1, 1, 1, 0, ('ws', 64, 1, 2, 1, 1), 512),
    (256, 256, 32, 0, 32, 3, 'conv', 1, 1, 1, 0, ('tr', 32, 32, 8), 256),
    # data gradients (GEMM: dy channels -> dx channels), with the fused BatchNorm-backward sums where the engine asks for them
    (128, 128, 64, 0, 128, 3, 'conv', 0, 0, 0, 0, ('m16p', 128, 0), 256),
    (64, 64, 128, 0, 128, 3, 'conv', 0, 0, 1, 1, ('m16p', 128, 1), 256),
    (64, 64, 128, 0, 256, 3, 'conv', 0, 0, 0, 0, ('m16p', 128, 0), 256),
    (32, 32, 128, 0, 256, 1, 'convt_dgrad', 0, 0, 1, 1, ('fast', 32) + FAST['ks4'] + (0,), 1024),
    (32, 32, 256, 0, 256, 3, 'conv', 0, 0, 1, 1, ('m16p', 128, 1), 256),
    (32, 32, 256, 0, 512, 3, 'conv', 0, 0, 1, 2, ('m16p', 128, 1), 256),
    (16, 16, 256, 0, 512, 1, 'convt_dgrad', 0, 0, 1, 1, ('fast', 16) + FAST['ks4'] + (0,), 512),
    (16, 16, 512, 0, 512, 3, 'conv', 0, 0, 1, 1, ('m16', 16, 1, 1), 256),
    (16, 16, 512, 0, 1024, 3, 'conv', 0, 0, 1, 2, ('m16', 16, 1, 1), 512),
    (8, 8, 512, 0, 1024, 1, 'convt_dgrad', 0, 0, 0, 0, ('fast', 8) + FAST['ks4'] + (0,), 256),
    (8, 8, 1024, 0, 512, 3, 'conv', 0, 0, 0, 0, ('fast', 8) + FAST['t128-9'] + (0,), 128),
    (16, 16, 512, 0, 256, 3, 'conv', 0, 0, 1, 1, ('fast', 16) + FAST['t128-9'] + (0,), 256),
    (32, 32, 256, 0, 128, 3, 'conv', 0, 0, 1, 1, ('m16', 32, 1, 1), 256),
    (64, 64, 128, 0, 64, 3, 'conv', 0, 0, 1, 1, ('m16p', 64, 1), 256),
]
BENCH_LAUNCHES = []
_main, CASES = CASES, BENCH_LAUNCHES
for _i, (_h, _w, _c0, _c1, _co, _k, _mode, _aff, _b, _st, _bst, _key, _wg) in enumerate(_BENCH):
    case(f'bench-{_i:02d}-{_mode}-{_h}x{_w}-{_c0}+{_c1}-{_co}', BENCH_N, _h, _w, _c0, _co, (BF16,) + _key, c1=_c1, k=_k, mode=_mode, f=1 if _mode == 'conv' else 2,
         affine=bool(_aff), bias=bool(_b), stats=bool(_st), bst=_bst, tile_policy=2, workgroups=_wg, gpu=False,
         stats_ld=(_c0 if _mode == 'convt' else None))       # (a transposed conv's statistics rows are as wide as the concatenation it feeds)
CASES = _main

# keys no descriptor reaches under any option setting, with the reason (DESIGN.md section 4 repeats them)
UNREACHABLE = {}
for _dt in (F32, BF16, FP8, FP8X):
    for _f in ('t128-9', 't64-9') if _dt != FP8X else ('t64-9',):
        UNREACHABLE[fast_key(_dt, 32, _f, 1)] = ('dilated-halo form of a 4-row x 32-pixel tile: its halo tile is at least (4 + 2 dil) x (32 + 2 dil) >= 8 x 36 pixels, '
                                                'two 8-channel items each = 576 register-staged items against the 512 the 256-thread instantiation holds '
                                                '(fast_cfg: rl * cl * KC / EL > AI * NTHREADS); several images per tile only add halo rows.  Dilated 3x3 launches of '
                                                '32-pixel-wide tiles with 64 / 128 output columns always run the tap loop')
