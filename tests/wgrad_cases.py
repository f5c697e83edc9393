"""Case table of the weight-gradient tests (tests/test_wgrad_plan_cpu.py, tests/test_wgrad_plan_gpu.py).

An instantiation KEY names one template instantiation of csrc/conv_wgrad.hip:

    (dtype, kernel, tw, nci, nco, nks, ntaps, pix, nw, m16)

    kernel 'single' wgrad_kernel<T, tw, nci, nco, nks, ntaps, pix>
           'db'     wgrad_db_kernel<bf16, tw, nci, nco, nks, ntaps, pix, nw>
           'dma'    wgrad_dma_kernel<tw, m16>       (always the 2 x 4 block, 9 taps, 128 pixels)

ALL_KEYS is written out by hand from the `if` chain of wgrad_form (once per kernel), wgrad_cfg and wgrad_dma_launch; CASES is the table, every entry
with the key it is meant to reach.  The CPU test asks the library's plan query (satcv_conv2d_wgrad_plan_info: the launch path's own
decision chain, nothing launched) that every case lands on its key and that the union of the reached keys is ALL_KEYS minus UNREACHABLE;
the GPU test runs every case against a float64 oracle and, on integer data, bit-exactly.

Shapes are the smallest that select a form, read off wgrad_plan():
    tile width      pick_tw_w(w): w = 8 / 20 -> 8, 16 / 44 -> 16, 32 / 60 -> 32 (284 -> 32 for the 256-pixel form)
    tile height     pix / tw rows: 16 / 8 / 4 at 128 pixels, 8 / 4 / 2 at 64 (1x1 nw = 4), 8 at 256
    3x3 block form  cout % 128, cout % 64, cinx % 64:  32->128 (1,4)  64->64 (2,2)  32->64 (1,2)  64->32 (2,1)  32->32 (1,1)
    1x1 block form  bf16 double-buffered: 128->256 nw = 4, 64->32 (2,4), 32->32 (1,4); everything else (1,4)
    LDS-DMA         cinx % 64 == 0, cout % 128 == 0, whole 128-pixel tiles, cin == cinx: 64->128
Every form has a whole-tile case ('w'), a ragged one ('r': two images, rows no multiple of the tile height, w no multiple of tw) and a
several-images-per-tile one ('m': three images, two per tile, the last group half empty).  The DMA kernel takes whole tiles only: its
'r' / 'm' neighbours are in the table with the key they fall to (the (1,4) double-buffered form).
"""
F32, BF16 = 'f32', 'bf16'
KEY_FIELDS = ('dtype', 'kernel', 'tw', 'nci', 'nco', 'nks', 'ntaps', 'pix', 'nw', 'm16')
TWS = (8, 16, 32)

# ------------------------------------------------------------------------------------------------ every instantiation, by hand
# wgrad_form<false> (single-buffered wgrad_kernel), both storage types, every tile width: (nci, nco, nks, ntaps)
_SINGLE = [(1, 4, 1, 1), (1, 4, 1, 9), (2, 2, 1, 9), (1, 2, 2, 9), (2, 1, 2, 9), (1, 1, 4, 9)]
# wgrad_form<true> (wgrad_db_kernel, bf16 only), every tile width: (nci, nco, nks, ntaps, pix, nw)
_DB = [(4, 2, 1, 1, 64, 4), (2, 4, 1, 1, 128, 1), (1, 4, 2, 1, 128, 1), (1, 4, 2, 9, 128, 1), (2, 2, 2, 9, 128, 1), (1, 2, 4, 9, 128, 1),
       (2, 1, 4, 9, 128, 1), (1, 1, 8, 9, 128, 1)]
ALL_KEYS = set()
for _tw in TWS:
    for _dt in (F32, BF16):
        for (_a, _b, _c, _d) in _SINGLE:
            ALL_KEYS.add((_dt, 'single', _tw, _a, _b, _c, _d, 128, 1, 0))
    for (_a, _b, _c, _d, _e, _f) in _DB:
        ALL_KEYS.add((BF16, 'db', _tw, _a, _b, _c, _d, _e, _f, 0))
    for _m16 in (0, 1):
        ALL_KEYS.add((BF16, 'dma', _tw, 2, 4, 1, 9, 128, 1, _m16))
# the 256-pixel forms exist at tw = 32 in bf16 only (`if constexpr (TW == 32)`)
ALL_KEYS.add((BF16, 'single', 32, 1, 1, 4, 9, 256, 1, 0))
ALL_KEYS.add((BF16, 'db', 32, 1, 1, 8, 9, 256, 1, 0))
assert len(ALL_KEYS) == 3 * (2 * 6 + 8 + 2) + 2 == 68

# keys no descriptor reaches under any option setting, with the reason (none today: see DESIGN.md section 4)
UNREACHABLE = {}

# ------------------------------------------------------------------------------------------------ the table
# options: in-process (satcv_set_option) wgrad_db, wgrad_m16; startup-only (environment of a fresh child) wgrad_dma, wgrad_pix256, wgrad_wgs
SETTABLE = ('wgrad_db', 'wgrad_m16')
STARTUP_ENV = {'wgrad_dma': 'SATCV_WGRAD_DMA', 'wgrad_pix256': 'SATCV_WGRAD_PIX256', 'wgrad_wgs': 'SATCV_WGRAD_WGS'}

# (n, h, w) per tile width: whole / ragged / several images per tile with a partial last group
SHAPES128 = {8: {'w': (1, 16, 8), 'r': (2, 21, 20), 'm': (3, 8, 8)},
             16: {'w': (1, 8, 16), 'r': (2, 11, 44), 'm': (3, 4, 16)},
             32: {'w': (1, 4, 32), 'r': (2, 5, 60), 'm': (3, 2, 32)}}
SHAPES64 = {8: {'w': (1, 8, 8), 'r': (2, 11, 20), 'm': (3, 4, 8)},           # 1x1 nw = 4 stages 64 pixels
            16: {'w': (1, 4, 16), 'r': (2, 7, 44), 'm': (3, 2, 16)},
            32: {'w': (1, 2, 32), 'r': (2, 3, 60), 'm': (3, 1, 32)}}

CASES = []


def case(name, n, h, w, c0, cout, key, *, c1=0, cin=None, k=3, dil=1, f=0, affine=False, accumulate=False, defer_reduce=False, whole_chip=False,
         opts=None, reduce=None, nsplit=None, per_tap=False, lddy=None):
    """c0 / c1 stored channels of the two sources (c1 > 0: dual source), cin real channels (default: all stored ones), f >= 2: transposed conv
    (mode_dy, 1x1 taps, dW layout (f, f, cout, cin)), affine: the loader's scale / shift / ReLU, lddy: stored dY channels (default cout).
    reduce / nsplit: pinned where the case is about them."""
    cin = c0 + c1 if cin is None else cin
    assert not any(c['name'] == name for c in CASES), name
    CASES.append(dict(name=name, n=n, h=h, w=w, c0=c0, c1=c1, cin=cin, cout=cout, k=1 if f else k, dil=dil, f=f, dtype=key[0], affine=affine,
                      accumulate=accumulate, defer_reduce=defer_reduce, whole_chip=whole_chip, opts=dict(opts or {}), key=tuple(key), reduce=reduce,
                      nsplit=nsplit, per_tap=per_tap, lddy=lddy or cout))


# 3x3 / 1x1 forms: (cinx, cout, taps) that select the block form
_CH3 = {(1, 4): (32, 128), (2, 2): (64, 64), (1, 2): (32, 64), (2, 1): (64, 32), (1, 1): (32, 32)}
for tw in TWS:
    for kind, (n, h, w) in SHAPES128[tw].items():
        for dt in (F32, BF16):
            off = {'wgrad_db': 0} if dt == BF16 else {}          # bf16 reaches wgrad_kernel at dilation 1 only with the double-buffered kernel off
            case(f'single-1x1-{dt}-tw{tw}-{kind}', n, h, w, 32, 32, (dt, 'single', tw, 1, 4, 1, 1, 128, 1, 0), k=1, opts=off)
            for (nci, nco, nks, nt) in _SINGLE[1:]:
                ci, co = _CH3[(nci, nco)]
                case(f'single-{nci}{nco}-{dt}-tw{tw}-{kind}', n, h, w, ci, co, (dt, 'single', tw, nci, nco, nks, 9, 128, 1, 0), opts=off)
        case(f'db-1x1-24-tw{tw}-{kind}', n, h, w, 64, 32, (BF16, 'db', tw, 2, 4, 1, 1, 128, 1, 0), k=1)
        case(f'db-1x1-14-tw{tw}-{kind}', n, h, w, 32, 32, (BF16, 'db', tw, 1, 4, 2, 1, 128, 1, 0), k=1)
        # several images per tile at tw = 32 (tile height 4, two images of two rows): the halo tile has 8 rows, the double-buffered and the
        # DMA kernel stage at most 6 in registers (their launch functions' fit test) -> the single-buffered kernel serves these shapes, the
        # only bf16 / dilation-1 ones that reach it with default options
        short = tw == 32 and kind == 'm'
        for (nci, nco, nks, nt, pix, nw) in _DB[3:]:
            ci, co = _CH3[(nci, nco)]
            key = (BF16, 'single', tw, nci, nco, nks // 2, 9, 128, 1, 0) if short else (BF16, 'db', tw, nci, nco, nks, 9, 128, 1, 0)
            case(f'db-{nci}{nco}-tw{tw}-{kind}', n, h, w, ci, co, key)
        # the DMA kernel's shapes; ragged and partial-group neighbours fall to the (1,4) double-buffered form
        for m16 in (0, 1):
            key = (BF16, 'dma', tw, 2, 4, 1, 9, 128, 1, m16) if kind == 'w' else (BF16, 'single', tw, 1, 4, 1, 9, 128, 1, 0) if short else \
                (BF16, 'db', tw, 1, 4, 2, 9, 128, 1, 0)
            case(f'dma-m16_{m16}-tw{tw}-{kind}', n, h, w, 64, 128, key, opts={'wgrad_m16': m16})
    # ... and its several-images-per-tile branch with every group whole (two images per tile; at tw = 32 see `short` above: before the
    # plan asked wgrad_dma_fits() this shape kept the DMA kernel's 64 x 128 slab geometry and ran a 32 x 32 kernel on it)
    n, h, w = SHAPES128[tw]['m']
    for m16 in (0, 1):
        key = (BF16, 'single', tw, 1, 4, 1, 9, 128, 1, 0) if tw == 32 else (BF16, 'dma', tw, 2, 4, 1, 9, 128, 1, m16)
        case(f'dma-m16_{m16}-tw{tw}-m2', 2, h, w, 64, 128, key, opts={'wgrad_m16': m16})
    for kind, (n, h, w) in SHAPES64[tw].items():
        case(f'db-1x1-nw4-tw{tw}-{kind}', n, h, w, 128, 256, (BF16, 'db', tw, 4, 2, 1, 1, 64, 4, 0), k=1)

# the 256-pixel forms (bf16, tw = 32, w >= 256, h >= 8 = the tile height: no several-images-per-tile form exists)
case('db-11-pix256-w', 1, 8, 256, 32, 32, (BF16, 'db', 32, 1, 1, 8, 9, 256, 1, 0))
case('db-11-pix256-r', 1, 11, 284, 32, 32, (BF16, 'db', 32, 1, 1, 8, 9, 256, 1, 0))
case('single-11-pix256-w', 1, 8, 256, 32, 32, (BF16, 'single', 32, 1, 1, 4, 9, 256, 1, 0), opts={'wgrad_db': 0})
case('single-11-pix256-r', 1, 11, 284, 32, 32, (BF16, 'single', 32, 1, 1, 4, 9, 256, 1, 0), opts={'wgrad_db': 0})

# transposed convolution (mode_dy, f = 2): nspace = 4 cout selects the 1x1 form; dW in the transposed layout -> generic slab sum
case('convt-nw4-w', 1, 8, 8, 128, 64, (BF16, 'db', 8, 4, 2, 1, 1, 64, 4, 0), f=2, reduce='generic')
case('convt-nw4-r', 3, 5, 7, 128, 64, (BF16, 'db', 8, 4, 2, 1, 1, 64, 4, 0), f=2, reduce='generic')
case('convt-db2-64x128-block', 1, 8, 8, 128, 64, (BF16, 'db', 8, 2, 4, 1, 1, 128, 1, 0), f=2, opts={'wgrad_db': 2}, reduce='generic')
case('convt-24-r', 2, 11, 44, 64, 32, (BF16, 'db', 16, 2, 4, 1, 1, 128, 1, 0), f=2, reduce='generic')
case('convt-14-f3', 1, 6, 6, 32, 32, (BF16, 'db', 8, 1, 4, 2, 1, 128, 1, 0), f=3, reduce='generic')
case('convt-single-f32-r', 2, 5, 60, 64, 32, (F32, 'single', 32, 1, 4, 1, 1, 128, 1, 0), f=2, reduce='generic')
case('convt-single-bf16-w', 1, 8, 16, 32, 32, (BF16, 'single', 16, 1, 4, 1, 1, 128, 1, 0), f=2, opts={'wgrad_db': 0}, reduce='generic')

# ---- cross-cutting features, once per kernel template ('single', 'db', 'dma', 'dma m16'): dual source + affine + ReLU, cin below the stored
# count, accumulate, defer_reduce + satcv_reduce_slabs_batched, whole_chip, each slab-sum kernel.
# Pairs the planner forbids:
#   dma / dma m16  x  cin below the stored count   wgrad_plan() takes the DMA kernel only with cin == c0 + c1
#   dma / dma m16  x  generic slab sum             needs cout % 128 == 0 (so nvalid % 4 == 0) and no mode_dy (so no transposed layout)
#   generic slab sum x defer_reduce                satcv_conv2d_wgrad_reduce_job refuses nvalid % 4 != 0
_TEMPL = {'single-f32': dict(key=(F32, 'single', 32, 2, 2, 1, 9, 128, 1, 0), ch=(64, 64), opts={}),
          'single-bf16': dict(key=(BF16, 'single', 32, 2, 2, 1, 9, 128, 1, 0), ch=(64, 64), opts={'wgrad_db': 0}),
          'db': dict(key=(BF16, 'db', 32, 2, 2, 2, 9, 128, 1, 0), ch=(64, 64), opts={}),
          'dma': dict(key=(BF16, 'dma', 32, 2, 4, 1, 9, 128, 1, 0), ch=(64, 128), opts={'wgrad_m16': 0}),
          'dma-m16': dict(key=(BF16, 'dma', 32, 2, 4, 1, 9, 128, 1, 1), ch=(64, 128), opts={'wgrad_m16': 1})}
for tn, t in _TEMPL.items():
    ci, co = t['ch']
    case(f'feat-{tn}-dual-affine', 2, 8, 32, 32, co, t['key'], c1=ci - 32, affine=True, opts=t['opts'])
    case(f'feat-{tn}-accumulate', 2, 8, 32, ci, co, t['key'], accumulate=True, opts=t['opts'])
    case(f'feat-{tn}-defer', 2, 8, 32, ci, co, t['key'], defer_reduce=True, opts=t['opts'])
    case(f'feat-{tn}-defer-accumulate-affine', 3, 4, 32, ci, co, t['key'], defer_reduce=True, accumulate=True, affine=True, opts=t['opts'])
    # whole_chip: 256 workgroups instead of wgrad_wgs (128) for the double-buffered and DMA kernels.  512 input channels make 8 (ci, co)
    # blocks, 4 x 32 x 32 is 32 pixel tiles: 128 / 8 = 16 slabs without the flag, 256 / 8 = 32 with it.  wgrad_kernel's slab count does not
    # depend on it (512 / 8 = 64, capped by the 32 tiles both ways).  WHOLE_CHIP_PAIRS: (without, with) for the CPU test
    ns0 = 32 if t['key'][1] == 'single' else 16
    case(f'feat-{tn}-shared-chip', 4, 32, 32, 512, co, t['key'], opts=t['opts'], nsplit=ns0, reduce='reduce16' if ns0 == 32 else 'reduce4')
    case(f'feat-{tn}-whole-chip', 4, 32, 32, 512, co, t['key'], whole_chip=True, opts=t['opts'], nsplit=32, reduce='reduce16')
    # slab sums: one tile -> one slab (float4 form); 4 x 32 x 32 = 32 pixel tiles -> 32 slabs (16-lane form)
    case(f'feat-{tn}-reduce4-one-slab', 1, 4, 32, ci, co, t['key'], opts=t['opts'], reduce='reduce4', nsplit=1)
    case(f'feat-{tn}-reduce4-some-slabs', 3, 4, 32, ci, co, t['key'], opts=t['opts'], reduce='reduce4', nsplit=3)
    case(f'feat-{tn}-reduce16', 4, 32, 32, ci, co, t['key'], opts=t['opts'], reduce='reduce16', nsplit=32)
    if not tn.startswith('dma'):
        # 12 real of 64 stored input channels (the first layer's padded tiles); the padded channels hold data that must not leak
        case(f'feat-{tn}-cin-below-stored', 2, 5, 60, 64, co, t['key'], cin=12, opts=t['opts'])
        # 30 output channels of 32 stored: nvalid % 4 != 0 -> generic slab sum; the form is then (2,1)
        k21 = t['key'][:3] + (2, 1, 2 if t['key'][1] == 'single' else 4) + t['key'][6:]
        case(f'feat-{tn}-generic-reduce', 2, 5, 60, 64, 30, k21, lddy=32, opts=t['opts'], reduce='generic')
        case(f'feat-{tn}-generic-reduce-accumulate', 3, 4, 16, 64, 30, (k21[0], k21[1], 16) + k21[3:], lddy=32, accumulate=True, opts=t['opts'], reduce='generic')

# ---- strongly dilated 3x3: the halo tile exceeds the LDS, nine shifted 1x1 launches (the smallest such cases by the plan query) and the
# largest dilation that still runs the 3x3 kernel beside them
case('dil-per-tap-f32', 1, 4, 32, 64, 128, (F32, 'single', 32, 1, 4, 1, 1, 128, 1, 0), dil=12, per_tap=True)
case('dil-per-tap-bf16', 2, 5, 60, 64, 128, (BF16, 'single', 32, 1, 4, 1, 1, 128, 1, 0), dil=24, per_tap=True)
case('dil-per-tap-accumulate-affine', 1, 32, 32, 128, 256, (F32, 'single', 32, 1, 4, 1, 1, 128, 1, 0), dil=12, per_tap=True, accumulate=True, affine=True)
case('dil-3x3-f32', 2, 5, 60, 32, 32, (F32, 'single', 32, 1, 1, 4, 9, 128, 1, 0), dil=3)
case('dil-3x3-bf16', 2, 11, 44, 64, 64, (BF16, 'single', 16, 2, 2, 1, 9, 128, 1, 0), dil=2, affine=True)

# ---- startup-only options: one fresh child process runs these (environment below)
STARTUP_OPTS = {'wgrad_dma': 0, 'wgrad_pix256': 0, 'wgrad_wgs': 64}
STARTUP_CASES = []
_main = CASES
CASES = STARTUP_CASES
case('startup-dma-off', 1, 4, 32, 64, 128, (BF16, 'db', 32, 1, 4, 2, 9, 128, 1, 0), opts=STARTUP_OPTS)
case('startup-pix256-off', 1, 8, 256, 32, 32, (BF16, 'db', 32, 1, 1, 8, 9, 128, 1, 0), opts=STARTUP_OPTS)
# wgrad_wgs = 64: 256 -> 64 has 4 blocks, so 64 / 4 = 16 slabs here against 128 / 4 = 32 by default ('wgs-default' below, the same descriptor
# in the main table); whole_chip overrides the option (512 -> 64, 8 blocks: 64 / 8 = 8 slabs without the flag, 256 / 8 = 32 with it)
case('startup-wgs-64', 4, 32, 32, 256, 64, (BF16, 'db', 32, 2, 2, 2, 9, 128, 1, 0), opts=STARTUP_OPTS, nsplit=16, reduce='reduce4')
case('startup-wgs-64-shared-chip', 4, 32, 32, 512, 64, (BF16, 'db', 32, 2, 2, 2, 9, 128, 1, 0), opts=STARTUP_OPTS, nsplit=8, reduce='reduce4')
case('startup-wgs-64-whole-chip', 4, 32, 32, 512, 64, (BF16, 'db', 32, 2, 2, 2, 9, 128, 1, 0), opts=STARTUP_OPTS, whole_chip=True, nsplit=32, reduce='reduce16')
CASES = _main
case('wgs-default', 4, 32, 32, 256, 64, (BF16, 'db', 32, 2, 2, 2, 9, 128, 1, 0), nsplit=32, reduce='reduce16')
WHOLE_CHIP_PAIRS = [(f'feat-{tn}-shared-chip', f'feat-{tn}-whole-chip') for tn in _TEMPL] + [('startup-wgs-64-shared-chip', 'startup-wgs-64-whole-chip')]
WGS_PAIRS = [('wgs-default', 'startup-wgs-64'), ('feat-db-shared-chip', 'startup-wgs-64-shared-chip')]      # (default 128, 64): the same descriptor
BY_NAME = {c['name']: c for c in CASES + STARTUP_CASES}


def startup_env(opts):
    return {STARTUP_ENV[k]: str(v) for k, v in opts.items() if k in STARTUP_ENV}


# ------------------------------------------------------------------------------------------------ the benchmark's launches
# bench.py's workload: get_unet_model(2, 4), five levels, 256 x 256 tiles, batch 64, bf16.  The satcv_conv2d_wgrad launches of one training
# step in the order engine.py's wgrad_step describes them, with today's plan; none accumulates, and none takes the whole chip (wgrad_step's
# `last` is set for no layer of this model).  There are FOURTEEN: of the model's 16 conv + 5 transposed-conv + 1 head layers the 32- and
# 64-filter ones run the fused backward kernels (conv_bwd_fused.hip, convt_bwd_fused.hip) and never reach this planner.
# tests/test_wgrad_plan_gpu.py::test_bench_table_is_what_the_engine_builds compares this table with the descriptors the engine builds.
#   (h, w, c0, c1, cout, k, f, loader affine + ReLU, key, nsplit, slab sum)
BENCH_N = 64
_BENCH = [
    (128, 128, 64, 64, 64, 3, 0, True, ('bf16', 'db', 32, 2, 2, 2, 9, 128, 1, 0), 64, 'reduce16'),
    (64, 64, 128, 0, 128, 3, 0, True, ('bf16', 'dma', 32, 2, 4, 1, 9, 128, 1, 0), 64, 'reduce16'),
    (64, 64, 128, 128, 128, 3, 0, True, ('bf16', 'dma', 32, 2, 4, 1, 9, 128, 1, 0), 32, 'reduce16'),
    (32, 32, 256, 0, 128, 1, 2, True, ('bf16', 'db', 32, 4, 2, 1, 1, 64, 4, 0), 32, 'generic'),
    (32, 32, 256, 0, 256, 3, 0, True, ('bf16', 'dma', 32, 2, 4, 1, 9, 128, 1, 0), 16, 'reduce4'),
    (32, 32, 256, 256, 256, 3, 0, True, ('bf16', 'dma', 32, 2, 4, 1, 9, 128, 1, 0), 8, 'reduce4'),
    (16, 16, 512, 0, 256, 1, 2, True, ('bf16', 'db', 16, 4, 2, 1, 1, 64, 4, 0), 8, 'generic'),
    (16, 16, 512, 0, 512, 3, 0, True, ('bf16', 'dma', 16, 2, 4, 1, 9, 128, 1, 0), 4, 'reduce4'),
    (16, 16, 512, 512, 512, 3, 0, True, ('bf16', 'dma', 16, 2, 4, 1, 9, 128, 1, 0), 2, 'reduce4'),
    (8, 8, 1024, 0, 512, 1, 2, True, ('bf16', 'db', 8, 4, 2, 1, 1, 64, 4, 0), 2, 'generic'),
    (8, 8, 512, 0, 1024, 3, 0, False, ('bf16', 'dma', 8, 2, 4, 1, 9, 128, 1, 0), 2, 'reduce4'),
    (16, 16, 256, 0, 512, 3, 0, False, ('bf16', 'dma', 16, 2, 4, 1, 9, 128, 1, 0), 8, 'reduce4'),
    (32, 32, 128, 0, 256, 3, 0, False, ('bf16', 'dma', 32, 2, 4, 1, 9, 128, 1, 0), 32, 'reduce16'),
    (64, 64, 64, 0, 128, 3, 0, False, ('bf16', 'dma', 32, 2, 4, 1, 9, 128, 1, 0), 128, 'reduce16'),
]
BENCH_LAUNCHES = []
for _i, (_h, _w, _c0, _c1, _co, _k, _f, _aff, _key, _ns, _red) in enumerate(_BENCH):
    _main, CASES = CASES, BENCH_LAUNCHES
    case(f'bench-{_i:02d}-{_h}x{_w}-{_c0}+{_c1}-{_co}' + (f'-convT{_f}' if _f else ''), BENCH_N, _h, _w, _c0, _co, _key, c1=_c1, k=_k, f=_f, affine=_aff,
         nsplit=_ns, reduce=_red)
    CASES = _main


# ------------------------------------------------------------------------------------------------ helpers shared by the two tests
def make_desc(c, ptrs=None):
    """satcv_wgrad_desc of a case; ptrs: dict of device pointers (x0, x1, dy, dw, in_scale, in_shift, workspace, workspace_bytes) or None for
    the host-only plan query."""
    from satellite_computervision_amd import ops
    p = ptrs or {}
    f = c['f']
    return ops.make_wgrad_desc(x0=p.get('x0'), c0=c['c0'], x1=p.get('x1'), c1=c['c1'], dy=p.get('dy'), lddy=c['lddy'], dw=p.get('dw'), cin=c['cin'], cout=c['cout'],
                               n=c['n'], h=c['h'], w_=c['w'], dtype=ops.BF16 if c['dtype'] == BF16 else ops.F32,
                               in_scale=p.get('in_scale'), in_shift=p.get('in_shift'), in_relu=1 if c['affine'] else 0,
                               kh=c['k'], kw=c['k'], dil=c['dil'], mode_dy=1 if f else 0, f=f if f else 1, transposed=1 if f else 0,
                               workspace=p.get('workspace'), workspace_bytes=p.get('workspace_bytes', 0), accumulate=c['accumulate'],
                               whole_chip=c['whole_chip'], defer_reduce=c['defer_reduce'])


def plan_info(d):
    """dict of satcv_conv2d_wgrad_plan_info(d) with 'key' in the table's form; raises on a refused descriptor."""
    import ctypes
    from satellite_computervision_amd import _lib
    info = _lib.WgradPlanInfo()
    _lib.check(_lib.lib.satcv_conv2d_wgrad_plan_info(ctypes.byref(d), ctypes.byref(info)))
    o = {k: int(getattr(info, k)) for k, _ in _lib.WgradPlanInfo._fields_}
    o['kernel'] = _lib.WGRAD_KERNELS[o['kernel']]
    o['reduce'] = _lib.WGRAD_REDUCES[o['reduce']]
    o['key'] = (BF16 if d.dtype == _lib.BF16 else F32, o['kernel'], o['tw'], o['nci'], o['nco'], o['nks'], o['ntaps'], o['pix'], o['nw'], o['m16'])
    return o


class options:
    """with options({'wgrad_db': 0}): ... -- the in-process switches of a case, put back on exit.  Startup-only ones must already hold."""

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


def check_plan(c):
    """the plan query's answer for a case, asserted against what the table says; returns it."""
    d = make_desc(c)
    got = plan_info(d)
    assert got['key'] == c['key'], f"{c['name']}: planned {got['key']}, the table says {c['key']}"
    assert bool(got['per_tap']) == c['per_tap'], (c['name'], got)
    if c['reduce'] is not None:
        assert got['reduce'] == c['reduce'], (c['name'], got)
    if c['nsplit'] is not None:
        assert got['nsplit'] == c['nsplit'], (c['name'], got)
    return got


def lattice_bound(c):
    """largest |partial sum| of the integer-lattice data in units of its grid (1, or 1/2 with the affine's 0.5 scale): must stay below 2^24
    for fp32 sums to be exact in any order.  |x| <= 4, |dy| <= 4; the affine maps x to at most 2 * 4 + 3 in half steps; the accumulate
    base adds at most 4."""
    amax, unit = (2 * 4 + 3, 2) if c['affine'] else (4, 1)
    return unit * (amax * 4 * c['n'] * c['h'] * c['w'] + 4)
