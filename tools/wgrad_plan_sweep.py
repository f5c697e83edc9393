"""The weight gradient's host-side decisions of two builds of libsatcv.so, compared over a grid of descriptors wider than
tests/wgrad_cases.py -- for a change of csrc/conv_wgrad.hip's host code that must not move a plan:

    python tools/wgrad_plan_sweep.py <libsatcv.so of A> <libsatcv.so of B>

Both libraries are loaded into this process (each keeps its own options); nothing touches a device.  Per descriptor and library:
the return code and every field of satcv_conv2d_wgrad_plan_info, satcv_conv2d_wgrad_workspace, and the satcv_last_error text of a
refused descriptor.  Prints the number of descriptors, how many are equal, and the first differences; exit status 1 on any."""
import ctypes as C
import importlib.util
import itertools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.join(HERE, '..'))
from satellite_computervision_amd import _lib, ops      # noqa: E402  (the structures and the descriptor's one constructor)


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    lib.satcv_conv2d_wgrad_plan_info.argtypes = [C.POINTER(_lib.WgradDesc), C.POINTER(_lib.WgradPlanInfo)]
    lib.satcv_conv2d_wgrad_workspace.argtypes, lib.satcv_conv2d_wgrad_workspace.restype = [C.POINTER(_lib.WgradDesc)], C.c_int64
    lib.satcv_last_error.restype = C.c_char_p
    lib.satcv_set_option.argtypes = [C.c_char_p, C.c_int32]
    return lib


def ask(lib, d):
    info = _lib.WgradPlanInfo()
    rc = lib.satcv_conv2d_wgrad_plan_info(C.byref(d), C.byref(info))
    err = lib.satcv_last_error() if rc else b''
    return (rc, err, lib.satcv_conv2d_wgrad_workspace(C.byref(d))) + tuple(getattr(info, k) for k, _ in _lib.WgradPlanInfo._fields_)


def descriptors():
    spec = importlib.util.spec_from_file_location('wgrad_cases', os.path.join(HERE, '..', 'tests', 'wgrad_cases.py'))
    wc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(wc)
    shapes = sorted({s for t in (wc.SHAPES128, wc.SHAPES64) for by_kind in t.values() for s in by_kind.values()} | {(1, 8, 8), (2, 64, 64), (1, 256, 284)})
    chans = (8, 32, 64, 128, 256)
    sources = ('one', 'two', 'two, cin below stored')
    # none / accumulate / defer_reduce / whole_chip / all three / dW off the 16-byte boundary (the slab-sum kernel depends on it)
    flags = ((0, 0, 0, None), (1, 0, 0, None), (0, 1, 0, None), (0, 0, 1, None), (1, 1, 1, None), (0, 0, 0, 4))
    for (n, h, w), c0, cout, src, k, dil, f, dt, (acc, defer, chip, dw) in itertools.product(
            shapes, chans, chans, sources, (1, 3), (1, 2, 12), (0, 2), (ops.F32, ops.BF16), flags):
        c1 = 0 if src == 'one' else c0
        cin = c0 + c1 - (4 if src.endswith('stored') else 0)
        yield (n, h, w, c0, c1, cin, cout, k, dil, f, dt, acc, defer, chip, dw), ops.make_wgrad_desc(
            x0=None, c0=c0, x1=None, c1=c1, dy=None, lddy=cout, dw=dw, cin=cin, cout=cout, n=n, h=h, w_=w, dtype=dt, kh=k, kw=k, dil=dil,
            mode_dy=1 if f else 0, f=f if f else 1, transposed=1 if f else 0, accumulate=acc, defer_reduce=defer, whole_chip=chip)


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    total = equal = refused = 0
    forms = set()
    for db, m16 in itertools.product((0, 1, 2), (0, 1)):
        for lib in (a, b):
            assert lib.satcv_set_option(b'wgrad_db', db) == 0 and lib.satcv_set_option(b'wgrad_m16', m16) == 0
        for what, d in descriptors():
            ra, rb = ask(a, d), ask(b, d)
            total += 1
            equal += ra == rb
            refused += ra[0] != 0
            if ra[0] == 0:
                forms.add((what[10],) + ra[3:14])
            if ra != rb and total - equal <= 10:
                print('DIFFER', dict(wgrad_db=db, wgrad_m16=m16), what, '\n  A', ra, '\n  B', rb)
    print(f'{total} descriptors, {equal} equal; library A refuses {refused} of them and plans {len(forms)} distinct (dtype, kernel form) rows')
    return 0 if equal == total else 1


if __name__ == '__main__':
    sys.exit(main())
