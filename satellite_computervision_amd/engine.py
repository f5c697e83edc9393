"""Graph + executor behind the Keras-style surface of model_tools.py.

A model is a list of block-level nodes (conv+BN+ReLU, max-pool, transposed conv,
concat+BN+ReLU, 1x1 head) built by the layer classes in model_tools.py.  `Plan`
lowers that list, for one (batch, H, W), into a static sequence of C-ABI kernel
launches on preallocated device buffers (torch tensors are only the allocator).

Fusion contract (what the HIP kernels expect):
  * a conv output is stored RAW (pre-BatchNorm); its BN affine + ReLU is applied by
    whichever kernel consumes it (conv loader, pool kernel, head);
  * concat([skip, up]) is never materialised: the consumer conv reads two sources;
  * train-mode BN statistics come from the producing kernel's epilogue.
Parameters, gradients, optimizer state and packed weight images are the params.FlatParams that `Runtime` is.
There is no CPU path: everything here requires the HIP library and a ROCm device.
"""
import ctypes as C
import itertools
from collections import defaultdict, namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import ops, parallel, switches
from ._lib import lib, check, F32, BF16, STAT_ROWS
from .params import FlatParams

_M16_DEFAULT = ops.options()['igemm_m16']      # the library's value of option igemm_m16 at import (csrc/options.hpp)

BN_EPS = 1e-3
BN_MOMENTUM = 0.99


# ------------------------------------------------------------------ symbolic graph
class KTensor:
    """Symbolic NHWC tensor (the analogue of a KerasTensor)."""
    _ids = itertools.count()

    def __init__(self, node, channels, down=Fraction(1), name=None):
        self.id = next(KTensor._ids)
        self.node, self.channels, self.down, self.name = node, channels, down, name

    @property
    def shape(self):
        return (None, None, None, self.channels)


class Node:
    def __init__(self, op, inputs, layer=None, **attrs):
        self.op, self.inputs, self.layer, self.attrs = op, list(inputs), layer, attrs
        self.outputs = []

    def out(self, channels, down, name=None):
        t = KTensor(self, channels, down, name)
        self.outputs.append(t)
        return t


class ParamSpec:
    def __init__(self, name, shape, kind, init):
        self.name, self.shape, self.kind, self.init = name, tuple(shape), kind, init

    @property
    def size(self):
        return int(np.prod(self.shape))


# Import-time switches (switches.py holds variable, default and meaning of each; DESIGN.md section 6 the measurements).
# BIAS_NOISE: the bias of a convolution that feeds a training-mode BatchNormalization has an identically zero gradient: with
# dy = scale*rstd*(g - mean(g) - xhat*mean(g*xhat)) the sum over the batch vanishes because sum(xhat) = 0.  TensorFlow computes
# reduce_sum(dy) anyway and gets rounding noise (~1e-9), which Adam's normalisation turns into +-lr steps of a parameter that has
# no effect on any output.  Here the gradient is the exact 0 (the bias stays at its value) unless the summed-noise form is asked for;
# the atomics it needs are also the one remaining source of run-to-run differences in a training step.
BIAS_NOISE = switches.read('bn_bias_noise')
CTBF = switches.read('ctbf')
CTBF_COUTS = switches.read('ctbf_couts')
FUSE_RESIDUAL = switches.read('fuse_residual')
FUSE_DGRAD_ALL = switches.read('fuse_dgrad_bn_bwd') == 2      # (Model.fuse_dgrad_bn_bwd is the same row != 0)


def rup(a, b):
    return (a + b - 1) // b * b


def topo_nodes(outputs):
    seen, order = set(), []

    def visit(node):
        if id(node) in seen:
            return
        seen.add(id(node))
        for t in node.inputs:
            visit(t.node)
        order.append(node)
    for t in outputs:
        visit(t.node)
    return order


# -------------------------------------------------------------------- runtime refs
class TRef:
    """Runtime tensor: 1-2 device sources + an optional pending BN affine (+ReLU)."""

    def __init__(self, srcs, n, h, w, affine=None, relu=False):
        self.srcs, self.n, self.h, self.w = srcs, n, h, w      # srcs: [(torch tensor, channels)]
        self.affine, self.relu = affine, relu                   # affine: dict(scale, shift, mean, rstd)

    @property
    def c(self):
        return sum(c for _, c in self.srcs)


def _fp(t, off=0):
    """device address of element `off` of a float32 (parameters, affines) or float64 (statistics rows) tensor, or None."""
    return None if t is None else t.data_ptr() + t.element_size() * off


class Runtime(FlatParams):
    """Device state of one graph model: the FlatParams store of its trainables (params.py), the BN moving statistics beside it (sflat),
    every layer's packed MFMA weight images -- allocated here, repacked at once whenever the parameters change -- and the plans."""

    def __init__(self, model, dtype):
        if not torch.cuda.is_available():
            raise RuntimeError('satellite_computervision_amd needs a ROCm GPU (no CPU fallback)')
        super().__init__()
        self.model, self.dtype = model, dtype
        self.pack_dtype = dtype
        self.tdtype = ops.TORCH_DTYPE[dtype]
        self.esize = 2 if dtype == BF16 else 4
        self.dev = torch.device('cuda', torch.cuda.current_device())
        # flat layout: trainables (the optimizer sees one buffer), then non-trainable BN moving statistics in a buffer of their own
        self.offsets, self.soffsets = {}, {}
        off = soff = 0
        for p in model.param_specs:
            if p.kind in ('moving_mean', 'moving_var'):
                self.soffsets[p.name] = soff
                soff += rup(p.size, 4)
            else:
                self.offsets[p.name] = off
                off += rup(p.size, 4)
        self.n_train = off
        self.dropout_seed = 0x5A7C0FFEE
        host = np.zeros(max(off, 4), np.float32)
        hs = np.zeros(max(soff, 4), np.float32)
        self.zero_gamma = set()
        for p in model.param_specs:
            v = np.asarray(p.init(), np.float32).reshape(-1)
            self._note_gamma(p.name, v)
            if p.name in self.offsets:
                host[self.offsets[p.name]:self.offsets[p.name] + p.size] = v
            else:
                hs[self.soffsets[p.name]:self.soffsets[p.name] + p.size] = v
        self.allocate(host, self.dev)
        self.sflat = torch.from_numpy(hs).to(self.dev)
        self.specs = {p.name: p for p in model.param_specs}
        # packed weights per conv-like layer
        for node in model.nodes:
            if node.op in ('cba', 'convT'):
                lay = node.layer
                if lay.name in self.packed:
                    continue
                ks = self.specs[lay.kernel_name].shape
                tr = node.op == 'convT'
                cin, cout = (ks[3], ks[2]) if tr else (ks[2], ks[3])
                cin_pad = rup(cin, 16)
                ef, ed, _, _ = ops.packed_sizes(ks[0], ks[1], cin, cout, cin_pad, tr)
                self.register_image(lay.name, self.pptr(lay.name + '/kernel'), torch.zeros(ef, dtype=self.tdtype, device=self.dev),
                                    torch.zeros(ed, dtype=self.tdtype, device=self.dev), (ks[0], ks[1]), cin, cout, cin_pad, tr)
        self.repack()
        self.plans = {}

    def weights_changed(self):
        """after every optimizer step and every set_weights_dict: the images follow at once (one batched launch), `version` moves on"""
        self.repack()
        self.bump()

    # ---- parameter access
    def pptr(self, name):
        return _fp(self.pflat, self.offsets[name])

    def gptr(self, name):
        return _fp(self.gflat, self.offsets[name])

    def sptr(self, name):
        return _fp(self.sflat, self.soffsets[name])

    def get_param(self, name):
        p = self.specs[name]
        if name in self.offsets:
            return self.pflat[self.offsets[name]:self.offsets[name] + p.size].view(p.shape)
        return self.sflat[self.soffsets[name]:self.soffsets[name] + p.size].view(p.shape)

    def get_grad(self, name):
        p = self.specs[name]
        return self.gflat[self.offsets[name]:self.offsets[name] + p.size].view(p.shape)

    def set_param(self, name, value):
        v = np.asarray(value, np.float32)
        self._note_gamma(name, v)
        self.get_param(name).copy_(torch.as_tensor(v).to(self.dev).view(self.specs[name].shape))

    def _note_gamma(self, name, v):
        """BatchNorm layers with a zero (or subnormal) gamma, tracked on the host as the weights are set (no device read).  The sums of
        their backward must come from the raw output: a form built from the activation a = relu(gamma xhat + beta) recovers sum g xhat as
        (sum g a - beta sum g) / gamma, which is undefined where gamma = 0 (there a is the constant relu(beta) and carries nothing of xhat,
        satcv_bn_bwd_finalize2 returns 0 -- while dgamma = sum g [beta > 0] xhat is not 0)."""
        if name.endswith('/gamma'):
            bn = name[:-len('/gamma')]
            if np.any(np.abs(v) < np.finfo(np.float32).tiny):
                self.zero_gamma.add(bn)
            else:
                self.zero_gamma.discard(bn)

    def plan(self, n, h, w, training):
        # tf.keras runs a BatchNormalization whose `trainable` is False in INFERENCE mode even inside fit() (moving statistics, no
        # update): the set of frozen layers is part of a training plan's identity (retrain_model(freeze=True), utils/model_tools.py:1174)
        frozen = tuple(sorted(l.name for l in self.model.layers if not l.trainable)) if training else ()
        # (as is the set of BatchNorms whose backward sums must stay in the raw form: Runtime._note_gamma)
        raw_bn = tuple(sorted(self.zero_gamma)) if training else ()
        key = (n, h, w, bool(training), frozen, raw_bn)
        if key not in self.plans:
            self.plans[key] = Plan(self, n, h, w, training, frozen, raw_bn)
        return self.plans[key]


class Plan:
    """Static launch sequence for one input shape."""

    def __init__(self, rt, n, h, w, training, frozen=(), raw_bn=()):
        self.rt, self.n, self.h, self.w, self.training = rt, n, h, w, training
        self.frozen = set(frozen)
        self.raw_bn = set(raw_bn)             # BatchNorms (zero gamma) whose backward sums no activation-based producer may form
        self.tile_policy = 2 if (training and _M16_DEFAULT == 1) else 0      # satcv_conv_desc.tile_policy of this plan's convolution launches
        self.fwd, self.bwd = [], []
        self.keep = []                        # ctypes descriptors / tensors kept alive
        self.dropouts = []                    # dropout masks (regenerated every training step)
        self.x_inputs = []                    # fp32 staging tensor of every model input
        self.x_by_tid = {}
        self.x_src = {}                       # tensor id -> device pointer of a caller's batch read in place (Model._stage_x), else the staging tensor
        self.side = torch.cuda.Stream() if (training and rt.model.wgrad_side_stream) else None
        self.step_count = 0
        self.outputs = {}
        self.sync_bn = bool(training and getattr(rt.model, 'sync_bn', False) and parallel.active())
        self.amax_of = {}                     # encoder output tensor id -> arg-max bytes of its 2 x 2 pooling windows (training)
        self._bn_jobs = []
        self._build()
        if self._bn_jobs:
            tab = torch.tensor([[int(v or 0) for v in j] for j in self._bn_jobs], dtype=torch.int64).to(rt.dev)      # satcv_bn_affine_job rows: 6 pointers, c, 2 optional pointers
            self.keep.append(tab)
            nj = len(self._bn_jobs)
            self.fwd.insert(0, lambda st: check(lib.satcv_bn_affine_infer_batched(tab.data_ptr(), nj, BN_EPS, st)))

    # -- helpers
    def _z(self, *shape, dtype=None):
        t = torch.zeros(*shape, dtype=dtype or self.rt.tdtype, device=self.rt.dev)
        self.keep.append(t)
        return t

    def _dims(self, t):
        hh, ww = self.h * t.down, self.w * t.down
        if hh.denominator != 1 or ww.denominator != 1:
            raise ValueError(f'input {self.h}x{self.w} is not divisible by the model downsampling ({1 / t.down})')
        return int(hh), int(ww)

    def _conv_step(self, role='fwd', **kw):
        kw.setdefault('tile_policy', self.tile_policy)
        d = ops.make_conv_desc(**kw)
        self.keep.append(d)
        fn = lambda st, d=d: check(lib.satcv_conv2d_igemm(C.byref(d), st))
        # label + algorithmic work of the launch (tools/step_probe.py, bench.py's per-layer roofline)
        k, cin, cout = kw.get('kh', 1) * kw.get('kw', 1), kw.get('c0', 0) + (kw.get('c1', 0) or 0), kw['cout']
        px = kw['n'] * kw['h'] * kw['w_']
        fn.label = (f"conv_{role} k{kw.get('kh', 1)} d{kw.get('dil', 1)} n{kw['n']} {kw['h']}x{kw['w_']} {kw.get('c0', 0)}+{kw.get('c1', 0) or 0}->{cout}"
                    f"{' d2s' if kw.get('mode_out') else ''}{' s2d' if kw.get('mode_in') else ''}")
        fn.work = dict(kind='conv', role=role, taps=k, px=px, cin=cin, cout=cout, esize=self.rt.esize)
        return fn

    def _src_args(self, r):
        (x0, c0) = r.srcs[0]
        x1, c1 = (r.srcs[1] if len(r.srcs) > 1 else (None, 0))
        a = r.affine
        return dict(x0=x0.data_ptr(), c0=c0, x1=x1.data_ptr() if x1 is not None else None, c1=c1,
                    in_scale=_fp(a['scale']) if a else None, in_shift=_fp(a['shift']) if a else None,
                    in_relu=1 if (a and r.relu) else 0)

    def _bn_forward(self, bnname, stats, ld, off, c, count, updates, aff=None, aoff=0, conv_bias=None, bias_eff=None):
        """emit finalize (train) / affine (infer); returns affine dict of per-channel tensors
        (freshly allocated [c], or the caller's shared arrays written at channel offset aoff)."""
        rt = self.rt
        a = aff or dict(scale=self._z(c, dtype=torch.float32), shift=self._z(c, dtype=torch.float32),
                        mean=self._z(c, dtype=torch.float32), rstd=self._z(c, dtype=torch.float32))
        g, b = rt.pptr(bnname + '/gamma'), rt.pptr(bnname + '/beta')
        mm, mv = rt.sptr(bnname + '/moving_mean'), rt.sptr(bnname + '/moving_var')
        if self.training:
            bessel = 1 if rt.model.bn_bessel else 0
            if self.sync_bn:            # SyncBN: [Σx, Σx²] averaged over replicas before the finalize
                self.fwd.append(lambda st: parallel.allreduce_mean_(stats))
            if bnname in self.frozen:
                # frozen BatchNormalization: the batch statistics are consumed (rows cleared, batch mean / rstd kept for the backward
                # kernels' addressing) but the layer normalises with its MOVING statistics and does not update them
                ts, tt = self._z(c, dtype=torch.float32), self._z(c, dtype=torch.float32)
                self.fwd.append(lambda st: check(lib.satcv_bn_finalize_train(
                    _fp(stats, off), ld, c, float(count), g, b, BN_EPS, BN_MOMENTUM, updates, bessel, None, None,
                    _fp(ts), _fp(tt), _fp(a['mean'], aoff), _fp(a['rstd'], aoff), st)))
                self.fwd.append(lambda st: check(lib.satcv_bn_affine_infer(g, b, mm, mv, BN_EPS, c, _fp(a['scale'], aoff), _fp(a['shift'], aoff), st)))
                return a
            self.fwd.append(lambda st: check(lib.satcv_bn_finalize_train(
                _fp(stats, off), ld, c, float(count), g, b, BN_EPS, BN_MOMENTUM, updates, bessel, mm, mv,
                _fp(a['scale'], aoff), _fp(a['shift'], aoff), _fp(a['mean'], aoff), _fp(a['rstd'], aoff), st)))
        else:
            # inference: scale / shift depend on the parameters only -- every layer's pair is computed by ONE launch at the head of the
            # list (satcv_bn_affine_infer_batched, table built at the end of _build)
            self._bn_jobs.append((g, b, mm, mv, _fp(a['scale'], aoff), _fp(a['shift'], aoff), c, conv_bias, bias_eff))
        return a

    def _materialize(self, t, r, f=1, pooled=None, sink=None, actslot=None):
        """relu(bn(raw)) -> dense activated tensor (and optional pooled / stats).  actslot = (tensor, channel offset,
        channel stride): write into a slice of a shared concatenation buffer instead of a fresh tensor."""
        if not r.relu:
            raise NotImplementedError('materialising a linear (no-ReLU) BatchNorm output')
        (y, c) = r.srcs[0]
        hh, ww = r.h, r.w
        if actslot is None:
            act = self._z(self.n, hh, ww, c)
            act_ptr, act_ld = act.data_ptr(), c
        else:
            act = actslot[0]
            act_ptr, act_ld = actslot[0].data_ptr() + actslot[1] * self.rt.esize, actslot[2]
        st_ptr, ld = (None, 0)
        if sink is not None and self.training:
            st_ptr, ld = _fp(sink[0], sink[1]), sink[2]
        a = r.affine
        dt = self.rt.dtype
        if (self.training and pooled is not None and f == 2 and dt == BF16 and getattr(self.rt.model, 'fuse_pool_bwd', True)
                and hh % 8 == 0 and ww % 32 == 0 and c in (32, 64)):
            # training: also the arg-max byte of every window -- the fused pooled backward (satcv_conv2d_bwd_fused with dpool) routes
            # MaxPooling2D's gradient with it
            amax = self._z(self.n, hh // 2, ww // 2, c, dtype=torch.uint8)
            self.amax_of[t.id] = amax
            self.fwd.append(lambda st: check(lib.satcv_bn_relu_pool_amax(
                y.data_ptr(), _fp(a['scale']), _fp(a['shift']), act_ptr, act_ld, pooled.data_ptr(), amax.data_ptr(),
                st_ptr, ld, self.n, hh, ww, c, f, dt, st)))
            return TRef([(act, c)], self.n, hh, ww) if actslot is None else None
        self.fwd.append(lambda st: check(lib.satcv_bn_relu_pool(
            y.data_ptr(), _fp(a['scale']), _fp(a['shift']), act_ptr, act_ld, pooled.data_ptr() if pooled is not None else None,
            st_ptr, ld, self.n, hh, ww, c, f, dt, st)))
        return TRef([(act, c)], self.n, hh, ww) if actslot is None else None

    # -- lowering
    def _build(self):
        fw = _ForwardLowering(self)
        fw.run()
        self.vals, self.node_ctx = fw.vals, fw.ctx
        if self.training:
            self._build_backward(fw.consumers, fw.vals, fw.ctx)

    def _build_backward(self, consumers, vals, ctx):
        _BackwardLowering(self, consumers, vals, ctx).run()

    # -- execution
    # (a training plan lets EVERY eligible deep 3x3 launch -- also the data gradients that carry no statistics -- run on the 16x16x32 tile;
    #  inference keeps the library default, which preserves bit-identical results across batch splits: csrc/conv_igemm_fast.hip.  Round 6:
    #  the choice travels in each launch's descriptor (satcv_conv_desc.tile_policy, set in _conv_step) -- no process-global option is touched)
    def _run(self, steps, st):
        for s in steps:
            s(st)

    def run_forward(self, st):
        self._run(self.fwd, st)

    def run_backward(self, st):
        self._run(self.bwd, st)


class _ForwardLowering:
    """Lowers model.nodes into plan.fwd: two preparation passes over the concatenations, then one method per op."""
    OPS = ('input', 'cba', 'concat', 'pool', 'convT', 'concat_bn_relu', 'maxpool', 'raw', 'add_relu', 'upsample_head', 'dropout', 'head', 'classes')

    def __init__(self, plan):
        self.plan, self.rt, self.m, self.n = plan, plan.rt, plan.rt.model, plan.n
        self.dt, self.es, self.training = plan.rt.dtype, plan.rt.esize, plan.training
        # the plan's lists and helpers under the names the lowering code uses
        self.fwd, self.keep, self.outputs = plan.fwd, plan.keep, plan.outputs
        self._z, self._dims, self._conv_step, self._src_args = plan._z, plan._dims, plan._conv_step, plan._src_args
        self._bn_forward, self._materialize = plan._bn_forward, plan._materialize
        self.consumers = defaultdict(list)         # tensor id -> the nodes that read it
        for node in self.m.nodes:
            for t in node.inputs:
                self.consumers[t.id].append(node)
        self.vals = {}                             # tensor id -> TRef (stored form: raw + pending affine, or final)
        self.acts = {}                             # tensor id -> TRef of its materialised activation
        self.ctx = {}                              # node id -> what the backward lowering needs of the node (plan.node_ctx)
        self.sinks = {}                            # tensor id -> (statistics rows, channel offset, row stride) of the decoder concat BatchNorm it feeds
        self.cat_stats = {}                        # concat_bn_relu node id -> its statistics rows
        self.slots = {}                            # tensor id -> channel slice of a shared raw concatenation (ASPP branches)
        self.actslots = {}                         # tensor id -> (tensor, channel offset, channel stride) of a shared ACTIVATED concatenation
        self.order = {id(nd): i for i, nd in enumerate(self.m.nodes)}
        self.fused_join = {}                       # add_relu node id -> the shortcut tensor its sum was written into
        self.folded_plain = {}                     # tensor id -> a conv -> BatchNorm branch stored normalised, waiting for the join's other branch

    def run(self):
        self._prepare_concat_stats()
        self._prepare_concat_slots()
        for node in self.m.nodes:
            if node.op not in self.OPS:
                raise NotImplementedError(f'op {node.op}')
            getattr(self, node.op)(node)

    def _prepare_concat_stats(self):
        for node in self.m.nodes:
            if node.op == 'concat_bn_relu':
                a, b = node.inputs
                ctot = a.channels + b.channels
                st = self._z(STAT_ROWS, 2, ctot, dtype=torch.float64)
                self.cat_stats[id(node)] = st
                self.sinks[a.id] = (st, 0, ctot)
                self.sinks[b.id] = (st, a.channels, ctot)

    def _prepare_concat_slots(self):
        n, consumers, sinks = self.n, self.consumers, self.sinks
        for node in self.m.nodes:
            if node.op != 'concat':
                continue
            if all(t.node.op == 'cba' and len(consumers[t.id]) > 1 for t in node.inputs):
                # concatenation of ACTIVATED encoder outputs that are also pooled (Siamese skips): the pool kernels write
                # their activation straight into channel slices of one tensor
                ctot = sum(t.channels for t in node.inputs)
                hh, ww = self._dims(node.inputs[0])
                shared = self._z(n, hh, ww, ctot)
                off = 0
                for t in node.inputs:
                    self.actslots[t.id] = (shared, off, ctot)
                    if node.outputs[0].id in sinks:                      # statistics for the decoder's concat BatchNorm
                        st_, so_, sl_ = sinks[node.outputs[0].id]
                        sinks[t.id] = (st_, so_ + off, sl_)
                    off += t.channels
                self.ctx[id(node)] = dict(act=shared, ctot=ctot)
                continue
            if not all(t.node.op == 'cba' and len(consumers[t.id]) == 1 for t in node.inputs):
                raise NotImplementedError('concatenate is supported for conv_batch_act outputs consumed only by the concat (ASPP)')
            ctot = sum(t.channels for t in node.inputs)
            hh, ww = self._dims(node.inputs[0])
            yshared = self._z(n, hh, ww, ctot)
            stshared = self._z(STAT_ROWS, 2, ctot, dtype=torch.float64) if self.training else None
            aff = dict(scale=self._z(ctot, dtype=torch.float32), shift=self._z(ctot, dtype=torch.float32),
                       mean=self._z(ctot, dtype=torch.float32), rstd=self._z(ctot, dtype=torch.float32))
            off = 0
            for t in node.inputs:
                self.slots[t.id] = dict(y=yshared, off=off, ctot=ctot, stats=stshared, aff=aff)
                off += t.channels
            self.ctx[id(node)] = dict(y=yshared, ctot=ctot, aff=aff)

    def input(self, node):
        p, n, dt = self.plan, self.n, self.dt
        t = node.outputs[0]
        cp = rup(t.channels, 16)
        x = self._z(n, p.h, p.w, cp)
        xin = self._z(n, p.h, p.w, t.channels, dtype=torch.float32)
        p.x_f32 = xin
        p.x_inputs.append(xin)
        p.x_by_tid[t.id] = xin
        npix = n * p.h * p.w
        cc = t.channels
        self.fwd.append(lambda st, xin=xin, x=x, npix=npix, cc=cc, cp=cp, tid=t.id: check(lib.satcv_ingest_nhwc(
            p.x_src.get(tid) or xin.data_ptr(), x.data_ptr(), npix, cc, cp, dt, st)))
        self.vals[t.id] = TRef([(x, cp)], n, p.h, p.w)

    def cba(self, node):
        rt, n, dt, es = self.rt, self.n, self.dt, self.es
        tin, tout = node.inputs[0], node.outputs[0]
        r = self.vals[tin.id]
        lay = node.layer
        pk = rt.packed[lay.name]
        cout = tout.channels
        if cout % 16:
            raise NotImplementedError(f'{lay.name}: filters must be a multiple of 16 (got {cout})')
        if r.c != pk['cin_pad']:
            raise ValueError(f'{lay.name}: input has {r.c} stored channels, kernel expects {pk["cin_pad"]}')
        k, dil = node.attrs['k'], node.attrs['dil']
        stride, relu_out = node.attrs.get('stride', 1), node.attrs.get('relu', True)
        hin, win = r.h, r.w
        if stride > 1:
            if self.training:
                raise NotImplementedError('strided convolutions are inference-only (DeepLab backbone)')
            r = TRef(r.srcs, r.n, (hin - 1) // stride + 1, (win - 1) // stride + 1, r.affine, r.relu)   # output grid
        sl = self.slots.get(tout.id)
        if not node.attrs.get('bn', True):
            # plain Conv2D + bias, no normalisation (atrous CNN family): consumers read the stored values as they are
            if sl is not None or stride > 1:
                raise NotImplementedError('a convolution without BatchNormalization as a concatenation branch / with a stride')
            y = self._z(n, r.h, r.w, cout)
            self.fwd.append(self._conv_step(w=pk['fwd'].data_ptr(), bias=rt.pptr(lay.name + '/bias'), y=y.data_ptr(), ldy=cout, n=n, h=r.h, w_=r.w,
                                            cout=cout, cout_pad=rup(cout, 32), kh=k, kw=k, dil=dil, dtype=dt, **self._src_args(r)))
            self.vals[tout.id] = TRef([(y, cout)], n, r.h, r.w)
            self.ctx[id(node)] = dict(r=r, y=y, yoff=0, ldy=cout, aff=None, aoff=0, cout=cout, k=k, dil=dil)
            return
        strided = dict(stride=stride, hin=hin if stride > 1 else 0, win=win if stride > 1 else 0)
        fold = self._residual_fold(node, r, stride) if (sl is None and not relu_out) else None
        if fold is not None:
            fold_args, sb = fold
            be = self._z(cout, dtype=torch.float32)
            aff = self._bn_forward(lay.bn_name, None, cout, 0, cout, n * r.h * r.w, node.attrs.get('bn_updates', 1),
                                   conv_bias=rt.pptr(lay.name + '/bias'), bias_eff=_fp(be))
            self.fwd.append(self._conv_step(w=pk['fwd'].data_ptr(), bias=_fp(be), out_scale=_fp(aff['scale']), ldy=cout,
                                            n=n, h=r.h, w_=r.w, cout=cout, cout_pad=rup(cout, 32), kh=k, kw=k, dil=dil, dtype=dt,
                                            **strided, **fold_args, **self._src_args(r)))
            self.vals[tout.id] = TRef([(sb, cout)], n, r.h, r.w)
            self.ctx[id(node)] = dict(r=r, y=sb, yoff=0, ldy=cout, aff=None, aoff=0, cout=cout, k=k, dil=dil)
            return
        if sl is None:
            y = self._z(n, r.h, r.w, cout)
            stats = self._z(STAT_ROWS, 2, cout, dtype=torch.float64) if self.training else None
            yoff, ldy, aoff, aff_in = 0, cout, 0, None
        else:           # branch of a concatenation: write into the channel slice of the shared tensor
            y, stats, yoff, ldy, aoff, aff_in = sl['y'], sl['stats'], sl['off'], sl['ctot'], sl['off'], sl['aff']
        self.fwd.append(self._conv_step(w=pk['fwd'].data_ptr(), bias=rt.pptr(lay.name + '/bias'), y=y.data_ptr() + yoff * es, ldy=ldy,
                                        stats=_fp(stats, aoff), stats_ld=ldy, n=n, h=r.h, w_=r.w, cout=cout, cout_pad=rup(cout, 32),
                                        kh=k, kw=k, dil=dil, dtype=dt, **strided, **self._src_args(r)))
        aff = self._bn_forward(lay.bn_name, stats, ldy, aoff, cout, n * r.h * r.w, node.attrs.get('bn_updates', 1), aff_in, aoff)
        if sl is None:
            self.vals[tout.id] = TRef([(y, cout)], n, r.h, r.w, affine=aff, relu=relu_out)
        self.ctx[id(node)] = dict(r=r, y=y, yoff=yoff, ldy=ldy, aff=aff, aoff=aoff, cout=cout, k=k, dil=dil)

    def _residual_fold(self, node, r, stride):
        """inference, residual join (ResNet bottleneck: ReLU(BN(conv) + shortcut), utils-free build-defined DeepLab backbone): when this
        block's output only feeds the join and nothing reads the shortcut afterwards, the convolution applies its own
        BatchNormalization in the epilogue (out_scale / bias_eff from the batched affine launch) and writes
        ReLU(shortcut + result) IN PLACE over the shortcut (accumulate = 2): no add_relu launch, no third tensor
        (20 launches of ~10 us on a single 512 x 512 tile, 11 % of the kernel time at batch 16; SATCV_FUSE_RESIDUAL=0: separate).
        Returns (the launch's y / accumulate arguments, the tensor it writes), or None when the join stays a launch of its own."""
        consumers, vals = self.consumers, self.vals
        tout = node.outputs[0]
        cout, cons = tout.channels, consumers[tout.id]
        if self.training or not FUSE_RESIDUAL or len(cons) != 1 or cons[0].op != 'add_relu' or tout not in cons[0].inputs:
            return None
        join = cons[0]
        tsc = join.inputs[1] if join.inputs[0] is tout else join.inputs[0]      # the join's other addend
        rs_ = vals.get(tsc.id)
        if rs_ is None:
            # (B) the other addend is a conv -> BatchNorm branch that runs LATER in the list (the projection shortcut of a stage's
            # first block): store this branch normalised (its BatchNorm in the epilogue, nothing pending), the later branch
            # then adds itself in place (A)
            if (stride == 1 and tsc.node is not None and tsc.node.op == 'cba' and len(consumers[tsc.id]) == 1
                    and tsc.node.attrs.get('bn', True) and not tsc.node.attrs.get('relu', True) and tsc.channels == cout):
                y = self._z(self.n, r.h, r.w, cout)
                self.folded_plain[tout.id] = y
                return dict(y=y.data_ptr(), accumulate=0), y
            return None
        # (A) the other addend is final: a plain activated tensor written by an earlier join, or a branch stored normalised (B)
        src_ok = (tsc.id in self.folded_plain) or (tsc.node is not None and tsc.node.op == 'add_relu' and stride == 1)
        if (src_ok and not rs_.affine and len(rs_.srcs) == 1 and rs_.srcs[0][1] == cout and rs_.srcs[0][0].shape[-1] == cout
                and (rs_.h, rs_.w) == (r.h, r.w)
                and all(cn is join or self.order[id(cn)] < self.order[id(node)] for cn in consumers[tsc.id])):
            sb = rs_.srcs[0][0]
            self.fused_join[id(join)] = sb
            return dict(y=sb.data_ptr(), accumulate=2), sb
        return None

    def concat(self, node):
        cx = self.ctx[id(node)]
        hh, ww = self._dims(node.inputs[0])
        if 'act' in cx:
            self.vals[node.outputs[0].id] = TRef([(cx['act'], cx['ctot'])], self.n, hh, ww)
        else:
            self.vals[node.outputs[0].id] = TRef([(cx['y'], cx['ctot'])], self.n, hh, ww, affine=cx['aff'], relu=True)

    def pool(self, node):
        p, n, dt = self.plan, self.n, self.dt
        tin, tout = node.inputs[0], node.outputs[0]
        r = self.vals[tin.id]
        f = node.attrs['f']
        if not (r.affine and len(r.srcs) == 1):
            raise NotImplementedError('max-pool expects the output of a conv_batch_act block')
        c = r.c
        if r.h % f or r.w % f:
            raise ValueError(f'input {p.h}x{p.w} is not divisible by the model downsampling (a {r.h}x{r.w} map meets a {f}x{f} pool)')
        pooled = self._z(n, r.h // f, r.w // f, c)
        others = [cn for cn in self.consumers[tin.id] if cn is not node]
        if others:
            self.acts[tin.id] = self._materialize(tin, r, f, pooled, self.sinks.get(tin.id), self.actslots.get(tin.id))
        else:
            (y, _) = r.srcs[0]
            a = r.affine
            hh, ww = r.h, r.w
            self.fwd.append(lambda st, y=y, a=a, pooled=pooled, hh=hh, ww=ww, c=c, f=f: check(lib.satcv_bn_relu_pool(
                y.data_ptr(), _fp(a['scale']), _fp(a['shift']), None, 0, pooled.data_ptr(), None, 0, n, hh, ww, c, f, dt, st)))
        self.vals[tout.id] = TRef([(pooled, c)], n, r.h // f, r.w // f)
        self.ctx[id(node)] = dict(f=f)

    def convT(self, node):
        rt, n = self.rt, self.n
        tin, tout = node.inputs[0], node.outputs[0]
        r = self.vals[tin.id]
        if len(r.srcs) != 1:
            raise NotImplementedError('transposed conv on a concatenated input')
        lay = node.layer
        pk = rt.packed[lay.name]
        cout, f = tout.channels, node.attrs['f']
        if cout % 16:
            raise NotImplementedError(f'{lay.name}: transposed-conv filters must be a multiple of 16')
        u = self._z(n, r.h * f, r.w * f, cout)
        sink = self.sinks.get(tout.id) if self.training else None
        self.fwd.append(self._conv_step(w=pk['fwd'].data_ptr(), bias=rt.pptr(lay.name + '/bias'), y=u.data_ptr(), ldy=cout,
                                        stats=_fp(sink[0], sink[1]) if sink else None, stats_ld=sink[2] if sink else 0,
                                        n=n, h=r.h, w_=r.w, cout=f * f * cout, cout_pad=rup(f * f * cout, 32), kh=1, kw=1, dil=1,
                                        mode_out=1, f=f, cstat=cout, dtype=self.dt, **self._src_args(r)))
        self.vals[tout.id] = TRef([(u, cout)], n, r.h * f, r.w * f)
        self.ctx[id(node)] = dict(r=r, u=u, cout=cout, f=f)

    def concat_bn_relu(self, node):
        vals, acts = self.vals, self.acts
        ta, tb = node.inputs
        tout = node.outputs[0]
        if ta.id not in acts:
            ra0 = vals[ta.id]
            acts[ta.id] = self._materialize(ta, ra0, 1, None, self.sinks.get(ta.id)) if ra0.affine else ra0
        ra, rb = acts[ta.id], vals[tb.id]
        if (ra.h, ra.w) != (rb.h, rb.w):
            raise ValueError(f'concatenation of a {ra.h}x{ra.w} skip with a {rb.h}x{rb.w} up-sampled map: the input size must be divisible by the model downsampling')
        if rb.affine or len(rb.srcs) != 1 or len(ra.srcs) != 1:
            raise NotImplementedError('concat+BN expects (activated skip, transposed-conv output)')
        ca, cb = ra.c, rb.c
        st = self.cat_stats[id(node)]
        aff = self._bn_forward(node.layer.name, st, ca + cb, 0, ca + cb, self.n * ra.h * ra.w, 1)
        vals[tout.id] = TRef([ra.srcs[0], rb.srcs[0]], self.n, ra.h, ra.w, affine=aff, relu=True)
        self.ctx[id(node)] = dict(ra=ra, rb=rb, aff=aff, ca=ca, cb=cb)

    def maxpool(self, node):
        n, dt = self.n, self.dt
        tin, tout = node.inputs[0], node.outputs[0]
        r = self.vals[tin.id]
        if r.affine:
            r = self._materialize(tin, r)
        (src, c) = r.srcs[0]
        kk, ss, pp = node.attrs['k'], node.attrs['s'], node.attrs['pad']
        ho, wo = (r.h + 2 * pp - kk) // ss + 1, (r.w + 2 * pp - kk) // ss + 1
        out = self._z(n, ho, wo, c)
        self.fwd.append(lambda st, src=src, out=out, hh=r.h, ww=r.w, c=c, kk=kk, ss=ss, pp=pp: check(lib.satcv_maxpool(
            src.data_ptr(), out.data_ptr(), n, hh, ww, c, kk, ss, pp, dt, st)))
        self.vals[tout.id] = TRef([(out, c)], n, ho, wo)

    def raw(self, node):
        # the convolution output BEFORE its BatchNormalization (build_acnn_layers feeds it to the next Conv2D, utils/model_tools.py:930)
        r = self.vals[node.inputs[0].id]
        if len(r.srcs) != 1 or node.inputs[0].node.op != 'cba':
            raise NotImplementedError('raw view of a tensor that is not a single convolution output')
        self.vals[node.outputs[0].id] = TRef(r.srcs, self.n, r.h, r.w)

    def add_relu(self, node):
        n, dt, vals, acts = self.n, self.dt, self.vals, self.acts
        ty, tsc = node.inputs
        tout = node.outputs[0]
        if id(node) in self.fused_join:            # written in place by the block's last convolution (_residual_fold)
            sb = self.fused_join[id(node)]
            c = sb.shape[-1]
            vals[tout.id] = TRef([(sb, c)], n, vals[ty.id].h, vals[ty.id].w)
            self.ctx[id(node)] = dict(out=sb, c=c, h=vals[ty.id].h, w=vals[ty.id].w)
            return
        ry, rs = vals[ty.id], vals[tsc.id]
        if rs.affine and rs.relu and len(rs.srcs) == 1:       # shortcut = ReLU(BN(conv)) kept in raw form: activate it once
            if tsc.id not in acts:
                acts[tsc.id] = self._materialize(tsc, rs)
            rs = acts[tsc.id]
        if len(ry.srcs) != 1 or len(rs.srcs) != 1 or ry.relu or (rs.affine and rs.relu):
            raise NotImplementedError('residual join expects linear (BN without ReLU) branches')
        (yb, c), (sb, c2) = ry.srcs[0], rs.srcs[0]
        assert c == c2 and (ry.h, ry.w) == (rs.h, rs.w)
        out = self._z(n, ry.h, ry.w, c)
        ya, sa = ry.affine, rs.affine
        npx = n * ry.h * ry.w
        self.fwd.append(lambda st, yb=yb, sb=sb, out=out, ya=ya, sa=sa, npx=npx, c=c: check(lib.satcv_add_act(
            yb.data_ptr(), _fp(ya['scale']) if ya else None, _fp(ya['shift']) if ya else None, sb.data_ptr(),
            _fp(sa['scale']) if sa else None, _fp(sa['shift']) if sa else None, 1, out.data_ptr(), npx, c, dt, st)))
        vals[tout.id] = TRef([(out, c)], n, ry.h, ry.w)
        self.ctx[id(node)] = dict(out=out, c=c, h=ry.h, w=ry.w)

    def upsample_head(self, node):
        n = self.n
        tin, tout = node.inputs[0], node.outputs[0]
        lg = self.outputs[tin.id]                         # fp32 logits written by the linear head
        hctx = self.ctx[id(tin.node)]
        f = node.attrs['factor']
        act = 0 if node.attrs['activation'] == 'softmax' else 1
        hh, ww, ncls = hctx['r'].h, hctx['r'].w, hctx['ncls']
        probs = self._z(n, hh * f, ww * f, ncls, dtype=torch.float32)
        classes = self._z(*((n, hh * f, ww * f) if act == 0 else (n, hh * f, ww * f, ncls)), dtype=torch.int32)
        th = float(node.attrs.get('thresh', 0.5))
        self.fwd.append(lambda st, lg=lg, probs=probs, classes=classes, hh=hh, ww=ww, ncls=ncls, f=f, act=act, th=th: check(
            lib.satcv_upsample_head(lg.data_ptr(), n, hh, ww, ncls, f, act, th, probs.data_ptr(), classes.data_ptr(), st)))
        self.outputs[tout.id] = probs
        self.ctx[id(node)] = dict(classes=classes)
        if self.training:
            raise NotImplementedError('the up-sampling head is inference-only')

    def dropout(self, node):
        p, n, dt, es, vals = self.plan, self.n, self.dt, self.es, self.vals
        tin, tout = node.inputs[0], node.outputs[0]
        r = vals[tin.id]
        if not self.training:                     # identity at inference (Keras semantics)
            vals[tout.id] = r
            if tin.id in self.acts:
                self.acts[tout.id] = self.acts[tin.id]
            return
        ctot = r.c
        spatial = node.attrs['spatial']
        hw = r.h * r.w
        mask = self._z(*((n, ctot) if spatial else (n * hw, ctot)), dtype=torch.float32)
        out = self._z(n, r.h, r.w, ctot)
        rate = float(node.attrs['rate'])
        slot = len(p.dropouts)
        p.dropouts.append(dict(mask=mask, node=node))
        cnt = mask.numel()

        def gen(st, mask=mask, rate=rate, cnt=cnt, slot=slot):
            # a fresh mask every step: counter = (step, dropout slot)
            check(lib.satcv_dropout_mask(p.rt.dropout_seed, (p.step_count << 8) + slot, rate, cnt, mask.data_ptr(), st))
        self.fwd.append(gen)
        off = 0
        mode = 0 if spatial else 1
        for (src, cs) in r.srcs:             # dual-source (concat) inputs: one launch per source / channel slice
            a = r.affine
            self.fwd.append(lambda st, src=src, cs=cs, off=off, a=a, rl=1 if r.relu else 0, mask=mask, ctot=ctot, mode=mode, out=out,
                            hw=hw: check(lib.satcv_dropout_apply(
                src.data_ptr(), cs, _fp(a['scale'], off) if a else None, _fp(a['shift'], off) if a else None, rl,
                _fp(mask, off), ctot, mode, out.data_ptr() + off * es, ctot, n, hw, cs, dt, st)))
            off += cs
        vals[tout.id] = TRef([(out, ctot)], n, r.h, r.w)
        self.ctx[id(node)] = dict(mask=mask, spatial=spatial, ctot=ctot, hw=hw, r=r)

    def head(self, node):
        rt, n = self.rt, self.n
        tin, tout = node.inputs[0], node.outputs[0]
        r = self.vals[tin.id]
        if len(r.srcs) != 1:
            raise NotImplementedError('head on concatenated input')
        lay = node.layer
        ncls = tout.channels
        act = {'softmax': 0, 'sigmoid': 1, 'linear': 2}[node.attrs['activation']]
        (y, c) = r.srcs[0]
        npix = n * r.h * r.w
        probs = self._z(n, r.h, r.w, ncls, dtype=torch.float32)
        classes = self._z(*((n, r.h, r.w) if act != 1 else (n, r.h, r.w, ncls)), dtype=torch.int32)
        hd = ops.make_head_desc(x=y.data_ptr(), ldx=c, cin=c, w=rt.pptr(lay.name + '/kernel'), b=rt.pptr(lay.name + '/bias'),
                                ncls=ncls, activation=act, npix=npix, dtype=self.dt,
                                in_scale=_fp(r.affine['scale']) if r.affine else None,
                                in_shift=_fp(r.affine['shift']) if r.affine else None,
                                thresh=node.attrs.get('thresh', 0.5), probs=probs.data_ptr(), classes=classes.data_ptr())
        self.keep.append(hd)
        self.fwd.append(lambda st, hd=hd: check(lib.satcv_head_fwd(C.byref(hd), st)))
        self.outputs[tout.id] = probs
        self.ctx[id(node)] = dict(r=r, probs=probs, classes=classes, act=act, ncls=ncls)
        self.plan.head = self.ctx[id(node)]
        self.plan.head_node = node

    def classes(self, node):
        hctx = self.ctx[id(node.inputs[0].node)]
        if 'thresh' in node.attrs:
            node.inputs[0].node.attrs['thresh'] = node.attrs['thresh']
        self.outputs[node.outputs[0].id] = hctx['classes']


# one visit of a conv -> BatchNorm block by the backward lowering: its gradients (da activated, dp pooled, graws of raw consumers), the sums
# buffer (pre: already filled by the producer of da) and whether its weight gradient accumulates
_CbaVisit = namedtuple('_CbaVisit', 'node cx da dp da_ptr graws pre sums accum')


class _BackwardLowering:
    """Lowers the backward pass of a training plan into plan.bwd: one method per op, called for reversed(model.nodes)."""
    OPS = ('head', 'add_relu', 'cba', 'dropout', 'concat', 'pool', 'concat_bn_relu', 'convT')
    HEAD_FAST = {(1, 16), (2, 16), (1, 32), (2, 32), (3, 32), (4, 32), (1, 64), (2, 64)}

    def __init__(self, plan, consumers, vals, ctx):
        self.plan, self.consumers, self.vals, self.ctx = plan, consumers, vals, ctx
        rt = self.rt = plan.rt
        self.m, self.n, self.dt, self.es = rt.model, plan.n, rt.dtype, rt.esize
        plan.dbg = {}                       # layer name -> intermediate gradient tensors (diagnostics only)
        # the plan's lists and helpers under the names the lowering code uses
        self.bwd, self.keep, self.dbg, self.amax_of = plan.bwd, plan.keep, plan.dbg, plan.amax_of
        self._z, self._conv_step, self._src_args = plan._z, plan._conv_step, plan._src_args
        self.frozen, self.raw_bn, self.side, self.sync_bn, self.tile_policy = plan.frozen, plan.raw_bn, plan.side, plan.sync_bn, plan.tile_policy
        self.gact = {}                      # tensor id -> (tensor, channel offset, channels) of the gradient of its activated form
        self.gpool, self.gpool_f = {}, {}   # tensor id -> gradient of its max-pooled form (same triple); -> the pooling factor
        self.graw = {}                      # transposed-conv output id -> gradient of its raw values (a tensor; a dict: what the fused launch needs)
        _cnt = defaultdict(int)
        for nd in self.m.nodes:
            if nd.layer is not None:
                _cnt[nd.layer.name] += 1
        self.shared_layers = {k for k, v in _cnt.items() if v > 1}      # layers applied to several inputs (Siamese encoders)
        self.seen_layers = set()            # layers applied more than once (shared weights): later visits accumulate their gradients
        self.ws_need, self.wdescs = 0, []   # the workspace the weight-gradient launches (side stream) share: bytes, descriptors
        self.fused_ws_need, self.fdescs = 0, []     # the fused thin-layer backward launches run on the MAIN stream: a workspace of their own
        # loss -> dlogits is written by Model.train step into this buffer
        h = plan.head
        self.dlogits = plan.dlogits = self._z(self.n * h['r'].h * h['r'].w, h['ncls'], dtype=torch.float32)
        plan.loss_buf = self._z(1, dtype=torch.float32)
        # ---- sums of an ENCODER block's BatchNorm backward formed by the producers of its two gradients (activated form, see
        # satcv_bn_bwd_finalize2): encoder conv output tensor id -> dict(buf, parts)
        self.act_sums = {}
        self.POOL_SUMS = getattr(rt.model, 'fuse_pool_bn_sums', True) and self.dt == ops.BF16
        self.ident = {}                     # channels -> (ones, zeros) vectors
        self.fused = {}                     # tensor id -> sums buffer whose BN-backward reduce pass was done by the producer of the gradient
        self.head_feed = {}                 # tensor id -> the head launch that writes its gradient
        # data-parallel overlap: after every parameter-bearing node tell the gradient exchange which tail of the flat
        # gradient buffer is final (parallel.GradSync.ready_above)
        pending = self.pending = {}         # layer name -> remaining visits
        for node in self.m.nodes:
            if node.layer is not None and any(ps.name in rt.offsets for ps in node.layer.specs):
                pending[node.layer.name] = pending.get(node.layer.name, 0) + 1
        # layer name -> end of its parameters in the flat buffer
        self.layer_hi = {l.name: max(rt.offsets[ps.name] + ps.size for ps in l.specs if ps.name in rt.offsets)
                         for l in self.m.layers if l.name in pending}
        # a conv_batch_act node also writes the gamma / beta gradients of ITS BatchNormalization (a layer of its own, directly
        # above the convolution in the flat buffer): until the node has run, nothing below the end of that layer is final
        by_name = {l.name: l for l in self.m.layers}
        for node in self.m.nodes:
            bn = getattr(node.layer, 'bn_name', None) if node.op == 'cba' else None
            if bn in by_name and node.layer.name in self.layer_hi:
                his = [rt.offsets[ps.name] + ps.size for ps in by_name[bn].specs if ps.name in rt.offsets]
                if his:
                    self.layer_hi[node.layer.name] = max(self.layer_hi[node.layer.name], max(his))

    def run(self):
        for node in reversed(self.m.nodes):
            if node.op in self.OPS:
                getattr(self, node.op)(node, self.ctx.get(id(node)))
            self.grads_ready(node)
        if self.ws_need:
            ws = self._z(max(self.ws_need // 4, 1), dtype=torch.float32)
            for d in self.wdescs:
                d.workspace, d.workspace_bytes = ws.data_ptr(), self.ws_need
        if self.fused_ws_need:
            wsf = self._z(max(self.fused_ws_need // 4, 1), dtype=torch.float32)
            for d in self.fdescs:
                d.workspace, d.workspace_bytes = wsf.data_ptr(), self.fused_ws_need
        if self.side is not None:
            side, evj = self.side, torch.cuda.Event()

            def join(st):          # the optimizer (main stream) must see every weight gradient
                evj.record(side)
                torch.cuda.current_stream().wait_event(evj)
            self.bwd.append(join)

    # -- helpers
    def bn_bwd_steps(self, da, ldda, dp, lddp, f, yraw, ldy, aff, aoff, sums, sums_off, sums_ld, c, hh, ww, dy, lddy, dbias,
                     dgamma, dbeta, accum=0, linear=0, frozen=False, second=None, act=None, coef=None):
        """(reduce, finalize, apply) steps of one BatchNorm backward; reduce is None where nothing is left for it.
        act: dict(buf=[ROWS][2][c] rows in the ACTIVATED form, parts={'skip', 'pool'}) -- the parts of this layer's gradient whose
        sums a producer already formed (the decoder's concat-BN apply pass for the skip gradient `da`, the data gradient of the next
        encoder block for the pooled gradient `dp`); the separate reduce pass then only covers what is left.
        coef: the coefficient rows where the caller made them (a fused launch reads them), else allocated here."""
        n, dt, es = self.n, self.dt, self.es
        if coef is None:
            coef = self._z(2, c, dtype=torch.float32)
        common = dict(yraw=yraw, ldy=ldy, scale=_fp(aff['scale'], aoff), shift=_fp(aff['shift'], aoff),
                      mean=_fp(aff['mean'], aoff), rstd=_fp(aff['rstd'], aoff), n=n, h=hh, w_=ww, c=c, dtype=dt,
                      f=f, sums=_fp(sums, sums_off), sums_ld=sums_ld, coef=_fp(coef), dy=dy, lddy_out=lddy, dbias=dbias, linear=linear)
        d = ops.make_bnbwd_desc(da=da, ldda=ldda, dpool=dp, lddp=lddp, **common, **(second or {}))
        self.keep.append(d)
        parts = act['parts'] if (act and not frozen) else set()
        need_da, need_dp = da is not None and 'skip' not in parts, dp is not None and 'pool' not in parts
        dr = d
        if parts and (need_da or need_dp):          # reduce pass over the part no producer covered
            dr = ops.make_bnbwd_desc(da=da if need_da else None, ldda=ldda if need_da else 0, dpool=dp if need_dp else None,
                                     lddp=lddp if need_dp else 0, **common)
            self.keep.append(dr)
        cnt = float(n * hh * ww)
        red = lambda st: check(lib.satcv_bn_bwd_reduce(C.byref(dr), st))
        red.label = f"bn_bwd_reduce n{n} {hh}x{ww} c{c} f{f}{' (part)' if dr is not d else ''}"
        red.work = dict(kind='bn_bwd_reduce', px=n * hh * ww, c=c, esize=es)
        if parts and not (need_da or need_dp):
            red = None
        if parts:
            abuf = act['buf']
            fin0 = lambda st: check(lib.satcv_bn_bwd_finalize2(_fp(sums, sums_off) if red is not None else None, sums_ld, _fp(abuf), c, c, cnt,
                                                               _fp(aff['scale'], aoff), _fp(aff['shift'], aoff), _fp(aff['mean'], aoff),
                                                               _fp(aff['rstd'], aoff), dgamma, dbeta, _fp(coef), accum, st))
        else:
            fin0 = lambda st: check(lib.satcv_bn_bwd_finalize(_fp(sums, sums_off), sums_ld, c, cnt, dgamma, dbeta, _fp(coef), accum, st))
        if self.sync_bn:
            def fin(st):            # SyncBN: Σdy, Σdy·x̂ averaged over replicas (linear + idempotent, so the whole buffer is reduced)
                parallel.allreduce_mean_(sums)
                if parts:
                    parallel.allreduce_mean_(act['buf'])
                fin0(st)
        else:
            fin = fin0
        app = lambda st: check(lib.satcv_bn_bwd_apply(C.byref(d), st))
        app.label = f"bn_bwd_apply n{n} {hh}x{ww} c{c} f{f}"
        app.work = dict(kind='bn_bwd_apply', px=n * hh * ww, c=c, esize=es)
        app.coef = coef
        if frozen:
            # inference-mode BatchNormalization: dy = scale * g * mask, no batch-statistics terms (coef stays 0), no dgamma / dbeta
            def fin_frozen(st):
                sums.zero_()
                coef.zero_()
                if act:
                    act['buf'].zero_()
            return None, fin_frozen, app
        return red, fin, app

    def ident_vecs(self, c):
        if c not in self.ident:
            self.ident[c] = (torch.ones(c, dtype=torch.float32, device=self.rt.dev), torch.zeros(c, dtype=torch.float32, device=self.rt.dev))
            self.keep.append(self.ident[c])
        return self.ident[c]

    def act_sums_for(self, t):
        """the registry entry of encoder output t (a conv -> BN -> ReLU node that is pooled AND used as a skip), or None"""
        if not self.POOL_SUMS or t.node.op != 'cba' or not t.node.attrs.get('bn', True) or not t.node.attrs.get('relu', True):
            return None
        if t.node.layer.bn_name in self.frozen or t.node.layer.bn_name in self.raw_bn or t.node.layer.name in self.shared_layers:
            return None
        if t.id not in self.act_sums:
            self.act_sums[t.id] = dict(buf=self._z(STAT_ROWS, 2, t.channels, dtype=torch.float64), parts=set())
        return self.act_sums[t.id]

    def fuse_target(self, t):
        """bnr_* fields (and the sums buffer) if the head's backward kernel can also do the reduce pass of the BN+ReLU
        that produced its input tensor `t` (the raw values are in its registers anyway); None otherwise."""
        if not self.rt.model.fuse_head_bn_bwd or t.id in self.gact or len(self.consumers[t.id]) != 1:
            return None
        P, pc = t.node, self.ctx.get(id(t.node))
        if P.op != 'cba' or pc['yoff'] != 0 or pc['ldy'] != pc['cout']:
            return None
        c, aff = pc['cout'], pc['aff']
        sums = self._z(STAT_ROWS, 2, c, dtype=torch.float64)
        return dict(mean=_fp(aff['mean']), rstd=_fp(aff['rstd']), sums=_fp(sums), sums_ld=c), sums

    def bst_target(self, t):
        """(bst fields, channels) if the data-gradient launch that writes dL/d t -- t the activated output of a
        conv -> BN -> ReLU node or of the decoder's BN over [skip, up] -- may also form the sums of that BatchNorm's backward
        (satcv.h: bst_*): the gradient has this one contributor, so the tile in the accumulators IS the whole gradient."""
        if (not getattr(self.rt.model, 'fuse_dgrad_bn_bwd', True) or self.dt != ops.BF16 or t.id in self.gact or t.id in self.gpool
                or len(self.consumers[t.id]) != 1):
            return None
        P, pc = t.node, self.ctx.get(id(t.node))
        if P.op == 'cba' and P.attrs.get('bn', True) and P.layer.bn_name not in self.frozen:
            c, aff, aoff = pc['cout'], pc['aff'], pc['aoff']
            b = dict(y=pc['y'].data_ptr() + pc['yoff'] * self.es, ld=pc['ldy'], relu=1 if P.attrs.get('relu', True) else 0)
        elif P.op == 'concat_bn_relu' and P.layer.name not in self.frozen:
            ra, rb, aff, ca, cb = pc['ra'], pc['rb'], pc['aff'], pc['ca'], pc['cb']
            if (P.inputs[1].node.op == 'convT' and BIAS_NOISE) or ca % 8:
                return None            # (the two-launch form of that BN backward keeps its own reduce passes)
            c, aoff = ca + cb, 0
            b = dict(y=ra.srcs[0][0].data_ptr(), ld=ca, y1=rb.srcs[0][0].data_ptr(), ld1=cb, split=ca, relu=1)
        else:
            return None
        b.update(scale=_fp(aff['scale'], aoff), shift=_fp(aff['shift'], aoff), mean=_fp(aff['mean'], aoff), rstd=_fp(aff['rstd'], aoff))
        return b, c

    def act_form_unfit(self, t):
        """t is the output of a BatchNorm with a zero gamma: its backward sums cannot be rebuilt from the activation (the fused
        backward kernels' in-loader activation included) -- the separate reduce pass over the raw output forms them"""
        P = t.node
        return (P.op == 'cba' and P.layer.bn_name in self.raw_bn) or (P.op == 'concat_bn_relu' and P.layer.name in self.raw_bn)

    def sums_below(self, fz, tin, sa, cinp):
        """offer a fused launch fz, whose input tin is a BatchNorm + ReLU fed only by this gradient, the sums of THAT layer's backward
        (what satcv_bn_bwd_reduce would compute in a pass over dx and that layer's raw output): bst_*.  Returns the sums buffer or None."""
        bt = self.bst_target(tin) if (sa['in_relu'] and sa['in_scale'] is not None and not self.act_form_unfit(tin)) else None
        if bt is None or bt[1] != cinp or bt[0].get('relu', 0) != 1:
            return None
        sums = self._z(STAT_ROWS, 2, cinp, dtype=torch.float64)
        fz.bst_sums, fz.bst_sums_ld, fz.bst_mean, fz.bst_rstd = _fp(sums), cinp, bt[0]['mean'], bt[0]['rstd']
        return sums

    def dgrad_step(self, t, **kw):
        """data-gradient launch writing the activation gradient of tensor t (and, where the kernel can, the sums of the
        BatchNorm backward of the node that produced t: one pass over two tensors less per such layer)"""
        vals = self.vals
        # the gradient of a max-pooled encoder output: this launch sees the pooled activation p = maxpool(relu(BN(y_enc))) (its own
        # input), so its epilogue can form the pooled part of that BatchNorm's backward sums in the activated form -- sum dp [p > 0],
        # sum dp p (bst_* with unit scale / rstd and zero shift / mean on the pooled tensor)
        kw.setdefault('tile_policy', self.tile_policy)        # (the dry-run probes below must ask for the tile family the launch will get)
        if (self.POOL_SUMS and not kw.get('accumulate') and t.node.op == 'pool' and len(self.consumers[t.id]) == 1 and t.id not in self.gact
                and len(vals[t.id].srcs) == 1 and vals[t.id].affine is None):
            ent = self.act_sums_for(t.node.inputs[0])
            if ent is not None and vals[t.id].srcs[0][1] == kw['cout'] == t.node.inputs[0].channels:
                one, zero = self.ident_vecs(kw['cout'])
                kwp = dict(kw, bst=dict(y=vals[t.id].srcs[0][0].data_ptr(), ld=kw['cout'], scale=_fp(one), shift=_fp(zero), mean=_fp(zero),
                                        rstd=_fp(one), relu=1), stats=_fp(ent['buf']), stats_ld=kw['cout'])
                probe = ops.make_conv_desc(**kwp)
                if lib.satcv_conv2d_igemm_pipelined(C.byref(probe)) == 1:
                    ent['parts'].add('pool')
                    fn = self._conv_step(role='dgrad', **kwp)
                    fn.label += ' +poolsums'
                    return fn
        bt = None if kw.get('accumulate') else self.bst_target(t)
        # where it pays (measured per layer of the five-level U-Net, batch 64): the extra tile read hides under a
        # K loop of >= 1152 (3x3 x 128 channels) and under the 1x1 kernels.  The thin and middle layers are HBM-bound
        # themselves -- there the read costs the conv what the separate pass had cost -- and the thin ones run on the
        # persistent weights-stationary kernel, which does not carry the sums.
        kdepth = kw.get('kh', 1) * kw.get('kw', 1) * (kw.get('c0', 0) + (kw.get('c1', 0) or 0))
        # (128 -> 256 at 64 x 64, the one K = 1152 layer whose output is wider than its input, measured +49 us against -41 us)
        pays = FUSE_DGRAD_ALL or kdepth >= 2304 or (kdepth >= 1152 and kw['cout'] <= kw.get('c0', 0)) or kw.get('kh', 1) == 1
        if bt is not None and bt[1] == kw['cout'] and pays:
            sums = self._z(STAT_ROWS, 2, bt[1], dtype=torch.float64)
            kw2 = dict(kw, bst=bt[0], stats=_fp(sums), stats_ld=bt[1])
            probe = ops.make_conv_desc(**kw2)
            if lib.satcv_conv2d_igemm_pipelined(C.byref(probe)) == 1:
                self.fused[t.id] = sums
                fn = self._conv_step(role='dgrad', **kw2)
                fn.label += ' +bnred'
                return fn
        return self._conv_step(role='dgrad', **kw)

    def wgrad_step(self, r, dy, lddy, lay, cin_real, cout, hh, ww, k, dil, f=0, accum=0, last=False):
        rt, n = self.rt, self.n
        sa = self._src_args(r)
        if sa['x1'] is not None and sa['c0'] % 8:
            raise NotImplementedError(f'{lay.name}: training a convolution over a concatenation needs a first part of a multiple of 8 channels '
                                      f'(got {sa["c0"]}); inference has no such limit')
        d = ops.make_wgrad_desc(dy=dy, lddy=lddy, dw=rt.gptr(lay.name + '/kernel'), cin=cin_real, cout=cout, n=n, h=hh, w_=ww,
                                dtype=self.dt, kh=k, kw=k, dil=dil, mode_dy=1 if f else 0, f=f if f else 1, transposed=1 if f else 0, accumulate=accum,
                                whole_chip=1 if last else 0, **sa)
        nb = lib.satcv_conv2d_wgrad_workspace(C.byref(d))
        if nb < 0:
            raise RuntimeError(lib.satcv_last_error().decode())
        self.ws_need = max(self.ws_need, nb)
        self.wdescs.append(d)
        self.keep.append(d)
        if self.side is None:
            run = lambda st: check(lib.satcv_conv2d_wgrad(C.byref(d), st))
        else:
            # weight gradient and data gradient of a layer only share their INPUT (dy): run the weight gradients on a
            # second HIP stream so that their load/MFMA/store phases interleave with the main stream's kernels
            ev = torch.cuda.Event()
            side, sptr = self.side, C.c_void_p(self.side.cuda_stream)

            def run(st):
                ev.record(torch.cuda.current_stream())
                side.wait_event(ev)
                check(lib.satcv_conv2d_wgrad(C.byref(d), sptr))
        run.label = f"wgrad k{k} d{dil} n{n} {hh}x{ww} {sa['c0']}+{sa['c1']}->{cout}{' convT f%d' % f if f else ''}"
        run.work = dict(kind='wgrad', taps=(f * f if f else k * k), px=n * hh * ww, cin=cin_real, cout=cout, esize=self.es)
        return run

    def conv_dgrad(self, tin, dy, cout, pk, r, k, dil):
        """data gradient of a convolution into dL/d tin, added where that tensor already holds a gradient (several consumers)"""
        n, hh, ww, cinp = self.n, r.h, r.w, r.c
        prev = self.gact.get(tin.id)
        if prev is not None and (prev[1] != 0 or prev[2] != cinp):
            raise NotImplementedError('gradient fan-in into a channel slice')
        gin = prev[0] if prev is not None else self._z(n, hh, ww, cinp)
        self.bwd.append(self.dgrad_step(tin, x0=dy.data_ptr(), c0=cout, w=pk['dgrad'].data_ptr(), y=gin.data_ptr(), ldy=cinp,
                                        n=n, h=hh, w_=ww, cout=cinp, cout_pad=rup(cinp, 32), kh=k, kw=k,
                                        dil=dil, dtype=self.dt, accumulate=1 if prev is not None else 0))
        return gin

    def set_grad(self, tin, lay, gin, cinp):
        self.gact[tin.id] = (gin, 0, cinp)
        self.dbg['dx:' + lay.name] = gin

    def dbg_ctx(self, lay, da, dp, cx):
        self.dbg['_ctx:' + lay.name] = dict(da=da, dp=dp, **{k: cx[k] for k in ('y', 'yoff', 'ldy', 'aff', 'aoff', 'cout')})

    def grads_ready(self, node):
        """bookkeeping of the node just finished: once a layer has had all its visits, the tail of the flat gradient buffer above the
        layers still pending is final"""
        lay, pending = node.layer, self.pending
        if lay is None or lay.name not in pending:
            return
        pending[lay.name] -= 1
        if pending[lay.name] == 0:
            del pending[lay.name]
        lo = max((self.layer_hi[k] for k in pending), default=0)
        plan, rt, m = self.plan, self.rt, self.m

        def ckpt(st, lo=lo):
            sync = getattr(m, '_sync_grads', None)
            if sync is not None and hasattr(sync, 'ready_above'):
                sync.ready_above(rt.gflat, lo, plan.side)
        self.bwd.append(ckpt)

    # -- one method per op
    def head(self, node, cx):
        rt, n = self.rt, self.n
        r = cx['r']
        (y, c) = r.srcs[0]
        dx = self._z(n, r.h, r.w, c)
        lay = node.layer
        hb = None
        ft = self.fuse_target(node.inputs[0]) if (cx['ncls'], c) in self.HEAD_FAST and r.affine else None
        if ft is not None:
            hb = dict(mean=ft[0]['mean'], rstd=ft[0]['rstd'], sums=ft[0]['sums'], sums_ld=ft[0]['sums_ld'])
            self.fused[node.inputs[0].id] = ft[1]
        hd = ops.make_head_desc(x=y.data_ptr(), ldx=c, cin=c, w=rt.pptr(lay.name + '/kernel'), b=rt.pptr(lay.name + '/bias'),
                                ncls=cx['ncls'], activation=cx['act'], npix=n * r.h * r.w, dtype=self.dt,
                                in_scale=_fp(r.affine['scale']) if r.affine else None,
                                in_shift=_fp(r.affine['shift']) if r.affine else None,
                                dlogits=self.dlogits.data_ptr(), dx=dx.data_ptr(), lddx=c,
                                dw=rt.gptr(lay.name + '/kernel'), db=rt.gptr(lay.name + '/bias'), bnr=hb)
        self.keep.append(hd)
        self.bwd.append(lambda st, hd=hd: check(lib.satcv_head_bwd(C.byref(hd), st)))
        nb = lib.satcv_head_bwd_workspace(C.byref(hd))
        if nb > 0:            # per-workgroup partial rows + an ordered sum instead of float atomics: reproducible dW / db
            part = self._z(nb // 4, dtype=torch.float32)
            hd.partials = part.data_ptr()
            self.bwd.append(lambda st, hd=hd: check(lib.satcv_head_bwd_finalize(C.byref(hd), st)))
        self.gact[node.inputs[0].id] = (dx, 0, c)
        # (the block under the head may form this gradient itself from the logit gradients: see _thin_fused)
        self.head_feed[node.inputs[0].id] = dict(hd=hd, ncls=cx['ncls'], c=c, w=rt.pptr(lay.name + '/kernel'), wname=lay.name + '/kernel',
                                                 fused_reduce=ft is not None)

    def add_relu(self, node, cx):
        # out = ReLU(BN(conv) + shortcut): the masked gradient g * (out > 0) belongs to BOTH addends.  It is formed in place
        # and handed to the branch's (linear) BN backward and to the shortcut; a tensor that already holds a gradient
        # (several consumers) receives it by addition.
        n, dt, gact = self.n, self.dt, self.gact
        g = gact.get(node.outputs[0].id)
        if g is None or cx is None:
            return
        c, hh, ww, out = cx['c'], cx['h'], cx['w'], cx['out']
        if g[1] != 0 or g[2] != c:
            raise NotImplementedError('residual-join gradient in a channel slice')
        gb, cnt = g[0], n * hh * ww * c
        self.bwd.append(lambda st, out=out, gb=gb, cnt=cnt: check(lib.satcv_relu_bwd(out.data_ptr(), gb.data_ptr(), cnt, dt, st)))
        for t in node.inputs:
            prev = gact.get(t.id)
            if prev is None:
                gact[t.id] = (gb, 0, c)
            else:
                if prev[1] != 0 or prev[2] != c:
                    raise NotImplementedError('gradient fan-in into a channel slice')
                self.bwd.append(lambda st, pb=prev[0], gb=gb, npx=n * hh * ww, c=c: check(lib.satcv_add_act(
                    pb.data_ptr(), None, None, gb.data_ptr(), None, None, 0, pb.data_ptr(), npx, c, dt, st)))

    def plain_cba(self, node, cx):
        # plain Conv2D: the gradient of its stored output is the incoming one as it is
        rt, n, dt = self.rt, self.n, self.dt
        tin, tout = node.inputs[0], node.outputs[0]
        da = self.gact.get(tout.id)
        if da is None:
            return
        lay, r, cout = node.layer, cx['r'], cx['cout']
        if da[1] != 0 or da[2] != cout:
            raise NotImplementedError('plain-convolution gradient in a channel slice')
        hh, ww, dyb = r.h, r.w, da[0]
        accum = 1 if lay.name in self.seen_layers else 0
        self.seen_layers.add(lay.name)
        bpart = self._z(max(lib.satcv_bias_grad_workspace(n * hh * ww, cout) // 4, 1), dtype=torch.float32)
        self.bwd.append(lambda st, dyb=dyb, cout=cout, npx=n * hh * ww, db=rt.gptr(lay.name + '/bias'), bpart=bpart: check(lib.satcv_bias_grad(
            dyb.data_ptr(), cout, npx, cout, dt, db, bpart.data_ptr(), st)))
        pk = rt.packed[lay.name]
        self.bwd.append(self.wgrad_step(r, dyb.data_ptr(), cout, lay, pk['cin'], cout, hh, ww, cx['k'], cx['dil'], accum=accum))
        if tin.node.op != 'input':
            gin = self.conv_dgrad(tin, dyb, cout, pk, r, cx['k'], cx['dil'])
            self.gact[tin.id] = (gin, 0, r.c)

    def cba(self, node, cx):
        if not node.attrs.get('bn', True):
            return self.plain_cba(node, cx)
        rt, es = self.rt, self.es
        tout = node.outputs[0]
        da, dp = self.gact.get(tout.id), self.gpool.get(tout.id)
        graws = [self.gact[cn.outputs[0].id] for cn in self.consumers.get(tout.id, []) if cn.op == 'raw' and cn.outputs[0].id in self.gact]
        if da is None and dp is None:
            if graws:
                raise NotImplementedError('a convolution consumed only through its un-normalised output')
            return
        lay, r, cout = node.layer, cx['r'], cx['cout']
        pre = self.fused.get(tout.id)
        sums = pre if pre is not None else self._z(STAT_ROWS, 2, cout, dtype=torch.float64)
        accum = 1 if lay.name in self.seen_layers else 0
        self.seen_layers.add(lay.name)
        v = _CbaVisit(node, cx, da, dp, da[0].data_ptr() + da[1] * es if da is not None else None, graws, pre, sums, accum)
        # what the two fused forms share: one input, no consumer of the raw output, no bias noise, a 3 x 3 undilated kernel, a gradient
        # laid out like the raw output, no gradient of the input yet and a layer applied once (a shared layer's other visit may have its
        # weight gradient in flight on the side stream)
        fusable = (self.dt == ops.BF16 and da is not None and not graws and not BIAS_NOISE and cx['k'] == 3 and cx['dil'] == 1 and da[2] == cx['ldy']
                   and self.gact.get(node.inputs[0].id) is None and lay.name not in self.shared_layers)
        if fusable and dp is None and self._thin_fused(v) is not None:
            return
        dy = self._z(self.n, r.h, r.w, cout)
        bn = self.bn_bwd_steps(v.da_ptr, da[2] if da is not None else 0, dp[0].data_ptr() if dp is not None else None,
                               cout, self.gpool_f.get(tout.id, 1), cx['y'].data_ptr() + cx['yoff'] * es, cx['ldy'], cx['aff'], cx['aoff'], sums, 0, cout, cout,
                               r.h, r.w, dy.data_ptr(), cout, rt.gptr(lay.name + '/bias') if BIAS_NOISE else None,
                               rt.gptr(lay.bn_name + '/gamma'), rt.gptr(lay.bn_name + '/beta'), accum,
                               linear=0 if node.attrs.get('relu', True) else 1, frozen=lay.bn_name in self.frozen,
                               act=self.act_sums.get(tout.id) if (self.act_sums.get(tout.id) or {}).get('parts') else None)
        if fusable and dp is not None and self._pooled_fused(v, bn) is not None:
            return
        self._separate(v, bn, dy)

    def _fused_desc(self, v, coef, want_dx=True, **kw):
        """(satcv_conv2d_bwd_fused descriptor, source arguments, data-gradient tensor or None) of a conv -> BN (-> ReLU) block"""
        rt, n, es, cx = self.rt, self.n, self.es, v.cx
        lay, r, aff, aoff, cout = v.node.layer, cx['r'], cx['aff'], cx['aoff'], cx['cout']
        pk, sa = rt.packed[lay.name], self._src_args(r)
        gin = self._z(n, r.h, r.w, r.c) if want_dx else None
        fz = ops.make_bwdf_desc(g=v.da_ptr, yraw=cx['y'].data_ptr() + cx['yoff'] * es, ldg=cx['ldy'], bn_scale=_fp(aff['scale'], aoff), bn_shift=_fp(aff['shift'], aoff),
                                bn_mean=_fp(aff['mean'], aoff), bn_rstd=_fp(aff['rstd'], aoff), bn_coef=_fp(coef),
                                w_dgrad=pk['dgrad'].data_ptr() if want_dx else None, dx=gin.data_ptr() if want_dx else None, lddx=r.c if want_dx else 0,
                                dw=rt.gptr(lay.name + '/kernel'), cin=pk['cin'], cout=cout, n=n, h=r.h, w_=r.w, dtype=self.dt, accumulate=v.accum, **kw, **sa)
        return fz, sa, gin

    def _emit_fused(self, v, fz, nb, red, fin, gin, suffix, dyparts, **work):
        """the steps and records of an accepted fused backward launch: whose workspace, BatchNorm reduce / finalize, the launch itself"""
        n, cx, lay = self.n, v.cx, v.node.layer
        r, cout = cx['r'], cx['cout']
        self.fused_ws_need = max(self.fused_ws_need, nb)
        self.fdescs.append(fz)
        self.keep.append(fz)
        self.bwd += [fin] if (v.pre is not None or red is None) else [red, fin]
        fstep = lambda st: check(lib.satcv_conv2d_bwd_fused(C.byref(fz), st))
        fstep.label = f"bwd_fused k3 n{n} {r.h}x{r.w} {fz.c0}+{fz.c1}->{cout}{suffix}"
        fstep.work = dict(kind='bwd_fused', taps=9, px=n * r.h * r.w, cin=fz.cin, cout=cout, esize=self.es, **work)
        self.bwd.append(fstep)
        if gin is not None:
            self.set_grad(v.node.inputs[0], lay, gin, r.c)
        self.dbg['dyparts:' + lay.name] = dict(g=v.da, **{k: cx[k] for k in ('y', 'yoff', 'ldy', 'aff', 'aoff', 'cout')}, **dyparts)
        self.dbg_ctx(lay, v.da, v.dp, cx)
        return fstep

    def _thin_fused(self, v):
        """thin full- / half-resolution layers: ONE launch forms dy = BN-backward(g, y) in registers and uses the tile for
        the data gradient AND the weight gradient (csrc/conv_bwd_fused.hip): 4 tensor passes instead of 7, no dy tensor.
        None when the model or the library's workspace query refuses it."""
        node, cx = v.node, v.cx
        rt, tin, tout, lay, r, cout = self.rt, node.inputs[0], node.outputs[0], node.layer, cx['r'], cx['cout']
        if not getattr(rt.model, 'fuse_thin_bwd', True) or tin.node.op == 'input':
            return None
        cinp = r.c
        coef = self._z(2, cout, dtype=torch.float32)
        fz, sa, gin = self._fused_desc(v, coef, linear=0 if node.attrs.get('relu', True) else 1)
        sums_below = self.sums_below(fz, tin, sa, cinp)
        # ... and, for the block under the 1 x 1 head, the gradient g itself: two logit gradients per pixel instead of the
        # head's dx tensor written and read back (2 x 64 bytes per pixel)
        hf = self.head_feed.get(tout.id)
        if (hf is not None and getattr(rt.model, 'fuse_head_grad', True) and hf['ncls'] == 2 and hf['c'] == cout == 32 and cinp == 32
                and hf['fused_reduce'] and v.pre is not None and len(self.consumers.get(tout.id, [])) == 1):
            fz.hg_dlogits, fz.hg_w, fz.hg_ncls = self.dlogits.data_ptr(), hf['w'], 2
            if lib.satcv_conv2d_bwd_fused_workspace(C.byref(fz)) < 0:
                fz.hg_dlogits, fz.hg_w, fz.hg_ncls = None, None, 0
            else:
                hf['hd'].dx = None                      # satcv_head_bwd keeps its dW / db and the fused sums, stores no dx
        nbf = lib.satcv_conv2d_bwd_fused_workspace(C.byref(fz))
        if nbf < 0 and sums_below is not None:              # (the 64 -> 64 form does not carry the sums)
            fz.bst_sums, fz.bst_sums_ld, fz.bst_mean, fz.bst_rstd = None, 0, None, None
            sums_below = None
            nbf = lib.satcv_conv2d_bwd_fused_workspace(C.byref(fz))
        if nbf < 0:
            return None
        if sums_below is not None:
            self.fused[tin.id] = sums_below
        # (the launch applies the BatchNorm backward itself: of the three steps only reduce and finalize are used)
        red, fin, _ = self.bn_bwd_steps(v.da_ptr, v.da[2], None, 0, 1, cx['y'].data_ptr() + cx['yoff'] * self.es, cx['ldy'], cx['aff'], cx['aoff'], v.sums, 0,
                                        cout, cout, r.h, r.w, None, 0, None, rt.gptr(lay.bn_name + '/gamma'), rt.gptr(lay.bn_name + '/beta'), v.accum,
                                        linear=fz.linear, frozen=lay.bn_name in self.frozen, coef=coef)
        dyparts = dict(coef=coef, linear=fz.linear)
        if fz.hg_dlogits:
            dyparts['head'] = (self.dlogits, hf['wname'])
        return self._emit_fused(v, fz, nbf, red, fin, gin, f"{' +bnred' if fz.bst_sums else ''}{' +headgrad' if fz.hg_dlogits else ''}", dyparts)

    def _pooled_fused(self, v, bn):
        """encoder blocks of the full- / half-resolution levels: the pooled BatchNorm apply + weight gradient (+ data gradient)
        in ONE launch (satcv_conv2d_bwd_fused with dpool / amax): no dy tensor, no separate weight-gradient launch.  `bn`: the block's
        (reduce, finalize, apply) steps -- the launch reads the coefficients the finalize writes.  None when refused."""
        node, dp = v.node, v.dp
        rt, tin, tout, lay = self.rt, node.inputs[0], node.outputs[0], node.layer
        red, fin, app = bn
        amax = self.amax_of.get(tout.id)
        if (amax is None or not getattr(rt.model, 'fuse_pool_bwd', True) or self.gpool_f.get(tout.id, 1) != 2 or dp[1] != 0
                or lay.bn_name in self.frozen):
            return None
        want_dx = tin.node.op != 'input'
        cinp = v.cx['r'].c
        fzp, sa, ginp = self._fused_desc(v, app.coef, want_dx, linear=0, dpool=dp[0].data_ptr(), lddp=dp[2], amax=amax.data_ptr())
        # its input is the max-pooled output of the block below: the pooled part of THAT block's sums, activated form
        ent = None
        if (want_dx and self.POOL_SUMS and tin.node.op == 'pool' and len(self.consumers[tin.id]) == 1 and sa['in_scale'] is None
                and len(self.vals[tin.id].srcs) == 1 and tin.node.inputs[0].channels == cinp):
            ent = self.act_sums_for(tin.node.inputs[0])
        if ent is not None:
            fzp.bst_sums, fzp.bst_sums_ld, fzp.bst_act_form = _fp(ent['buf']), cinp, 1
        nbp = lib.satcv_conv2d_bwd_fused_workspace(C.byref(fzp))
        if nbp < 0:
            return None
        if ent is not None:
            ent['parts'].add('pool')
        return self._emit_fused(v, fzp, nbp, red, fin, ginp, f" pooled{'' if want_dx else ' nodx'}{' +poolsums' if fzp.bst_sums else ''}",
                                dict(coef=app.coef, linear=0, dp=dp, amax=amax), nodx=not want_dx, pooled=True)

    def _separate(self, v, bn, dy):
        """BatchNorm reduce / finalize / apply into dy, then the weight gradient (side stream) and the data gradient as launches of their own"""
        rt, n, dt, node, cx = self.rt, self.n, self.dt, v.node, v.cx
        tin, lay, r, cout = node.inputs[0], node.layer, cx['r'], cx['cout']
        red, fin, app = bn
        hh, ww = r.h, r.w
        self.bwd += [fin, app] if (v.pre is not None or red is None) else [red, fin, app]
        for gr in v.graws:            # consumers of the un-normalised output add their gradient to dy (and to the bias gradient)
            if gr[1] != 0 or gr[2] != cout:
                raise NotImplementedError('raw-output gradient in a channel slice')
            bpart = self._z(max(lib.satcv_bias_grad_workspace(n * hh * ww, cout) // 4, 1), dtype=torch.float32)
            self.bwd.append(lambda st, dy=dy, gb=gr[0], npx=n * hh * ww, cout=cout, db=rt.gptr(lay.name + '/bias'), bpart=bpart: (
                check(lib.satcv_bias_grad(gb.data_ptr(), cout, npx, cout, dt, db, bpart.data_ptr(), st)),
                check(lib.satcv_add_act(dy.data_ptr(), None, None, gb.data_ptr(), None, None, 0, dy.data_ptr(), npx, cout, dt, st))))
        self.dbg['dy:' + lay.name] = dy
        self.dbg_ctx(lay, v.da, v.dp, cx)
        pk = rt.packed[lay.name]
        # a layer's weight gradient (second stream) is enqueued BEFORE its data gradient -- it starts beside its own layer's data gradient and
        # the side stream finishes earlier
        # (the weight gradient of a layer fed by a model input is the last launch of the backward pass: nothing runs beside it)
        self.bwd.append(self.wgrad_step(r, dy.data_ptr(), cout, lay, pk['cin'], cout, hh, ww, cx['k'], cx['dil'], accum=v.accum,
                                        last=tin.node.op == 'input' and len(self.m.inputs) == 1 and switches.read('wgrad_last_full')))
        if tin.node.op != 'input':
            self.set_grad(tin, lay, self.conv_dgrad(tin, dy, cout, pk, r, cx['k'], cx['dil']), r.c)

    def dropout(self, node, cx):
        n, dt = self.n, self.dt
        tin, tout = node.inputs[0], node.outputs[0]
        g = self.gact.get(tout.id)
        if g is None or cx is None:
            return
        if g[1] != 0 or g[2] != cx['ctot']:
            raise NotImplementedError('dropout gradient in a channel slice')
        gt, mask, ctot, hw = g[0], cx['mask'], cx['ctot'], cx['hw']
        mode = 0 if cx['spatial'] else 1
        self.bwd.append(lambda st, gt=gt, mask=mask, ctot=ctot, hw=hw, mode=mode: check(lib.satcv_dropout_apply(
            gt.data_ptr(), ctot, None, None, 0, _fp(mask), ctot, mode, gt.data_ptr(), ctot, n, hw, ctot, dt, st)))
        self.gact[tin.id] = (gt, 0, ctot)

    def concat(self, node, cx):
        g = self.gact.get(node.outputs[0].id)
        if g is None:
            return
        off = 0
        for t in node.inputs:          # each branch sees its channel slice of the gradient
            self.gact[t.id] = (g[0], g[1] + off, g[2])
            off += t.channels

    def pool(self, node, cx):
        tin, tout = node.inputs[0], node.outputs[0]
        if tout.id in self.gact:
            if self.gact[tout.id][1] != 0:
                raise NotImplementedError('pooled gradient in a channel slice')
            self.gpool[tin.id] = self.gact[tout.id]
            self.gpool_f[tin.id] = cx['f']

    def concat_bn_relu(self, node, cx):
        rt, n, dt, es, consumers = self.rt, self.n, self.dt, self.es, self.consumers
        ta, tb = node.inputs
        tout = node.outputs[0]
        g = self.gact.get(tout.id)
        if g is None:
            return
        ra, rb, aff, ca, cb = cx['ra'], cx['rb'], cx['aff'], cx['ca'], cx['cb']
        ctot = ca + cb
        hh, ww = ra.h, ra.w
        pre = self.fused.get(tout.id)
        sums = pre if pre is not None else self._z(STAT_ROWS, 2, ctot, dtype=torch.float64)
        dskip = self._z(n, hh, ww, ca)
        du = self._z(n, hh, ww, cb)
        bn = node.layer.name
        upl = tb.node.layer
        if g[2] != ctot:
            raise NotImplementedError('decoder concat gradient in a channel slice')
        gptr_ = g[0].data_ptr() + g[1] * es
        if not (tb.node.op == 'convT' and BIAS_NOISE) and ca % 8 == 0:
            # ONE reduce / finalize / apply over the whole concatenation: the gradient of the concatenated tensor is read
            # once per pass in full lines (the two half launches each touched every line of it for half of its bytes)
            # the skip is the activated output of an encoder block that is also max-pooled: this apply pass has dskip and that
            # activation in registers -- it also forms the skip part of the encoder BatchNorm's backward sums (sk_sums)
            sec = dict(yraw1=rb.srcs[0][0].data_ptr(), ldy1=cb, dy1=du.data_ptr(), lddy1=cb, c_split=ca)
            # round 5: the `up` channels' part of this apply pass, the transposed convolution's data gradient and its weight gradient as ONE
            # launch (satcv_convt_bwd_fused, built at the convT node): the apply pass then covers the skip channels only
            ctbf = None
            cxt = self.ctx.get(id(tb.node)) if tb.node.op == 'convT' else None
            if (CTBF and dt == ops.BF16 and cxt is not None and bn not in self.frozen and upl.name not in self.shared_layers and cxt['f'] == 2
                    and cb in CTBF_COUTS and len(consumers.get(tb.id, [])) == 1):
                rT = cxt['r']
                saT = self._src_args(rT)
                probe = ops.make_ctbf_desc(g=gptr_ + ca * es, ldg=ctot, yup=rb.srcs[0][0].data_ptr(), ldy=cb, bn_scale=None, bn_shift=None, bn_mean=None,
                                           bn_rstd=None, bn_c1=None, bn_c2=None, x=saT['x0'], ldx=saT['c0'], w_dgrad=rt.packed[upl.name]['dgrad'].data_ptr(),
                                           w_npad=rup(rT.c, 32), dx=saT['x0'], lddx=rT.c, dw=rt.gptr(upl.name + '/kernel'), cin=rT.c, cout=cb, n=n,
                                           h=rT.h, w_=rT.w, dtype=dt)
                if saT['x1'] is None and saT['c0'] == rT.c == rt.packed[upl.name]['cin'] and lib.satcv_convt_bwd_fused_workspace(C.byref(probe)) > 0:
                    ctbf = dict(g=gptr_ + ca * es, ldg=ctot, yup=rb.srcs[0][0].data_ptr(), ldy=cb, aff=aff, aoff=ca, ctot=ctot)
                    sec['dy1'] = None
            ent = None
            if (bn not in self.frozen and ta.id not in self.gact and any(cn.op == 'pool' for cn in consumers[ta.id])
                    and len([cn for cn in consumers[ta.id] if cn.op != 'pool']) == 1 and ta.channels == ca):
                ent = self.act_sums_for(ta)
            if ent is not None:
                sec.update(sk_sums=_fp(ent['buf']), sk_sums_ld=ca)
                ent['parts'].add('skip')
            r_, f_, a_ = self.bn_bwd_steps(gptr_, ctot, None, 0, 1, ra.srcs[0][0].data_ptr(), ca, aff, 0, sums, 0, ctot, ctot, hh, ww,
                                           dskip.data_ptr(), ca, None, rt.gptr(bn + '/gamma'), rt.gptr(bn + '/beta'), frozen=bn in self.frozen,
                                           second=sec)
            if ent is not None:
                a_.label += ' +skipsums'
            if ctbf is not None:
                a_.label += ' (skip half)'
                a_.work = dict(kind='bn_bwd_apply', px=n * hh * ww, c=ca, esize=es)
                ctbf['coef'] = a_.coef
            self.bwd += [f_, a_] if (pre is not None or r_ is None) else [r_, f_, a_]
            self.graw[tb.id] = ctbf if ctbf is not None else du
        else:
            ra_, fa_, aa_ = self.bn_bwd_steps(gptr_, ctot, None, 0, 1, ra.srcs[0][0].data_ptr(), ca, aff, 0, sums, 0, ctot, ca, hh, ww,
                                              dskip.data_ptr(), ca, None, rt.gptr(bn + '/gamma'), rt.gptr(bn + '/beta'), frozen=bn in self.frozen)
            rb_, fb_, ab_ = self.bn_bwd_steps(gptr_ + ca * es, ctot, None, 0, 1, rb.srcs[0][0].data_ptr(), cb, aff, ca, sums, ca, ctot, cb,
                                              hh, ww, du.data_ptr(), cb, rt.gptr(upl.name + '/bias') if (tb.node.op == 'convT' and BIAS_NOISE) else None,
                                              rt.gptr(bn + '/gamma') + 4 * ca, rt.gptr(bn + '/beta') + 4 * ca, frozen=bn in self.frozen)
            self.bwd += [fa_, fb_, aa_, ab_] if (pre is not None or ra_ is None) else [ra_, rb_, fa_, fb_, aa_, ab_]
            self.graw[tb.id] = du
        # the skip is the activated output of an encoder conv_batch_act block
        self.gact[ta.id] = (dskip, 0, ca)
        self.dbg['dskip:' + bn] = dskip
        self.dbg['du:' + bn] = du

    def convT(self, node, cx):
        rt, n, dt = self.rt, self.n, self.dt
        tin, tout = node.inputs[0], node.outputs[0]
        du = self.graw.get(tout.id)
        if du is None:
            return
        lay, r, cout, f = node.layer, cx['r'], cx['cout'], cx['f']
        pk = rt.packed[lay.name]
        cinp = r.c
        gin = self._z(n, r.h, r.w, cinp)
        if isinstance(du, dict):
            # fused: BatchNorm-backward apply of the `up` channels + data gradient + weight gradient (csrc/convt_bwd_fused.hip)
            cb_, sa = du, self._src_args(r)
            af_, ao_, ct_ = cb_['aff'], cb_['aoff'], cb_['ctot']
            fz = ops.make_ctbf_desc(g=cb_['g'], ldg=cb_['ldg'], yup=cb_['yup'], ldy=cb_['ldy'], bn_scale=_fp(af_['scale'], ao_), bn_shift=_fp(af_['shift'], ao_),
                                    bn_mean=_fp(af_['mean'], ao_), bn_rstd=_fp(af_['rstd'], ao_), bn_c1=_fp(cb_['coef'], ao_), bn_c2=_fp(cb_['coef'], ct_ + ao_),
                                    x=sa['x0'], ldx=sa['c0'], in_scale=sa['in_scale'], in_shift=sa['in_shift'], in_relu=sa['in_relu'],
                                    w_dgrad=pk['dgrad'].data_ptr(), w_npad=rup(cinp, 32), dx=gin.data_ptr(), lddx=cinp, dw=rt.gptr(lay.name + '/kernel'),
                                    cin=cinp, cout=cout, n=n, h=r.h, w_=r.w, dtype=dt)
            sums_below = self.sums_below(fz, tin, sa, cinp)
            if sums_below is not None:
                self.fused[tin.id] = sums_below
            nbc = lib.satcv_convt_bwd_fused_workspace(C.byref(fz))
            if nbc <= 0:
                raise RuntimeError('convt_bwd_fused: the probe accepted this shape, the final descriptor did not')
            wsc = self._z(max(nbc // 4, 1), dtype=torch.float32)
            fz.workspace, fz.workspace_bytes = wsc.data_ptr(), nbc
            self.keep.append(fz)
            cstep = lambda st: check(lib.satcv_convt_bwd_fused(C.byref(fz), st))
            cstep.label = f"convt_bwd_fused n{n} {r.h}x{r.w} {cinp}<-4x{cout}{' +bnred' if fz.bst_sums else ''}"
            cstep.work = dict(kind='convt_bwd_fused', px=n * r.h * r.w, cin=cinp, cout=cout, esize=self.es)
            self.bwd.append(cstep)
        else:
            self.bwd.append(self.wgrad_step(r, du.data_ptr(), cout, lay, pk['cin'], cout, r.h, r.w, 1, 1, f=f))      # (before its data gradient, as in _separate)
            self.bwd.append(self.dgrad_step(tin, x0=du.data_ptr(), c0=cout, w=pk['dgrad'].data_ptr(), y=gin.data_ptr(), ldy=cinp, n=n, h=r.h,
                                            w_=r.w, cout=cinp, cout_pad=rup(cinp, 32), kh=1, kw=1, dil=1, mode_in=1, f=f, dtype=dt))
        self.set_grad(tin, lay, gin, cinp)
