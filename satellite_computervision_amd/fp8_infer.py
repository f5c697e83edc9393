"""Folded inference of the plain U-Net and the Siamese U-Net, in bf16 (the default `predict` of bf16 models) or FP8 (OCP e4m3fn) -- BASELINE
config 5 ("1024x1024 large-tile sliding-window inference, fp8 MFMA conv path").  The reference has no reduced-precision path (all arithmetic
fp32); this is the north-star's extension and is checked against the fp32 path of this build / the oracle by IoU.

Folded graph (inference only, `utils/model_tools.py:174-415` semantics):
  * every tensor in HBM is the ACTIVATED output relu(bn(conv)), stored as bf16 (scale 1) or as fp8 with one scale per tensor,
    value = q * fp8;  q comes from a calibration run of the bf16/fp32 plan (`Model.enable_fp8_inference`);
  * weights are bf16, or fp8 with one scale per output channel;
  * BatchNorm (moving statistics), conv bias and all quantisation scales are folded into ONE per-channel multiplier and
    bias applied to the fp32 accumulator in the conv epilogue (`satcv_conv_desc.out_scale` / `bias`):
        out8 = Q( relu( acc * (q_in*w_scale*bn_scale/q_out) + (bn_scale*b + bn_shift)/q_out ) )
  * max-pool is fused into the producing conv's epilogue where the pipelined kernel takes the shape, else it runs on the stored values
    directly (monotone);
  * concat([skip, up]) -> BN -> ReLU: the transposed conv applies its half of the BatchNorm in its epilogue.  In bf16, and in fp8 where the
    thin-layer kernel serves the consumers, the concatenation is NOT materialised: the up-sampled half gets its own tensor and the consumer
    conv reads (skip, up) as two sources, the skip half's BN + ReLU in its loader.  Otherwise (fp8, general tiled kernel) the transposed conv
    writes its channel slice of the concatenation and `satcv_affine_requant` re-quantises the skip half into the other;
  * hybrid (fp8 store, default): the full- and half-resolution levels keep bf16 tensors and run on the bf16 kernels, the levels below run in
    e4m3; a pooled map / a transposed conv's input crossing the boundary is (de-)quantised by one `satcv_affine_requant` pass.
MFMA: v_mfma_f32_32x32x16_fp8_fp8 (bf16 rate, half the operand bytes in HBM and LDS).
Siamese graphs (utils/model_tools.py:576-663): the two dates of a shared encoder / ASPP layer run as one launch over 2n images whose
epilogue stores straight into the channel concatenation (satcv_conv_desc pair store), or, with pair=False, as one launch per date into the
same channel slices; see _FoldedLowering (one method per op; cba and pool serve both the single-date and the two-date part).
"""
import ctypes as C
from collections import namedtuple

import torch

from . import ops, switches
from ._lib import lib, check, FP8, FP8X, BF16
from .engine import rup

USE_SCALED_MFMA = switches.read('fp8_scaled')      # (2x the bf16 rate)
FUSE_POOL = switches.read('fuse_pool')
HYBRID = switches.read('fp8_hybrid')               # (Fp8Plan)
THIN_FP8 = switches.read('fp8_thin')
SIAMESE_PAIR = switches.read('siamese_pair')       # the epilogue remaps the store into the channel concatenation (satcv_conv_desc pair_n); off: Fp8Plan(pair=False)

E4M3_MAX = 448.0
BN_EPS = 1e-3
B16 = torch.bfloat16


def _relu_amax(t, scale, shift):
    return float((t.float() * scale + shift).clamp_min_(0).amax())


def siamese_graph(model):
    """True for graphs with channel concatenations (make_siamese_unet): the folded plan lowers them when asked to (enable_folded_inference /
    enable_fp8_inference); the automatic folded default of bf16 models stays on the plain U-Net graphs."""
    return any(nd.op == 'concat' for nd in model.nodes)


def calibrate(model, x):
    """Per-tensor activation maxima of the folded graph from one run of the regular inference plan on `x`
    (ndarray / device tensor NHWC).  Returns {tensor id: q} with q = amax / 448."""
    n, h, w, _ = model._shape_of(x)
    plan = model._head_plan(n, h, w, False)
    model._stage_x(plan, x)
    plan.run_forward(ops.stream_ptr())
    torch.cuda.synchronize()
    q = {}

    def put(tid, amax):
        q[tid] = max(amax, 1e-12) / E4M3_MAX
    for node in model.nodes:
        cx = plan.node_ctx.get(id(node))
        if node.op == 'input':
            # (a resident float32 batch is read in place by the ingest kernel -- Model._stage_x sets plan.x_src and holds the tensor --
            #  so the staging tensor then holds zeros or an older batch: take the maximum of the tensor that was actually ingested)
            tid = node.outputs[0].id
            held = getattr(plan, '_x_hold', {}).get(tid) if plan.x_src.get(tid) else None
            put(tid, float((held if held is not None else plan.x_by_tid[tid]).abs().amax()))
        elif node.op == 'cba':
            y, aff, c = cx['y'], cx['aff'], cx['cout']
            yoff, ldy, aoff = cx['yoff'], cx['ldy'], cx.get('aoff', 0)
            if yoff != 0 or ldy != c:           # branch of a concatenation (ASPP): its channel slice of the shared tensor
                y = y.reshape(-1, ldy)[:, yoff:yoff + c]
            put(node.outputs[0].id, _relu_amax(y, aff['scale'][aoff:aoff + c], aff['shift'][aoff:aoff + c]))
        elif node.op == 'concat_bn_relu':
            ra, rb, aff, ca = cx['ra'], cx['rb'], cx['aff'], cx['ca']
            a = _relu_amax(ra.srcs[0][0], aff['scale'][:ca], aff['shift'][:ca])
            b = _relu_amax(rb.srcs[0][0], aff['scale'][ca:], aff['shift'][ca:])
            put(node.outputs[0].id, max(a, b))
    return q


class _Stored(namedtuple('_Stored', 't c h w q dual', defaults=(None,))):
    """A tensor of the folded graph as its consumers find it: value = q * t.
      t        the stored tensor (n or 2n, h, w, c): bf16, or uint8 holding e4m3.  None: the output of a shared layer that went into a channel
               slice of a concatenation -- it is read only through that concatenation and through its pooled map
      c, h, w  stored channels (the input bands padded to 16) and map size
      q        1.0 for bf16 storage, the tensor's fp8 scale otherwise.  None: the bf16 input bands of a graph whose every other tensor is
               e4m3 (first_bf16 without hybrid) -- the conv block behind them runs in bf16 and quantises in a pass of its own
      dual     _TwoSource: concat([skip, up]) that was not materialised -- t is the skip half, only a conv block may read it"""
    __slots__ = ()

    @property
    def b16(self):
        return self.t.dtype == B16


# the up-sampled half x1 of a two-source read: c0 skip + c1 up channels, in_scale / in_shift the loader's affine (+ ReLU) over all c0 + c1
_TwoSource = namedtuple('_TwoSource', 'x1 c0 c1 in_scale in_shift')

# what convT leaves for its concat_bn_relu: `dst` is the up-sampled half's own tensor where the concatenation is read as two sources (split),
# else the materialised concatenation whose channels [ca, ca + cb) it wrote; q the concatenation's scale, (scale, shift) its BatchNorm
_Cat = namedtuple('_Cat', 'dst ca cb q scale shift h w b16 split')

# one conv launch of a conv block: images [img0, img0 + n) of the source (and of the pooled map) into channels [choff, choff + cout) of y
_Launch = namedtuple('_Launch', 'img0 n y choff ldy pair', defaults=(None,))


class Fp8Plan:
    """Static launch list of the folded bf16 / fp8 forward for one (n, h, w)."""

    def __init__(self, model, n, h, w, q, first_bf16=True, store=FP8, hybrid=None, pair=None):
        # store = BF16: the same folded graph with bf16 tensors and no quantisation (every scale 1) -- BatchNorm in the conv epilogues
        # instead of the consumers' loaders, activations written once
        # hybrid (fp8 store only, default on: SATCV_FP8_HYBRID=0 turns it off): the full- and half-resolution levels keep bf16 tensors and
        # run on the bf16 kernels, the levels below run in fp8.  The thin high-resolution layers are HBM-bound and have a persistent
        # weights-stationary kernel, fused pooling and a two-source loader only in bf16 (their fp8 forms went through the general tiled
        # kernel plus a requantisation pass per concatenation and were SLOWER than bf16: 1.32 vs 0.83 ms per batch of 64); the deep
        # layers are where e4m3 pays, on the block-scaled K = 64 MFMA at twice the bf16 rate.
        # pair (Siamese graphs, default SATCV_SIAMESE_PAIR): a shared layer's two dates as one launch with a pair store; False: one launch
        # per date into the same channel slices (the bit-exact yardstick of the remap)
        self.model, self.n, self.h, self.w, self.first_bf16, self.store = model, n, h, w, first_bf16, store
        self.hybrid = (HYBRID if hybrid is None else bool(hybrid)) and store == FP8
        self.pair = SIAMESE_PAIR if pair is None else bool(pair)
        self.fwd, self.keep, self.outputs, self.x_by_tid = [], [], {}, {}
        _FoldedLowering(self, q).run()

    def run_forward(self, st):
        for f in self.fwd:
            f(st)


class _FoldedLowering:
    """Lowers model.nodes into plan.fwd, one method per op: op(node, tw).  tw is None on the single-date part of a graph.  On the two-date
    part of a Siamese graph it is the id of the node's twin tensor: the shared layers' weights and moving statistics are the same for both
    dates, so the two calls of a layer are lowered ONCE, over the 2n images of a tensor that holds date d in images [d n, d n + n)."""
    OPS = ('input', 'cba', 'pool', 'dropout', 'concat', 'convT', 'concat_bn_relu', 'head', 'classes')
    TWO_DATE_OPS = ('input', 'cba', 'pool', 'dropout', 'concat')

    def __init__(self, plan, q):
        self.plan, self.m, self.rt, self.dev = plan, plan.model, plan.model.runtime, plan.model.runtime.dev
        self.n, self.h, self.w, self.store = plan.n, plan.h, plan.w, plan.store
        self.fwd, self.keep, self.outputs, self.x_by_tid = plan.fwd, plan.keep, plan.outputs, plan.x_by_tid
        self.tdt = B16 if self.store == BF16 else torch.float8_e4m3fn
        self.esz = 2 if self.store == BF16 else 1
        self.bf16_bands = plan.first_bf16 or self.store == BF16 or plan.hybrid     # the input bands are ingested as bf16 (else: scaled e4m3)
        self.consumers = {}                                # tensor id -> the nodes that read it
        for node in self.m.nodes:
            for t in node.inputs:
                self.consumers.setdefault(t.id, []).append(node)
        self.vals = {}                                     # tensor id -> _Stored
        self.prepooled = {}                                # conv output tensor id -> _Stored of its max-pooled map, written by the conv epilogue
        self.cats = {}                                     # concat_bn_relu node id -> _Cat left by its transposed conv
        self.catbuf = {}                                   # concat node id -> the tensor its producers write (pair concat: n images, ASPP slots: 2n)
        # date: tensor id -> 0 / 1 on the two-date part; twin: tensor id -> the same layers applied to the other date;
        # group: tensor id -> representative of the tensors that share one stored tensor and so one fp8 scale (_dates)
        self.date, self.twin, self.group = self._dates()
        self.qgroup = {}                                   # group -> its fp8 scale: the largest calibrated scale (q) of its tensors
        for tid, v in (q.items() if self.store == FP8 else ()):
            self.qgroup[self.group(tid)] = max(v, self.qgroup.get(self.group(tid), 0.0))
        self.seen = set()                                  # two-date tensors whose node was met while its twin's was still to come
        self.x2 = None                                     # the 2n-image bf16 band tensor of a pair of inputs of which one is still to come
        self.class_map = None                              # the head's class tensor, for the `classes` node

    def run(self):
        for node in self.m.nodes:
            if node.op not in self.OPS:
                raise NotImplementedError(f'fp8 inference: op {node.op} is not lowered (plain and Siamese U-Net graphs only)')
            if not (node.outputs and node.outputs[0].id in self.date):
                getattr(self, node.op)(node, None)
            elif self._later_twin(node):
                getattr(self, node.op)(node, self.twin[node.outputs[0].id])

    def _later_twin(self, node):
        """True at the LATER of the two twin nodes of a two-date op, where it is lowered for both dates: the node list need not interleave
        the dates (the second input may be staged after the first date's encoder), and the launch reads both.  An input is lowered at its
        own node: one staging slot per input."""
        op, tout = node.op, node.outputs[0]
        if tout.id in self.vals:
            return False
        tw = self.twin.get(tout.id)
        if tw is None:
            raise NotImplementedError(f'folded inference: a {op} applied to one date only')
        if op not in self.TWO_DATE_OPS:
            raise NotImplementedError(f'folded inference: op {op} on the two-date part of a Siamese graph')
        if op == 'input' or tw in self.seen:
            return True
        self.seen.add(tout.id)
        return False

    # ---- helpers
    def _put(self, tout, tw, v):
        self.vals[tout.id] = v
        if tw is not None:
            self.vals[tw] = v

    def _whole(self, v):
        """`v` for an op that reads one stored tensor"""
        if v.dual is not None:
            raise NotImplementedError('folded inference: only a conv block may consume the (skip, up) pair')
        return v

    def _hi(self, hh, ww):
        """True where a map of hh x ww pixels is stored in bf16: everywhere in the unquantised graph, the full- and half-resolution levels
        of the hybrid one."""
        return self.store == BF16 or (self.plan.hybrid and hh * ww * 4 >= self.h * self.w)

    def _divisible(self, hh, ww, f):
        if hh % f or ww % f:
            raise ValueError(f'input {self.h}x{self.w} is not divisible by the model downsampling')

    def _z(self, *shape, dtype=None):
        dtype = dtype or self.tdt
        t = torch.zeros(*shape, dtype=torch.uint8 if dtype == torch.float8_e4m3fn else dtype, device=self.dev)
        self.keep.append(t)
        return t

    def _f32(self, t):
        t = t.to(torch.float32).contiguous()
        self.keep.append(t)
        return t

    def _bn(self, name):
        rt = self.rt
        g, b = rt.get_param(name + '/gamma'), rt.get_param(name + '/beta')
        mm, mv = rt.get_param(name + '/moving_mean'), rt.get_param(name + '/moving_var')
        s = g / torch.sqrt(mv + BN_EPS)
        return s, b - mm * s

    def _pack(self, kernel, cin_pad, transposed, b16=False, thin=False):
        """operand image + per-output-channel scale of a Keras kernel: e4m3 with one scale per output channel, or bf16 (scale 1).
        thin: plain e4m3 items even where Cin % 64 == 0 -- the persistent thin-layer kernel's form (its layers are HBM-bound: the
        block-scaled MFMA's rate buys nothing there, the kernel's fused pooling / two-source loader do)."""
        if self.store == BF16 or b16:
            fwd, _ = ops.pack_weights(kernel.contiguous(), cin_pad, BF16, transposed=transposed, want_dgrad=False)
            self.keep.append(fwd)
            return fwd, 1.0, BF16
        if transposed:                                  # (f, f, cout, cin)
            amax = kernel.abs().amax(dim=(0, 1, 3))
            wscale = amax.clamp_min(1e-12) / E4M3_MAX
            kq = kernel / wscale.view(1, 1, -1, 1)
        else:                                           # (kh, kw, cin, cout)
            amax = kernel.abs().amax(dim=(0, 1, 2))
            wscale = amax.clamp_min(1e-12) / E4M3_MAX
            kq = kernel / wscale.view(1, 1, 1, -1)
        dt = FP8X if (USE_SCALED_MFMA and cin_pad % 64 == 0 and not thin) else FP8
        fwd, _ = ops.pack_weights(kq.contiguous(), cin_pad, dt, transposed=transposed, want_dgrad=False)
        self.keep.append(fwd)
        return fwd, wscale, dt

    def _dates(self):
        """Two-date structure of a Siamese graph (make_siamese_unet): tensor id -> date (0: input a, 1: input b) of every tensor computed
        from one input alone, tensor id -> its twin (the same layers applied to the other date), and a scale group per tensor -- twins,
        the two halves of a concatenation and the branches of an ASPP slot tensor share one tensor (and so one fp8 scale)."""
        m = self.m
        date, sig, bysig = {}, {}, {}
        if len(m.inputs) == 2:
            for d, t in enumerate(m.inputs):
                date[t.id], sig[t.id] = d, ('input',)
                bysig[(sig[t.id], d)] = t.id
        for node in m.nodes:
            ds = {date.get(t.id, -1) for t in node.inputs}
            if node.op == 'input' or len(ds) != 1 or -1 in ds:
                continue
            d = ds.pop()
            for t in node.outputs:
                date[t.id] = d
                sig[t.id] = (node.op, id(node.layer) if node.layer is not None else None, node.attrs.get('f'), node.attrs.get('dil'),
                             tuple(sig[u.id] for u in node.inputs))
                bysig[(sig[t.id], d)] = t.id
        twin = {tid: bysig[(sig[tid], 1 - d)] for tid, d in date.items() if (sig[tid], 1 - d) in bysig}
        parent = {}

        def find(t):
            while parent.get(t, t) != t:
                t = parent[t]
            return t

        def union(a, b):
            parent[find(a)] = find(b)
        for a_, b_ in twin.items():
            union(a_, b_)
        for node in m.nodes:
            if node.op == 'concat':
                for t in node.inputs:
                    union(t.id, node.outputs[0].id)
        return date, twin, find

    def _qof(self, tid):
        """fp8 scale of a tensor: that of its group (_dates) -- its own calibrated scale where it shares its tensor with no other"""
        return self.qgroup[self.group(tid)] if self.store == FP8 else 1.0

    def _tr_serves(self, b16, k, dil, cin_s, cout, ww):
        """True where conv_thin_roles.hip takes the launch (igemm_tr_launch: it has no pair store, and its K order differs from the
        weights-stationary kernel that would take the paired launch): such a shared layer keeps one launch per date on it."""
        on, thin = C.c_int(0), C.c_int(0)
        check(lib.satcv_get_option(b'thin_roles', C.byref(on)))
        check(lib.satcv_get_option(b'igemm_thin', C.byref(thin)))
        return (b16 and on.value > 0 and thin.value > 0 and k == 3 and dil == 1 and cout in (32, 64) and ww % 32 == 0 and cin_s in (16, 32, 64)
                and (cin_s == 32 or on.value >= 2) and not (cin_s == 64 and cout == 64))

    def _conv(self, dtype=None, out_relu=1, **kw):
        dtype = dtype if dtype is not None else self.store
        d = ops.make_conv_desc(dtype=dtype, out_relu=out_relu, **kw)
        self.keep.append(d)
        self.fwd.append(lambda st, d=d: check(lib.satcv_conv2d_igemm(C.byref(d), st)))

    def _pool_fuses(self, conv_kw, pool_kw):
        """True where the pipelined conv kernel takes the launch with the max-pool in its epilogue"""
        return bool(lib.satcv_conv2d_igemm_pipelined(C.byref(ops.make_conv_desc(out_relu=1, **conv_kw, **pool_kw))))

    def _requant(self, src, c, npix, sc, sh, relu, dt_in, dt_out, dst, ldd=None):
        """channels [0, c) of dst (row stride ldd) = Q(sc * src + sh), ReLU'd first where `relu`; sc, sh per channel (float32, kept)"""
        ldd = ldd or c
        self.fwd.append(lambda st: check(
            lib.satcv_affine_requant(src.data_ptr(), c, sc.data_ptr(), sh.data_ptr(), relu, dst.data_ptr(), ldd, npix, c, dt_in, dt_out, st)))

    def _rescale(self, v, scale, dt_in, dt_out, dst):
        """dst = Q(scale * v.t): a tensor changing storage between the bf16 and the fp8 levels of the hybrid graph"""
        sc = self._f32(torch.full((v.c,), float(scale), device=self.dev))
        sh = self._f32(torch.zeros(v.c, device=self.dev))
        self._requant(v.t, v.c, v.t.shape[0] * v.h * v.w, sc, sh, 0, dt_in, dt_out, dst)

    def _to_fp8_level(self, pooled, qp):
        """`pooled` (bf16, written by a bf16 level) belongs to the fp8 levels: quantise it (small: a quarter of the level above).  qp: the
        scale calibrated for the un-pooled activation -- max-pooling cannot exceed it."""
        pq = self._z(pooled.t.shape[0], pooled.h, pooled.w, pooled.c)
        self._rescale(pooled, 1.0 / qp, BF16, FP8, pq)
        return pooled._replace(t=pq, q=qp)

    # ---- ops
    def input(self, node, tw):
        n, h, w = self.n, self.h, self.w
        t = node.outputs[0]
        cp = rup(t.channels, 16)
        xin = self._z(n, h, w, t.channels, dtype=torch.float32)
        self.x_by_tid[t.id] = xin
        npix, cc = n * h * w, t.channels
        if tw is not None and not self.bf16_bands:
            raise NotImplementedError('folded inference: a Siamese graph with fp8 input bands')
        if not self.bf16_bands:
            x8 = self._z(n, h, w, cp)
            inv = 1.0 / self._qof(t.id)
            self.fwd.append(lambda st: check(lib.satcv_ingest_nhwc_scaled(xin.data_ptr(), x8.data_ptr(), npix, cc, cp, inv, FP8, st)))
            self.vals[t.id] = _Stored(x8, cp, h, w, self._qof(t.id))
            return
        # the input bands stay bf16 and the first conv block runs on the bf16 kernel: e4m3's 3 mantissa bits on
        # the reflectances themselves were measured to flip ~1 % of confidently classified pixels
        if tw is None:
            xb, img0 = self._z(n, h, w, cp, dtype=B16), 0
        else:                                              # date d of a pair of inputs: images [d n, d n + n) of one tensor
            if self.x2 is None:
                self.x2 = self._z(2 * n, h, w, cp, dtype=B16)
            xb, img0 = self.x2, self.date[t.id] * n
            if tw in self.x_by_tid:
                self.x2 = None                             # (both inputs staged: the next pair of inputs would get its own tensor)
        dst = xb.data_ptr() + img0 * h * w * cp * 2
        self.fwd.append(lambda st: check(lib.satcv_ingest_nhwc(xin.data_ptr(), dst, npix, cc, cp, BF16, st)))
        self.vals[t.id] = _Stored(xb, cp, h, w, 1.0 if self._hi(h, w) else None)

    def cba(self, node, tw):
        """conv -> BatchNorm -> ReLU (-> max-pool) as one launch per destination: the checks and the cut of the kernel here, operands
        and epilogue vectors in _folded_conv, where the launches store in _dest_two_date / its single-date line below."""
        tin, tout, lay = node.inputs[0], node.outputs[0], node.layer
        src = self.vals[tin.id]
        if tw is not None and (src.t is None or src.q is None):
            raise NotImplementedError(f'{lay.name}: input of a shared layer not lowered')
        if node.attrs.get('stride', 1) != 1 or not node.attrs.get('relu', True):
            raise NotImplementedError('fp8 inference: strided / linear conv blocks are not lowered')
        kernel = self.rt.get_param(lay.name + '/kernel')
        cout, k, dil, hh, ww = tout.channels, node.attrs['k'], node.attrs['dil'], src.h, src.w
        if cout % 16 or src.c != rup(kernel.shape[2], 16):
            raise NotImplementedError(f'{lay.name}: unsupported channel counts for the fp8 path')
        if src.q is None:
            return self._cba_behind_bf16_bands(node, src, kernel)
        if k == 3 and dil > 1 and dil >= hh and dil >= ww:
            # every off-centre tap reads only zero padding (ASPP's dilation 6 / 12 on small maps): the 1x1 conv of the centre tap
            kernel, k, dil = kernel[1:2, 1:2], 1, 1
        b16 = self._hi(hh, ww)                             # this map's storage: bf16 (no quantisation, scale 1) or e4m3
        if b16 != src.b16:
            raise NotImplementedError(f'{lay.name}: input and output of a conv block live on different sides of the bf16 / fp8 boundary')
        thin = (THIN_FP8 and not b16 and k == 3 and dil == 1 and src.c in (32, 64) and cout in (32, 64) and hh % 8 == 0 and ww % 32 == 0)
        if src.dual is not None and not b16 and not thin:
            raise NotImplementedError(f'{lay.name}: a two-source fp8 conv outside the thin-layer kernel')
        # (dilated convs: plain e4m3 -- the tap-loop tile has no block-scaled form)
        base, qo = self._folded_conv(node, src, kernel, k, dil, b16, thin or dil > 1)
        ydt = B16 if b16 else None
        if tw is None:
            launches, must_fuse = [_Launch(0, self.n, self._z(self.n, hh, ww, cout, dtype=ydt), 0, cout)], False
        else:
            launches, must_fuse = self._dest_two_date(node, src, k, dil, b16)
        pooled = self._launch_conv(node, tw, base, src, launches, must_fuse, b16)
        self._put(tout, tw, _Stored(launches[0].y if launches[0].ldy == cout else None, cout, hh, ww, qo))
        if pooled is not None:
            pooled = _Stored(pooled, cout, pooled.shape[1], pooled.shape[2], qo)
            if b16 and not self._hi(pooled.h, pooled.w):
                pooled = self._to_fp8_level(pooled, self._qof(tout.id))
            self.prepooled[tout.id] = pooled
            if tw is not None:
                self.prepooled[tw] = pooled

    def _folded_conv(self, node, src, kernel, k, dil, b16, plain_e4m3):
        """(descriptor fields every launch of the conv block shares, scale of its output): packed weights, the folded epilogue vectors,
        the second source of a two-source read"""
        lay, cout = node.layer, node.outputs[0].channels
        w8, wscale, cdt = self._pack(kernel, src.c, False, b16, plain_e4m3)
        s, t_ = self._bn(lay.bn_name)
        qo = 1.0 if b16 else self._qof(node.outputs[0].id)
        oscale = self._f32(src.q * wscale * s / qo)
        obias = self._f32((s * self.rt.get_param(lay.name + '/bias') + t_) / qo)
        base = dict(c0=src.c, w=w8.data_ptr(), bias=obias.data_ptr(), out_scale=oscale.data_ptr(), h=src.h, w_=src.w, cout=cout,
                    cout_pad=rup(cout, 32), kh=k, kw=k, dil=dil, dtype=cdt)
        if src.dual is not None:
            d = src.dual
            base.update(c0=d.c0, x1=d.x1.data_ptr(), c1=d.c1, in_scale=d.in_scale.data_ptr(), in_shift=d.in_shift.data_ptr(), in_relu=1)
        return base, qo

    def _dest_two_date(self, node, src, k, dil, b16):
        """(launches, whether a max-pool must fuse) of a shared layer: one launch over 2n images into its own tensor or its channel slice
        of an ASPP slot tensor; into concat([x_b, x_a]) one launch with the pair store, or one per date"""
        n, date, tout = self.n, self.date, node.outputs[0]
        cout, hh, ww, ydt = tout.channels, src.h, src.w, B16 if b16 else None
        cons = self.consumers.get(tout.id, [])
        catn = [cn for cn in cons if cn.op == 'concat']
        pooln = [cn for cn in cons if cn.op == 'pool']
        if len(catn) + len(pooln) != len(cons) or len(catn) > 1 or len(pooln) > 1:
            raise NotImplementedError(f'{node.layer.name}: consumers of a shared layer not lowered')
        if not catn:
            return [_Launch(0, 2 * n, self._z(2 * n, hh, ww, cout, dtype=ydt), 0, cout)], False
        cat = catn[0]
        ctot = cat.outputs[0].channels
        offs, o = {}, 0                                    # tensor id -> channel offset in the concatenation
        for t in cat.inputs:
            offs[t.id] = o
            o += t.channels
        if len({date.get(t.id) for t in cat.inputs}) == 2:
            # the channel concatenation of the two dates, (n, hh, ww, ctot): date d's half at the channel offset of its tensor
            if id(cat) not in self.catbuf:
                self.catbuf[id(cat)] = self._z(n, hh, ww, ctot, dtype=ydt)
            y, off = self.catbuf[id(cat)], {date[t.id]: offs[t.id] for t in cat.inputs}
            if self.plan.pair and not self._tr_serves(b16, k, dil, src.c, cout, ww):
                return [_Launch(0, 2 * n, y, 0, ctot, (n, off[0], off[1]))], True
            return [_Launch(d * n, n, y, off[d], ctot) for d in (0, 1)], True
        # a branch of a slot concatenation (ASPP): its channel slice of one 2n-image tensor for the slot concatenations of both dates
        if id(cat) not in self.catbuf:
            tcat = self.twin[cat.outputs[0].id]
            buf = self._z(2 * n, hh, ww, ctot, dtype=ydt)
            for nd in self.m.nodes:
                if nd is cat or (nd.op == 'concat' and nd.outputs[0].id == tcat):
                    self.catbuf[id(nd)] = buf
        return [_Launch(0, 2 * n, self.catbuf[id(cat)], offs[tout.id], ctot)], False

    def _launch_conv(self, node, tw, base, src, launches, must_fuse, b16):
        """The launches of one conv block, with the block's MaxPooling2D in their epilogue where the pipelined kernel takes the shape.
        Returns the pooled tensor, or None where the pool node has to run on its own."""
        cout, hh, ww, esz = base['cout'], src.h, src.w, 2 if b16 else 1
        pools = [cn for cn in self.consumers.get(node.outputs[0].id, []) if cn.op == 'pool']
        f = pools[0].attrs['f'] if pools else 1
        if tw is not None and pools:
            self._divisible(hh, ww, f)                     # (single-date: left to the pool node, which may never be reached)
        want = len(pools) == 1 and hh % f == 0 and ww % f == 0
        ph, pw = hh // f, ww // f
        p = self._z(sum(L.n for L in launches), ph, pw, cout, dtype=B16 if b16 else None) if want and FUSE_POOL else None
        for L in launches:
            kw = dict(base, x0=src.t.data_ptr() + L.img0 * hh * ww * src.c * src.t.element_size(), n=L.n, y=L.y.data_ptr() + L.choff * esz,
                      ldy=L.ldy, pair=L.pair)
            pool_kw = dict(pool_y=p.data_ptr() + L.img0 * ph * pw * cout * esz, pool_ld=cout, pool_f=f) if p is not None else {}
            if pool_kw and not self._pool_fuses(kw, pool_kw):
                pool_kw, p = {}, None
            if want and p is None and must_fuse:
                raise NotImplementedError(f'{node.layer.name}: the max-pool of a shared encoder level does not fuse into its conv')
            self._conv(**kw, **pool_kw)
        return p

    def _cba_behind_bf16_bands(self, node, src, kernel):
        """first conv block of a graph whose tensors are all e4m3 but the input bands: bf16 conv (raw output), then BN + ReLU +
        quantisation in one pass"""
        n, hh, ww, lay, tout = self.n, src.h, src.w, node.layer, node.outputs[0]
        cout = tout.channels
        wb, _, _ = self._pack(kernel, src.c, False, b16=True)
        yb = self._z(n, hh, ww, cout, dtype=B16)
        self._conv(dtype=BF16, out_relu=0, x0=src.t.data_ptr(), c0=src.c, w=wb.data_ptr(), bias=self.rt.pptr(lay.name + '/bias'), y=yb.data_ptr(),
                   ldy=cout, n=n, h=hh, w_=ww, cout=cout, cout_pad=rup(cout, 32), kh=node.attrs['k'], kw=node.attrs['k'], dil=node.attrs['dil'])
        s, t_ = self._bn(lay.bn_name)
        qo = self._qof(tout.id)
        y8 = self._z(n, hh, ww, cout)
        self._requant(yb, cout, n * hh * ww, self._f32(s / qo), self._f32(t_ / qo), 1, BF16, FP8, y8)
        self.vals[tout.id] = _Stored(y8, cout, hh, ww, qo)

    def pool(self, node, tw):
        tin, tout = node.inputs[0], node.outputs[0]
        if tin.id in self.prepooled:                       # already produced by the conv's epilogue
            return self._put(tout, tw, self.prepooled[tin.id])
        v = self._whole(self.vals[tin.id])
        if v.t is None:
            raise NotImplementedError('folded inference: a shared encoder level whose max-pool did not fuse into the pair store')
        f, imgs = node.attrs['f'], v.t.shape[0]
        self._divisible(v.h, v.w, f)
        x, c, hh, ww, dt_ = v.t, v.c, v.h, v.w, BF16 if v.b16 else self.store
        p = self._z(imgs, hh // f, ww // f, c, dtype=B16 if v.b16 else None)
        self.fwd.append(lambda st: check(lib.satcv_maxpool(x.data_ptr(), p.data_ptr(), imgs, hh, ww, c, f, f, 0, dt_, st)))
        pooled = _Stored(p, c, hh // f, ww // f, v.q)
        if v.b16 and not self._hi(pooled.h, pooled.w):
            pooled = self._to_fp8_level(pooled, self._qof(tin.id))
        self._put(tout, tw, pooled)

    def dropout(self, node, tw):
        self._put(node.outputs[0], tw, self.vals[node.inputs[0].id])          # identity at inference

    def concat(self, node, tw):
        """single-date: concat([x_b, x_a]) of the two dates; two-date: an ASPP slot tensor.  Either was written by its producers' stores."""
        tout = node.outputs[0]
        if tw is None and id(node) not in self.catbuf:
            raise NotImplementedError('folded inference: a concatenation that is not the pair store of a shared layer')
        buf, first = self.catbuf[id(node)], self.vals[node.inputs[0].id]
        self._put(tout, tw, _Stored(buf, tout.channels, first.h, first.w, 1.0 if buf.dtype == B16 else self._qof(tout.id)))      # (bf16 tensors: scale 1)

    def convT(self, node, tw):
        n, rt = self.n, self.rt
        tin, tout = node.inputs[0], node.outputs[0]
        cons = self.consumers.get(tout.id, [])
        if len(cons) != 1 or cons[0].op != 'concat_bn_relu' or cons[0].inputs[1] is not tout:
            raise NotImplementedError('fp8 inference: a transposed conv must feed concat([skip, up]) -> BN -> ReLU')
        cat = cons[0]
        v = self._whole(self.vals[tin.id])
        x8, cin_s, hh, ww, qin = v.t, v.c, v.h, v.w, v.q
        lay, f = node.layer, node.attrs['f']
        ca, cb = cat.inputs[0].channels, tout.channels
        if cb % 16 or ca % 16:
            raise NotImplementedError(f'{lay.name}: unsupported channel counts for the fp8 path')
        b16 = self._hi(hh * f, ww * f)                     # storage of the up-sampled map (and of the skip it is concatenated with)
        if b16 and x8.dtype != B16:
            # the decoder climbs from the fp8 levels to the bf16 ones: de-quantise this block's input (a quarter of its output)
            xb = self._z(n, hh, ww, cin_s, dtype=B16)
            self._rescale(v, qin, FP8, BF16, xb)
            x8, qin = xb, 1.0
        kernel = rt.get_param(lay.name + '/kernel')
        w8, wscale, cdt = self._pack(kernel, cin_s, True, b16)
        s0, t0 = self._bn(cat.layer.name)
        qc = 1.0 if b16 else self._qof(cat.outputs[0].id)
        oscale = self._f32(qin * wscale * s0[ca:] / qc)
        obias = self._f32((s0[ca:] * rt.get_param(lay.name + '/bias') + t0[ca:]) / qc)
        two_src = (THIN_FP8 and not b16 and ca + cb in (32, 64) and (hh * f) % 8 == 0 and (ww * f) % 32 == 0 and
                   all(cn.op == 'cba' and cn.attrs['k'] == 3 and cn.attrs['dil'] == 1 and cn.outputs[0].channels in (32, 64)
                       for cn in self.consumers.get(cat.outputs[0].id, [])))
        if b16 or two_src:
            # the concatenation is not materialised -- the up-sampled half goes to its own tensor and the consumer conv reads
            # (skip, up) as two sources, with the skip half's BN + ReLU (and, in fp8, its requantisation to the concatenation's
            # scale) applied in its loader
            dst, ldy = self._z(n, hh * f, ww * f, cb, dtype=B16 if b16 else None), cb
            yptr = dst.data_ptr()
        else:
            dst, ldy = self._z(n, hh * f, ww * f, ca + cb), ca + cb
            yptr = dst.data_ptr() + ca * self.esz
        self._conv(x0=x8.data_ptr(), c0=cin_s, w=w8.data_ptr(), bias=obias.data_ptr(), out_scale=oscale.data_ptr(),
                   y=yptr, ldy=ldy, n=n, h=hh, w_=ww, cout=f * f * cb, cout_pad=rup(f * f * cb, 32),
                   kh=1, kw=1, dil=1, mode_out=1, f=f, cstat=cb, dtype=cdt)
        self.cats[id(cat)] = _Cat(dst, ca, cb, qc, s0, t0, hh * f, ww * f, b16, b16 or two_src)

    def concat_bn_relu(self, node, tw):
        ta, tout = node.inputs[0], node.outputs[0]
        cat = self.cats[id(node)]
        ca, cb, qc, s0, t0 = cat.ca, cat.cb, cat.q, cat.scale, cat.shift
        a = self._whole(self.vals[ta.id])
        if a.c != ca or (a.h, a.w) != (cat.h, cat.w):
            raise ValueError(f'concatenation of a {a.h}x{a.w}x{a.c} skip with a {cat.h}x{cat.w} up-sampled map')
        if cat.split:
            if cat.b16 != a.b16:
                raise NotImplementedError('an up-sampled map concatenated with a skip of the other storage type')
            insc = self._f32(torch.cat([s0[:ca] * a.q / qc, torch.ones(cb, device=self.dev)]))
            insh = self._f32(torch.cat([t0[:ca] / qc, torch.zeros(cb, device=self.dev)]))      # identity on the (already activated) up half
            self.vals[tout.id] = _Stored(a.t, ca + cb, cat.h, cat.w, qc, _TwoSource(cat.dst, ca, cb, insc, insh))
            return
        # the skip half's BN + ReLU, re-quantised to the concatenation's scale, into channels [0, ca) of the materialised concatenation
        self._requant(a.t, ca, self.n * cat.h * cat.w, self._f32(s0[:ca] * a.q / qc), self._f32(t0[:ca] / qc), 1, self.store, self.store,
                      cat.dst, ca + cb)
        self.vals[tout.id] = _Stored(cat.dst, ca + cb, cat.h, cat.w, qc)

    def head(self, node, tw):
        n, rt = self.n, self.rt
        tin, tout = node.inputs[0], node.outputs[0]
        v = self._whole(self.vals[tin.id])
        lay, c, hh, ww = node.layer, v.c, v.h, v.w
        ncls = tout.channels
        act = {'softmax': 0, 'sigmoid': 1, 'linear': 2}[node.attrs['activation']]
        probs = self._z(n, hh, ww, ncls, dtype=torch.float32)
        classes = self._z(*((n, hh, ww) if act != 1 else (n, hh, ww, ncls)), dtype=torch.int32)
        sc = self._f32(torch.full((c,), v.q, device=self.dev))
        sh = self._f32(torch.zeros(c, device=self.dev))
        hd = ops.make_head_desc(x=v.t.data_ptr(), ldx=c, cin=c, w=rt.pptr(lay.name + '/kernel'), b=rt.pptr(lay.name + '/bias'),
                                ncls=ncls, activation=act, npix=n * hh * ww, dtype=BF16 if v.b16 else self.store,
                                in_scale=sc.data_ptr(), in_shift=sh.data_ptr(),
                                thresh=node.attrs.get('thresh', 0.5), probs=probs.data_ptr(), classes=classes.data_ptr())
        self.keep.append(hd)
        self.fwd.append(lambda st: check(lib.satcv_head_fwd(C.byref(hd), st)))
        self.outputs[tout.id] = probs
        self.class_map = classes

    def classes(self, node, tw):
        self.outputs[node.outputs[0].id] = self.class_map
