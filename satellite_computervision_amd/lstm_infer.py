"""Inference plan of the ConvLSTM2D time-series models (lstm_tools.LSTMModel / LSTMAutoencoder): what fp8_infer.Fp8Plan is to the U-Net
family.  `predict_on_device` runs the training tape in eval mode -- per time step a recurrent `ops.conv2d` that writes hg (npix x 4 F)
to HBM and a `satcv_convlstm_gates_fwd` that reads it back, every tensor allocated by torch.  A SeriesInferPlan

  * owns every buffer of the forward pass for ONE input shape (xg, the h sequence, two c buffers, the head outputs, the class tensor),
  * holds the packed weights and the BatchNorm layers as inference scale / shift (ops.bn_affine_infer), applied by the consumer's input
    transform exactly as on the tape,
  * with fused=True runs a time step as ONE launch, satcv_convlstm_step_fwd (csrc/convlstm_step.hip), on gate-interleaved channels,
  * after one eager run is captured into a graph and replayed (SATCV_LSTM_GRAPH=0, the `lstm_graph` switch, keeps it eager).

Gate order.  The fused step needs the four pre-activations of a filter in one lane's accumulators, 32 MFMA columns apart; Keras puts them F
channels apart.  `gate_order(F)` is the permutation of the 4 F output channels applied ONCE, on the host side of the plan, to the recurrent
kernel, the input kernel and the bias before packing: xg, as the unchanged input convolution writes it, and the accumulators then share
one channel order.  c and h stay in natural order.

Numerics: with fused=False the plan issues the tape's launches and is bit-equal to predict_on_device.  The fused step in bf16 is NOT: the
pair of launches rounds hg to bf16 before the gates, the fused step keeps z = xg + conv(h) in fp32.
"""
import warnings

import numpy as np
import torch

from . import ops
from . import lstm_tools as lt
from ._lib import lib

STEP_FILTERS = (16, 32, 64)          # filter counts satcv_convlstm_step_fwd is built for


def gate_order(F, group=None):
    """Gate-interleaved order of the 4 F gate channels of a ConvLSTM2D (natural Keras order: i, f, c, o blocks of F): an int64 array
    `perm` of length 4 F with   perm[blk * 4 * group + gate * group + j] = gate * F + blk * group + j.   Permuted tensor = natural[..., perm];
    natural = permuted[..., np.argsort(perm)].  group defaults to min(F, 32), the order satcv_convlstm_step_fwd reads (include/satcv.h)."""
    F = int(F)
    g = min(F, 32) if group is None else int(group)
    if F <= 0 or g <= 0 or F % g:
        raise ValueError(f'gate_order: group {g} does not divide F = {F}')
    blk, gate, j = np.meshgrid(np.arange(F // g), np.arange(4), np.arange(g), indexing='ij')
    return (gate * F + blk * g + j).reshape(-1).astype(np.int64)


def step_supported(F, dtype_code):
    """whether the fused step kernel takes this filter count and storage type (asked of the library, once per layer at plan build)"""
    return bool(lib.satcv_convlstm_step_supported(int(F), int(dtype_code)))


_CAPTURE_STREAMS = {}


def _capture_stream():
    """ONE capture stream per device for every plan (the library has a bounded table of per-stream workspaces); replays run on the
    caller's current stream, in stream order, so plans sharing the workspaces captured here never overlap"""
    dev = torch.cuda.current_device()
    if dev not in _CAPTURE_STREAMS:
        _CAPTURE_STREAMS[dev] = torch.cuda.Stream(device=dev)
    return _CAPTURE_STREAMS[dev]


class _PlannedLayer:
    """one ConvLSTM2D of the plan: buffers, packed weights, and its launches"""

    def __init__(self, layer, T, B, H, W, dtype, fused):
        self.layer, self.T, self.B, self.dtype = layer, T, B, dtype
        F = self.F = layer.F
        td, dev = ops.TORCH_DTYPE[dtype], lt._dev()
        self.fused = bool(fused) and step_supported(F, dtype)                   # decided here, never by catching an error per step
        self.Fp = ops.rup(F, 16)
        self.xg = torch.empty(T * B, H, W, ops.rup(4 * F, 16), dtype=td, device=dev)
        self.hseq = torch.zeros(T * B, H, W, self.Fp, dtype=td, device=dev)      # (pad channels stay zero: the kernels write F of them)
        self.c = [torch.empty(B * H * W, F, dtype=torch.float32, device=dev) for _ in range(2)]
        self.hg = None if self.fused else torch.empty(B, H, W, ops.rup(4 * F, 16), dtype=td, device=dev)
        ek, _, _, _ = ops.packed_sizes(3, 3, layer.cin, 4 * F, ops.rup(layer.cin, 16), False)
        er, _, _, _ = ops.packed_sizes(3, 3, F, 4 * F, ops.rup(F, 16), False)
        self.wk = torch.empty(ek, dtype=td, device=dev)
        self.wr = torch.empty(er, dtype=td, device=dev)
        self.bias = torch.empty(4 * F, dtype=torch.float32, device=dev)
        self.perm = torch.from_numpy(gate_order(F)).to(dev) if self.fused else None

    def refresh(self):
        """(re)pack the kernels and the bias from the model's parameters -- permuted to the gate-interleaved order for the fused step"""
        L, P = self.layer, self.layer.P
        k, r, b = P.p(f'{L.name}/kernel'), P.p(f'{L.name}/recurrent_kernel'), P.p(f'{L.name}/bias')
        if self.perm is not None:
            k, r, b = k.index_select(3, self.perm), r.index_select(3, self.perm), b.index_select(0, self.perm)
        ops.pack_weights(k, ops.rup(L.cin, 16), self.dtype, want_dgrad=False, out_fwd=self.wk)
        ops.pack_weights(r, ops.rup(self.F, 16), self.dtype, want_dgrad=False, out_fwd=self.wr)
        self.bias.copy_(b)

    def launch(self, x):
        """x: lstm_tools.Act, time-major (T * B, H, W, Cpad).  -> Act of the raw output: lstm_tools.convlstm_forward, the tape's routine,
        on the plan's buffers and images, the c of step t in slot t & 1"""
        out, self.h_last = lt.convlstm_forward(self.layer, x, self.T, self.B, self.wk, self.wr, self.bias, self.xg, self.hseq,
                                               lambda t: self.c[t & 1], hg=self.hg, fused=self.fused)
        return out


class _PlannedBN:
    """a BatchNormalization as inference scale / shift over the padded channel count, in buffers the captured graph reads"""

    def __init__(self, bn, cp):
        self.bn, self.cp = bn, cp
        self.scale = torch.empty(cp, dtype=torch.float32, device=lt._dev())
        self.shift = torch.empty(cp, dtype=torch.float32, device=lt._dev())

    def refresh(self):
        sc, sh = lt.bn_affine_infer(self.bn, self.cp)
        self.scale.copy_(sc); self.shift.copy_(sh)

    def apply(self, a, relu=True):
        return lt.Act(a.t, a.c, (self.scale, self.shift, None, None), relu)


def _stage_prefix(dst, src, lead, B, what):
    """copy an input into its static tensor `dst` ((lead * B, ...)); `src` may hold fewer chips than the plan (a short last batch): they
    fill a prefix of every one of the `lead` time steps, the stale rest is computed and ignored (inference BatchNorm uses moving
    statistics: chips are independent).  -> the number of chips staged"""
    if src.dtype != dst.dtype or not src.is_cuda or src.dim() != dst.dim() or tuple(src.shape[1:]) != tuple(dst.shape[1:]) or not src.is_contiguous():
        raise ValueError(f'{what}: expected a contiguous {dst.dtype} CUDA tensor {tuple(dst.shape)}, got {src.dtype} {tuple(src.shape)}')
    if src.shape[0] == dst.shape[0]:
        if src.data_ptr() != dst.data_ptr():
            dst.copy_(src, non_blocking=True)
        return B
    n = src.shape[0] // lead
    if n * lead != src.shape[0] or not 0 < n < B:
        raise ValueError(f'{what}: {src.shape[0]} images do not make {lead} steps of at most {B} chips')
    dst.view(lead, B, *dst.shape[1:])[:, :n].copy_(src.view(lead, n, *src.shape[1:]), non_blocking=True)
    return n


class _ConvLstmPlan:
    """What SeriesInferPlan and HybridInferPlan share -- the ConvLSTM branch of `model` (its layers in `stack`) for B chips of H x W pixels:
    the static input x_in (T * B, H, W, cpad), both ConvLSTM2D layers and their BatchNorms as planned launches on preallocated buffers,
    the repack of parameters that changed, and the capture of the subclass's launch list (`_launch`) into a graph."""

    def __init__(self, model, stack, B, H, W, fused):
        self.model, self.dtype = model, model.dtype_code
        T = self.T = model.n_time
        self.cpad = ops.rup(model.n_channels, 16)
        self.x_in = torch.zeros(T * B, H, W, self.cpad, dtype=ops.TORCH_DTYPE[self.dtype], device=lt._dev())
        self.l1 = _PlannedLayer(stack.l1, T, B, H, W, self.dtype, fused)
        self.bn1 = _PlannedBN(stack.bn1, self.l1.Fp)
        self.l2 = _PlannedLayer(stack.l2, T, B, H, W, self.dtype, fused)
        self.bn2 = _PlannedBN(stack.bn2, self.l2.Fp)
        self.fused_layers = tuple(n for n, l in (('conv_lstm', self.l1), ('dilated_conv_lstm', self.l2)) if l.fused)
        self._ver = None
        self._runs, self._graph, self._graph_off = 0, None, False

    def _check_dtype(self):
        if self.model.dtype_code != self.dtype:
            raise ValueError('the model\'s compute_dtype changed since this plan was built; build a new plan')

    def _refresh(self):
        """parameters changed since the last run (set_weights, training) are repacked, into the same buffers"""
        if self._ver != self.model.P.version:
            for p in (self.l1, self.bn1, self.l2, self.bn2):
                p.refresh()
            self._ver = self.model.P.version

    def _launch_lstm(self):
        """the head of both launch lists: conv_lstm -> batch_norm -> dilated_conv_lstm; -> Act of the second layer's raw output"""
        s1 = self.l1.launch(lt.Act(self.x_in, self.model.n_channels))
        a1 = self.bn1.apply(s1)                                             # (Dropout passes through at inference)
        return self.l2.launch(a1)

    def _run_captured(self):
        """One run of `self._launch`: the first run is eager, the second captures the launch list into a graph, later runs replay it on
        the current stream."""
        self._runs += 1
        if self._graph is None and self._runs > 1 and not self._graph_off and lt.graph_enabled():
            try:
                # The launch list runs once, eagerly, ON THE CAPTURE STREAM first: the library keeps per-stream workspaces (split-K slabs)
                # that it never allocates inside a capture, and a convolution that finds none takes another kernel form -- the replay
                # would differ from the eager run in the last bits.  Then the same list is captured there, one linear chain.
                g, cap, cur = torch.cuda.CUDAGraph(), _capture_stream(), torch.cuda.current_stream()
                cap.wait_stream(cur)
                with torch.cuda.stream(cap):
                    self._launch()
                cur.wait_stream(cap)
                torch.cuda.synchronize()
                with torch.cuda.graph(g, stream=cap):
                    self._launch()
                self._graph = g
            except Exception as e:           # a forward that cannot be captured stays eager (and says so once)
                warnings.warn(f'{type(self).__name__}: forward not captured ({e}); running eagerly')
                self._graph_off = True
        if self._graph is not None and lt.graph_enabled():
            self._graph.replay()
        else:
            self._launch()

    @property
    def replaying(self):
        """whether the next run replays a captured graph"""
        return self._graph is not None and bool(lt.graph_enabled())


class SeriesInferPlan(_ConvLstmPlan):
    """SeriesInferPlan(model, shape=(B, T, H, W), fused=...) for an LSTMModel or an LSTMAutoencoder, in the model's storage type at the time
    it is built.  `run(xt, want_classes=False)` takes what `predict_on_device(..., shape=shape)` takes -- the ingested time-major tensor
    (T * B, H, W, cpad); for the autoencoder the pair [xt, sincos] -- and returns what it returns.

    THE RETURNED TENSORS ARE THE PLAN'S OWN: they are valid until the next `run` of this plan; clone what must outlive it.

    fused=False: the tape's launches (ops.conv2d + satcv_convlstm_gates_fwd, natural channel order) on preallocated buffers, bit-equal to
    predict_on_device.  fused=True: satcv_convlstm_step_fwd per time step; a layer whose filter count or storage type that kernel was not
    built for keeps the pair (decided here, at build: `fused_layers`).  The first run is eager, the second captures the forward into one
    graph (one stream, a linear chain, after an eager run on that stream) and later runs replay it; a capture that fails stays eager and warns once.  Parameters changed
    after the plan was built (set_weights, training) are repacked at the next run, into the same buffers."""

    def __init__(self, model, shape, fused=False):
        if not isinstance(model, (lt.LSTMModel, lt.LSTMAutoencoder)):
            raise NotImplementedError(f'SeriesInferPlan covers LSTMModel and LSTMAutoencoder; {type(model).__name__} (two inputs at two resolutions, '
                                      f'a U-Net / ACNN branch) runs through its own predict')
        B, T, H, W = (int(v) for v in shape)
        if T != model.n_time:
            raise ValueError(f'model was built for {model.n_time} time steps, got {T}')
        if min(B, H, W) < 1:
            raise ValueError(f'bad plan shape {shape}')
        self.shape = (B, T, H, W)
        self.is_ae = isinstance(model, lt.LSTMAutoencoder)
        super().__init__(model, model.enc if self.is_ae else model.layers_, B, H, W, fused)
        td, dev = ops.TORCH_DTYPE[self.dtype], lt._dev()
        self.head = model.single if self.is_ae else model.dense
        self.out = torch.empty(B, H, W, self.head.cout, dtype=torch.float32, device=dev)
        self.classes = torch.empty(B, H, W, dtype=torch.int32, device=dev) if (not self.is_ae and model.class_output) else None
        if self.is_ae:
            self.sc_in = torch.zeros(B, H, W, 2, dtype=torch.float32, device=dev)
            self.enc_out = torch.empty(B, H, W, self.l1.Fp, dtype=td, device=dev)

    # ------------------------------------------------------------------ the launch list (the structure of _forward_ingested, inference)
    def _launch(self):
        h2 = self._launch_lstm()
        if not self.is_ae:
            srcs = [(self.bn2.apply(h2), False)]
        else:
            # build_lstm_layers2: ReLU(state_h + BatchNorm(h2)), state_h the first layer's last hidden state; the decoder branch
            # (`temporal`) is left out, as in LSTMAutoencoder.predict_on_device
            lt.lstm_layers2_tail(self.bn2.apply(h2, relu=False), self.l1.h_last, self.enc_out)
            srcs = [(lt.Act(self.enc_out, self.l1.F), False), (lt.Act(self.sc_in, 2), False)]
        self.head.forward(srcs, out=self.out, classes=self.classes)

    # ------------------------------------------------------------------ run
    def _stage(self, dst, src, lead, what):
        """copy an input into its static tensor; a short last batch fills a prefix of every time step (_stage_prefix)"""
        return _stage_prefix(dst, src, lead, self.shape[0], what)

    def run(self, xt, want_classes=False):
        """-> (B, H, W, n_classes) float32 (with want_classes also the (B, H, W) int32 class tensor of a softmax head); the autoencoder takes
        [xt, sincos] and returns its `single` output.  An input of n < B chips ((T * n, ...), and (n, ...) harmonics) runs as a prefix: the
        first n chips of the result are its prediction.  The tensors returned belong to the plan and are overwritten by its next run."""
        if want_classes and self.classes is None:
            raise ValueError("want_classes needs a model with activation='softmax'")
        self._check_dtype()
        T = self.T
        if self.is_ae:
            xt, sincos = xt
            n = self._stage(self.x_in, xt, T, 'xt')
            if self._stage(self.sc_in, sincos, 1, 'sincos') != n:
                raise ValueError('xt and sincos hold different numbers of chips')
        else:
            self._stage(self.x_in, xt, T, 'xt')
        self._refresh()
        self._run_captured()
        return (self.out, self.classes) if want_classes else self.out


class HybridInferPlan(_ConvLstmPlan):
    """HybridInferPlan(model, batch, side, side_lo, fused=False): the inference plan of a lstm_tools.HybridModel for scene prediction
    (prediction_tools.predict_hybrid_scene), in the model's storage type at the time it is built; also HybridModel.scene_plan(...).

    The ConvLSTM branch is the base class's, as for SeriesInferPlan: the static input x_in (T * batch, side_lo, side_lo, cpad) and both
    ConvLSTM2D layers and BatchNorms as planned launches on preallocated buffers.  The plan's own tail is the `lstm_dense` launch into a
    static (batch, side_lo, side_lo, k) tensor.  That chain, and only that chain, is captured into a graph after one eager run and replayed
    (SATCV_LSTM_GRAPH=0 keeps it eager; a capture that fails warns once and stays eager).  The U-Net branch (the engine's static plan for
    the n chips of the batch) and the fusion head are launched eagerly on the current stream around the replay: the head's `first`
    changes with every batch, so it cannot live in the graph.  fused=True runs a time step as satcv_convlstm_step_fwd where that kernel
    was built for the layer (`fused_layers`); fused=False issues the tape's launches and is bit-equal to predict_on_device.
    Parameters changed after the plan was built are repacked at the next run, into the same buffers.

    NOTHING `run` RETURNS OUTLIVES THE NEXT RUN of this plan: the tensors are the plan's own."""

    def __init__(self, model, batch, side, side_lo, fused=False):
        if not isinstance(model, lt.HybridModel):
            raise NotImplementedError(f'HybridInferPlan covers HybridModel; {type(model).__name__} has no plan of this kind')
        B, S, SL = int(batch), int(side), int(side_lo)
        if min(B, S, SL) < 1:
            raise ValueError(f'bad plan sizes batch={batch}, side={side}, side_lo={side_lo}')
        self.shape = (B, S, SL)
        super().__init__(model, model.lstm, B, SL, SL, fused)
        self.zl = torch.empty(B, SL, SL, model.n_classes, dtype=torch.float32, device=lt._dev())
        self.out = self.classes = None                                      # (allocated by the first run without scene_head)

    def _launch(self):
        """the captured chain: conv_lstm -> batch_norm -> dilated_conv_lstm -> batch_norm2 -> lstm_dense (ReLU), into self.zl"""
        self.model.lstm_dense.forward([(self.bn2.apply(self._launch_lstm()), False)], out=self.zl)

    def run(self, xu, xt, scene_head=None, want_classes=False):
        """xu: (n, side, side, C) float32 CUDA tensor, xt: the ingested time-major tensor (T * n, side_lo, side_lo, cpad), n <= batch (a
        short last batch fills a prefix of every time step of x_in; the U-Net branch and the head run on the n chips).
        scene_head=<callable>: receives the descriptor of the `probabilities` layer (as HybridModel.predict_on_device passes it) and its
        result is returned; without it -> (n, side, side, n_classes) float32 probabilities, with want_classes also the int32 classes.
        Everything returned, and everything the descriptor points to, belongs to the plan and is overwritten by its next run."""
        m, (B, S, SL) = self.model, self.shape
        self._check_dtype()
        if not (m._is_fine_batch(xu) and tuple(xu.shape[1:3]) == (S, S)):
            raise ValueError(f'xu: expected an (n, {S}, {S}, {m.hi_channels}) float32 CUDA tensor, got {getattr(xu, "dtype", None)} {tuple(getattr(xu, "shape", ()))}')
        n = _stage_prefix(self.x_in, xt, self.T, B, 'xt')
        if xu.shape[0] != n:
            raise ValueError(f'xu and xt hold different numbers of chips: {xu.shape[0]} and {n}')
        self._refresh()
        _, zu = m._unet_branch(xu, False)
        self._run_captured()
        if scene_head is None and self.out is None:
            self.out = torch.empty(B, S, S, m.n_classes, dtype=torch.float32, device=self.zl.device)
            self.classes = torch.empty(B, S, S, dtype=torch.int32, device=self.zl.device)
        res = m._fuse(self.zl[:n], zu, scene_head, out=self.out, classes=self.classes)
        if scene_head is not None:
            return res
        return (self.out[:n], self.classes[:n]) if want_classes else self.out[:n]
