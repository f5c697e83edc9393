"""FlatParams: the device state that both model families train on -- engine.Runtime (static U-Net plans) is one, lstm_tools._Params
(the ConvLSTM tape) is one, and training.apply_optimizer reads its attributes:
  pflat / gflat   flat fp32 parameters and gradients (every variable starts at a multiple of 4 floats)
  adam_state      [learning rate, step count, gradient scale, spare] of whichever optimizer is compiled
  lr_mul          per-element multiplier of the update (None: 1 everywhere; 0 freezes a variable)
  slot_kind/slots the optimizer's slots by name -- Adam is kind 'adam' with {'m', 'v'} -- allocated on the first step that needs them
  version         counts the changes of the parameters; whatever is derived from them (packed images, folded plans) compares it
  packed          registry of the MFMA operand images of the convolution kernels, repacked by ONE satcv_pack_weights_batched launch
WHEN the images are repacked is the subclass's policy (Runtime: at once, after every change; _Params: when next asked for)."""
import numpy as np
import torch

from . import ops
from ._lib import lib, check, PackJob


class FlatParams:
    def __init__(self):
        self.pflat = self.gflat = self.adam_state = self.lr_mul = None
        self.slot_kind, self.slots, self._clip_ws = None, {}, None
        self.version = 0
        self.packed, self._ptab, self.pack_dtype = {}, None, None

    def allocate(self, host, dev):
        """device buffers for the host image of the parameters; zero gradients, no slots, step 0"""
        self.pflat = torch.from_numpy(host).to(dev)
        self.gflat = torch.zeros_like(self.pflat)
        self.slot_kind, self.slots, self._clip_ws = None, {}, None
        self.adam_state = torch.tensor([1e-3, 0.0, 1.0, 0.0], dtype=torch.float32, device=dev)

    def bump(self):
        """the parameters changed (optimizer step, set_weights): whatever was derived from them is stale"""
        self.version += 1

    # ---- optimizer state
    def opt_slots(self, opt):
        """the slots of `opt` by name, zero-filled on first use; slots of another kind (or of another flag set) are dropped"""
        if self.slot_kind != opt.kind or set(self.slots) != set(opt.slot_names):
            self.slot_kind, self.slots = opt.kind, {k: torch.zeros_like(self.pflat) for k in opt.slot_names}
        return self.slots

    def clip_workspace(self):
        if self._clip_ws is None:
            self._clip_ws = ops.grad_clip_workspace(self.gflat.numel(), self.gflat.device)
        return self._clip_ws

    def reset_opt_slots(self):
        self.slot_kind, self.slots = None, {}
        self.adam_state[1:2].zero_()

    def optimizer_arrays(self):
        """(kind, {slot: array}, state) for a file; restore_optimizer takes them back"""
        return self.slot_kind, {k: v.cpu().numpy() for k, v in self.slots.items()}, self.adam_state.cpu().numpy()

    def restore_optimizer(self, kind, arrays, state):
        self.slot_kind = kind
        self.slots = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(self.pflat.device) for k, v in arrays.items()}
        self.adam_state.copy_(torch.from_numpy(np.asarray(state, np.float32)))

    # ---- packed operand images
    def register_image(self, key, src, fwd, dgrad, k, cin, cout, cin_pad, transposed=False, **more):
        """forward / data-gradient image buffers of the (kh, kw, cin, cout) kernel at device address `src` (of pflat); -> the entry"""
        self.packed[key] = e = dict(src=src, fwd=fwd, dgrad=dgrad, k=tuple(k), cin=cin, cout=cout, cin_pad=cin_pad, transposed=transposed, **more)
        self._ptab = None
        return e

    def pack_table(self):
        """device table of the pack jobs (forward + data-gradient image) of every registered kernel, built once per set of images"""
        if self._ptab is None:
            jobs = []
            for e in self.packed.values():
                taps, cin, cout, cp = e['k'][0] * e['k'][1], e['cin'], e['cout'], e['cin_pad']
                wide = taps * cout if e['transposed'] else cout          # a transposed convolution is a GEMM over taps x cout columns
                mode = 2 if e['transposed'] else 0
                jobs.append(PackJob(e['src'], e['fwd'].data_ptr(), mode, taps, cin, cout, cp, ops.rup(wide, 32)))
                jobs.append(PackJob(e['src'], e['dgrad'].data_ptr(), mode + 1, taps, cin, cout, ops.rup(wide, 16), ops.rup(cin, 32)))
            self._ptab = ops.job_table(jobs, lib.satcv_pack_job_items, self.pflat.device)
        return self._ptab

    def repack(self):
        """fp32 Keras-layout kernels -> MFMA operand images, one launch for all registered kernels"""
        if not self.packed:
            return
        t = self.pack_table()
        check(lib.satcv_pack_weights_batched(t['jobs'].data_ptr(), t['prefix'].data_ptr(), t['n'], t['total'], self.pack_dtype, ops.stream_ptr()))
