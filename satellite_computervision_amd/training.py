"""The Keras-facing training surface shared by the two model families: losses as LossSpec, the optimizers and their one step
dispatch, metrics, History, the callbacks and the epoch loop of fit().  model_tools.Model (static engine plans) and
lstm_tools._SeqModelBase (eager tape) differ in how an epoch is trained and validated; everything around that is here, once.
This module knows neither executor: it imports no model_tools, lstm_tools or engine; the optimizer step works on a params.FlatParams."""
import json
import os
import time
from collections import defaultdict

import numpy as np
import torch

from . import ops
from ._lib import lib, check


# ---------------------------------------------------------------------------- losses
class LossSpec:
    def __init__(self, kind, weights=None, eps=1e-6):
        self.kind, self.eps = kind, float(eps)
        self.weights = None if weights is None else np.asarray(weights, np.float32).reshape(-1)


class _LossArg:
    """placeholder handed to a user loss function so that it can describe itself"""

    def __init__(self, what):
        self.what = what


def _eager_loss(kind, y_true, y_pred, weights, activation='softmax', eps=1e-6):
    dev = torch.device('cuda')
    p = torch.as_tensor(np.asarray(y_pred, np.float32)).to(dev).contiguous()
    t = torch.as_tensor(np.asarray(y_true, np.float32)).to(dev).contiguous()
    w = None if weights is None else torch.as_tensor(np.asarray(weights, np.float32).reshape(-1)).to(dev)
    loss, _ = ops.loss_fwd_bwd(kind, p, t, w, activation, eps=eps)
    return float(loss.item())


def weighted_categorical_crossentropy(target, output, weights, axis=-1):
    """utils/model_tools.py:25-40 (reduced to its mean, as Keras does for a loss function)."""
    if isinstance(output, _LossArg):
        return LossSpec('weighted_categorical_crossentropy', weights)
    return _eager_loss('weighted_categorical_crossentropy', target, output, weights)


def weighted_bce(y_true, y_pred, pos_weight, logits=False):
    """utils/model_tools.py:96-112 (probability form; logits=True is not on the fused path)."""
    if logits:
        raise NotImplementedError('weighted_bce(logits=True): the model heads output probabilities')
    if isinstance(y_pred, _LossArg):
        return LossSpec('weighted_bce', [pos_weight])
    return _eager_loss('weighted_bce', y_true, y_pred, [pos_weight])


def gen_dice(y_true, y_pred, eps=1e-6, global_weights=None):
    """utils/model_tools.py:42-94: generalised Dice over (b, h*w, classes), mean over the batch.
    With global_weights=None the per-image class weights are 1/count^2 (eps where a class is absent) --
    the documented intent; the reference's own reduction axis (:80) does not broadcast."""
    if isinstance(y_pred, _LossArg):
        return LossSpec('gen_dice', global_weights if global_weights else None, eps)
    return _eager_loss('gen_dice', y_true, y_pred, global_weights if global_weights else None, eps=eps)


def iou_loss(true, pred):
    """utils/model_tools.py:131-140: 1 - sum(t*p) / sum(t + (1-t)*p) over the whole batch."""
    if isinstance(pred, _LossArg):
        return LossSpec('iou_loss')
    return _eager_loss('iou_loss', true, pred, None)


def mse_4d(y_true, y_pred, eps=1e-6):
    """utils/model_tools.py:142-166: mean squared error over the finite elements."""
    if isinstance(y_pred, _LossArg):
        return LossSpec('mse_4d')
    return _eager_loss('mse_4d', y_true, y_pred, None)


# ------------------------------------------------------------- optimizers / metrics
class _LR:
    def __init__(self, opt):
        self._opt = opt

    def numpy(self):
        return np.float32(self._opt._lr)

    def assign(self, v):
        self._opt._set_lr(float(v))

    def __float__(self):
        return float(self._opt._lr)


class _Optimizer:
    """what the Keras optimizers share: the `learning_rate` / `lr` property whose value lands in the device state buffer, and the
    base-class gradient clipping arguments `clipvalue` / `global_clipnorm` (at most one; the per-variable `clipnorm` is refused)."""
    kind = None
    slot_names = ()

    def _init_base(self, learning_rate, kwargs, strict=True):
        kwargs = dict(kwargs)
        if kwargs.pop('clipnorm', None) is not None:
            raise ValueError(f'{type(self).__name__}(clipnorm=...): per-variable norm clipping is not implemented; global_clipnorm= clips by the '
                             'norm of the whole gradient')
        self.clipvalue, self.global_clipnorm = kwargs.pop('clipvalue', None), kwargs.pop('global_clipnorm', None)
        if self.clipvalue is not None and self.global_clipnorm is not None:
            raise ValueError(f'{type(self).__name__}: at most one of clipvalue and global_clipnorm may be set')
        for name in ('clipvalue', 'global_clipnorm'):
            c = getattr(self, name)
            if c is not None and not float(c) > 0:
                raise ValueError(f'{type(self).__name__}({name}={c!r}): must be positive')
        self._lr = float(kwargs.pop('lr', learning_rate))
        if strict and kwargs:
            raise TypeError(f'{type(self).__name__}: unsupported arguments {sorted(kwargs)}')
        self._rt = None

    def _set_lr(self, v):
        self._lr = v
        if self._rt is not None:
            self._rt.adam_state[0:1].fill_(v)

    @property
    def learning_rate(self):
        return _LR(self)

    @learning_rate.setter
    def learning_rate(self, v):
        self._set_lr(float(v))

    lr = learning_rate


class Adam(_Optimizer):
    """tf.keras.optimizers.Adam: epsilon 1e-7 outside the bias correction."""
    kind = 'adam'
    slot_names = ('m', 'v')

    def __init__(self, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, **kwargs):
        self._init_base(learning_rate, kwargs, strict=False)
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon


class SGD(_Optimizer):
    """tf.keras.optimizers.SGD: v = momentum v - lr g, p += v (nesterov: p += momentum v - lr g); no slot without momentum."""
    kind = 'sgd'

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, **kwargs):
        self._init_base(learning_rate, kwargs)
        if not 0.0 <= float(momentum) <= 1.0:
            raise ValueError('`momentum` must be between [0, 1].')
        self.momentum, self.nesterov = float(momentum), bool(nesterov) and float(momentum) > 0     # (Keras: nesterov without momentum is plain SGD)
        self.slot_names = ('v',) if self.momentum > 0 else ()


class RMSprop(_Optimizer):
    """tf.keras.optimizers.RMSprop: epsilon inside the root (ApplyRMSProp / ApplyCenteredRMSProp); `mg` only when centered, `mom`
    only with momentum."""
    kind = 'rmsprop'

    def __init__(self, learning_rate=1e-3, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, **kwargs):
        self._init_base(learning_rate, kwargs)
        if not 0.0 <= float(momentum) <= 1.0:
            raise ValueError('`momentum` must be between [0, 1].')
        self.rho, self.momentum, self.epsilon, self.centered = float(rho), float(momentum), float(epsilon), bool(centered)
        self.slot_names = ('ms',) + (('mg',) if self.centered else ()) + (('mom',) if self.momentum > 0 else ())


_OPTIMIZERS = {'adam': Adam, 'sgd': SGD, 'rmsprop': RMSprop}


def resolve_optimizer(optimizer):
    """the `optimizer=` of compile(): 'adam' / 'sgd' / 'rmsprop' or an instance of Adam, SGD, RMSprop; anything else is refused"""
    if isinstance(optimizer, str):
        if optimizer.lower() not in _OPTIMIZERS:
            raise ValueError(f'unknown optimizer {optimizer!r}: one of {sorted(_OPTIMIZERS)}')
        return _OPTIMIZERS[optimizer.lower()]()
    if isinstance(optimizer, (Adam, SGD, RMSprop)):
        return optimizer
    raise TypeError(f'compile(optimizer={type(optimizer).__name__}): supported are model_tools.Adam, model_tools.SGD, model_tools.RMSprop '
                    "or the strings 'adam', 'sgd', 'rmsprop'")


def reset_slots_on_recompile(owner, prev, new):
    """Keras builds fresh slots for a newly compiled optimizer.  Here the moments of an Adam model have always survived a re-compile with
    another Adam; any other change of optimizer starts from zero slots and step 0."""
    if prev is not None and prev is not new and (prev.kind != new.kind or new.kind != 'adam'):
        owner.reset_opt_slots()


def apply_optimizer(opt, owner, st=None):
    """The one step dispatch of every training path (U-Net engine, ConvLSTM tape, hybrid, data parallel -- whose all-reduce has run by
    now): clip the flat gradient if the optimizer asks for it, then launch its update.  `owner` is the model's FlatParams
    (engine.Runtime or lstm_tools._Params).  A missing kernel is an error: there is no eager fallback."""
    p, g, state, lr_mul = owner.pflat, owner.gflat, owner.adam_state, owner.lr_mul
    st = ops.stream_ptr() if st is None else st
    if opt.clipvalue is not None:
        check(lib.satcv_grad_clip(g.data_ptr(), g.numel(), ops.CLIP_VALUE, float(opt.clipvalue), state.data_ptr(), None, st))
    elif opt.global_clipnorm is not None:
        check(lib.satcv_grad_clip(g.data_ptr(), g.numel(), ops.CLIP_GLOBAL_NORM, float(opt.global_clipnorm), state.data_ptr(),
                                  owner.clip_workspace().data_ptr(), st))
    lm = lr_mul.data_ptr() if lr_mul is not None else None
    sl = owner.opt_slots(opt)
    if opt.kind == 'adam':
        check(lib.satcv_adam_step(p.data_ptr(), g.data_ptr(), sl['m'].data_ptr(), sl['v'].data_ptr(), p.numel(), opt.beta_1, opt.beta_2, opt.epsilon,
                                  state.data_ptr(), lm, st))
    elif opt.kind == 'sgd':
        check(lib.satcv_sgd_step(p.data_ptr(), g.data_ptr(), sl['v'].data_ptr() if 'v' in sl else None, p.numel(), opt.momentum, int(opt.nesterov),
                                 state.data_ptr(), lm, st))
    elif opt.kind == 'rmsprop':
        check(lib.satcv_rmsprop_step(p.data_ptr(), g.data_ptr(), sl['ms'].data_ptr(), sl['mg'].data_ptr() if 'mg' in sl else None,
                                     sl['mom'].data_ptr() if 'mom' in sl else None, p.numel(), opt.rho, opt.momentum, opt.epsilon, state.data_ptr(), lm, st))
    else:
        raise TypeError(f'no update kernel for optimizer {type(opt).__name__}')


class MeanIoU:
    """tf.keras.metrics.MeanIoU(num_classes): mean over classes of TP/(TP+FP+FN), on class ids."""

    def __init__(self, num_classes, name='mean_io_u'):
        self.num_classes, self.name = num_classes, name


class History:
    def __init__(self):
        self.history = defaultdict(list)
        self.epoch = []


class ModelCheckpoint:
    """tf.keras.callbacks.ModelCheckpoint (nb:1228-1235); `.best` is mutable as retrain_model needs (:1168)."""

    def __init__(self, filepath, monitor='val_loss', verbose=0, save_best_only=False, save_weights_only=False, mode='auto', **kw):
        self.filepath, self.monitor, self.verbose = filepath, monitor, verbose
        self.save_best_only, self.save_weights_only = save_best_only, save_weights_only
        if mode == 'auto':
            mode = 'max' if ('acc' in monitor or 'io_u' in monitor or 'iou' in monitor) else 'min'
        self.mode = mode
        self.best = -np.inf if mode == 'max' else np.inf
        self.model = None

    def on_epoch_end(self, epoch, logs):
        cur = logs.get(self.monitor)
        path = self.filepath.format(epoch=epoch + 1, **logs)
        if self.save_best_only:
            if cur is None:
                return
            better = cur > self.best if self.mode == 'max' else cur < self.best
            if not better:
                return
            self.best = cur
        (self.model.save_weights if self.save_weights_only else self.model.save)(path)


def _auto_mode(mode, monitor):
    if mode not in ('auto', 'min', 'max'):
        raise ValueError(f"mode {mode!r}: one of 'auto', 'min', 'max'")
    if mode == 'auto':
        mode = 'max' if 'acc' in monitor else 'min'
    return mode


class LearningRateScheduler:
    """tf.keras.callbacks.LearningRateScheduler: at the start of every epoch the rate becomes schedule(epoch, lr) (or schedule(epoch)
    for a one-argument schedule), through `optimizer.learning_rate`; `lr` is added to the epoch logs."""

    def __init__(self, schedule, verbose=0):
        self.schedule, self.verbose = schedule, verbose
        self.model = None

    def on_epoch_begin(self, epoch, logs=None):
        opt = self.model.optimizer
        lr = float(opt.learning_rate)
        try:
            lr = self.schedule(epoch, lr)
        except TypeError:               # (old one-argument form, as Keras still accepts)
            lr = self.schedule(epoch)
        if not isinstance(lr, (float, np.float32, np.float64)):
            raise ValueError(f'The output of the "schedule" function should be float. Got: {lr}')
        opt.learning_rate = float(lr)
        if self.verbose:
            print(f'Epoch {epoch + 1}: LearningRateScheduler setting learning rate to {float(lr)}.')

    def on_epoch_end(self, epoch, logs):
        logs['lr'] = float(self.model.optimizer.learning_rate)


class ReduceLROnPlateau:
    """tf.keras.callbacks.ReduceLROnPlateau: after `patience` epochs without an improvement of `monitor` by more than `min_delta` the rate
    is multiplied by `factor` (not below `min_lr`), then `cooldown` epochs pass before the count starts again.  The rate goes through
    `optimizer.learning_rate`; `lr` (the rate the epoch ran with) is added to the epoch logs."""

    def __init__(self, monitor='val_loss', factor=0.1, patience=10, verbose=0, mode='auto', min_delta=1e-4, cooldown=0, min_lr=0, **kw):
        if kw:
            raise TypeError(f'ReduceLROnPlateau: unsupported arguments {sorted(kw)}')
        if factor >= 1.0:
            raise ValueError('ReduceLROnPlateau does not support a factor >= 1.0.')
        self.monitor, self.factor, self.patience, self.verbose = monitor, factor, patience, verbose
        self.min_delta, self.cooldown, self.min_lr = min_delta, cooldown, min_lr
        self.mode = _auto_mode(mode, monitor)
        self.model = None
        self._reset()

    def _reset(self):
        self.best = -np.inf if self.mode == 'max' else np.inf
        self.cooldown_counter, self.wait = 0, 0

    def _better(self, cur):
        return cur > self.best + self.min_delta if self.mode == 'max' else cur < self.best - self.min_delta

    def on_train_begin(self, logs=None):
        self._reset()

    def on_epoch_end(self, epoch, logs):
        opt = self.model.optimizer
        logs['lr'] = float(opt.learning_rate)
        cur = logs.get(self.monitor)
        if cur is None:
            import warnings
            warnings.warn(f'ReduceLROnPlateau: metric `{self.monitor}` is not available (have {sorted(logs)})')
            return
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.wait = 0
        if self._better(cur):
            self.best, self.wait = cur, 0
        elif self.cooldown_counter <= 0:
            self.wait += 1
            if self.wait >= self.patience:
                old = float(opt.learning_rate)
                if old > float(self.min_lr):
                    opt.learning_rate = max(old * self.factor, float(self.min_lr))
                    if self.verbose:
                        print(f'Epoch {epoch + 1}: ReduceLROnPlateau reducing learning rate to {float(opt.learning_rate)}.')
                    self.cooldown_counter, self.wait = self.cooldown, 0


def _snapshot_weights(model):
    snap = {'': model.get_weights_dict()}
    for tag, bm in getattr(model, '_branch_models', dict)().items():
        snap[tag] = bm.get_weights_dict()
    return snap


def _restore_weights(model, snap):
    model.set_weights_dict(snap[''])
    for tag, bm in getattr(model, '_branch_models', dict)().items():
        bm.set_weights_dict(snap[tag])


class EarlyStopping:
    """tf.keras.callbacks.EarlyStopping: sets `model.stop_training` after `patience` epochs in which `monitor` has not improved on its
    best value by more than `min_delta`; restore_best_weights puts the best epoch's variables (moving statistics included) back."""

    def __init__(self, monitor='val_loss', min_delta=0, patience=0, verbose=0, mode='auto', restore_best_weights=False, **kw):
        if kw:
            raise TypeError(f'EarlyStopping: unsupported arguments {sorted(kw)}')
        self.monitor, self.min_delta, self.patience, self.verbose = monitor, abs(min_delta), patience, verbose
        self.mode = _auto_mode(mode, monitor)
        self.restore_best_weights = restore_best_weights
        self.model = None
        self.on_train_begin()

    def on_train_begin(self, logs=None):
        self.wait, self.stopped_epoch, self.best_epoch = 0, 0, 0
        self.best = -np.inf if self.mode == 'max' else np.inf
        self.best_weights = None

    def _better(self, cur):
        return cur - self.min_delta > self.best if self.mode == 'max' else cur + self.min_delta < self.best

    def on_epoch_end(self, epoch, logs):
        cur = logs.get(self.monitor)
        if cur is None:
            import warnings
            warnings.warn(f'EarlyStopping: metric `{self.monitor}` is not available (have {sorted(logs)})')
            return
        if self._better(cur):
            self.best, self.best_epoch, self.wait = cur, epoch, 0
            if self.restore_best_weights:
                self.best_weights = _snapshot_weights(self.model)
            return
        self.wait += 1
        if self.wait >= self.patience:
            self.stopped_epoch = epoch
            self.model.stop_training = True
            if self.restore_best_weights and self.best_weights is not None:
                _restore_weights(self.model, self.best_weights)
            if self.verbose:
                print(f'Epoch {epoch + 1}: early stopping')


def run_callbacks(callbacks, hook, *args):
    """call `hook` on every callback that has it (the callbacks of this module define only the hooks they use)"""
    for cb in callbacks:
        fn = getattr(cb, hook, None)
        if fn is not None:
            fn(*args)


def record_callback_logs(hist, logs, before):
    """entries the callbacks added to the epoch logs (`lr`) join the history, as in Keras, where History runs last"""
    for k, v in logs.items():
        if k not in before:
            hist.history[k].append(v)


class TensorBoard:
    """tf.keras.callbacks.TensorBoard(log_dir): epoch scalars as real TensorBoard event files -- `<log_dir>/train` and
    `<log_dir>/validation`, tags `epoch_<name>` like Keras (notebooks/UNET_G4G_2019_solar.ipynb:1255) -- written without
    TensorFlow (tfrecord_io.EventFileWriter), plus one JSON line per epoch in `<log_dir>/scalars.jsonl`."""

    def __init__(self, log_dir='logs', **kw):
        self.log_dir = log_dir
        self.model = None
        self._writers = {}

    def _writer(self, which):
        from . import tfrecord_io
        if which not in self._writers:
            self._writers[which] = tfrecord_io.EventFileWriter(os.path.join(self.log_dir, which))
        return self._writers[which]

    def on_epoch_end(self, epoch, logs):
        os.makedirs(self.log_dir, exist_ok=True)
        with open(os.path.join(self.log_dir, 'scalars.jsonl'), 'a') as f:
            f.write(json.dumps(dict(epoch=epoch, **{k: float(v) for k, v in logs.items()})) + '\n')
        train = {f'epoch_{k}': float(v) for k, v in logs.items() if not k.startswith('val_')}
        val = {f'epoch_{k[4:]}': float(v) for k, v in logs.items() if k.startswith('val_')}
        if train:
            self._writer('train').scalars(epoch, train)
        if val:
            self._writer('validation').scalars(epoch, val)



# ------------------------------------------------------- what compile / fit / evaluate of both model families share
def resolve_loss(loss):
    """the `loss=` of compile(): one of this module's loss functions, a lambda wrapping one, or a LossSpec -> LossSpec; anything else is refused"""
    if callable(loss):
        spec = loss(_LossArg('y_true'), _LossArg('y_pred'))
    elif isinstance(loss, LossSpec):
        spec = loss
    else:
        raise ValueError('loss must be one of the model_tools loss functions (or a lambda wrapping one)')
    if not isinstance(spec, LossSpec):
        raise ValueError('loss function did not resolve to a fused device loss')
    return spec


def metric_from_confusion(kind, conf):
    """'accuracy' -> trace / sum; any other kind -> mean IoU over the classes that occur (as a label or as a prediction); 0.0 for an empty matrix"""
    conf = conf.astype(np.float64)
    if kind == 'accuracy':
        return float(np.trace(conf) / max(conf.sum(), 1))
    tp = np.diag(conf)
    denom = conf.sum(0) + conf.sum(1) - tp
    valid = denom > 0
    return float((tp[valid] / denom[valid]).mean()) if valid.any() else 0.0


def fit_loop(model, x, epochs, initial_epoch, callbacks, verbose, train_epoch, validate, show_time):
    """The epoch skeleton of fit() -> History.  train_epoch(epoch) trains one epoch and returns its logs; validate() returns the validation
    values under their plain names (None: no validation), which join the logs as `val_<name>`.  Callbacks see the logs in on_epoch_end and
    may add to them or set model.stop_training; x.on_epoch_end() (generators reshuffle there) runs after them."""
    hist = History()
    callbacks = list(callbacks or [])
    for cb in callbacks:
        cb.model = model
    model.stop_training = False
    run_callbacks(callbacks, 'on_train_begin')
    for epoch in range(initial_epoch, epochs):
        t0 = time.time()
        run_callbacks(callbacks, 'on_epoch_begin', epoch)
        logs = train_epoch(epoch)
        if validate is not None:
            logs.update({'val_' + k: v for k, v in validate().items()})
        for k, v in logs.items():
            hist.history[k].append(v)
        hist.epoch.append(epoch)
        if verbose:
            took = f'{time.time() - t0:.1f}s - ' if show_time else ''
            print(f'Epoch {epoch + 1}/{epochs} - {took}' + ' - '.join(f'{k}: {v:.4f}' for k, v in logs.items()))
        before = set(logs)
        run_callbacks(callbacks, 'on_epoch_end', epoch, logs)
        record_callback_logs(hist, logs, before)
        if hasattr(x, 'on_epoch_end'):
            x.on_epoch_end()
        if model.stop_training:
            break
    run_callbacks(callbacks, 'on_train_end')
    return hist
