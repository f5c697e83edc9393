"""NumPy float64 restatements of the optimizer family: the three update rules (tf.keras.optimizers.SGD / RMSprop / Adam), the two
gradient-clipping modes of the Keras optimizer base class (`clipvalue`, `global_clipnorm`) and the epoch-level decision logic of
tf.keras.callbacks.LearningRateScheduler / ReduceLROnPlateau / EarlyStopping.

Like all Keras arithmetic in this repository these are UNPINNED restatements: TensorFlow cannot be imported here, so nothing below has
been compared with a running Keras.  They follow the formulas TensorFlow documents (ApplyGradientDescent / ApplyKerasMomentum,
ApplyRMSProp / ApplyCenteredRMSProp with epsilon inside the root, Adam with epsilon outside the bias correction as
oracle/unet.py states it, tf.clip_by_value, tf.clip_by_global_norm).  tests/test_optimizers_cpu.py pins what can be pinned without
TensorFlow: SGD and the global-norm clip against PyTorch on the CPU."""
import numpy as np


# ------------------------------------------------------------------ update rules.  `slots` is a dict the rule creates and updates.
def sgd_step(p, g, slots, lr, momentum=0.0, nesterov=False):
    g = np.asarray(g, np.float64)
    if momentum == 0.0:
        return p - lr * g
    v = momentum * slots.get('v', np.zeros_like(p)) - lr * g
    slots['v'] = v
    return p + (momentum * v - lr * g if nesterov else v)


def rmsprop_step(p, g, slots, lr, rho=0.9, momentum=0.0, eps=1e-7, centered=False):
    g = np.asarray(g, np.float64)
    ms = rho * slots.get('ms', np.zeros_like(p)) + (1 - rho) * g * g
    slots['ms'] = ms
    var = ms
    if centered:
        mg = rho * slots.get('mg', np.zeros_like(p)) + (1 - rho) * g
        slots['mg'] = mg
        var = ms - mg * mg
    upd = lr * g / np.sqrt(var + eps)
    if momentum > 0.0:
        upd = momentum * slots.get('mom', np.zeros_like(p)) + upd
        slots['mom'] = upd
    return p - upd


def adam_step(p, g, slots, lr, beta1=0.9, beta2=0.999, eps=1e-7):
    """as oracle/unet.py UNetOracle.adam_step and tests/test_ops_gpu.py::test_adam_keras_formulation state it"""
    g = np.asarray(g, np.float64)
    t = slots['t'] = slots.get('t', 0) + 1
    m = slots['m'] = beta1 * slots.get('m', np.zeros_like(p)) + (1 - beta1) * g
    v = slots['v'] = beta2 * slots.get('v', np.zeros_like(p)) + (1 - beta2) * g * g
    alpha = lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    return p - alpha * m / (np.sqrt(v) + eps)


def masked(step, p, g, slots, mask, *a, **kw):
    """a 0 / 1 update mask: masked-out elements keep their weight and their slots"""
    old = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in slots.items()}
    new = step(p, g, slots, *a, **kw)
    keep = np.asarray(mask) == 0
    for k, v in slots.items():
        if isinstance(v, np.ndarray):
            v[keep] = old[k][keep] if k in old else 0.0
    return np.where(keep, p, new)


# ------------------------------------------------------------------ clipping
def clip_value(g, c):
    return np.clip(np.asarray(g, np.float64), -c, c)


def global_norm(g):
    g = np.asarray(g, np.float64)
    return float(np.sqrt(np.sum(g * g)))


def clip_global_norm(g, c):
    """g * min(1, c / ||g||); a non-finite norm leaves g as it is.  Returns (clipped, norm)."""
    g = np.asarray(g, np.float64)
    n = global_norm(g)
    if not np.isfinite(n) or n <= c:
        return g.copy(), n
    return g * (c / n), n


# ------------------------------------------------------------------ callbacks: the decisions, on a scripted metric sequence
def _mode(mode, monitor):
    return ('max' if 'acc' in monitor else 'min') if mode == 'auto' else mode


def reduce_lr_on_plateau(values, lr, factor=0.1, patience=10, min_delta=1e-4, cooldown=0, min_lr=0.0, mode='min'):
    """-> the rate each epoch RAN with (what Keras logs as `lr` at the end of that epoch), plus the rate after the last epoch"""
    best = -np.inf if mode == 'max' else np.inf
    wait = cool = 0
    out = []
    for cur in values:
        out.append(lr)
        if cool > 0:
            cool -= 1
            wait = 0
        better = cur > best + min_delta if mode == 'max' else cur < best - min_delta
        if better:
            best, wait = cur, 0
        elif cool <= 0:
            wait += 1
            if wait >= patience and lr > min_lr:
                lr = max(lr * factor, min_lr)
                cool, wait = cooldown, 0
    return out, lr


def early_stopping(values, min_delta=0.0, patience=0, mode='min'):
    """-> (epoch at which training stops or None, best epoch)"""
    best = -np.inf if mode == 'max' else np.inf
    wait, best_epoch = 0, 0
    for epoch, cur in enumerate(values):
        better = cur - abs(min_delta) > best if mode == 'max' else cur + abs(min_delta) < best
        if better:
            best, best_epoch, wait = cur, epoch, 0
            continue
        wait += 1
        if wait >= patience:
            return epoch, best_epoch
    return None, best_epoch


def scheduled_rates(schedule, lr, epochs):
    """LearningRateScheduler: the rate of every epoch, schedule(epoch, previous rate)"""
    out = []
    for e in range(epochs):
        lr = float(schedule(e, lr))
        out.append(lr)
    return out
