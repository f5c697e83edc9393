"""CPU checks of the training surface both model families share (satellite_computervision_amd/training.py): the epoch loop of fit() on a stub
model with scripted epoch logs -- hook order, what lands in History, the `val_` entries, early stopping, the printed line -- the two metrics of
a confusion matrix, and what compile() accepts as a loss.  Nothing here touches a GPU."""
import re
import types

import numpy as np
import pytest


@pytest.fixture(scope='module')
def tr():
    from satellite_computervision_amd import training
    return training


class StubModel:
    def __init__(self, lr=0.1):
        self.stop_training = True                   # (fit_loop resets it)
        self.optimizer = types.SimpleNamespace(_lr=lr, learning_rate=lr)
        self.weights = {'w': np.zeros(2, np.float32)}

    def get_weights_dict(self):
        return {k: v.copy() for k, v in self.weights.items()}

    def set_weights_dict(self, d):
        self.weights = {k: np.asarray(v).copy() for k, v in d.items()}


class Recorder:
    def __init__(self):
        self.calls = []

    def on_train_begin(self):
        self.calls.append(('train_begin',))

    def on_epoch_begin(self, epoch):
        self.calls.append(('epoch_begin', epoch))

    def on_epoch_end(self, epoch, logs):
        self.calls.append(('epoch_end', epoch, dict(logs)))

    def on_train_end(self):
        self.calls.append(('train_end',))


def scripted(losses):
    """train_epoch closure: epoch e -> {'loss': losses[e]}; the epochs it was asked for are kept in `.seen`"""
    def train_epoch(epoch):
        train_epoch.seen.append(epoch)
        return {'loss': losses[epoch]}
    train_epoch.seen = []
    return train_epoch


def loop(tr, model, train_epoch, epochs=2, x=None, initial_epoch=0, callbacks=None, verbose=0, validate=None, show_time=False):
    return tr.fit_loop(model, x, epochs, initial_epoch, callbacks, verbose, train_epoch, validate, show_time)


def test_hooks_run_in_order_and_missing_hooks_are_skipped(tr):
    rec = Recorder()
    only_end = types.SimpleNamespace(ends=[])
    only_end.on_epoch_end = lambda epoch, logs: only_end.ends.append(epoch)        # a callback with one hook only
    m = StubModel()
    hist = loop(tr, m, scripted([0.5, 0.25]), callbacks=[rec, only_end])
    assert rec.calls == [('train_begin',), ('epoch_begin', 0), ('epoch_end', 0, {'loss': 0.5}), ('epoch_begin', 1),
                         ('epoch_end', 1, {'loss': 0.25}), ('train_end',)]
    assert only_end.ends == [0, 1]
    assert rec.model is m and only_end.model is m and m.stop_training is False
    assert dict(hist.history) == {'loss': [0.5, 0.25]} and hist.epoch == [0, 1]


def test_entries_added_by_a_callback_join_the_history_once(tr):
    class AddsLR:
        def on_epoch_end(self, epoch, logs):
            logs['lr'] = 0.1 / (epoch + 1)
    hist = loop(tr, StubModel(), scripted([3.0, 2.0, 1.0]), epochs=3, callbacks=[AddsLR()])
    assert hist.history['lr'] == [0.1, 0.05, 0.1 / 3]
    assert hist.history['loss'] == [3.0, 2.0, 1.0]                                  # (not appended a second time after the callbacks)
    assert list(hist.history) == ['loss', 'lr']


def test_learning_rate_scheduler_logs_the_rate(tr):
    m = StubModel(lr=0.5)
    hist = loop(tr, m, scripted([1.0, 1.0]), callbacks=[tr.LearningRateScheduler(lambda epoch, lr: lr * 0.5)])
    assert hist.history['lr'] == [0.25, 0.125] and m.optimizer.learning_rate == 0.125


def test_validation_values_are_prefixed(tr):
    vals = iter([{'loss': 0.9, 'acc': 0.5}, {'loss': 0.8, 'acc': 0.75}])
    hist = loop(tr, StubModel(), scripted([1.0, 0.5]), validate=lambda: next(vals))
    assert dict(hist.history) == {'loss': [1.0, 0.5], 'val_loss': [0.9, 0.8], 'val_acc': [0.5, 0.75]}
    assert list(hist.history) == ['loss', 'val_loss', 'val_acc']


def test_no_validation_no_val_keys(tr):
    rec = Recorder()
    hist = loop(tr, StubModel(), scripted([1.0, 0.5]), callbacks=[rec], validate=None)
    assert not [k for k in hist.history if k.startswith('val_')]
    assert all(not k.startswith('val_') for c in rec.calls if c[0] == 'epoch_end' for k in c[2])


def test_early_stopping_ends_the_loop_and_train_end_still_runs(tr):
    """val_loss 1, 2, 3, 4 with patience 1: epoch 0 is the best, epoch 1 is the first without an improvement -> the loop ends after epoch 1"""
    rec, train = Recorder(), scripted([1.0] * 4)
    val = iter([1.0, 2.0, 3.0, 4.0])
    m = StubModel()
    es = tr.EarlyStopping(monitor='val_loss', patience=1)
    hist = loop(tr, m, train, epochs=4, callbacks=[es, rec], validate=lambda: {'loss': next(val)})
    assert hist.epoch == [0, 1] and train.seen == [0, 1]
    assert hist.history['val_loss'] == [1.0, 2.0]
    assert m.stop_training is True and es.stopped_epoch == 1
    assert rec.calls[-1] == ('train_end',)


def test_early_stopping_restores_the_best_weights(tr):
    m = StubModel()
    val = iter([1.0, 2.0, 3.0])

    def train_epoch(epoch):
        m.weights['w'] = np.full(2, epoch + 1, np.float32)
        return {'loss': 1.0}
    loop(tr, m, train_epoch, epochs=3, callbacks=[tr.EarlyStopping(patience=1, restore_best_weights=True)], validate=lambda: {'loss': next(val)})
    np.testing.assert_array_equal(m.weights['w'], np.full(2, 1, np.float32))       # (the weights epoch 0 ended with)


def test_the_epoch_end_hook_of_x_runs_once_per_completed_epoch(tr):
    x = types.SimpleNamespace(n=0)

    def on_epoch_end():
        x.n += 1
    x.on_epoch_end = on_epoch_end
    loop(tr, StubModel(), scripted([1.0] * 3), epochs=3, x=x)
    assert x.n == 3
    loop(tr, StubModel(), scripted([1.0]), epochs=1, x=np.zeros(3))                 # (arrays have no such hook)


def test_initial_epoch(tr):
    rec, train = Recorder(), scripted([9.0, 9.0, 9.0, 0.5, 0.25])
    hist = loop(tr, StubModel(), train, epochs=5, initial_epoch=3, callbacks=[rec])
    assert hist.epoch == [3, 4] and train.seen == [3, 4] and hist.history['loss'] == [0.5, 0.25]
    assert [c[1] for c in rec.calls if c[0] == 'epoch_begin'] == [3, 4]


def test_the_printed_line(tr, capsys):
    loop(tr, StubModel(), scripted([0.5]), epochs=1, verbose=1, show_time=True, validate=lambda: {'loss': 0.25})
    line = capsys.readouterr().out.strip()
    assert re.fullmatch(r'Epoch 1/1 - \d+\.\ds - loss: 0\.5000 - val_loss: 0\.2500', line), line
    loop(tr, StubModel(), scripted([0.5]), epochs=1, verbose=1, show_time=False, validate=lambda: {'loss': 0.25})
    assert capsys.readouterr().out.strip() == 'Epoch 1/1 - loss: 0.5000 - val_loss: 0.2500'
    loop(tr, StubModel(), scripted([0.5]), epochs=1, verbose=0, show_time=True)
    assert capsys.readouterr().out == ''


def test_metrics_of_a_confusion_matrix(tr):
    """classes 0 and 2 occur, class 1 neither as a label nor as a prediction: IoU_0 = 5 / (5 + 1 + 2), IoU_2 = 4 / (4 + 2 + 1), class 1 is
    left out of the mean; accuracy = 9 / 12"""
    conf = np.array([[5, 0, 1], [0, 0, 0], [2, 0, 4]], np.int64)
    assert tr.metric_from_confusion('accuracy', conf) == pytest.approx(9 / 12, rel=1e-15)
    assert tr.metric_from_confusion('mean_io_u', conf) == pytest.approx((5 / 8 + 4 / 7) / 2, rel=1e-15)
    zero = np.zeros((3, 3), np.int64)
    assert tr.metric_from_confusion('accuracy', zero) == 0.0 and tr.metric_from_confusion('mean_io_u', zero) == 0.0


def test_loss_resolution(tr):
    spec = tr.LossSpec('iou_loss')
    assert tr.resolve_loss(spec) is spec
    got = tr.resolve_loss(lambda t, p: tr.weighted_bce(t, p, 3.0))
    assert isinstance(got, tr.LossSpec) and got.kind == 'weighted_bce' and got.weights.tolist() == [3.0]
    assert tr.resolve_loss(tr.iou_loss).kind == 'iou_loss'
    with pytest.raises(ValueError):
        tr.resolve_loss('binary_crossentropy')
    with pytest.raises(ValueError):
        tr.resolve_loss(lambda t, p: 0.5)
    with pytest.raises(ValueError):
        tr.resolve_loss(None)


def test_model_tools_hands_out_the_same_objects(tr):
    from satellite_computervision_amd import model_tools as mt
    for name in ('Adam', 'SGD', 'RMSprop', 'ModelCheckpoint', 'EarlyStopping', 'ReduceLROnPlateau', 'LearningRateScheduler', 'TensorBoard', 'MeanIoU',
                 'History', 'weighted_bce', 'weighted_categorical_crossentropy', 'gen_dice', 'iou_loss', 'mse_4d', 'LossSpec', '_LossArg',
                 'resolve_optimizer', 'apply_optimizer', 'run_callbacks', 'record_callback_logs'):
        assert getattr(mt, name) is getattr(tr, name), name
