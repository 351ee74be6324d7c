"""Training on the device: loss and gradients, Nadam, the resident ``Trainer``, device-fed
batches from a ``Dataset`` and validation (DESIGN.md sections 18 and 19)."""

import ctypes

import numpy as np

from .._cabi import Finalised, Owner, Scoped
from ..model_format import ModelWeights
from ._abi import NadamCoefficients, TrainerOptions, _seed64, check, load_library
from ._device import device_arrays, set_device, synchronize
from ._training_file import read_training_data

BATCH_STATS_FLOATS = 2 * 480       # batch mean then batch variance of batch_normalization_1..7


def _windows_and_labels(x, labels, input_size):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, input_size))
    labels = np.ascontiguousarray(np.asarray(labels).reshape(-1).astype(np.int32))
    if labels.size != x.shape[0]:
        raise ValueError('{} labels for {} windows'.format(labels.size, x.shape[0]))
    return x, labels


MAX_FROZEN_BLOCKS = 7              # block j ends at batch_normalization_j; conv1d_20 is never frozen


def loss_and_gradients(weights, x, labels, dropout_rate=0.15, seed=0, frozen_blocks=0):
    """The first half of a training step (dbh_gradients; reference train_network.py:53-55): the
    network in training mode on the windows ``x`` [N, input_size] (already normalised; the
    GaussianNoise layer is the caller's to add), the mean categorical cross-entropy against
    ``labels`` [N], and its gradient.  Returns ``(loss, n_correct, grads, batch_stats)``: ``grads``
    a flat fp32 array in the layout of ``weights.flat()`` (``ModelWeights.from_flat`` splits it;
    the moving-statistics slots are zeros), ``batch_stats`` the 960 batch means and variances.
    ``frozen_blocks`` 1..7 (dbh_gradients_frozen): the same forward pass, the gradients of the
    tensors behind the frozen blocks with the bits they have at 0, zeros in the frozen slots."""
    lib = load_library()
    flat = weights.flat()
    x, labels = _windows_and_labels(x, labels, weights.input_size)
    grads = np.zeros(flat.size, dtype=np.float32)
    stats = np.zeros(BATCH_STATS_FLOATS, dtype=np.float32)
    loss, correct = ctypes.c_double(0), ctypes.c_int64(0)
    check(lib.dbh_gradients_frozen(flat, flat.size, weights.n_classes, weights.input_size, x, labels,
                                   x.shape[0], float(dropout_rate), _seed64(seed),
                                   ctypes.byref(loss), ctypes.byref(correct), grads, stats,
                                   int(frozen_blocks)), 'dbh_gradients_frozen')
    return loss.value, int(correct.value), grads, stats


def gradients_workspace_bytes(n_classes, input_size, n_windows):
    size = ctypes.c_size_t(0)
    check(load_library().dbh_gradients_workspace_bytes(int(n_classes), int(input_size),
                                                       int(n_windows), ctypes.byref(size)),
          'dbh_gradients_workspace_bytes')
    return size.value


def gradients_dev(weights_ptr, n_floats, n_classes, input_size, x_ptr, labels_ptr, n_windows,
                  dropout_rate, seed, loss_ptr, correct_ptr, grads_ptr, stats_ptr, workspace_ptr,
                  stream=None, frozen_blocks=0):
    """dbh_gradients_frozen_dev on device pointers (``DeviceBuffer.ptr``); queued, not
    synchronised."""
    check(load_library().dbh_gradients_frozen_dev(
        weights_ptr, int(n_floats), int(n_classes), int(input_size), x_ptr, labels_ptr,
        int(n_windows), float(dropout_rate), _seed64(seed), loss_ptr, correct_ptr, grads_ptr,
        stats_ptr, workspace_ptr, stream, int(frozen_blocks)), 'dbh_gradients_frozen_dev')


# ---- the resident trainer (include/deepbinner_hip.h, "a resident trainer") --
# Nadam as Keras 2.1.4 configures it for optimizer='nadam' (reference train_network.py:53-55; the
# shipped model files' training_config records lr, beta_1 and beta_2 as fp32 values), Keras's
# BatchNormalization momentum, and the network's own Dropout(0.15) and GaussianNoise(0.02)
# (network_architecture.py:25,31).  These are what Trainer passes unless told otherwise.
TRAINER_DEFAULTS = {
    'lr': float(np.float32(0.002)), 'beta_1': float(np.float32(0.9)),
    'beta_2': float(np.float32(0.999)), 'epsilon': 1e-7, 'schedule_decay': 0.004,
    'bn_momentum': 0.99, 'dropout_rate': 0.15, 'noise_std': 0.02, 'seed': 0,
}
STEP_SEED_STRIDE = 0x9E3779B97F4A7C15


def trainer_options(**options):
    """A TrainerOptions struct: TRAINER_DEFAULTS with ``options`` over them."""
    unknown = sorted(set(options) - set(TRAINER_DEFAULTS))
    if unknown:
        raise TypeError('unknown trainer option(s): {}'.format(', '.join(unknown)))
    merged = dict(TRAINER_DEFAULTS, **options)
    merged['seed'] = _seed64(merged['seed'])
    return TrainerOptions(**merged)


def library_trainer_defaults():
    """The defaults the library itself uses for a null options pointer, as a dict."""
    o = TrainerOptions()
    check(load_library().dbh_trainer_default_options(ctypes.byref(o)), 'dbh_trainer_default_options')
    return {name: getattr(o, name) for name, _ in TrainerOptions._fields_}


def step_seed(seed, t0):
    """The seed of the step behind ``t0`` steps: noise and dropout of that step hash it."""
    return _seed64(int(seed) + int(t0) * STEP_SEED_STRIDE)


def nadam_schedule(t0, m_schedule=1.0, **options):
    """dbh_nadam_schedule (host only): the coefficients of step ``t0`` as a dict; its 'sched_new' is
    the m_schedule of the step after."""
    k = NadamCoefficients()
    o = trainer_options(**options)
    check(load_library().dbh_nadam_schedule(int(t0), float(m_schedule), ctypes.byref(o),
                                            ctypes.byref(k)), 'dbh_nadam_schedule')
    return {name: getattr(k, name) for name, _ in NadamCoefficients._fields_}


def train_noise(x, noise_std, seed):
    """dbh_train_noise: ``x`` [N, input_size] plus the step's Gaussian noise, a new fp32 array."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError('expected windows of shape (N, input_size)')
    out = np.empty_like(x)
    check(load_library().dbh_train_noise(x, x.shape[0], x.shape[1], float(noise_std),
                                         _seed64(seed), out), 'dbh_train_noise')
    return out


def nadam_update(params, grads, m, v, batch_stats, n_classes, coefficients, frozen_blocks=0):
    """dbh_nadam_update_frozen on copies: returns the new ``(params, m, v)``; ``coefficients`` as
    nadam_schedule() gives them.  The elements of the first ``frozen_blocks`` blocks - weights,
    moments, moving statistics - come back as they went in."""
    params, m, v = (np.array(a, dtype=np.float32, order='C').ravel() for a in (params, m, v))
    grads = np.ascontiguousarray(grads, dtype=np.float32).ravel()
    batch_stats = np.ascontiguousarray(batch_stats, dtype=np.float32).ravel()
    if not (grads.size == m.size == v.size == params.size) or batch_stats.size != BATCH_STATS_FLOATS:
        raise ValueError('params, grads, m and v must have one size, batch_stats {} floats'
                         .format(BATCH_STATS_FLOATS))
    k = NadamCoefficients(**coefficients)
    check(load_library().dbh_nadam_update_frozen(
        params.ctypes.data, grads.ctypes.data, m.ctypes.data, v.ctypes.data, batch_stats.ctypes.data,
        params.size, int(n_classes), ctypes.byref(k), int(frozen_blocks)), 'dbh_nadam_update_frozen')
    return params, m, v


# ---- device-fed batches and validation (include/deepbinner_hip.h, "device-fed batches"; DESIGN.md
# section 19) ------------------------------------------------------------------------------------
def epoch_order(seed, epoch_pass, n):
    """dbh_epoch_order (host only): the int64 sample order of pass ``epoch_pass`` over ``n``
    samples."""
    order = np.empty(max(int(n), 0), dtype=np.int64)
    check(load_library().dbh_epoch_order(_seed64(seed), int(epoch_pass), int(n),
                                         order.ctypes.data), 'dbh_epoch_order')
    return order


class Dataset(Owner, Scoped, Finalised):
    """A training-data set resident on the device: the int16 windows as the file holds them, their
    labels, and each window's mean and standard deviation (dbh_dataset)."""

    _release = 'dbh_dataset_destroy'

    def __init__(self, samples, labels, n_classes, device=None):
        self._lib = load_library()
        self._handle = None
        samples = np.ascontiguousarray(samples, dtype=np.int16)
        labels = np.ascontiguousarray(np.asarray(labels).reshape(-1).astype(np.int32))
        if samples.ndim != 2 or labels.size != samples.shape[0]:
            raise ValueError('expected samples of shape (n, input_size) and n labels')
        if device is not None:
            set_device(device)
        self.input_size, self.n_classes = int(samples.shape[1]), int(n_classes)
        handle = ctypes.c_void_p()
        check(self._lib.dbh_dataset_create(samples.ctypes.data, labels.ctypes.data,
                                           samples.shape[0], self.input_size, self.n_classes,
                                           ctypes.byref(handle)), 'dbh_dataset_create')
        self._handle = handle

    @classmethod
    def from_arrays(cls, samples, labels, n_classes, device=None):
        return cls(samples, labels, n_classes, device=device)

    @classmethod
    def from_file(cls, path, n_classes, input_size=None, device=None, parse=None):
        samples, labels = read_training_data(path, input_size, parse=parse)
        return cls(samples, labels, n_classes, device=device)

    @property
    def handle(self):
        return self._handle

    def __len__(self):
        n = ctypes.c_int64(0)
        check(self._lib.dbh_dataset_count(self._handle, ctypes.byref(n)), 'dbh_dataset_count')
        return int(n.value)

    def batch(self, indices, augmentation=1.0, seed=0):
        """dbh_dataset_batch: (x fp32 [N, input_size], labels int32 [N]) for the samples
        ``indices``, normalised, and augmented as ``seed`` decides per batch slot."""
        indices = np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.int64)
        x = np.empty((indices.size, self.input_size), dtype=np.float32)
        labels = np.empty(indices.size, dtype=np.int32)
        check(self._lib.dbh_dataset_batch(self._handle, indices.ctypes.data, indices.size,
                                          float(augmentation), _seed64(seed),
                                          x.ctypes.data, labels.ctypes.data), 'dbh_dataset_batch')
        return x, labels

    def batch_dev(self, indices_ptr, n_windows, augmentation, seed, x_ptr, labels_ptr, stream=None):
        """dbh_dataset_batch_dev on device pointers; queued, not synchronised."""
        check(self._lib.dbh_dataset_batch_dev(self._handle, indices_ptr, int(n_windows),
                                              float(augmentation), _seed64(seed), x_ptr,
                                              labels_ptr, stream), 'dbh_dataset_batch_dev')


def evaluate(weights, x, labels):
    """dbh_evaluate: the network in Keras's test phase (moving statistics, no dropout, no noise) on
    the windows ``x`` [N, input_size]: (loss sum, windows called right, fp64 loss per window)."""
    lib = load_library()
    flat = weights.flat()
    x, labels = _windows_and_labels(x, labels, weights.input_size)
    per_window = np.empty(x.shape[0], dtype=np.float64)
    loss, correct = ctypes.c_double(0), ctypes.c_int64(0)
    check(lib.dbh_evaluate(flat.ctypes.data, flat.size, weights.n_classes, weights.input_size,
                           x.ctypes.data, labels.ctypes.data, x.shape[0], ctypes.byref(loss),
                           ctypes.byref(correct), per_window.ctypes.data), 'dbh_evaluate')
    return loss.value, int(correct.value), per_window


def write_npz(path, arrays):
    """An uncompressed ``.npz`` that ``np.load`` reads, with the zip members' time stamps fixed:
    the same arrays give the same bytes (``np.savez`` stamps the time of writing)."""
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_STORED, allowZip64=True) as z:
        for name, array in arrays.items():
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o600 << 16
            with z.open(info, 'w', force_zip64=True) as member:
                np.lib.format.write_array(member, np.asanyarray(array), allow_pickle=False)


class Trainer(Owner, Scoped, Finalised):
    """A model in training, resident on one MI355X: weights, Nadam's m and v, gradients and batch
    statistics stay on the device between steps.  ``options``: TRAINER_DEFAULTS' names.
    ``frozen_blocks`` 1..7: every step leaves the first blocks' weights, moments and moving
    statistics as they are; an option of the run, kept in no state file."""

    _release = 'dbh_trainer_destroy'

    def __init__(self, weights, max_windows, frozen_blocks=0, device=None, **options):
        if not isinstance(weights, ModelWeights):
            raise TypeError('weights must be a ModelWeights')
        if not 0 <= int(frozen_blocks) <= MAX_FROZEN_BLOCKS:     # before anything is allocated
            raise ValueError('frozen_blocks must be 0 to {}'.format(MAX_FROZEN_BLOCKS))
        self._lib = load_library()
        self._handle = None
        self.options = dict(TRAINER_DEFAULTS, **options)
        struct = trainer_options(**options)
        if device is not None:
            set_device(device)
        self.n_classes, self.input_size = weights.n_classes, weights.input_size
        self.max_windows = int(max_windows)
        flat = weights.flat()
        self.n_floats = flat.size
        handle = ctypes.c_void_p()
        check(self._lib.dbh_trainer_create(flat.ctypes.data, flat.size, self.n_classes,
                                           self.input_size, self.max_windows, ctypes.byref(struct),
                                           ctypes.byref(handle)), 'dbh_trainer_create')
        self._handle = handle
        if frozen_blocks:
            self.frozen_blocks = frozen_blocks

    @property
    def frozen_blocks(self):
        f = ctypes.c_int(0)
        check(self._lib.dbh_trainer_get_frozen(self._handle, ctypes.byref(f)), 'dbh_trainer_get_frozen')
        return int(f.value)

    @frozen_blocks.setter
    def frozen_blocks(self, value):
        """Allowed between steps: the steps queued from here on use it."""
        check(self._lib.dbh_trainer_set_frozen(self._handle, int(value)), 'dbh_trainer_set_frozen')

    def step(self, x, labels):
        """One training step on the windows ``x`` [N, input_size] (normalised, without noise) and
        ``labels`` [N]: returns (mean loss, windows called right) of the batch before the update."""
        x, labels = _windows_and_labels(x, labels, self.input_size)
        loss, correct = ctypes.c_double(0), ctypes.c_int64(0)
        check(self._lib.dbh_trainer_step(self._handle, x.ctypes.data, labels.ctypes.data, x.shape[0],
                                         ctypes.byref(loss), ctypes.byref(correct)),
              'dbh_trainer_step')
        return loss.value, int(correct.value)

    def step_dev(self, x_ptr, labels_ptr, n_windows, loss_ptr, correct_ptr, stream=None):
        """dbh_trainer_step_dev on device pointers; queued, not synchronised."""
        check(self._lib.dbh_trainer_step_dev(self._handle, x_ptr, labels_ptr, int(n_windows),
                                             loss_ptr, correct_ptr, stream), 'dbh_trainer_step_dev')

    def step_dataset(self, dataset, indices, augmentation=1.0):
        """One step on the samples ``indices`` of a ``Dataset``, assembled on the device with this
        step's seed (dbh_trainer_step_dataset): (mean loss, windows called right)."""
        indices = np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.int64)
        loss, correct = ctypes.c_double(0), ctypes.c_int64(0)
        check(self._lib.dbh_trainer_step_dataset(self._handle, dataset.handle, indices.ctypes.data,
                                                 indices.size, float(augmentation),
                                                 ctypes.byref(loss), ctypes.byref(correct)),
              'dbh_trainer_step_dataset')
        return loss.value, int(correct.value)

    def step_dataset_dev(self, dataset, indices_ptr, n_windows, augmentation, loss_ptr, correct_ptr,
                         stream=None):
        """dbh_trainer_step_dataset_dev: int64 indices on the device; queued, not synchronised."""
        check(self._lib.dbh_trainer_step_dataset_dev(self._handle, dataset.handle, indices_ptr,
                                                     int(n_windows), float(augmentation), loss_ptr,
                                                     correct_ptr, stream),
              'dbh_trainer_step_dataset_dev')

    def run_epoch(self, dataset, indices, batch_size, augmentation):
        """``len(indices) // batch_size`` steps queued without a host synchronisation in between:
        the indices are uploaded once, every step writes its own loss and count slot, one
        synchronisation at the end.  -> (mean loss per step fp64, windows right per step int64)."""
        batch_size = int(batch_size)
        steps = len(indices) // batch_size
        indices = np.ascontiguousarray(np.asarray(indices)[:steps * batch_size], dtype=np.int64)
        with device_arrays(indices, steps * 8, steps * 8) as (on_device, losses, counts):
            for t in range(steps):
                self.step_dataset_dev(dataset, on_device.ptr + 8 * batch_size * t, batch_size,
                                      augmentation, losses.ptr + 8 * t, counts.ptr + 8 * t)
            synchronize()
            return losses.download(steps, np.float64), counts.download(steps, np.int64)

    def evaluate(self, dataset, first=0, count=None, window_losses=False):
        """The resident weights in Keras's test phase on the samples [first, first + count) of a
        ``Dataset`` (dbh_trainer_evaluate_dataset): (loss sum, windows called right), and with
        ``window_losses`` the fp64 loss of each window as a third value."""
        count = len(dataset) - first if count is None else int(count)
        per_window = np.empty(count, dtype=np.float64) if window_losses else None
        loss, correct = ctypes.c_double(0), ctypes.c_int64(0)
        check(self._lib.dbh_trainer_evaluate_dataset(
            self._handle, dataset.handle, int(first), count, ctypes.byref(loss),
            ctypes.byref(correct), per_window.ctypes.data if window_losses else None),
            'dbh_trainer_evaluate_dataset')
        result = (loss.value, int(correct.value))
        return result + (per_window,) if window_losses else result

    def weights(self):
        flat = np.empty(self.n_floats, dtype=np.float32)
        check(self._lib.dbh_trainer_get_weights(self._handle, flat, flat.size),
              'dbh_trainer_get_weights')
        return ModelWeights.from_flat(flat, self.n_classes, self.input_size)

    def state(self):
        """Nadam's state: {'m', 'v' (flat fp32, the blob's layout), 'iterations', 'm_schedule'}."""
        m, v = (np.empty(self.n_floats, dtype=np.float32) for _ in 'mv')
        iterations, schedule = ctypes.c_int64(0), ctypes.c_double(0)
        check(self._lib.dbh_trainer_get_state(self._handle, m, v, m.size, ctypes.byref(iterations),
                                              ctypes.byref(schedule)), 'dbh_trainer_get_state')
        return {'m': m, 'v': v, 'iterations': int(iterations.value), 'm_schedule': schedule.value}

    def load_state(self, state):
        m = np.ascontiguousarray(state['m'], dtype=np.float32).ravel()
        v = np.ascontiguousarray(state['v'], dtype=np.float32).ravel()
        if m.size != self.n_floats or v.size != self.n_floats:
            raise ValueError('m and v must have {} floats'.format(self.n_floats))
        check(self._lib.dbh_trainer_set_state(self._handle, m.ctypes.data, v.ctypes.data, m.size,
                                              int(state['iterations']), float(state['m_schedule'])),
              'dbh_trainer_set_state')

    @property
    def iterations(self):
        n = ctypes.c_int64(0)
        check(self._lib.dbh_trainer_iterations(self._handle, ctypes.byref(n)),
              'dbh_trainer_iterations')
        return int(n.value)

    # -- checkpoints: the weights as a model file `classify` loads as it is, the rest beside it ----
    @staticmethod
    def state_path(path):
        return str(path) + '.state.npz'

    def save_checkpoint(self, path):
        self.weights().save(path)
        options = {'option_' + name: np.asarray(value, dtype=np.float64)
                   for name, value in self.options.items() if name != 'seed'}
        options['option_seed'] = np.asarray(_seed64(self.options['seed']), dtype=np.uint64)
        state = self.state()
        write_npz(self.state_path(path), dict(
            m=state['m'], v=state['v'], iterations=np.asarray(state['iterations'], dtype=np.int64),
            m_schedule=np.asarray(state['m_schedule'], dtype=np.float64), **options))

    @classmethod
    def from_checkpoint(cls, path, max_windows, frozen_blocks=0, device=None, **options):
        """The trainer save_checkpoint wrote, with its options unless ``options`` names others
        (``frozen_blocks`` is not in the file: it is the caller's to give again)."""
        weights, _ = ModelWeights.load(path)
        with np.load(cls.state_path(path)) as z:
            saved = {name[len('option_'):]: (int(z[name]) if name == 'option_seed' else float(z[name]))
                     for name in z.files if name.startswith('option_')}
            state = {'m': z['m'], 'v': z['v'], 'iterations': int(z['iterations']),
                     'm_schedule': float(z['m_schedule'])}
        trainer = cls(weights, max_windows, frozen_blocks=frozen_blocks, device=device,
                      **dict(saved, **options))
        trainer.load_state(state)
        return trainer
