"""
ctypes binding of ``libdeepbinner_hip.so`` (C ABI: ``include/deepbinner_hip.h``) and the
``HipModel`` object that stands where the reference has a Keras ``Model``:

* ``model.inputs[0].shape`` / ``model.outputs[0].shape`` / ``len(model.inputs)`` — what
  ``load_trained_model`` inspects (reference ``deepbinner/classify.py:92-99``);
* ``model.predict(x, batch_size=...)`` — seam b1 (``classify.py:361``);
* ``model.classify_signals(...)`` — seam b2, all of ``call_batch`` (``classify.py:325-384``) on
  the device.

The binding idiom follows the reference's own native binding
(``deepbinner/dtw_semi_global.py:30-41``): ``LoadLibrary`` + ``ndpointer(..., C_CONTIGUOUS)`` +
explicit ``restype``/``argtypes`` + caller-allocated outputs.

There is deliberately NO CPU fallback: if the library or a GPU is missing the error is loud.
"""

import ctypes
import io
import os

import numpy as np
from numpy.ctypeslib import ndpointer

from .model_format import ModelWeights

# Kernel arguments in device memory: 54.4 us per forward launch against 56.5 us with the
# arguments fetched from host memory (HIP_FORCE_DEV_KERNARG=0), same box.  It is this image's
# default; say so before the HIP runtime starts, unless the user said otherwise.
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

_LIB_NAME = 'libdeepbinner_hip.so'
_lib = None

SIDE_START, SIDE_END = 0, 1


class HipBackendError(RuntimeError):
    pass


def library_path():
    # DEEPBINNER_HIP_LIB: developer knob for A/B runs of two builds on the same GPU box
    return os.environ.get('DEEPBINNER_HIP_LIB') or os.path.join(
        os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)


def _f32(flags='C_CONTIGUOUS'):
    return ndpointer(dtype=np.float32, flags=flags)


class TrainerOptions(ctypes.Structure):
    """dbh_trainer_options"""
    _fields_ = [(name, ctypes.c_double) for name in
                ('lr', 'beta_1', 'beta_2', 'epsilon', 'schedule_decay', 'bn_momentum')] + [
                    ('dropout_rate', ctypes.c_float), ('noise_std', ctypes.c_float),
                    ('seed', ctypes.c_uint64)]


class NadamCoefficients(ctypes.Structure):
    """dbh_nadam_coefficients"""
    _fields_ = [(name, ctypes.c_double) for name in
                ('lr', 'beta_1', 'beta_2', 'epsilon', 'mu_t', 'mu_t1', 'sched_new', 'sched_next',
                 'beta_2_t', 'bn_momentum')]


def load_library():
    """Load (once) and type the shared library.  Raises HipBackendError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.isfile(path):
        raise HipBackendError(
            '{} has not been built - run `python -c "import __graft_entry__ as g; g.build()"` '
            '(or `make -C deepbinner_amd/csrc`). There is no CPU fallback.'.format(path))
    # (the HIP runtime maps a process's streams onto four hardware queues unless told otherwise,
    # and streams that share one run their kernels one after the other: the streaming path keeps
    # several containers in flight, each on a stream of its own - realtime.inflate_queues)
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise HipBackendError('could not load {}: {}'.format(path, e)) from e

    c_int, c_i64, c_void_p, c_size_t = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    P = ctypes.POINTER
    sigs = {
        'dbh_version': (ctypes.c_char_p, []),
        'dbh_status_string': (ctypes.c_char_p, [c_int]),
        'dbh_last_error': (ctypes.c_char_p, []),
        'dbh_device_count': (c_int, [P(c_int)]),
        'dbh_set_device': (c_int, [c_int]),
        'dbh_get_device': (c_int, [P(c_int)]),
        'dbh_device_name': (c_int, [c_int, ctypes.c_char_p, c_int]),
        'dbh_device_synchronize': (c_int, []),
        'dbh_malloc': (c_int, [P(c_void_p), c_size_t]),
        'dbh_free': (c_int, [c_void_p]),
        'dbh_malloc_host': (c_int, [P(c_void_p), c_size_t]),
        'dbh_free_host': (c_int, [c_void_p]),
        'dbh_host_device_pointer': (c_int, [c_void_p, P(c_void_p)]),
        'dbh_memcpy_h2d': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
        'dbh_memcpy_d2h': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
        'dbh_memcpy_d2d': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
        'dbh_stream_create': (c_int, [P(c_void_p)]),
        'dbh_stream_destroy': (c_int, [c_void_p]),
        'dbh_stream_synchronize': (c_int, [c_void_p]),
        'dbh_event_create': (c_int, [P(c_void_p)]),
        'dbh_event_destroy': (c_int, [c_void_p]),
        'dbh_event_record': (c_int, [c_void_p, c_void_p]),
        'dbh_event_synchronize': (c_int, [c_void_p]),
        'dbh_stream_wait_event': (c_int, [c_void_p, c_void_p]),
        'dbh_event_elapsed_ms': (c_int, [c_void_p, c_void_p, P(ctypes.c_float)]),
        'dbh_model_create': (c_int, [_f32(), c_i64, c_int, c_int, P(c_void_p)]),
        'dbh_model_create_ex': (c_int, [_f32(), c_i64, c_int, c_int, ctypes.c_uint, P(c_void_p)]),
        'dbh_model_kind': (c_int, [c_void_p, P(c_int)]),
        'dbh_model_destroy': (c_int, [c_void_p]),
        'dbh_model_input_size': (c_int, [c_void_p, P(c_int)]),
        'dbh_model_output_size': (c_int, [c_void_p, P(c_int)]),
        'dbh_predict': (c_int, [c_void_p, _f32(), c_i64, _f32()]),
        'dbh_predict_dev': (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
        'dbh_classify_i16': (c_int, [c_void_p, ndpointer(np.int16, flags='C_CONTIGUOUS'),
                                     ndpointer(np.int64, flags='C_CONTIGUOUS'), c_i64, c_int,
                                     c_int, ctypes.c_double, _f32(),
                                     ndpointer(np.int32, flags='C_CONTIGUOUS')]),
        'dbh_classify_pair_i16': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int,
                                          ctypes.c_double, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
        'dbh_model_set_host_group': (c_int, [c_void_p, c_i64]),
        'dbh_model_reserve_cus': (c_int, [c_void_p, c_int]),
        'dbh_host_alloc': (c_void_p, [c_size_t, c_void_p]),
        'dbh_host_release': (None, [c_void_p, c_void_p]),
        'dbh_host_is_pinned': (c_int, [c_void_p, c_size_t, P(c_int)]),
        'dbh_inflate_last_error': (ctypes.c_char_p, []),
        'dbh_zstd_decode_host': (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, P(c_size_t),
                                         P(ctypes.c_int32)]),
        'dbh_inflate_workspace_bytes': (c_int, [c_i64, c_i64, P(c_size_t)]),
        'dbh_inflate_dev': (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_void_p,
                                    c_void_p, c_int, c_void_p]),
        'dbh_inflate': (c_int, [c_void_p, c_size_t, c_void_p, c_i64, c_void_p, c_size_t, c_void_p,
                                c_int, P(ctypes.c_double)]),
        'dbh_classify_pair_deflated': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64,
                                               c_void_p, c_i64, c_int, ctypes.c_double, c_int,
                                               c_void_p, c_void_p, c_void_p, c_void_p]),
        'dbh_classify_pair_deflated_verbose': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p,
                                                       c_i64, c_void_p, c_i64, c_int,
                                                       ctypes.c_double, c_int, c_void_p, c_void_p,
                                                       c_void_p, c_void_p, c_void_p, c_void_p,
                                                       c_void_p, c_void_p]),
        'dbh_classify_workspace_bytes': (c_int, [c_void_p, c_i64, c_int, P(c_size_t)]),
        'dbh_classify_i16_dev': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int,
                                         ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
        'dbh_classify_i16_batched_dev': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int,
                                                 c_int, ctypes.c_double, c_void_p, c_void_p,
                                                 c_void_p]),
        'dbh_normalise_windows_dev': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p,
                                              c_void_p]),
        'dbh_merge_calls_dev': (c_int, [c_void_p, c_i64, c_int, c_int, ctypes.c_double, c_void_p,
                                        c_void_p, c_void_p]),
        'dbh_combine_calls_dev': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p, c_void_p]),
        'dbh_sweep_windows_dev': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p, c_void_p,
                                          c_void_p]),
        'dbh_sweep_workspace_bytes': (c_int, [c_void_p, c_i64, c_int, P(c_size_t)]),
        'dbh_sweep_i16_dev': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
        'dbh_sweep_pair_i16': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
        'dbh_sweep_tally_dev': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64,
                                        c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
        'dbh_sweep_tally': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int,
                                    c_int, c_void_p, c_int, c_void_p]),
        'dbh_scan_window_count': (c_int, [c_int, c_i64, P(c_i64)]),
        'dbh_scan_window_offsets_dev': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p]),
        'dbh_scan_windows_dev': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_i64,
                                         c_i64, c_void_p, c_void_p]),
        'dbh_scan_events_dev': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, ctypes.c_double, c_int,
                                        c_int, c_void_p, c_i64, c_void_p, c_void_p, c_void_p]),
        'dbh_scan_i16': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, ctypes.c_double, c_int,
                                 c_int, c_void_p, c_void_p, c_void_p, c_i64, P(c_i64), P(c_i64)]),
        'dbh_stage_floats': (c_int, [c_int, P(c_i64)]),
        'dbh_debug_forward': (c_int, [c_void_p, _f32(), c_i64, c_int, _f32()]),
        'dbh_forward_kernel_info': (c_int, [P(c_int), P(c_int), P(c_int)]),
        'dbh_forward_truncated_dev': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p]),
        'dbh_forward_executed_mfmas': (c_int, [c_int, P(c_i64), P(c_i64)]),
        'dbh_forward_timeline': (c_int, [c_void_p, _f32(), c_i64,
                                         ndpointer(np.int64, flags='C_CONTIGUOUS')]),
        'dbh_model_set_read_length_hint': (c_int, [c_void_p, c_i64, c_i64]),
        'dbh_forward_timeline_i16': (c_int, [c_void_p, np.ctypeslib.ndpointer(np.int16, flags='C_CONTIGUOUS'),
                                     c_i64, np.ctypeslib.ndpointer(np.int64, flags='C_CONTIGUOUS')]),
        'dbh_forward_timing_enable': (c_int, [c_void_p, c_int]),
        'dbh_forward_timing_enable_span': (c_int, [c_void_p, c_int, c_int]),
        'dbh_forward_timing_read': (c_int, [c_void_p, P(ctypes.c_double), P(c_i64), P(c_i64)]),
        'dbh_forward_clock_enable': (c_int, [c_void_p, c_int]),
        'dbh_forward_clock_read': (c_int, [c_void_p, P(ctypes.c_double)]),
        'dbh_forward_phases_enable': (c_int, [c_void_p, c_int]),
        'dbh_forward_phases_read': (c_int, [c_void_p, P(ctypes.c_double), P(ctypes.c_int64)]),
        'dbh_forward_phases_count': (c_int, [P(c_int)]),
        'dbh_gradients_max_windows': (c_int, [c_int, P(c_i64)]),
        'dbh_gradients_workspace_bytes': (c_int, [c_int, c_int, c_i64, P(ctypes.c_size_t)]),
        'dbh_gradients': (c_int, [_f32(), c_i64, c_int, c_int, _f32(),
                                  ndpointer(np.int32, flags='C_CONTIGUOUS'), c_i64, ctypes.c_float,
                                  ctypes.c_uint64, P(ctypes.c_double), P(c_i64), _f32(), _f32()]),
        'dbh_gradients_dev': (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_i64,
                                      ctypes.c_float, ctypes.c_uint64, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
        'dbh_trainer_default_options': (c_int, [P(TrainerOptions)]),
        'dbh_nadam_schedule': (c_int, [c_i64, ctypes.c_double, P(TrainerOptions),
                                       P(NadamCoefficients)]),
        'dbh_train_noise': (c_int, [_f32(), c_i64, c_int, ctypes.c_float, ctypes.c_uint64, _f32()]),
        'dbh_train_noise_dev': (c_int, [c_void_p, c_i64, c_int, ctypes.c_float, ctypes.c_uint64,
                                        c_void_p, c_void_p]),
        'dbh_nadam_update': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int,
                                     P(NadamCoefficients)]),
        'dbh_nadam_update_dev': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64,
                                         c_int, P(NadamCoefficients), c_void_p]),
        'dbh_trainer_create': (c_int, [c_void_p, c_i64, c_int, c_int, c_i64, P(TrainerOptions),
                                       P(c_void_p)]),
        'dbh_trainer_destroy': (c_int, [c_void_p]),
        'dbh_trainer_step': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, P(ctypes.c_double),
                                     P(c_i64)]),
        'dbh_trainer_step_dev': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p,
                                         c_void_p]),
        'dbh_trainer_get_weights': (c_int, [c_void_p, _f32(), c_i64]),
        'dbh_trainer_get_state': (c_int, [c_void_p, _f32(), _f32(), c_i64, P(c_i64),
                                          P(ctypes.c_double)]),
        'dbh_trainer_set_state': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i64,
                                          ctypes.c_double]),
        'dbh_trainer_iterations': (c_int, [c_void_p, P(c_i64)]),
        'dbh_epoch_order': (c_int, [ctypes.c_uint64, c_i64, c_i64, c_void_p]),
        'dbh_dataset_create': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, P(c_void_p)]),
        'dbh_dataset_destroy': (c_int, [c_void_p]),
        'dbh_dataset_count': (c_int, [c_void_p, P(c_i64)]),
        'dbh_dataset_batch': (c_int, [c_void_p, c_void_p, c_i64, ctypes.c_double, ctypes.c_uint64,
                                      c_void_p, c_void_p]),
        'dbh_dataset_batch_dev': (c_int, [c_void_p, c_void_p, c_i64, ctypes.c_double,
                                          ctypes.c_uint64, c_void_p, c_void_p, c_void_p]),
        'dbh_evaluate': (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_i64,
                                 P(ctypes.c_double), P(c_i64), c_void_p]),
        'dbh_evaluate_dev': (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_i64,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
        'dbh_trainer_step_dataset': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, ctypes.c_double,
                                             P(ctypes.c_double), P(c_i64)]),
        'dbh_trainer_step_dataset_dev': (c_int, [c_void_p, c_void_p, c_void_p, c_i64,
                                                 ctypes.c_double, c_void_p, c_void_p, c_void_p]),
        'dbh_trainer_evaluate_dataset': (c_int, [c_void_p, c_void_p, c_i64, c_i64,
                                                 P(ctypes.c_double), P(c_i64), c_void_p]),
        'dbh_text_parse': (c_int, [c_void_p, c_i64, c_int, c_i64, c_void_p, c_void_p, c_void_p,
                                   P(c_i64), P(c_i64)]),
        'dbh_text_parse_host': (c_int, [c_void_p, c_i64, c_int, c_i64, c_void_p, c_void_p, c_void_p,
                                        P(c_i64), P(c_i64)]),
        'dbh_text_stage_ms': (c_int, [P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_double)]),
        'dbh_random_signals': (c_int, [ctypes.c_uint64, c_i64, c_i64, c_int, c_void_p]),
        'dbh_random_signals_dev': (c_int, [ctypes.c_uint64, c_i64, c_i64, c_int, c_void_p, c_void_p]),
        'dbh_random_signals_host': (c_int, [ctypes.c_uint64, c_i64, c_i64, c_int, c_void_p]),
        'dbh_text_format_bound': (c_int, [c_i64, c_int, P(c_i64)]),
        'dbh_text_format_workspace_bytes': (c_int, [c_i64, P(c_size_t)]),
        'dbh_text_format': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p, c_i64, P(c_i64)]),
        'dbh_text_format_dev': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p, c_i64, c_void_p,
                                        c_void_p, c_void_p]),
        'dbh_text_format_host': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p, c_i64, P(c_i64)]),
        'dbh_comm_available': (c_int, []),
        'dbh_comm_last_error': (ctypes.c_char_p, []),
        'dbh_comm_init_all': (c_int, [c_int, P(c_int), c_int, P(c_void_p)]),
        'dbh_comm_unique_id': (c_int, [ctypes.c_char_p]),
        'dbh_comm_init_rank': (c_int, [ctypes.c_char_p, c_int, c_int, P(c_void_p)]),
        'dbh_comm_info': (c_int, [c_void_p, P(c_int), P(c_int), P(c_int)]),
        'dbh_comm_all_gather_i32': (c_int, [c_void_p, P(c_void_p), P(c_void_p), c_i64,
                                            P(c_void_p)]),
        'dbh_comm_destroy': (c_int, [c_void_p]),
    }
    for name, (restype, argtypes) in sigs.items():
        fn = getattr(lib, name)     # AttributeError here = header and library out of step
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    'dbh_version', 'dbh_status_string', 'dbh_last_error', 'dbh_device_count', 'dbh_set_device',
    'dbh_get_device', 'dbh_device_name', 'dbh_device_synchronize', 'dbh_malloc', 'dbh_free',
    'dbh_malloc_host', 'dbh_free_host', 'dbh_memcpy_h2d', 'dbh_memcpy_d2h', 'dbh_memcpy_d2d',
    'dbh_stream_create', 'dbh_stream_destroy', 'dbh_stream_synchronize', 'dbh_event_create',
    'dbh_event_destroy', 'dbh_event_record', 'dbh_event_synchronize', 'dbh_stream_wait_event',
    'dbh_event_elapsed_ms',
    'dbh_model_create', 'dbh_model_create_ex', 'dbh_model_kind', 'dbh_model_destroy', 'dbh_model_set_read_length_hint', 'dbh_model_input_size', 'dbh_model_output_size',
    'dbh_predict', 'dbh_predict_dev', 'dbh_classify_i16', 'dbh_classify_pair_i16',
    'dbh_model_set_host_group', 'dbh_model_reserve_cus', 'dbh_host_device_pointer',
    'dbh_host_alloc', 'dbh_host_release',
    'dbh_host_is_pinned',
    'dbh_classify_workspace_bytes', 'dbh_inflate_last_error', 'dbh_inflate_workspace_bytes',
    'dbh_inflate_dev', 'dbh_inflate', 'dbh_zstd_decode_host', 'dbh_classify_pair_deflated',
    'dbh_classify_pair_deflated_verbose',
    'dbh_classify_i16_dev', 'dbh_classify_i16_batched_dev', 'dbh_normalise_windows_dev', 'dbh_merge_calls_dev', 'dbh_combine_calls_dev',
    'dbh_sweep_windows_dev', 'dbh_sweep_workspace_bytes', 'dbh_sweep_i16_dev', 'dbh_sweep_pair_i16',
    'dbh_sweep_tally_dev', 'dbh_sweep_tally',
    'dbh_scan_window_count', 'dbh_scan_window_offsets_dev', 'dbh_scan_windows_dev',
    'dbh_scan_events_dev', 'dbh_scan_i16',
    'dbh_stage_floats', 'dbh_debug_forward', 'dbh_forward_kernel_info',
    'dbh_forward_truncated_dev', 'dbh_forward_executed_mfmas', 'dbh_forward_timeline', 'dbh_forward_timeline_i16', 'dbh_forward_timing_enable', 'dbh_forward_timing_enable_span',
    'dbh_forward_timing_read', 'dbh_forward_clock_enable', 'dbh_forward_clock_read', 'dbh_forward_phases_enable', 'dbh_forward_phases_read',
    'dbh_forward_phases_count',
    'dbh_gradients_max_windows', 'dbh_gradients_workspace_bytes', 'dbh_gradients', 'dbh_gradients_dev',
    'dbh_trainer_default_options', 'dbh_nadam_schedule', 'dbh_train_noise', 'dbh_train_noise_dev',
    'dbh_nadam_update', 'dbh_nadam_update_dev', 'dbh_trainer_create', 'dbh_trainer_destroy',
    'dbh_trainer_step', 'dbh_trainer_step_dev', 'dbh_trainer_get_weights', 'dbh_trainer_get_state',
    'dbh_trainer_set_state', 'dbh_trainer_iterations',
    'dbh_epoch_order', 'dbh_dataset_create', 'dbh_dataset_destroy', 'dbh_dataset_count',
    'dbh_dataset_batch', 'dbh_dataset_batch_dev', 'dbh_evaluate', 'dbh_evaluate_dev',
    'dbh_trainer_step_dataset', 'dbh_trainer_step_dataset_dev', 'dbh_trainer_evaluate_dataset',
    'dbh_text_parse', 'dbh_text_parse_host', 'dbh_text_stage_ms',
    'dbh_random_signals', 'dbh_random_signals_dev', 'dbh_random_signals_host',
    'dbh_text_format_bound', 'dbh_text_format_workspace_bytes', 'dbh_text_format',
    'dbh_text_format_dev', 'dbh_text_format_host',
    'dbh_comm_available', 'dbh_comm_last_error', 'dbh_comm_init_all', 'dbh_comm_unique_id',
    'dbh_comm_init_rank', 'dbh_comm_info', 'dbh_comm_all_gather_i32', 'dbh_comm_destroy',
]


def check(status, what='libdeepbinner_hip call'):
    if status != 0:
        lib = load_library()
        msg = lib.dbh_status_string(status).decode()
        detail = (lib.dbh_comm_last_error() if status == 7 else lib.dbh_last_error()).decode()
        raise HipBackendError('{} failed: {}{}'.format(what, msg,
                                                       ' ({})'.format(detail) if detail else ''))


def device_count():
    lib = load_library()
    n = ctypes.c_int(0)
    status = lib.dbh_device_count(ctypes.byref(n))
    if status != 0:
        return 0
    return n.value


def device_name(ordinal=0):
    lib = load_library()
    buf = ctypes.create_string_buffer(256)
    check(lib.dbh_device_name(ordinal, buf, 256), 'dbh_device_name')
    return buf.value.decode()


def set_device(ordinal):
    check(load_library().dbh_set_device(int(ordinal)), 'dbh_set_device')


def get_device():
    ordinal = ctypes.c_int(0)
    check(load_library().dbh_get_device(ctypes.byref(ordinal)), 'dbh_get_device')
    return ordinal.value


COMBINE_MODES = {'require_either': 0, 'require_start': 1, 'require_both': 2}


def combine_calls_dev(start_calls_ptr, end_calls_ptr, n_reads, mode, out_ptr, stream=None):
    """combine_calls (classify.py:298-322) over device arrays of call numbers; ``mode`` is one of
    COMBINE_MODES.  Does not block."""
    check(load_library().dbh_combine_calls_dev(start_calls_ptr, end_calls_ptr, int(n_reads),
                                               COMBINE_MODES[mode], out_ptr, stream),
          'dbh_combine_calls_dev')


def synchronize():
    check(load_library().dbh_device_synchronize(), 'dbh_device_synchronize')


def classify_pair(start_model, end_model, samples, offsets, scan_size, score_diff,
                  mode='require_either', want_sides=False, want_probs=False):
    """One batch of packed reads (``samples`` int16, ``offsets`` int64: read i is
    ``samples[offsets[i]:offsets[i+1]]``, long reads possibly cut to their scanned ends) through
    the start and the end model in ONE call of the C ABI: one upload, both models' kernels, the
    min/max merges and ``combine_calls`` on the device -> final calls int32 [N] (0 = 'none').
    Either model may be None.  ``want_sides`` / ``want_probs``: also return the per-side calls /
    probabilities: (calls, (start_calls, end_calls), (start_probs, end_probs))."""
    lib = load_library()
    models = (start_model, end_model)
    if start_model is None and end_model is None:
        raise ValueError('no model')
    samples, offsets, n = _packed(samples, offsets)
    calls = np.empty(max(n, 0), dtype=np.int32)
    n_classes = next(m.n_classes for m in models if m is not None)
    side_calls = [np.empty(n, dtype=np.int32) if (want_sides and m is not None) else None
                  for m in models]
    side_probs = [np.empty((n, n_classes), dtype=np.float32) if (want_probs and m is not None)
                  else None for m in models]
    if n > 0:
        check(lib.dbh_classify_pair_i16(
            _handle(start_model), _handle(end_model),
            samples.ctypes.data if samples.size else None, offsets.ctypes.data, n, int(scan_size),
            float(score_diff), COMBINE_MODES[mode], calls.ctypes.data, _ptr(side_calls[0]),
            _ptr(side_calls[1]), _ptr(side_probs[0]), _ptr(side_probs[1])), 'dbh_classify_pair_i16')
    if want_sides or want_probs:
        return calls, tuple(side_calls), tuple(side_probs)
    return calls


def _ptr(array):
    return array.ctypes.data if array is not None else None


def _handle(model):
    return model.handle if model is not None else None


def _packed(samples, offsets):
    samples = np.ascontiguousarray(samples, dtype=np.int16)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    if n < 0 or (n and (offsets[0] != 0 or offsets[-1] != len(samples))):
        raise ValueError('offsets do not describe the sample buffer')
    return samples, offsets, n


def sweep_steps(input_size, max_scan_size):
    """Scan sizes a sweep covers: input_size / 2 times 1 .. this many."""
    half = int(input_size) // 2
    steps = int(max_scan_size) // half if half else 0
    if steps < 1 or steps * half != int(max_scan_size):
        raise ValueError('max_scan_size must be a positive multiple of half the model input size')
    return steps


def sweep_pair(start_model, end_model, samples, offsets, max_scan_size):
    """One batch of packed reads (as ``classify_pair`` takes them) through the window pass of the
    start and the end model at ``max_scan_size`` and the fold over scan sizes, in ONE call of the
    C ABI (``dbh_sweep_pair_i16``) -> ((best_s, margin_s), (best_e, margin_e)): int32 and float64
    [N, K], column k - 1 for scan size k * input_size / 2.  The call at threshold t is
    ``np.where((best != 0) & (margin >= t), best, 0)``.  The pair of a model that is None is
    (None, None)."""
    lib = load_library()
    models = (start_model, end_model)
    first = next((m for m in models if m is not None), None)
    if first is None:
        raise ValueError('no model')
    if any(m is not None and m.input_size != first.input_size for m in models):
        raise ValueError('the two models of a sweep must have one input size')
    steps = sweep_steps(first.input_size, max_scan_size)
    samples, offsets, n = _packed(samples, offsets)
    best = [np.zeros((n, steps), dtype=np.int32) if m is not None else None for m in models]
    margin = [np.zeros((n, steps), dtype=np.float64) if m is not None else None for m in models]
    if n > 0:
        check(lib.dbh_sweep_pair_i16(
            _handle(start_model), _handle(end_model),
            samples.ctypes.data if samples.size else None, offsets.ctypes.data, n,
            int(max_scan_size), _ptr(best[0]), _ptr(margin[0]), _ptr(best[1]), _ptr(margin[1])),
            'dbh_sweep_pair_i16')
    return (best[0], margin[0]), (best[1], margin[1])


SWEEP_MODES = ('either', 'start', 'both')      # DBH_REQUIRE_EITHER, _START, _BOTH


def sweep_counts(steps, n_thresholds, both, n_classes):
    """The zeroed counts of ``sweep_tally``: int64 [K, T, modes, C + 3] - per final class, then
    right, wrong, missed - with three modes (SWEEP_MODES) for two sides and one for one."""
    return np.zeros((int(steps), int(n_thresholds), 3 if both else 1, int(n_classes) + 3),
                    dtype=np.int64)


def sweep_tally(start, end, thresholds, n_classes, labels=None, counts=None):
    """The outcomes of one batch, counted on the device (``dbh_sweep_tally``): ``start`` / ``end``
    are the (best, margin) pairs of ``sweep_pair`` (None or (None, None): that side is not there),
    ``labels`` int32 per read (0 = known to carry no barcode, negative = unknown) or None.  ADDS
    into ``counts`` (``sweep_counts``; made when None) and returns it."""
    sides = [side if side is not None and side[0] is not None else None for side in (start, end)]
    if sides[0] is None and sides[1] is None:
        raise ValueError('no side')
    shape = next(side[0].shape for side in sides if side is not None)
    n, steps = shape
    held = []
    for side in sides:
        if side is None:
            held.append((None, None))
            continue
        best = np.ascontiguousarray(side[0], dtype=np.int32)
        margin = np.ascontiguousarray(side[1], dtype=np.float64)
        if best.shape != shape or margin.shape != shape:
            raise ValueError('best and margin of both sides must be [N, K] alike')
        held.append((best, margin))
    thresholds = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.shape != (n,):
            raise ValueError('one label per read')
    if counts is None:
        counts = sweep_counts(steps, len(thresholds), sides[0] is not None and sides[1] is not None,
                              n_classes)
    want = sweep_counts(steps, len(thresholds), sides[0] is not None and sides[1] is not None,
                        n_classes).shape
    if counts.shape != want or counts.dtype != np.int64 or not counts.flags['C_CONTIGUOUS']:
        raise ValueError('counts must be a C-contiguous int64 array of shape {}'.format(want))
    check(load_library().dbh_sweep_tally(
        _ptr(held[0][0]), _ptr(held[0][1]), _ptr(held[1][0]), _ptr(held[1][1]), _ptr(labels), n, steps,
        int(n_classes), thresholds.ctypes.data if thresholds.size else None, len(thresholds),
        counts.ctypes.data), 'dbh_sweep_tally')
    return counts


def sweep_windows(model, window_probs):
    """The fold alone (``dbh_sweep_windows_dev``; parity tests): per-window probabilities float32
    [N, K, C] of ``model``'s class count -> (best int32 [N, K], margin float64 [N, K]), by the form
    of the fold that belongs to the model's kind."""
    window_probs = np.ascontiguousarray(window_probs, dtype=np.float32)
    n, steps, n_classes = window_probs.shape
    if n_classes != model.n_classes:
        raise ValueError('window_probs must have the model\'s {} classes'.format(model.n_classes))
    best = np.zeros((n, steps), dtype=np.int32)
    margin = np.zeros((n, steps), dtype=np.float64)
    if n == 0:
        return best, margin
    d_probs = DeviceBuffer.from_array(window_probs)
    d_best, d_margin = DeviceBuffer(best.nbytes), DeviceBuffer(margin.nbytes)
    try:
        check(load_library().dbh_sweep_windows_dev(model.handle, d_probs.ptr, n, steps, d_best.ptr,
                                                   d_margin.ptr, None), 'dbh_sweep_windows_dev')
        synchronize()
        return (d_best.download(best.shape, np.int32), d_margin.download(margin.shape, np.float64))
    finally:
        for buf in (d_probs, d_best, d_margin):
            buf.free()


# dbh_scan_event: a run of windows of one read that fire one class (include/deepbinner_hip.h, "scan")
SCAN_EVENT = np.dtype([('read', np.int64), ('cls', np.int32), ('first', np.int32),
                       ('last', np.int32), ('reserved', np.int32), ('peak', np.float64)])
assert SCAN_EVENT.itemsize == 32


def scan_window_count(input_size, n_samples):
    """W(n): the windows a scan cuts from a read of ``n_samples`` samples (an integer, or an array
    of them -> int64 array): 1 up to ``input_size`` samples, then one more per half input size
    begun (``dbh_scan_window_count``)."""
    input_size = int(input_size)
    if input_size % 2 or not 96 <= input_size <= 16384:
        raise ValueError('input_size must be even and from 96 to 16,384')
    if np.ndim(n_samples):
        n = np.asarray(n_samples, dtype=np.int64)
        if (n < 0).any():
            raise ValueError('a read cannot have a negative length')
        half = input_size // 2
        return np.where(n <= input_size, 1, (n - input_size + half - 1) // half + 1).astype(np.int64)
    count = ctypes.c_int64(0)
    check(load_library().dbh_scan_window_count(input_size, int(n_samples), ctypes.byref(count)),
          'dbh_scan_window_count')
    return count.value


def scan_packed(model, samples, offsets, side, threshold, min_windows=1, skip_windows=0):
    """``model.scan_packed`` as a function of the backend (what ``scan.scan`` calls)."""
    return model.scan_packed(samples, offsets, side, threshold, min_windows, skip_windows)


def scan_window_offsets(offsets, input_size):
    """``dbh_scan_window_offsets_dev`` alone (parity tests): sample offsets int64 [N + 1] ->
    window offsets int64 [N + 1]."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    d_offsets, d_out = DeviceBuffer.from_array(offsets), DeviceBuffer(8 * (n + 1))
    try:
        check(load_library().dbh_scan_window_offsets_dev(d_offsets.ptr, n, int(input_size),
                                                         d_out.ptr, None),
              'dbh_scan_window_offsets_dev')
        synchronize()
        return d_out.download((n + 1,), np.int64)
    finally:
        d_offsets.free()
        d_out.free()


def scan_windows(samples, offsets, input_size, side, first_window=0, n_windows=None):
    """The scan's front alone (``dbh_scan_windows_dev``; parity tests): global windows
    [first_window, first_window + n_windows) of the packed reads, cut, normalised and padded ->
    float32 [n_windows, input_size].  ``n_windows`` None: up to the batch's last."""
    samples, offsets, n = _packed(samples, offsets)
    lib = load_library()
    window_offsets = np.concatenate(
        [[0], np.cumsum(scan_window_count(input_size, np.diff(offsets)))]).astype(np.int64)
    if n_windows is None:
        n_windows = int(window_offsets[-1]) - int(first_window)
    x = np.zeros((int(n_windows), int(input_size)), dtype=np.float32)
    if n == 0 or n_windows == 0:
        return x
    held = [DeviceBuffer.from_array(samples), DeviceBuffer.from_array(offsets),
            DeviceBuffer(window_offsets.nbytes), DeviceBuffer(x.nbytes)]
    try:
        check(lib.dbh_scan_window_offsets_dev(held[1].ptr, n, int(input_size), held[2].ptr, None),
              'dbh_scan_window_offsets_dev')
        check(lib.dbh_scan_windows_dev(held[0].ptr, held[1].ptr, held[2].ptr, n, int(input_size),
                                       0 if side == 'start' else 1, int(first_window),
                                       int(n_windows), held[3].ptr, None), 'dbh_scan_windows_dev')
        synchronize()
        return held[3].download(x.shape, np.float32)
    finally:
        for buf in held:
            buf.free()


def scan_events(best, margin, window_offsets, threshold, min_windows=1, skip_windows=0,
                max_events=None):
    """The event pass alone (``dbh_scan_events_dev``): a track in global window order (``best``
    int32, ``margin`` float64) and the reads' window offsets -> (events SCAN_EVENT array - the
    first ``max_events`` of them; None: room for all - , the true total, interior events per read
    int32 [N])."""
    best = np.ascontiguousarray(best, dtype=np.int32)
    margin = np.ascontiguousarray(margin, dtype=np.float64)
    window_offsets = np.ascontiguousarray(window_offsets, dtype=np.int64)
    n = len(window_offsets) - 1
    if best.shape != margin.shape or best.ndim != 1 or (n >= 0 and len(best) != window_offsets[-1]):
        raise ValueError('best and margin must hold one entry per window')
    capacity = len(best) if max_events is None else int(max_events)
    held = [DeviceBuffer.from_array(best), DeviceBuffer.from_array(margin),
            DeviceBuffer.from_array(window_offsets), DeviceBuffer(max(capacity, 1) * 32),
            DeviceBuffer(max(n, 1) * 4), DeviceBuffer(8)]
    try:
        check(load_library().dbh_scan_events_dev(
            held[0].ptr, held[1].ptr, held[2].ptr, n, float(threshold), int(min_windows),
            int(skip_windows), held[3].ptr, capacity, held[4].ptr, held[5].ptr, None),
            'dbh_scan_events_dev')
        synchronize()
        total = int(held[5].download((1,), np.int64)[0])
        events = held[3].download((min(total, capacity),), SCAN_EVENT)
        return events, total, held[4].download((max(n, 0),), np.int32)
    finally:
        for buf in held:
            buf.free()


INFLATE_ZLIB, INFLATE_STORED, INFLATE_VBZ = 0, 1, 2
# HDF5's shuffle filter (int16) undone on the GPU: u32 LE N, then a zlib stream of the N shuffled
# bytes / the N shuffled bytes themselves; the status of a stream these modes refuse
INFLATE_ZLIB_SHUFFLE, INFLATE_STORED_SHUFFLE = 4, 5
INFLATE_SHUFFLE_REFUSED = 32
# dbh_inflate_stream (include/deepbinner_hip.h)
INFLATE_STREAM = np.dtype([('comp_offset', '<i8'), ('comp_bytes', '<i8'), ('out_offset', '<i8'),
                           ('out_bytes', '<i8'), ('mode', '<i4'), ('reserved', '<i4')])


def inflate(comp, streams, out_bytes, streams_per_lane=0):
    """zlib streams inflated on the GPU (``dbh_inflate``: host buffers in and out - tests and
    tools; the classify path keeps everything on the device).  ``comp``: uint8 array holding the
    streams, ``streams``: array of INFLATE_STREAM records, ``out_bytes``: size of the output
    buffer, ``streams_per_lane``: must be >= 0 and is otherwise ignored (it belonged to a retired
    form of kernel 1) -> (output uint8 array, status int32 per stream,
    milliseconds the two kernels took)."""
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    streams = np.ascontiguousarray(streams, dtype=INFLATE_STREAM)
    out = np.zeros(int(out_bytes), dtype=np.uint8)
    status = np.zeros(len(streams), dtype=np.int32)
    ms = ctypes.c_double(0)
    check(load_library().dbh_inflate(comp.ctypes.data, comp.nbytes, streams.ctypes.data,
                                     len(streams), out.ctypes.data, out.nbytes, status.ctypes.data,
                                     int(streams_per_lane), ctypes.byref(ms)), 'dbh_inflate')
    return out, status, ms.value


def classify_pair_deflated(start_model, end_model, comp, streams, offsets, scan_size, score_diff,
                           mode='require_either', want_samples=False, want_stages=False,
                           want_sides=False):
    """A raw batch of the native loader (``fast5_native.stream_raw``: the reads' Signal chunks
    as stored) -> final calls int32 [N] and the decoder's status per stream, in ONE call of the C
    ABI: upload, inflate on the GPU, both models, ``combine_calls``.  ``comp`` must include its 64
    bytes of padding (``stream_raw``'s arrays do).  ``want_samples``: also the decoded signals
    (int16, all reads back to back); ``want_stages``: milliseconds of upload / inflate / classify
    on the device; ``want_sides``: also what the verbose table prints - a dict with the sides'
    own calls (``start_calls`` / ``end_calls``, int32 [N]) and merged probabilities
    (``start_probs`` / ``end_probs``, float32 [N, classes]); None for a side without a model."""
    lib = load_library()
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    streams = np.ascontiguousarray(streams)
    if streams.dtype.itemsize != INFLATE_STREAM.itemsize:
        raise ValueError('stream records of {} bytes'.format(streams.dtype.itemsize))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    calls = np.empty(max(n, 0), dtype=np.int32)
    status = np.zeros(len(streams), dtype=np.int32)
    samples = np.empty(int(offsets[-1]) if want_samples and n > 0 else 0, dtype=np.int16)
    stages = (ctypes.c_double * 3)()
    sides = {'start_calls': None, 'end_calls': None, 'start_probs': None, 'end_probs': None}
    if want_sides:
        for side, model in (('start', start_model), ('end', end_model)):
            if model is not None:
                sides[side + '_calls'] = np.zeros(max(n, 0), dtype=np.int32)
                sides[side + '_probs'] = np.zeros((max(n, 0), model.n_classes), dtype=np.float32)

    if n > 0:
        check(lib.dbh_classify_pair_deflated_verbose(
            _handle(start_model), _handle(end_model),
            comp.ctypes.data, max(comp.nbytes - 64, 0), streams.ctypes.data, len(streams),
            offsets.ctypes.data, n, int(scan_size), float(score_diff), COMBINE_MODES[mode],
            calls.ctypes.data, status.ctypes.data, samples.ctypes.data if want_samples else None,
            stages if want_stages else None, _ptr(sides['start_calls']), _ptr(sides['end_calls']),
            _ptr(sides['start_probs']), _ptr(sides['end_probs'])), 'dbh_classify_pair_deflated_verbose')
    out = [calls, status]
    if want_samples:
        out.append(samples)
    if want_stages:
        out.append(list(stages))
    if want_sides:
        out.append(sides)
    return tuple(out)


_PINNED_LOADER = False


def use_pinned_loader_buffers(on=True):
    """Have the native fast5 loader keep its packed batches in pinned host memory (this library's
    ``dbh_host_alloc`` / ``dbh_host_release`` handed to ``f5_set_sample_allocator`` as plain C
    function pointers: the two libraries do not link each other), so that ``classify_packed`` /
    ``classify_pair`` upload them without a staging copy.  Needs a GPU; idempotent."""
    global _PINNED_LOADER
    from . import fast5_native
    if on == _PINNED_LOADER:
        return
    if on:
        lib = load_library()
        fast5_native.set_sample_allocator(ctypes.cast(lib.dbh_host_alloc, ctypes.c_void_p).value,
                                          ctypes.cast(lib.dbh_host_release, ctypes.c_void_p).value)
    else:
        fast5_native.set_sample_allocator(None, None)
    _PINNED_LOADER = bool(on)


def is_pinned(array):
    """Does this numpy array lie in pinned host memory?"""
    flag = ctypes.c_int(0)
    check(load_library().dbh_host_is_pinned(array.ctypes.data, array.nbytes, ctypes.byref(flag)),
          'dbh_host_is_pinned')
    return bool(flag.value)


class Stream:
    """A non-blocking HIP stream owned through the C ABI; ``ptr`` is the raw hipStream_t (what the
    ``*_dev`` entry points take, and what ``torch.cuda.ExternalStream`` wraps)."""

    def __init__(self):
        self._lib = load_library()
        s = ctypes.c_void_p()
        check(self._lib.dbh_stream_create(ctypes.byref(s)), 'dbh_stream_create')
        self.ptr = s.value

    def synchronize(self):
        check(self._lib.dbh_stream_synchronize(self.ptr), 'dbh_stream_synchronize')

    def wait_event(self, event):
        """Work queued from now on waits for ``event`` (an ``Event`` recorded on another stream)."""
        check(self._lib.dbh_stream_wait_event(self.ptr, event.handle), 'dbh_stream_wait_event')

    def close(self):
        if self.ptr:
            self._lib.dbh_stream_destroy(self.ptr)
            self.ptr = None


class DeviceBuffer:
    """A raw HBM allocation owned through the C ABI (no torch / no other GPU library)."""

    def __init__(self, nbytes):
        self._lib = load_library()
        self.nbytes = int(nbytes)
        ptr = ctypes.c_void_p()
        check(self._lib.dbh_malloc(ctypes.byref(ptr), self.nbytes), 'dbh_malloc')
        self.ptr = ptr.value

    @classmethod
    def from_array(cls, array, stream=None):
        array = np.ascontiguousarray(array)
        buf = cls(max(array.nbytes, 1))
        buf.upload(array, stream)
        return buf

    def upload(self, array, stream=None):
        array = np.ascontiguousarray(array)
        assert array.nbytes <= self.nbytes
        check(self._lib.dbh_memcpy_h2d(self.ptr, array.ctypes.data, array.nbytes, stream),
              'dbh_memcpy_h2d')
        check(self._lib.dbh_stream_synchronize(stream), 'dbh_stream_synchronize')

    def download(self, shape, dtype, stream=None):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(self._lib.dbh_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, stream),
              'dbh_memcpy_d2h')
        check(self._lib.dbh_stream_synchronize(stream), 'dbh_stream_synchronize')
        return out

    def free(self):
        if self.ptr:
            self._lib.dbh_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Event:
    def __init__(self):
        self._lib = load_library()
        e = ctypes.c_void_p()
        check(self._lib.dbh_event_create(ctypes.byref(e)), 'dbh_event_create')
        self.handle = e.value

    def record(self, stream=None):
        check(self._lib.dbh_event_record(self.handle, stream), 'dbh_event_record')

    def synchronize(self):
        check(self._lib.dbh_event_synchronize(self.handle), 'dbh_event_synchronize')

    def elapsed_ms(self, later):
        ms = ctypes.c_float(0)
        check(self._lib.dbh_event_elapsed_ms(self.handle, later.handle, ctypes.byref(ms)),
              'dbh_event_elapsed_ms')
        return ms.value

    def __del__(self):
        try:
            if self.handle:
                self._lib.dbh_event_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class _TensorSpec:
    """Minimal stand-in for the Keras tensors load_trained_model looks at (classify.py:93-97)."""

    def __init__(self, shape):
        self.shape = tuple(shape)


MODEL_AUTO, MODEL_GENERAL = 0, 1                 # dbh_model_create_ex flags
KIND_PERSISTENT, KIND_GENERAL = 0, 1             # dbh_model_kind
# (the geometry dbh_model_create_ex takes: classify.MIN_INPUT_SIZE .. MAX_CLASSES)


class HipModel:
    """A trained Deepbinner model resident on one MI355X.  Models of the shipped geometry (input
    size 1024, at most 32 classes) run on the persistent forward kernel; any other supported
    geometry - or ``general=True`` - on the general path (``kind``: KIND_PERSISTENT / KIND_GENERAL)."""

    def __init__(self, weights, device=None, general=False):
        if not isinstance(weights, ModelWeights):
            raise TypeError('weights must be a ModelWeights')
        self._lib = load_library()
        if device_count() < 1:
            raise HipBackendError('no HIP device is visible - Deepbinner-AMD needs an MI355X '
                                  '(gfx950) GPU; there is no CPU fallback')
        if device is not None:
            set_device(device)
        self.device = get_device()
        self.weights = weights
        flat = weights.flat()
        handle = ctypes.c_void_p()
        check(self._lib.dbh_model_create_ex(flat, flat.size, weights.n_classes, weights.input_size,
                                            MODEL_GENERAL if general else MODEL_AUTO,
                                            ctypes.byref(handle)), 'dbh_model_create_ex')
        self._handle = handle
        self.general = bool(general)
        kind = ctypes.c_int(0)
        check(self._lib.dbh_model_kind(handle, ctypes.byref(kind)), 'dbh_model_kind')
        self.kind = kind.value
        self.n_classes = weights.n_classes
        self.input_size = weights.input_size
        self.inputs = [_TensorSpec((None, self.input_size, 1))]
        self.outputs = [_TensorSpec((None, self.n_classes))]

    @property
    def handle(self):
        return self._handle

    def close(self):
        # further queues on the same GPU that realtime.queue_clones made of this model go with it
        for _pair, more in self.__dict__.pop('_queue_clones', []):
            for clones in more:
                for clone in clones:
                    if clone is not None and clone is not self:
                        clone.close()
        if self._handle:
            self._lib.dbh_model_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- seam b1 ------------------------------------------------------------------------------
    def predict(self, x, batch_size=None, verbose=0):
        """x: [N, L, 1] (or [N, L]) float -> float32 [N, n_classes], a fresh writable array.
        ``batch_size`` is accepted for signature compatibility; results do not depend on it."""
        x = np.asarray(x)
        if x.ndim == 3:
            if x.shape[2] != 1:
                raise ValueError('expected input of shape (N, {}, 1)'.format(self.input_size))
            x = x[:, :, 0]
        if x.ndim != 2 or x.shape[1] != self.input_size:
            raise ValueError('expected input of shape (N, {}, 1)'.format(self.input_size))
        x = np.ascontiguousarray(x, dtype=np.float32)      # Keras casts float64 -> float32 too
        probs = np.empty((x.shape[0], self.n_classes), dtype=np.float32)
        if x.shape[0]:
            check(self._lib.dbh_predict(self._handle, x, x.shape[0], probs), 'dbh_predict')
        return probs

    # -- seam b2 ------------------------------------------------------------------------------
    def classify_signals(self, signals, side, scan_size, score_diff):
        """signals: list of 1-D integer arrays -> (probs float32 [N, C], calls int32 [N])."""
        n = len(signals)
        keep = int(scan_size) + self.input_size // 2      # samples any window can touch
        parts = []
        offsets = np.zeros(n + 1, dtype=np.int64)
        for i, s in enumerate(signals):
            s = np.asarray(s)
            if s.ndim != 1:
                raise ValueError('signals must be one-dimensional')
            if s.dtype != np.int16 and len(s) and (s.min() < -32768 or s.max() > 32767):
                raise ValueError('signal values do not fit int16')
            # only the scanned end of the read is shipped to the GPU; window contents and
            # positions are unchanged by dropping samples no window reaches
            part = s[:keep] if side == 'start' else s[max(len(s) - keep, 0):]
            parts.append(np.asarray(part, dtype=np.int16))
            offsets[i + 1] = offsets[i] + len(part)
        samples = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int16)
        return self.classify_packed(samples, offsets, side, scan_size, score_diff)

    def classify_packed(self, samples, offsets, side, scan_size, score_diff):
        """``classify_signals`` for reads that are already packed the way the C ABI takes them:
        read i is ``samples[offsets[i]:offsets[i+1]]`` (int16, int64).  A long read may have had
        its middle dropped as long as the first and the last ``scan_size + input_size // 2``
        samples are there (what the loaders keep): no window reaches further."""
        samples = np.ascontiguousarray(samples, dtype=np.int16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        if n < 0 or (n and (offsets[0] != 0 or offsets[-1] != len(samples))):
            raise ValueError('offsets do not describe the sample buffer')
        if samples.size == 0:
            samples = np.zeros(1, dtype=np.int16)
        probs = np.empty((max(n, 0), self.n_classes), dtype=np.float32)
        calls = np.empty(max(n, 0), dtype=np.int32)
        if n > 0:
            check(self._lib.dbh_classify_i16(self._handle, samples, offsets, n,
                                             SIDE_START if side == 'start' else SIDE_END,
                                             int(scan_size), float(score_diff), probs, calls),
                  'dbh_classify_i16')
        return probs, calls

    def sweep_packed(self, samples, offsets, side, max_scan_size):
        """``classify_packed``'s reads through the window pass at ``max_scan_size`` and the fold
        over scan sizes -> (best int32 [N, K], margin float64 [N, K]): see ``sweep_pair``."""
        pair = sweep_pair(self if side == 'start' else None, None if side == 'start' else self,
                          samples, offsets, max_scan_size)
        return pair[0] if side == 'start' else pair[1]

    def scan_packed(self, samples, offsets, side, threshold, min_windows=1, skip_windows=0,
                    track=False):
        """EVERY window of the packed reads through the network (``dbh_scan_i16``) -> the events
        of the track as a SCAN_EVENT array ordered by (read, first): runs of at least
        ``min_windows`` consecutive windows of one read whose best class is one barcode leading
        by ``threshold``; an event is interior when ``first >= skip_windows``.  ``track=True``:
        (events, best int32, margin float64, window_offsets int64 [N + 1]) - the whole ragged
        track in global window order."""
        samples, offsets, n = _packed(samples, offsets)
        window_offsets = np.concatenate(
            [[0], np.cumsum(scan_window_count(self.input_size, np.diff(offsets)))]).astype(np.int64)
        total = int(window_offsets[-1])
        events = np.zeros(total, dtype=SCAN_EVENT)          # (no more events than windows)
        best = np.zeros(total, dtype=np.int32) if track else None
        margin = np.zeros(total, dtype=np.float64) if track else None
        found, interior = ctypes.c_int64(0), ctypes.c_int64(0)
        if n > 0:
            check(self._lib.dbh_scan_i16(
                self._handle, samples.ctypes.data if samples.size else None, offsets.ctypes.data,
                n, 0 if side == 'start' else 1, float(threshold), int(min_windows),
                int(skip_windows), best.ctypes.data if track else None,
                margin.ctypes.data if track else None, events.ctypes.data, total,
                ctypes.byref(found), ctypes.byref(interior)), 'dbh_scan_i16')
        events = events[:found.value]
        assert int((events['first'] >= skip_windows).sum()) == interior.value
        return (events, best, margin, window_offsets) if track else events

    # -- device-resident entry points (inputs/outputs are raw device pointers) -----------------
    def workspace_bytes(self, n_reads, scan_size):
        n = ctypes.c_size_t(0)
        check(self._lib.dbh_classify_workspace_bytes(self._handle, n_reads, int(scan_size),
                                                     ctypes.byref(n)),
              'dbh_classify_workspace_bytes')
        return n.value

    def classify_dev(self, samples_ptr, offsets_ptr, n_reads, side, scan_size, score_diff,
                     probs_ptr, calls_ptr, workspace_ptr, stream=None):
        check(self._lib.dbh_classify_i16_dev(self._handle, samples_ptr, offsets_ptr, n_reads,
                                             SIDE_START if side == 'start' else SIDE_END,
                                             int(scan_size), float(score_diff), probs_ptr,
                                             calls_ptr, workspace_ptr, stream),
              'dbh_classify_i16_dev')

    def classify_batched_dev(self, samples_ptr, offsets_ptr, n_reads, batch_size, side, scan_size,
                             score_diff, probs_ptr, calls_ptr, stream=None):
        check(self._lib.dbh_classify_i16_batched_dev(
            self._handle, samples_ptr, offsets_ptr, n_reads, int(batch_size),
            SIDE_START if side == 'start' else SIDE_END, int(scan_size), float(score_diff),
            probs_ptr, calls_ptr, stream), 'dbh_classify_i16_batched_dev')

    def predict_dev(self, x_ptr, n_windows, probs_ptr, stream=None):
        check(self._lib.dbh_predict_dev(self._handle, x_ptr, n_windows, probs_ptr, stream),
              'dbh_predict_dev')

    def forward_truncated_dev(self, x_ptr, n_windows, last_stage, stream=None):
        check(self._lib.dbh_forward_truncated_dev(self._handle, x_ptr, n_windows, last_stage,
                                                  stream), 'dbh_forward_truncated_dev')

    def timeline(self, x):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, self.input_size))
        out = np.zeros((x.shape[0], 8, 64), dtype=np.int64)
        check(self._lib.dbh_forward_timeline(self._handle, x, x.shape[0], out),
              'dbh_forward_timeline')
        return out

    def set_host_group(self, windows_per_group=0):
        """Windows per model and group of the host-buffer pipeline (0 = the default 32,768)."""
        check(self._lib.dbh_model_set_host_group(self._handle, int(windows_per_group)),
              'dbh_model_set_host_group')

    def reserve_cus(self, n_cus=0):
        """Leave ``n_cus`` CUs out of this model's forward launches (0 = take all again): room
        for the inflate kernels of the containers that follow on other queues."""
        check(self._lib.dbh_model_reserve_cus(self._handle, int(n_cus)), 'dbh_model_reserve_cus')

    def clone(self):
        """The same weights as another model on the same GPU: its own streams and buffers - one
        more queue."""
        return HipModel(self.weights, device=self.device, general=self.general)

    def set_read_length_hint(self, read_length, capacity_samples=0):
        """Tell the ``*_dev`` entry points that every read is ``read_length`` samples long (0
        clears it); the hint is checked on the device, a wrong one only costs time."""
        check(self._lib.dbh_model_set_read_length_hint(self._handle, int(read_length),
                                                       int(capacity_samples)),
              'dbh_model_set_read_length_hint')

    def timeline_i16(self, reads):
        reads = np.ascontiguousarray(np.asarray(reads, dtype=np.int16).reshape(-1, self.input_size))
        out = np.zeros((reads.shape[0], 8, 64), dtype=np.int64)
        check(self._lib.dbh_forward_timeline_i16(self._handle, reads, reads.shape[0], out),
              'dbh_forward_timeline_i16')
        return out

    def timing_enable(self, every_nth=1, span=1):
        """Bracket a run of ``span`` consecutive forward launches with one HIP event pair at
        every n-th launch (0/False = off, True = every launch on its own)."""
        check(self._lib.dbh_forward_timing_enable_span(self._handle, int(every_nth), int(span)),
              'dbh_forward_timing_enable_span')

    def clock_enable(self, on=True):
        """Have production launches of the forward kernel note the shader clock against the wall
        clock (see dbh_forward_clock_enable)."""
        check(self._lib.dbh_forward_clock_enable(self._handle, 1 if on else 0),
              'dbh_forward_clock_enable')

    def phases_enable(self, on=True):
        """Have production launches keep the phase stamps as well (on top of clock_enable): about 1 % of
        the kernel's time, so not for timed runs."""
        check(self._lib.dbh_forward_phases_enable(self._handle, 1 if on else 0), 'dbh_forward_phases_enable')

    def phases_read(self):
        """Mean shader cycles of the five phases of a group of windows in this model's latest forward
        launch (see dbh_forward_phases_read): stages A-C, the stage D-E chain, stage F, the batched
        tail, what lies between two groups; and the number of groups averaged."""
        count = ctypes.c_int(0)
        check(self._lib.dbh_forward_phases_count(ctypes.byref(count)), 'dbh_forward_phases_count')
        out = (ctypes.c_double * count.value)()
        n = ctypes.c_int64(0)
        check(self._lib.dbh_forward_phases_read(self._handle, out, ctypes.byref(n)), 'dbh_forward_phases_read')
        return [float(v) for v in out], int(n.value)

    def clock_read(self):
        """Shader clock (GHz) during this model's latest forward launch."""
        ghz = ctypes.c_double(0)
        check(self._lib.dbh_forward_clock_read(self._handle, ctypes.byref(ghz)),
              'dbh_forward_clock_read')
        return ghz.value

    def timing_read(self):
        ms, launches, windows = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(self._lib.dbh_forward_timing_read(self._handle, ctypes.byref(ms),
                                                ctypes.byref(launches), ctypes.byref(windows)),
              'dbh_forward_timing_read')
        return ms.value, launches.value, windows.value

    # -- introspection ------------------------------------------------------------------------
    def debug_stage(self, x, stage):
        """Activations after stage 'A'..'G' (or 'logits') for windows x [N, 1024]."""
        idx = {'A': 0, 'B': 1, 'C': 2, 'D': 3, 'E': 4, 'F': 5, 'G': 6, 'logits': 7}[stage]
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, self.input_size))
        per = ctypes.c_int64(0)
        check(self._lib.dbh_stage_floats(idx, ctypes.byref(per)), 'dbh_stage_floats')
        out = np.empty((x.shape[0], per.value), dtype=np.float32)
        check(self._lib.dbh_debug_forward(self._handle, x, x.shape[0], idx, out),
              'dbh_debug_forward')
        shapes = {0: (512, 48), 1: (256, 48), 2: (128, 48), 3: (64, 48), 4: (32, 192),
                  5: (16, 48), 6: (8, 48), 7: (32,)}
        return out.reshape((x.shape[0],) + shapes[idx])


BATCH_STATS_FLOATS = 2 * 480       # batch mean then batch variance of batch_normalization_1..7


def loss_and_gradients(weights, x, labels, dropout_rate=0.15, seed=0):
    """The first half of a training step (dbh_gradients; reference train_network.py:53-55): the
    network in training mode on the windows ``x`` [N, input_size] (already normalised; the
    GaussianNoise layer is the caller's to add), the mean categorical cross-entropy against
    ``labels`` [N], and its gradient.  Returns ``(loss, n_correct, grads, batch_stats)``: ``grads``
    a flat fp32 array in the layout of ``weights.flat()`` (``ModelWeights.from_flat`` splits it;
    the moving-statistics slots are zeros), ``batch_stats`` the 960 batch means and variances."""
    lib = load_library()
    flat = weights.flat()
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, weights.input_size))
    labels = np.ascontiguousarray(np.asarray(labels).reshape(-1).astype(np.int32))
    if labels.size != x.shape[0]:
        raise ValueError('{} labels for {} windows'.format(labels.size, x.shape[0]))
    grads = np.zeros(flat.size, dtype=np.float32)
    stats = np.zeros(BATCH_STATS_FLOATS, dtype=np.float32)
    loss, correct = ctypes.c_double(0), ctypes.c_int64(0)
    check(lib.dbh_gradients(flat, flat.size, weights.n_classes, weights.input_size, x, labels,
                            x.shape[0], float(dropout_rate), int(seed) & (2 ** 64 - 1),
                            ctypes.byref(loss), ctypes.byref(correct), grads, stats),
          'dbh_gradients')
    return loss.value, int(correct.value), grads, stats


def gradients_workspace_bytes(n_classes, input_size, n_windows):
    size = ctypes.c_size_t(0)
    check(load_library().dbh_gradients_workspace_bytes(int(n_classes), int(input_size),
                                                       int(n_windows), ctypes.byref(size)),
          'dbh_gradients_workspace_bytes')
    return size.value


def gradients_dev(weights_ptr, n_floats, n_classes, input_size, x_ptr, labels_ptr, n_windows,
                  dropout_rate, seed, loss_ptr, correct_ptr, grads_ptr, stats_ptr, workspace_ptr,
                  stream=None):
    """dbh_gradients_dev on device pointers (``DeviceBuffer.ptr``); queued, not synchronised."""
    check(load_library().dbh_gradients_dev(weights_ptr, int(n_floats), int(n_classes),
                                           int(input_size), x_ptr, labels_ptr, int(n_windows),
                                           float(dropout_rate), int(seed) & (2 ** 64 - 1), loss_ptr,
                                           correct_ptr, grads_ptr, stats_ptr, workspace_ptr, stream),
          'dbh_gradients_dev')


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
    merged['seed'] = int(merged['seed']) & (2 ** 64 - 1)
    return TrainerOptions(**merged)


def library_trainer_defaults():
    """The defaults the library itself uses for a null options pointer, as a dict."""
    o = TrainerOptions()
    check(load_library().dbh_trainer_default_options(ctypes.byref(o)), 'dbh_trainer_default_options')
    return {name: getattr(o, name) for name, _ in TrainerOptions._fields_}


def step_seed(seed, t0):
    """The seed of the step behind ``t0`` steps: noise and dropout of that step hash it."""
    return (int(seed) + int(t0) * STEP_SEED_STRIDE) & (2 ** 64 - 1)


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
                                         int(seed) & (2 ** 64 - 1), out), 'dbh_train_noise')
    return out


def nadam_update(params, grads, m, v, batch_stats, n_classes, coefficients):
    """dbh_nadam_update on copies: returns the new ``(params, m, v)``; ``coefficients`` as
    nadam_schedule() gives them."""
    params, m, v = (np.array(a, dtype=np.float32, order='C').ravel() for a in (params, m, v))
    grads = np.ascontiguousarray(grads, dtype=np.float32).ravel()
    batch_stats = np.ascontiguousarray(batch_stats, dtype=np.float32).ravel()
    if not (grads.size == m.size == v.size == params.size) or batch_stats.size != BATCH_STATS_FLOATS:
        raise ValueError('params, grads, m and v must have one size, batch_stats {} floats'
                         .format(BATCH_STATS_FLOATS))
    k = NadamCoefficients(**coefficients)
    check(load_library().dbh_nadam_update(params.ctypes.data, grads.ctypes.data, m.ctypes.data,
                                          v.ctypes.data, batch_stats.ctypes.data, params.size,
                                          int(n_classes), ctypes.byref(k)), 'dbh_nadam_update')
    return params, m, v


# ---- device-fed batches and validation (include/deepbinner_hip.h, "device-fed batches"; DESIGN.md
# section 19) ------------------------------------------------------------------------------------
def epoch_order(seed, epoch_pass, n):
    """dbh_epoch_order (host only): the int64 sample order of pass ``epoch_pass`` over ``n``
    samples."""
    order = np.empty(max(int(n), 0), dtype=np.int64)
    check(load_library().dbh_epoch_order(int(seed) & (2 ** 64 - 1), int(epoch_pass), int(n),
                                         order.ctypes.data), 'dbh_epoch_order')
    return order


class TrainingDataError(ValueError):
    pass


_DATA_MESSAGES = {'label': 'a non-integer barcode class was encountered in {}',
                  'line': 'training signal not formatted correctly',
                  'sizes': 'inconsistent signal sizes in training data'}


TEXT_OK, TEXT_FORM, TEXT_COUNT, TEXT_RANGE = 0, 1, 2, 3
TEXT_BLOCK_BYTES = 64 << 20
_TEXT_LOOKAHEAD = 8192      # a text-mode reader decodes this much at a time (io.TextIOWrapper)


def text_parse_route(parse=None):
    """'host' or 'gpu': ``parse``, or DEEPBINNER_TEXT_PARSE where it is None; unset: 'host'."""
    route = parse or os.environ.get('DEEPBINNER_TEXT_PARSE') or 'host'
    if route not in ('host', 'gpu'):
        raise ValueError("the training-data text route is 'host' or 'gpu', not {!r}".format(route))
    return route


def _parse_text_block(entry, data, input_size, max_lines):
    lib = load_library()
    text, input_size = np.frombuffer(data, dtype=np.uint8), int(input_size)    # no copy
    own_bound = max_lines is None
    if own_bound:
        # 2 * input_size + 2 bytes: the shortest line that can be TEXT_OK
        max_lines = text.size // (2 * max(input_size, 1) + 2) + 1
    n_lines, first_bad = ctypes.c_int64(0), ctypes.c_int64(-1)
    for attempt in range(2):
        samples = np.empty((max_lines, max(input_size, 0)), dtype=np.int16)
        labels = np.empty(max_lines, dtype=np.int32)
        kinds = np.empty(max_lines, dtype=np.uint8)
        status = getattr(lib, entry)(text.ctypes.data if text.size else None, text.size, input_size,
                                     max_lines, samples.ctypes.data,
                                     labels.ctypes.data, kinds.ctypes.data, ctypes.byref(n_lines),
                                     ctypes.byref(first_bad))
        if not (own_bound and status == 1 and attempt == 0 and n_lines.value > max_lines):
            break
        max_lines = int(n_lines.value)      # lines shorter than a strict one: the block's own count
    check(status, entry)
    n = int(n_lines.value)
    return samples[:n], labels[:n], kinds[:n], int(first_bad.value)


def parse_training_text(data, input_size, max_lines=None):
    """dbh_text_parse: a block of whole lines (bytes, or any buffer, ending in a LF) parsed on the GPU ->
    (int16 samples [n_lines, input_size], int32 labels, uint8 kinds, first line whose kind is not
    TEXT_OK or -1).  Rows and labels of lines that are not TEXT_OK are unspecified.  ``max_lines``
    None: as many as strict lines would fit, and the block's own count where that is too few."""
    return _parse_text_block('dbh_text_parse', data, input_size, max_lines)


def parse_training_text_host(data, input_size, max_lines=None):
    """dbh_text_parse_host: the same parser as parse_training_text, run on the CPU; no device."""
    return _parse_text_block('dbh_text_parse_host', data, input_size, max_lines)


def text_stage_ms():
    """(upload, kernels, download) in ms of this thread's last parse_training_text"""
    ms = [ctypes.c_double(0) for _ in range(3)]
    check(load_library().dbh_text_stage_ms(*[ctypes.byref(m) for m in ms]), 'dbh_text_stage_ms')
    return tuple(m.value for m in ms)


def _training_line(line, number, path, input_size, messages):
    """One line of a training-data file, as the text-mode reader hands it out -> (label, int16 row,
    input_size: the row's where it was None); what does not fit raises TrainingDataError."""
    fields = line.strip().split('\t')
    if len(fields) != 2:
        raise TrainingDataError(messages['line'])
    label, values = fields
    if not label.lstrip('+-').isdigit():
        raise TrainingDataError(messages['label'].format(path))
    try:
        row = np.array(values.split(','), dtype=np.int64)
    except (ValueError, OverflowError):
        raise TrainingDataError(messages['line'])
    if row.size and (row.min() < -32768 or row.max() > 32767):
        raise TrainingDataError('line {} of {} holds signal values outside the int16 range'
                                .format(number, path))
    input_size = row.size if input_size is None else input_size
    if row.size != input_size:
        raise TrainingDataError(messages['sizes'])
    return int(label), row.astype(np.int16), input_size


def _read_training_data_host(path, input_size, messages):
    labels, rows = [], []
    with open(path, 'rt') as text:
        for number, line in enumerate(text, 1):
            label, row, input_size = _training_line(line, number, path, input_size, messages)
            labels.append(label)
            rows.append(row)
    if not rows:
        raise TrainingDataError(messages['line'])
    return np.stack(rows), np.array(labels, dtype=np.int32)


def training_text_blocks(path, block_bytes=None):
    """The file as blocks of whole lines, at most ``block_bytes`` each, cut behind a LF; a last
    line without a LF gets one.  A block is a view into one buffer that the next block reuses:
    it is good until the next one is asked for.  Yields None, and stops, at a line longer than a
    block."""
    block_bytes = block_bytes or TEXT_BLOCK_BYTES
    buffer = bytearray(block_bytes + 1)          # + 1: the LF a last line may lack
    view, held = memoryview(buffer), 0           # held: bytes of a line begun in the last read
    with open(path, 'rb') as raw:
        while True:
            got = raw.readinto(view[held:block_bytes])
            filled = held + got
            if not got:
                if held:
                    buffer[held] = 0x0a
                    yield view[:held + 1]
                return
            cut = buffer.rfind(b'\n', 0, filled) + 1
            if cut == 0:
                if filled >= block_bytes:
                    yield None
                    return
                held = filled
                continue
            yield view[:cut]
            held = filled - cut
            buffer[:held] = bytes(view[cut:filled])      # the line the cut left unfinished


def _refused_line(path, offset, length):
    """Line text as the text-mode reader would hand it out, for a line at ``offset`` that follows
    strict lines only; None where only a read of the whole file can tell (bytes outside ASCII in
    the line or in what that reader decodes along with it)."""
    with open(path, 'rb') as raw:
        raw.seek(offset)
        near = raw.read(length + _TEXT_LOOKAHEAD)
    if max(near, default=0) >= 0x80:
        return None
    return io.TextIOWrapper(io.BytesIO(near[:length]), encoding='ascii').readline()


def _read_training_data_blocks(path, input_size, messages, block_parser, block_bytes):
    asked = input_size
    with open(path, 'rt') as text:
        first = text.readline()
    if not first:
        raise TrainingDataError(messages['line'])
    _, _, input_size = _training_line(first, 1, path, input_size, messages)
    parts, lines_before, bytes_before = [], 0, 0
    for block in training_text_blocks(path, block_bytes):
        if block is None:
            return _read_training_data_host(path, asked, messages)
        samples, labels, kinds, first_bad = block_parser(block, input_size)
        if first_bad >= 0:
            block, start = bytes(block), 0
            for _ in range(first_bad):
                start = block.index(b'\n', start) + 1
            length = block.index(b'\n', start) + 1 - start
            line = _refused_line(path, bytes_before + start, length)
            if line is not None:
                # raises what the host route raises at this line, which is the first it refuses
                _training_line(line, lines_before + first_bad + 1, path, input_size, messages)
            # Python took what the grammar does not (or only it can tell): the host's route
            return _read_training_data_host(path, asked, messages)
        parts.append((samples, labels))
        lines_before += len(labels)
        bytes_before += len(block)
    if len(parts) == 1:
        return parts[0]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def strict_training_text(path, block_parser=None, block_bytes=None):
    """(int16 samples [n, L], int32 labels [n]) where EVERY line of the file is TEXT_OK with the
    first line's number of values, through ``block_parser`` (default parse_training_text); None
    otherwise, an empty file included - the caller then reads the file its own way."""
    block_parser = block_parser or parse_training_text
    with open(path, 'rb') as raw:
        input_size = raw.readline().count(b',') + 1
    if input_size > 1 << 20:
        return None
    parts = []
    for block in training_text_blocks(path, block_bytes):
        if block is None:
            return None
        samples, labels, _, first_bad = block_parser(block, input_size)
        if first_bad >= 0:
            return None
        parts.append((samples, labels))
    if len(parts) < 2:
        return parts[0] if parts else None
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def read_training_data(path, input_size=None, messages=None, parse=None, block_parser=None,
                       block_bytes=None):
    """A training-data text file (``label<TAB>v1,v2,...`` per line) as (int16 samples [n, L],
    int32 labels [n]), in one pass.  ``input_size`` None: the first line's.  A line that does not
    fit raises TrainingDataError; values outside int16 name the line, as in ``classify``.

    ``parse``: 'host' (one line at a time in Python), 'gpu' (the first line on the host, then
    blocks of ``block_bytes`` through ``block_parser``, by default parse_training_text; the first
    line a block refuses goes to the host's own code, which raises its error or, where it takes the
    line, reads the whole file), None: DEEPBINNER_TEXT_PARSE, unset 'host'.  Both routes return the
    same arrays and raise the same errors."""
    messages = messages or _DATA_MESSAGES
    if text_parse_route(parse) == 'host':
        return _read_training_data_host(path, input_size, messages)
    return _read_training_data_blocks(path, input_size, messages,
                                      block_parser or parse_training_text, block_bytes)


# ---- random signals and training-data text written (include/deepbinner_hip.h, "random signals" and
# "training-data text, written") -------------------------------------------
class DeviceSignals:
    """int16 signals [n, input_size] in a ResidentText's device buffer, queued on its stream: what
    ResidentText.random_signals returns and ResidentText.format_training_text takes."""

    def __init__(self, owner, n):
        self.owner, self.n, self.input_size = owner, int(n), owner.input_size

    def download(self):
        return self.owner.samples.download((self.n, self.input_size), np.int16, self.owner.stream.ptr)


class ResidentText:
    """Generator and formatter on the device for chunks of up to ``max_signals`` signals of
    ``input_size`` values: one stream, the device buffers and one pinned host buffer, all sized here
    and kept from chunk to chunk.  A chunk is random_signals() then format_training_text(): two
    entries queued on the stream, the text's length and the text brought down by one copy into
    the pinned buffer, ONE synchronisation; the int16 values never visit the host.
    ``last_ms``: (generator, formatter) of the last chunk in ms, by device events."""

    def __init__(self, max_signals, input_size):
        lib = self._lib = load_library()
        self.max_signals, self.input_size = int(max_signals), int(input_size)
        self.bound = text_format_bound(self.max_signals, self.input_size)
        work = ctypes.c_size_t(0)
        check(lib.dbh_text_format_workspace_bytes(self.max_signals, ctypes.byref(work)),
              'dbh_text_format_workspace_bytes')
        self.stream = Stream()
        self.samples = DeviceBuffer(self.max_signals * self.input_size * 2)
        self.labels = DeviceBuffer(self.max_signals * 4)
        self.text = DeviceBuffer(8 + self.bound)             # the length, then the text behind it
        self.work = DeviceBuffer(work.value)
        self.events = [Event() for _ in range(3)]
        host = ctypes.c_void_p()
        check(lib.dbh_malloc_host(ctypes.byref(host), 8 + self.bound), 'dbh_malloc_host')
        self._host = host.value
        self._view = memoryview((ctypes.c_ubyte * (8 + self.bound)).from_address(self._host)).cast('B')
        self.last_ms = (0.0, 0.0)

    def random_signals(self, seed, first_signal, n_signals, input_size=None):
        """dbh_random_signals_dev into the resident buffer: queued, not synchronised"""
        n = int(n_signals)
        if not 1 <= n <= self.max_signals or input_size not in (None, self.input_size):
            raise ValueError('expected 1 to {} signals of {} values'.format(self.max_signals,
                                                                            self.input_size))
        self.events[0].record(self.stream.ptr)
        check(self._lib.dbh_random_signals_dev(int(seed) & (2 ** 64 - 1), int(first_signal), n,
                                               self.input_size, self.samples.ptr, self.stream.ptr),
              'dbh_random_signals_dev')
        self.events[1].record(self.stream.ptr)
        return DeviceSignals(self, n)

    def format_training_text(self, labels, signals):
        """dbh_text_format_dev behind the generator -> the text, as a view of the pinned buffer
        that is good until the next call."""
        lib, stream = self._lib, self.stream.ptr
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if not isinstance(signals, DeviceSignals) or signals.owner is not self or \
                labels.shape != (signals.n,):
            raise ValueError('expected the signals random_signals() returned, and a label for each')
        n, bound = signals.n, text_format_bound(signals.n, self.input_size)
        check(lib.dbh_memcpy_h2d(self.labels.ptr, labels.ctypes.data, labels.nbytes, stream),
              'dbh_memcpy_h2d')
        check(lib.dbh_text_format_dev(self.labels.ptr, self.samples.ptr, n, self.input_size,
                                      self.text.ptr + 8, bound, self.text.ptr, self.work.ptr, stream),
              'dbh_text_format_dev')
        self.events[2].record(stream)
        check(lib.dbh_memcpy_d2h(self._host, self.text.ptr, 8 + bound, stream), 'dbh_memcpy_d2h')
        self.stream.synchronize()                        # the one synchronisation
        total = int.from_bytes(self._view[:8], 'little', signed=True)
        if total < 0:
            check(1, 'dbh_text_format_dev')              # a label outside +-(10^9 - 1)
        self.last_ms = (self.events[0].elapsed_ms(self.events[1]),
                        self.events[1].elapsed_ms(self.events[2]))
        return self._view[8:8 + total]

    def close(self):
        if self._host:
            self._view.release()                         # (raises while a text it handed out is held)
            self._lib.dbh_free_host(self._host)
            self._host = None
            for buffer in (self.samples, self.labels, self.text, self.work):
                buffer.free()
            self.stream.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def random_signals(seed, first_signal, n_signals, input_size, host=False):
    """dbh_random_signals: signals ``first_signal .. first_signal + n_signals`` of ``seed`` as int16
    [n_signals, input_size].  ``host``: dbh_random_signals_host, the CPU model, no device."""
    seed, first, n, size = int(seed) & (2 ** 64 - 1), int(first_signal), int(n_signals), int(input_size)
    out = np.empty((max(n, 0), max(size, 0)), dtype=np.int16)
    entry = 'dbh_random_signals_host' if host else 'dbh_random_signals'
    check(getattr(load_library(), entry)(seed, first, n, size, out.ctypes.data), entry)
    return out


def text_format_bound(n_lines, input_size):
    """dbh_text_format_bound: the bytes that the text of ``n_lines`` lines never exceeds"""
    bound = ctypes.c_int64(0)
    check(load_library().dbh_text_format_bound(int(n_lines), int(input_size), ctypes.byref(bound)),
          'dbh_text_format_bound')
    return bound.value


def format_training_text(labels, samples, host=False):
    """dbh_text_format: the training-data text of int32 ``labels`` [n] and int16 ``samples`` [n, L]
    as bytes - what parse_training_text reads back.  ``host``: dbh_text_format_host, the CPU model,
    no device."""
    lib = load_library()
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    given = np.asarray(samples)
    samples = np.ascontiguousarray(given, dtype=np.int16)
    if samples.ndim != 2 or labels.shape != (samples.shape[0],) or not np.array_equal(samples, given):
        raise ValueError('expected int16 samples of shape (n, input_size) and n labels')
    n, size = samples.shape
    entry = 'dbh_text_format_host' if host else 'dbh_text_format'
    bound = text_format_bound(n, size)
    out, n_bytes = np.empty(bound, dtype=np.uint8), ctypes.c_int64(0)
    check(getattr(lib, entry)(labels.ctypes.data, samples.ctypes.data, n, size, out.ctypes.data, bound,
                              ctypes.byref(n_bytes)), entry)
    return out[:n_bytes.value].tobytes()


def write_training_data(path, labels, samples, host=False):
    """The counterpart of read_training_data: ``labels`` and ``samples`` as a training-data text
    file at ``path``, formatted by format_training_text."""
    with open(path, 'wb') as out:
        out.write(format_training_text(labels, samples, host=host))


class Dataset:
    """A training-data set resident on the device: the int16 windows as the file holds them, their
    labels, and each window's mean and standard deviation (dbh_dataset)."""

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
                                          float(augmentation), int(seed) & (2 ** 64 - 1),
                                          x.ctypes.data, labels.ctypes.data), 'dbh_dataset_batch')
        return x, labels

    def batch_dev(self, indices_ptr, n_windows, augmentation, seed, x_ptr, labels_ptr, stream=None):
        """dbh_dataset_batch_dev on device pointers; queued, not synchronised."""
        check(self._lib.dbh_dataset_batch_dev(self._handle, indices_ptr, int(n_windows),
                                              float(augmentation), int(seed) & (2 ** 64 - 1), x_ptr,
                                              labels_ptr, stream), 'dbh_dataset_batch_dev')

    def close(self):
        if self._handle:
            self._lib.dbh_dataset_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def evaluate(weights, x, labels):
    """dbh_evaluate: the network in Keras's test phase (moving statistics, no dropout, no noise) on
    the windows ``x`` [N, input_size]: (loss sum, windows called right, fp64 loss per window)."""
    lib = load_library()
    flat = weights.flat()
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, weights.input_size))
    labels = np.ascontiguousarray(np.asarray(labels).reshape(-1).astype(np.int32))
    if labels.size != x.shape[0]:
        raise ValueError('{} labels for {} windows'.format(labels.size, x.shape[0]))
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


class Trainer:
    """A model in training, resident on one MI355X: weights, Nadam's m and v, gradients and batch
    statistics stay on the device between steps.  ``options``: TRAINER_DEFAULTS' names."""

    def __init__(self, weights, max_windows, device=None, **options):
        if not isinstance(weights, ModelWeights):
            raise TypeError('weights must be a ModelWeights')
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

    def close(self):
        if self._handle:
            self._lib.dbh_trainer_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, x, labels):
        """One training step on the windows ``x`` [N, input_size] (normalised, without noise) and
        ``labels`` [N]: returns (mean loss, windows called right) of the batch before the update."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, self.input_size))
        labels = np.ascontiguousarray(np.asarray(labels).reshape(-1).astype(np.int32))
        if labels.size != x.shape[0]:
            raise ValueError('{} labels for {} windows'.format(labels.size, x.shape[0]))
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
        on_device = DeviceBuffer.from_array(indices)
        losses, counts = DeviceBuffer(steps * 8), DeviceBuffer(steps * 8)
        try:
            for t in range(steps):
                self.step_dataset_dev(dataset, on_device.ptr + 8 * batch_size * t, batch_size,
                                      augmentation, losses.ptr + 8 * t, counts.ptr + 8 * t)
            synchronize()
            return losses.download(steps, np.float64), counts.download(steps, np.int64)
        finally:
            for buffer in (on_device, losses, counts):
                buffer.free()

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
        m = np.empty(self.n_floats, dtype=np.float32)
        v = np.empty(self.n_floats, dtype=np.float32)
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
        options['option_seed'] = np.asarray(int(self.options['seed']) & (2 ** 64 - 1), dtype=np.uint64)
        state = self.state()
        write_npz(self.state_path(path), dict(
            m=state['m'], v=state['v'], iterations=np.asarray(state['iterations'], dtype=np.int64),
            m_schedule=np.asarray(state['m_schedule'], dtype=np.float64), **options))

    @classmethod
    def from_checkpoint(cls, path, max_windows, device=None, **options):
        """The trainer save_checkpoint wrote, with its options unless ``options`` names others."""
        weights, _ = ModelWeights.load(path)
        with np.load(cls.state_path(path)) as z:
            saved = {name[len('option_'):]: (int(z[name]) if name == 'option_seed' else float(z[name]))
                     for name in z.files if name.startswith('option_')}
            state = {'m': z['m'], 'v': z['v'], 'iterations': int(z['iterations']),
                     'm_schedule': float(z['m_schedule'])}
        trainer = cls(weights, max_windows, device=device, **dict(saved, **options))
        trainer.load_state(state)
        return trainer


def forward_executed_mfmas(n_classes):
    """(MFMA instructions, FLOP) the forward kernel issues per window."""
    lib = load_library()
    n, f = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib.dbh_forward_executed_mfmas(int(n_classes), ctypes.byref(n), ctypes.byref(f)),
          'dbh_forward_executed_mfmas')
    return n.value, f.value


def forward_kernel_info():
    lib = load_library()
    t, l, v = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(lib.dbh_forward_kernel_info(ctypes.byref(t), ctypes.byref(l), ctypes.byref(v)),
          'dbh_forward_kernel_info')
    return {'threads_per_block': t.value, 'lds_bytes': l.value, 'vgprs': v.value}
