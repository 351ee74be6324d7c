"""
The C ABI of ``libdeepbinner_hip.so`` as ctypes sees it (``include/deepbinner_hip.h``): the one
table of its functions, the two structs, the constants mirrored from the header, the loader and
``check``.  Every other submodule of ``hip_backend`` builds on this one.
"""

import ctypes
import os

import numpy as np
from numpy.ctypeslib import ndpointer

from .. import _cabi

# Kernel arguments in device memory: 54.4 us per forward launch against 56.5 us with the
# arguments fetched from host memory (HIP_FORCE_DEV_KERNARG=0), same box.  It is this image's
# default; say so before the HIP runtime starts, unless the user said otherwise.
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

_LIB_NAME = 'libdeepbinner_hip.so'
_lib = None

# mirrored from the header: dbh_status (the one code Python tells apart), DBH_SIDE_*,
# DBH_REQUIRE_*, the flags of dbh_model_create_ex and the answers of dbh_model_kind
ERR_COMM = 7
SIDE_START, SIDE_END = 0, 1
COMBINE_MODES = {'require_either': 0, 'require_start': 1, 'require_both': 2}
MODEL_AUTO, MODEL_GENERAL = 0, 1                 # dbh_model_create_ex flags
KIND_PERSISTENT, KIND_GENERAL = 0, 1             # dbh_model_kind
# (the geometry dbh_model_create_ex takes: classify.MIN_INPUT_SIZE .. MAX_CLASSES)


class HipBackendError(RuntimeError):
    pass


def library_path():
    # DEEPBINNER_HIP_LIB: developer knob for A/B runs of two builds on the same GPU box
    return os.environ.get('DEEPBINNER_HIP_LIB') or os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), _LIB_NAME)


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


def _signatures():
    c_int, c_i64, c_u64, c_size_t = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t
    c_float, c_double, c_char_p = ctypes.c_float, ctypes.c_double, ctypes.c_char_p
    ptr, P = ctypes.c_void_p, ctypes.POINTER            # void*; pointer to
    i16, i32, i64, f32 = (ndpointer(t, flags='C_CONTIGUOUS')
                          for t in (np.int16, np.int32, np.int64, np.float32))
    return {
        'dbh_version': (c_char_p, []),
        'dbh_status_string': (c_char_p, [c_int]),
        'dbh_last_error': (c_char_p, []),
        'dbh_device_count': (c_int, [P(c_int)]),
        'dbh_set_device': (c_int, [c_int]),
        'dbh_get_device': (c_int, [P(c_int)]),
        'dbh_device_name': (c_int, [c_int, c_char_p, c_int]),
        'dbh_device_synchronize': (c_int, []),
        'dbh_malloc': (c_int, [P(ptr), c_size_t]),
        'dbh_free': (c_int, [ptr]),
        'dbh_malloc_host': (c_int, [P(ptr), c_size_t]),
        'dbh_free_host': (c_int, [ptr]),
        'dbh_host_device_pointer': (c_int, [ptr, P(ptr)]),
        'dbh_memcpy_h2d': (c_int, [ptr, ptr, c_size_t, ptr]),
        'dbh_memcpy_d2h': (c_int, [ptr, ptr, c_size_t, ptr]),
        'dbh_memcpy_d2d': (c_int, [ptr, ptr, c_size_t, ptr]),
        'dbh_stream_create': (c_int, [P(ptr)]),
        'dbh_stream_destroy': (c_int, [ptr]),
        'dbh_stream_synchronize': (c_int, [ptr]),
        'dbh_event_create': (c_int, [P(ptr)]),
        'dbh_event_destroy': (c_int, [ptr]),
        'dbh_event_record': (c_int, [ptr, ptr]),
        'dbh_event_synchronize': (c_int, [ptr]),
        'dbh_stream_wait_event': (c_int, [ptr, ptr]),
        'dbh_event_elapsed_ms': (c_int, [ptr, ptr, P(c_float)]),
        'dbh_model_create': (c_int, [f32, c_i64, c_int, c_int, P(ptr)]),
        'dbh_model_create_ex': (c_int, [f32, c_i64, c_int, c_int, ctypes.c_uint, P(ptr)]),
        'dbh_model_kind': (c_int, [ptr, P(c_int)]),
        'dbh_model_destroy': (c_int, [ptr]),
        'dbh_model_input_size': (c_int, [ptr, P(c_int)]),
        'dbh_model_output_size': (c_int, [ptr, P(c_int)]),
        'dbh_predict': (c_int, [ptr, f32, c_i64, f32]),
        'dbh_predict_dev': (c_int, [ptr, ptr, c_i64, ptr, ptr]),
        'dbh_classify_i16': (c_int, [ptr, i16, i64, c_i64, c_int, c_int, c_double, f32, i32]),
        'dbh_classify_pair_i16': (c_int, [ptr, ptr, ptr, ptr, c_i64, c_int, c_double, c_int, ptr,
                                          ptr, ptr, ptr, ptr]),
        'dbh_model_set_host_group': (c_int, [ptr, c_i64]),
        'dbh_model_reserve_cus': (c_int, [ptr, c_int]),
        'dbh_host_alloc': (ptr, [c_size_t, ptr]),
        'dbh_host_release': (None, [ptr, ptr]),
        'dbh_host_is_pinned': (c_int, [ptr, c_size_t, P(c_int)]),
        'dbh_inflate_last_error': (c_char_p, []),
        'dbh_zstd_decode_host': (c_int, [ptr, c_size_t, ptr, c_size_t, P(c_size_t),
                                         P(ctypes.c_int32)]),
        'dbh_svb16_decode_host': (c_int, [ptr, c_size_t, c_i64, ptr, P(ctypes.c_int32)]),
        'dbh_inflate_workspace_bytes': (c_int, [c_i64, c_i64, P(c_size_t)]),
        'dbh_inflate_dev': (c_int, [ptr, c_i64, ptr, c_i64, c_i64, ptr, ptr, ptr, c_int, ptr]),
        'dbh_inflate': (c_int, [ptr, c_size_t, ptr, c_i64, ptr, c_size_t, ptr, c_int, P(c_double)]),
        'dbh_classify_pair_deflated': (c_int, [ptr, ptr, ptr, c_i64, ptr, c_i64, ptr, c_i64, c_int,
                                               c_double, c_int, ptr, ptr, ptr, ptr]),
        'dbh_classify_pair_deflated_verbose': (c_int, [ptr, ptr, ptr, c_i64, ptr, c_i64, ptr, c_i64,
                                                       c_int, c_double, c_int, ptr, ptr, ptr, ptr,
                                                       ptr, ptr, ptr, ptr]),
        'dbh_classify_workspace_bytes': (c_int, [ptr, c_i64, c_int, P(c_size_t)]),
        'dbh_classify_i16_dev': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_int, c_double, ptr, ptr,
                                         ptr, ptr]),
        'dbh_classify_i16_batched_dev': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_int, c_int,
                                                 c_double, ptr, ptr, ptr]),
        'dbh_normalise_windows_dev': (c_int, [ptr, ptr, c_i64, c_int, c_int, ptr, ptr]),
        'dbh_merge_calls_dev': (c_int, [ptr, c_i64, c_int, c_int, c_double, ptr, ptr, ptr]),
        'dbh_combine_calls_dev': (c_int, [ptr, ptr, c_i64, c_int, ptr, ptr]),
        'dbh_sweep_windows_dev': (c_int, [ptr, ptr, c_i64, c_int, ptr, ptr, ptr]),
        'dbh_sweep_workspace_bytes': (c_int, [ptr, c_i64, c_int, P(c_size_t)]),
        'dbh_sweep_i16_dev': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_int, ptr, ptr, ptr, ptr]),
        'dbh_sweep_pair_i16': (c_int, [ptr, ptr, ptr, ptr, c_i64, c_int, ptr, ptr, ptr, ptr]),
        'dbh_sweep_tally_dev': (c_int, [ptr, ptr, ptr, ptr, ptr, c_i64, c_int, c_int, ptr, c_int,
                                        ptr, ptr]),
        'dbh_sweep_tally': (c_int, [ptr, ptr, ptr, ptr, ptr, c_i64, c_int, c_int, ptr, c_int, ptr]),
        'dbh_sweep_early_pushes': (c_int, [c_int, c_int, c_i64, P(c_int)]),
        'dbh_sweep_early_tally_dev': (c_int, [ptr, ptr, ptr, ptr, ptr, ptr, c_i64, c_int, c_int, c_int,
                                              c_i64, ptr, c_int, ptr, ptr, ptr, ptr, ptr]),
        'dbh_sweep_early_tally': (c_int, [ptr, ptr, ptr, ptr, ptr, ptr, c_i64, c_int, c_int, c_int,
                                          c_i64, ptr, c_int, ptr, ptr, ptr, ptr]),
        'dbh_sweep_early_host': (c_int, [ptr, ptr, ptr, ptr, ptr, ptr, c_i64, c_int, c_int, c_int,
                                         c_i64, ptr, c_int, ptr, ptr, ptr, ptr]),
        'dbh_scan_window_count': (c_int, [c_int, c_i64, P(c_i64)]),
        'dbh_scan_window_offsets_dev': (c_int, [ptr, c_i64, c_int, ptr, ptr]),
        'dbh_scan_windows_dev': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_int, c_i64, c_i64, ptr,
                                         ptr]),
        'dbh_scan_events_dev': (c_int, [ptr, ptr, ptr, c_i64, c_double, c_int, c_int, ptr, c_i64,
                                        ptr, ptr, ptr]),
        'dbh_scan_i16': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_double, c_int, c_int, ptr, ptr, ptr,
                                 c_i64, P(c_i64), P(c_i64)]),
        'dbh_evidence_floats': (c_int, [ptr, P(c_i64)]),
        'dbh_evidence_dev': (c_int, [ptr, ptr, c_i64, ptr, ptr, ptr]),
        'dbh_locate_dev': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_int, c_int, c_int, c_int, ptr,
                                   ptr]),
        'dbh_locate_host': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_int, c_int, c_int, c_int, ptr]),
        'dbh_locate_workspace_bytes': (c_int, [ptr, c_i64, c_int, P(c_size_t)]),
        'dbh_locate_i16': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_int, c_double, ptr, ptr, ptr]),
        'dbh_occlude_plan_dev': (c_int, [ptr, ptr, c_i64, c_int, c_int, c_int, ptr, ptr, ptr]),
        'dbh_occlude_plan_host': (c_int, [ptr, ptr, c_i64, c_int, c_int, c_int, ptr, ptr]),
        'dbh_occlude_windows_dev': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_int, c_int, ptr, ptr]),
        'dbh_occlude_windows_host': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_int, c_int, ptr]),
        'dbh_locate_occluded_workspace_bytes': (c_int, [ptr, c_i64, c_int, P(c_size_t)]),
        'dbh_locate_occluded_i16': (c_int, [ptr, ptr, ptr, c_i64, c_int, c_int, c_double, ptr, ptr,
                                            ptr, ptr]),
        'dbh_live_create': (c_int, [ptr, c_int, c_int, c_double, c_int, ctypes.c_uint32, c_i64,
                                    P(ptr)]),
        'dbh_live_destroy': (c_int, [ptr]),
        'dbh_live_push': (c_int, [ptr, ptr, ptr, ptr, ptr, ptr, c_i64]),
        'dbh_live_track': (c_int, [ptr, c_int, ptr, ptr, P(ctypes.c_int32)]),
        'dbh_live_fold_dev': (c_int, [ptr, ptr, ptr, c_i64, c_i64, c_int, c_double, c_int,
                                      ctypes.c_uint32, ptr, ptr, ptr, ptr, ptr]),
        'dbh_live_plan_host': (c_int, [c_int, c_int, c_double, c_int, ctypes.c_uint32, ptr, ptr,
                                       c_i64, ptr, ptr, ptr, ptr]),
        'dbh_live_create_pair': (c_int, [ptr, ptr, c_int, c_int, c_double, c_int, ctypes.c_uint32,
                                         c_int, c_i64, P(ptr)]),
        'dbh_live_push_pair': (c_int, [ptr, ptr, ptr, ptr, ptr, ptr, ptr, c_i64]),
        'dbh_live_end_track': (c_int, [ptr, c_int, ptr, ptr, P(ctypes.c_int32)]),
        'dbh_live_tail_plan_host': (c_int, [c_int, c_int, ptr, ptr, c_i64, ptr, ptr, ptr, ptr]),
        'dbh_live_set_policy': (c_int, [ptr, ptr, c_int, c_i64, c_int]),
        'dbh_live_push_policy': (c_int, [ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, c_i64]),
        'dbh_live_yield': (c_int, [ptr, ptr, ptr]),
        'dbh_live_set_yield': (c_int, [ptr, ptr, ptr]),
        'dbh_live_policy_dev': (c_int, [ptr, ptr, ptr, c_i64, ptr, c_int, c_i64, c_int, ptr, ptr,
                                        ptr, ptr, ptr]),
        'dbh_live_policy_plan_host': (c_int, [ptr, c_int, c_i64, c_int, ptr, c_i64, ptr, ptr, ptr,
                                              c_int, ptr, ptr, ptr, ptr, ptr]),
        'dbh_stage_floats': (c_int, [c_int, P(c_i64)]),
        'dbh_debug_forward': (c_int, [ptr, f32, c_i64, c_int, f32]),
        'dbh_forward_kernel_info': (c_int, [P(c_int), P(c_int), P(c_int)]),
        'dbh_forward_truncated_dev': (c_int, [ptr, ptr, c_i64, c_int, ptr]),
        'dbh_forward_executed_mfmas': (c_int, [c_int, P(c_i64), P(c_i64)]),
        'dbh_forward_timeline': (c_int, [ptr, f32, c_i64, i64]),
        'dbh_model_set_read_length_hint': (c_int, [ptr, c_i64, c_i64]),
        'dbh_forward_timeline_i16': (c_int, [ptr, i16, c_i64, i64]),
        'dbh_forward_timing_enable': (c_int, [ptr, c_int]),
        'dbh_forward_timing_enable_span': (c_int, [ptr, c_int, c_int]),
        'dbh_forward_timing_read': (c_int, [ptr, P(c_double), P(c_i64), P(c_i64)]),
        'dbh_forward_clock_enable': (c_int, [ptr, c_int]),
        'dbh_forward_clock_read': (c_int, [ptr, P(c_double)]),
        'dbh_forward_phases_enable': (c_int, [ptr, c_int]),
        'dbh_forward_phases_read': (c_int, [ptr, P(c_double), P(c_i64)]),
        'dbh_forward_phases_count': (c_int, [P(c_int)]),
        'dbh_lds_fill': (c_int, [c_int, ctypes.c_uint32, c_int, c_int, P(c_int), P(c_int)]),
        'dbh_lds_survey': (c_int, [c_int, ctypes.c_uint32, c_int, c_int, i64, i64, P(c_int),
                                   P(c_int)]),
        'dbh_gradients_max_windows': (c_int, [c_int, P(c_i64)]),
        'dbh_gradients_workspace_bytes': (c_int, [c_int, c_int, c_i64, P(c_size_t)]),
        'dbh_gradients': (c_int, [f32, c_i64, c_int, c_int, f32, i32, c_i64, c_float, c_u64,
                                  P(c_double), P(c_i64), f32, f32]),
        'dbh_gradients_dev': (c_int, [ptr, c_i64, c_int, c_int, ptr, ptr, c_i64, c_float, c_u64,
                                      ptr, ptr, ptr, ptr, ptr, ptr]),
        'dbh_gradients_frozen': (c_int, [f32, c_i64, c_int, c_int, f32, i32, c_i64, c_float, c_u64,
                                         P(c_double), P(c_i64), f32, f32, c_int]),
        'dbh_gradients_frozen_dev': (c_int, [ptr, c_i64, c_int, c_int, ptr, ptr, c_i64, c_float,
                                             c_u64, ptr, ptr, ptr, ptr, ptr, ptr, c_int]),
        'dbh_trainer_default_options': (c_int, [P(TrainerOptions)]),
        'dbh_nadam_schedule': (c_int, [c_i64, c_double, P(TrainerOptions), P(NadamCoefficients)]),
        'dbh_train_noise': (c_int, [f32, c_i64, c_int, c_float, c_u64, f32]),
        'dbh_train_noise_dev': (c_int, [ptr, c_i64, c_int, c_float, c_u64, ptr, ptr]),
        'dbh_nadam_update': (c_int, [ptr, ptr, ptr, ptr, ptr, c_i64, c_int, P(NadamCoefficients)]),
        'dbh_nadam_update_dev': (c_int, [ptr, ptr, ptr, ptr, ptr, c_i64, c_int,
                                         P(NadamCoefficients), ptr]),
        'dbh_nadam_update_frozen': (c_int, [ptr, ptr, ptr, ptr, ptr, c_i64, c_int,
                                            P(NadamCoefficients), c_int]),
        'dbh_nadam_update_frozen_dev': (c_int, [ptr, ptr, ptr, ptr, ptr, c_i64, c_int,
                                                P(NadamCoefficients), ptr, c_int]),
        'dbh_trainer_create': (c_int, [ptr, c_i64, c_int, c_int, c_i64, P(TrainerOptions), P(ptr)]),
        'dbh_trainer_destroy': (c_int, [ptr]),
        'dbh_trainer_step': (c_int, [ptr, ptr, ptr, c_i64, P(c_double), P(c_i64)]),
        'dbh_trainer_step_dev': (c_int, [ptr, ptr, ptr, c_i64, ptr, ptr, ptr]),
        'dbh_trainer_get_weights': (c_int, [ptr, f32, c_i64]),
        'dbh_trainer_get_state': (c_int, [ptr, f32, f32, c_i64, P(c_i64), P(c_double)]),
        'dbh_trainer_set_state': (c_int, [ptr, ptr, ptr, c_i64, c_i64, c_double]),
        'dbh_trainer_iterations': (c_int, [ptr, P(c_i64)]),
        'dbh_trainer_set_frozen': (c_int, [ptr, c_int]),
        'dbh_trainer_get_frozen': (c_int, [ptr, P(c_int)]),
        'dbh_epoch_order': (c_int, [c_u64, c_i64, c_i64, ptr]),
        'dbh_dataset_create': (c_int, [ptr, ptr, c_i64, c_int, c_int, P(ptr)]),
        'dbh_dataset_destroy': (c_int, [ptr]),
        'dbh_dataset_count': (c_int, [ptr, P(c_i64)]),
        'dbh_dataset_batch': (c_int, [ptr, ptr, c_i64, c_double, c_u64, ptr, ptr]),
        'dbh_dataset_batch_dev': (c_int, [ptr, ptr, c_i64, c_double, c_u64, ptr, ptr, ptr]),
        'dbh_evaluate': (c_int, [ptr, c_i64, c_int, c_int, ptr, ptr, c_i64, P(c_double), P(c_i64),
                                 ptr]),
        'dbh_evaluate_dev': (c_int, [ptr, c_i64, c_int, c_int, ptr, ptr, c_i64, ptr, ptr, ptr, ptr,
                                     ptr]),
        'dbh_trainer_step_dataset': (c_int, [ptr, ptr, ptr, c_i64, c_double, P(c_double),
                                             P(c_i64)]),
        'dbh_trainer_step_dataset_dev': (c_int, [ptr, ptr, ptr, c_i64, c_double, ptr, ptr, ptr]),
        'dbh_trainer_evaluate_dataset': (c_int, [ptr, ptr, c_i64, c_i64, P(c_double), P(c_i64),
                                                 ptr]),
        'dbh_text_parse': (c_int, [ptr, c_i64, c_int, c_i64, ptr, ptr, ptr, P(c_i64), P(c_i64)]),
        'dbh_text_parse_host': (c_int, [ptr, c_i64, c_int, c_i64, ptr, ptr, ptr, P(c_i64),
                                        P(c_i64)]),
        'dbh_text_stage_ms': (c_int, [P(c_double), P(c_double), P(c_double)]),
        'dbh_random_signals': (c_int, [c_u64, c_i64, c_i64, c_int, ptr]),
        'dbh_random_signals_dev': (c_int, [c_u64, c_i64, c_i64, c_int, ptr, ptr]),
        'dbh_random_signals_host': (c_int, [c_u64, c_i64, c_i64, c_int, ptr]),
        'dbh_text_format_bound': (c_int, [c_i64, c_int, P(c_i64)]),
        'dbh_text_format_workspace_bytes': (c_int, [c_i64, P(c_size_t)]),
        'dbh_text_format': (c_int, [ptr, ptr, c_i64, c_int, ptr, c_i64, P(c_i64)]),
        'dbh_text_format_dev': (c_int, [ptr, ptr, c_i64, c_int, ptr, c_i64, ptr, ptr, ptr]),
        'dbh_text_format_host': (c_int, [ptr, ptr, c_i64, c_int, ptr, c_i64, P(c_i64)]),
        'dbh_comm_available': (c_int, []),
        'dbh_comm_last_error': (c_char_p, []),
        'dbh_comm_init_all': (c_int, [c_int, P(c_int), c_int, P(ptr)]),
        'dbh_comm_unique_id': (c_int, [c_char_p]),
        'dbh_comm_init_rank': (c_int, [c_char_p, c_int, c_int, P(ptr)]),
        'dbh_comm_info': (c_int, [ptr, P(c_int), P(c_int), P(c_int)]),
        'dbh_comm_all_gather_i32': (c_int, [ptr, P(ptr), P(ptr), c_i64, P(ptr)]),
        'dbh_comm_destroy': (c_int, [ptr]),
    }


# The ABI, once: {name: (restype, argtypes)}.  tests/test_abi.py holds its names to the header.
SIGNATURES = _signatures()
EXPORTED_SYMBOLS = list(SIGNATURES)


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
        _lib = _cabi.bind(path, SIGNATURES)     # AttributeError = header and library out of step
    except OSError as e:
        raise HipBackendError('could not load {}: {}'.format(path, e)) from e
    return _lib


def check(status, what='libdeepbinner_hip call'):
    if status != 0:
        lib = load_library()
        msg = lib.dbh_status_string(status).decode()
        detail = (lib.dbh_comm_last_error() if status == ERR_COMM else lib.dbh_last_error()).decode()
        raise HipBackendError('{} failed: {}{}'.format(what, msg,
                                                       ' ({})'.format(detail) if detail else ''))


# ---- small rules of the ABI's arguments, each spelled once ----------------------------------------
def _seed64(seed):
    """A Python integer as the uint64 seed the ABI takes."""
    return int(seed) & (2 ** 64 - 1)


def _side(side):
    return SIDE_START if side == 'start' else SIDE_END


def _ptr(array):
    return array.ctypes.data if array is not None else None


def _handle(model):
    return model.handle if model is not None else None


def _packed(samples, offsets):
    """Packed reads as the ABI takes them: (int16 samples, int64 offsets, number of reads)."""
    samples = np.ascontiguousarray(samples, dtype=np.int16)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    if n < 0 or (n and (offsets[0] != 0 or offsets[-1] != len(samples))):
        raise ValueError('offsets do not describe the sample buffer')
    return samples, offsets, n
