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

This file is the public surface and only that: it imports and re-exports.  The code lies in the
private submodules beside it, one per subsystem, each building on those before it: ``_abi``,
``_device``, ``_sweep``, ``_scan``, ``_locate``, ``_live``, ``_model``, ``_text``, ``_training_file``, ``_training``
("The binding as a package").  Code outside this package goes through this file.
"""

from ._abi import (COMBINE_MODES, ERR_COMM, EXPORTED_SYMBOLS, KIND_GENERAL, KIND_PERSISTENT,
                   MODEL_AUTO, MODEL_GENERAL, SIDE_END, SIDE_START, SIGNATURES, HipBackendError,
                   NadamCoefficients, TrainerOptions, check, library_path, load_library, ndpointer)
from ._device import (LDS_ARENA_WORDS, DeviceBuffer, Event, Stream, device_arrays, device_count,
                      device_name, fill_lds, get_device, is_pinned, set_device, survey_lds,
                      synchronize, use_pinned_loader_buffers)
from ._sweep import (EARLY_COLUMNS, SWEEP_MODES, sweep_counts, sweep_early_counts,
                     sweep_early_host, sweep_early_pushes, sweep_early_tally, sweep_pair,
                     sweep_steps, sweep_tally, sweep_windows)
from ._scan import (SCAN_EVENT, scan_events, scan_packed, scan_window_count, scan_window_offsets,
                    scan_windows)
from ._locate import (CELL_SAMPLES, LOCATION, OCCLUDE_PLAN, OCCLUSION, evidence_floats,
                      locate_occluded_packed, locate_occluded_workspace_bytes, locate_packed,
                      locate_rule, locate_rule_dev, locate_workspace_bytes, occlude_plan,
                      occlude_windows)
from ._live import (LIVE_ACTION, LIVE_ACTIONS, LIVE_BEGIN, LIVE_DECIDED, LIVE_EJECT, LIVE_END,
                    LIVE_END_RESULT, LIVE_FINAL, LIVE_IDLE, LIVE_KEEP, LIVE_NO_ACTION, LIVE_PENDING,
                    LIVE_REASONS, LIVE_RESULT, LIVE_STOP_ON_DECISION, LiveSession,
                    live_chunk_flags, live_fold, live_plan_host, live_policy_dev,
                    live_policy_plan_host, live_tail_plan_host)
from ._model import (INFLATE_SHUFFLE_REFUSED, INFLATE_STORED, INFLATE_STORED_SHUFFLE,
                     INFLATE_STREAM, INFLATE_SVB16, INFLATE_SVB16_ZSTD, INFLATE_VBZ, INFLATE_ZLIB,
                     INFLATE_ZLIB_SHUFFLE, HipModel,
                     ModelWeights, _TensorSpec, classify_pair, classify_pair_deflated,
                     combine_calls_dev, forward_executed_mfmas, forward_kernel_info, general_model,
                     inflate)
from ._text import (TEXT_COUNT, TEXT_FORM, TEXT_OK, TEXT_RANGE, DeviceSignals, ResidentText,
                    format_training_text, parse_training_text, parse_training_text_host,
                    random_signals, text_format_bound, text_stage_ms, write_training_data)
from ._training_file import (TEXT_BLOCK_BYTES, TrainingDataError, read_training_data,
                             strict_training_text, text_parse_route, training_text_blocks)
from ._training import (BATCH_STATS_FLOATS, MAX_FROZEN_BLOCKS, STEP_SEED_STRIDE, TRAINER_DEFAULTS,
                        Dataset, Trainer,
                        epoch_order, evaluate, gradients_dev, gradients_workspace_bytes,
                        library_trainer_defaults, loss_and_gradients, nadam_schedule,
                        nadam_update, step_seed, train_noise, trainer_options, write_npz)
