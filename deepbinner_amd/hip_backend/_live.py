"""Live sessions: each channel's barcode called while its signal arrives (include/deepbinner_hip.h,
"live").  ``LiveSession`` holds the channels' state on the device between pushes - with an ``end_model`` also
the tail of every open read, and gives the read's full call when it ends; with a ``policy`` also
what each barcode has yielded, and gives a keep / eject action with the push that decides.
``live_fold``, ``live_plan_host``, ``live_tail_plan_host``, ``live_policy_dev`` and
``live_policy_plan_host`` are the parity-only entries of its parts."""

import ctypes

import numpy as np

from .._cabi import Finalised, Owner, Scoped
from ._abi import COMBINE_MODES, check, load_library
from ._device import device_arrays, synchronize

# dbh_live_result (include/deepbinner_hip.h, "live"): a channel's record behind a push
LIVE_RESULT = np.dtype([('status', np.int32), ('call', np.int32), ('final_call', np.int32),
                        ('windows', np.int32), ('decided_windows', np.int32), ('best', np.int32),
                        ('margin', np.float64), ('samples', np.int64),
                        ('decided_samples', np.int64)])
assert LIVE_RESULT.itemsize == 48
# dbh_live_end_result: a channel's end side and combined call, known behind END (pair sessions)
LIVE_END_RESULT = np.dtype([('status', np.int32), ('end_call', np.int32), ('start_call', np.int32),
                            ('read_call', np.int32), ('end_best', np.int32),
                            ('end_windows', np.int32), ('end_margin', np.float64),
                            ('samples', np.int64)])
assert LIVE_END_RESULT.itemsize == 40
# dbh_live_action: what a yield policy says about a chunk's read ("Yield policies")
LIVE_ACTION = np.dtype([('action', np.int32), ('reason', np.int32), ('klass', np.int32),
                        ('reserved', np.int32), ('level', np.int64), ('floor', np.int64)])
assert LIVE_ACTION.itemsize == 32
LIVE_NO_ACTION, LIVE_KEEP, LIVE_EJECT = 0, 1, 2                      # action
LIVE_ACTIONS = {'keep': LIVE_KEEP, 'eject': LIVE_EJECT}
LIVE_REASONS = ('none', 'weight_keep', 'balanced', 'weight_eject', 'over_level', 'undecided')

LIVE_IDLE, LIVE_PENDING, LIVE_DECIDED, LIVE_FINAL = 0, 1, 2, 3       # status
LIVE_BEGIN, LIVE_END = 1, 2                                          # chunk flags
LIVE_STOP_ON_DECISION = 1                                            # session flag


def live_chunk_flags(n, begin=None, end=None):
    """``begin`` / ``end`` (None, one truth value or one per chunk) as the ABI's chunk flags."""
    flags = np.zeros(n, dtype=np.uint32)
    for bit, which in ((LIVE_BEGIN, begin), (LIVE_END, end)):
        if which is not None:
            flags |= np.where(np.broadcast_to(np.asarray(which, dtype=bool), (n,)), bit,
                              0).astype(np.uint32)
    return flags


class LiveSession(Owner, Scoped, Finalised):
    """``n_channels`` sequencer channels of one start-side ``model``: ``push`` appends a chunk of
    signal to each channel named, runs the windows that became complete and folds them; a channel
    is DECIDED at the first window from ``min_windows`` on whose best class is a barcode that leads
    by ``score_diff``, and FINAL when all ``scan_size`` windows are folded.  With an ``end_model`` (a
    pair session) the push that ends a read also runs the end model over the read's last
    ``scan_size`` samples and combines the two sides under ``combine`` ('either', 'start' or 'both':
    ``--require_*``): ``push_pair`` returns that beside the start records.  ``policy``:
    ``dict(weights=..., slack_samples=0, undecided='keep')`` - int32 weights per class (-1 always
    keep, 0 always eject, 1 .. 1 << 20 a share of the balance); ``push_policy`` then returns a
    LIVE_ACTION per chunk beside the records, and ``yields`` what each barcode has yielded.  Close it
    before its models."""

    _held, _release = 'handle', 'dbh_live_destroy'

    def __init__(self, model, n_channels, scan_size=6144, score_diff=0.5, min_windows=1,
                 stop_on_decision=False, max_round_windows=0, end_model=None, combine='either',
                 policy=None):
        self._lib = load_library()
        self.model, self.n_channels, self.scan_size = model, int(n_channels), int(scan_size)
        self.end_model = end_model
        half = model.input_size // 2
        self.steps = self.scan_size // half if half else 0
        flags = LIVE_STOP_ON_DECISION if stop_on_decision else 0
        handle = ctypes.c_void_p()
        if end_model is None:
            check(self._lib.dbh_live_create(model.handle, self.n_channels, self.scan_size,
                                            float(score_diff), int(min_windows), flags,
                                            int(max_round_windows), ctypes.byref(handle)),
                  'dbh_live_create')
        else:
            end_half = end_model.input_size // 2
            self.end_steps = self.scan_size // end_half if end_half else 0
            mode = COMBINE_MODES[combine if combine.startswith('require_') else 'require_' + combine]
            check(self._lib.dbh_live_create_pair(model.handle, end_model.handle, self.n_channels,
                                                 self.scan_size, float(score_diff),
                                                 int(min_windows), flags, mode,
                                                 int(max_round_windows), ctypes.byref(handle)),
                  'dbh_live_create_pair')
        self.handle = handle.value
        self.policy = None
        if policy is not None:
            try:
                self._set_policy(**policy)
            except BaseException:
                self.close()
                raise

    def _set_policy(self, weights, slack_samples=0, undecided='keep'):
        weights = np.ascontiguousarray(weights, dtype=np.int32)
        if undecided not in LIVE_ACTIONS:
            raise ValueError("undecided must be 'keep' or 'eject'")
        check(self._lib.dbh_live_set_policy(self.handle, weights.ctypes.data, len(weights),
                                            int(slack_samples), LIVE_ACTIONS[undecided]),
              'dbh_live_set_policy')
        self.policy = dict(weights=weights, slack_samples=int(slack_samples), undecided=undecided)

    def _packed(self, channels, offsets, samples, flags, want_end, want_actions=False):
        channels = np.ascontiguousarray(channels, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        samples = np.ascontiguousarray(samples, dtype=np.int16)
        flags = np.ascontiguousarray(flags, dtype=np.uint32)
        n = len(channels)
        if len(offsets) != n + 1 or len(flags) != n or (n and offsets[-1] > len(samples)):
            raise ValueError('one offset more than channels, one flag per channel')
        if samples.size == 0:
            samples = np.zeros(1, dtype=np.int16)           # (a pointer, whatever the chunks hold)
        results = np.zeros(n, dtype=LIVE_RESULT)
        if want_actions:
            ends = None
            if want_end:
                ends = np.zeros(n, dtype=LIVE_END_RESULT)
                ends['end_call'] = ends['start_call'] = ends['read_call'] = -1
            actions = np.zeros(max(n, 1), dtype=LIVE_ACTION)[:n]
            check(self._lib.dbh_live_push_policy(
                self.handle, channels.ctypes.data, offsets.ctypes.data, samples.ctypes.data,
                flags.ctypes.data, results.ctypes.data, None if ends is None else ends.ctypes.data,
                actions.ctypes.data, n), 'dbh_live_push_policy')
            return results, ends, actions
        if not want_end:
            check(self._lib.dbh_live_push(self.handle, channels.ctypes.data, offsets.ctypes.data,
                                          samples.ctypes.data, flags.ctypes.data,
                                          results.ctypes.data, n), 'dbh_live_push')
            return results
        ends = np.zeros(n, dtype=LIVE_END_RESULT)
        ends['end_call'] = ends['start_call'] = ends['read_call'] = -1
        check(self._lib.dbh_live_push_pair(self.handle, channels.ctypes.data, offsets.ctypes.data,
                                           samples.ctypes.data, flags.ctypes.data,
                                           results.ctypes.data, ends.ctypes.data, n),
              'dbh_live_push_pair')
        return results, ends

    def push_packed(self, channels, offsets, samples, flags):
        """``dbh_live_push`` as it is: int32 channels [n], int64 offsets [n + 1] into int16
        ``samples``, uint32 flags [n] -> LIVE_RESULT [n]."""
        return self._packed(channels, offsets, samples, flags, False)

    def push_pair_packed(self, channels, offsets, samples, flags):
        """``dbh_live_push_pair`` as it is -> (LIVE_RESULT [n], LIVE_END_RESULT [n])."""
        return self._packed(channels, offsets, samples, flags, True)

    def push_policy_packed(self, channels, offsets, samples, flags):
        """``dbh_live_push_policy`` as it is -> (LIVE_RESULT [n], LIVE_END_RESULT [n] or None on a
        start-only session, LIVE_ACTION [n])."""
        return self._packed(channels, offsets, samples, flags, self.end_model is not None, True)

    @staticmethod
    def _pack(chunks):
        chunks = [np.ascontiguousarray(chunk, dtype=np.int16).reshape(-1) for chunk in chunks]
        offsets = np.zeros(len(chunks) + 1, dtype=np.int64)
        np.cumsum([len(chunk) for chunk in chunks], out=offsets[1:])
        return offsets, np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.int16)

    def push(self, channels, chunks, begin=None, end=None):
        """One chunk of int16 signal per channel named (each channel at most once) -> LIVE_RESULT
        [n].  ``begin``: a new read starts with this chunk; ``end``: the read ends with it (one
        truth value, or one per chunk).  Chunks may be empty."""
        offsets, samples = self._pack(chunks)
        return self.push_packed(channels, offsets, samples,
                                live_chunk_flags(len(chunks), begin, end))

    def push_pair(self, channels, chunks, begin=None, end=None):
        """``push`` on a pair session -> (LIVE_RESULT [n], LIVE_END_RESULT [n]): behind END the end
        model's call, the start call that went into ``combine_calls`` and the read's call."""
        offsets, samples = self._pack(chunks)
        return self.push_pair_packed(channels, offsets, samples,
                                     live_chunk_flags(len(chunks), begin, end))

    def push_policy(self, channels, chunks, begin=None, end=None):
        """``push`` on a session with a policy -> (LIVE_RESULT [n], LIVE_END_RESULT [n] or None,
        LIVE_ACTION [n]): the action the policy takes on each chunk's read - with the push that
        decides it, standing from then on."""
        offsets, samples = self._pack(chunks)
        return self.push_policy_packed(channels, offsets, samples,
                                       live_chunk_flags(len(chunks), begin, end))

    def yields(self):
        """(samples int64 [C], reads int64 [C]): what the reads that ended with each call held."""
        n_classes = self.model.n_classes
        samples, reads = np.zeros(n_classes, np.int64), np.zeros(n_classes, np.int64)
        check(self._lib.dbh_live_yield(self.handle, samples.ctypes.data, reads.ctypes.data),
              'dbh_live_yield')
        return samples, reads

    def set_yields(self, samples, reads):
        """Seeds the yields: a run taken up again, or yield from before the session."""
        samples = np.ascontiguousarray(samples, dtype=np.int64)
        reads = np.ascontiguousarray(reads, dtype=np.int64)
        if len(samples) != self.model.n_classes or len(reads) != self.model.n_classes:
            raise ValueError('one yield per class')
        check(self._lib.dbh_live_set_yield(self.handle, samples.ctypes.data, reads.ctypes.data),
              'dbh_live_set_yield')

    def track(self, channel):
        """(best int32 [windows], margin float64 [windows]) of the channel's read so far: entry k
        is what a run at scan size (k + 1) * input_size / 2 would say."""
        best = np.zeros(max(self.steps, 1), dtype=np.int32)
        margin = np.zeros(max(self.steps, 1), dtype=np.float64)
        windows = ctypes.c_int32(0)
        check(self._lib.dbh_live_track(self.handle, int(channel), best.ctypes.data,
                                       margin.ctypes.data, ctypes.byref(windows)), 'dbh_live_track')
        return best[:windows.value].copy(), margin[:windows.value].copy()

    def end_track(self, channel):
        """(best int32 [windows], margin float64 [windows]) of the end side of the channel's read:
        ``end_steps`` entries behind END, window s = 0 the read's last samples; none before."""
        best = np.zeros(max(self.end_steps, 1), dtype=np.int32)
        margin = np.zeros(max(self.end_steps, 1), dtype=np.float64)
        windows = ctypes.c_int32(0)
        check(self._lib.dbh_live_end_track(self.handle, int(channel), best.ctypes.data,
                                           margin.ctypes.data, ctypes.byref(windows)),
              'dbh_live_end_track')
        return best[:windows.value].copy(), margin[:windows.value].copy()


def live_fold(model, window_probs, counts, steps, merged=None, state=None, score_diff=0.5,
              min_windows=1, stop_on_decision=False):
    """The resumable fold alone (``dbh_live_fold_dev``; parity tests): ``window_probs`` float32
    [sum of counts, C] holds, channel after channel, the ``counts[i]`` windows that come next for
    channel i; ``merged`` float32 [N, C] and ``state`` LIVE_RESULT [N] are what an earlier call gave
    back (None: nothing folded yet).  -> (merged, state, best int32 [N, steps], margin float64
    [N, steps]); of best and margin only the entries of the windows folded here are written."""
    counts = np.asarray(counts, dtype=np.int64)
    n, n_classes = len(counts), model.n_classes
    window_probs = np.ascontiguousarray(window_probs, dtype=np.float32).reshape(-1, n_classes)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if offsets[-1] != len(window_probs):
        raise ValueError('window_probs must hold the sum of counts windows')
    merged = np.zeros((n, n_classes), np.float32) if merged is None else \
        np.ascontiguousarray(merged, dtype=np.float32)
    if state is None:
        state = np.zeros(n, dtype=LIVE_RESULT)
        state['final_call'] = -1
        state['status'] = LIVE_PENDING
    state = np.ascontiguousarray(state, dtype=LIVE_RESULT)
    best = np.zeros((n, int(steps)), dtype=np.int32)
    margin = np.zeros((n, int(steps)), dtype=np.float64)
    probs = window_probs if len(window_probs) else np.zeros((1, n_classes), np.float32)
    with device_arrays(probs, offsets, merged, state, best, margin) as \
            (d_probs, d_offsets, d_merged, d_state, d_best, d_margin):
        check(load_library().dbh_live_fold_dev(
            model.handle, d_probs.ptr, d_offsets.ptr, n, len(window_probs), int(steps),
            float(score_diff), int(min_windows), LIVE_STOP_ON_DECISION if stop_on_decision else 0,
            d_merged.ptr, d_state.ptr, d_best.ptr, d_margin.ptr, None), 'dbh_live_fold_dev')
        synchronize()
        return (d_merged.download(merged.shape, np.float32), d_state.download((n,), LIVE_RESULT),
                d_best.download(best.shape, np.int32), d_margin.download(margin.shape, np.float64))


def live_plan_host(input_size, scan_size, lengths, flags, track_best, track_margin, score_diff=0.5,
                   min_windows=1, stop_on_decision=False):
    """One channel's planning and decision rules on the host (``dbh_live_plan_host``, the lines the
    kernels compile): pushes of ``lengths[i]`` samples with chunk ``flags[i]``, window k folding to
    (track_best[k], track_margin[k]) -> (LIVE_RESULT [n], the record behind each push; int32 [n],
    the windows each push made ready)."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    flags = np.ascontiguousarray(flags, dtype=np.uint32)
    half = int(input_size) // 2
    steps = max(int(scan_size) // half if half else 0, 1)
    track_best = np.ascontiguousarray(track_best, dtype=np.int32)
    track_margin = np.ascontiguousarray(track_margin, dtype=np.float64)
    if len(flags) != len(lengths) or len(track_best) < steps or len(track_margin) < steps:
        raise ValueError('one flag per length, a track of scan_size / (input_size / 2) windows')
    results = np.zeros(len(lengths), dtype=LIVE_RESULT)
    new_windows = np.zeros(len(lengths), dtype=np.int32)
    check(load_library().dbh_live_plan_host(
        int(input_size), int(scan_size), float(score_diff), int(min_windows),
        LIVE_STOP_ON_DECISION if stop_on_decision else 0, lengths.ctypes.data, flags.ctypes.data,
        len(lengths), track_best.ctypes.data, track_margin.ctypes.data, results.ctypes.data,
        new_windows.ctypes.data), 'dbh_live_plan_host')
    return results, new_windows


def live_tail_plan_host(end_input_size, scan_size, lengths, flags):
    """One channel's tail ring and end windows on the host (``dbh_live_tail_plan_host``, the lines
    the kernels compile): pushes of ``lengths[i]`` samples with chunk ``flags[i]`` -> (store int64
    [n, 4]: from, keep, ring index, samples before the wrap; samples int64 [n]: n behind each push;
    ends int32 [n]; windows int64 [n, steps_e, 4]: a, m, pad, ring index of a - filled where ends)."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    flags = np.ascontiguousarray(flags, dtype=np.uint32)
    if len(flags) != len(lengths):
        raise ValueError('one flag per length')
    half = int(end_input_size) // 2
    steps = max(int(scan_size) // half if half else 0, 1)
    n = len(lengths)
    store = np.zeros((n, 4), dtype=np.int64)
    samples = np.zeros(n, dtype=np.int64)
    ends = np.zeros(n, dtype=np.int32)
    windows = np.zeros((n, steps, 4), dtype=np.int64)
    check(load_library().dbh_live_tail_plan_host(
        int(end_input_size), int(scan_size), lengths.ctypes.data, flags.ctypes.data, n,
        store.ctypes.data, samples.ctypes.data, ends.ctypes.data, windows.ctypes.data),
        'dbh_live_tail_plan_host')
    return store, samples, ends, windows


def _policy_arguments(weights, undecided, yield_samples, yield_reads):
    weights = np.ascontiguousarray(weights, dtype=np.int32)
    n_classes = len(weights)
    if undecided not in LIVE_ACTIONS:
        raise ValueError("undecided must be 'keep' or 'eject'")
    zeros = np.zeros(n_classes, np.int64)
    yield_samples = np.array(zeros if yield_samples is None else yield_samples, dtype=np.int64)
    yield_reads = np.array(zeros if yield_reads is None else yield_reads, dtype=np.int64)
    if len(yield_samples) != n_classes or len(yield_reads) != n_classes:
        raise ValueError('one yield per class')
    return weights, n_classes, yield_samples, yield_reads


def live_policy_dev(records, flags, channels, weights, slack_samples=0, undecided='keep',
                    yield_samples=None, yield_reads=None, channel_action=None):
    """The two policy kernels alone (``dbh_live_policy_dev``; parity tests): LIVE_RESULT ``records``
    [n] as a push reports them, chunk ``flags`` [n], ``channels`` [n] (each at most once), the
    policy, the yields so far (None: zeros) and every channel's action so far (None: NONE for
    max(channels) + 1 channels).  -> (LIVE_ACTION [n], yield_samples, yield_reads, channel_action)"""
    records = np.ascontiguousarray(records, dtype=LIVE_RESULT)
    flags = np.ascontiguousarray(flags, dtype=np.uint32)
    channels = np.ascontiguousarray(channels, dtype=np.int32)
    n = len(records)
    weights, n_classes, yield_samples, yield_reads = _policy_arguments(weights, undecided,
                                                                       yield_samples, yield_reads)
    if channel_action is None:
        channel_action = np.zeros(int(channels.max()) + 1 if n else 1, np.int32)
    channel_action = np.array(channel_action, dtype=np.int32)
    if len(flags) != n or len(channels) != n:
        raise ValueError('one flag and one channel per record')
    if n and (channels.min() < 0 or channels.max() >= len(channel_action) or
              len(np.unique(channels)) != n):
        raise ValueError('each channel once, inside channel_action')
    actions = np.zeros(max(n, 1), dtype=LIVE_ACTION)
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)          # noqa: E731
    with device_arrays(pad(records), pad(flags), pad(channels), weights, yield_samples, yield_reads,
                       channel_action, actions) as (d_records, d_flags, d_channels, d_weights,
                                                    d_samples, d_reads, d_action, d_actions):
        check(load_library().dbh_live_policy_dev(
            d_records.ptr, d_flags.ptr, d_channels.ptr, n, d_weights.ptr, n_classes,
            int(slack_samples), LIVE_ACTIONS[undecided], d_samples.ptr, d_reads.ptr, d_action.ptr,
            d_actions.ptr, None), 'dbh_live_policy_dev')
        synchronize()
        return (d_actions.download(actions.shape, LIVE_ACTION)[:n],
                d_samples.download((n_classes,), np.int64), d_reads.download((n_classes,), np.int64),
                d_action.download(channel_action.shape, np.int32))


def live_policy_plan_host(pushes, weights, n_channels, slack_samples=0, undecided='keep',
                          yield_samples=None, yield_reads=None, channel_action=None):
    """The policy's rules on the host (``dbh_live_policy_plan_host``, the lines the kernels compile)
    over ``pushes``, each (channels [n], chunk flags [n], LIVE_RESULT records [n]).  -> (a list of
    LIVE_ACTION [n] per push, yield trace int64 [pushes, 2, C]: samples and reads behind each push,
    channel_action int32 [n_channels] behind the last)"""
    weights, n_classes, yield_samples, yield_reads = _policy_arguments(weights, undecided,
                                                                       yield_samples, yield_reads)
    channel_action = np.array(np.zeros(n_channels, np.int32) if channel_action is None
                              else channel_action, dtype=np.int32)
    if len(channel_action) != n_channels:
        raise ValueError('one action per channel')
    sizes = [len(p[0]) for p in pushes]
    for channels, flags, records in pushes:
        if len(flags) != len(channels) or len(records) != len(channels):
            raise ValueError('one flag and one record per channel of a push')
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offsets[-1])
    join = lambda k, dtype: np.ascontiguousarray(                    # noqa: E731
        np.concatenate([np.asarray(p[k], dtype=dtype) for p in pushes] +
                       [np.zeros(1, dtype)]), dtype=dtype)
    channels, flags, records = join(0, np.int32), join(1, np.uint32), join(2, LIVE_RESULT)
    actions = np.zeros(total + 1, dtype=LIVE_ACTION)
    trace = np.zeros((max(len(pushes), 1), 2, n_classes), dtype=np.int64)
    check(load_library().dbh_live_policy_plan_host(
        weights.ctypes.data, n_classes, int(slack_samples), LIVE_ACTIONS[undecided],
        offsets.ctypes.data, len(pushes), channels.ctypes.data, flags.ctypes.data,
        records.ctypes.data, int(n_channels), channel_action.ctypes.data,
        yield_samples.ctypes.data, yield_reads.ctypes.data, actions.ctypes.data,
        trace.ctypes.data), 'dbh_live_policy_plan_host')
    return ([actions[a:b].copy() for a, b in zip(offsets[:-1], offsets[1:])], trace[:len(pushes)],
            channel_action)
