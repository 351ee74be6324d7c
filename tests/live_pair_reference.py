"""A helper, not a test: the pair sessions' contract (include/deepbinner_hip.h, "live", "Pair
sessions") restated in NumPy, as simply as it can be said - the tail ring as an array indexed modulo
its size, the end windows with their front from tests/scan_reference.py (the window's bounds, the
normalising over the samples present, padded in front), the fold from tests/sweep_reference.py,
``combine_calls`` from the oracle, and the end record.  Also a host stand-in for the backend of
``replay --both_ends`` (``HostBackend``), which drives models that only have ``predict``."""
import numpy as np

import feed_reference
import live_reference as ref
import scan_reference
import sweep_reference
from oracle import classify_ref

END_RESULT = np.dtype([('status', np.int32), ('end_call', np.int32), ('start_call', np.int32),
                       ('read_call', np.int32), ('end_best', np.int32), ('end_windows', np.int32),
                       ('end_margin', np.float64), ('samples', np.int64)])
MODES = ('require_either', 'require_start', 'require_both')


def mode_name(combine):
    return combine if combine.startswith('require_') else 'require_' + combine


def combine(start, end, mode):
    """``combine_calls`` on call numbers (0 = 'none'), by the oracle's restatement on names."""
    name = lambda c: 'none' if c == 0 else str(int(c))             # noqa: E731
    out = classify_ref.combine_calls(name(start), name(end), mode_name(mode))
    return 0 if out == 'none' else int(out)


def read_lengths(input_size, steps):
    """The read lengths at which an end window's padding or the ring's wrap changes."""
    L, h = input_size, input_size // 2
    cap = steps * h + h
    return [0, 1, h - 1, h, L - 1, L, L + 1, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1, 3 * cap + 7]


# ---- the ring --------------------------------------------------------------------------------------
class Ring:
    """Sample p of a read (counted from BEGIN) lives at ring[p % cap]; a chunk stores its last
    min(length, cap) samples.  ``who[i]`` remembers which sample position wrote ring[i]."""

    def __init__(self, cap):
        self.cap = cap
        self.ring = np.zeros(cap, np.int16)
        self.who = np.full(cap, -1, np.int64)

    def store(self, n, chunk):
        chunk = np.asarray(chunk, dtype=np.int16)
        keep = min(len(chunk), self.cap)
        positions = np.arange(n + len(chunk) - keep, n + len(chunk))
        self.ring[positions % self.cap] = chunk[len(chunk) - keep:]
        self.who[positions % self.cap] = positions

    def read(self, a, m):
        positions = np.arange(a, a + m)
        assert (self.who[positions % self.cap] == positions).all()   # written by this read
        return self.ring[positions % self.cap]


def tail_plan(end_input_size, scan_size, lengths, flags):
    """``dbh_live_tail_plan_host``: -> (store int64 [n, 4], samples int64 [n], ends int32 [n],
    windows int64 [n, steps, 4])"""
    L, h = end_input_size, end_input_size // 2
    steps, cap = scan_size // h, scan_size + h
    n_chunks = len(lengths)
    store = np.zeros((n_chunks, 4), np.int64)
    samples = np.zeros(n_chunks, np.int64)
    ends = np.zeros(n_chunks, np.int32)
    windows = np.zeros((n_chunks, steps, 4), np.int64)
    is_open, n = False, 0
    for i, (length, f) in enumerate(zip(lengths, flags)):
        length = int(length)
        if f & ref.BEGIN:
            is_open, n = True, 0
        elif not is_open:
            samples[i] = n
            continue
        keep = min(length, cap)
        at = (n + length - keep) % cap
        store[i] = (length - keep, keep, at, min(keep, cap - at))
        n += length
        samples[i] = n
        if f & ref.END:
            is_open = False
            ends[i] = 1
            for s in range(steps):
                a, b = scan_reference.window_bounds(n, s, L, 'end')
                windows[i, s] = (a, b - a, L - (b - a), a % cap)
    return store, samples, ends, windows


# ---- the end windows -------------------------------------------------------------------------------
def end_front(tail, n, input_size, steps, read=None):
    """float32 [steps, L]: end windows 0 .. steps - 1 of a read of ``n`` samples whose last
    ``len(tail)`` samples are ``tail`` (at least min(n, cap) of them): [max(n - s h - L, 0),
    max(n - s h, 0)) normalised over the samples present and padded in front.  ``read(a, m)``
    (default: out of ``tail``) fetches samples [a, a + m) of the read."""
    if read is None:
        tail = np.asarray(tail, dtype=np.int16)
        read = lambda a, m: tail[len(tail) - (n - a):len(tail) - (n - a) + m]      # noqa: E731
    out = np.zeros((steps, input_size), dtype=np.float32)
    for s in range(steps):
        a, b = scan_reference.window_bounds(n, s, input_size, 'end')
        if b > a:
            out[s, input_size - (b - a):] = feed_reference.normalise(
                np.asarray(read(a, b - a), np.int16)[None])[0]
    return out


def end_call_of(best, margin, score_diff):
    return int(best) if best != 0 and margin >= score_diff else 0


# ---- a channel -------------------------------------------------------------------------------------
class PairChannel:
    """A start-side ``live_reference.Channel`` with the ring and, at END, the end side beside it.
    ``end_predict``: float32 [W, L_e] -> [W, C]."""

    def __init__(self, input_size, end_input_size, scan_size, score_diff=0.5, min_windows=1,
                 stop_on_decision=False, predict=None, end_predict=None, combine='either'):
        self.start = ref.Channel(input_size, scan_size, score_diff, min_windows, stop_on_decision,
                                 predict=predict)
        self.L, self.h = end_input_size, end_input_size // 2
        self.steps, self.cap = scan_size // self.h, scan_size + self.h
        self.score_diff, self.mode, self.end_predict = score_diff, mode_name(combine), end_predict
        self.ring = Ring(self.cap)
        self.track_best, self.track_margin = np.zeros(0, np.int32), np.zeros(0)
        self.end = (ref.IDLE, -1, -1, -1, 0, 0, 0.0, 0)

    def push(self, chunk, flags=0):
        """-> (the start record, the end record) behind the push"""
        chunk = np.asarray(chunk, dtype=np.int16)
        idle = not (flags & ref.BEGIN) and not self.start.open
        n_before = 0 if flags & ref.BEGIN else self.start.n
        record, _ = self.start.push(chunk, flags)
        if idle:
            return record, (ref.IDLE,) + tuple(self.end[1:])
        self.ring.store(n_before, chunk)               # whatever the start side's record says
        n = self.start.n
        self.end = (ref.PENDING, -1, -1, -1, 0, 0, 0.0, n)
        self.track_best, self.track_margin = np.zeros(0, np.int32), np.zeros(0)
        if flags & ref.END:
            x = end_front(None, n, self.L, self.steps, read=self.ring.read)
            probs = np.asarray(self.end_predict(x), dtype=np.float32)
            best, margin = sweep_reference.sweep(probs[None])
            self.track_best, self.track_margin = best[0].astype(np.int32), margin[0]
            end_call = end_call_of(best[0, -1], margin[0, -1], self.score_diff)
            start_call = self.start.final_call if self.start.status == ref.FINAL else self.start.call
            self.end = (ref.FINAL, end_call, start_call, combine(start_call, end_call, self.mode),
                        int(best[0, -1]), self.steps, float(margin[0, -1]), n)
        return record, self.end


def chunkings(read, input_size, steps, rng=None):
    """name -> the pieces of ``read`` under every chunking the contract names (END rides on the last
    piece; a trailing empty piece is END alone)."""
    read = np.asarray(read, dtype=np.int16)
    h = input_size // 2
    cap = steps * h + h
    empty = np.zeros(0, np.int16)
    out = {'whole': [read], 'end alone': [read, empty]}
    for size in (h - 1, h, h + 1, 1600):
        out[size] = ref.chunked(read, size)
    if len(read) <= cap + input_size and input_size <= 96:      # (one sample per push: short reads)
        out[1] = ref.chunked(read, 1)
    for first in (cap, cap + 1, 2 * cap + 3):                  # one chunk of exactly that, the rest
        if len(read) >= first:
            out['first %d' % first] = [read[:first], read[first:]]
    out['empty chunks'] = [empty, read[:len(read) // 2], empty, read[len(read) // 2:], empty]
    if rng is not None:
        cuts = np.sort(rng.integers(0, len(read) + 1, 4))
        cuts = np.concatenate([[0], cuts, [len(read)]])
        out['random'] = [read[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    return out


# ---- the session and the command's backend -----------------------------------------------------------
class HostPairSession:
    """``hip_backend.LiveSession`` with an end model, on the host."""

    def __init__(self, model, n_channels, scan_size=6144, score_diff=0.5, min_windows=1,
                 stop_on_decision=False, max_round_windows=0, end_model=None, combine='either'):
        if end_model is None:
            raise ValueError('a pair session needs an end model')
        size = int(model.inputs[0].shape[1])
        end_size = int(end_model.inputs[0].shape[1])
        self.end_steps = scan_size // (end_size // 2)
        self.channels = [PairChannel(size, end_size, scan_size, score_diff, min_windows,
                                     stop_on_decision,
                                     predict=lambda w: model.predict(w[:, :, None]),
                                     end_predict=lambda w: end_model.predict(w[:, :, None]),
                                     combine=combine)
                         for _ in range(n_channels)]

    def push_pair(self, channels, chunks, begin=None, end=None):
        n = len(chunks)
        begin = np.broadcast_to(np.asarray(False if begin is None else begin, dtype=bool), (n,))
        end = np.broadcast_to(np.asarray(False if end is None else end, dtype=bool), (n,))
        both = [self.channels[ch].push(chunk, ref.BEGIN * bool(b) + ref.END * bool(e))
                for ch, chunk, b, e in zip(channels, chunks, begin, end)]
        return (np.array([r for r, _ in both], dtype=ref.RESULT),
                np.array([e for _, e in both], dtype=END_RESULT))

    def push(self, channels, chunks, begin=None, end=None):
        return self.push_pair(channels, chunks, begin, end)[0]

    def track(self, channel):
        ch = self.channels[channel].start
        return (np.array(ch.track_best, dtype=np.int32), np.array(ch.track_margin, dtype=np.float64))

    def end_track(self, channel):
        ch = self.channels[channel]
        return ch.track_best.copy(), ch.track_margin.copy()

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HostBackend(ref.HostBackend):
    """What ``replay.replay`` asks of ``hip_backend`` with and without ``--both_ends``."""

    @staticmethod
    def LiveSession(model, n_channels, end_model=None, **options):
        if end_model is None:
            options.pop('combine', None)
            return ref.HostSession(model, n_channels, **options)
        return HostPairSession(model, n_channels, end_model=end_model, **options)
