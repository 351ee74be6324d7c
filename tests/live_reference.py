"""A helper, not a test: the live sessions' contract (include/deepbinner_hip.h, "live") restated in
NumPy, as simply as it can be said - a channel's state machine as a plain class (reset on BEGIN,
append with the clip at cap, END; which windows are ready; what a folded window does to the
record), its front from tests/scan_reference.py (the window's bounds, the normalising over the
samples present) and its fold from tests/sweep_reference.py.  Also a host stand-in for the
``replay`` command's backend (``HostBackend``), which drives a model that only has ``predict`` - the
oracle of the conftest - through these rules."""
import numpy as np

import feed_reference
import scan_reference
import sweep_reference

RESULT = np.dtype([('status', np.int32), ('call', np.int32), ('final_call', np.int32),
                   ('windows', np.int32), ('decided_windows', np.int32), ('best', np.int32),
                   ('margin', np.float64), ('samples', np.int64), ('decided_samples', np.int64)])
IDLE, PENDING, DECIDED, FINAL = 0, 1, 2, 3
BEGIN, END = 1, 2


def seam_lengths(input_size, steps):
    """The read lengths at which the ready-window count, a window's padding or the clip changes."""
    L, h = input_size, input_size // 2
    cap = steps * h + h
    return [0, 1, h - 1, L - 1, L, L + 1, L + h - 1, L + h, cap - 1, cap, cap + 1, 2 * cap]


def ready_windows(n, ended, input_size, steps):
    """Window k < steps is ready when k h + L <= n, or when the read has ended."""
    if ended:
        return steps
    return min(steps, max(0, (n - input_size) // (input_size // 2) + 1))


def front(signal, input_size, steps, first=0, count=None):
    """float32 [count, L]: windows first .. first + count - 1 of the start side of ``signal``, each
    [min(k h, n), min(k h + L, n)) normalised over the samples present and padded behind; an empty
    window is zeros."""
    signal = np.asarray(signal, dtype=np.int16)
    count = steps - first if count is None else count
    out = np.zeros((count, input_size), dtype=np.float32)
    for j in range(count):
        a, b = scan_reference.window_bounds(len(signal), first + j, input_size, 'start')
        if b > a:
            out[j, :b - a] = feed_reference.normalise(signal[None, a:b])[0]
    return out


class Channel:
    """One channel.  ``predict``: float32 [W, L] -> [W, C] (None: ``track`` gives each window's
    outcome instead, as ``dbh_live_plan_host`` takes it)."""

    def __init__(self, input_size, scan_size, score_diff=0.5, min_windows=1, stop_on_decision=False,
                 predict=None, track=None):
        self.L, self.h = input_size, input_size // 2
        self.steps = scan_size // self.h
        self.cap = scan_size + self.h
        self.score_diff, self.min_windows, self.stop = score_diff, min_windows, stop_on_decision
        self.predict, self.given = predict, track
        self.open = self.ended = False
        self.reset()
        self.status = IDLE

    def reset(self):
        self.signal = np.zeros(0, np.int16)
        self.n = self.windows = self.call = self.decided_windows = self.decided_samples = 0
        self.final_call, self.best, self.margin = -1, 0, 0.0
        self.status = PENDING
        self.merged = None
        self.track_best, self.track_margin = [], []

    def stopped(self):
        return self.status == FINAL or (self.status == DECIDED and self.stop)

    def record(self, idle=False):
        return (IDLE if idle else self.status, self.call, self.final_call, self.windows,
                self.decided_windows, self.best, self.margin, self.n, self.decided_samples)

    def push(self, chunk, flags=0):
        """-> (the record behind the push, the windows it folded)"""
        chunk = np.asarray(chunk, dtype=np.int16)
        if flags & BEGIN:
            self.reset()
            self.open, self.ended = True, False
        elif not self.open:
            return self.record(idle=True), 0
        stop = self.stopped()
        if not stop:
            self.signal = np.concatenate([self.signal, chunk])[:self.cap]
        self.n += len(chunk)
        if flags & END:
            self.ended, self.open = True, False
        ready = self.windows if stop else ready_windows(self.n, self.ended, self.L, self.steps)
        done, first = 0, self.windows
        if ready > first and self.predict is not None:
            probs = np.asarray(self.predict(front(self.signal, self.L, self.steps, first,
                                                  ready - first)), dtype=np.float32)
        for k in range(first, ready):
            if self.stopped():
                break
            if self.predict is not None:
                p = probs[k - first]
                if self.merged is None:
                    self.merged = p.copy()
                else:
                    self.merged[0] = min(self.merged[0], p[0])
                    self.merged[1:] = np.maximum(self.merged[1:], p[1:])
                best, margin = sweep_reference.best_and_margin(
                    sweep_reference.renormalise(self.merged))
                best, margin = int(best), float(margin)
            else:
                best, margin = int(self.given[0][k]), float(self.given[1][k])
            self.folded(best, margin)
            done += 1
        return self.record(), done

    def folded(self, best, margin):
        k = self.windows
        self.windows = k + 1
        self.best, self.margin = best, margin
        self.track_best.append(best)
        self.track_margin.append(margin)
        leads = best != 0 and margin >= self.score_diff
        if self.decided_windows == 0 and k + 1 >= self.min_windows and leads:
            self.call, self.decided_windows, self.decided_samples = best, k + 1, self.n
            self.status = DECIDED
        if self.windows == self.steps:
            self.status = FINAL
            self.final_call = best if leads else 0


def plan(input_size, scan_size, lengths, flags, track_best, track_margin, **options):
    """``dbh_live_plan_host``: -> (RESULT [n], new windows int32 [n])"""
    channel = Channel(input_size, scan_size, track=(track_best, track_margin), **options)
    records, new = [], []
    for length, f in zip(lengths, flags):
        record, done = channel.push(np.zeros(int(length), np.int16), int(f))
        records.append(record)
        new.append(done)
    return np.array(records, dtype=RESULT), np.array(new, dtype=np.int32)


def chunked(signal, size):
    """A read cut into chunks of ``size`` samples (the last one shorter; an empty read: one empty
    chunk)."""
    signal = np.asarray(signal, dtype=np.int16)
    return [signal[a:a + size] for a in range(0, max(len(signal), 1), size)]


class HostSession:
    """``hip_backend.LiveSession`` on the host."""

    def __init__(self, model, n_channels, scan_size=6144, score_diff=0.5, min_windows=1,
                 stop_on_decision=False, max_round_windows=0):
        size = int(model.inputs[0].shape[1])
        self.channels = [Channel(size, scan_size, score_diff, min_windows, stop_on_decision,
                                 predict=lambda w: model.predict(w[:, :, None]))
                         for _ in range(n_channels)]

    def push(self, channels, chunks, begin=None, end=None):
        n = len(chunks)
        begin = np.broadcast_to(np.asarray(False if begin is None else begin, dtype=bool), (n,))
        end = np.broadcast_to(np.asarray(False if end is None else end, dtype=bool), (n,))
        return np.array([self.channels[ch].push(chunk, BEGIN * bool(b) + END * bool(e))[0]
                         for ch, chunk, b, e in zip(channels, chunks, begin, end)], dtype=RESULT)

    def track(self, channel):
        ch = self.channels[channel]
        return (np.array(ch.track_best, dtype=np.int32), np.array(ch.track_margin, dtype=np.float64))

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HostBackend:
    """What ``replay.replay`` asks of ``hip_backend`` - ``LiveSession`` and the status numbers - on
    the host, for models with ``predict`` and ``inputs`` (the conftest's OracleModel)."""
    LIVE_IDLE, LIVE_PENDING, LIVE_DECIDED, LIVE_FINAL = IDLE, PENDING, DECIDED, FINAL
    LiveSession = HostSession
