"""A helper, not a test: the yield policy of a live session (include/deepbinner_hip.h, "Yield
policies") restated in NumPy and plain Python integers, as simply as it can be
said - per push the yields of the chunks that ended a read, then each balanced class's level and the
floor, then every chunk's action.  Also a host stand-in for the backend of ``replay`` with a policy
(``HostBackend``): the stand-in sessions of tests/live_reference.py and tests/live_pair_reference.py
with this restatement behind every push."""
import numpy as np

import live_pair_reference as pair
import live_reference as ref

ACTION = np.dtype([('action', np.int32), ('reason', np.int32), ('klass', np.int32),
                   ('reserved', np.int32), ('level', np.int64), ('floor', np.int64)])
NONE, KEEP, EJECT = 0, 1, 2
WEIGHT_KEEP, BALANCED, WEIGHT_EJECT, OVER_LEVEL, UNDECIDED = 1, 2, 3, 4, 5
MAX_WEIGHT = 1 << 20
ACTIONS = {'keep': KEEP, 'eject': EJECT}


def policy_ok(weights, slack_samples, undecided):
    weights = [int(w) for w in weights]
    return (len(weights) >= 1 and weights[0] == -1 and all(-1 <= w <= MAX_WEIGHT for w in weights)
            and slack_samples >= 0 and undecided in ACTIONS)


class Policy:
    """The policy's state - the two yields per class, the action per channel - and its one step."""

    def __init__(self, weights, n_channels, slack_samples=0, undecided='keep', yield_samples=None,
                 yield_reads=None):
        assert policy_ok(weights, slack_samples, undecided)
        self.weights = [int(w) for w in weights]
        self.slack, self.undecided = int(slack_samples), ACTIONS[undecided]
        n = len(self.weights)
        self.samples = [int(v) for v in (yield_samples if yield_samples is not None else [0] * n)]
        self.reads = [int(v) for v in (yield_reads if yield_reads is not None else [0] * n)]
        self.action = [NONE] * n_channels

    def yields(self):
        return np.array(self.samples, np.int64), np.array(self.reads, np.int64)

    def levels(self):
        return {c: self.samples[c] // w for c, w in enumerate(self.weights) if w >= 1}

    def push(self, channels, flags, records):
        """One push: ``records`` as the push reports them (status IDLE = an idle chunk).
        -> ACTION [n]"""
        idle = [int(r['status']) == ref.IDLE for r in records]
        for f, r, is_idle in zip(flags, records, idle):            # 1. every END of the push
            if int(f) & ref.END and not is_idle:
                self.samples[int(r['call'])] += int(r['samples'])
                self.reads[int(r['call'])] += 1
        levels = self.levels()                                      # 2. the levels and the floor
        floor = min(levels.values()) if levels else 0
        out = np.zeros(len(records), dtype=ACTION)
        for i, (ch, f, r) in enumerate(zip(channels, flags, records)):      # 3. the actions
            ch = int(ch)
            standing = NONE if int(f) & ref.BEGIN else self.action[ch]
            out[i]['action'] = standing
            if idle[i] or standing != NONE:
                continue
            if int(r['decided_windows']) > 0:
                c = int(r['call'])
                w = self.weights[c]
                level = levels.get(c, 0)
                if w == -1:
                    took = (KEEP, WEIGHT_KEEP)
                elif w == 0:
                    took = (EJECT, WEIGHT_EJECT)
                elif level > floor + self.slack:
                    took = (EJECT, OVER_LEVEL)
                else:
                    took = (KEEP, BALANCED)
                out[i] = (took[0], took[1], c, 0, level, floor)
            elif int(r['status']) == ref.FINAL:
                out[i] = (self.undecided, UNDECIDED, 0, 0, 0, floor)
            self.action[ch] = int(out[i]['action'])
        return out


def record(status=ref.PENDING, call=0, samples=0, decided=None):
    """A LIVE_RESULT as far as the policy reads it: ``decided`` defaults to call != 0."""
    decided = (call != 0) if decided is None else decided
    final = status == ref.FINAL
    return (status, call, (call if final else -1), 1 if decided or final else 0,
            1 if decided else 0, call, 0.75, samples, samples if decided else 0)


# ---- the session and the command's backend -----------------------------------------------------------
class HostPolicySession:
    """``hip_backend.LiveSession`` with a policy, on the host: a stand-in session of the two other
    reference files, its records untouched, and the restatement above behind every push."""

    def __init__(self, inner, n_channels, n_classes, weights, slack_samples=0, undecided='keep'):
        if len(weights) != n_classes or not policy_ok(weights, slack_samples, undecided):
            raise ValueError('dbh_live_set_policy failed: invalid argument')
        self.inner, self.is_pair = inner, hasattr(inner, 'push_pair')
        self.policy = Policy(weights, n_channels, slack_samples, undecided)
        if self.is_pair:
            self.end_steps = inner.end_steps

    def push_policy(self, channels, chunks, begin=None, end=None):
        n = len(chunks)
        flags = (np.where(np.broadcast_to(np.asarray(False if begin is None else begin, bool), (n,)),
                          ref.BEGIN, 0) |
                 np.where(np.broadcast_to(np.asarray(False if end is None else end, bool), (n,)),
                          ref.END, 0))
        if self.is_pair:
            results, ends = self.inner.push_pair(channels, chunks, begin, end)
        else:
            results, ends = self.inner.push(channels, chunks, begin, end), None
        return results, ends, self.policy.push(channels, flags, results)

    def push(self, channels, chunks, begin=None, end=None):
        return self.push_policy(channels, chunks, begin, end)[0]

    def push_pair(self, channels, chunks, begin=None, end=None):
        return self.push_policy(channels, chunks, begin, end)[:2]

    def yields(self):
        return self.policy.yields()

    def set_yields(self, samples, reads):
        if min(samples) < 0 or min(reads) < 0:
            raise ValueError('dbh_live_set_yield failed: invalid argument')
        self.policy.samples = [int(v) for v in samples]
        self.policy.reads = [int(v) for v in reads]

    def track(self, channel):
        return self.inner.track(channel)

    def end_track(self, channel):
        return self.inner.end_track(channel)

    def close(self):
        self.inner.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HostBackend(pair.HostBackend):
    """What ``replay.replay`` asks of ``hip_backend`` with and without a policy."""
    LIVE_NO_ACTION, LIVE_KEEP, LIVE_EJECT = NONE, KEEP, EJECT

    @staticmethod
    def LiveSession(model, n_channels, end_model=None, policy=None, **options):
        inner = pair.HostBackend.LiveSession(model, n_channels, end_model=end_model, **options)
        if policy is None:
            return inner
        n_classes = int(model.outputs[0].shape[1]) if hasattr(model, 'outputs') else \
            len(policy['weights'])
        return HostPolicySession(inner, n_channels, n_classes, **policy)
