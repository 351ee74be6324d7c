"""Log-space comparison of device probabilities with the fp64 oracle (a plain module, not a
conftest: tests import it).

The shipped models are confident: logits reach 50 to 72, and most classes of a real window sit
at 1e-10 .. 1e-30, where an absolute probability bound sees nothing.  So besides the 1e-4
absolute bound:

* where the oracle's p >= TINY, |log p_dev - log p_oracle| <= LOG_TOL x scale, with scale =
  max(1, max |oracle logit| of the window);
* where the oracle's p < TINY, p_dev < TINY_DEV.

Why 4e-5 x scale: ``test_stage_activations`` holds the logits to 2e-5 x scale, and a log-softmax
moves by at most twice the largest logit error (``log p_j = z_j - logsumexp(z)``; both terms are
1-Lipschitz in the max norm).  Per-read results (make_sum_to_one of a min / max over the scan
steps) take the largest scale of the read's windows, and one more term for the barcodes:

* make_sum_to_one scales barcode j by (1 - p0) / (sum of the barcodes), p0 being the merged class 0
  of float32 per-window probabilities (the reference casts model.predict's output to float32
  before the merge; classify.py:361-393).  Next to one, float32 resolves p0 only to 2^-24: a
  softmax in float32 sums its C exponentials (the largest is 1) with up to C - 1 roundings of at
  most 2^-24 each and divides with one more of 2^-25, and the oracle's cast adds another 2^-25,
  so the two p0 may lie C x 2^-24 apart - far inside the 1e-4 absolute bound - and log(1 - p0)
  moves by up to C x 2^-24 / (1 - p0), the same for every barcode of the read.  That term is
  added to the bound of classes 1.. of a per-read row; where it passes 0.5 (float32 does not
  resolve the factor) the barcodes of that row keep the absolute rules only.  On real reads it
  matters for confident 'none' reads alone (an empty read: p0 = 1 - 2^-24 in the oracle, 1.0 in
  float32 arithmetic, every barcode 0).
"""
import numpy as np

PROB_TOL = 1e-4
LOG_TOL = 4e-5
TINY = 1e-30
TINY_DEV = 1e-25


def log_softmax(logits):
    z = np.asarray(logits, dtype=np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=-1, keepdims=True))


def logit_scale(logits):
    """max(1, max |logit|) of each window."""
    return np.maximum(1.0, np.abs(np.asarray(logits, dtype=np.float64)).max(axis=-1))


def read_scale(logits, n_reads):
    """The scale of each read, from the oracle logits of its windows in the order of
    ``classify_ref.make_windows`` (step-major: [steps, n_reads, C] flattened)."""
    logits = np.asarray(logits, dtype=np.float64)
    return logit_scale(logits.reshape(-1, n_reads, logits.shape[-1])).max(axis=0)


def _ratios(p_dev, logits, probs, scale):
    """Error / bound of every element under the rule that applies to it, and the oracle's p."""
    p_dev = np.asarray(p_dev, dtype=np.float64)
    if logits is not None:
        log_ref, scale = log_softmax(logits), logit_scale(logits)
    else:
        with np.errstate(divide='ignore'):
            log_ref = np.log(np.asarray(probs, dtype=np.float64))
        scale = np.maximum(1.0, np.asarray(scale, dtype=np.float64))
    assert p_dev.shape == log_ref.shape, (p_dev.shape, log_ref.shape)
    p_ref = np.exp(log_ref)
    bound = np.repeat(LOG_TOL * scale[:, None], p_dev.shape[1], axis=1)
    log_rule = p_ref >= TINY
    if logits is None:
        # per-read results: the float32 resolution of 1 - p0 (module docstring)
        res = p_dev.shape[1] * 2.0 ** -24 / np.maximum(1.0 - p_ref[:, :1], 1e-300)
        bound[:, 1:] += res
        log_rule[:, 1:] &= res <= 0.5
    with np.errstate(divide='ignore', invalid='ignore'):
        log_err = np.abs(np.log(p_dev) - log_ref) / bound
    log_err = np.where(np.isnan(log_err), np.inf, log_err)
    ratio = np.where(log_rule, log_err, np.where(p_ref >= TINY, 0.0, p_dev / TINY_DEV))
    ratio = np.maximum(ratio, np.abs(p_dev - p_ref) / PROB_TOL)
    ratio[~np.isfinite(p_dev)] = np.inf
    return ratio, p_ref


def log_space_ratio(p_dev, logits=None, probs=None, scale=None):
    """The worst error / bound (<= 1 passes).  Give the oracle's ``logits`` [N, C] for
    per-window results, or its merged ``probs`` [N, C] and a ``scale`` [N] for per-read ones."""
    ratio, _ = _ratios(p_dev, logits, probs, scale)
    return float(ratio.max()) if ratio.size else 0.0


def assert_log_close(p_dev, logits=None, probs=None, scale=None, what=''):
    """Assert the rules of the module docstring; print and return the worst error / bound, so
    that a run records its margin."""
    p_dev = np.asarray(p_dev, dtype=np.float64)
    assert np.isfinite(p_dev).all(), '{}: non-finite probabilities'.format(what)
    ratio, p_ref = _ratios(p_dev, logits, probs, scale)
    worst = float(ratio.max()) if ratio.size else 0.0
    print('log-space {}: {} rows, worst error / bound = {:.3f}'.format(what, len(p_dev), worst))
    if worst > 1.0:
        i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError('{}: error / bound {:.3g} at row {} class {} (p_oracle {:.6e}, '
                             'p_dev {:.6e})'.format(what, worst, i, j, p_ref[i, j], p_dev[i, j]))
    return worst


def oracle_logits(weights, windows):
    """fp64 oracle probabilities and logits of fp32 windows [N, L]."""
    from oracle import network_ref
    probs, stages = network_ref.forward(weights, np.asarray(windows, dtype=np.float32),
                                        dtype=np.float64, return_stages=True)
    return probs, stages['logits']


def oracle_call_batch(weights, signals, scan_size, score_diff, side):
    """classify_ref.call_batch around the fp64 oracle -> (calls, merged probs, scale of each
    read: the largest of its windows')."""
    from oracle import classify_ref
    logits = []

    def predict(w):
        probs, lg = oracle_logits(weights, w)
        logits.append(lg)
        return probs
    calls, probs = classify_ref.call_batch(predict, signals, weights.input_size, scan_size,
                                           score_diff, side)
    scale = read_scale(np.stack(logits), len(signals)) if len(signals) else np.zeros(0)
    return calls, probs, scale
