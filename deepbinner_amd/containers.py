"""
Multi-read fast5 containers as units of work, shared by ``deepbinner realtime`` (which bins their
reads) and ``deepbinner classify --multi_read`` (which tabulates them).  The reference unpacks a
container with an external tool first (realtime.py:183-190) and refuses it in ``classify``
(classify.py:113-116); here the reads are classified where they are, by one of three routes:

* **raw** - ``fast5_native.stream_raw``: the Signal chunks as stored go to the GPU, which inflates
  them (and undoes streamvbyte / zstd of VBZ chunks) beside the classification of the container
  before: ``hip_backend.classify_pair_deflated``.  A stream the device decoder refuses is read
  again by the host's loader, which has the last word.
* **packed** - ``fast5_native.stream_reads``: the loader's thread team inflates, the packed buffer
  of a container goes to the C ABI as it is.
* **lists** - the Python reader, or models without the packed entry point: ``--batch_size`` reads
  at a time through ``classify.classify_read_batch``.

``route`` picks one (the rule is ``realtime``'s: DEEPBINNER_GPU_INFLATE,
DEEPBINNER_HOST_INFLATE_SHARE, DEEPBINNER_LOADER_DEPTH, DEEPBINNER_VBZ_ZSTD, DEEPBINNER_SHUFFLE)
and hands back the stream of units and the function ``classify.dispatch_batches`` runs on each.
"""

import functools
import os

import numpy as np

from . import classify
from .load_fast5s import iter_reads, reader_kind
from .misc import usable_cpus


class Units:
    """What the container units need from their caller: the run's ``args`` and model geometry,
    the samples per read end the loaders keep (``keep``; None = whole signals), whether the whole
    signals are wanted back (``want_signals``: ``realtime``'s Python writer), whether the rows of
    ``classify``'s table are (``want_rows``), the loader threads asked for (0 = automatic), and
    what the lists route does at a read it cannot read: ``skip_damaged`` goes on behind it, as
    the native routes do (``classify --multi_read``); without it the container ends there
    (``realtime``, as ever)."""

    def __init__(self, args, start_size, end_size, n_classes, keep=None, want_signals=False,
                 want_rows=False, threads=0, skip_damaged=False):
        self.args = args
        self.start_size, self.end_size, self.n_classes = start_size, end_size, n_classes
        self.keep, self.want_signals, self.want_rows = keep, want_signals, want_rows
        self.threads = int(threads or 0)
        self.skip_damaged = bool(skip_damaged)


class Result:
    """One classified unit: container ``number`` (from 1, in the order of the file list) and
    ``path``, the ``ids`` and call ``names`` of its readable reads, ``signal(k)`` -> read k's
    whole signal (None unless wanted), ``where`` - which read of the container each one is (None
    on the lists route), the table ``lines`` (None unless wanted) and ``last``: whether this is
    the container's last unit."""
    __slots__ = ('number', 'path', 'ids', 'names', 'signal', 'where', 'lines', 'last')

    def __init__(self, number, path, ids, names, signal=None, where=None, lines=None, last=True):
        self.number, self.path, self.ids, self.names = number, path, ids, names
        self.signal, self.where, self.lines, self.last = signal, where, lines, last


def packed_containers(fast5s, units):
    """(container number, path, read ids, samples, offsets, where) per readable container, in
    order; unreadable reads are dropped (the reference skips what it cannot read,
    load_fast5s.py:47-49)."""
    from . import fast5_native
    stream = fast5_native.stream_reads(fast5s, keep=units.keep, threads=units.threads,
                                       depth=int(os.environ.get('DEEPBINNER_LOADER_DEPTH', 0)))
    for index, ids, samples, offsets, status in stream:
        if ids is None:
            continue
        classify.warn_about_filters(status)
        where = list(range(len(ids)))          # which read of the container each one is
        if any(rid is None for rid in ids):
            where = [i for i, rid in enumerate(ids) if rid is not None]
            parts = [samples[offsets[i]:offsets[i + 1]] for i in where]
            lengths = [len(part) for part in parts]
            samples = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int16)
            offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
            ids = [ids[i] for i in where]
        yield index + 1, fast5s[index], ids, samples, offsets, where


def classify_container(units, item, start_replica, end_replica):
    number, path, ids, samples, offsets, where = item
    lines = None
    if units.want_rows:
        signals = classify.PackedSignals([samples[offsets[i]:offsets[i + 1]]
                                          for i in range(len(ids))], samples, offsets)
        lines = classify.classify_read_batch(ids, signals, start_replica, units.start_size,
                                             end_replica, units.end_size, units.n_classes,
                                             units.args, {})
        names = [line.split('\t', 2)[1] for line in lines]
    else:
        numbers = classify.classify_packed_numbers(samples, offsets, start_replica, end_replica,
                                                   units.args)
        names = [classify.call_name(c) for c in numbers.tolist()]
    signal = (lambda i: samples[offsets[i]:offsets[i + 1]]) if units.want_signals else None
    return Result(number, path, ids, names, signal, where, lines)


# The same with (part of) the inflating on the GPU: the loader hands over Signal chunks as
# stored - zlib streams; 85 % of what loading a read costs a CPU core is inflating them, and a
# host has few cores per GPU - and dbh_classify_pair_deflated does the
# rest.  The host's threads keep the longest streams of every container (a lane of the GPU
# decoder walks ONE stream, however long): `host_inflate_share` of the bytes.
def raw_containers(fast5s, units, host_share, n_gpus=1):
    from . import fast5_native, realtime
    threads = units.threads
    if threads <= 0 and host_share == 0:
        # nothing to inflate: a read costs a loader thread ~5 us, and a GPU takes ~210 k a second -
        # two threads feed it, sixteen cost the process 19 us of CPU per read instead of 13
        # (woken sixteen times per container for a fifth of what they can deliver:
        # profiles/r06_loader/loader_team_size.txt)
        threads = min(usable_cpus(), realtime.RAW_LOADER_THREADS_PER_GPU * max(1, n_gpus))
    stream = fast5_native.stream_raw(fast5s, threads=threads, host_inflate_above=-host_share,
                                     depth=int(os.environ.get('DEEPBINNER_LOADER_DEPTH', 0)),
                                     vbz_zstd=fast5_native.vbz_zstd_route(),
                                     shuffle=fast5_native.shuffle_route())
    for index, ids, offsets, status, comp, records in stream:
        if ids is None:
            continue
        classify.warn_about_filters(status)
        yield index + 1, fast5s[index], ids, offsets, comp, records


def classify_raw_container(units, item, start_replica, end_replica):
    from . import fast5_native, hip_backend, realtime
    args = units.args
    number, path, ids, offsets, comp, records = item
    cus = realtime.inflate_cus_for(records['comp_bytes'].tolist(), records['mode'].tolist())
    if cus is not None:
        for model in (start_replica, end_replica):
            if model is not None:
                model.reserve_cus(cus)
    both = start_replica is not None and end_replica is not None
    verbose = units.want_rows and bool(getattr(args, 'verbose', False))
    result = hip_backend.classify_pair_deflated(
        start_replica, end_replica, comp, records, offsets, int(args.scan_size),
        args.score_diff, classify.combine_mode(args) if both else 'require_either',
        want_samples=units.want_signals, want_sides=verbose)
    numbers, stream_status = result[0], result[1]
    samples = result[2] if units.want_signals else None
    sides = result[-1] if verbose else None
    redone, redone_rows = {}, {}
    for i in sorted(set(records['read'][stream_status != 0].tolist())):
        # a stream the GPU decoder refused (damaged, or beyond it): zlib on the host has the
        # last word, as it has in the reference (h5py -> libhdf5 -> zlib)
        try:
            _, one, one_offsets, one_status = fast5_native.load_reads(path, first=i, count=1,
                                                                      threads=1)
        except OSError:
            one_status = [1]
        classify.warn_about_filters(np.asarray(one_status))
        if one_status[0] != 0:
            ids[i] = None
            continue
        if verbose:
            redone_rows[i] = classify.redone_verbose_row(ids[i], one[one_offsets[0]:one_offsets[1]],
                                                         start_replica, end_replica, args)
            numbers[i] = classify.call_number(redone_rows[i])
        else:
            numbers[i] = classify.classify_packed_numbers(one, one_offsets, start_replica,
                                                          end_replica, args)[0]
        redone[i] = np.array(one)
    keep = [i for i, rid in enumerate(ids) if rid is not None]
    names = [classify.call_name(int(numbers[i])) for i in keep]
    lines = None
    if units.want_rows:
        lines = classify.raw_table_rows(ids, numbers, sides, redone_rows, start_replica,
                                        end_replica, verbose)

    def signal(k):
        i = keep[k]
        return redone[i] if i in redone else samples[offsets[i]:offsets[i + 1]]

    return Result(number, path, [ids[i] for i in keep], names,
                  signal if samples is not None else None, keep, lines)


def read_chunks(fast5s, units):
    """The same units for the Python reader and for models without the packed entry point:
    (container number, path, read ids, signals, whether the container ends here) per
    --batch_size reads.  A read that cannot be read is dropped; the reads behind it are kept
    with ``units.skip_damaged`` only."""
    for number, path in enumerate(fast5s, start=1):
        try:
            reads = list(iter_reads(path, skip_damaged=units.skip_damaged))
        except OSError:
            continue
        chunks = list(classify.chunker(reads, units.args.batch_size))
        for k, chunk in enumerate(chunks):
            yield number, path, [r[0] for r in chunk], [r[1] for r in chunk], k + 1 == len(chunks)


def classify_chunk(units, item, start_replica, end_replica):
    number, path, ids, signals, last = item
    found = {}
    lines = classify.classify_read_batch(ids, signals, start_replica, units.start_size,
                                         end_replica, units.end_size, units.n_classes, units.args,
                                         found)
    if units.want_rows:         # (a read id seen twice in a chunk has two rows and two calls)
        names = [line.split('\t', 2)[1] for line in lines]
    else:
        names = [found[rid] for rid in ids]
    return Result(number, path, ids, names, signals.__getitem__, None,
                  lines if units.want_rows else None, last)


def route(fast5s, start_model, end_model, units):
    """-> (items, work, replicas, queues): the stream of units of the containers ``fast5s`` by
    the route this process takes, the function that classifies one of them on a (start, end)
    replica pair, the pairs ``classify.dispatch_batches`` deals them to, and the models whose
    ``reserve_cus(0)`` the caller owes when it is done (the raw route's inflate queues)."""
    from . import realtime
    models = [m for m in (start_model, end_model) if m is not None]
    packed = reader_kind() == 'native' and all(hasattr(m, 'classify_packed') for m in models)
    replicas = classify.device_replicas(start_model, end_model)
    n_gpus = len({getattr(r[0] or r[1], 'device', 0) for r in replicas})
    host_share = realtime.host_inflate_share(n_gpus)
    queues = []
    if packed and host_share < 100 and all(hasattr(m, 'handle') for m in models):
        items, work = raw_containers(fast5s, units, host_share, n_gpus), classify_raw_container
        replicas, queues = realtime.inflate_queues(replicas, host_share)
    elif packed:
        items, work = packed_containers(fast5s, units), classify_container
    else:
        items, work = read_chunks(fast5s, units), classify_chunk
    return items, functools.partial(work, units), replicas, queues
