"""
The units of work of the classify path, shared by ``deepbinner classify`` (which tabulates their
reads) and ``deepbinner realtime`` (which bins them).  A unit is a multi-read fast5 container - the
reference unpacks one with an external tool first (realtime.py:183-190) and refuses it in
``classify`` (classify.py:113-116); here its reads are classified where they are - or a POD5 file
(``Pod5Container``: the same, its signal rows read by ``pod5_lite``) - or a batch of
one-read files, which is a container whose reads happen to live in separate files: its ``origin``
(``Container`` / ``OneReadFiles``) says which file read i is and reads it again through the host's
loader, and nothing else tells the two apart.  A unit goes one of three routes:

* **raw** - ``fast5_native.stream_raw`` / ``load_batch_raw``: the Signal chunks as stored go to the
  GPU, which inflates them (and undoes streamvbyte / zstd of VBZ chunks, and HDF5's shuffle) beside
  the classification of the unit before: ``classify_raw`` -> ``hip_backend.classify_pair_deflated``.
  A stream the device decoder refuses is read again by the host's loader, which has the last word.
* **packed** - ``fast5_native.stream_reads`` / ``load_batch``: the loader's thread team inflates,
  the packed buffer of the unit goes to the C ABI as it is (``classify_packed``).
* **lists** - the Python reader, or containers for models without the packed entry point:
  ``--batch_size`` reads at a time through ``classify.classify_read_batch`` (``classify_lists``).

``route`` picks one (the rule is ``realtime``'s: DEEPBINNER_GPU_INFLATE,
DEEPBINNER_HOST_INFLATE_SHARE, DEEPBINNER_LOADER_DEPTH, DEEPBINNER_VBZ_ZSTD, DEEPBINNER_SHUFFLE;
for one-read files ``classify.raw_inflate_share`` adds its own conditions) and hands back, as a
context manager, the stream of classified units (``Result``) in the order they went in.
"""

import collections
import contextlib
import functools
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import classify
from .load_fast5s import iter_reads, reader_kind
from .misc import usable_cpus


class Units:
    """What the units need from their caller: the run's ``args`` and model geometry, the samples
    per read end the loaders keep (``keep``; None = whole signals), whether the whole signals are
    wanted back (``want_signals``: ``realtime``'s Python writer), whether the rows of
    ``classify``'s table are (``want_rows``), the loader threads asked for (0 = automatic), and
    what the lists route does at a read of a container it cannot read: ``skip_damaged`` goes on
    behind it, as the native routes do (``classify --multi_read``); without it the container ends
    there (``realtime``, as ever)."""

    def __init__(self, args, start_size, end_size, n_classes, keep=None, want_signals=False,
                 want_rows=False, threads=0, skip_damaged=False):
        self.args = args
        self.start_size, self.end_size, self.n_classes = start_size, end_size, n_classes
        self.keep, self.want_signals, self.want_rows = keep, want_signals, want_rows
        self.threads = int(threads or 0)
        self.skip_damaged = bool(skip_damaged)


class Container:
    """The origin of a unit whose reads are those of one multi-read container; its forward
    launches leave CUs to the inflate kernels by its streams (realtime.inflate_cus_for)."""
    files = None            # (every read's file is ``path``)
    reserves_cus = True

    def __init__(self, path):
        self.path = path

    def reread(self, i):
        """Read i again by the host's loader -> (ids, samples, offsets, status)."""
        from . import fast5_native
        try:
            return fast5_native.load_reads(self.path, first=i, count=1, threads=1)
        except OSError:
            return None, None, None, np.ones(1, dtype=np.int32)


class Pod5Container:
    """The origin of a unit whose reads are reads ``first`` onwards of one POD5 file (``pod5``: the
    open ``pod5_lite.Pod5``, shared by the file's units); dealt and given CUs like ``Container``."""
    files = None
    reserves_cus = True

    def __init__(self, path, pod5=None, first=0):
        self.path, self.pod5, self.first = path, pod5, int(first)

    def reread(self, i):
        """Read i of the unit decoded on the host (``pod5_lite.signal``), which has the last word
        -> (ids, samples, offsets, status)."""
        from . import fast5_native, pod5_lite
        if self.pod5 is None:
            self.pod5 = classify.opened_pod5(self.path)
        k = self.first + i
        try:
            signal = pod5_lite.signal(self.pod5, k)
        except OSError:                         # (no libzstd on this host)
            signal = None
        if signal is None:
            classify.warn_about_pod5_read(self.path, self.pod5.read_ids[k])
            return None, None, None, np.full(1, fast5_native.F5_ERR_FORMAT, dtype=np.int32)
        return ([self.pod5.read_ids[k]], signal, np.array([0, len(signal)], dtype=np.int64),
                np.zeros(1, dtype=np.int32))


class OneReadFiles:
    """The origin of a unit whose read i is the read of ``files[i]``; the host's loader reads it
    again with the ``keep`` samples per end of every other batch."""
    path = None
    reserves_cus = False

    def __init__(self, files, keep=None):
        self.files, self.keep = files, keep

    def reread(self, i):
        from . import fast5_native
        return fast5_native.load_batch([self.files[i]], self.keep, 1)


class Unit:
    """One unit on its way to its route's work function: its ``origin``, the read ``ids`` (None
    for a read nobody could read: raw route only), container ``number`` (from 1, in the order of
    the file list), how many files of the list are done with it (``n_files``), whether it is its
    container's ``last``, and what the route carries: ``offsets`` + ``comp`` + ``records`` (raw),
    ``samples`` + ``offsets`` + ``where`` (packed) or ``signals`` (lists)."""

    def __init__(self, origin, ids, number=0, n_files=1, last=True, **carried):
        self.origin, self.ids = origin, ids
        self.number, self.n_files, self.last = number, n_files, last
        self.__dict__.update(carried)


class Result:
    """One classified unit: container ``number`` and ``path`` (None for one-read files), the
    ``ids`` and call ``names`` of its readable reads, ``signal(k)`` -> read k's whole signal (None
    unless wanted), ``where`` - which read of the unit each one is (None on the lists route), the
    table ``lines`` (None unless wanted), ``last``: whether this is the container's last unit, and
    ``n_files``: how many files of the list are finished with it."""
    __slots__ = ('number', 'path', 'ids', 'names', 'signal', 'where', 'lines', 'last', 'n_files',
                 '_files')

    def __init__(self, unit, ids, names, signal=None, where=None, lines=None):
        self.number, self.path, self.last = unit.number, unit.origin.path, unit.last
        self.n_files, self._files = unit.n_files, unit.origin.files
        self.ids, self.names, self.signal, self.where, self.lines = ids, names, signal, where, lines

    def files(self):
        """{read id: the fast5 file it came from}"""
        if self._files is None:
            return dict.fromkeys(self.ids, self.path)
        if self.where is None:
            return dict(zip(self.ids, self._files))
        return {rid: self._files[i] for rid, i in zip(self.ids, self.where)}


# ---- the three work functions: (units, unit, start replica, end replica) -> Result ----------------
def classify_packed(units, unit, start_replica, end_replica):
    ids, samples, offsets = unit.ids, unit.samples, unit.offsets
    lines = None
    if units.want_rows:
        lines = classify.classify_read_batch(ids, None, start_replica, units.start_size,
                                             end_replica, units.end_size, units.n_classes,
                                             units.args, {}, packed=(samples, offsets))
        names = [line.split('\t', 2)[1] for line in lines]
    else:
        numbers = classify.classify_packed_numbers(samples, offsets, start_replica, end_replica,
                                                   units.args)
        names = [classify.call_name(c) for c in numbers.tolist()]
    signal = (lambda i: samples[offsets[i]:offsets[i + 1]]) if units.want_signals else None
    return Result(unit, ids, names, signal, unit.where, lines)


# The same with (part of) the inflating on the GPU: the loader hands over Signal chunks as
# stored - zlib streams; 85 % of what loading a read costs a CPU core is inflating them, and a
# host has few cores per GPU - and dbh_classify_pair_deflated does the
# rest.  The host's threads keep the longest streams of every unit (a lane of the GPU decoder
# walks ONE stream, however long): `host_inflate_share` of the bytes.
def classify_raw(units, unit, start_replica, end_replica):
    from . import hip_backend, realtime
    args = units.args
    ids, offsets, records = unit.ids, unit.offsets, unit.records
    cus = None
    if unit.origin.reserves_cus:
        cus = realtime.inflate_cus_for(records['comp_bytes'].tolist(), records['mode'].tolist())
    if cus is not None:
        for model in (start_replica, end_replica):
            if model is not None:
                model.reserve_cus(cus)
    both = start_replica is not None and end_replica is not None
    verbose = units.want_rows and bool(getattr(args, 'verbose', False))
    result = hip_backend.classify_pair_deflated(
        start_replica, end_replica, unit.comp, records, offsets, int(args.scan_size),
        args.score_diff, classify.combine_mode(args) if both else 'require_either',
        want_samples=units.want_signals, want_sides=verbose)
    numbers, stream_status = result[0], result[1]
    samples = result[2] if units.want_signals else None
    sides = result[-1] if verbose else None
    redone, redone_rows = {}, {}
    for i in sorted(set(records['read'][stream_status != 0].tolist())):
        # a stream the GPU decoder refused (damaged, or beyond it): zlib on the host has the
        # last word, as it has in the reference (h5py -> libhdf5 -> zlib)
        _, one, one_offsets, one_status = unit.origin.reread(i)
        classify.warn_about_filters(np.asarray(one_status))   # (damage only the GPU's VBZ
        if one_status[0] != 0:                                # self-checks could see)
            ids[i] = None
            continue
        if verbose:
            redone_rows[i] = classify.redone_verbose_row(ids[i], one[one_offsets[0]:one_offsets[1]],
                                                         start_replica, end_replica, args)
            numbers[i] = classify.call_number(redone_rows[i].split('\t', 2)[1])
        else:
            numbers[i] = classify.classify_packed_numbers(one, one_offsets, start_replica,
                                                          end_replica, args)[0]
        if samples is not None:
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

    return Result(unit, [ids[i] for i in keep], names, signal if samples is not None else None,
                  keep, lines)


def classify_lists(units, unit, start_replica, end_replica):
    ids, signals = unit.ids, unit.signals
    found = {}
    lines = classify.classify_read_batch(ids, signals, start_replica, units.start_size,
                                         end_replica, units.end_size, units.n_classes, units.args,
                                         found)
    if units.want_rows:         # (a read id seen twice in a unit has two rows and two calls)
        names = [line.split('\t', 2)[1] for line in lines]
    else:
        names = [found[rid] for rid in ids]
    return Result(unit, ids, names, signals.__getitem__, None, lines if units.want_rows else None)


# ---- the units of multi-read containers ---------------------------------------------------------
def loader_depth():
    return int(os.environ.get('DEEPBINNER_LOADER_DEPTH', 0))


def readable(ids, samples, offsets):
    """A loaded packed buffer without the reads that could not be read (the reference skips what
    it cannot read, load_fast5s.py:47-49) -> (ids, samples, offsets, which read each one was)."""
    where = list(range(len(ids)))
    if any(rid is None for rid in ids):
        where = [i for i, rid in enumerate(ids) if rid is not None]
        parts = [samples[offsets[i]:offsets[i + 1]] for i in where]
        lengths = [len(part) for part in parts]
        samples = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int16)
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        ids = [ids[i] for i in where]
    return ids, samples, offsets, where


def files_done(units):
    """Sets every unit's ``n_files`` by its container number: a container nobody could open
    yields no unit and is done with the next one that does."""
    done = 0
    for unit in units:
        upto = unit.number - (0 if unit.last else 1)
        unit.n_files, done = upto - done, upto
        yield unit


def packed_containers(fast5s, units):
    """One packed unit per readable container, in order."""
    from . import fast5_native
    stream = fast5_native.stream_reads(fast5s, keep=units.keep, threads=units.threads,
                                       depth=loader_depth())
    for index, ids, samples, offsets, status in stream:
        if ids is None:
            continue
        classify.warn_about_filters(status)
        ids, samples, offsets, where = readable(ids, samples, offsets)
        yield Unit(Container(fast5s[index]), ids, index + 1, samples=samples, offsets=offsets,
                   where=where)


def raw_containers(fast5s, units, host_share, n_gpus=1):
    """One raw unit per readable container, in order."""
    from . import fast5_native, realtime
    threads = units.threads
    if threads <= 0 and host_share == 0:
        # nothing to inflate: a read costs a loader thread ~5 us, and a GPU takes ~210 k a second -
        # two threads feed it, sixteen cost the process 19 us of CPU per read instead of 13
        # (woken sixteen times per container for a fifth of what they can deliver:
        # profiles/r06_loader/loader_team_size.txt)
        threads = min(usable_cpus(), realtime.RAW_LOADER_THREADS_PER_GPU * max(1, n_gpus))
    stream = fast5_native.stream_raw(fast5s, threads=threads, host_inflate_above=-host_share,
                                     depth=loader_depth(), vbz_zstd=fast5_native.vbz_zstd_route(),
                                     shuffle=fast5_native.shuffle_route())
    for index, ids, offsets, status, comp, records in stream:
        if ids is None:
            continue
        classify.warn_about_filters(status)
        yield Unit(Container(fast5s[index]), ids, index + 1, offsets=offsets, comp=comp,
                   records=records)


def read_chunks(fast5s, units):
    """The same for the Python reader and for models without the packed entry point: a lists
    unit per --batch_size reads.  A read that cannot be read is dropped; the reads behind it are
    kept with ``units.skip_damaged`` only."""
    for number, path in enumerate(fast5s, start=1):
        try:
            reads = list(iter_reads(path, skip_damaged=units.skip_damaged))
        except OSError:
            continue
        chunks = list(classify.chunker(reads, units.args.batch_size))
        for k, chunk in enumerate(chunks):
            yield Unit(Container(path), [r[0] for r in chunk], number, last=k + 1 == len(chunks),
                       signals=[r[1] for r in chunk])


# ---- the units of POD5 files --------------------------------------------------------------------
def pod5_host_only():
    """Whether POD5 files are decoded on the host (the lists route): only where the GPU inflate is
    switched off in so many words - DEEPBINNER_GPU_INFLATE=0, or DEEPBINNER_HOST_INFLATE_SHARE=100.
    A host with cores to spare (``realtime.host_inflate_share``'s rule for fast5, where the C++
    loader's thread team is then as fast as the GPU) changes nothing here: the alternative to the
    kernels is NumPy on one thread."""
    if os.environ.get('DEEPBINNER_GPU_INFLATE') == '0':
        return True
    if os.environ.get('DEEPBINNER_GPU_INFLATE') == '1':
        return False
    explicit = os.environ.get('DEEPBINNER_HOST_INFLATE_SHARE')
    return bool(explicit) and int(explicit) >= 100


def pod5_raw_units(pod5s, units):
    """Raw units of at most ``pod5_lite.READS_PER_UNIT`` reads per POD5 file, in order: one record
    per signal row, the rows' zstd frames undone here or left to the GPU (DEEPBINNER_VBZ_ZSTD);
    the next unit is put together on a background thread while the caller classifies this one."""
    from . import pod5_lite
    zstd = pod5_lite.zstd_route()
    opened = {}

    def chunks():
        for number, path in enumerate(pod5s, start=1):
            try:
                pod5 = opened[path] = classify.opened_pod5(path)
            except OSError:
                continue
            firsts = list(range(0, len(pod5), pod5_lite.READS_PER_UNIT))
            for first in firsts:
                yield number, path, first, first == firsts[-1]

    def load(chunk):
        _, path, first, _ = chunk
        return pod5_lite.raw_unit(opened[path], first, pod5_lite.READS_PER_UNIT, zstd=zstd,
                                  threads=units.threads)

    for (number, path, first, last), (ids, offsets, comp, records) in loaded_ahead(
            chunks(), load, 1, 1):
        pod5 = opened[path]
        for k, rid in enumerate(ids):
            if rid is None:
                classify.warn_about_pod5_read(path, pod5.read_ids[first + k])
        if all(rid is None for rid in ids):     # (nothing for the device: no unit, as for a
            continue                            #  container nobody could open)
        yield Unit(Pod5Container(path, pod5, first), ids, number, last=last, offsets=offsets,
                   comp=comp, records=records)


def pod5_chunks(pod5s, units):
    """The same files read on the host (``pod5_lite.signal``): a lists unit per --batch_size
    reads, handed on as soon as its reads are decoded (one unit's signals are held at a time); a
    read that is refused is dropped."""
    from . import pod5_lite
    size = max(1, int(units.args.batch_size))
    for number, path in enumerate(pod5s, start=1):
        try:
            pod5 = classify.opened_pod5(path)
        except OSError:
            continue
        ids, signals = [], []
        for i, read_id in enumerate(pod5.read_ids):
            try:
                signal = pod5_lite.signal(pod5, i)
            except OSError:                     # (no libzstd: said once by classify)
                signal = None
            if signal is None:
                classify.warn_about_pod5_read(path, read_id)
                continue
            ids.append(read_id)
            signals.append(signal)
            if len(ids) == size and i + 1 < len(pod5):
                yield Unit(Pod5Container(path, pod5), ids, number, last=False, signals=signals)
                ids, signals = [], []
        if ids:
            yield Unit(Pod5Container(path, pod5), ids, number, last=True, signals=signals)


# ---- the units of one-read files ------------------------------------------------------------------
def loader_threads(args):
    """The native loader's threads for a batch of one-read files: ``--loader_procs``, or one per
    hardware thread this process may keep busy (misc.usable_cpus), at most 32."""
    return int(getattr(args, 'loader_procs', 0) or 0) or max(1, min(32, usable_cpus()))


def containers_among(files, status, set_aside):
    """The multi-read files a batch of one-read files met -> how many: they end the run, unless
    the caller gave a list to ``set_aside`` such files in (--multi_read), whose units come after
    the batches'.  Then the batch goes on without them."""
    from . import fast5_native
    multi = (status == fast5_native.F5_ERR_MULTI)
    if not multi.any():
        return 0
    if set_aside is None:
        sys.exit('Error: Deepbinner does not (yet) support multi-read fast5 files')
    set_aside.extend(f for f, m in zip(files, multi.tolist()) if m)
    return int(multi.sum())


def loaded_ahead(chunks, load, workers, ahead):
    """``load(chunk)`` per chunk, in order, on ``workers`` background threads (the native loader
    releases the GIL): ``ahead`` + 1 chunks are loading or loaded while the caller works on the
    one before them."""
    with ThreadPoolExecutor(max_workers=workers, thread_name_prefix='deepbinner-loader') as pool:
        waiting = collections.deque()
        upcoming = iter(chunks)
        for chunk in upcoming:
            waiting.append((chunk, pool.submit(load, chunk)))
            if len(waiting) > ahead:
                break
        while waiting:
            chunk, pending = waiting.popleft()
            loaded = pending.result()
            following = next(upcoming, None)
            if following is not None:
                waiting.append((following, pool.submit(load, following)))
            yield chunk, loaded


def raw_batches(fast5s, units, host_share, n_queues, set_aside=None):
    """Raw unit after raw unit of max(--batch_size, RAW_BATCH_FILES) one-read files, loaded ahead
    of the GPU: two loads at a time on background threads (each on half of the loader's threads),
    as many waiting as there are queues."""
    from . import fast5_native
    threads = max(1, loader_threads(units.args) // 2)
    size = max(int(units.args.batch_size), classify.RAW_BATCH_FILES)

    def load(chunk):
        # DEEPBINNER_VBZ_ZSTD=gpu: VBZ chunks keep their zstd stage for the GPU (default: host);
        # DEEPBINNER_SHUFFLE=gpu: so do shuffled chunks their shuffle
        return fast5_native.load_batch_raw(chunk, threads, -host_share,
                                           vbz_zstd=fast5_native.vbz_zstd_route(),
                                           shuffle=fast5_native.shuffle_route())

    for chunk, (ids, offsets, status, comp, records) in loaded_ahead(
            list(classify.chunker(fast5s, size)), load, 2, n_queues):
        aside = containers_among(chunk, status, set_aside)
        classify.warn_about_filters(status)
        yield Unit(OneReadFiles(list(chunk), units.keep), ids, n_files=len(chunk) - aside,
                   offsets=offsets, comp=comp, records=records)


def packed_batches(fast5s, args, keep, set_aside=None):
    """Packed unit after packed unit of --batch_size one-read files: every batch is parsed and
    inflated by the native loader's own worker threads (``loader_threads``), the next one on a
    background thread while the caller classifies the current one."""
    from . import fast5_native
    threads = loader_threads(args)

    def load(chunk):
        return fast5_native.load_batch(chunk, keep, threads)

    for chunk, (ids, samples, offsets, status) in loaded_ahead(
            list(classify.chunker(fast5s, args.batch_size)), load, 1, 0):
        aside = containers_among(chunk, status, set_aside)
        classify.warn_about_filters(status)
        ids, samples, offsets, where = readable(ids, samples, offsets)
        yield Unit(OneReadFiles(chunk, keep), ids, n_files=len(chunk) - aside, samples=samples,
                   offsets=offsets, where=where)


def list_batch(loaded):
    """The lists unit of the (fast5_file, read_id, signal) triples the reference's loop builds
    (classify.py:141-150; signal None: a file that could not be read)."""
    read = [triple for triple in loaded if triple[2] is not None]
    return Unit(OneReadFiles([f for f, _, _ in read]), [rid for _, rid, _ in read],
                n_files=len(loaded), signals=[signal for _, _, signal in read])


# ---- the route choice -----------------------------------------------------------------------------
@contextlib.contextmanager
def route(fast5s, start_model, end_model, units, one_read=False, set_aside=None,
          host_loader=False, pod5=False):
    """The files ``fast5s`` - multi-read containers, or with ``one_read`` one-read files - by the
    route this process takes: the ``Result`` of every unit, in order (``classify.dispatch_batches``
    deals the units to the (start, end) replica pairs), for as long as the ``with`` lasts; behind
    it the raw route's inflate queues have given their CUs back (``reserve_cus(0)``).
    ``set_aside`` (one-read files): see ``containers_among``.  ``host_loader``: one-read files
    through ``classify.load_in_batches`` whatever ``classify.raw_inflate_share`` says.  ``pod5``:
    the files are POD5 files - the raw route (``pod5_raw_units``) on every host, whichever fast5
    reader this process has, unless the GPU inflate is switched off (``pod5_host_only``) or the
    models are stand-ins without a device handle: then the lists route."""
    from . import realtime
    models = [m for m in (start_model, end_model) if m is not None]
    packed = reader_kind() == 'native' and all(hasattr(m, 'classify_packed') for m in models)
    replicas = classify.device_replicas(start_model, end_model)
    n_gpus = len({getattr(r[0] or r[1], 'device', 0) for r in replicas})
    if one_read:
        host_share = None if host_loader else classify.raw_inflate_share(
            start_model, end_model, units.args, len(fast5s), replicas)
        raw = host_share is not None
    elif pod5:
        host_share = 100 if pod5_host_only() else 0     # (no share in between: every row is the GPU's)
        raw = host_share < 100 and all(hasattr(m, 'handle') for m in models)
    else:
        host_share = realtime.host_inflate_share(n_gpus)
        raw = packed and host_share < 100 and all(hasattr(m, 'handle') for m in models)
    queues = []
    if raw:
        # several units in flight per GPU, each on a replica of the models
        replicas, queues = realtime.inflate_queues(replicas, host_share)
        items, work = (raw_batches(fast5s, units, host_share, len(replicas), set_aside) if one_read
                       else pod5_raw_units(fast5s, units) if pod5
                       else raw_containers(fast5s, units, host_share, n_gpus)), classify_raw
    elif pod5:
        items, work = pod5_chunks(fast5s, units), classify_lists
    elif one_read:
        items = classify.load_in_batches(fast5s, units.args, units.keep, set_aside)
        work = classify_packed if reader_kind() == 'native' else classify_lists
    elif packed:
        items, work = packed_containers(fast5s, units), classify_packed
    else:
        items, work = read_chunks(fast5s, units), classify_lists
    if not one_read:
        items = files_done(items)
    try:
        yield classify.dispatch_batches(items, replicas, functools.partial(work, units))
    finally:
        for model in queues:                # the forward kernel gets every CU back
            model.reserve_cus(0)
